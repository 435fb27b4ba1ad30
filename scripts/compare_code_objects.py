#!/usr/bin/env python3
"""Developer loop (CPU box): are the gfx950 code objects of two builds of this library (a parent commit's and a
refactored tree's) byte-identical?
    python scripts/compare_code_objects.py LABEL PARENT_OBJDIR CHILD_OBJDIR [OUT.json]
Every *.o of the two object directories (csrc/_obj of a full build, csrc/_obj_stamps_fast of the stamps build, ab/obj of
scripts/ab_ablate.py) is unbundled with rlcontrol_amd/build.py's extract_code_object and its device code hashed; host
code is not compared (RLC_HIP embeds __LINE__).  The result -- per unit both sha256 and an `equal` flag, with the
`hipcc --version` string -- is stored under LABEL in OUT.json (default profiles/switch_retirement_code_objects.json: the
record that retiring the lost-experiment switches left every shipped and diagnostic kernel as it was);
other labels in the file are kept.  A unit whose code objects differ also gets `sections_differ`: the names of the ELF
sections whose bytes differ (.text = the instructions, .rodata = the kernel descriptors, .note = the kernels' metadata;
.strtab / .dynstr / .hash / .gnu.hash only hold symbol names -- a lambda left out of line carries the name of the
function it is written in).  Exit status 1 if any unit differs or exists on one side only.
Both trees must be built with the same command lines, i.e. at the same absolute path (one after the other, or the
second in a bind mount): HIP names a symbol per unit after a hash of the command line as written (__hip_cuid_...)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rlcontrol_amd import build as B  # noqa: E402


def device_sha256(obj):
    """sha256 of the unit's gfx950 code object; "host-only" for a unit without device code, None for a missing unit"""
    if not os.path.exists(obj):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "x.co")
        if not B.extract_code_object(obj, co):
            return "host-only"
        with open(co, "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()


def sections(obj):
    """{section name: sha256 of its bytes} of the unit's gfx950 code object"""
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "x.co")
        B.extract_code_object(obj, co)
        table = subprocess.check_output([os.path.join(B._LLVM, "llvm-readelf"), "-S", "-W", co], text=True)
        names = [w[1] for w in (l.replace("[ ", "[").split() for l in table.splitlines())
                 if len(w) > 1 and w[0].startswith("[") and w[1].startswith(".")]
        out = {}
        for n in names:
            raw = os.path.join(tmp, "sec.bin")
            if subprocess.call([os.path.join(B._LLVM, "llvm-objcopy"), "--dump-section", n + "=" + raw, co,
                                os.path.join(tmp, "y.co")], stderr=subprocess.DEVNULL) == 0:
                with open(raw, "rb") as f:
                    out[n] = hashlib.sha256(f.read()).hexdigest()
        return out


def main(label, dir_a, dir_b, out=os.path.join(ROOT, "profiles", "switch_retirement_code_objects.json")):
    names = sorted({f for d in (dir_a, dir_b) for f in os.listdir(d) if f.endswith(".o")})
    with ThreadPoolExecutor(max_workers=8) as ex:
        ha = list(ex.map(lambda n: device_sha256(os.path.join(dir_a, n)), names))
        hb = list(ex.map(lambda n: device_sha256(os.path.join(dir_b, n)), names))
    units = {n: {"parent": a, "child": b, "equal": a is not None and a == b} for n, a, b in zip(names, ha, hb)}
    for n, u in units.items():
        if not u["equal"] and u["parent"] and u["child"] and "host-only" not in (u["parent"], u["child"]):
            sa, sb = sections(os.path.join(dir_a, n)), sections(os.path.join(dir_b, n))
            u["sections_differ"] = sorted(k for k in set(sa) | set(sb) if sa.get(k) != sb.get(k))
    try:
        with open(out) as f:
            doc = json.load(f)
    except OSError:
        doc = {}
    doc["hipcc_version"] = subprocess.check_output([B._hipcc(), "--version"], text=True).strip()
    doc.setdefault("builds", {})[label] = {"units": units, "all_equal": all(u["equal"] for u in units.values())}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    bad = [n for n, u in units.items() if not u["equal"]]
    print("%s: %d units, %d differ%s" % (label, len(units), len(bad), "".join(
        "\n  %s: sections %s" % (n, " ".join(units[n].get("sections_differ", ["?"]))) for n in bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) not in (4, 5):
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
