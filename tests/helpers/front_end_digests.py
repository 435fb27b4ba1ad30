"""Writes tests/golden/front_end_digests.json (or the path given): the sha256 digests that property P6 of
tests/test_gpu_minibatch_front_end.py compares against, computed by that module's lab_digests() from the library in use
(RLCONTROL_HIP_LIB selects another build).  The committed file was written from the build of the commit before the
thirteen copies of the minibatch front end became call sites of one body in rlc_common.h, before any kernel was edited:
run this only to record a deliberate change of results."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import front_end_cases as T
    import test_gpu_minibatch_front_end as t
    from rlcontrol_amd import build
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "front_end_digests.json")
    digests = {}
    for fe in T.cases():
        lab = t.Lab(fe)
        digests.update(t.lab_digests(lab))
        lab.runs.clear()
    doc = {"what": "sha256 over the sorted keys (name, dtype, shape, raw bytes) of each agent's state after P1's run: "
                   "rotated ring, device sampler, %d updates, %d agents" % (T.K, T.NA),
           "recorded_from": "the build of the parent commit of the front-end merge (before any kernel was edited)",
           "hipcc": subprocess.check_output([build._hipcc(), "--version"], text=True).strip(),
           "digests": digests}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(digests), out))


if __name__ == "__main__":
    main()
