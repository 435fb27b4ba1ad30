"""Writes tests/golden/ddpg_packed_pair_digests.json (or the path given): the sha256 digests that
tests/test_gpu_ddpg_packed_pair.py compares against, computed by that module's state_digests() from the library in use
(RLCONTROL_HIP_LIB selects another build).  The committed file was written from the build of the commit before the
packed ragged tile and the phase merges of the DDPG MFMA kernel: run this only to record a deliberate change of results."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import test_gpu_ddpg_packed_pair as t
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ddpg_packed_pair_digests.json")
    doc = {"what": "sha256 of float32 bytes after five device-sampled updates (3 + 2), one agent, seed 4242",
           "recorded_from": "the build of the parent commit of the packed ragged tile (before the kernel was changed)",
           "digests": {t.digest_key(*c): t.state_digests(*c) for c in t.DIGEST_CASES}}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc["digests"], sort_keys=True))


if __name__ == "__main__":
    main()
