"""Which macros may alter kernel code.

Only these RLC_ names may stand in an #if / #ifdef / #ifndef / #elif of rlcontrol_amd/csrc:
  * the instantiation parameters of the *_inst.hip and dispatcher files: RLC_MT, RLC_AD, RLC_NTW, RLC_T4, RLC_WIDE,
    RLC_ONLY_7_1;
  * the two instruments that have scripts driving them: RLC_STAMPS (RLC_STAMPS=1 builds) and RLC_ABLATE
    (scripts/ab_ablate.py);
  * the two settings that ship with different values in different units: RLC_WG_EXACT and RLC_WG_LATE_ISSUE (on for
    SoftActorCritic only).
An experiment that did not pay is recorded in DESIGN.md 8.0 with its measurement and taken out of the tree again, not
left behind as a default-off switch: every shipped kernel is built from the code such a switch is threaded through.
"""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rlcontrol_amd", "csrc")
ALLOWED = {"RLC_MT", "RLC_AD", "RLC_NTW", "RLC_T4", "RLC_WIDE", "RLC_ONLY_7_1",
           "RLC_STAMPS", "RLC_ABLATE",
           "RLC_WG_EXACT", "RLC_WG_LATE_ISSUE"}


def test_only_the_listed_macros_switch_kernel_code():
    files = sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")))
    assert files
    found = {}
    for path in files:
        with open(path) as f:
            for no, line in enumerate(f, 1):
                if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                    for name in re.findall(r"\bRLC_\w+", line.split("//")[0]):
                        found.setdefault(name, []).append("%s:%d" % (os.path.basename(path), no))
    assert found, "the scan found no conditional at all: it is looking in the wrong place"
    extra = {n: w for n, w in found.items() if n not in ALLOWED}
    assert not extra, "compile switches outside the rule (DESIGN.md 8.0): %r" % extra
