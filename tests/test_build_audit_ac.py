"""The build audit's record of the ActorCritic unit (rlcontrol_amd/kernel_resource_usage.json, written by
__graft_entry__.build()): ac_generic.o is present with its three kernels, free of whole-wave spills and exec-0 restore
copies (rlcontrol_amd/build.py::audit_object), and held to the build's spill policy."""
import json
import os


def _usage():
    from rlcontrol_amd import build as B
    if not os.path.exists(B.USAGE_JSON):
        import __graft_entry__ as g
        g.build()
    with open(B.USAGE_JSON) as f:
        return json.load(f)


def test_ac_unit_is_audited_and_clean():
    usage = _usage()
    assert "ac_generic.o" in usage, sorted(usage)
    kernels = usage["ac_generic.o"]
    for want in ("rlc_ac_update_kernel", "rlc_ac_act_kernel", "rlc_ac_qval_kernel"):
        assert sum(want in name for name in kernels) == 1, (want, sorted(kernels))
    for name, k in kernels.items():
        print("%s: %d VGPRs, %d VGPR spills, %d SGPR spills, %d B of scratch" % (
            name, k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"], k["private_segment_fixed_size"]))
        assert k["exec0_copies"] == 0 and k["wwm_spills"] == 0, (name, k)


def test_ac_unit_is_under_the_spill_policy():
    from rlcontrol_amd import build as B
    assert "ac_generic.o" in B.GUARDED_UNITS
    assert "ac_generic.hip" in B.PLAIN and "rlc_api_ac.hip" in B.PLAIN
