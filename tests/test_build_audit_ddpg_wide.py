"""The build audit's record of the wide instantiations of the MFMA DDPG kernel (state_dim <= 32, action_dim in
{1,2,3,4,6}; rlcontrol_amd/kernel_resource_usage.json, written by __graft_entry__.build()): every (MT, AD) unit present
once, free of whole-wave spills and exec-0 restore copies (rlcontrol_amd/build.py::audit_object), and held to the build's
spill policy; the narrow units are still there."""
import json
import os
import re

import pytest

WIDE = [(mt, ad) for ad in (1, 2, 3, 4, 6) for mt in (2, 4, 7, 8)]
NARROW = ["ddpg_mfma_%d_%d.o" % (mt, ad) for ad in (1, 2) for mt in (2, 4, 7, 8)] + ["ddpg_mfma_7_1_t4.o", "ddpg_mfma_7_2_t4.o"]


def _usage():
    from rlcontrol_amd import build as B
    if not os.path.exists(B.USAGE_JSON):
        import __graft_entry__ as g
        g.build()
    with open(B.USAGE_JSON) as f:
        return json.load(f)


@pytest.mark.parametrize("mt,ad", WIDE)
def test_wide_ddpg_instantiations_are_audited_and_clean(mt, ad):
    usage = _usage()
    unit = "ddpg_mfma_w_%d_%d.o" % (mt, ad)
    assert unit in usage, (unit, sorted(u for u in usage if u.startswith("ddpg_mfma")))
    # <MT, AD, FUSE, T4 = false, WIDE = true> in the Itanium mangling of the kernel's template arguments: the fused and
    # the two-pass form of the forward, once each
    for fuse in (0, 1):
        tag = "rlc_ddpg_update_mfma_kernelILi%dELi%dELb%dELb0ELb1EE" % (mt, ad, fuse)
        found = [(n, k) for n, k in usage[unit].items() if tag in n]
        assert len(found) == 1, (tag, sorted(usage[unit]))
        name, k = found[0]
        print("wide <MT %d, AD %d, FUSE %d>: %d VGPRs, %d VGPR spills, %d SGPR spills, %d B of scratch" % (
            mt, ad, fuse, k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"], k["private_segment_fixed_size"]))
        assert k["exec0_copies"] == 0 and k["wwm_spills"] == 0, (name, k)


def test_wide_units_are_under_the_spill_policy():
    from rlcontrol_amd import build as B
    for mt, ad in WIDE:
        assert "ddpg_mfma_w_%d_%d.o" % (mt, ad) in B.GUARDED_UNITS


def test_narrow_ddpg_mfma_units_are_still_there():
    usage = _usage()
    for unit in NARROW:
        assert unit in usage and any("rlc_ddpg_update_mfma_kernel" in n for n in usage[unit]), unit
        # <MT, AD, FUSE, T4, WIDE = true>: none in a narrow unit
        assert not any(re.search(r"rlc_ddpg_update_mfma_kernelILi\d+ELi\d+ELb[01]ELb[01]ELb1EE", n) for n in usage[unit]), unit
