"""The build audit's record of the layer-norm instantiations of the MFMA DDPG kernel (rlcontrol_amd/kernel_resource_usage.json,
written by __graft_entry__.build()): the eight ddpg_mfma_ln_<MT>_<AD> units are present, each holds exactly one update
kernel, free of whole-wave spills and exec-0 restore copies (rlcontrol_amd/build.py::audit_object); the narrow and wide
units are still there."""
import json
import os

import pytest

LN_UNITS = [(mt, ad) for ad in (1, 2) for mt in (2, 4, 7, 8)]


def _usage():
    from rlcontrol_amd import build as B
    if not os.path.exists(B.USAGE_JSON):
        import __graft_entry__ as g
        g.build()
    with open(B.USAGE_JSON) as f:
        return json.load(f)


@pytest.mark.parametrize("mt,ad", LN_UNITS)
def test_ddpg_layer_mfma_units_are_audited_and_clean(mt, ad):
    usage = _usage()
    unit = "ddpg_mfma_ln_%d_%d.o" % (mt, ad)
    assert unit in usage, sorted(u for u in usage if u.startswith("ddpg_mfma"))
    kernels = usage[unit]
    # <MT, AD> in the Itanium mangling of rlc_ddpg_update_ln_mfma_kernel's template arguments
    found = [(n, k) for n, k in kernels.items() if "rlc_ddpg_update_ln_mfma_kernelILi%dELi%dEE" % (mt, ad) in n]
    assert len(found) == 1 and len(kernels) == 1, (unit, sorted(kernels))
    name, k = found[0]
    print("%s: %d VGPRs, %d VGPR spills, %d SGPR spills, %d B of scratch" % (
        unit, k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"], k["private_segment_fixed_size"]))
    assert k["exec0_copies"] == 0 and k["wwm_spills"] == 0, (name, k)


def test_ddpg_layer_mfma_units_are_guarded_by_the_build():
    from rlcontrol_amd import build as B
    for mt, ad in LN_UNITS:
        assert "ddpg_mfma_ln_%d_%d.o" % (mt, ad) in B.GUARDED_UNITS


def test_narrow_and_wide_ddpg_mfma_units_are_still_there():
    usage = _usage()
    for ad in (1, 2):
        for mt in (2, 4, 7, 8):
            assert any("rlc_ddpg_update_mfma_kernel" in n for n in usage["ddpg_mfma_%d_%d.o" % (mt, ad)]), (mt, ad)
    for ad in (1, 2, 3, 4, 6):
        for mt in (2, 4, 7, 8):
            assert any("rlc_ddpg_update_mfma_kernel" in n for n in usage["ddpg_mfma_w_%d_%d.o" % (mt, ad)]), (mt, ad)
