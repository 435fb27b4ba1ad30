"""The build audit's record of the wide instantiations of the MFMA NAF kernel (state_dim <= 32, action_dim in {1,2,3,4,6};
rlcontrol_amd/kernel_resource_usage.json, written by __graft_entry__.build()): every (MT, NTW, AD) unit present once, free
of whole-wave spills and exec-0 restore copies (rlcontrol_amd/build.py::audit_object), and held to the build's spill
policy; the 20 narrow units are still there and hold no wide instantiation."""
import json
import os
import re

import pytest

# every combination is compiled: each is reached by some shape within the LDS limit
WIDE = [(mt, ntw, ad) for ad in (1, 2, 3, 4, 6) for ntw in (1, 2) for mt in (2, 4, 7, 8)]
NARROW = ["naf_mfma_%d_%d_%d.o" % (mt, ntw, ad) for ad in (1, 2) for ntw in (1, 2) for mt in (2, 4, 7, 8)] + [
    "naf_mfma_7_%d_%d_t4.o" % (ntw, ad) for ad in (1, 2) for ntw in (1, 2)]


def _usage():
    from rlcontrol_amd import build as B
    if not os.path.exists(B.USAGE_JSON):
        import __graft_entry__ as g
        g.build()
    with open(B.USAGE_JSON) as f:
        return json.load(f)


@pytest.mark.parametrize("mt,ntw,ad", WIDE)
def test_wide_naf_instantiations_are_audited_and_clean(mt, ntw, ad):
    usage = _usage()
    unit = "naf_mfma_w_%d_%d_%d.o" % (mt, ntw, ad)
    assert unit in usage, (unit, sorted(u for u in usage if u.startswith("naf_mfma")))
    # <MT, NTW, AD, T4 = false, WIDE = true> in the Itanium mangling of the kernel's template arguments
    tag = "rlc_naf_update_mfma_kernelILi%dELi%dELi%dELb0ELb1EE" % (mt, ntw, ad)
    found = [(n, k) for n, k in usage[unit].items() if "rlc_naf_update_mfma_kernel" in n]
    assert len(found) == 1 and tag in found[0][0], (tag, sorted(usage[unit]))
    name, k = found[0]
    print("wide <MT %d, NTW %d, AD %d>: %d VGPRs, %d VGPR spills, %d SGPR spills, %d B of scratch" % (
        mt, ntw, ad, k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"], k["private_segment_fixed_size"]))
    assert k["exec0_copies"] == 0 and k["wwm_spills"] == 0, (name, k)


def test_wide_naf_units_are_under_the_spill_policy():
    from rlcontrol_amd import build as B
    assert sorted(B.NAF_WIDE_VARIANTS) == sorted(WIDE)
    for v in WIDE:
        assert "naf_mfma_w_%d_%d_%d.o" % v in B.GUARDED_UNITS


def test_narrow_naf_mfma_units_are_still_there():
    usage = _usage()
    assert len(NARROW) == 20
    for unit in NARROW:
        assert unit in usage and any("rlc_naf_update_mfma_kernel" in n for n in usage[unit]), unit
        # <MT, NTW, AD, T4, WIDE = true>: none in a narrow unit
        assert not any(re.search(r"rlc_naf_update_mfma_kernelILi\d+ELi\d+ELi\d+ELb[01]ELb1EE", n) for n in usage[unit]), unit
        for n, k in usage[unit].items():
            print("narrow %s: %d VGPRs, %d VGPR spills, %d SGPR spills, %d B of scratch" % (
                unit, k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"], k["private_segment_fixed_size"]))
