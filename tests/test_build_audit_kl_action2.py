"""The build audit's record of the action_dim 2 instantiations of the MFMA ReverseKL / ForwardKL kernel
(rlcontrol_amd/kernel_resource_usage.json, written by __graft_entry__.build()): present, and free of whole-wave spills
and exec-0 restore copies (rlcontrol_amd/build.py::audit_object)."""
import json
import os

import pytest

# <MT, MTQ, SPLIT = false, AD = 2> in the Itanium mangling of rlc_kl_update_mfma_kernel's template arguments
NEW = {"<2,7,2>": "rlc_kl_update_mfma_kernelILi2ELi7ELb0ELi2EE", "<7,7,2>": "rlc_kl_update_mfma_kernelILi7ELi7ELb0ELi2EE",
       "<8,8,2>": "rlc_kl_update_mfma_kernelILi8ELi8ELb0ELi2EE"}


def _usage():
    from rlcontrol_amd import build as B
    if not os.path.exists(B.USAGE_JSON):
        import __graft_entry__ as g
        g.build()
    with open(B.USAGE_JSON) as f:
        return json.load(f)


@pytest.mark.parametrize("inst", sorted(NEW))
def test_kl_mfma_action2_instantiations_are_audited_and_clean(inst):
    kernels = _usage()["kl_mfma_a2.o"]
    found = [(n, k) for n, k in kernels.items() if NEW[inst] in n]
    assert len(found) == 1, (inst, sorted(kernels))
    name, k = found[0]
    print("%s: %d VGPRs, %d VGPR spills, %d SGPR spills, %d B of scratch" % (
        inst, k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"], k["private_segment_fixed_size"]))
    assert k["exec0_copies"] == 0 and k["wwm_spills"] == 0, (name, k)


def test_kl_mfma_action1_instantiations_are_still_there():
    kernels = _usage()["kl_mfma.o"]
    for tag in ("ILi2ELi7ELb0ELi1EE", "ILi7ELi7ELb0ELi1EE", "ILi8ELi8ELb0ELi1EE", "ILi2ELi7ELb1ELi1EE"):
        assert any("rlc_kl_update_mfma_kernel" + tag in n for n in kernels), tag
