// kl_mfma_a2.hip -- the action_dim 2 instantiations of the MFMA ReverseKL / ForwardKL update kernel (kl_mfma_kernel.h);
// shape check and dispatch are in kl_mfma.hip.
#include "kl_mfma_kernel.h"

// mt: batch tiles of the three small networks as kl_mfma.hip chose them (2, 7 or 8)
int rlc_launch_kl_update_mfma_a2(const RlcSacDev& dv, int mt, int first_agent, int n_agents, int n_updates, int source,
                                 const long long* idx_dev, const float* eps_dev, int grad_taps, hipStream_t st,
                                 const RlcSacRollout* rollout) {
    RLC_REQUIRE(dv.d.A == 2, "these instantiations are built for action_dim 2 (got %d)", dv.d.A);
    if (mt == 2) return kl_launch_t<2, 7, 2>(dv, first_agent, n_agents, n_updates, source, idx_dev, eps_dev, grad_taps, st, rollout);
    if (mt == 7) return kl_launch_t<7, 7, 2>(dv, first_agent, n_agents, n_updates, source, idx_dev, eps_dev, grad_taps, st, rollout);
    return kl_launch_t<8, 8, 2>(dv, first_agent, n_agents, n_updates, source, idx_dev, eps_dev, grad_taps, st, rollout);
}
