// kl_mfma.hip -- shape check + launch of the MFMA ReverseKL / ForwardKL update kernel (kl_mfma_kernel.h).
// Instantiations: 2, 7 or 8 batch tiles for the three small networks (batch_size <= 32, the reference's default; <= 112;
// <= 128), 7 (8) batch tiles per pass of the action integral; the action_dim 1 instantiations and latency mode are
// compiled here, the action_dim 2 instantiations in kl_mfma_a2.hip (a unit of its own: the two compile side by side).
#include "kl_mfma_kernel.h"

int rlc_launch_kl_update_mfma_a2(const RlcSacDev& dv, int mt, int first_agent, int n_agents, int n_updates, int source,
                                 const long long* idx_dev, const float* eps_dev, int grad_taps, hipStream_t st,
                                 const RlcSacRollout* rollout);

// batch tiles of the three small networks: 2 (the reference's default batch 32), 7 (BASELINE's 100) or 8; the node passes
// always run at 7 (8) tiles
static inline int kl_mt_for(int B) { return B <= 32 ? 2 : (B <= 112 ? 7 : 8); }

// null when the MFMA kernel takes the shape, else the limit it exceeds
const char* rlc_kl_mfma_refusal(const RlcSacDims& d, int nodes) {
    auto okdim = [](int h) { return h >= 16 && h <= 256 && (h % 4) == 0; };
    if (!d.qcat) return "the MFMA KL kernel needs the input-concatenated Q layout";
    if (d.A != 1 && d.A != 2) return "the MFMA KL kernel is built for action_dim 1 and 2 (action_dim >= 3 runs the any-shape kernel)";
    if (!(okdim(d.L1A) && okdim(d.L2A) && okdim(d.L1C) && okdim(d.L2C)))
        return "the MFMA KL kernel needs layer widths that are multiples of 4 in [16, 256]";
    if (d.S < 1 || d.S + d.A > SMAX) return "the MFMA KL kernel needs state_dim + action_dim <= 8";
    if (d.B < 1 || d.B > 128) return "the MFMA KL kernel needs a batch size in [1, 128]";
    if (nodes < 0 || nodes > KL_MAXNODES) return "the MFMA KL kernel holds at most 256 quadrature nodes";
    const int mt = kl_mt_for(d.B);
    if (ksmem_carve(d, mt, mt == 8 ? 8 : 7, nullptr, nullptr) > 160 * 1024)
        return "the MFMA KL kernel needs more than 160 KiB of LDS at these widths and this batch size";
    return nullptr;
}

bool rlc_kl_mfma_supported(const RlcSacDims& d, int nodes) { return rlc_kl_mfma_refusal(d, nodes) == nullptr; }

size_t rlc_kl_mfma_scratch_floats(const RlcSacDims& d, int nodes) { return kl_mfma_scratch_floats(d, nodes, kl_mt_for(d.B)); }

int rlc_launch_kl_update_mfma(const RlcSacDev& dv, int first_agent, int n_agents, int n_updates, int source,
                              const long long* idx_dev, const float* eps_dev, int grad_taps, hipStream_t st,
                              const RlcSacRollout* rollout) {
    RLC_REQUIRE(rlc_kl_mfma_supported(dv.d, dv.kl_nodes), "MFMA KL kernel does not support these dimensions");
    RLC_REQUIRE(dv.d.blocked, "the MFMA kernel reads tile-blocked weights (rlc_kl_set_kernel re-packs them)");
    RLC_REQUIRE((size_t)dv.scratch_stride >= rlc_kl_mfma_scratch_floats(dv.d, dv.kl_nodes), "KL scratch row too short for the MFMA kernel");
    const int mt = kl_mt_for(dv.d.B);
    if (dv.d.A == 2)
        return rlc_launch_kl_update_mfma_a2(dv, mt, first_agent, n_agents, n_updates, source, idx_dev, eps_dev, grad_taps, st, rollout);
    if (mt == 2) return kl_launch_t<2, 7>(dv, first_agent, n_agents, n_updates, source, idx_dev, eps_dev, grad_taps, st, rollout);
    if (mt == 7) return kl_launch_t<7, 7>(dv, first_agent, n_agents, n_updates, source, idx_dev, eps_dev, grad_taps, st, rollout);
    return kl_launch_t<8, 8>(dv, first_agent, n_agents, n_updates, source, idx_dev, eps_dev, grad_taps, st, rollout);
}

// latency mode: the node passes of every agent's action integral dealt over C workgroups (kl_mfma_kernel.h)
size_t rlc_kl_split_zbuf_floats(const RlcSacDims& d) { return (size_t)32 * kl_mfma_ldh(d); }
int rlc_kl_split_grid(int n_agents, int C) { return kl_split_grid(n_agents, C); }

int rlc_launch_kl_update_mfma_split(const RlcSacDev& dv, float* zbuf, unsigned int* bar, int* err, int C, int first_agent,
                                    int n_agents, int n_updates, int source, const long long* idx_dev, const float* eps_dev,
                                    int grad_taps, hipStream_t st) {
    RLC_REQUIRE(rlc_kl_mfma_supported(dv.d, dv.kl_nodes), "MFMA KL kernel does not support these dimensions");
    RLC_REQUIRE(dv.d.blocked, "the MFMA kernel reads tile-blocked weights (rlc_kl_set_kernel re-packs them)");
    RLC_REQUIRE(dv.kl_optim == RLC_KL_OPTIM_INTG || dv.kl_optim == RLC_KL_OPTIM_HARD_INTG,
                "latency mode splits the action integral; the 'll' updates have none");
    RLC_REQUIRE(dv.d.A == 1, "latency mode of the KL agents is built for action_dim 1 (got %d)", dv.d.A);
    RLC_REQUIRE(dv.d.B <= 32, "latency mode of the KL agents is built for batch sizes up to 32 (got %d)", dv.d.B);
    const KlSplit sp = {zbuf, bar, err, C, n_agents};
    return kl_launch_split_t<2, 7>(dv, sp, first_agent, n_updates, source, idx_dev, eps_dev, grad_taps, st);
}
