// sac_mfma.hip -- shape check + dispatch to the per-shape instantiations of the MFMA SAC kernel
// (kernel: sac_mfma_kernel.h; instantiations: sac_mfma_inst.hip compiled per (MT, NTW, AD)).
#include <cstdio>

#include "sac_mfma_kernel.h"

#ifdef RLC_ONLY_7_1   // developer loop (RLC_FAST_BUILD=1): only the BASELINE shape is compiled
#define RLC_FOR_SAC(X) X(7, 1, 1)
#else
#define RLC_FOR_SAC(X)                                                                  \
    X(2, 1, 1) X(4, 1, 1) X(7, 1, 1) X(8, 1, 1) X(2, 2, 1) X(4, 2, 1) X(7, 2, 1) X(8, 2, 1) \
    X(2, 1, 2) X(4, 1, 2) X(7, 1, 2) X(8, 1, 2) X(2, 2, 2) X(4, 2, 2) X(7, 2, 2) X(8, 2, 2)
#endif

#define RLC_DECL3(M, N_, A_)                                                                                        \
    int rlc_sac_mfma_launch_##M##_##N_##_##A_(const RlcSacDev&, int, int, int, int, const long long*, const float*, int, \
                                              hipStream_t, const RlcSacRollout*);
RLC_FOR_SAC(RLC_DECL3)
// tail-of-four variants (compiled for the seven-tile shapes only: batch 97..100)
#ifdef RLC_ONLY_7_1
#define RLC_FOR_SAC_T4(X) X(7, 1, 1)
#else
#define RLC_FOR_SAC_T4(X) X(7, 1, 1) X(7, 2, 1) X(7, 1, 2) X(7, 2, 2)
#endif
#define RLC_DECLT4(M, N_, A_)                                                                                          \
    int rlc_sac_mfma_launch_t4_##M##_##N_##_##A_(const RlcSacDev&, int, int, int, int, const long long*, const float*, int, \
                                                 hipStream_t, const RlcSacRollout*);
RLC_FOR_SAC_T4(RLC_DECLT4)

// the wide form (sac_mfma_kernel.h, WIDE): state_dim <= 32, action_dim in {1,2,3,4,6}; no tail-of-four units.  The two
// eight-tile units at action_dim 6 are left out: their smallest shape needs 165,008 B of LDS, so
// rlc_sac_mfma_refusal names the LDS limit for every shape that would reach them.
#ifdef RLC_ONLY_7_1
#define RLC_FOR_SAC_W(X)
#else
#define RLC_FOR_SAC_W1(X, A_) X(2, 1, A_) X(4, 1, A_) X(7, 1, A_) X(8, 1, A_) X(2, 2, A_) X(4, 2, A_) X(7, 2, A_) X(8, 2, A_)
#define RLC_FOR_SAC_W(X)                                                                            \
    RLC_FOR_SAC_W1(X, 1) RLC_FOR_SAC_W1(X, 2) RLC_FOR_SAC_W1(X, 3) RLC_FOR_SAC_W1(X, 4)             \
    X(2, 1, 6) X(4, 1, 6) X(7, 1, 6) X(2, 2, 6) X(4, 2, 6) X(7, 2, 6)
#endif
#define RLC_DECLW(M, N_, A_)                                                                                          \
    int rlc_sac_mfma_launch_w_##M##_##N_##_##A_(const RlcSacDev&, int, int, int, int, const long long*, const float*, int, \
                                                hipStream_t, const RlcSacRollout*);
RLC_FOR_SAC_W(RLC_DECLW)

static inline int sac_mt_for(int B) { return B <= 32 ? 2 : (B <= 64 ? 4 : (B <= 112 ? 7 : 8)); }
static inline int sac_ntw_for(const RlcSacDims& d) {
    const int w = d.L2A > d.L2C ? d.L2A : d.L2C, k = d.L1A > d.L1C ? d.L1A : d.L1C;
    return (w <= 128 && k <= 128) ? 1 : 2;
}

static const size_t kLdsLimit = 160 * 1024;

// why the MFMA kernel (either form) cannot run these dimensions, or null; the text names the limit
const char* rlc_sac_mfma_refusal(const RlcSacDims& d) {
    if (d.norm) return "norm_type 'layer' runs on the any-shape kernel";
    if (d.qcat) return "the KL agents' input-concatenated Q network is not a SoftActorCritic shape";
    auto okdim = [](int h) { return h >= 16 && h <= 256 && (h % 4) == 0; };
    if (!(okdim(d.L1A) && okdim(d.L2A) && okdim(d.L1C) && okdim(d.L2C)))
        return "the MFMA kernel needs layer widths that are multiples of 4 in [16, 256]";
    if (d.S < 1 || d.S > SWIDE) return "the MFMA kernel needs state_dim <= 32";
    if (!(d.A == 1 || d.A == 2 || d.A == 3 || d.A == 4 || d.A == 6)) return "the MFMA kernel needs action_dim in {1, 2, 3, 4, 6}";
    if (d.B < 1 || d.B > 128) return "the MFMA kernel needs batch_size <= 128";
    const bool wide = rlc_sac_mfma_wide(d);
#ifdef RLC_ONLY_7_1
    if (wide) return "this build holds the headline shape's MFMA kernel only (state_dim <= 8, action_dim 1)";
#endif
    const int mt = sac_mt_for(d.B);
    size_t lds;
    if (sac_ntw_for(d) == 1) lds = wide ? ssmem_carve_wide<mask_stride(8)>(d, mt, nullptr, nullptr) : ssmem_carve<mask_stride(8)>(d, mt, nullptr, nullptr);
    else lds = wide ? ssmem_carve_wide<mask_stride(16)>(d, mt, nullptr, nullptr) : ssmem_carve<mask_stride(16)>(d, mt, nullptr, nullptr);
    if (lds > kLdsLimit) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "the MFMA kernel needs %zu bytes of LDS at these dimensions and batch size, %zu are allowed", lds,
                 kLdsLimit);
        return msg;
    }
    return nullptr;
}

// The shapes the MFMA kernel is the DEFAULT for (rlc_sac_create, the `auto` variant, the device loop): state_dim <= 8,
// action_dim <= 2.  The wide form runs on request only (rlc_sac_set_kernel).
bool rlc_sac_mfma_supported(const RlcSacDims& d) { return !rlc_sac_mfma_wide(d) && rlc_sac_mfma_refusal(d) == nullptr; }

int rlc_launch_sac_update_mfma(const RlcSacDev& dv, int first_agent, int n_agents, int n_updates, int source,
                               const long long* idx_dev, const float* eps_dev, int grad_taps, hipStream_t st,
                               const RlcSacRollout* rollout) {
    const char* why = rlc_sac_mfma_refusal(dv.d);
    RLC_REQUIRE(!why, "MFMA SAC kernel does not support these dimensions: %s", why);
    RLC_REQUIRE(dv.d.blocked, "the MFMA kernel reads tile-blocked weights (rlc_sac_set_kernel re-packs them)");
    RLC_REQUIRE(!(rollout && eps_dev), "the on-device loop draws its own eps");
    const int mt = sac_mt_for(dv.d.B), ntw = sac_ntw_for(dv.d);
    if (rlc_sac_mfma_wide(dv.d)) {
        RLC_REQUIRE(!rollout, "the on-device experiment loop runs the narrow MFMA kernel (state_dim <= 8, action_dim <= 2)");
#define RLC_CASEW(M, N_, A_)                       \
    if (mt == M && ntw == N_ && dv.d.A == A_)      \
        return rlc_sac_mfma_launch_w_##M##_##N_##_##A_(dv, first_agent, n_agents, n_updates, source, idx_dev, eps_dev, \
                                                       grad_taps, st, nullptr);
        RLC_FOR_SAC_W(RLC_CASEW)
#undef RLC_CASEW
        rlc_set_error("no wide MFMA SAC instantiation for MT=%d NTW=%d A=%d in this build", mt, ntw, dv.d.A);
        return 3;
    }
#define RLC_CASET4(M, N_, A_)                                                  \
    if (mt == M && ntw == N_ && dv.d.A == A_ && rlc_tail4_enabled(dv.d.B, M))  \
        return rlc_sac_mfma_launch_t4_##M##_##N_##_##A_(dv, first_agent, n_agents, n_updates, source, idx_dev, eps_dev, \
                                                        grad_taps, st, rollout);
    RLC_FOR_SAC_T4(RLC_CASET4)
#undef RLC_CASET4
#define RLC_CASE3(M, N_, A_)                       \
    if (mt == M && ntw == N_ && dv.d.A == A_)      \
        return rlc_sac_mfma_launch_##M##_##N_##_##A_(dv, first_agent, n_agents, n_updates, source, idx_dev, eps_dev, \
                                                     grad_taps, st, rollout);
    RLC_FOR_SAC(RLC_CASE3)
#undef RLC_CASE3
    rlc_set_error("no MFMA SAC instantiation for MT=%d NTW=%d A=%d in this build", mt, ntw, dv.d.A);
    return 3;
}
