// ddpg_mfma.hip -- shape check + dispatch to the per-shape instantiations of the MFMA DDPG kernel
// (kernel: ddpg_mfma_kernel.h; instantiations: ddpg_mfma_inst.hip compiled per (MT, AD)).
#include <cstdio>

#include "ddpg_mfma_kernel.h"
#include "ddpg_ln_mfma_kernel.h"

#ifdef RLC_ONLY_7_1   // developer loop (RLC_FAST_BUILD=1): only the headline shape is compiled
#define RLC_FOR_V2(X) X(7, 1)
#else
#define RLC_FOR_V2(X) X(2, 1) X(4, 1) X(7, 1) X(8, 1) X(2, 2) X(4, 2) X(7, 2) X(8, 2)
#endif

#define RLC_DECL2(M, A_) \
    int rlc_mfma_launch_##M##_##A_(const RlcDev&, int, int, int, int, const long long*, int, hipStream_t, const RlcRollout*, int);
RLC_FOR_V2(RLC_DECL2)
// tail-of-four variants (compiled for the seven-tile shapes only: batch 97..100)
#ifdef RLC_ONLY_7_1
#define RLC_FOR_T4(X) X(7, 1)
#else
#define RLC_FOR_T4(X) X(7, 1) X(7, 2)
#endif
#define RLC_DECLT4(M, A_) \
    int rlc_mfma_launch_t4_##M##_##A_(const RlcDev&, int, int, int, int, const long long*, int, hipStream_t, const RlcRollout*, int);
RLC_FOR_T4(RLC_DECLT4)

// the wide form (ddpg_mfma_kernel.h, WIDE): state_dim <= 32, action_dim in {1,2,3,4,6}; no tail-of-four units
#ifdef RLC_ONLY_7_1
#define RLC_FOR_W(X)
#else
#define RLC_FOR_W(X)                                                                                         \
    X(2, 1) X(4, 1) X(7, 1) X(8, 1) X(2, 2) X(4, 2) X(7, 2) X(8, 2) X(2, 3) X(4, 3) X(7, 3) X(8, 3) X(2, 4) \
    X(4, 4) X(7, 4) X(8, 4) X(2, 6) X(4, 6) X(7, 6) X(8, 6)
#endif
#define RLC_DECLW(M, A_) \
    int rlc_mfma_launch_w_##M##_##A_(const RlcDev&, int, int, int, int, const long long*, int, hipStream_t, const RlcRollout*, int);
RLC_FOR_W(RLC_DECLW)

// the layer-norm form (ddpg_ln_mfma_kernel.h): the hydra network at state_dim <= 8, action_dim <= 2; no tail-of-four units;
// the on-device loop as the narrow form has it (a runtime pointer, not units of its own)
#ifdef RLC_ONLY_7_1
#define RLC_FOR_LN(X)
#else
#define RLC_FOR_LN(X) X(2, 1) X(4, 1) X(7, 1) X(8, 1) X(2, 2) X(4, 2) X(7, 2) X(8, 2)
#endif
#define RLC_DECLLN(M, A_) \
    int rlc_mfma_launch_ln_##M##_##A_(const RlcDev&, int, int, int, int, const long long*, int, hipStream_t, const RlcRollout*, int);
RLC_FOR_LN(RLC_DECLLN)

static inline int mt_for(int B) { return B <= 32 ? 2 : (B <= 64 ? 4 : (B <= 112 ? 7 : 8)); }

static const size_t kLdsLimit = 160 * 1024;

// why the MFMA kernel (either form) cannot run these dimensions, or null; the text names the limit
const char* rlc_mfma_refusal(const RlcDims& d) {
    auto okdim = [](int h) { return h >= 16 && h <= 256 && (h % 4) == 0; };
    if (!(okdim(d.H1) && okdim(d.HA) && okdim(d.HC))) return "the MFMA kernel needs layer widths that are multiples of 4 in [16, 256]";
    if (d.S < 1 || d.S > SWIDE) return "the MFMA kernel needs state_dim <= 32";
    if (!(d.A == 1 || d.A == 2 || d.A == 3 || d.A == 4 || d.A == 6)) return "the MFMA kernel needs action_dim in {1, 2, 3, 4, 6}";
    if (d.B < 1 || d.B > 128) return "the MFMA kernel needs batch_size <= 128";
#ifdef RLC_ONLY_7_1
    if (rlc_mfma_wide(d)) return "this build holds the headline shape's MFMA kernel only (state_dim <= 8, action_dim 1)";
#endif
    if (d.norm) {
        // the layer-norm form: opt-in like the wide form (rlc_mfma_supported stays false for it)
        if (d.sep) return "norm_type 'layer' with network 'separate' runs on the any-shape kernel";
        if (rlc_mfma_wide(d)) return "norm_type 'layer' on the MFMA kernel needs state_dim <= 8 and action_dim <= 2";
#ifdef RLC_ONLY_7_1
        return "this build holds no MFMA kernel for norm_type 'layer'";
#endif
    }
    const size_t lds = d.norm ? smem_carve_ln(d, mt_for(d.B), nullptr, nullptr)
                       : rlc_mfma_wide(d) ? smem_carve<true>(d, mt_for(d.B), nullptr, nullptr)
                                        : smem_carve<false>(d, mt_for(d.B), nullptr, nullptr);
    if (lds > kLdsLimit) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "the MFMA kernel needs %zu bytes of LDS at these dimensions and batch size, %zu are allowed", lds,
                 kLdsLimit);
        return msg;
    }
    return nullptr;
}

// The shapes the MFMA kernel is the DEFAULT for (rlc_ddpg_create, the `auto` variant, latency mode, the device loop):
// state_dim <= 8, action_dim <= 2, no layer norm.  The wide form and the layer-norm form run on request only
// (rlc_ddpg_set_kernel).
bool rlc_mfma_supported(const RlcDims& d) { return !d.norm && !rlc_mfma_wide(d) && rlc_mfma_refusal(d) == nullptr; }

int rlc_launch_ddpg_update_mfma(const RlcDev& dv, int first_agent, int n_agents, int n_updates, int source,
                                const long long* idx_dev, int grad_taps, hipStream_t st, const RlcRollout* rollout,
                                int q8_first) {
    const char* why = rlc_mfma_refusal(dv.d);
    RLC_REQUIRE(!why, "MFMA kernel does not support these dimensions: %s", why);
    RLC_REQUIRE(dv.d.blocked, "the MFMA kernel reads tile-blocked weights (rlc_ddpg_set_kernel re-packs them)");
    const int mt = mt_for(dv.d.B);
    if (dv.d.norm) {
#define RLC_CASELN(M, A_)         \
    if (mt == M && dv.d.A == A_)  \
        return rlc_mfma_launch_ln_##M##_##A_(dv, first_agent, n_agents, n_updates, source, idx_dev, grad_taps, st, rollout, \
                                             q8_first);
        RLC_FOR_LN(RLC_CASELN)
#undef RLC_CASELN
        rlc_set_error("no layer-norm MFMA instantiation for MT=%d A=%d in this build", mt, dv.d.A);
        return 3;
    }
    if (rlc_mfma_wide(dv.d)) {
        RLC_REQUIRE(!rollout, "the on-device experiment loop runs the narrow MFMA kernel (state_dim <= 8, action_dim <= 2)");
#define RLC_CASEW(M, A_)          \
    if (mt == M && dv.d.A == A_)  \
        return rlc_mfma_launch_w_##M##_##A_(dv, first_agent, n_agents, n_updates, source, idx_dev, grad_taps, st, nullptr, 0);
        RLC_FOR_W(RLC_CASEW)
#undef RLC_CASEW
        rlc_set_error("no wide MFMA instantiation for MT=%d A=%d in this build", mt, dv.d.A);
        return 3;
    }
#define RLC_CASET4(M, A_)                                           \
    if (mt == M && dv.d.A == A_ && rlc_tail4_enabled(dv.d.B, M))    \
        return rlc_mfma_launch_t4_##M##_##A_(dv, first_agent, n_agents, n_updates, source, idx_dev, grad_taps, st, rollout, \
                                             q8_first);
    RLC_FOR_T4(RLC_CASET4)
#undef RLC_CASET4
#define RLC_CASE2(M, A_)          \
    if (mt == M && dv.d.A == A_)  \
        return rlc_mfma_launch_##M##_##A_(dv, first_agent, n_agents, n_updates, source, idx_dev, grad_taps, st, rollout, \
                                          q8_first);
    RLC_FOR_V2(RLC_CASE2)
#undef RLC_CASE2
    rlc_set_error("no MFMA instantiation for MT=%d A=%d in this build", mt, dv.d.A);
    return 3;
}
