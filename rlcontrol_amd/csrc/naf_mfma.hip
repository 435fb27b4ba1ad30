// naf_mfma.hip -- shape check + dispatch to the per-shape instantiations of the MFMA NAF kernel
// (kernel: naf_mfma_kernel.h; instantiations: naf_mfma_inst.hip compiled per (MT, NTW, AD)).
#include <cstdio>

#include "naf_mfma_kernel.h"

#ifdef RLC_ONLY_7_1   // developer loop (RLC_FAST_BUILD=1): only the BASELINE shape is compiled
#define RLC_FOR_NAF(X) X(7, 2, 2)
#else
#define RLC_FOR_NAF(X)                                                                  \
    X(2, 1, 1) X(4, 1, 1) X(7, 1, 1) X(8, 1, 1) X(2, 2, 1) X(4, 2, 1) X(7, 2, 1) X(8, 2, 1) \
    X(2, 1, 2) X(4, 1, 2) X(7, 1, 2) X(8, 1, 2) X(2, 2, 2) X(4, 2, 2) X(7, 2, 2) X(8, 2, 2)
#endif

#define RLC_DECL3(M, N_, A_)                                                                                  \
    int rlc_naf_mfma_launch_##M##_##N_##_##A_(const RlcNafDev&, int, int, int, int, const long long*, int, hipStream_t, \
                                              const RlcNafRollout*);
RLC_FOR_NAF(RLC_DECL3)
// tail-of-four variants (compiled for the seven-tile shapes only: batch 97..100)
#ifdef RLC_ONLY_7_1
#define RLC_FOR_NAF_T4(X) X(7, 2, 2)
#else
#define RLC_FOR_NAF_T4(X) X(7, 1, 1) X(7, 2, 1) X(7, 1, 2) X(7, 2, 2)
#endif
#define RLC_DECLT4(M, N_, A_)                                                                                    \
    int rlc_naf_mfma_launch_t4_##M##_##N_##_##A_(const RlcNafDev&, int, int, int, int, const long long*, int, hipStream_t, \
                                                 const RlcNafRollout*);
RLC_FOR_NAF_T4(RLC_DECLT4)

// the wide form (naf_mfma_kernel.h, WIDE): state_dim <= 32, action_dim in {1,2,3,4,6}; no tail-of-four units
#ifdef RLC_ONLY_7_1
#define RLC_FOR_NAF_W(X)
#else
#define RLC_FOR_NAF_W1(X, A_) X(2, 1, A_) X(4, 1, A_) X(7, 1, A_) X(8, 1, A_) X(2, 2, A_) X(4, 2, A_) X(7, 2, A_) X(8, 2, A_)
#define RLC_FOR_NAF_W(X) RLC_FOR_NAF_W1(X, 1) RLC_FOR_NAF_W1(X, 2) RLC_FOR_NAF_W1(X, 3) RLC_FOR_NAF_W1(X, 4) RLC_FOR_NAF_W1(X, 6)
#endif
#define RLC_DECLW(M, N_, A_)                                                                                    \
    int rlc_naf_mfma_launch_w_##M##_##N_##_##A_(const RlcNafDev&, int, int, int, int, const long long*, int, hipStream_t, \
                                                const RlcNafRollout*);
RLC_FOR_NAF_W(RLC_DECLW)

static inline int naf_mt_for(int B) { return B <= 32 ? 2 : (B <= 64 ? 4 : (B <= 112 ? 7 : 8)); }
static inline int naf_ntw_for(const RlcNafDims& d) { return (d.L1 <= 128 && d.L2 <= 128) ? 1 : 2; }

static const size_t kLdsLimit = 160 * 1024;

// why the MFMA kernel (either form) cannot run these dimensions, or null; the text names the limit
const char* rlc_naf_mfma_refusal(const RlcNafDims& d) {
    if (d.norm) return "norm_type 'layer' runs on the any-shape kernel";
    auto okdim = [](int h) { return h >= 16 && h <= 256 && (h % 4) == 0; };
    if (!(okdim(d.L1) && okdim(d.L2))) return "the MFMA kernel needs layer widths that are multiples of 4 in [16, 256]";
    if (d.S < 1 || d.S > SWIDE) return "the MFMA kernel needs state_dim <= 32";
    if (!(d.A == 1 || d.A == 2 || d.A == 3 || d.A == 4 || d.A == 6)) return "the MFMA kernel needs action_dim in {1, 2, 3, 4, 6}";
    if (d.B < 1 || d.B > 128) return "the MFMA kernel needs batch_size <= 128";
    const bool wide = rlc_naf_mfma_wide(d);
#ifdef RLC_ONLY_7_1
    if (wide) return "this build holds the headline shape's MFMA kernel only (state_dim <= 8, action_dim <= 2)";
#endif
    const int mt = naf_mt_for(d.B);
    size_t lds;
    if (naf_ntw_for(d) == 1) lds = wide ? nsmem_carve_wide<mask_stride(8)>(d, mt, nullptr, nullptr) : nsmem_carve<mask_stride(8)>(d, mt, nullptr, nullptr);
    else lds = wide ? nsmem_carve_wide<mask_stride(16)>(d, mt, nullptr, nullptr) : nsmem_carve<mask_stride(16)>(d, mt, nullptr, nullptr);
    if (lds > kLdsLimit) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "the MFMA kernel needs %zu bytes of LDS at these dimensions and batch size, %zu are allowed", lds,
                 kLdsLimit);
        return msg;
    }
    return nullptr;
}

// The shapes the MFMA kernel is the DEFAULT for (rlc_naf_create, the `auto` variant, the device loop): state_dim <= 8,
// action_dim <= 2.  The wide form runs on request only (rlc_naf_set_kernel).
bool rlc_naf_mfma_supported(const RlcNafDims& d) { return !rlc_naf_mfma_wide(d) && rlc_naf_mfma_refusal(d) == nullptr; }

int rlc_launch_naf_update_mfma(const RlcNafDev& dv, int first_agent, int n_agents, int n_updates, int source,
                               const long long* idx_dev, int grad_taps, hipStream_t st, const RlcNafRollout* rollout) {
    const char* why = rlc_naf_mfma_refusal(dv.d);
    RLC_REQUIRE(!why, "MFMA NAF kernel does not support these dimensions: %s", why);
    RLC_REQUIRE(dv.d.blocked, "the MFMA kernel reads tile-blocked weights (rlc_naf_set_kernel re-packs them)");
    const int mt = naf_mt_for(dv.d.B), ntw = naf_ntw_for(dv.d);
    if (rlc_naf_mfma_wide(dv.d)) {
        RLC_REQUIRE(!rollout, "the on-device experiment loop runs the narrow MFMA kernel (state_dim <= 8, action_dim <= 2)");
#define RLC_CASEW(M, N_, A_)                       \
    if (mt == M && ntw == N_ && dv.d.A == A_)      \
        return rlc_naf_mfma_launch_w_##M##_##N_##_##A_(dv, first_agent, n_agents, n_updates, source, idx_dev, grad_taps, st, \
                                                       nullptr);
        RLC_FOR_NAF_W(RLC_CASEW)
#undef RLC_CASEW
        rlc_set_error("no wide MFMA NAF instantiation for MT=%d NTW=%d A=%d in this build", mt, ntw, dv.d.A);
        return 3;
    }
#define RLC_CASET4(M, N_, A_)                                                  \
    if (mt == M && ntw == N_ && dv.d.A == A_ && rlc_tail4_enabled(dv.d.B, M))  \
        return rlc_naf_mfma_launch_t4_##M##_##N_##_##A_(dv, first_agent, n_agents, n_updates, source, idx_dev, grad_taps, st, \
                                                        rollout);
    RLC_FOR_NAF_T4(RLC_CASET4)
#undef RLC_CASET4
#define RLC_CASE3(M, N_, A_)                       \
    if (mt == M && ntw == N_ && dv.d.A == A_)      \
        return rlc_naf_mfma_launch_##M##_##N_##_##A_(dv, first_agent, n_agents, n_updates, source, idx_dev, grad_taps, st, \
                                                     rollout);
    RLC_FOR_NAF(RLC_CASE3)
#undef RLC_CASE3
    rlc_set_error("no MFMA NAF instantiation for MT=%d NTW=%d A=%d in this build", mt, ntw, dv.d.A);
    return 3;
}
