// wf_common.h -- geometry and device view of the WireFitting population.
// Blob = variable creation order (agents/network/wf_network.py:66-125):
//   W1[S,L1] b1 | W2[L1,L2] b2 | Wa[L2,N*A] ba | Wq[L2,N] bq | kappa[N]      (N = app_points; kappa = smooth_c, :116)
// Wire i owns columns i*A .. i*A+A-1 of the action head (the reshape to [B, N, A], :112).
// Device layout pads every tensor to 64 floats, always row-major (the agent runs on the any-shape kernel only); the
// ABI blob is compact.
#pragma once
#include "rlc_common.h"

#define RLC_WF_MAX_A 6
#define RLC_WF_MAX_NA 1024      // app_points * action_dim
#define RLC_WF_SEG 9

struct RlcWfDims {
    int S, A, L1, L2, N, B;
    int blocked;                // always 0 (the field the shared segment code reads)
    int W1, b1, W2, b2, Wa, ba, Wq, bq, kap;
    int P, Pdev, Ppad, nseg;
    int seg_len[RLC_WF_SEG], seg_compact[RLC_WF_SEG], seg_dev[RLC_WF_SEG];
    int seg_rows[RLC_WF_SEG], seg_cols[RLC_WF_SEG], seg_h[RLC_WF_SEG];
    char seg_big[RLC_WF_SEG];
};

inline RlcWfDims rlc_wf_make_dims(int S, int A, int L1, int L2, int N, int B) {
    RlcWfDims d;
    d.S = S; d.A = A; d.L1 = L1; d.L2 = L2; d.N = N; d.B = B; d.blocked = 0;
    int n = 0;
    int* slot[RLC_WF_SEG];
    auto seg = [&](int* where, int r, int c) {
        slot[n] = where; d.seg_rows[n] = r; d.seg_cols[n] = c; d.seg_h[n] = r; d.seg_big[n] = 0; n++;
    };
    seg(&d.W1, S, L1); seg(&d.b1, 1, L1);
    seg(&d.W2, L1, L2); seg(&d.b2, 1, L2);
    seg(&d.Wa, L2, N * A); seg(&d.ba, 1, N * A);
    seg(&d.Wq, L2, N); seg(&d.bq, 1, N);
    seg(&d.kap, 1, N);
    d.nseg = n;
    rlc_layout_segs(d);
    for (int i = 0; i < n; i++) *slot[i] = d.seg_dev[i];
    return d;
}

struct RlcWfDev {
    RlcWfDims d;
    RlcReplayDev rep;
    int n_agents;
    int clip_state;
    float tau;
    float amax0;                      // action_max[0]: the one scalar that scales every wire action (wf_network.py:88)
    float *theta, *theta_t, *m, *v;   // [n_agents][Ppad]
    float* pw;                        // [n_agents][2] beta powers
    const float* lr;                  // [n_agents]
    const float *smin, *smax;
    float *tap_q, *tap_y, *tap_maxq;  // [n_agents][RLC_MAX_BATCH]
    float* tap_g;                     // [n_agents][Ppad] (rlc_wf_enable_grad_taps)
    float* scratch;
    long long scratch_stride;
};

size_t rlc_wf_scratch_floats(const RlcWfDims& d);
// null, or why these dimensions cannot run (the LDS the kernels need against 64 KiB)
const char* rlc_wf_refusal(const RlcWfDims& d);
int rlc_launch_wf_update(const RlcWfDev& dv, int first_agent, int n_agents, int n_updates, int source,
                         const long long* idx_dev, int grad_taps, hipStream_t st);
// per state of agents [first_agent, first_agent + n): out_dev = the arg-max wire's action [n][A], then every wire's
// action [n][N][A], then every wire's value [n][N]
int rlc_launch_wf_act(const RlcWfDev& dv, int first_agent, int n, const float* states_dev, float* out_dev,
                      hipStream_t st, int* done_flag = nullptr, int done_val = 0);
int rlc_launch_wf_qval(const RlcWfDev& dv, int agent, int n, const float* states_dev, const float* actions_dev,
                       float* out_dev, hipStream_t st);
