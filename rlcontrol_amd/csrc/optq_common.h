// optq_common.h -- geometry and device view of the OptimalQ population.
// Blob = variable creation order (agents/network/optimal_q_network.py:82-108):
//   W1[S,L1] b1 | W2[L1+A,L2] b2 | W3[L2] b3        (the action rows are the LAST A rows of W2, :94)
// Device layout pads every tensor to 64 floats, always row-major (the agent runs on the any-shape kernel only); the
// ABI blob is compact.
#pragma once
#include "rlc_common.h"

#define RLC_OPTQ_MAX_A 6
#define RLC_OPTQ_SEG 6

struct RlcOptqDims {
    int S, A, L1, L2, B;
    int blocked;                // always 0 (the field the shared segment code reads)
    int W1, b1, W2, b2, W3, b3;
    int P, Pdev, Ppad, nseg;
    int seg_len[RLC_OPTQ_SEG], seg_compact[RLC_OPTQ_SEG], seg_dev[RLC_OPTQ_SEG];
    int seg_rows[RLC_OPTQ_SEG], seg_cols[RLC_OPTQ_SEG], seg_h[RLC_OPTQ_SEG];
    char seg_big[RLC_OPTQ_SEG];
};

inline RlcOptqDims rlc_optq_make_dims(int S, int A, int L1, int L2, int B) {
    RlcOptqDims d;
    d.S = S; d.A = A; d.L1 = L1; d.L2 = L2; d.B = B; d.blocked = 0;
    int n = 0;
    int* slot[RLC_OPTQ_SEG];
    auto seg = [&](int* where, int r, int c) {
        slot[n] = where; d.seg_rows[n] = r; d.seg_cols[n] = c; d.seg_h[n] = r; d.seg_big[n] = 0; n++;
    };
    seg(&d.W1, S, L1); seg(&d.b1, 1, L1);
    seg(&d.W2, L1 + A, L2); seg(&d.b2, 1, L2);
    seg(&d.W3, L2, 1); seg(&d.b3, 1, 1);
    d.nseg = n;
    rlc_layout_segs(d);
    for (int i = 0; i < n; i++) *slot[i] = d.seg_dev[i];
    return d;
}

struct RlcOptqDev {
    RlcOptqDims d;
    RlcReplayDev rep;
    int n_agents;
    int clip_state;
    float tau;
    int n_nodes;
    float *theta, *theta_t, *m, *v;   // [n_agents][Ppad]
    float* pw;                        // [n_agents][2] beta powers
    const float* lr;                  // [n_agents]
    const float *smin, *smax;
    const float* grid;                // [n_nodes][A] discretized_action_pairs, shared by every agent
    float *tap_q, *tap_y, *tap_maxq;  // [n_agents][RLC_MAX_BATCH]
    float* tap_astar;                 // [n_agents][RLC_MAX_BATCH][A]
    float* tap_g;                     // [n_agents][Ppad] (rlc_optq_enable_grad_taps)
    float* scratch;
    long long scratch_stride;
};

size_t rlc_optq_scratch_floats(const RlcOptqDims& d);
// null, or why these dimensions cannot run (the LDS the grid pass needs against 64 KiB)
const char* rlc_optq_refusal(const RlcOptqDims& d);
int rlc_launch_optq_update(const RlcOptqDev& dv, int first_agent, int n_agents, int n_updates, int source,
                           const long long* idx_dev, int grad_taps, hipStream_t st);
// greedy grid row [n][A] and its online Q [n] for one state per agent of [first_agent, first_agent + n)
int rlc_launch_optq_act(const RlcOptqDev& dv, int first_agent, int n, const float* states_dev, float* action_dev,
                        float* q_dev, hipStream_t st, int* done_flag = nullptr, int done_val = 0);
int rlc_launch_optq_qval(const RlcOptqDev& dv, int agent, int n, const float* states_dev, const float* actions_dev,
                         float* out_dev, hipStream_t st);
