// ae_common.h -- geometry and device view of the ActorExpert population.
// Blob = variable creation order (agents/network/ae_network.py:138-229):
//   W1[S,L1] b1 | Wa2[L1,La] ba2 | Wm[La,M*A] bm | Ws[La,M*A] bs | Wal[La,M] bal | Wq2[L1+A,Le] bq2 | Wq3[Le] bq3
// (M = num_modal; the action rows are LAST in Wq2, :214).  Mode m, dimension d is column m*A + d of the mean and the
// sigma head (the reshape to [B, M, A], :189-190).
// Device layout pads every tensor to 64 floats, always row-major (the agent runs on the any-shape kernel only); the
// ABI blob is compact.
#pragma once
#include "rlc_common.h"

#define RLC_AE_MAX_A 6
#define RLC_AE_MAX_M 8
#define RLC_AE_MAX_SAMPLES 1024
#define RLC_AE_SEG 14

struct RlcAeDims {
    int S, A, L1, La, Le, M, n, k, B;   // n = num_samples, k = top_k = int(num_samples * rho)
    int blocked;                        // always 0 (the field the shared segment code reads)
    int W1, b1, Wa2, ba2, Wm, bm, Ws, bs, Wal, bal, Wq2, bq2, Wq3, bq3;
    int P, Pdev, Ppad, nseg;
    int seg_len[RLC_AE_SEG], seg_compact[RLC_AE_SEG], seg_dev[RLC_AE_SEG];
    int seg_rows[RLC_AE_SEG], seg_cols[RLC_AE_SEG], seg_h[RLC_AE_SEG];
    char seg_big[RLC_AE_SEG];
};

inline RlcAeDims rlc_ae_make_dims(int S, int A, int L1, int La, int Le, int M, int n, int k, int B) {
    RlcAeDims d;
    d.S = S; d.A = A; d.L1 = L1; d.La = La; d.Le = Le; d.M = M; d.n = n; d.k = k; d.B = B; d.blocked = 0;
    int c = 0;
    int* slot[RLC_AE_SEG];
    auto seg = [&](int* where, int r, int cols) {
        slot[c] = where; d.seg_rows[c] = r; d.seg_cols[c] = cols; d.seg_h[c] = r; d.seg_big[c] = 0; c++;
    };
    seg(&d.W1, S, L1); seg(&d.b1, 1, L1);
    seg(&d.Wa2, L1, La); seg(&d.ba2, 1, La);
    seg(&d.Wm, La, M * A); seg(&d.bm, 1, M * A);
    seg(&d.Ws, La, M * A); seg(&d.bs, 1, M * A);
    seg(&d.Wal, La, M); seg(&d.bal, 1, M);
    seg(&d.Wq2, L1 + A, Le); seg(&d.bq2, 1, Le);
    seg(&d.Wq3, Le, 1); seg(&d.bq3, 1, 1);
    d.nseg = c;
    rlc_layout_segs(d);
    for (int i = 0; i < c; i++) *slot[i] = d.seg_dev[i];
    return d;
}

struct RlcAeDev {
    RlcAeDims d;
    RlcReplayDev rep;
    int n_agents;
    int clip_state;
    float tau;
    float amin[RLC_AE_MAX_A], amax[RLC_AE_MAX_A];   // per dimension (ae_network.py:194, :487)
    float *theta, *theta_t;             // [n_agents][Ppad]
    float *m_a, *v_a, *m_c, *v_c;       // the actor's Adam, the expert's Adam (both own W1, b1)
    float* pw;                          // [n_agents][4] beta powers {actor b1^t, b2^t, expert b1^t, b2^t}
    const float *actor_lr, *expert_lr;  // [n_agents]
    const float *smin, *smax;
    unsigned long long* noise_ctr;      // [n_agents] draws of the device's Philox stream so far (updates and acting)
    float *tap_q, *tap_y;               // [n_agents][RLC_MAX_BATCH]
    float* tap_anext;                   // [n_agents][RLC_MAX_BATCH][A]
    float* tap_sa;                      // [n_agents][B][n][A] the sampled actions (the kernel's working copy as well)
    float* tap_sq;                      // [n_agents][B][n] their Q
    float* tap_sel;                     // [n_agents][B][k] the selected sample indices, ascending
    float* tap_loss;                    // [n_agents][4]: the actor loss
    float *tap_ga, *tap_gc;             // [n_agents][Ppad] (rlc_ae_enable_grad_taps): actor / expert gradient
    float* scratch;
    long long scratch_stride;
};

size_t rlc_ae_scratch_floats(const RlcAeDims& d);
// null, or why these dimensions cannot run (the LDS the kernels need against 64 KiB)
const char* rlc_ae_refusal(const RlcAeDims& d);
// u_dev / eps_dev: the caller's draws [n_agents][n_updates][B][n] and [..][n][A], or both null: the device's Philox stream
int rlc_launch_ae_update(const RlcAeDev& dv, int first_agent, int n_agents, int n_updates, int source,
                         const long long* idx_dev, const float* u_dev, const float* eps_dev, int grad_taps, hipStream_t st);
// per state of agents [first_agent, first_agent + n): out_dev [n][A] = the mean of the mode of the largest alpha
// (sample 0) or one draw clipped to the action bounds (sample 1; u_dev [n], eps_dev [n][A] or both null)
int rlc_launch_ae_act(const RlcAeDev& dv, int first_agent, int n, const float* states_dev, const float* u_dev,
                      const float* eps_dev, int sample, float* out_dev, hipStream_t st, int* done_flag = nullptr,
                      int done_val = 0);
int rlc_launch_ae_qval(const RlcAeDev& dv, int agent, int n, const float* states_dev, const float* actions_dev,
                       float* out_dev, hipStream_t st);
