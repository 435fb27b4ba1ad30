// ac_common.h -- geometry and device view of the ActorCritic population.
// Blob = variable creation order (agents/network/ac_network.py:124-288):
//   W1[S,L1] b1 | Wp2[L1,La] bp2 | Wmu[La,A] bmu | Wls[La,A] bls | Wal[La,1] bal | Wq2[L1+A,Lc] bq2 | Wq3[Lc] bq3
// (num_modal = 1, ac_network.py:175; the action rows are LAST in Wq2, :271).  The alpha head (Wal, bal) is carried in
// the blob and in Polyak and is never evaluated: no loss reaches it, so TF's minimize gives it no moments.
// Device layout pads every tensor to 64 floats, always row-major (the agent runs on the any-shape kernel only); the
// ABI blob is compact.
#pragma once
#include "rlc_common.h"

#define RLC_AC_MAX_A 6
#define RLC_AC_MAX_SAMPLES 1024
#define RLC_AC_SEG 14

// critic_update (agents/ActorCritic.py:123-146): the next action of the TD target
enum { RLC_AC_CRITIC_MEAN = 0, RLC_AC_CRITIC_SAMPLED = 1, RLC_AC_CRITIC_EXPECTED = 2 };
// actor_update (agents/ActorCritic.py:203-254)
enum { RLC_AC_ACTOR_LL = 0, RLC_AC_ACTOR_LL_ALL = 1, RLC_AC_ACTOR_CEM = 2 };

struct RlcAcDims {
    int S, A, L1, La, Lc, n, k, B;      // n = num_samples, k = top_k = int(num_samples * rho) (cem only)
    int blocked;                        // always 0 (the field the shared segment code reads)
    int W1, b1, Wp2, bp2, Wmu, bmu, Wls, bls, Wal, bal, Wq2, bq2, Wq3, bq3;
    int P, Pdev, Ppad, nseg;
    int seg_len[RLC_AC_SEG], seg_compact[RLC_AC_SEG], seg_dev[RLC_AC_SEG];
    int seg_rows[RLC_AC_SEG], seg_cols[RLC_AC_SEG], seg_h[RLC_AC_SEG];
    char seg_big[RLC_AC_SEG];
};

inline RlcAcDims rlc_ac_make_dims(int S, int A, int L1, int La, int Lc, int n, int k, int B) {
    RlcAcDims d;
    d.S = S; d.A = A; d.L1 = L1; d.La = La; d.Lc = Lc; d.n = n; d.k = k; d.B = B; d.blocked = 0;
    int c = 0;
    int* slot[RLC_AC_SEG];
    auto seg = [&](int* where, int r, int cols) {
        slot[c] = where; d.seg_rows[c] = r; d.seg_cols[c] = cols; d.seg_h[c] = r; d.seg_big[c] = 0; c++;
    };
    seg(&d.W1, S, L1); seg(&d.b1, 1, L1);
    seg(&d.Wp2, L1, La); seg(&d.bp2, 1, La);
    seg(&d.Wmu, La, A); seg(&d.bmu, 1, A);
    seg(&d.Wls, La, A); seg(&d.bls, 1, A);
    seg(&d.Wal, La, 1); seg(&d.bal, 1, 1);
    seg(&d.Wq2, L1 + A, Lc); seg(&d.bq2, 1, Lc);
    seg(&d.Wq3, Lc, 1); seg(&d.bq3, 1, 1);
    d.nseg = c;
    rlc_layout_segs(d);
    for (int i = 0; i < c; i++) *slot[i] = d.seg_dev[i];
    return d;
}

// next actions per row of the TD target: 1 (mean, sampled) or n (expected); draws per row: 0, 1 or n
inline int rlc_ac_next_actions(int critic_mode, int n) { return critic_mode == RLC_AC_CRITIC_EXPECTED ? n : 1; }
inline int rlc_ac_next_draws(int critic_mode, int n) {
    return critic_mode == RLC_AC_CRITIC_MEAN ? 0 : critic_mode == RLC_AC_CRITIC_SAMPLED ? 1 : n;
}

struct RlcAcDev {
    RlcAcDims d;
    RlcReplayDev rep;
    int n_agents;
    int clip_state;
    int critic_mode, actor_mode;
    float tau;
    float amax[RLC_AC_MAX_A];           // per dimension: the scale of the squashed action (ac_network.py:236-237)
    float *theta, *theta_t;             // [n_agents][Ppad]
    float *m_a, *v_a, *m_c, *v_c;       // the actor's Adam, the critic's Adam (both own W1, b1)
    float* pw;                          // [n_agents][4] beta powers {actor b1^t, b2^t, critic b1^t, b2^t}
    const float *actor_lr, *critic_lr;  // [n_agents]
    const float *smin, *smax;
    unsigned long long* noise_ctr;      // [n_agents] draws of the device's Philox stream so far (updates and acting)
    float *tap_q, *tap_y;               // [n_agents][RLC_MAX_BATCH]
    float* tap_anext;                   // [n_agents][B][n_next_actions][A] the next actions of the TD target
    float* tap_raw;                     // [n_agents][B][n][A] the raw (pre-tanh) samples
    float* tap_sa;                      // [n_agents][B][n][A] the squashed samples
    float* tap_sq;                      // [n_agents][B][n] their Q (before that: the target Q of the next actions)
    float* tap_w;                       // [n_agents][B][n] the per-sample weights of the actor loss
    float *tap_ga, *tap_gc;             // [n_agents][Ppad] (rlc_ac_enable_grad_taps): actor / critic gradient
    float* scratch;
    long long scratch_stride;
};

size_t rlc_ac_scratch_floats(const RlcAcDims& d);
// null, or why these dimensions cannot run (the LDS the kernels need against 64 KiB)
const char* rlc_ac_refusal(const RlcAcDims& d);
// eps_next_dev [n_agents][n_updates][B][n_next_draws][A] and eps_dev [..][B][n][A]: the caller's standard normals
// (eps_next_dev null when critic_update is 'mean'), or both null: the device's Philox stream
int rlc_launch_ac_update(const RlcAcDev& dv, int first_agent, int n_agents, int n_updates, int source,
                         const long long* idx_dev, const float* eps_next_dev, const float* eps_dev, int grad_taps,
                         hipStream_t st);
// per state of agents [first_agent, first_agent + n): out_dev [n][A] = tanh(mu) * action_max (sample 0) or
// tanh(mu + sigma * eps) * action_max (sample 1; eps_dev [n][A], or null: the device's stream)
int rlc_launch_ac_act(const RlcAcDev& dv, int first_agent, int n, const float* states_dev, const float* eps_dev,
                      int sample, float* out_dev, hipStream_t st, int* done_flag = nullptr, int done_val = 0);
int rlc_launch_ac_qval(const RlcAcDev& dv, int agent, int n, const float* states_dev, const float* actions_dev,
                       float* out_dev, hipStream_t st);
