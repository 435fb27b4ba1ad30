// ac_generic.hip -- fused ActorCritic update, acting and Q-value kernels (any-shape VALU path).
//
// One workgroup per agent, n_updates sequential updates per launch; each update = sample_batch
// (utils/replaybuffer.py:32-37) + ActorCritic_Network_Manager.update_network (agents/ActorCritic.py:116-263):
//   a' from the ONLINE actor on s', before any step of this update (critic_update: 'mean' the greedy action, :141-146;
//        'sampled' one draw per row, :123-128; 'expected' n draws per row and the target Q averaged over them, :130-139),
//   y = r + gamma * Q_target(s', a') formed in float64 then cast (:163-167),
//   critic step: Adam(critic_lr) on MEAN (y - Q(s,a))^2 over W1 b1 Wq2 bq2 Wq3 bq3 (ac_network.py:91-92),
//   n raw samples per row on the weights AFTER that step, squashed, and their Q (:174-189),
//   actor step: Adam(actor_lr) on L = -(1/R) sum_rows sum_j w_j logN(raw_j; mu, sigma) over W1 b1 Wp2 bp2 Wmu bmu Wls
//        bls (ac_network.py:96-101, 322-334), Polyak on every tensor (:69-71).
// Network (ac_network.py:124-288): h1 = relu(x.W1 + b1), hp = relu(h1.Wp2 + bp2), mu = hp.Wmu + bmu (LINEAR: the
// density lives in pre-tanh space), sigma = exp(-20 + 11 (tanh(hp.Wls + bls) + 1)), raw = mu + sigma eps,
// action = tanh(raw) * action_max[d] (not clipped), greedy action = tanh(mu) * action_max[d],
// Q(s,a) = bq3 + Wq3 . relu(bq2 + h1.Wq2[:L1] + a.Wq2[L1:]).  The alpha head is in the blob and in Polyak only.
//
// THE UNIFIED WEIGHT FORM.  The three actor updates differ in the constants w_j and in R alone:
//   ll             R = B,     w_0 = q_0 - mean_j q_j, every other w_j = 0        (ActorCritic.py:203-218)
//   ll_update_all  R = B n,   w_j = q_j - mean_j q_j                             (:220-232)
//   cem            R = B k,   w_j = 1 on the k largest q_j, 0 elsewhere          (:235-254)
// w is a constant of the step, and the tanh-correction term of pi_actions_logprob (ac_network.py:242) has no parameter
// gradient, so with z = (raw - mu) / sigma: dL/dmu_d = -(1/R) sum_j w_j z_jd / sigma_d, dL/dsigma_d = -(1/R) sum_j w_j
// (z_jd^2 - 1) / sigma_d, summed over j ascending in float64 on the fp32 operands.  The actor therefore runs at B rows,
// not at the reference's B n or B k stacked rows.
// Q OF THE SAMPLES: the action enters Q at the second layer only: h1 and u = bq2 + h1.Wq2[:L1] are computed once per
// state.  ARITHMETIC ORDER (that of ae_generic.hip): pre = u[n], pre = fmaf(a_d, Wq2[L1+d][n], pre) for d ascending; four
// partial sums acc_c (c = n mod 4), each an ascending chain acc_c = fmaf(Wq3[n], max(pre, 0), acc_c); q = ((acc_0 + acc_1)
// + (acc_2 + acc_3)) + bq3.  The target Q of the next actions takes the same pass on the target weights.
// SELECTION (cem): a wave per row by rank counting: sample j is selected when fewer than k samples beat it, where i
// beats j if q_i > q_j, or q_i == q_j and i < j -- among equal values the lower index ranks first.  (The reference's
// argsort()[::-1] orders exact ties the other way round; that matters only between different actions with bit-equal Q.)
// The actor's second layer and both heads accumulate in float64 (each product of two floats is exact there): sigma
// multiplies the error of its pre-activation by 11 and enters the seeds as 1 / sigma.
// No atomics anywhere: one launch of K updates equals K launches of one bit for bit.
#include <limits.h>
#include <stdio.h>

#include "generic_blocks.h"
#include "ac_common.h"

namespace {

using namespace gen;

constexpr int kWaves = kThreads / 64;
// Philox counter words of the device's draws: apart from the replay sampler's (rlc_common.h) and from ActorExpert's
// (0xA..., 0xB...)
constexpr unsigned long long kTagUpdate = 0xC000000000000000ull;   // the n samples of the actor step
constexpr unsigned long long kTagNext = 0xD000000000000000ull;     // the next actions of the TD target
constexpr unsigned long long kTagAct = 0xE000000000000000ull;      // acting

__host__ __device__ inline size_t pad4z(size_t n) { return (n + 3) & ~(size_t)3; }
__host__ __device__ inline int pad4(int n) { return (n + 3) & ~3; }

__device__ __forceinline__ double wave_sum64d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Y[b,n] = act(sum_k X[b,k] W[k,n] + bias[n]) with the sum carried in float64 (ae_generic.hip's block): the correctly
// rounded value of the exact dot product (and of its tanh).  act: 0 none, 1 relu, 2 tanh.
__device__ inline void ac_dense_f64(const float* X, int ldx, int K, const float* W, const float* bias, int N, float* Y,
                                    int ldy, int B, int act) {
    const int rb = (B + kRows - 1) / kRows;
    for (int it = threadIdx.x; it < rb * N; it += kThreads) {
        const int n = it % N;
        const int b0 = (it / N) * kRows;
        double acc[kRows];
#pragma unroll
        for (int i = 0; i < kRows; i++) acc[i] = 0.0;
        for (int k = 0; k < K; k++) {
            const double w = (double)W[(size_t)k * N + n];
#pragma unroll
            for (int i = 0; i < kRows; i++) acc[i] = fma((double)X[(size_t)min(b0 + i, B - 1) * ldx + k], w, acc[i]);
        }
        const double bs = (double)bias[n];
#pragma unroll
        for (int i = 0; i < kRows; i++) {
            if (b0 + i < B) {
                double v = acc[i] + bs;
                if (act == 1) v = fmax(v, 0.0);
                else if (act == 2) v = tanh(v);
                Y[(size_t)(b0 + i) * ldy + n] = (float)v;
            }
        }
    }
}

// one row, one thread per output unit, the same float64 sum (the acting kernel)
__device__ inline void ac_row_f64(const float* W, const float* bias, const float* in, int K, int N, float* out, int act) {
    for (int n = threadIdx.x; n < N; n += kThreads) {
        double acc = 0.0;
        for (int k = 0; k < K; k++) acc = fma((double)in[k], (double)W[(size_t)k * N + n], acc);
        double v = acc + (double)bias[n];
        if (act == 1) v = fmax(v, 0.0);
        else if (act == 2) v = tanh(v);
        out[n] = (float)v;
    }
}

// ac_network.py:187: LOG_STD_MIN + 0.5 (LOG_STD_MAX - LOG_STD_MIN) (t + 1) with the bounds -20 and 2
__device__ __forceinline__ float ac_sigma(float t) { return (float)exp(-20.0 + 11.0 * ((double)t + 1.0)); }
// mvn.sample (ac_network.py:221): float64 on the fp32 operands, fed back as fp32
__device__ __forceinline__ float ac_raw(float mu, float sigma, float eps) {
    return (float)((double)mu + (double)sigma * (double)eps);
}
// tanh then the scale (ac_network.py:231-237); no clip
__device__ __forceinline__ float ac_squash(float raw, float amax) { return (float)tanh((double)raw) * amax; }

// the device's own normals of item `item`: RLC_AC_MAX_A of them
__device__ inline void ac_philox_draws(unsigned long long key, unsigned long long ctr, unsigned long long tag,
                                       unsigned long long item, int A, float* eps) {
    philox_normal2(philox4x32_10(key, ctr, tag | (item << 2)), eps[0], eps[1]);
    if (A > 2) philox_normal2(philox4x32_10(key, ctr, tag | (item << 2) | 1ull), eps[2], eps[3]);
    if (A > 4) philox_normal2(philox4x32_10(key, ctr, tag | (item << 2) | 2ull), eps[4], eps[5]);
}

// Wq3 [Lc] and the A action rows of Wq2 -> their zero-padded LDS rows
__device__ inline void ac_stage_q_weights(const float* P, int oW2, int oW3, int L1, int Lc, int A, int Lcp, float* sw3,
                                          float* sw2a) {
    for (int i = threadIdx.x; i < Lcp; i += kThreads) sw3[i] = i < Lc ? P[oW3 + i] : 0.0f;
    for (int i = threadIdx.x; i < A * Lcp; i += kThreads) {
        const int k = i / Lcp, n = i % Lcp;
        sw2a[i] = n < Lc ? P[oW2 + (size_t)(L1 + k) * Lc + n] : 0.0f;
    }
}

// q of one action on the row's u = bq2 + h1.Wq2[:L1] (the arithmetic order stated at the top of the file)
__device__ __forceinline__ float ac_q_of(const float (&a)[RLC_AC_MAX_A], const float* ub, const float* sw2a,
                                         const float* sw3, int A, int Lc, int Lcp, float bq3) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < Lcp; n0 += 4) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int n = n0 + c;
            float pre = n < Lc ? ub[n] : 0.0f;
#pragma unroll
            for (int j = 0; j < RLC_AC_MAX_A; j++)
                if (j < A) pre = fmaf(a[j], sw2a[j * Lcp + n], pre);
            acc[c] = fmaf(sw3[n], fmaxf(pre, 0.0f), acc[c]);
        }
    }
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + bq3;
}

struct CLds {
    double *r, *g;
    long long* idx;
    float *x, *x2, *a, *q, *y, *dq;
    int* pool;
    int* dups;
    float *sw3, *sw2a;
};

__host__ __device__ inline size_t clds_carve(const RlcAcDims& d, unsigned char* base, CLds* out) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        unsigned char* p = base ? base + off : nullptr;
        off += (bytes + 15) & ~(size_t)15;
        return p;
    };
    const size_t B = d.B, S = d.S, A = d.A, Lcp = pad4(d.Lc);
    CLds L;
    L.r = (double*)take(sizeof(double) * B);
    L.g = (double*)take(sizeof(double) * B);
    L.idx = (long long*)take(sizeof(long long) * RLC_MAX_BATCH);
    L.x = (float*)take(sizeof(float) * B * S);
    L.x2 = (float*)take(sizeof(float) * B * S);
    L.a = (float*)take(sizeof(float) * B * A);
    float** pb[] = {&L.q, &L.y, &L.dq};
    for (auto p : pb) *p = (float*)take(sizeof(float) * B);
    L.pool = (int*)take(sizeof(int) * 3 * RLC_MAX_BATCH);
    L.dups = (int*)take(sizeof(int) * 4);
    L.sw3 = (float*)take(sizeof(float) * Lcp);
    L.sw2a = (float*)take(sizeof(float) * A * Lcp);
    if (out) *out = L;
    return off;
}

__global__ __launch_bounds__(kThreads) void rlc_ac_update_kernel(RlcAcDev dv_arg, int first_agent, int n_updates,
                                                                 int source, const long long* host_idx,
                                                                 const float* eps_next_in, const float* eps_in,
                                                                 int grad_taps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the population view is read through gen::kernarg_view (generic_blocks.h), made opaque again by AC_PHASE() at the
    // start of every phase (dv_arg is the first argument: offset 0)
    const RlcAcDev* dvp;
#define AC_PHASE() (dvp = kernarg_view<RlcAcDev>())
#define dv (*dvp)
#define d (dvp->d)
    AC_PHASE();
    const int S = d.S, A = d.A, L1 = d.L1, La = d.La, Lc = d.Lc, ns = d.n, kk = d.k, B = d.B;
    const int cmode = dv.critic_mode, amode = dv.actor_mode;
    const int nn = cmode == RLC_AC_CRITIC_EXPECTED ? ns : 1;      // next actions per row
    const int nd = cmode == RLC_AC_CRITIC_MEAN ? 0 : nn;          // next draws per row
    const int Lcp = pad4(Lc);
    const int agent = first_agent + blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    CLds L;
    clds_carve(d, smem, &L);
    float* th = dv.theta + (size_t)agent * d.Ppad;
    float* tt = dv.theta_t + (size_t)agent * d.Ppad;
    float* pw = dv.pw + agent * 4;
    float* sc = dv.scratch + (size_t)agent * dv.scratch_stride;
    float* h1 = sc;  sc += pad4z((size_t)B * L1);
    float* hq = sc;  sc += pad4z((size_t)B * Lc);     // critic hidden layer, or u = bq2 + h1.Wq2[:L1]
    float* d2 = sc;  sc += pad4z((size_t)B * Lc);
    float* dh1 = sc; sc += pad4z((size_t)B * L1);
    float* hp = sc;  sc += pad4z((size_t)B * La);
    float* dhp = sc; sc += pad4z((size_t)B * La);
    float* tm = sc;  sc += pad4z((size_t)B * A);      // mu, then its backward seeds
    float* ts = sc;  sc += pad4z((size_t)B * A);      // tanh of the sigma head, then its backward seeds
    float* sg = sc;  sc += pad4z((size_t)B * A);      // sigma
    float* an = dv.tap_anext + (size_t)agent * B * nn * A;
    float* sr = dv.tap_raw + (size_t)agent * B * ns * A;
    float* sa = dv.tap_sa + (size_t)agent * B * ns * A;
    float* sq = dv.tap_sq + (size_t)agent * B * ns;
    float* wt = dv.tap_w + (size_t)agent * B * ns;
    float* tapga = grad_taps ? dv.tap_ga + (size_t)agent * d.Ppad : nullptr;
    float* tapgc = grad_taps ? dv.tap_gc + (size_t)agent * d.Ppad : nullptr;

    for (int u = 0; u < n_updates; u++) {
        // ---- sample + gather (utils/replaybuffer.py:32-37) ----
        AC_PHASE();
        const RlcRingMeta ring = dv.rep.ring[agent];
        rlc_pick_indices<kThreads>(dv.rep, agent, ring, source, B, host_idx, (size_t)blockIdx.x * n_updates + u, L.pool, L.idx,
                                   L.dups);
        AC_PHASE();
        for (int b = tid; b < B; b += kThreads) {
            const RlcRow w = rlc_locate_row(dv.rep, agent, ring, source, S, A, b, L.idx);
            L.r[b] = w.r; L.g[b] = w.g;
            for (int i = 0; i < S; i++) {
                L.x[b * S + i] = clip_state_val(w.s[i], dv.clip_state, dv.smin[i], dv.smax[i]);
                L.x2[b * S + i] = clip_state_val(w.s2[i], dv.clip_state, dv.smin[i], dv.smax[i]);
            }
            for (int j = 0; j < A; j++) L.a[b * A + j] = w.a[j];
        }
        __syncthreads();
        const unsigned long long key = dv.rep.seed[agent], nctr = dv.noise_ctr[agent];
        // ---- the ONLINE actor on s' (ActorCritic.py:123-146): mu, sigma ----
        AC_PHASE();
        blk_dense(L.x2, S, S, nullptr, 0, th + d.W1, th + d.b1, L1, h1, L1, B, 1);
        __syncthreads();
        ac_dense_f64(h1, L1, L1, th + d.Wp2, th + d.bp2, La, hp, La, B, 1);
        __syncthreads();
        ac_dense_f64(hp, La, La, th + d.Wmu, th + d.bmu, A, tm, A, B, 0);
        ac_dense_f64(hp, La, La, th + d.Wls, th + d.bls, A, ts, A, B, 2);
        __syncthreads();
        // ---- the TARGET trunk on s': h1, u = bq2 + h1.Wq2[:L1] ----
        AC_PHASE();
        for (int it = tid; it < B * A; it += kThreads) sg[it] = ac_sigma(ts[it]);
        blk_dense(L.x2, S, S, nullptr, 0, tt + d.W1, tt + d.b1, L1, h1, L1, B, 1);
        ac_stage_q_weights(tt, d.Wq2, d.Wq3, L1, Lc, A, Lcp, L.sw3, L.sw2a);
        __syncthreads();
        blk_dense(h1, L1, L1, nullptr, 0, tt + d.Wq2, tt + d.bq2, Lc, hq, Lc, B, 0);
        __syncthreads();
        // ---- the next actions and their target Q ----
        AC_PHASE();
        {
            const float bq3 = tt[d.bq3];
            float hi[RLC_AC_MAX_A];
#pragma unroll
            for (int j = 0; j < RLC_AC_MAX_A; j++) hi[j] = dv.amax[j];
            for (int it = tid; it < B * nn; it += kThreads) {
                const int b = it / nn;
                float eps[RLC_AC_MAX_A];
#pragma unroll
                for (int j = 0; j < RLC_AC_MAX_A; j++) eps[j] = 0.0f;
                if (nd > 0) {
                    if (eps_in) {
                        const size_t at = ((size_t)blockIdx.x * n_updates + u) * B * nn + it;
#pragma unroll
                        for (int j = 0; j < RLC_AC_MAX_A; j++)
                            if (j < A) eps[j] = eps_next_in[at * A + j];
                    } else {
                        ac_philox_draws(key, nctr, kTagNext, (unsigned long long)it, A, eps);
                    }
                }
                float a[RLC_AC_MAX_A];
#pragma unroll
                for (int j = 0; j < RLC_AC_MAX_A; j++) {
                    a[j] = 0.0f;
                    if (j < A) {
                        const float mu = tm[(size_t)b * A + j];
                        a[j] = ac_squash(nd > 0 ? ac_raw(mu, sg[(size_t)b * A + j], eps[j]) : mu, hi[j]);
                        an[(size_t)it * A + j] = a[j];
                    }
                }
                sq[it] = ac_q_of(a, hq + (size_t)b * Lc, L.sw2a, L.sw3, A, Lc, Lcp, bq3);   // nn <= ns: sq holds B * nn
            }
        }
        __syncthreads();
        AC_PHASE();
        for (int b = tid; b < B; b += kThreads) {
            // np.mean over the row's next actions (ActorCritic.py:139), then the float64 TD glue (:163-167), fed as fp32
            double s = 0.0;
            for (int j = 0; j < nn; j++) s += (double)sq[(size_t)b * nn + j];
            const float qn = (float)(s / (double)nn);
            const float y = (float)(L.r[b] + L.g[b] * (double)qn);
            L.y[b] = y;
            dv.tap_y[(size_t)agent * RLC_MAX_BATCH + b] = y;
        }
        // ---- critic step: online Q(s, a), MSE backward with the pre-step weights, Adam(critic_lr) ----
        blk_dense(L.x, S, S, nullptr, 0, th + d.W1, th + d.b1, L1, h1, L1, B, 1);
        __syncthreads();
        blk_dense(h1, L1, L1, L.a, A, th + d.Wq2, th + d.bq2, Lc, hq, Lc, B, 1);
        __syncthreads();
        blk_dense(hq, Lc, Lc, nullptr, 0, th + d.Wq3, th + d.bq3, 1, L.q, 1, B, 0);
        __syncthreads();
        AC_PHASE();
        for (int b = tid; b < B; b += kThreads) {
            dv.tap_q[(size_t)agent * RLC_MAX_BATCH + b] = L.q[b];
            L.dq[b] = 2.0f * (L.q[b] - L.y[b]) / (float)B;              // d mean((y-q)^2) / dq
        }
        __syncthreads();
        for (int it = tid; it < B * Lc; it += kThreads) {
            const int b = it / Lc, n = it % Lc;
            d2[it] = hq[it] > 0.0f ? L.dq[b] * th[d.Wq3 + n] : 0.0f;
        }
        __syncthreads();
        blk_dense_bwd_input(d2, Lc, th + d.Wq2, h1, L1, dh1, B);
        __syncthreads();
        AC_PHASE();
        {
            const AdamCtx c = {th, dv.m_c + (size_t)agent * d.Ppad, dv.v_c + (size_t)agent * d.Ppad,
                               adam_alpha(dv.critic_lr[agent], pw[2], pw[3]), tapgc};
            blk_dense_grad_adam(hq, Lc, Lc, nullptr, 0, L.dq, 1, B, c, d.Wq3, d.bq3);
            blk_dense_grad_adam(h1, L1, L1, L.a, A, d2, Lc, B, c, d.Wq2, d.bq2);
            AC_PHASE();
            blk_dense_grad_adam(L.x, S, S, nullptr, 0, dh1, L1, B, c, d.W1, d.b1);
        }
        __syncthreads();
        // ---- forward on s with the weights AFTER the critic step: the actor's heads, and u = bq2 + h1.Wq2[:L1] ----
        AC_PHASE();
        blk_dense(L.x, S, S, nullptr, 0, th + d.W1, th + d.b1, L1, h1, L1, B, 1);
        ac_stage_q_weights(th, d.Wq2, d.Wq3, L1, Lc, A, Lcp, L.sw3, L.sw2a);
        __syncthreads();
        ac_dense_f64(h1, L1, L1, th + d.Wp2, th + d.bp2, La, hp, La, B, 1);
        blk_dense(h1, L1, L1, nullptr, 0, th + d.Wq2, th + d.bq2, Lc, hq, Lc, B, 0);
        __syncthreads();
        AC_PHASE();
        ac_dense_f64(hp, La, La, th + d.Wmu, th + d.bmu, A, tm, A, B, 0);
        ac_dense_f64(hp, La, La, th + d.Wls, th + d.bls, A, ts, A, B, 2);
        __syncthreads();
        for (int it = tid; it < B * A; it += kThreads) sg[it] = ac_sigma(ts[it]);
        __syncthreads();
        // ---- the sampling pass (sample_action, ac_network.py:425-443) and Q of every sample ----
        AC_PHASE();
        {
            const float bq3 = th[d.bq3];
            float hi[RLC_AC_MAX_A];
#pragma unroll
            for (int j = 0; j < RLC_AC_MAX_A; j++) hi[j] = dv.amax[j];
            for (int it = tid; it < B * ns; it += kThreads) {
                const int b = it / ns;
                float eps[RLC_AC_MAX_A];
#pragma unroll
                for (int j = 0; j < RLC_AC_MAX_A; j++) eps[j] = 0.0f;
                if (eps_in) {
                    const size_t at = ((size_t)blockIdx.x * n_updates + u) * B * ns + it;
#pragma unroll
                    for (int j = 0; j < RLC_AC_MAX_A; j++)
                        if (j < A) eps[j] = eps_in[at * A + j];
                } else {
                    ac_philox_draws(key, nctr, kTagUpdate, (unsigned long long)it, A, eps);
                }
                float a[RLC_AC_MAX_A];
#pragma unroll
                for (int j = 0; j < RLC_AC_MAX_A; j++) {
                    a[j] = 0.0f;
                    if (j < A) {
                        const float raw = ac_raw(tm[(size_t)b * A + j], sg[(size_t)b * A + j], eps[j]);
                        a[j] = ac_squash(raw, hi[j]);
                        sr[(size_t)it * A + j] = raw;
                        sa[(size_t)it * A + j] = a[j];
                    }
                }
                sq[it] = ac_q_of(a, hq + (size_t)b * Lc, L.sw2a, L.sw3, A, Lc, Lcp, bq3);
            }
            if (tid == 0 && !eps_in) dv.noise_ctr[agent] = nctr + 1;
        }
        __syncthreads();
        // ---- the per-sample weights w_j: a wave per row ----
        AC_PHASE();
        for (int b = wave; b < B; b += kWaves) {
            const float* qrow = sq + (size_t)b * ns;
            float* wrow = wt + (size_t)b * ns;
            if (amode != RLC_AC_ACTOR_CEM) {
                // the baseline: the row's mean Q (ActorCritic.py:210, :223), float64 on the fp32 values
                double s = 0.0;
                for (int j = lane; j < ns; j += 64) s += (double)qrow[j];
                const double qbar = wave_sum64d(s) / (double)ns;
                for (int j = lane; j < ns; j += 64)
                    wrow[j] = (amode == RLC_AC_ACTOR_LL && j > 0) ? 0.0f : (float)((double)qrow[j] - qbar);
            } else {
                for (int c0 = 0; c0 < ns; c0 += 64) {
                    const int j = c0 + lane;
                    const bool valid = j < ns;
                    const float qj = qrow[valid ? j : ns - 1];
                    int rank = 0;
                    for (int i = 0; i < ns; i++) {
                        const float qi = qrow[i];
                        rank += (qi > qj || (qi == qj && i < j)) ? 1 : 0;
                    }
                    if (valid) wrow[j] = rank < kk ? 1.0f : 0.0f;      // the slot is the sample's own: j < n
                }
            }
        }
        __syncthreads();
        // ---- backward seeds of the two heads, summed over each row's samples (ascending index) ----
        AC_PHASE();
        {
            const double R = amode == RLC_AC_ACTOR_LL ? (double)B
                             : amode == RLC_AC_ACTOR_LL_ALL ? (double)B * (double)ns : (double)B * (double)kk;
            const double G = -1.0 / R;
            const int jn = amode == RLC_AC_ACTOR_LL ? 1 : ns;            // ll: only sample 0 carries weight
            for (int it = tid; it < B * A; it += kThreads) {
                const int b = it / A, j2 = it % A;
                const double mu = (double)tm[it], sd = (double)sg[it], tsig = (double)ts[it];
                double gmu = 0.0, gsd = 0.0;
                for (int j = 0; j < jn; j++) {
                    const double w = (double)wt[(size_t)b * ns + j];
                    const double z = ((double)sr[((size_t)b * ns + j) * A + j2] - mu) / sd;
                    gmu += w * z / sd;
                    gsd += w * (z * z - 1.0) / sd;
                }
                tm[it] = (float)(G * gmu);
                ts[it] = (float)(G * gsd * (sd * 11.0 * (1.0 - tsig * tsig)));
            }
        }
        __syncthreads();
        // ---- actor backward: the two heads into hp, then Wp2 into h1 ----
        AC_PHASE();
        blk_dense_bwd_input_ex(tm, A, th + d.Wmu, hp, La, dhp, B, false);
        __syncthreads();
        blk_dense_bwd_input_ex(ts, A, th + d.Wls, hp, La, dhp, B, true);
        __syncthreads();
        blk_dense_bwd_input(dhp, La, th + d.Wp2, h1, L1, dh1, B);
        __syncthreads();
        // ---- gradients + Adam(actor_lr) over the actor's eight tensors; the alpha head has no gradient ----
        AC_PHASE();
        {
            const AdamCtx c = {th, dv.m_a + (size_t)agent * d.Ppad, dv.v_a + (size_t)agent * d.Ppad,
                               adam_alpha(dv.actor_lr[agent], pw[0], pw[1]), tapga};
            blk_dense_grad_adam(hp, La, La, nullptr, 0, tm, A, B, c, d.Wmu, d.bmu);
            blk_dense_grad_adam(hp, La, La, nullptr, 0, ts, A, B, c, d.Wls, d.bls);
            AC_PHASE();
            blk_dense_grad_adam(h1, L1, L1, nullptr, 0, dhp, La, B, c, d.Wp2, d.bp2);
            blk_dense_grad_adam(L.x, S, S, nullptr, 0, dh1, L1, B, c, d.W1, d.b1);
        }
        __syncthreads();
        // ---- Polyak on every tensor, the alpha head included (ac_network.py:69-71) ----
        AC_PHASE();
        if (tid == 0) { pw[0] *= 0.9f; pw[1] *= 0.999f; pw[2] *= 0.9f; pw[3] *= 0.999f; }
        for (int p = tid; p < d.Pdev; p += kThreads) {
            const float t = tt[p];
            tt[p] = t + dv.tau * (th[p] - t);
        }
        __syncthreads();
    }
#undef AC_PHASE
#undef dv
#undef d
}

// LDS of the one-row kernels: x [S + A], h1 [L1], hp [La], hq [Lc], the two heads' rows, reduction words
struct CRowLds { float *x, *h1, *hp, *hq, *tm, *ts, *redv; };
__host__ __device__ inline size_t crow_carve(const RlcAcDims& d, float* base, CRowLds* out) {
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 3) & ~(size_t)3; return p; };
    CRowLds L;
    L.x = take(d.S + d.A); L.h1 = take(d.L1); L.hp = take(d.La); L.hq = take(d.Lc);
    L.tm = take(d.A); L.ts = take(d.A);
    L.redv = take(kWaves + 8);
    if (out) *out = L;
    return off * sizeof(float);
}

// predict_action (sample 0; ac_network.py:449-472) or one draw of sample_action (sample 1; :425-443, is_single_sample)
// of the ONLINE network for one state per agent.  done_flag (or null): a word in host-visible memory that receives
// done_val once the launch's outputs are stored (rlc_ac_act_queue; see rlc_ddpg_act_kernel)
__global__ __launch_bounds__(kThreads) void rlc_ac_act_kernel(RlcAcDev dv, int first_agent, const float* states,
                                                              const float* eps_in, int sample, float* out,
                                                              int* done_flag, int done_val) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RlcAcDims& d = dv.d;
    const int S = d.S, A = d.A;
    const int agent = first_agent + blockIdx.x, tid = threadIdx.x;
    CRowLds L;
    crow_carve(d, (float*)smem, &L);
    const float* th = dv.theta + (size_t)agent * d.Ppad;
    for (int i = tid; i < S; i += kThreads)
        L.x[i] = clip_state_val(states[(size_t)blockIdx.x * S + i], dv.clip_state, dv.smin[i], dv.smax[i]);
    __syncthreads();
    rlc_hidden_forward_row(th + d.W1, 0, th + d.b1, L.x, S, d.L1, L.h1, true);
    __syncthreads();
    ac_row_f64(th + d.Wp2, th + d.bp2, L.h1, d.L1, d.La, L.hp, 1);
    __syncthreads();
    ac_row_f64(th + d.Wmu, th + d.bmu, L.hp, d.La, A, L.tm, 0);
    ac_row_f64(th + d.Wls, th + d.bls, L.hp, d.La, A, L.ts, 2);
    __syncthreads();
    if (tid == 0) {
        if (!sample) {
            for (int j = 0; j < A; j++) out[(size_t)blockIdx.x * A + j] = ac_squash(L.tm[j], dv.amax[j]);
        } else {
            float eps[RLC_AC_MAX_A] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (eps_in) {
                for (int j = 0; j < A; j++) eps[j] = eps_in[(size_t)blockIdx.x * A + j];
            } else {
                const unsigned long long nctr = dv.noise_ctr[agent];
                ac_philox_draws(dv.rep.seed[agent], nctr, kTagAct, 0ull, A, eps);
                dv.noise_ctr[agent] = nctr + 1;
            }
            for (int j = 0; j < A; j++)
                out[(size_t)blockIdx.x * A + j] = ac_squash(ac_raw(L.tm[j], ac_sigma(L.ts[j]), eps[j]), dv.amax[j]);
        }
        if (done_flag) {
            __threadfence_system();                     // the output stores first
            __hip_atomic_store(done_flag, done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// Q(s,a) rows on one agent's online network (getQFunction, ac_network.py:480-483).  One workgroup per row; the sum over
// the critic layer's units is split over the threads (fixed order: deterministic).
__global__ __launch_bounds__(kThreads) void rlc_ac_qval_kernel(RlcAcDev dv, int agent, const float* states,
                                                               const float* actions, float* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RlcAcDims& d = dv.d;
    const int S = d.S, A = d.A, L1 = d.L1, Lc = d.Lc;
    const int tid = threadIdx.x, row = blockIdx.x;
    CRowLds L;
    crow_carve(d, (float*)smem, &L);
    const float* th = dv.theta + (size_t)agent * d.Ppad;
    for (int i = tid; i < S; i += kThreads)
        L.x[i] = clip_state_val(states[(size_t)row * S + i], dv.clip_state, dv.smin[i], dv.smax[i]);
    for (int k = tid; k < A; k += kThreads) L.x[S + k] = actions[(size_t)row * A + k];
    __syncthreads();
    rlc_hidden_forward_row(th + d.W1, 0, th + d.b1, L.x, S, L1, L.h1, true);
    __syncthreads();
    rlc_hidden_forward_row(th + d.Wq2, 0, th + d.bq2, L.h1, L1, Lc, L.hq, false);
    __syncthreads();
    float part = 0.0f;
    for (int n = tid; n < Lc; n += kThreads) {
        float pre = L.hq[n];
        for (int k = 0; k < A; k++) pre = fmaf(L.x[S + k], th[d.Wq2 + (size_t)(L1 + k) * Lc + n], pre);
        part = fmaf(th[d.Wq3 + n], fmaxf(pre, 0.0f), part);
    }
    const float q = blk_sum(part, L.redv);
    if (tid == 0) out[row] = q + th[d.bq3];
}

}  // namespace

size_t rlc_ac_scratch_floats(const RlcAcDims& d) {
    const size_t B = d.B;
    return 2 * pad4z(B * d.L1) + 2 * pad4z(B * d.Lc) + 2 * pad4z(B * d.La) + 3 * pad4z(B * d.A);
}

const char* rlc_ac_refusal(const RlcAcDims& d) {
    static thread_local char msg[200];
    const size_t up = clds_carve(d, nullptr, nullptr), row = crow_carve(d, nullptr, nullptr);
    const size_t need = up > row ? up : row;
    if (need <= 64 * 1024) return nullptr;
    snprintf(msg, sizeof(msg), "state_dim %d, layer widths %d / %d / %d at batch_size %d need %zu B of LDS (> 65536)", d.S,
             d.L1, d.La, d.Lc, d.B, need);
    return msg;
}

int rlc_launch_ac_update(const RlcAcDev& dv, int first_agent, int n_agents, int n_updates, int source,
                         const long long* idx_dev, const float* eps_next_dev, const float* eps_dev, int grad_taps,
                         hipStream_t st) {
    const size_t lds = clds_carve(dv.d, nullptr, nullptr);
    RLC_REQUIRE(lds <= 64 * 1024, "ActorCritic kernel needs %zu B of LDS (> 64 KiB)", lds);
    const bool wants_next = rlc_ac_next_draws(dv.critic_mode, dv.d.n) > 0;
    RLC_REQUIRE((eps_next_dev != nullptr) == (eps_dev != nullptr && wants_next),
                "eps_next and eps: both null (the device's draws), or eps with eps_next exactly when critic_update draws");
    hipLaunchKernelGGL(rlc_ac_update_kernel, dim3(n_agents), dim3(kThreads), lds, st, dv, first_agent, n_updates, source,
                       idx_dev, eps_next_dev, eps_dev, grad_taps);
    RLC_HIP(hipGetLastError());
    return 0;
}

int rlc_launch_ac_act(const RlcAcDev& dv, int first_agent, int n, const float* states_dev, const float* eps_dev,
                      int sample, float* out_dev, hipStream_t st, int* done_flag, int done_val) {
    const size_t lds = crow_carve(dv.d, nullptr, nullptr);
    RLC_REQUIRE(lds <= 64 * 1024, "ActorCritic acting kernel needs %zu B of LDS (> 64 KiB)", lds);
    RLC_REQUIRE(done_flag == nullptr || n == 1, "a completion flag needs a one-workgroup acting launch");
    hipLaunchKernelGGL(rlc_ac_act_kernel, dim3(n), dim3(kThreads), lds, st, dv, first_agent, states_dev, eps_dev, sample,
                       out_dev, done_flag, done_val);
    RLC_HIP(hipGetLastError());
    return 0;
}

int rlc_launch_ac_qval(const RlcAcDev& dv, int agent, int n, const float* states_dev, const float* actions_dev,
                       float* out_dev, hipStream_t st) {
    const size_t lds = crow_carve(dv.d, nullptr, nullptr);
    RLC_REQUIRE(lds <= 64 * 1024, "ActorCritic Q-value kernel needs %zu B of LDS (> 64 KiB)", lds);
    hipLaunchKernelGGL(rlc_ac_qval_kernel, dim3(n), dim3(kThreads), lds, st, dv, agent, states_dev, actions_dev, out_dev);
    RLC_HIP(hipGetLastError());
    return 0;
}
