// ae_generic.hip -- fused ActorExpert update, acting and Q-value kernels (any-shape VALU path).
//
// One workgroup per agent, n_updates sequential updates per launch; each update = sample_batch
// (utils/replaybuffer.py:32-37) + ActorExpert_Network_Manager.update_network (agents/ActorExpert.py:116-185):
//   a' = the mean of the mode with the largest alpha on s', ONLINE network (predict_action, ae_network.py:409-435; the
//        lowest index among equal alphas, as np.argmax), y = r + gamma * Q_target(s', a') formed in float64 then cast,
//   expert step: Adam(expert_lr) on MEAN (y - Q(s,a))^2 over W1 b1 Wq2 bq2 Wq3 bq3 (ae_network.py:108-109),
//   n sampled actions per row from the mixture on the weights AFTER that step (sample_action, :461-496), their Q,
//   the k largest per row (ActorExpert.py:177), actor step: Adam(actor_lr) on
//        L = -(1 / (B k)) sum_rows sum_selected log clip(sum_m alpha_m prod_d N(a_d; mean_md, sigma_md), 1e-30, 1e30)
//   over W1 b1 Wa2 ba2 Wm bm Ws bs Wal bal (get_lossfunc, :262-278), Polyak on every tensor (:84-86).
// Network (ae_network.py:138-229): h1 = relu(x.W1 + b1), ha = relu(h1.Wa2 + ba2), mean = tanh(ha.Wm + bm) * action_max[d],
// sigma = exp(-20 + 11 (tanh(ha.Ws + bs) + 1)), alpha = softmax_M(tanh(ha.Wal + bal)),
// Q(s,a) = bq3 + Wq3 . relu(bq2 + h1.Wq2[:L1] + a.Wq2[L1:]).
//
// TWO RESTRUCTURINGS against the reference, which pushes B*n rows through the Q network and B*k rows through the actor:
//  1. the action enters Q at the second layer only: h1 and u = bq2 + h1.Wq2[:L1] are computed once per state, a sample
//     costs q_j = (sum_n Wq3[n] relu(u[n] + sum_d a_jd Wq2[L1+d][n])) + bq3 (the node pass of optq_generic.hip).
//     ARITHMETIC ORDER: pre = u[n], pre = fmaf(a_d, Wq2[L1+d][n], pre) for d ascending; four partial sums acc_c
//     (c = n mod 4), each an ascending chain acc_c = fmaf(Wq3[n], max(pre, 0), acc_c); q = ((acc_0 + acc_1) + (acc_2 +
//     acc_3)) + bq3.
//  2. the actor runs at B rows: the loss of a row's k selected actions shares the row's (alpha, mean, sigma), so the
//     backward seeds dL/dmean, dL/dsigma, dL/dalpha are summed over the selected actions (ascending sample index) before
//     the dense backward.
// SELECTION: a wave per row by rank counting: sample j is selected when fewer than k samples beat it, where i beats j if
// q_i > q_j, or q_i == q_j and i < j -- among equal values the lower index ranks first.  (The reference's argsort()[::-1]
// orders exact ties the other way round; that matters only between DIFFERENT actions with bit-equal Q.  Samples clipped
// to the same bound are the same action.)  The selected indices come out in ascending order by ballot / prefix count.
// DENSITY: evaluated in log space in float64 on the fp32 (mean, sigma, alpha, action): log c_m = log alpha_m + sum_d
// (-log sqrt(2 pi) - log sigma_md - z^2 / 2), log p by log-sum-exp; sigma reaches e^-20, so the linear-space product
// spans 1e-35 .. 1e+35 per dimension and the reference's fp32 product over- or underflows where this form does not.
// tf.clip_by_value passes no gradient outside its bounds: a sample whose log p lies outside [log 1e-30, log 1e30] gets
// responsibility 0 for every mode, and its loss term is the bound.
// The actor's second layer and the three heads accumulate in float64 (each product of two floats is exact there):
// sigma multiplies the error of its pre-activation by 11 and enters the seeds as 1 / sigma^2.
// No atomics anywhere: one launch of K updates equals K launches of one bit for bit.
#include <limits.h>
#include <stdio.h>

#include "generic_blocks.h"
#include "ae_common.h"

namespace {

using namespace gen;

constexpr int kWaves = kThreads / 64;
constexpr double kLogClipLo = -69.07755278982137;     // log 1e-30
constexpr double kLogClipHi = 69.07755278982137;      // log 1e30
constexpr double kHalfLog2Pi = 0.9189385332046727;
constexpr unsigned long long kTagUpdate = 0xA000000000000000ull;   // Philox counter words of the sampled actions:
constexpr unsigned long long kTagAct = 0xB000000000000000ull;      // apart from the replay sampler's (rlc_common.h)

__host__ __device__ inline size_t pad4z(size_t n) { return (n + 3) & ~(size_t)3; }
__host__ __device__ inline int pad4(int n) { return (n + 3) & ~3; }

__device__ __forceinline__ double wave_sum64d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Y[b,n] = act(sum_k X[b,k] W[k,n] + bias[n]) with the sum carried in float64 (wf_generic.hip's block): the correctly
// rounded value of the exact dot product (and of its tanh).  act: 0 none, 1 relu, 2 tanh.
__device__ inline void ae_dense_f64(const float* X, int ldx, int K, const float* W, const float* bias, int N, float* Y,
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
__device__ inline void ae_row_f64(const float* W, const float* bias, const float* in, int K, int N, float* out, int act) {
    for (int n = threadIdx.x; n < N; n += kThreads) {
        double acc = 0.0;
        for (int k = 0; k < K; k++) acc = fma((double)in[k], (double)W[(size_t)k * N + n], acc);
        double v = acc + (double)bias[n];
        if (act == 1) v = fmax(v, 0.0);
        else if (act == 2) v = tanh(v);
        out[n] = (float)v;
    }
}

// alpha [M] = softmax of the tanh outputs t [M] (ae_network.py:206-211), float64 on the fp32 inputs, rounded once
__device__ inline void ae_alpha_row(const float* t, int M, float* alpha) {
    double mx = (double)t[0];
    for (int m = 1; m < M; m++) mx = fmax(mx, (double)t[m]);
    double s = 0.0;
    for (int m = 0; m < M; m++) s += exp((double)t[m] - mx);
    for (int m = 0; m < M; m++) alpha[m] = (float)(exp((double)t[m] - mx) / s);     // (no register array: M is a run-time size)
}
__device__ __forceinline__ float ae_sigma(float t) { return (float)exp(-20.0 + 11.0 * ((double)t + 1.0)); }

// the lowest index of the largest alpha (np.argmax, ae_network.py:425)
__device__ inline int ae_best_mode(const float* alpha, int M) {
    int best = 0;
    for (int m = 1; m < M; m++)
        if (alpha[m] > alpha[best]) best = m;
    return best;
}

// RandomState.choice(M, p=alpha) for the uniform draw u: the number of cdf entries <= u, cdf = cumsum(alpha) / its last
// element, in float64 (searchsorted(side='right'))
__device__ inline int ae_mode_of(const float* alpha, int M, float u) {
    double tot = 0.0;
    for (int m = 0; m < M; m++) tot += (double)alpha[m];
    double run = 0.0;
    int mode = 0;
    for (int m = 0; m < M; m++) {
        run += (double)alpha[m];
        if (run / tot <= (double)u) mode++;
    }
    return min(mode, M - 1);
}

// rng.normal(mean, sigma) then np.clip (ae_network.py:487): float64 on the fp32 operands, fed back as fp32
__device__ __forceinline__ float ae_draw(float mean, float sigma, float eps, float lo, float hi) {
    const double a = (double)mean + (double)sigma * (double)eps;
    return (float)fmin(fmax(a, (double)lo), (double)hi);
}

// the device's own draws of item `item`: one uniform and RLC_AE_MAX_A normals
__device__ inline void ae_philox_draws(unsigned long long key, unsigned long long ctr, unsigned long long tag,
                                       unsigned long long item, int A, float& u, float* eps) {
    const Philox4 p0 = philox4x32_10(key, ctr, tag | (item << 2));
    u = (float)(p0.z >> 8) * (1.0f / 16777216.0f);                       // [0,1)
    philox_normal2(p0, eps[0], eps[1]);
    if (A > 2) philox_normal2(philox4x32_10(key, ctr, tag | (item << 2) | 1ull), eps[2], eps[3]);
    if (A > 4) philox_normal2(philox4x32_10(key, ctr, tag | (item << 2) | 2ull), eps[4], eps[5]);
}

// Wq3 [Le] and the A action rows of Wq2 -> their zero-padded LDS rows
__device__ inline void ae_stage_q_weights(const float* P, int oW2, int oW3, int L1, int Le, int A, int Lep, float* sw3,
                                          float* sw2a) {
    for (int i = threadIdx.x; i < Lep; i += kThreads) sw3[i] = i < Le ? P[oW3 + i] : 0.0f;
    for (int i = threadIdx.x; i < A * Lep; i += kThreads) {
        const int k = i / Lep, n = i % Lep;
        sw2a[i] = n < Le ? P[oW2 + (size_t)(L1 + k) * Le + n] : 0.0f;
    }
}

struct ALds {
    double *r, *g, *rowloss;
    long long* idx;
    float *x, *x2, *a, *a2, *q, *y, *dq;
    int* pool;
    int* dups;
    int* rowcnt;
    float *sw3, *sw2a;
};

__host__ __device__ inline size_t alds_carve(const RlcAeDims& d, unsigned char* base, ALds* out) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        unsigned char* p = base ? base + off : nullptr;
        off += (bytes + 15) & ~(size_t)15;
        return p;
    };
    const size_t B = d.B, S = d.S, A = d.A, Lep = pad4(d.Le);
    ALds L;
    L.r = (double*)take(sizeof(double) * B);
    L.g = (double*)take(sizeof(double) * B);
    L.rowloss = (double*)take(sizeof(double) * B);
    L.idx = (long long*)take(sizeof(long long) * RLC_MAX_BATCH);
    L.x = (float*)take(sizeof(float) * B * S);
    L.x2 = (float*)take(sizeof(float) * B * S);
    L.a = (float*)take(sizeof(float) * B * A);
    L.a2 = (float*)take(sizeof(float) * B * A);
    float** pb[] = {&L.q, &L.y, &L.dq};
    for (auto p : pb) *p = (float*)take(sizeof(float) * B);
    L.pool = (int*)take(sizeof(int) * 3 * RLC_MAX_BATCH);
    L.dups = (int*)take(sizeof(int) * 4);
    L.rowcnt = (int*)take(sizeof(int) * B);
    L.sw3 = (float*)take(sizeof(float) * Lep);
    L.sw2a = (float*)take(sizeof(float) * A * Lep);
    if (out) *out = L;
    return off;
}

__global__ __launch_bounds__(kThreads) void rlc_ae_update_kernel(RlcAeDev dv_arg, int first_agent, int n_updates,
                                                                 int source, const long long* host_idx,
                                                                 const float* u_in, const float* eps_in, int grad_taps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the population view is read through gen::kernarg_view (generic_blocks.h), made opaque again by AE_PHASE() at the
    // start of every phase (dv_arg is the first argument: offset 0)
    const RlcAeDev* dvp;
#define AE_PHASE() (dvp = kernarg_view<RlcAeDev>())
#define dv (*dvp)
#define d (dvp->d)
    AE_PHASE();
    const int S = d.S, A = d.A, L1 = d.L1, La = d.La, Le = d.Le, M = d.M, ns = d.n, kk = d.k, B = d.B;
    const int MA = M * A, Lep = pad4(Le);
    const int agent = first_agent + blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    ALds L;
    alds_carve(d, smem, &L);
    float* th = dv.theta + (size_t)agent * d.Ppad;
    float* tt = dv.theta_t + (size_t)agent * d.Ppad;
    float* pw = dv.pw + agent * 4;
    float* sc = dv.scratch + (size_t)agent * dv.scratch_stride;
    float* h1 = sc;  sc += pad4z((size_t)B * L1);
    float* hq = sc;  sc += pad4z((size_t)B * Le);     // expert hidden layer, then u = bq2 + h1.Wq2[:L1]
    float* d2 = sc;  sc += pad4z((size_t)B * Le);
    float* dh1 = sc; sc += pad4z((size_t)B * L1);
    float* ha = sc;  sc += pad4z((size_t)B * La);
    float* dha = sc; sc += pad4z((size_t)B * La);
    float* tm = sc;  sc += pad4z((size_t)B * MA);     // tanh of the mean head, then its backward seeds
    float* ts = sc;  sc += pad4z((size_t)B * MA);     // tanh of the sigma head, then its backward seeds
    float* sg = sc;  sc += pad4z((size_t)B * MA);     // sigma
    float* tl = sc;  sc += pad4z((size_t)B * M);      // tanh of the alpha head, then its backward seeds
    float* al = sc;  sc += pad4z((size_t)B * M);      // alpha
    float* rs = sc;  sc += pad4z((size_t)B * kk * M); // responsibilities of the selected samples [B][k][M]
    float* sa = dv.tap_sa + (size_t)agent * B * ns * A;
    float* sq = dv.tap_sq + (size_t)agent * B * ns;
    float* sel = dv.tap_sel + (size_t)agent * B * kk;
    float* tapga = grad_taps ? dv.tap_ga + (size_t)agent * d.Ppad : nullptr;
    float* tapgc = grad_taps ? dv.tap_gc + (size_t)agent * d.Ppad : nullptr;

    for (int u = 0; u < n_updates; u++) {
        // ---- sample + gather (utils/replaybuffer.py:32-37) ----
        AE_PHASE();
        const RlcRingMeta ring = dv.rep.ring[agent];
        rlc_pick_indices<kThreads>(dv.rep, agent, ring, source, B, host_idx, (size_t)blockIdx.x * n_updates + u, L.pool, L.idx,
                                   L.dups);
        AE_PHASE();
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
        // ---- a' = the mean of the largest-alpha mode on s', ONLINE network (ActorExpert.py:138) ----
        AE_PHASE();
        blk_dense(L.x2, S, S, nullptr, 0, th + d.W1, th + d.b1, L1, h1, L1, B, 1);
        __syncthreads();
        ae_dense_f64(h1, L1, L1, th + d.Wa2, th + d.ba2, La, ha, La, B, 1);
        __syncthreads();
        ae_dense_f64(ha, La, La, th + d.Wm, th + d.bm, MA, tm, MA, B, 2);
        ae_dense_f64(ha, La, La, th + d.Wal, th + d.bal, M, tl, M, B, 2);
        __syncthreads();
        AE_PHASE();
        for (int b = tid; b < B; b += kThreads) {
            float* alpha = al + (size_t)b * M;
            ae_alpha_row(tl + (size_t)b * M, M, alpha);
            const int best = ae_best_mode(alpha, M);
            for (int j = 0; j < A; j++) {
                const float an = tm[(size_t)b * MA + best * A + j] * dv.amax[j];
                L.a2[b * A + j] = an;
                dv.tap_anext[((size_t)agent * RLC_MAX_BATCH + b) * A + j] = an;
            }
        }
        __syncthreads();
        // ---- y = r + gamma * Q_target(s', a') (ActorExpert.py:148-154) ----
        AE_PHASE();
        blk_dense(L.x2, S, S, nullptr, 0, tt + d.W1, tt + d.b1, L1, h1, L1, B, 1);
        __syncthreads();
        blk_dense(h1, L1, L1, L.a2, A, tt + d.Wq2, tt + d.bq2, Le, hq, Le, B, 1);
        __syncthreads();
        blk_dense(hq, Le, Le, nullptr, 0, tt + d.Wq3, tt + d.bq3, 1, L.q, 1, B, 0);
        __syncthreads();
        AE_PHASE();
        for (int b = tid; b < B; b += kThreads) {
            // the float64 TD glue (ActorExpert.py:150-154), fed as fp32 (ae_network.py:101)
            const float y = (float)(L.r[b] + L.g[b] * (double)L.q[b]);
            L.y[b] = y;
            dv.tap_y[(size_t)agent * RLC_MAX_BATCH + b] = y;
        }
        // ---- expert step: online Q(s, a), MSE backward with the pre-step weights, Adam(expert_lr) ----
        blk_dense(L.x, S, S, nullptr, 0, th + d.W1, th + d.b1, L1, h1, L1, B, 1);
        __syncthreads();
        blk_dense(h1, L1, L1, L.a, A, th + d.Wq2, th + d.bq2, Le, hq, Le, B, 1);
        __syncthreads();
        blk_dense(hq, Le, Le, nullptr, 0, th + d.Wq3, th + d.bq3, 1, L.q, 1, B, 0);
        __syncthreads();
        AE_PHASE();
        for (int b = tid; b < B; b += kThreads) {
            dv.tap_q[(size_t)agent * RLC_MAX_BATCH + b] = L.q[b];
            L.dq[b] = 2.0f * (L.q[b] - L.y[b]) / (float)B;              // d mean((y-q)^2) / dq
        }
        __syncthreads();
        for (int it = tid; it < B * Le; it += kThreads) {
            const int b = it / Le, n = it % Le;
            d2[it] = hq[it] > 0.0f ? L.dq[b] * th[d.Wq3 + n] : 0.0f;
        }
        __syncthreads();
        blk_dense_bwd_input(d2, Le, th + d.Wq2, h1, L1, dh1, B);
        __syncthreads();
        AE_PHASE();
        {
            const AdamCtx c = {th, dv.m_c + (size_t)agent * d.Ppad, dv.v_c + (size_t)agent * d.Ppad,
                               adam_alpha(dv.expert_lr[agent], pw[2], pw[3]), tapgc};
            blk_dense_grad_adam(hq, Le, Le, nullptr, 0, L.dq, 1, B, c, d.Wq3, d.bq3);
            blk_dense_grad_adam(h1, L1, L1, L.a, A, d2, Le, B, c, d.Wq2, d.bq2);
            AE_PHASE();
            blk_dense_grad_adam(L.x, S, S, nullptr, 0, dh1, L1, B, c, d.W1, d.b1);
        }
        __syncthreads();
        // ---- forward on s with the weights AFTER the expert step: the actor's heads, and u = bq2 + h1.Wq2[:L1] ----
        AE_PHASE();
        blk_dense(L.x, S, S, nullptr, 0, th + d.W1, th + d.b1, L1, h1, L1, B, 1);
        ae_stage_q_weights(th, d.Wq2, d.Wq3, L1, Le, A, Lep, L.sw3, L.sw2a);
        __syncthreads();
        ae_dense_f64(h1, L1, L1, th + d.Wa2, th + d.ba2, La, ha, La, B, 1);
        blk_dense(h1, L1, L1, nullptr, 0, th + d.Wq2, th + d.bq2, Le, hq, Le, B, 0);
        __syncthreads();
        AE_PHASE();
        ae_dense_f64(ha, La, La, th + d.Wm, th + d.bm, MA, tm, MA, B, 2);
        ae_dense_f64(ha, La, La, th + d.Ws, th + d.bs, MA, ts, MA, B, 2);
        ae_dense_f64(ha, La, La, th + d.Wal, th + d.bal, M, tl, M, B, 2);
        __syncthreads();
        for (int it = tid; it < B * MA; it += kThreads) sg[it] = ae_sigma(ts[it]);
        for (int b = tid; b < B; b += kThreads) ae_alpha_row(tl + (size_t)b * M, M, al + (size_t)b * M);
        __syncthreads();
        // ---- the sampling pass (sample_action, ae_network.py:461-496) and Q of every sample ----
        AE_PHASE();
        {
            const unsigned long long key = dv.rep.seed[agent], nctr = dv.noise_ctr[agent];
            const float bq3 = th[d.bq3];
            float lo[RLC_AE_MAX_A], hi[RLC_AE_MAX_A];
#pragma unroll
            for (int j = 0; j < RLC_AE_MAX_A; j++) { lo[j] = dv.amin[j]; hi[j] = dv.amax[j]; }
            for (int it = tid; it < B * ns; it += kThreads) {
                const int b = it / ns;
                float uu, eps[RLC_AE_MAX_A];
                if (u_in) {
                    const size_t at = ((size_t)blockIdx.x * n_updates + u) * B * ns + it;
                    uu = u_in[at];
#pragma unroll
                    for (int j = 0; j < RLC_AE_MAX_A; j++) eps[j] = j < A ? eps_in[at * A + j] : 0.0f;
                } else {
#pragma unroll
                    for (int j = 0; j < RLC_AE_MAX_A; j++) eps[j] = 0.0f;
                    ae_philox_draws(key, nctr, kTagUpdate, (unsigned long long)it, A, uu, eps);
                }
                const int mode = ae_mode_of(al + (size_t)b * M, M, uu);
                float a[RLC_AE_MAX_A];
#pragma unroll
                for (int j = 0; j < RLC_AE_MAX_A; j++) {
                    a[j] = 0.0f;
                    if (j < A) {
                        const size_t at = (size_t)b * MA + mode * A + j;
                        a[j] = ae_draw(tm[at] * hi[j], sg[at], eps[j], lo[j], hi[j]);
                        sa[(size_t)it * A + j] = a[j];
                    }
                }
                const float* ub = hq + (size_t)b * Le;
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
                for (int n0 = 0; n0 < Lep; n0 += 4) {
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const int n = n0 + c;
                        float pre = n < Le ? ub[n] : 0.0f;
#pragma unroll
                        for (int j = 0; j < RLC_AE_MAX_A; j++)
                            if (j < A) pre = fmaf(a[j], L.sw2a[j * Lep + n], pre);
                        acc[c] = fmaf(L.sw3[n], fmaxf(pre, 0.0f), acc[c]);
                    }
                }
                sq[it] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + bq3;
            }
            if (tid == 0 && !u_in) dv.noise_ctr[agent] = nctr + 1;
        }
        __syncthreads();
        // ---- selection by rank counting and the selected samples' responsibilities: a wave per row ----
        AE_PHASE();
        for (int b = wave; b < B; b += kWaves) {
            const float* qrow = sq + (size_t)b * ns;
            const float* alr = al + (size_t)b * M;
            int base = 0;
            double lsum = 0.0;
            for (int c0 = 0; c0 < ns; c0 += 64) {
                const int j = c0 + lane;
                const bool valid = j < ns;
                const float qj = qrow[valid ? j : ns - 1];
                int rank = 0;
                for (int i = 0; i < ns; i++) {
                    const float qi = qrow[i];
                    rank += (qi > qj || (qi == qj && i < j)) ? 1 : 0;
                }
                const bool chosen = valid && rank < kk;
                const unsigned long long mask = __ballot(chosen);
                const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
                base += __popcll(mask);
                if (chosen && pos < kk) {
                    sel[(size_t)b * kk + pos] = (float)j;
                    // log c_m twice (an online log-sum-exp, then the responsibilities) rather than an array of M
                    auto log_comp = [&](int m) {
                        double s = log((double)alr[m]);
                        for (int j2 = 0; j2 < A; j2++) {
                            const size_t at = (size_t)b * MA + m * A + j2;
                            const double mu = (double)(tm[at] * dv.amax[j2]), sd = (double)sg[at];
                            const double z = ((double)sa[((size_t)b * ns + j) * A + j2] - mu) / sd;
                            s += -kHalfLog2Pi - log(sd) - 0.5 * z * z;
                        }
                        return s;
                    };
                    double mx = log_comp(0), ps = 1.0;
#pragma unroll 1
                    for (int m = 1; m < M; m++) {
                        const double s = log_comp(m);
                        if (s > mx) { ps = ps * exp(mx - s) + 1.0; mx = s; }
                        else ps += exp(s - mx);
                    }
                    const double logp = mx + log(ps);
                    const bool inside = logp >= kLogClipLo && logp <= kLogClipHi;     // clip_by_value's gradient mask
                    lsum += fmin(fmax(logp, kLogClipLo), kLogClipHi);
#pragma unroll 1
                    for (int m = 0; m < M; m++)
                        rs[((size_t)b * kk + pos) * M + m] = inside ? (float)exp(log_comp(m) - logp) : 0.0f;
                }
            }
            lsum = wave_sum64d(lsum);
            if (lane == 0) { L.rowcnt[b] = min(base, kk); L.rowloss[b] = lsum; }
        }
        __syncthreads();
        // ---- backward seeds of the three heads, summed over each row's selected samples (ascending index) ----
        AE_PHASE();
        {
            const double G = -1.0 / ((double)B * (double)kk);
            if (tid == 0) {
                double s = 0.0;
                for (int b = 0; b < B; b++) s += L.rowloss[b];
                dv.tap_loss[(size_t)agent * 4] = (float)(G * s);
            }
            for (int it = tid; it < B * MA; it += kThreads) {
                const int b = it / MA, md = it % MA, m = md / A, j2 = md % A;
                const float amx = dv.amax[j2];
                const double tmean = (double)tm[it], tsig = (double)ts[it];
                const double mu = (double)(tm[it] * amx), sd = (double)sg[it];
                double gmu = 0.0, gsd = 0.0;
                const int cnt = L.rowcnt[b];
                for (int p = 0; p < cnt; p++) {
                    const int j = (int)sel[(size_t)b * kk + p];
                    const double w = (double)rs[((size_t)b * kk + p) * M + m];
                    const double z = ((double)sa[((size_t)b * ns + j) * A + j2] - mu) / sd;
                    gmu += w * z / sd;
                    gsd += w * (z * z - 1.0) / sd;
                }
                tm[it] = (float)(G * gmu * ((double)amx * (1.0 - tmean * tmean)));
                ts[it] = (float)(G * gsd * (sd * 11.0 * (1.0 - tsig * tsig)));
            }
            for (int b = tid; b < B; b += kThreads) {
                const int cnt = L.rowcnt[b];
                auto mode_sum = [&](int m) {
                    double s = 0.0;
                    for (int p = 0; p < cnt; p++) s += (double)rs[((size_t)b * kk + p) * M + m];
                    return s;
                };
                double tot = 0.0;
                for (int m = 0; m < M; m++) tot += mode_sum(m);
                for (int m = 0; m < M; m++) {
                    const double t = (double)tl[(size_t)b * M + m];
                    // d alpha_m = G sm / alpha_m through the softmax: alpha_m (d alpha_m - sum_i alpha_i d alpha_i)
                    tl[(size_t)b * M + m] = (float)(G * (mode_sum(m) - (double)al[(size_t)b * M + m] * tot) * (1.0 - t * t));
                }
            }
        }
        __syncthreads();
        // ---- actor backward: the three heads into ha, then Wa2 into h1 ----
        AE_PHASE();
        blk_dense_bwd_input_ex(tm, MA, th + d.Wm, ha, La, dha, B, false);
        __syncthreads();
        blk_dense_bwd_input_ex(ts, MA, th + d.Ws, ha, La, dha, B, true);
        __syncthreads();
        blk_dense_bwd_input_ex(tl, M, th + d.Wal, ha, La, dha, B, true);
        __syncthreads();
        blk_dense_bwd_input(dha, La, th + d.Wa2, h1, L1, dh1, B);
        __syncthreads();
        // ---- gradients + Adam(actor_lr) over the actor's ten tensors (ae_network.py:112-114) ----
        AE_PHASE();
        {
            const AdamCtx c = {th, dv.m_a + (size_t)agent * d.Ppad, dv.v_a + (size_t)agent * d.Ppad,
                               adam_alpha(dv.actor_lr[agent], pw[0], pw[1]), tapga};
            blk_dense_grad_adam(ha, La, La, nullptr, 0, tm, MA, B, c, d.Wm, d.bm);
            blk_dense_grad_adam(ha, La, La, nullptr, 0, ts, MA, B, c, d.Ws, d.bs);
            blk_dense_grad_adam(ha, La, La, nullptr, 0, tl, M, B, c, d.Wal, d.bal);
            AE_PHASE();
            blk_dense_grad_adam(h1, L1, L1, nullptr, 0, dha, La, B, c, d.Wa2, d.ba2);
            blk_dense_grad_adam(L.x, S, S, nullptr, 0, dh1, L1, B, c, d.W1, d.b1);
        }
        __syncthreads();
        // ---- Polyak on every tensor (ae_network.py:84-86) ----
        AE_PHASE();
        if (tid == 0) { pw[0] *= 0.9f; pw[1] *= 0.999f; pw[2] *= 0.9f; pw[3] *= 0.999f; }
        for (int p = tid; p < d.Pdev; p += kThreads) {
            const float t = tt[p];
            tt[p] = t + dv.tau * (th[p] - t);
        }
        __syncthreads();
    }
#undef AE_PHASE
#undef dv
#undef d
}

// LDS of the one-row kernels: x [S + A], h1 [L1], ha [La], hq [Le], the three heads' rows, reduction words
struct ARowLds { float *x, *h1, *ha, *hq, *tm, *ts, *tl, *al, *redv; };
__host__ __device__ inline size_t arow_carve(const RlcAeDims& d, float* base, ARowLds* out) {
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 3) & ~(size_t)3; return p; };
    ARowLds L;
    L.x = take(d.S + d.A); L.h1 = take(d.L1); L.ha = take(d.La); L.hq = take(d.Le);
    L.tm = take((size_t)d.M * d.A); L.ts = take((size_t)d.M * d.A); L.tl = take(d.M); L.al = take(d.M);
    L.redv = take(kWaves + 8);
    if (out) *out = L;
    return off * sizeof(float);
}

// predict_action (sample 0; ae_network.py:409-435) or one draw of sample_action (sample 1; :461-496, is_single_sample)
// of the ONLINE network for one state per agent.  done_flag (or null): a word in host-visible memory that receives
// done_val once the launch's outputs are stored (rlc_ae_act_queue; see rlc_ddpg_act_kernel)
__global__ __launch_bounds__(kThreads) void rlc_ae_act_kernel(RlcAeDev dv, int first_agent, const float* states,
                                                              const float* u_in, const float* eps_in, int sample,
                                                              float* out, int* done_flag, int done_val) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RlcAeDims& d = dv.d;
    const int S = d.S, A = d.A, M = d.M, MA = M * A;
    const int agent = first_agent + blockIdx.x, tid = threadIdx.x;
    ARowLds L;
    arow_carve(d, (float*)smem, &L);
    const float* th = dv.theta + (size_t)agent * d.Ppad;
    for (int i = tid; i < S; i += kThreads)
        L.x[i] = clip_state_val(states[(size_t)blockIdx.x * S + i], dv.clip_state, dv.smin[i], dv.smax[i]);
    __syncthreads();
    rlc_hidden_forward_row(th + d.W1, 0, th + d.b1, L.x, S, d.L1, L.h1, true);
    __syncthreads();
    ae_row_f64(th + d.Wa2, th + d.ba2, L.h1, d.L1, d.La, L.ha, 1);
    __syncthreads();
    ae_row_f64(th + d.Wm, th + d.bm, L.ha, d.La, MA, L.tm, 2);
    ae_row_f64(th + d.Ws, th + d.bs, L.ha, d.La, MA, L.ts, 2);
    ae_row_f64(th + d.Wal, th + d.bal, L.ha, d.La, M, L.tl, 2);
    __syncthreads();
    if (tid == 0) {
        float* alpha = L.al;
        ae_alpha_row(L.tl, M, alpha);
        if (!sample) {
            const int best = ae_best_mode(alpha, M);
            for (int j = 0; j < A; j++) out[(size_t)blockIdx.x * A + j] = L.tm[best * A + j] * dv.amax[j];
        } else {
            float uu, eps[RLC_AE_MAX_A] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (u_in) {
                uu = u_in[blockIdx.x];
                for (int j = 0; j < A; j++) eps[j] = eps_in[(size_t)blockIdx.x * A + j];
            } else {
                const unsigned long long nctr = dv.noise_ctr[agent];
                ae_philox_draws(dv.rep.seed[agent], nctr, kTagAct, 0ull, A, uu, eps);
                dv.noise_ctr[agent] = nctr + 1;
            }
            const int mode = ae_mode_of(alpha, M, uu);
            for (int j = 0; j < A; j++)
                out[(size_t)blockIdx.x * A + j] = ae_draw(L.tm[mode * A + j] * dv.amax[j], ae_sigma(L.ts[mode * A + j]), eps[j],
                                                          dv.amin[j], dv.amax[j]);
        }
        if (done_flag) {
            __threadfence_system();                     // the output stores first
            __hip_atomic_store(done_flag, done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// Q(s,a) rows on one agent's online network (getQFunction, ae_network.py:504-507).  One workgroup per row; the sum over
// the expert layer's units is split over the threads (fixed order: deterministic).
__global__ __launch_bounds__(kThreads) void rlc_ae_qval_kernel(RlcAeDev dv, int agent, const float* states,
                                                               const float* actions, float* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RlcAeDims& d = dv.d;
    const int S = d.S, A = d.A, L1 = d.L1, Le = d.Le;
    const int tid = threadIdx.x, row = blockIdx.x;
    ARowLds L;
    arow_carve(d, (float*)smem, &L);
    const float* th = dv.theta + (size_t)agent * d.Ppad;
    for (int i = tid; i < S; i += kThreads)
        L.x[i] = clip_state_val(states[(size_t)row * S + i], dv.clip_state, dv.smin[i], dv.smax[i]);
    for (int k = tid; k < A; k += kThreads) L.x[S + k] = actions[(size_t)row * A + k];
    __syncthreads();
    rlc_hidden_forward_row(th + d.W1, 0, th + d.b1, L.x, S, L1, L.h1, true);
    __syncthreads();
    rlc_hidden_forward_row(th + d.Wq2, 0, th + d.bq2, L.h1, L1, Le, L.hq, false);
    __syncthreads();
    float part = 0.0f;
    for (int n = tid; n < Le; n += kThreads) {
        float pre = L.hq[n];
        for (int k = 0; k < A; k++) pre = fmaf(L.x[S + k], th[d.Wq2 + (size_t)(L1 + k) * Le + n], pre);
        part = fmaf(th[d.Wq3 + n], fmaxf(pre, 0.0f), part);
    }
    const float q = blk_sum(part, L.redv);
    if (tid == 0) out[row] = q + th[d.bq3];
}

}  // namespace

size_t rlc_ae_scratch_floats(const RlcAeDims& d) {
    const size_t B = d.B, MA = (size_t)d.M * d.A;
    return 2 * pad4z(B * d.L1) + 2 * pad4z(B * d.Le) + 2 * pad4z(B * d.La) + 3 * pad4z(B * MA) + 2 * pad4z(B * d.M) +
           pad4z(B * d.k * d.M);
}

const char* rlc_ae_refusal(const RlcAeDims& d) {
    static thread_local char msg[200];
    const size_t up = alds_carve(d, nullptr, nullptr), row = arow_carve(d, nullptr, nullptr);
    const size_t need = up > row ? up : row;
    if (need <= 64 * 1024) return nullptr;
    snprintf(msg, sizeof(msg), "state_dim %d, layer widths %d / %d / %d at batch_size %d need %zu B of LDS (> 65536)", d.S,
             d.L1, d.La, d.Le, d.B, need);
    return msg;
}

int rlc_launch_ae_update(const RlcAeDev& dv, int first_agent, int n_agents, int n_updates, int source,
                         const long long* idx_dev, const float* u_dev, const float* eps_dev, int grad_taps, hipStream_t st) {
    const size_t lds = alds_carve(dv.d, nullptr, nullptr);
    RLC_REQUIRE(lds <= 64 * 1024, "ActorExpert kernel needs %zu B of LDS (> 64 KiB)", lds);
    RLC_REQUIRE((u_dev == nullptr) == (eps_dev == nullptr), "u and eps: both null (the device's draws) or neither");
    hipLaunchKernelGGL(rlc_ae_update_kernel, dim3(n_agents), dim3(kThreads), lds, st, dv, first_agent, n_updates, source,
                       idx_dev, u_dev, eps_dev, grad_taps);
    RLC_HIP(hipGetLastError());
    return 0;
}

int rlc_launch_ae_act(const RlcAeDev& dv, int first_agent, int n, const float* states_dev, const float* u_dev,
                      const float* eps_dev, int sample, float* out_dev, hipStream_t st, int* done_flag, int done_val) {
    const size_t lds = arow_carve(dv.d, nullptr, nullptr);
    RLC_REQUIRE(lds <= 64 * 1024, "ActorExpert acting kernel needs %zu B of LDS (> 64 KiB)", lds);
    RLC_REQUIRE(done_flag == nullptr || n == 1, "a completion flag needs a one-workgroup acting launch");
    hipLaunchKernelGGL(rlc_ae_act_kernel, dim3(n), dim3(kThreads), lds, st, dv, first_agent, states_dev, u_dev, eps_dev,
                       sample, out_dev, done_flag, done_val);
    RLC_HIP(hipGetLastError());
    return 0;
}

int rlc_launch_ae_qval(const RlcAeDev& dv, int agent, int n, const float* states_dev, const float* actions_dev,
                       float* out_dev, hipStream_t st) {
    const size_t lds = arow_carve(dv.d, nullptr, nullptr);
    RLC_REQUIRE(lds <= 64 * 1024, "ActorExpert Q-value kernel needs %zu B of LDS (> 64 KiB)", lds);
    hipLaunchKernelGGL(rlc_ae_qval_kernel, dim3(n), dim3(kThreads), lds, st, dv, agent, states_dev, actions_dev, out_dev);
    RLC_HIP(hipGetLastError());
    return 0;
}
