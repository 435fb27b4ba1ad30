// wf_generic.hip -- fused WireFitting update, acting and Q-value kernels (any-shape fp32 VALU path).
//
// One workgroup per agent, n_updates sequential updates per launch; each update = sample_batch
// (utils/replaybuffer.py:32-37) + WireFitting_Network_Manager.update_network (agents/WireFitting.py:66-77):
//   max_q[b] = max_i qhat'_i(s'_b) with the TARGET network's wire values (wf_network.py:94,153-159),
//   y = r + gamma * max_q formed in float64 then cast (WireFitting.py:71), one Adam step on loss = MEAN (y - Q(s,a))^2
//   (wf_network.py:50,63) over all nine tensors, Polyak by assign_add on all nine (:56-58), kappa' included.
// Network (wf_network.py:66-104): h1 = relu(x.W1 + b1), h2 = relu(h1.W2 + b2), wire actions
// ahat = tanh(h2.Wa + ba) * action_max[0] read as [N][A], wire values qhat = h2.Wq + bq.
// Interpolation (wf_network.py:106-125), per row:
//   M = max_i qhat_i, c_i = sigmoid(kappa_i), d_i = sum_k (a_k - ahat_ik)^2 + c_i (M - qhat_i) + 1e-5, w_i = 1 / d_i,
//   Q = sum_i (w_i / sum_j w_j) qhat_i      (the weights are normalised first, as :123-124 do: with one wire Q is
//                                            qhat_0 bit for bit, whatever the action)
// ARITHMETIC ORDER of the interpolation (every kernel of this file): one wave per row, lane l owns wires l, l + 64, ...
// in ascending order.  The row's arithmetic runs in float64 on the fp32 inputs (tanh outputs, wire values, action, c):
// d_i = (fma chain over k ascending + c_i (M - qhat_i)) + 1e-5f, w_i = (float)(1 / d_i) -- the 1e-5 floor makes w as
// large as 1e5 -- then W, Q, e_i and the seeds from that fp32 w_i, each seed rounded to fp32 once.  The differences
// a_k - ahat_ik and qhat_i - Q cancel where w is large; in fp32 their rounding was the kernel's largest error (the row
// costs N (A + 20) operations: nothing beside the dense layers).  A lane's partial sums run over its wires ascending,
// the 64 partial sums go through one fixed xor-shuffle tree.  (max, index): a lane keeps a strict maximum,
// lanes merge by (larger value, then lower index) -- the lowest index among equal maxima, as tf.argmax (:97).
// Backward seeds, written in place over qhat and tanh(.) (g = 2 (Q - y) / B, W = sum w, e_i = -w_i^2 (qhat_i - Q) / W):
//   dL/dqhat_i = g (w_i / W - c_i e_i) + [i = i*] g sum_j c_j e_j          (the gradient through M goes to wire i*)
//   dL/dahat_ik = -2 g e_i (a_k - ahat_ik), times (1 - tanh^2) action_max[0] for the head's linear output
//   dL/dkappa_i = sum_b g e_i c_i (1 - c_i) (M - qhat_i), the rows summed in ascending order by one thread
// No atomics anywhere: one launch of K updates equals K launches of one bit for bit.
#include <limits.h>
#include <stdio.h>

#include "generic_blocks.h"
#include "wf_common.h"

namespace {

using namespace gen;

constexpr int kWaves = kThreads / 64;
constexpr float kSmoothEps = 0.00001f;          // smooth_eps (wf_network.py:27)

__host__ __device__ inline size_t pad4z(size_t n) { return (n + 3) & ~(size_t)3; }

__device__ __forceinline__ void best_merge(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void wave_best64(float& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        best_merge(v, i, ov, oi);
    }
}
__device__ __forceinline__ float wf_sigmoid(float k) { return (float)(1.0 / (1.0 + exp(-(double)k))); }
__device__ __forceinline__ double wave_sum64d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Y[b,n] = act(sum_k X[b,k] W[k,n] + bias[n]) with the sum carried in float64: every product of two floats is exact
// there, so the result is the correctly rounded value of the exact dot product (and of its tanh).  The ONLINE second
// layer and both heads go through it: the interpolation divides by d_i = |a - ahat_i|^2 + ..., so the rounding error of
// ahat is amplified by 1 / |a - ahat_i| in the wires next to the action -- with blk_dense's one fp32 chain over 200
// terms the gradient of `ba` at (3, 1, 200, 200, 100), batch 100, was 5.8e-5 off the float64 restatement where torch's
// blocked fp32 sums are 1.2e-5 off.  Same thread-item shape as blk_dense's element-wise path; act: 0 none, 1 relu, 2 tanh.
__device__ inline void wf_dense_f64(const float* X, int ldx, int K, const float* W, const float* bias, int N, float* Y,
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

struct WfRow { double M, W, Q; int istar; };

// One wave, one row: qh [N] wire values, tv [N][A] tanh outputs (unscaled), a [A] the action, c [N] sigmoid(kappa).
// Writes w [N] (lane l its own wires only) and returns M, i*, W, Q in every lane.
__device__ inline WfRow wf_row_forward(const float* qh, const float* tv, const float* a, const float* c, int N, int A,
                                       float amax0, float* w) {
    const int lane = threadIdx.x & 63;
    WfRow r;
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int i = lane; i < N; i += 64) {
        const float q = qh[i];
        if (q > bv) { bv = q; bi = i; }
    }
    wave_best64(bv, bi);
    r.M = bv;
    r.istar = bi < N ? bi : 0;                  // (no finite or infinite maximum: all NaN)
    double sw = 0.0;
    for (int i = lane; i < N; i += 64) {
        double dist = 0.0;
        for (int k = 0; k < A; k++) {
            const double df = (double)a[k] - (double)tv[(size_t)i * A + k] * (double)amax0;
            dist = fma(df, df, dist);
        }
        const double dd = (dist + (double)c[i] * (r.M - (double)qh[i])) + (double)kSmoothEps;
        const float wi = (float)(1.0 / dd);     // kept as fp32: every later pass reads this value
        w[i] = wi;
        sw += (double)wi;
    }
    r.W = wave_sum64d(sw);
    double sq = 0.0;
    for (int i = lane; i < N; i += 64) sq = fma((double)w[i] / r.W, (double)qh[i], sq);
    r.Q = wave_sum64d(sq);
    return r;
}

struct WLds {
    double *r, *g;
    long long* idx;
    float *x, *x2, *a, *y, *c;
    int* pool;
    int* dups;
};

__host__ __device__ inline size_t wlds_carve(const RlcWfDims& d, unsigned char* base, WLds* out) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        unsigned char* p = base ? base + off : nullptr;
        off += (bytes + 15) & ~(size_t)15;
        return p;
    };
    const size_t B = d.B, S = d.S, A = d.A;
    WLds L;
    L.r = (double*)take(sizeof(double) * B);
    L.g = (double*)take(sizeof(double) * B);
    L.idx = (long long*)take(sizeof(long long) * RLC_MAX_BATCH);
    L.x = (float*)take(sizeof(float) * B * S);
    L.x2 = (float*)take(sizeof(float) * B * S);
    L.a = (float*)take(sizeof(float) * B * A);
    L.y = (float*)take(sizeof(float) * B);
    L.c = (float*)take(sizeof(float) * (size_t)d.N);
    L.pool = (int*)take(sizeof(int) * 3 * RLC_MAX_BATCH);
    L.dups = (int*)take(sizeof(int) * 4);
    if (out) *out = L;
    return off;
}

__global__ __launch_bounds__(kThreads) void rlc_wf_update_kernel(RlcWfDev dv_arg, int first_agent, int n_updates,
                                                                 int source, const long long* host_idx, int grad_taps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the population view is read through gen::kernarg_view (generic_blocks.h), made opaque again by WF_PHASE() at the
    // start of every phase (dv_arg is the first argument: offset 0)
    const RlcWfDev* dvp;
#define WF_PHASE() (dvp = kernarg_view<RlcWfDev>())
#define dv (*dvp)
#define d (dvp->d)
    WF_PHASE();
    const int S = d.S, A = d.A, L1 = d.L1, L2 = d.L2, N = d.N, B = d.B, NA = N * A;
    const int agent = first_agent + blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    WLds L;
    wlds_carve(d, smem, &L);
    float* th = dv.theta + (size_t)agent * d.Ppad;
    float* tt = dv.theta_t + (size_t)agent * d.Ppad;
    float* pw = dv.pw + agent * 2;
    float* sc = dv.scratch + (size_t)agent * dv.scratch_stride;
    float* h1 = sc;  sc += pad4z((size_t)B * L1);
    float* h2 = sc;  sc += pad4z((size_t)B * L2);
    float* ah = sc;  sc += pad4z((size_t)B * NA);     // tanh outputs [B][N][A], then the action head's backward seeds
    float* qh = sc;  sc += pad4z((size_t)B * N);      // wire values [B][N] (target's, then online), then their seeds
    float* wb = sc;  sc += pad4z((size_t)B * N);      // w_i, then each row's term of the kappa gradient
    float* d2 = sc;  sc += pad4z((size_t)B * L2);
    float* dh1 = sc; sc += pad4z((size_t)B * L1);
    float* tapg = grad_taps ? dv.tap_g + (size_t)agent * d.Ppad : nullptr;

    for (int u = 0; u < n_updates; u++) {
        // ---- sample + gather (utils/replaybuffer.py:32-37) ----
        WF_PHASE();
        const RlcRingMeta ring = dv.rep.ring[agent];
        rlc_pick_indices<kThreads>(dv.rep, agent, ring, source, B, host_idx, (size_t)blockIdx.x * n_updates + u, L.pool, L.idx,
                                   L.dups);
        WF_PHASE();
        for (int b = tid; b < B; b += kThreads) {
            const RlcRow w = rlc_locate_row(dv.rep, agent, ring, source, S, A, b, L.idx);
            L.r[b] = w.r; L.g[b] = w.g;
            for (int i = 0; i < S; i++) {
                L.x[b * S + i] = clip_state_val(w.s[i], dv.clip_state, dv.smin[i], dv.smax[i]);
                L.x2[b * S + i] = clip_state_val(w.s2[i], dv.clip_state, dv.smin[i], dv.smax[i]);
            }
            for (int j = 0; j < A; j++) L.a[b * A + j] = w.a[j];
        }
        for (int i = tid; i < N; i += kThreads) L.c[i] = wf_sigmoid(th[d.kap + i]);
        __syncthreads();
        // ---- target: both hidden layers and the value head only, then the row maximum (WireFitting.py:69) ----
        WF_PHASE();
        blk_dense(L.x2, S, S, nullptr, 0, tt + d.W1, tt + d.b1, L1, h1, L1, B, 1);
        __syncthreads();
        blk_dense(h1, L1, L1, nullptr, 0, tt + d.W2, tt + d.b2, L2, h2, L2, B, 1);
        __syncthreads();
        blk_dense(h2, L2, L2, nullptr, 0, tt + d.Wq, tt + d.bq, N, qh, N, B, 0);
        __syncthreads();
        WF_PHASE();
        for (int b = wave; b < B; b += kWaves) {
            float bv = -INFINITY;
            int bi = INT_MAX;
            for (int i = lane; i < N; i += 64) {
                const float q = qh[(size_t)b * N + i];
                if (q > bv) { bv = q; bi = i; }
            }
            wave_best64(bv, bi);
            if (lane == 0) {
                // the float64 TD glue (agents/WireFitting.py:71), fed as fp32 (wf_network.py:62)
                const float y = (float)(L.r[b] + L.g[b] * (double)bv);
                L.y[b] = y;
                dv.tap_maxq[(size_t)agent * RLC_MAX_BATCH + b] = bv;
                dv.tap_y[(size_t)agent * RLC_MAX_BATCH + b] = y;
            }
        }
        __syncthreads();
        // ---- online forward on s: both hidden layers, both heads (the L1- and L2-deep sums in float64) ----
        WF_PHASE();
        blk_dense(L.x, S, S, nullptr, 0, th + d.W1, th + d.b1, L1, h1, L1, B, 1);
        __syncthreads();
        wf_dense_f64(h1, L1, L1, th + d.W2, th + d.b2, L2, h2, L2, B, 1);
        __syncthreads();
        wf_dense_f64(h2, L2, L2, th + d.Wa, th + d.ba, NA, ah, NA, B, 2);
        wf_dense_f64(h2, L2, L2, th + d.Wq, th + d.bq, N, qh, N, B, 0);
        __syncthreads();
        // ---- interpolation and its backward seeds with the pre-step weights: a wave per row ----
        WF_PHASE();
        {
            const float amax0 = dv.amax0;
            for (int b = wave; b < B; b += kWaves) {
                float* q = qh + (size_t)b * N;
                float* t = ah + (size_t)b * NA;
                float* w = wb + (size_t)b * N;
                const float* a = L.a + b * A;
                const WfRow r = wf_row_forward(q, t, a, L.c, N, A, amax0, w);
                const double g = 2.0 * (r.Q - (double)L.y[b]) / (double)B;  // d mean((y-Q)^2) / dQ
                double sce = 0.0, dq_star = 0.0;
                for (int i = lane; i < N; i += 64) {
                    const double wi = w[i], qi = q[i], ci = L.c[i];
                    const double e = -(wi * wi) * (qi - r.Q) / r.W;
                    sce = fma(ci, e, sce);
                    const double dq = g * (wi / r.W - ci * e);
                    if (i == r.istar) dq_star = dq;
                    q[i] = (float)dq;
                    w[i] = (float)(g * e * (ci * (1.0 - ci)) * (r.M - qi));
                    for (int k = 0; k < A; k++) {
                        const double tk = t[(size_t)i * A + k];
                        const double df = (double)a[k] - tk * (double)amax0;
                        t[(size_t)i * A + k] = (float)((-2.0 * g * e * df) * ((1.0 - tk * tk) * (double)amax0));
                    }
                }
                sce = wave_sum64d(sce);
                if (lane == (r.istar & 63)) q[r.istar] = (float)(dq_star + g * sce);   // the lane that owns wire i*
                if (lane == 0) dv.tap_q[(size_t)agent * RLC_MAX_BATCH + b] = (float)r.Q;
            }
        }
        __syncthreads();
        // ---- backward through the two heads (their dh2 contributions add), then W2 ----
        WF_PHASE();
        blk_dense_bwd_input_ex(ah, NA, th + d.Wa, h2, L2, d2, B, false);
        __syncthreads();
        blk_dense_bwd_input_ex(qh, N, th + d.Wq, h2, L2, d2, B, true);
        __syncthreads();
        blk_dense_bwd_input(d2, L2, th + d.W2, h1, L1, dh1, B);
        __syncthreads();
        // ---- gradients + one Adam over the nine tensors (wf_network.py:50) ----
        WF_PHASE();
        {
            const AdamCtx c = {th, dv.m + (size_t)agent * d.Ppad, dv.v + (size_t)agent * d.Ppad,
                               adam_alpha(dv.lr[agent], pw[0], pw[1]), tapg};
            blk_dense_grad_adam(h2, L2, L2, nullptr, 0, ah, NA, B, c, d.Wa, d.ba);
            blk_dense_grad_adam(h2, L2, L2, nullptr, 0, qh, N, B, c, d.Wq, d.bq);
            WF_PHASE();
            blk_dense_grad_adam(h1, L1, L1, nullptr, 0, d2, L2, B, c, d.W2, d.b2);
            blk_dense_grad_adam(L.x, S, S, nullptr, 0, dh1, L1, B, c, d.W1, d.b1);
            WF_PHASE();
            for (int i = tid; i < N; i += kThreads) {
                float gk = 0.0f;
                for (int b = 0; b < B; b++) gk += wb[(size_t)b * N + i];
                adam_apply(c, d.kap + i, gk);
            }
        }
        __syncthreads();
        // ---- Polyak (wf_network.py:56-58) ----
        WF_PHASE();
        if (tid == 0) { pw[0] *= 0.9f; pw[1] *= 0.999f; }
        for (int p = tid; p < d.Pdev; p += kThreads) {
            const float t = tt[p];
            tt[p] = t + dv.tau * (th[p] - t);
        }
        __syncthreads();
    }
#undef WF_PHASE
#undef dv
#undef d
}

// LDS of the one-row kernels: x [S + A], h1 [L1], h2 [L2], the action head's row [N*A], the value head's row [N],
// w [N], c [N], reduction words
struct WRowLds { float *x, *h1, *h2, *ta, *qv, *w, *c, *redv; int* redi; };
__host__ __device__ inline size_t wrow_carve(const RlcWfDims& d, float* base, WRowLds* out) {
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 3) & ~(size_t)3; return p; };
    WRowLds L;
    L.x = take(d.S + d.A); L.h1 = take(d.L1); L.h2 = take(d.L2); L.ta = take((size_t)d.N * d.A); L.qv = take(d.N);
    L.w = take(d.N); L.c = take(d.N); L.redv = take(kWaves); L.redi = (int*)take(kWaves);
    if (out) *out = L;
    return off * sizeof(float);
}

// the row in L.x through the online network: L.ta = tanh(h2.Wa + ba) (unscaled), L.qv = h2.Wq + bq
__device__ inline void wf_row_prelude(const RlcWfDims& d, const float* th, const WRowLds& L) {
    const int NA = d.N * d.A;
    __syncthreads();
    rlc_hidden_forward_row(th + d.W1, 0, th + d.b1, L.x, d.S, d.L1, L.h1, true);
    __syncthreads();
    rlc_hidden_forward_row(th + d.W2, 0, th + d.b2, L.h1, d.L1, d.L2, L.h2, true);
    __syncthreads();
    rlc_hidden_forward_row(th + d.Wa, 0, th + d.ba, L.h2, d.L2, NA, L.ta, false);
    rlc_hidden_forward_row(th + d.Wq, 0, th + d.bq, L.h2, d.L2, d.N, L.qv, false);
    __syncthreads();
    for (int i = threadIdx.x; i < NA; i += kThreads) L.ta[i] = tanhf(L.ta[i]);
    __syncthreads();
}

// predict_action (wf_network.py:136-143; agents/WireFitting.py:25) for one state per agent: the arg-max wire's action,
// every wire's action and every wire's value.  done_flag (or null): a word in host-visible memory that receives done_val
// once the launch's outputs are stored (rlc_wf_act_queue; see rlc_ddpg_act_kernel)
__global__ __launch_bounds__(kThreads) void rlc_wf_act_kernel(RlcWfDev dv, int first_agent, int n, const float* states,
                                                              float* out, int* done_flag, int done_val) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RlcWfDims& d = dv.d;
    const int S = d.S, A = d.A, N = d.N, NA = N * A;
    const int agent = first_agent + blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    WRowLds L;
    wrow_carve(d, (float*)smem, &L);
    const float* th = dv.theta + (size_t)agent * d.Ppad;
    for (int i = tid; i < S; i += kThreads)
        L.x[i] = clip_state_val(states[(size_t)blockIdx.x * S + i], dv.clip_state, dv.smin[i], dv.smax[i]);
    wf_row_prelude(d, th, L);
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int i = tid; i < N; i += kThreads) {
        const float q = L.qv[i];
        if (q > bv) { bv = q; bi = i; }
    }
    wave_best64(bv, bi);
    if (lane == 0) { L.redv[wave] = bv; L.redi[wave] = bi; }
    __syncthreads();
    bv = L.redv[0]; bi = L.redi[0];
    for (int w = 1; w < kWaves; w++) best_merge(bv, bi, L.redv[w], L.redi[w]);
    const int istar = bi < N ? bi : 0;
    float* o_act = out + (size_t)blockIdx.x * A;
    float* o_wa = out + (size_t)n * A + (size_t)blockIdx.x * NA;
    float* o_wq = out + (size_t)n * (A + NA) + (size_t)blockIdx.x * N;
    for (int k = tid; k < A; k += kThreads) o_act[k] = L.ta[istar * A + k] * dv.amax0;
    for (int i = tid; i < NA; i += kThreads) o_wa[i] = L.ta[i] * dv.amax0;
    for (int i = tid; i < N; i += kThreads) o_wq[i] = L.qv[i];
    if (done_flag) {
        __threadfence_system();                         // every thread's output stores first
        __syncthreads();
        if (tid == 0) __hip_atomic_store(done_flag, done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Q(s,a) rows on one agent's online network (getQFunction, wf_network.py:167-171).  One workgroup per row; the
// interpolation runs on its first wave exactly as in the update kernel.
__global__ __launch_bounds__(kThreads) void rlc_wf_qval_kernel(RlcWfDev dv, int agent, const float* states,
                                                               const float* actions, float* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RlcWfDims& d = dv.d;
    const int S = d.S, A = d.A, N = d.N;
    const int tid = threadIdx.x, row = blockIdx.x;
    WRowLds L;
    wrow_carve(d, (float*)smem, &L);
    const float* th = dv.theta + (size_t)agent * d.Ppad;
    for (int i = tid; i < S; i += kThreads)
        L.x[i] = clip_state_val(states[(size_t)row * S + i], dv.clip_state, dv.smin[i], dv.smax[i]);
    for (int k = tid; k < A; k += kThreads) L.x[S + k] = actions[(size_t)row * A + k];
    for (int i = tid; i < N; i += kThreads) L.c[i] = wf_sigmoid(th[d.kap + i]);
    wf_row_prelude(d, th, L);
    if (tid < 64) {
        const WfRow r = wf_row_forward(L.qv, L.ta, L.x + S, L.c, N, A, dv.amax0, L.w);
        if (tid == 0) out[row] = (float)r.Q;
    }
}

}  // namespace

size_t rlc_wf_scratch_floats(const RlcWfDims& d) {
    const size_t B = d.B;
    return 2 * pad4z(B * d.L1) + 2 * pad4z(B * d.L2) + pad4z(B * d.N * d.A) + 2 * pad4z(B * d.N);
}

const char* rlc_wf_refusal(const RlcWfDims& d) {
    static thread_local char msg[200];
    const size_t up = wlds_carve(d, nullptr, nullptr), row = wrow_carve(d, nullptr, nullptr);
    const size_t need = up > row ? up : row;
    if (need <= 64 * 1024) return nullptr;
    snprintf(msg, sizeof(msg), "state_dim %d, layer widths %d / %d, app_points %d at batch_size %d need %zu B of LDS (> 65536)",
             d.S, d.L1, d.L2, d.N, d.B, need);
    return msg;
}

int rlc_launch_wf_update(const RlcWfDev& dv, int first_agent, int n_agents, int n_updates, int source,
                         const long long* idx_dev, int grad_taps, hipStream_t st) {
    const size_t lds = wlds_carve(dv.d, nullptr, nullptr);
    RLC_REQUIRE(lds <= 64 * 1024, "WireFitting kernel needs %zu B of LDS (> 64 KiB)", lds);
    hipLaunchKernelGGL(rlc_wf_update_kernel, dim3(n_agents), dim3(kThreads), lds, st, dv, first_agent, n_updates, source,
                       idx_dev, grad_taps);
    RLC_HIP(hipGetLastError());
    return 0;
}

int rlc_launch_wf_act(const RlcWfDev& dv, int first_agent, int n, const float* states_dev, float* out_dev, hipStream_t st,
                      int* done_flag, int done_val) {
    const size_t lds = wrow_carve(dv.d, nullptr, nullptr);
    RLC_REQUIRE(lds <= 64 * 1024, "WireFitting acting kernel needs %zu B of LDS (> 64 KiB)", lds);
    RLC_REQUIRE(done_flag == nullptr || n == 1, "a completion flag needs a one-workgroup acting launch");
    hipLaunchKernelGGL(rlc_wf_act_kernel, dim3(n), dim3(kThreads), lds, st, dv, first_agent, n, states_dev, out_dev,
                       done_flag, done_val);
    RLC_HIP(hipGetLastError());
    return 0;
}

int rlc_launch_wf_qval(const RlcWfDev& dv, int agent, int n, const float* states_dev, const float* actions_dev,
                       float* out_dev, hipStream_t st) {
    const size_t lds = wrow_carve(dv.d, nullptr, nullptr);
    RLC_REQUIRE(lds <= 64 * 1024, "WireFitting Q-value kernel needs %zu B of LDS (> 64 KiB)", lds);
    hipLaunchKernelGGL(rlc_wf_qval_kernel, dim3(n), dim3(kThreads), lds, st, dv, agent, states_dev, actions_dev, out_dev);
    RLC_HIP(hipGetLastError());
    return 0;
}
