// optq_generic.hip -- fused OptimalQ update, acting and Q-value kernels (any-shape fp32 VALU path).
//
// One workgroup per agent, n_updates sequential updates per launch; each update = sample_batch
// (utils/replaybuffer.py:32-37) + OptimalQ_Network_Manager.update_network (agents/OptimalQ.py:68-89):
//   max_q[b] = max_j Q'(s'_b, grid_j) with the TARGET network over the whole action grid (optimal_q_network.py:121-161),
//   y = r + gamma * max_q formed in float64 then cast (OptimalQ.py:83), one Adam step on loss = MEAN (y - Q(s,a))^2
//   (optimal_q_network.py:56-57), Polyak by assign_add on all six tensors (:64-65).
// Q(s,a) = b3 + W3 . relu(b2 + h1 . W2[:L1] + a . W2[L1:]), h1 = relu(b1 + s . W1) (optimal_q_network.py:82-108).
//
// The action enters at the second layer only, so the grid search does not tile the states against the grid as the
// reference does: per state h1 and u = b2 + h1 . W2[:L1] are computed once (two dense blocks), and per grid node j
//   q_j = ( sum_n W3[n] * relu(u[n] + sum_k grid[j][k] * W2[L1+k][n]) ) + b3
// remains.  ARITHMETIC ORDER of the grid pass (every kernel of this file that runs it): pre = u[n], then
// pre = fmaf(grid[j][k], W2[L1+k][n], pre) for k ascending; FOUR partial sums acc_c = 0 (c = n mod 4), each an ascending
// chain acc_c = fmaf(W3[n], max(pre, 0), acc_c) over its n = c, c + 4, ...; q = ((acc_0 + acc_1) + (acc_2 + acc_3)) + b3.
// Four chains and not one: neighbouring nodes of a 1e-3 grid differ by a few fp32 ulps of Q near an interior maximum, and
// the rounding error of one 200-term chain (about 3x that of the blocked sums of a BLAS sgemm) moved the argmax off the
// restatement's in 4 of 96 rows of the shipped shape where four chains move it in 1; the chains are
// also independent instructions for the SIMD.  One lane owns node j (j = lane, lane + 512, ...: its grid row sits in
// registers) and kGridRows batch rows at a time; u, the A action rows of W2 and W3 are wave-uniform and come from LDS as
// 16-byte broadcast reads, each feeding kGridRows nodes' worth of FMAs.  The LDS rows are zero-padded to a multiple of
// four, a padded column adds fmaf(0, 0, acc) = acc.
// max / argmax: a lane visits its nodes in ascending order and keeps a strict maximum, lanes and waves are merged by
// (larger value, then lower index) -- the lowest index among equal maxima wins, as np.max / np.argmax
// (optimal_q_network.py:157-158), whatever the merge order.
#include <limits.h>
#include <stdio.h>

#include "generic_blocks.h"
#include "optq_common.h"

namespace {

using namespace gen;

constexpr int kGridRows = 4;      // batch rows per lane in the update's grid pass
constexpr int kWaves = kThreads / 64;

__host__ __device__ inline int pad4(int n) { return (n + 3) & ~3; }

__device__ __forceinline__ void best_merge(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// per lane: running (max, lowest index) of q over this lane's nodes, for RB rows whose u sit in su[RB][L2p]
template <int A, int RB>
__device__ __forceinline__ void grid_pass_rows(const float* __restrict__ grid, int n_nodes, const float* sw3,
                                               const float* sw2a, const float* su, int L2p, float b3, float (&bv)[RB],
                                               int (&bi)[RB]) {
#pragma unroll
    for (int r = 0; r < RB; r++) { bv[r] = -INFINITY; bi[r] = INT_MAX; }
    for (int j0 = 0; j0 < n_nodes; j0 += kThreads) {
        const int j = j0 + (int)threadIdx.x;
        const int jj = min(j, n_nodes - 1);
        float a[A];
#pragma unroll
        for (int k = 0; k < A; k++) a[k] = grid[(size_t)jj * A + k];
        gf4 acc[RB];
#pragma unroll
        for (int r = 0; r < RB; r++) acc[r] = gf4{0.f, 0.f, 0.f, 0.f};
        for (int n = 0; n < L2p; n += 4) {
            const gf4 w3 = *reinterpret_cast<const gf4*>(&sw3[n]);
            gf4 wa[A];
#pragma unroll
            for (int k = 0; k < A; k++) wa[k] = *reinterpret_cast<const gf4*>(&sw2a[k * L2p + n]);
#pragma unroll
            for (int r = 0; r < RB; r++) {
                const gf4 u = *reinterpret_cast<const gf4*>(&su[r * L2p + n]);
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    float pre = u[c];
#pragma unroll
                    for (int k = 0; k < A; k++) pre = fmaf(a[k], wa[k][c], pre);
                    acc[r][c] = fmaf(w3[c], fmaxf(pre, 0.0f), acc[r][c]);
                }
            }
        }
        if (j < n_nodes) {
#pragma unroll
            for (int r = 0; r < RB; r++) {
                const float q = ((acc[r][0] + acc[r][1]) + (acc[r][2] + acc[r][3])) + b3;
                if (q > bv[r]) { bv[r] = q; bi[r] = j; }
            }
        }
    }
}

template <int RB>
__device__ inline void grid_pass(int A, const float* grid, int n_nodes, const float* sw3, const float* sw2a,
                                 const float* su, int L2p, float b3, float (&bv)[RB], int (&bi)[RB]) {
    switch (A) {
        case 1: grid_pass_rows<1, RB>(grid, n_nodes, sw3, sw2a, su, L2p, b3, bv, bi); break;
        case 2: grid_pass_rows<2, RB>(grid, n_nodes, sw3, sw2a, su, L2p, b3, bv, bi); break;
        case 3: grid_pass_rows<3, RB>(grid, n_nodes, sw3, sw2a, su, L2p, b3, bv, bi); break;
        case 4: grid_pass_rows<4, RB>(grid, n_nodes, sw3, sw2a, su, L2p, b3, bv, bi); break;
        case 5: grid_pass_rows<5, RB>(grid, n_nodes, sw3, sw2a, su, L2p, b3, bv, bi); break;
        default: grid_pass_rows<6, RB>(grid, n_nodes, sw3, sw2a, su, L2p, b3, bv, bi); break;
    }
}

// workgroup-wide merge of the lanes' (max, index) pairs; every thread returns with the result.  redv / redi: kWaves * RB
// words of LDS each.  Deterministic: the pair order (value, then lower index) is total, so the merge tree does not matter.
template <int RB>
__device__ inline void best_reduce(float (&bv)[RB], int (&bi)[RB], float* redv, int* redi) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < RB; r++)
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv[r], off, 64);
            const int oi = __shfl_xor(bi[r], off, 64);
            best_merge(bv[r], bi[r], ov, oi);
        }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < RB; r++) { redv[wave * RB + r] = bv[r]; redi[wave * RB + r] = bi[r]; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RB; r++) {
        float v = redv[r];
        int i = redi[r];
        for (int w = 1; w < kWaves; w++) best_merge(v, i, redv[w * RB + r], redi[w * RB + r]);
        bv[r] = v;
        bi[r] = i;
    }
    __syncthreads();
}

// W3 [L2] and the A action rows of W2 -> their zero-padded LDS rows
__device__ inline void stage_grid_weights(const float* P, int oW2, int oW3, int L1, int L2, int A, int L2p, float* sw3,
                                          float* sw2a) {
    for (int i = threadIdx.x; i < L2p; i += kThreads) sw3[i] = i < L2 ? P[oW3 + i] : 0.0f;
    for (int i = threadIdx.x; i < A * L2p; i += kThreads) {
        const int k = i / L2p, n = i % L2p;
        sw2a[i] = n < L2 ? P[oW2 + (size_t)(L1 + k) * L2 + n] : 0.0f;
    }
}

struct QLds {
    double *r, *g;
    long long* idx;
    float *x, *x2, *a, *q, *y, *dq, *mq;
    int* pool;
    int* dups;
    float* redv;
    int* redi;
    float *sw3, *sw2a, *su;       // the grid pass's uniform operands: [L2p], [A][L2p], [kGridRows][L2p]
};

__host__ __device__ inline size_t qlds_carve(const RlcOptqDims& d, unsigned char* base, QLds* out) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        unsigned char* p = base ? base + off : nullptr;
        off += (bytes + 15) & ~(size_t)15;
        return p;
    };
    const int B = d.B, S = d.S, A = d.A, L2p = pad4(d.L2);
    QLds L;
    L.r = (double*)take(sizeof(double) * B);
    L.g = (double*)take(sizeof(double) * B);
    L.idx = (long long*)take(sizeof(long long) * RLC_MAX_BATCH);
    L.x = (float*)take(sizeof(float) * B * S);
    L.x2 = (float*)take(sizeof(float) * B * S);
    L.a = (float*)take(sizeof(float) * B * A);
    float** pb[] = {&L.q, &L.y, &L.dq, &L.mq};
    for (auto p : pb) *p = (float*)take(sizeof(float) * B);
    L.pool = (int*)take(sizeof(int) * 3 * RLC_MAX_BATCH);
    L.dups = (int*)take(sizeof(int) * 4);
    L.redv = (float*)take(sizeof(float) * kWaves * kGridRows);
    L.redi = (int*)take(sizeof(int) * kWaves * kGridRows);
    L.sw3 = (float*)take(sizeof(float) * L2p);
    L.sw2a = (float*)take(sizeof(float) * A * L2p);
    L.su = (float*)take(sizeof(float) * kGridRows * L2p);
    if (out) *out = L;
    return off;
}

__global__ __launch_bounds__(kThreads) void rlc_optq_update_kernel(RlcOptqDev dv_arg, int first_agent, int n_updates,
                                                                   int source, const long long* host_idx, int grad_taps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the population view is read through gen::kernarg_view (generic_blocks.h), made opaque again by OQ_PHASE() at the
    // start of every phase (dv_arg is the first argument: offset 0)
    const RlcOptqDev* dvp;
#define OQ_PHASE() (dvp = kernarg_view<RlcOptqDev>())
#define dv (*dvp)
#define d (dvp->d)
    OQ_PHASE();
    const int S = d.S, A = d.A, L1 = d.L1, L2 = d.L2, B = d.B, L2p = pad4(L2);
    const int agent = first_agent + blockIdx.x, tid = threadIdx.x;
    QLds L;
    qlds_carve(d, smem, &L);
    float* th = dv.theta + (size_t)agent * d.Ppad;
    float* tt = dv.theta_t + (size_t)agent * d.Ppad;
    float* pw = dv.pw + agent * 2;
    float* sc = dv.scratch + (size_t)agent * dv.scratch_stride;
    float* h1 = sc;  sc += (size_t)B * L1;
    float* g2 = sc;  sc += (size_t)B * L2;      // u' of the target prelude, then the online second layer
    float* d2 = sc;  sc += (size_t)B * L2;
    float* dh1 = sc; sc += (size_t)B * L1;
    float* tapg = grad_taps ? dv.tap_g + (size_t)agent * d.Ppad : nullptr;

    for (int u = 0; u < n_updates; u++) {
        // ---- sample + gather (utils/replaybuffer.py:32-37) ----
        OQ_PHASE();
        const RlcRingMeta ring = dv.rep.ring[agent];
        rlc_pick_indices<kThreads>(dv.rep, agent, ring, source, B, host_idx, (size_t)blockIdx.x * n_updates + u, L.pool, L.idx,
                                   L.dups);
        OQ_PHASE();
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
        // ---- target prelude: h1' and u' = b2' + h1' . W2'[:L1] once per next state ----
        OQ_PHASE();
        blk_dense(L.x2, S, S, nullptr, 0, tt + d.W1, tt + d.b1, L1, h1, L1, B, 1);
        stage_grid_weights(tt, d.W2, d.W3, L1, L2, A, L2p, L.sw3, L.sw2a);
        __syncthreads();
        blk_dense(h1, L1, L1, nullptr, 0, tt + d.W2, tt + d.b2, L2, g2, L2, B, 0);
        __syncthreads();
        // ---- grid-max pass: max_j Q'(s'_b, grid_j), kGridRows rows of the batch at a time ----
        OQ_PHASE();
        {
            const float b3t = tt[d.b3];
            const float* grid = dv.grid;
            const int n_nodes = dv.n_nodes;
            for (int b0 = 0; b0 < B; b0 += kGridRows) {
                for (int i = tid; i < kGridRows * L2p; i += kThreads) {
                    const int r = i / L2p, n = i % L2p;
                    L.su[i] = n < L2 ? g2[(size_t)min(b0 + r, B - 1) * L2 + n] : 0.0f;
                }
                __syncthreads();
                float bv[kGridRows];
                int bi[kGridRows];
                grid_pass<kGridRows>(A, grid, n_nodes, L.sw3, L.sw2a, L.su, L2p, b3t, bv, bi);
                best_reduce<kGridRows>(bv, bi, L.redv, L.redi);
#pragma unroll
                for (int r = 0; r < kGridRows; r++) {
                    const int b = b0 + r;
                    if (tid == r && b < B) {
                        const int jb = bi[r] < n_nodes ? bi[r] : 0;       // (no finite or infinite maximum: all NaN)
                        L.mq[b] = bv[r];
                        dv.tap_maxq[(size_t)agent * RLC_MAX_BATCH + b] = bv[r];
                        for (int k = 0; k < A; k++)
                            dv.tap_astar[((size_t)agent * RLC_MAX_BATCH + b) * A + k] = grid[(size_t)jb * A + k];
                    }
                }
            }
        }
        __syncthreads();
        // ---- the float64 TD glue (agents/OptimalQ.py:79-83), fed as fp32 (optimal_q_network.py:55) ----
        OQ_PHASE();
        for (int b = tid; b < B; b += kThreads) {
            const float y = (float)(L.r[b] + L.g[b] * (double)L.mq[b]);
            L.y[b] = y;
            dv.tap_y[(size_t)agent * RLC_MAX_BATCH + b] = y;
        }
        // ---- online forward on (s, a) ----
        blk_dense(L.x, S, S, nullptr, 0, th + d.W1, th + d.b1, L1, h1, L1, B, 1);
        __syncthreads();
        blk_dense(h1, L1, L1, L.a, A, th + d.W2, th + d.b2, L2, g2, L2, B, 1);
        __syncthreads();
        blk_dense(g2, L2, L2, nullptr, 0, th + d.W3, th + d.b3, 1, L.q, 1, B, 0);
        __syncthreads();
        // ---- MSE backward with the pre-step weights ----
        OQ_PHASE();
        for (int b = tid; b < B; b += kThreads) {
            dv.tap_q[(size_t)agent * RLC_MAX_BATCH + b] = L.q[b];
            L.dq[b] = 2.0f * (L.q[b] - L.y[b]) / (float)B;              // d mean((y-q)^2) / dq
        }
        __syncthreads();
        for (int it = tid; it < B * L2; it += kThreads) {
            const int b = it / L2, n = it % L2;
            d2[it] = g2[it] > 0.0f ? L.dq[b] * th[d.W3 + n] : 0.0f;
        }
        __syncthreads();
        blk_dense_bwd_input(d2, L2, th + d.W2, h1, L1, dh1, B);
        __syncthreads();
        // ---- gradients + one Adam over the six tensors (optimal_q_network.py:57) ----
        OQ_PHASE();
        {
            const AdamCtx c = {th, dv.m + (size_t)agent * d.Ppad, dv.v + (size_t)agent * d.Ppad,
                               adam_alpha(dv.lr[agent], pw[0], pw[1]), tapg};
            blk_dense_grad_adam(g2, L2, L2, nullptr, 0, L.dq, 1, B, c, d.W3, d.b3);
            blk_dense_grad_adam(h1, L1, L1, L.a, A, d2, L2, B, c, d.W2, d.b2);
            OQ_PHASE();
            blk_dense_grad_adam(L.x, S, S, nullptr, 0, dh1, L1, B, c, d.W1, d.b1);
        }
        __syncthreads();
        // ---- Polyak (optimal_q_network.py:64-65) ----
        OQ_PHASE();
        if (tid == 0) { pw[0] *= 0.9f; pw[1] *= 0.999f; }
        for (int p = tid; p < d.Pdev; p += kThreads) {
            const float t = tt[p];
            tt[p] = t + dv.tau * (th[p] - t);
        }
        __syncthreads();
    }
#undef OQ_PHASE
#undef dv
#undef d
}

// LDS of the one-row kernels: x [S + A], h1 [L1], u [L2p], W3 [L2p], action rows [A][L2p], reduction words
struct QRowLds { float *x, *h1, *su, *sw3, *sw2a, *redv; int* redi; };
__host__ __device__ inline size_t qrow_carve(const RlcOptqDims& d, float* base, QRowLds* out) {
    const int L2p = pad4(d.L2);
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 3) & ~(size_t)3; return p; };
    QRowLds L;
    L.x = take(d.S + d.A); L.h1 = take(d.L1); L.su = take(L2p); L.sw3 = take(L2p); L.sw2a = take((size_t)d.A * L2p);
    L.redv = take(kWaves + 8); L.redi = (int*)take(kWaves);
    if (out) *out = L;
    return off * sizeof(float);
}

// h1 and u = b2 + h1 . W2[:L1] of the row in L.x (online network), and the grid pass's weight rows
__device__ inline void optq_row_prelude(const RlcOptqDims& d, const float* th, const QRowLds& L) {
    const int L2p = pad4(d.L2);
    __syncthreads();
    rlc_hidden_forward_row(th + d.W1, 0, th + d.b1, L.x, d.S, d.L1, L.h1, true);
    stage_grid_weights(th, d.W2, d.W3, d.L1, d.L2, d.A, L2p, L.sw3, L.sw2a);
    for (int i = d.L2 + threadIdx.x; i < L2p; i += kThreads) L.su[i] = 0.0f;
    __syncthreads();
    rlc_hidden_forward_row(th + d.W2, 0, th + d.b2, L.h1, d.L1, d.L2, L.su, false);
    __syncthreads();
}

// greedy grid row (+ its Q) of the ONLINE network for one state per agent: get_max_action(use_target=False)
// (optimal_q_network.py:121-161; agents/OptimalQ.py:28-30).  done_flag (or null): a word in host-visible memory that
// receives done_val once the launch's outputs are stored (rlc_optq_act_queue; see rlc_ddpg_act_kernel)
__global__ __launch_bounds__(kThreads) void rlc_optq_act_kernel(RlcOptqDev dv, int first_agent, const float* states,
                                                                float* action_out, float* q_out, int* done_flag,
                                                                int done_val) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RlcOptqDims& d = dv.d;
    const int S = d.S, A = d.A;
    const int agent = first_agent + blockIdx.x, tid = threadIdx.x;
    QRowLds L;
    qrow_carve(d, (float*)smem, &L);
    const float* th = dv.theta + (size_t)agent * d.Ppad;
    for (int i = tid; i < S; i += kThreads)
        L.x[i] = clip_state_val(states[(size_t)blockIdx.x * S + i], dv.clip_state, dv.smin[i], dv.smax[i]);
    optq_row_prelude(d, th, L);
    float bv[1];
    int bi[1];
    grid_pass<1>(A, dv.grid, dv.n_nodes, L.sw3, L.sw2a, L.su, pad4(d.L2), th[d.b3], bv, bi);
    best_reduce<1>(bv, bi, L.redv, L.redi);
    if (tid == 0) {
        const int jb = bi[0] < dv.n_nodes ? bi[0] : 0;
        for (int k = 0; k < A; k++) action_out[(size_t)blockIdx.x * A + k] = dv.grid[(size_t)jb * A + k];
        q_out[blockIdx.x] = bv[0];
        if (done_flag) {
            __threadfence_system();                     // the output stores first
            __hip_atomic_store(done_flag, done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// Q(s,a) rows on one agent's online network (getQFunction, optimal_q_network.py:193-196).  One workgroup per row; the
// sum over the second layer's units is split over the threads (fixed order: deterministic).
__global__ __launch_bounds__(kThreads) void rlc_optq_qval_kernel(RlcOptqDev dv, int agent, const float* states,
                                                                 const float* actions, float* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RlcOptqDims& d = dv.d;
    const int S = d.S, A = d.A, L2 = d.L2, L2p = pad4(L2);
    const int tid = threadIdx.x, row = blockIdx.x;
    QRowLds L;
    qrow_carve(d, (float*)smem, &L);
    const float* th = dv.theta + (size_t)agent * d.Ppad;
    for (int i = tid; i < S; i += kThreads)
        L.x[i] = clip_state_val(states[(size_t)row * S + i], dv.clip_state, dv.smin[i], dv.smax[i]);
    for (int k = tid; k < A; k += kThreads) L.x[S + k] = actions[(size_t)row * A + k];
    optq_row_prelude(d, th, L);
    float part = 0.0f;
    for (int n = tid; n < L2; n += kThreads) {
        float pre = L.su[n];
        for (int k = 0; k < A; k++) pre = fmaf(L.x[S + k], L.sw2a[k * L2p + n], pre);
        part = fmaf(L.sw3[n], fmaxf(pre, 0.0f), part);
    }
    const float q = blk_sum(part, L.redv);
    if (tid == 0) out[row] = q + th[d.b3];
}

}  // namespace

size_t rlc_optq_scratch_floats(const RlcOptqDims& d) { return (size_t)d.B * 2 * ((size_t)d.L1 + (size_t)d.L2); }

const char* rlc_optq_refusal(const RlcOptqDims& d) {
    static thread_local char msg[160];
    const size_t up = qlds_carve(d, nullptr, nullptr), row = qrow_carve(d, nullptr, nullptr);
    const size_t need = up > row ? up : row;
    if (need <= 64 * 1024) return nullptr;
    snprintf(msg, sizeof(msg), "layer widths %d / %d need %zu B of LDS for the grid pass (> 65536)", d.L1, d.L2, need);
    return msg;
}

int rlc_launch_optq_update(const RlcOptqDev& dv, int first_agent, int n_agents, int n_updates, int source,
                           const long long* idx_dev, int grad_taps, hipStream_t st) {
    const size_t lds = qlds_carve(dv.d, nullptr, nullptr);
    RLC_REQUIRE(lds <= 64 * 1024, "OptimalQ kernel needs %zu B of LDS (> 64 KiB)", lds);
    hipLaunchKernelGGL(rlc_optq_update_kernel, dim3(n_agents), dim3(kThreads), lds, st, dv, first_agent, n_updates, source,
                       idx_dev, grad_taps);
    RLC_HIP(hipGetLastError());
    return 0;
}

int rlc_launch_optq_act(const RlcOptqDev& dv, int first_agent, int n, const float* states_dev, float* action_dev,
                        float* q_dev, hipStream_t st, int* done_flag, int done_val) {
    const size_t lds = qrow_carve(dv.d, nullptr, nullptr);
    RLC_REQUIRE(lds <= 64 * 1024, "OptimalQ acting kernel needs %zu B of LDS (> 64 KiB)", lds);
    RLC_REQUIRE(done_flag == nullptr || n == 1, "a completion flag needs a one-workgroup acting launch");
    hipLaunchKernelGGL(rlc_optq_act_kernel, dim3(n), dim3(kThreads), lds, st, dv, first_agent, states_dev, action_dev,
                       q_dev, done_flag, done_val);
    RLC_HIP(hipGetLastError());
    return 0;
}

int rlc_launch_optq_qval(const RlcOptqDev& dv, int agent, int n, const float* states_dev, const float* actions_dev,
                         float* out_dev, hipStream_t st) {
    const size_t lds = qrow_carve(dv.d, nullptr, nullptr);
    RLC_REQUIRE(lds <= 64 * 1024, "OptimalQ Q-value kernel needs %zu B of LDS (> 64 KiB)", lds);
    hipLaunchKernelGGL(rlc_optq_qval_kernel, dim3(n), dim3(kThreads), lds, st, dv, agent, states_dev, actions_dev, out_dev);
    RLC_HIP(hipGetLastError());
    return 0;
}
