// ddpg_ln_mfma_kernel.h -- the fused DDPG update with norm_type 'layer' on the gfx950 fp32 matrix cores.
//
// Same contract as rlc_ddpg_update_mfma_kernel (ddpg_mfma_kernel.h): one 512-thread workgroup per agent, n_updates
// sequential updates per launch, sample / gather / the whole update_network, the same taps, fixed-order reductions.
// Arithmetic and order are those of ddpg_generic.hip with NORM.
//
// What layer norm changes: d(hidden) of a normalised layer is no rank-NS product mask * (seed . w_out) any more --
//   dy = dh * [gamma*xhat + beta > 0],  g = dy * gamma,  dz = rstd * (g - mean_n g - xhat * mean_n(g * xhat))
// is full rank, and it is the A operand of the backward-to-input GEMM and an operand of the weight-gradient GEMM.  So the
// kernel keeps a SECOND activation-sized image in LDS next to hbuf: it holds xhat of the layer being differentiated
// and is overwritten in place by dz once the row scalars are known (ln_bwd_rows).  There are no mask bytes: with xhat in
// LDS a relu mask is the sign of gamma*xhat + beta where dz is formed.
//
//   forward, second layers   accumulators -> + bias (+ action rows) -> ln_acc: per-row mean, then the centred sum of
//                            squares (two passes, as the oracle does), summed over the eight waves' N tiles through
//                            `part` in a fixed order -> xhat in the accumulators (-> the image where the backward needs
//                            it) -> relu(gamma*xhat + beta) -> the output layer's row_dot
//   forward, first layer     the VALU pass trunk_z over S <= 8 inputs + one wave per row (ln_rows), in hbuf in place
//   backward, second layers  column pass (gamma / beta / output-layer gradients) -> ln_bwd_rows (xhat -> dz in place) ->
//                            column pass (bias gradient, Adam on the small tensors) -> bwd_gemm_img (dz . W^T, W before
//                            its step) -> wgrad_adam_img (Adam + Polyak in the epilogue)
//   backward, first layer    dh1 leaves the accumulators for the agent's slice of the any-shape kernel's scratch (both
//                            images are still operands of the weight-gradient GEMM; B x H1 floats, L2-resident), xhat1
//                            is RECOMPUTED into the second image once the second layer's dz is dead (a trunk pass, not
//                            a GEMM), then ln_bwd_rows and the first-layer column pass
//
// Scope: the hydra network (d.sep == 0), S <= 8, A <= 2, widths multiples of 4 in [16, 256], batch <= 128; the two-pass
// forward (no FUSE), the padded last tile (no tail-of-four).
//
// On-device experiment loop: with a rollout attached, one training step (rlc_train_step_device) opens every iteration of
// the update loop, as in rlc_ddpg_update_mfma_kernel.  That kernel lends the step its activation image; here both images,
// `stat` and the per-sample vectors are zeroed ONCE per launch and their rows >= B / columns >= N are relied on to stay
// zero, so the step gets the stretch of LDS from `part` to the end of `idx` instead (ln_step_scratch_floats): every float
// of it is written before it is read in every update, and none of its padding is ever read.
#pragma once
#include "ddpg_mfma_kernel.h"

namespace {

using namespace mfb;

#define RLC_LN_MFMA_EPS 1e-12f

struct SmemLn {
    lds_f32* hbuf;      // [MB][ldh_for(H1)] + 16
    lds_f32* img;       // [MB][ldh_for(max width)] + 16: xhat, then dz, of the layer being differentiated
    lds_f32* stat;      // [6][MB] per-row scalars: mean, rstd (first layer), rstd (second layer), rstd (Q at pi), mean g, mean g*xhat
    lds_f32* part;      // [kWaves][MB][2]
    lds_f32 *x, *x2, *a, *aout, *mu, *dz, *q, *y, *dq;
    lds_f64 *r, *g;
    lds_i64* idx;
    lds_i32* pool;
    lds_i32* dups;
    lds_f32x4* xbuf;    // hand-off of the split 13th tile, or null: no layer has 13 tiles
};

__host__ __device__ inline int ln_img_width(const RlcDims& d) {
    const int m = d.HA > d.HC ? d.HA : d.HC;
    return d.H1 > m ? d.H1 : m;
}

// carve the dynamic LDS of the layer-norm form; base may be null (host: only the size is wanted)
__host__ __device__ inline size_t smem_carve_ln(const RlcDims& d, int MT, lds_u8* base, SmemLn* out) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        lds_u8* p = base + off;
        off += (bytes + 15) & ~(size_t)15;
        return p;
    };
    const int MB = MT * 16, A = d.A;
    SmemLn L;
    // + 16 floats of tail: the unmasked fragment reads of the last k-chunk run up to 15 floats past a row's end
    L.hbuf = (lds_f32*)take(sizeof(float) * (MB * ldh_for(d.H1) + 16));
    L.img = (lds_f32*)take(sizeof(float) * (MB * ldh_for(ln_img_width(d)) + 16));
    L.stat = (lds_f32*)take(sizeof(float) * 6 * MB);
    L.part = (lds_f32*)take(sizeof(float) * kWaves * MB * 2);
    L.r = (lds_f64*)take(sizeof(double) * MB);
    L.g = (lds_f64*)take(sizeof(double) * MB);
    L.idx = (lds_i64*)take(sizeof(long long) * RLC_MAX_BATCH);
    L.x = (lds_f32*)take(sizeof(float) * MB * SMAX);
    L.x2 = (lds_f32*)take(sizeof(float) * MB * SMAX);
    L.a = (lds_f32*)take(sizeof(float) * MB * A);
    L.aout = (lds_f32*)take(sizeof(float) * MB * A);
    L.mu = (lds_f32*)take(sizeof(float) * MB * A);
    L.dz = (lds_f32*)take(sizeof(float) * MB * A);
    L.q = (lds_f32*)take(sizeof(float) * MB);
    L.y = (lds_f32*)take(sizeof(float) * MB);
    L.dq = (lds_f32*)take(sizeof(float) * MB);
    L.pool = (lds_i32*)take(sizeof(int) * 3 * RLC_MAX_BATCH);
    L.dups = (lds_i32*)take(sizeof(int) * 4);
    auto t13 = [](int n) { return (n + 15) >> 4 == 13; };
    if (t13(d.H1) || t13(d.HA) || t13(d.HC)) L.xbuf = (lds_f32x4*)take(sizeof(float) * 4 * 64 * (MT - (MT + 3) / 4));
    else L.xbuf = nullptr;
    if (out) *out = L;
    return off;
}

// LDS lent to the on-device training step: `part`, `r`, `g` and `idx`, contiguous in the carve above.  All four are dead
// at the top of an update and nobody relies on what they hold past their live rows: row_reduce / row_dot store every
// (wave, row) partial that row_stat / part_sum read; the gather stores r[b], g[b] and the sampler (or the host-index copy)
// idx[b] for every b < B, and nothing reads them at b >= B.  16 MB + 4 MB + 2 RLC_MAX_BATCH floats (MB = 16 MT): 896 at two
// tiles, against at most 564 the step needs (ddpg_policy_lds_floats + 4 at 256-wide layers).
__host__ __device__ inline size_t ln_step_scratch_floats(int MT) {
    const size_t MB = (size_t)MT * 16;
    return (sizeof(float) * kWaves * MB * 2 + 2 * sizeof(double) * MB + sizeof(long long) * RLC_MAX_BATCH) / sizeof(float);
}

__device__ __forceinline__ float ln_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Blk plus the layer-norm blocks.  A derived struct, not new members of Blk: no existing instantiation sees any of it.
template <int MT>
struct LnBlk : Blk<MT, NTW, MSTRIDE> {
    using Base = Blk<MT, NTW, MSTRIDE>;
    static constexpr int MB = Base::MB;
    static constexpr int MXS = Base::MXS;
    using Base::tid; using Base::lane; using Base::wave; using Base::c; using Base::g;
    using Base::S; using Base::H1; using Base::B; using Base::LDH; using Base::L;
    using typename Base::WgPre;

    lds_f32* img;       // the second image
    int LD2;            // its leading dimension
    lds_f32* part;

    // hbuf[b][k] = b1[k] + sum_i xs[b][i] W1[i][k]: Blk::trunk_t without its relu (rows >= B and columns >= H1 zeroed)
    __device__ __forceinline__ void trunk_z(const float* W1, const float* b1, const lds_f32* xs) {
        for (int q = lane; 4 * q < LDH; q += 64) {
            f32x4 w[SMAX], bias;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int k = 4 * q + e;
                const bool live = k < H1;
#pragma unroll
                for (int i = 0; i < SMAX; i++) w[i][e] = (live && i < S) ? W1[i * H1 + k] : 0.0f;
                bias[e] = live ? b1[k] : 0.0f;
            }
            const bool live4[4] = {4 * q < H1, 4 * q + 1 < H1, 4 * q + 2 < H1, 4 * q + 3 < H1};
#pragma unroll 2
            for (int b = wave; b < MB; b += kWaves) {
                const f32x4 x0 = *reinterpret_cast<const lds_f32x4*>(&xs[b * SMAX]);
                const f32x4 x1 = *reinterpret_cast<const lds_f32x4*>(&xs[b * SMAX + 4]);
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; i++) acc += x0[i] * w[i];
#pragma unroll
                for (int i = 0; i < 4; i++) acc += x1[i] * w[4 + i];
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; e++) o[e] = (live4[e] && b < B) ? acc[e] + bias[e] : 0.0f;
                *reinterpret_cast<lds_f32x4*>(&L.hbuf[b * LDH + 4 * q]) = o;
            }
        }
    }

    // the first layer's norm, in hbuf in place: one wave per row, lane l holds features l, l + 64, ... (the any-shape
    // kernel's blk_layernorm_relu).  KEEP: xhat goes to the second image and rstd to rs (the backward needs them).
    template <bool KEEP>
    __device__ __forceinline__ void ln_rows(const float* beta, const float* gamma, lds_f32* rs) {
        float gm[4], bt[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int n = lane + 64 * i;
            gm[i] = n < H1 ? gamma[n] : 0.0f;
            bt[i] = n < H1 ? beta[n] : 0.0f;
        }
        for (int r = wave; r < B; r += kWaves) {
            lds_f32* z = L.hbuf + r * LDH;
            float zv[4], s = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int n = lane + 64 * i;
                zv[i] = n < H1 ? z[n] : 0.0f;
                s += zv[i];
            }
            const float mean = ln_wave_sum(s) / (float)H1;
            float q = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float cz = zv[i] - mean;
                q += lane + 64 * i < H1 ? cz * cz : 0.0f;
            }
            const float rsd = 1.0f / sqrtf(ln_wave_sum(q) / (float)H1 + RLC_LN_MFMA_EPS);
            if (KEEP && lane == 0) rs[r] = rsd;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int n = lane + 64 * i;
                if (n < H1) {
                    const float nh = (zv[i] - mean) * rsd;
                    if (KEEP) img[r * LD2 + n] = nh;
                    z[n] = fmaxf(nh * gm[i] + bt[i], 0.0f);
                }
            }
        }
    }

    // acc = acc + bias[n] + sum_j E[b][j] * Wx[xrow0+j][n] (Blk::bias_relu without its relu); columns >= N zeroed
    template <int NE>
    __device__ __forceinline__ void bias_add(f32x4 (&acc)[MT][NTW], const float* bias, int N, const lds_f32* E = nullptr,
                                             const float* Wx = nullptr, int xrow0 = 0) {
        const int NT = (N + 15) >> 4;
#pragma unroll
        for (int i = 0; i < NTW; i++) {
            const int t = this->tile_of(i);
            const int n = 16 * t + c;
            const bool ok = t < NT && n < N;
            const float bs = ok ? bias[n] : 0.0f;
            float wx[NE > 0 ? NE : 1];
#pragma unroll
            for (int j = 0; j < NE; j++) wx[j] = ok ? Wx[rlc_blk_index(xrow0 + j, n, N)] : 0.0f;
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float v = acc[mt][i][r] + bs;
                    if (NE > 0) {
                        const int b = 16 * mt + 4 * g + r;
#pragma unroll
                        for (int j = 0; j < NE; j++) v += E[b * NE + j] * wx[j];
                    }
                    acc[mt][i][r] = ok ? v : 0.0f;
                }
        }
    }

    // part[wave][b][j] = sum over this wave's valid columns of what fn adds into p[0..NJ): fn(value, n, b, i, p)
    template <int NJ, class F>
    __device__ __forceinline__ void row_reduce(const f32x4 (&acc)[MT][NTW], int N, F fn) {
        const int NT = (N + 15) >> 4;
        bool ok[NTW];
        int nn[NTW];
#pragma unroll
        for (int i = 0; i < NTW; i++) {
            const int t = this->tile_of(i);
            nn[i] = 16 * t + c;
            ok[i] = t < NT && nn[i] < N;
            if (!ok[i]) nn[i] = 0;
        }
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int b = 16 * mt + 4 * g + r;
                float p[NJ];
#pragma unroll
                for (int j = 0; j < NJ; j++) p[j] = 0.0f;
#pragma unroll
                for (int i = 0; i < NTW; i++) {
                    float e[NJ];
#pragma unroll
                    for (int j = 0; j < NJ; j++) e[j] = 0.0f;
                    fn(acc[mt][i][r], nn[i], b, i, e);
#pragma unroll
                    for (int j = 0; j < NJ; j++) p[j] += ok[i] ? e[j] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < NJ; j++) {
                    const float s = row16_sum(p[j]);
                    if (c == 0) part[((size_t)wave * MB + b) * NJ + j] = s;
                }
            }
    }
    // dst[b] = f(fixed-order sum of the waves' partials j of row b), every row; ends behind a barrier
    template <int NJ, class F>
    __device__ __forceinline__ void row_stat(int j, lds_f32* dst, F f) {
        __syncthreads();
        for (int b = tid; b < MB; b += kThreads) dst[b] = f(this->template part_sum<NJ>(part, b, j));
        __syncthreads();
    }

    // the LN epilogue of forward accumulators: acc (the layer's linear output, columns >= N zero) -> xhat, rstd -> rs
    __device__ __forceinline__ void ln_acc(f32x4 (&acc)[MT][NTW], int N, lds_f32* mean, lds_f32* rs) {
        const int NT = (N + 15) >> 4;
        row_reduce<1>(acc, N, [](float v, int, int, int, float (&e)[1]) { e[0] = v; });
        row_stat<1>(0, mean, [&](float s) { return s / (float)N; });
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const f32x4 m4 = *reinterpret_cast<const lds_f32x4*>(&mean[16 * mt + 4 * g]);
#pragma unroll
            for (int i = 0; i < NTW; i++) {
                const int t = this->tile_of(i);
                const bool ok = t < NT && 16 * t + c < N;
#pragma unroll
                for (int r = 0; r < 4; r++) acc[mt][i][r] = ok ? acc[mt][i][r] - m4[r] : 0.0f;
            }
        }
        row_reduce<1>(acc, N, [](float v, int, int, int, float (&e)[1]) { e[0] = v * v; });
        row_stat<1>(0, rs, [&](float s) { return 1.0f / sqrtf(s / (float)N + RLC_LN_MFMA_EPS); });
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const f32x4 r4 = *reinterpret_cast<const lds_f32x4*>(&rs[16 * mt + 4 * g]);
#pragma unroll
            for (int i = 0; i < NTW; i++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[mt][i][r] *= r4[r];
        }
    }

    // xhat accumulators -> the second image (rows >= B and columns >= N stay zero)
    __device__ __forceinline__ void store_img(const f32x4 (&acc)[MT][NTW], int N) {
        const int NT = (N + 15) >> 4;
#pragma unroll
        for (int i = 0; i < NTW; i++) {
            const int t = this->tile_of(i);
            const int n = 16 * t + c;
            if (t < NT && n < N) {
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int b = 16 * mt + 4 * g + r;
                        if (b < B) img[b * LD2 + n] = acc[mt][i][r];
                    }
            }
        }
    }
    // acc = relu(gamma * xhat + beta); columns >= N zeroed
    __device__ __forceinline__ void ln_act(f32x4 (&acc)[MT][NTW], int N, const float* beta, const float* gamma) {
        const int NT = (N + 15) >> 4;
#pragma unroll
        for (int i = 0; i < NTW; i++) {
            const int t = this->tile_of(i);
            const int n = 16 * t + c;
            const bool ok = t < NT && n < N;
            const float gm = ok ? gamma[n] : 0.0f, bt = ok ? beta[n] : 0.0f;
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[mt][i][r] = ok ? fmaxf(acc[mt][i][r] * gm + bt, 0.0f) : 0.0f;
        }
    }

    // layer-norm backward of the image's rows, in place: xhat -> dz = rstd * (g - mean g - xhat * mean(g * xhat)),
    // g = [gamma*xhat + beta > 0] * up(r, n, i) * gamma.  One wave per row, lane l holds features l + 64 i.
    template <class UP>
    __device__ __forceinline__ void ln_bwd_rows(int N, const float* beta, const float* gamma, const lds_f32* rs, UP up) {
        float gm[4], bt[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int n = lane + 64 * i;
            gm[i] = n < N ? gamma[n] : 0.0f;
            bt[i] = n < N ? beta[n] : 0.0f;
        }
        for (int r = wave; r < B; r += kWaves) {
            lds_f32* row = img + r * LD2;
            float xh[4], gq[4], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int n = lane + 64 * i;
                const bool ok = n < N;
                xh[i] = ok ? row[n] : 0.0f;
                const float u = up(r, ok ? n : 0, i);
                gq[i] = (ok && xh[i] * gm[i] + bt[i] > 0.0f) ? u * gm[i] : 0.0f;
                s1 += gq[i];
                s2 += gq[i] * xh[i];
            }
            const float m1 = ln_wave_sum(s1) / (float)N, m2 = ln_wave_sum(s2) / (float)N, rsd = rs[r];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int n = lane + 64 * i;
                if (n < N) row[n] = rsd * (gq[i] - m1 - xh[i] * m2);
            }
        }
    }

    // ---------------------------------------------------------------------------------------
    // backward-to-input GEMM whose A operand is the dz image: acc[b][k'] = sum_n img[b][n] * W[k'][n].  Blk::bwd_loop
    // with four floats of the image (one ds_read_b128 per M tile per chunk) where it has four mask bytes times a seed;
    // the weight stream, the 13-tile split and the 8-float tail are the same.
    // ---------------------------------------------------------------------------------------
    template <int NOWN, int XMODE>
    __device__ __forceinline__ void bwd_loop_img(f32x4 (&acc)[MT][NTW], const float* W, int NTk, bool tail8, int NTblk,
                                                 f32x4 (&accx)[MXS], int xt, int xm0) {
        constexpr bool XTRA = XMODE != 0;
        const float* wp = W + (((size_t)this->tile0() * NTblk) << 8) + (lane << 2);
        const size_t tst = ((size_t)this->tstep() * NTblk) << 8;
        const lds_f32* ap = img + c * LD2 + 4 * g;
        const float* wpx = W + (((size_t)xt * NTblk) << 8) + (lane << 2);
        const lds_f32* apx[MXS];
#pragma unroll
        for (int m = 0; m < MXS; m++) apx[m] = ap + 16 * (xm0 + m < MT ? xm0 + m : xm0) * LD2;
        f32x4 b0[NOWN], b1[NOWN], bx0 = {0.f, 0.f, 0.f, 0.f}, bx1 = {0.f, 0.f, 0.f, 0.f};
        auto loadB = [&](f32x4 (&dst)[NOWN], f32x4& dx, int ch) {
#pragma unroll
            for (int i = 0; i < NOWN; i++) dst[i] = *reinterpret_cast<const f32x4*>(wp + i * tst + ((size_t)ch << 8));
            if (XTRA) dx = *reinterpret_cast<const f32x4*>(wpx + ((size_t)ch << 8));
        };
        auto mac = [&](const f32x4 (&b)[NOWN], const f32x4& bx, int ch) {
            f32x4 av[MT];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) av[mt] = *reinterpret_cast<const lds_f32x4*>(ap + 16 * mt * LD2 + 16 * ch);
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int i = 0; i < NOWN; i++)
#pragma unroll
                    for (int mt = 0; mt < MT; mt++) acc[mt][i] = mfma16(av[mt][s], b[i][s], acc[mt][i]);
            if (XTRA) {
#pragma unroll
                for (int m = 0; m < MXS; m++) {
                    const f32x4 ax = *reinterpret_cast<const lds_f32x4*>(apx[m] + 16 * ch);
#pragma unroll
                    for (int s = 0; s < 4; s++) accx[m] = mfma16(ax[s], bx[s], accx[m]);
                }
            }
        };
        loadB(b0, bx0, 0);
        int ch = 0;
        for (; ch + 2 <= NTk; ch += 2) {
            loadB(b1, bx1, ch + 1);
            mac(b0, bx0, ch);
            loadB(b0, bx0, ch + 2 < NTk ? ch + 2 : NTk - 1);
            mac(b1, bx1, ch + 1);
        }
        if (ch < NTk) mac(b0, bx0, ch);
        if (tail8) {
            // row length = 16 NTk + 8: lane group g takes n = 16 NTk + 2g + s (Blk::bwd_loop's tail)
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            const int tofs = ((((g >> 1) << 4) + c) << 2) + 2 * (g & 1);
            const float* wt = W + (((size_t)this->tile0() * NTblk + NTk) << 8) + tofs;
            const int kofs = 16 * NTk + 2 * g - 4 * g;              // relative to ap (which carries + 4g)
            f32x2 bt[NOWN];
#pragma unroll
            for (int i = 0; i < NOWN; i++) bt[i] = *reinterpret_cast<const f32x2*>(wt + i * tst);
            f32x2 av[MT];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) av[mt] = *reinterpret_cast<const RLC_LDS f32x2*>(ap + 16 * mt * LD2 + kofs);
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
                for (int i = 0; i < NOWN; i++)
#pragma unroll
                    for (int mt = 0; mt < MT; mt++) acc[mt][i] = mfma16(av[mt][s2], bt[i][s2], acc[mt][i]);
            if (XTRA) {
                const f32x2 btx = *reinterpret_cast<const f32x2*>(W + (((size_t)xt * NTblk + NTk) << 8) + tofs);
#pragma unroll
                for (int m = 0; m < MXS; m++) {
                    const f32x2 ax = *reinterpret_cast<const RLC_LDS f32x2*>(apx[m] + kofs);
#pragma unroll
                    for (int s2 = 0; s2 < 2; s2++) accx[m] = mfma16(ax[s2], btx[s2], accx[m]);
                }
            }
        }
    }

    __device__ __forceinline__ void bwd_gemm_img(f32x4 (&acc)[MT][NTW], const float* W, int Nk /* row length = k-dim */,
                                                 int Kout /* rows of W used */) {
        const int NT = (Kout + 15) >> 4;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int i = 0; i < NTW; i++) acc[mt][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int nown = this->nown_of(NT);
        const int NTblk = (Nk + 15) >> 4;
        const bool tail8 = (Nk & 15) == 8 && Nk > 16;
        const int NTk = tail8 ? Nk >> 4 : NTblk;
        f32x4 accx[MXS];
        if (this->split_mode(NT)) {                // workgroup-uniform
#pragma unroll
            for (int m = 0; m < MXS; m++) accx[m] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (wave >= 4) bwd_loop_img<1, 1>(acc, W, NTk, tail8, NTblk, accx, NT - 1, Base::share_lo(wave - 4));
            else bwd_loop_img<2, 0>(acc, W, NTk, tail8, NTblk, accx, 0, 0);
            this->template collect_split<false>(acc, accx);
        } else if (nown >= 2) bwd_loop_img<2, 0>(acc, W, NTk, tail8, NTblk, accx, 0, 0);
        else if (nown == 1) bwd_loop_img<1, 0>(acc, W, NTk, tail8, NTblk, accx, 0, 0);
    }

    // dh1 accumulators -> the agent's scratch rows [B][H1] (global)
    __device__ __forceinline__ void store_dh(const f32x4 (&acc)[MT][NTW], float* sc) {
        const int NT = (H1 + 15) >> 4;
#pragma unroll
        for (int i = 0; i < NTW; i++) {
            const int t = this->tile_of(i);
            const int k = 16 * t + c;
            if (t < NT && k < H1) {
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int b = 16 * mt + 4 * g + r;
                        if (b < B) sc[(size_t)b * H1 + k] = acc[mt][i][r];
                    }
            }
        }
    }

    // ---------------------------------------------------------------------------------------
    // weight-gradient GEMM + Adam + Polyak epilogue whose second operand is the dz image:
    //   G[k'][n] = sum_b X[b][k'] * img[b][n],  X = [hbuf | E].  Blk::wgrad_adam (same items, same transposed tiles, same
    //   prefetch of the next item's W / m / v / W' and the same epilogue) with one float of the image per k-step where it
    //   has a seed times a mask byte.
    // ---------------------------------------------------------------------------------------
    template <int NE>
    __device__ __forceinline__ void wgrad_adam_img(const lds_f32* E /* LDS [MB][NE] or null */, int N, float* Wp, float* mp,
                                                   float* vp, float alpha, float* tapp, float* Wt, float tau) {
        const int NT = (N + 15) >> 4;
        const int NMT = (H1 + 15) >> 4;
        const int nch = (NMT + 3) >> 2, cbase = NMT / nch, crem = NMT % nch;
        const int nitems = NT * nch;
        const int gperm = ((g & 1) << 1) | (g >> 1);     // 0,2,1,3
        const int lane4 = (g * 16 + c) << 2;
        auto run = [&](const WgPre& P, int idx, auto mcc_tag) {
            constexpr int MCC = decltype(mcc_tag)::value;
            int t, m0, nq;
            this->wg_item_geom(idx, N, t, m0, nq);
            f32x4 acc[MCC];
            const lds_f32* hq[MCC];
#pragma unroll
            for (int q = 0; q < MCC; q++) {
                acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                hq[q] = L.hbuf + gperm * LDH + (q < nq ? 16 * (m0 + q) : 0) + c;      // rows past the chunk alias tile 0 (never stored)
            }
            const lds_f32* dp = img + gperm * LD2 + 16 * t + c;
#pragma unroll
            for (int gi = 0; gi < MT; gi++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int row = 16 * gi + 4 * j;
                    if (gi == MT - 1 && j > 0 && row >= B) continue;          // wave-uniform: rows of zeros
                    const float df = dp[row * LD2];
#pragma unroll
                    for (int q = 0; q < MCC; q++) acc[q] = mfma16(df, hq[q][row * LDH], acc[q]);
                }
            const bool n4ok = 16 * t + 4 * g < N;
            // every prefetched register is demanded here, before the first store of the epilogue (Blk::wgrad_adam)
#pragma unroll
            for (int q = 0; q < 4; q++) asm volatile("" ::"v"(P.w[q]), "v"(P.m[q]), "v"(P.v[q]), "v"(P.t[q]));
#pragma unroll
            for (int q = 0; q < MCC; q++) {
                const int kp = 16 * (m0 + q) + c;
                f32x4 nw, nm = P.m[q], nv = P.v[q], nt;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float mm = nm[r], vv = nv[r];
                    nw[r] = this->astep_big(P.w[q][r], acc[q][r], mm, vv, alpha);
                    nm[r] = mm; nv[r] = vv;
                    nt[r] = Base::polyak(P.t[q][r], nw[r], tau);
                }
                if (q < nq && kp < H1 && n4ok) {
                    const size_t p = (((size_t)(m0 + q) * NT + t) << 8) + lane4;
                    st_stream(&mp[p], nm);
                    st_stream(&vp[p], nv);
                    *reinterpret_cast<f32x4*>(&Wp[p]) = nw;
                    st_target(&Wt[p], nt);
                    if (tapp) *reinterpret_cast<f32x4*>(&tapp[p]) = acc[q];
                }
            }
        };
        auto run_any = [&](const WgPre& P, int idx) {
            const int ch = idx / NT;
            const int nq = cbase + (ch < crem ? 1 : 0);
            if (nq == 4) run(P, idx, std::integral_constant<int, 4>{});
            else run(P, idx, std::integral_constant<int, 3>{});
        };
        auto issue = [&](WgPre& P, int idx) { this->template wg_issue<false>(P, idx, N, Wp, mp, vp, Wt, alpha); };
        WgPre PA, PB;
        int idx = wave;
        // compiler-level memory barriers pin the prefetch loads and the epilogue stores where they are written (Blk::wgrad_adam)
#define RLC_CBAR() asm volatile("" ::: "memory")
        RLC_CBAR();
        if (idx < nitems) issue(PA, idx);
        while (idx < nitems) {
            RLC_CBAR();
            if (idx + kWaves < nitems) issue(PB, idx + kWaves);
            RLC_CBAR();
            run_any(PA, idx);
            RLC_CBAR();
            idx += kWaves;
            if (idx >= nitems) break;
            if (idx + kWaves < nitems) issue(PA, idx + kWaves);
            RLC_CBAR();
            run_any(PB, idx);
            RLC_CBAR();
            idx += kWaves;
        }
#undef RLC_CBAR
        // extra rows of a concat layer: G[H1+j][n] = sum_b E[b][j] * img[b][n]; one N tile per wave at a time
        if constexpr (NE > 0) {
            for (int t = (wave + 4) & 7; t < NT; t += kWaves) {
                const int n = 16 * t + c;
                const bool nok = n < N;
                float ge[NE];
#pragma unroll
                for (int j = 0; j < NE; j++) ge[j] = 0.0f;
                for (int bb = 0; bb < MT * 4; bb++) {
                    const int b = 4 * bb + g;
                    const float dd = img[b * LD2 + 16 * t + c];
#pragma unroll
                    for (int j = 0; j < NE; j++) ge[j] += E[b * NE + j] * dd;
                }
#pragma unroll
                for (int j = 0; j < NE; j++) {
                    const float gr = col4_sum(ge[j]);
                    if (g == j && nok) {
                        const size_t p = rlc_blk_index(((H1 + 15) & ~15) + j, n, N);   // first extra block row + j
                        float mm = mp[p], vv = vp[p];
                        const float o = Wt[p];
                        const float nv = this->astep_small(Wp[p], gr, mm, vv, alpha);
                        mp[p] = mm; vp[p] = vv; Wp[p] = nv;
                        if (tapp) tapp[p] = gr;
                        Wt[p] = Base::polyak(o, nv, tau);
                    }
                }
            }
        }
    }
};

template <int MT, int AD>
__global__ __launch_bounds__(kThreads) void rlc_ddpg_update_ln_mfma_kernel(RlcDev dv, int first_agent, int n_updates,
                                                                           int source, const long long* host_idx,
                                                                           int grad_taps, const RlcRollout* rollout,
                                                                           int q8_first) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using U = LnBlk<MT>;
    static_assert(AD <= 2, "the layer-norm form takes action_dim <= 2");
    constexpr int MB = U::MB;
    const RlcDims d = dv.d;
    U u;
    u.init_geometry();
    u.S = d.S; u.H1 = d.H1; u.B = d.B; u.LDH = ldh_for(d.H1);
    SmemLn L;
    smem_carve_ln(d, MT, (lds_u8*)smem, &L);
    u.L.hbuf = L.hbuf; u.L.mask = nullptr; u.L.xbuf = L.xbuf;
    u.img = L.img; u.LD2 = ldh_for(ln_img_width(d)); u.part = L.part;
    const int LD2 = u.LD2;
    const int tid = u.tid, S = d.S, H1 = d.H1, HA = d.HA, HC = d.HC, B = d.B;
    const int agent = first_agent + blockIdx.x;
    lds_f32* st_mean = L.stat;            // scratch of ln_acc
    lds_f32* st_rs1 = L.stat + MB;        // rstd of the first layer (backward)
    lds_f32* st_rs2 = L.stat + 2 * MB;    // rstd of the second layer being differentiated
    lds_f32* st_rs3 = L.stat + 3 * MB;    // rstd of the critic's second layer at (s, pi(s)); the target networks' too
    lds_f32* st_m1 = L.stat + 4 * MB;     // mean g, mean g * xhat of that layer
    lds_f32* st_m2 = L.stat + 5 * MB;

    float* th = dv.theta + (size_t)agent * d.Ppad;
    float* tt = dv.theta_t + (size_t)agent * d.Ppad;
    float* m_a = dv.m_a + (size_t)agent * d.Ppad;
    float* v_a = dv.v_a + (size_t)agent * d.Ppad;
    float* m_c = dv.m_c + (size_t)agent * d.Ppad;
    float* v_c = dv.v_c + (size_t)agent * d.Ppad;
    float* sc = dv.scratch + (size_t)agent * dv.scratch_stride;       // dh1 [B][H1] between the backward GEMM and the first layer
    float* pw = dv.pw + agent * 4;
    const float lr_a = dv.actor_lr[agent], lr_c = dv.critic_lr[agent], tau = dv.tau;
    float* tap_gc = grad_taps ? dv.tap_gc + (size_t)agent * d.Ppad : nullptr;
    float* tap_ga = grad_taps ? dv.tap_ga + (size_t)agent * d.Ppad : nullptr;
    float amax[AD];
#pragma unroll
    for (int j = 0; j < AD; j++) amax[j] = dv.amax[j];

    // zero both images and the padded tails of the per-sample vectors once (rows >= B, columns >= N never change)
    for (int i = tid; i < MB * AD; i += kThreads) { L.a[i] = 0.f; L.aout[i] = 0.f; L.mu[i] = 0.f; L.dz[i] = 0.f; }
    for (int i = tid; i < MB * SMAX; i += kThreads) { L.x[i] = 0.f; L.x2[i] = 0.f; }
    for (int i = tid; i < MB; i += kThreads) { L.q[i] = 0.f; L.y[i] = 0.f; L.dq[i] = 0.f; }
    for (int i = tid; i < 6 * MB; i += kThreads) L.stat[i] = 0.f;
    for (int i = tid; i < MB * u.LDH + 16; i += kThreads) L.hbuf[i] = 0.f;
    for (int i = tid; i < MB * LD2 + 16; i += kThreads) L.img[i] = 0.f;
    __syncthreads();

    // the first layer with its norm: hbuf = relu(LN(x . W1 + b1)); KEEP: xhat -> the second image, rstd -> st_rs1
    auto first_layer = [&](const float* P, const lds_f32* xs, auto keep) {
        u.trunk_z(P + d.oW1, P + d.ob1, xs);
        __syncthreads();
        u.template ln_rows<decltype(keep)::value>(P + d.oL1b, P + d.oL1g, st_rs1);
        __syncthreads();
    };
    // Column pass in front of ln_bwd_rows: thread n < N (in both halves of the workgroup) sums over the batch
    //   gg = d gamma[n], gb = d beta[n], go[j] = d (output-layer weight [n][j]) = sum_b relu(y) * seed[b][j]
    // with y = gamma*xhat + beta and dy = [y > 0] * up(b, n).
    auto col_grads = [&](int N, const float* beta, const float* gamma, auto up, auto ns_tag, const lds_f32* seed, float& gg,
                         float& gb, float (&go)[2]) {
        constexpr int NS = decltype(ns_tag)::value;
        gg = 0.0f; gb = 0.0f; go[0] = 0.0f; go[1] = 0.0f;
        const int n = tid & 255;
        if (n < N) {
            const float gm = gamma[n], bt = beta[n];
            for (int b = 0; b < B; b++) {
                const float xh = L.img[b * LD2 + n];
                const float yv = xh * gm + bt;
                const float dy = yv > 0.0f ? up(b, n) : 0.0f;
                gg += dy * xh;
                gb += dy;
                const float hv = fmaxf(yv, 0.0f);
#pragma unroll
                for (int j = 0; j < NS; j++) go[j] += hv * seed[b * NS + j];
            }
        }
    };
    auto col_sum = [&](int N) {           // sum_b img[b][n] for thread n < N: the bias gradient once the image holds dz
        float s = 0.0f;
        const int n = tid & 255;
        if (n < N)
            for (int b = 0; b < B; b++) s += L.img[b * LD2 + n];
        return s;
    };
    // First-layer backward from dh1 in `sc`: xhat1 recomputed into the second image, d gamma1 / d beta1, dz1, the
    // first-layer gradient, and Adam (+ Polyak when ttp is not null) on W1, b1, gamma1, beta1
    auto first_layer_bwd = [&](float* mm, float* vv, float alpha, float* tap, float* ttp) {
        first_layer(th, L.x, std::true_type{});
        float gg, gb, go[2];
        auto up = [&](int b, int n) { return sc[(size_t)b * H1 + n]; };
        col_grads(H1, th + d.oL1b, th + d.oL1g, up, std::integral_constant<int, 0>{}, nullptr, gg, gb, go);
        __syncthreads();
        u.ln_bwd_rows(H1, th + d.oL1b, th + d.oL1g, st_rs1, [&](int r, int n, int) { return sc[(size_t)r * H1 + n]; });
        __syncthreads();
        const int k = tid & 255, half = tid >> 8;
        if (k < H1) {
            float gw[SMAX], gbias = 0.0f;
#pragma unroll
            for (int s = 0; s < SMAX; s++) gw[s] = 0.0f;
            for (int b = 0; b < B; b++) {
                const float dzv = L.img[b * LD2 + k];
                gbias += dzv;
                const f32x4 x0 = *reinterpret_cast<const lds_f32x4*>(&L.x[b * SMAX]);
                const f32x4 x1 = *reinterpret_cast<const lds_f32x4*>(&L.x[b * SMAX + 4]);
#pragma unroll
                for (int s = 0; s < 4; s++) { gw[s] += x0[s] * dzv; gw[4 + s] += x1[s] * dzv; }
            }
            // S + 3 slots per column (W1 rows, b1, gamma1, beta1): even slots to the lower half of the workgroup
            for (int s = half; s < S + 3; s += 2) {
                float gr = gbias;
                int p = d.ob1 + k;
#pragma unroll
                for (int q = 0; q < SMAX; q++)
                    if (q == s && s < S) { gr = gw[q]; p = d.oW1 + q * H1 + k; }
                if (s == S + 1) { gr = gg; p = d.oL1g + k; }
                if (s == S + 2) { gr = gb; p = d.oL1b + k; }
                U::adam_scalar(th, mm, vv, ttp, tap, p, gr, alpha, tau);
            }
        }
        __syncthreads();
    };

    f32x4 acc[MT][NTW];
    for (int upd = 0; upd < n_updates; upd++) {
        // re-materialise lane geometry every update (ddpg_mfma_kernel.h: keeps the address arithmetic of the phases from
        // being hoisted out of the update loop and spilled)
        asm volatile("" : "+v"(u.c), "+v"(u.g), "+s"(u.wave));
        if (rollout) {
            // on-device experiment loop: one environment step first; the update runs when learn() would
            // (agents/base_agent.py:65-70).  The step's scratch is part .. idx (ln_step_scratch_floats), not an image:
            // it writes nothing that this launch zeroed once; it opens and ends behind a barrier.
            if (!rlc_train_step_device(rollout, agent, (float*)L.part, upd == 0 ? q8_first : 0)) continue;
        }
        // ================= sample + gather (utils/replaybuffer.py:32-37) =================
        const RlcRingMeta ring = dv.rep.ring[agent];
        rlc_pick_indices<kThreads>(dv.rep, agent, ring, source, B, host_idx, (size_t)blockIdx.x * n_updates + upd, L.pool,
                                   L.idx, L.dups);
        for (int b = tid; b < B; b += kThreads) {
            const RlcRow w = rlc_locate_row(dv.rep, agent, ring, source, S, AD, b, L.idx);
            L.r[b] = w.r; L.g[b] = w.g;
            for (int i = 0; i < S; i++) {
                L.x[b * SMAX + i] = clip_state_val(w.s[i], dv.clip_state, dv.smin[i], dv.smax[i]);
                L.x2[b * SMAX + i] = clip_state_val(w.s2[i], dv.clip_state, dv.smin[i], dv.smax[i]);
            }
#pragma unroll
            for (int j = 0; j < AD; j++) L.a[b * AD + j] = w.a[j];
        }
        __syncthreads();

        // ================= steps 1-2: target networks on s' (DDPG.py:77): three layer norms, forward only =================
        first_layer(tt, L.x2, std::false_type{});
        u.fwd_gemm(acc, tt + d.oWa2, HA, H1);
        u.template bias_add<0>(acc, tt + d.oba2, HA);
        u.ln_acc(acc, HA, st_mean, st_rs3);
        u.ln_act(acc, HA, tt + d.oL2b, tt + d.oL2g);
        u.template row_dot<false, AD>(acc, HA, [&](int n, int j) { return tt[d.oWa3 + n * AD + j]; }, L.part);
        __syncthreads();
        for (int i = tid; i < B * AD; i += kThreads) {
            const int b = i / AD, j = i % AD;
            L.aout[i] = tanhf(u.template part_sum<AD>(L.part, b, j) + tt[d.oba3 + j]) * amax[j];
        }
        __syncthreads();
        u.fwd_gemm(acc, tt + d.oWc2, HC, H1);
        u.template bias_add<AD>(acc, tt + d.obc2, HC, L.aout, tt + d.oWc2, d.arow0);
        u.ln_acc(acc, HC, st_mean, st_rs3);
        u.ln_act(acc, HC, tt + d.oL3b, tt + d.oL3g);
        u.template row_dot<false, 1>(acc, HC, [&](int n, int) { return tt[d.oWc3 + n]; }, L.part);
        __syncthreads();
        for (int b = tid; b < B; b += kThreads) {
            const float qt = u.template part_sum<1>(L.part, b, 0) + tt[d.obc3];
            const float y = (float)(L.r[b] + L.g[b] * (double)qt);     // float64 TD glue (DDPG.py:80-84)
            L.y[b] = y;
            dv.tap_y[(size_t)agent * RLC_MAX_BATCH + b] = y;
        }
        __syncthreads();

        // ================= step 3: critic step =================
        first_layer(th, L.x, std::false_type{});
        u.fwd_gemm(acc, th + d.oWc2, HC, H1);
        u.template bias_add<AD>(acc, th + d.obc2, HC, L.a, th + d.oWc2, d.arow0);
        u.ln_acc(acc, HC, st_mean, st_rs2);
        u.store_img(acc, HC);                             // xhat of the critic's second layer
        u.ln_act(acc, HC, th + d.oL3b, th + d.oL3g);
        u.template row_dot<false, 1>(acc, HC, [&](int n, int) { return th[d.oWc3 + n]; }, L.part);
        __syncthreads();
        for (int b = tid; b < B; b += kThreads) {
            const float q = u.template part_sum<1>(L.part, b, 0) + th[d.obc3];
            L.q[b] = q;
            dv.tap_q[(size_t)agent * RLC_MAX_BATCH + b] = q;
            L.dq[b] = 2.0f * (q - L.y[b]) / (float)B;                  // d mean((y-q)^2)/dq
        }
        __syncthreads();
        const float alpha_c = adam_alpha(lr_c, pw[2], pw[3]);
        {
            // d gamma3 / d beta3 / dWc3 from xhat, then dz2 in place, then bc2 and Adam + Polyak on the small tensors
            float gg, gb, go[2];
            const float w3n = (tid & 255) < HC ? th[d.oWc3 + (tid & 255)] : 0.0f;
            col_grads(HC, th + d.oL3b, th + d.oL3g, [&](int b, int) { return L.dq[b] * w3n; },
                      std::integral_constant<int, 1>{}, L.dq, gg, gb, go);
            __syncthreads();
            float w3[4];
#pragma unroll
            for (int i = 0; i < 4; i++) w3[i] = u.lane + 64 * i < HC ? th[d.oWc3 + u.lane + 64 * i] : 0.0f;
            u.ln_bwd_rows(HC, th + d.oL3b, th + d.oL3g, st_rs2, [&](int r, int, int i) { return L.dq[r] * w3[i]; });
            __syncthreads();
            const float gbias = col_sum(HC);
            const int n = tid & 255, half = tid >> 8;
            if (n < HC) {
                if (half == 0) {
                    U::adam_scalar(th, m_c, v_c, tt, tap_gc, d.oWc3 + n, go[0], alpha_c, tau);
                    U::adam_scalar(th, m_c, v_c, tt, tap_gc, d.obc2 + n, gbias, alpha_c, tau);
                } else {
                    U::adam_scalar(th, m_c, v_c, tt, tap_gc, d.oL3g + n, gg, alpha_c, tau);
                    U::adam_scalar(th, m_c, v_c, tt, tap_gc, d.oL3b + n, gb, alpha_c, tau);
                }
            }
            if (u.wave == 7) {            // bc3: sum_b dq[b] by one wave (fixed-order shuffle tree)
                float gr = 0.0f;
                for (int b = u.lane; b < MB; b += 64) gr += L.dq[b];
                gr = ln_wave_sum(gr);
                if (u.lane == 0) U::adam_scalar(th, m_c, v_c, tt, tap_gc, d.obc3, gr, alpha_c, tau);
            }
        }
        // dh1 = dz2 . Wc2[:H1]^T with Wc2 before its step
        u.bwd_gemm_img(acc, th + d.oWc2, HC, H1);
        u.store_dh(acc, sc);
        __syncthreads();      // every wave has finished reading the pre-step Wc2 rows
        // dWc2 = [h1|a]^T . dz2 with Adam + Polyak in the epilogue
        u.template wgrad_adam_img<AD>(L.a, HC, th + d.oWc2, m_c + d.oWc2, v_c + d.oWc2, alpha_c,
                                      tap_gc ? tap_gc + d.oWc2 : nullptr, tt + d.oWc2, tau);
        __syncthreads();      // both images are free; dh1 is visible
        // the trunk's target copy follows in the actor step (the hydra network)
        first_layer_bwd(m_c, v_c, alpha_c, tap_gc, nullptr);
        if (tid == 0) { pw[2] *= 0.9f; pw[3] *= 0.999f; }

        // ================= step 4: actor forward with the updated trunk (DDPG.py:90) =================
        first_layer(th, L.x, std::false_type{});
        u.fwd_gemm(acc, th + d.oWa2, HA, H1);
        u.template bias_add<0>(acc, th + d.oba2, HA);
        u.ln_acc(acc, HA, st_mean, st_rs2);
        u.store_img(acc, HA);                             // xhat of the actor's second layer
        u.ln_act(acc, HA, th + d.oL2b, th + d.oL2g);
        u.template row_dot<false, AD>(acc, HA, [&](int n, int j) { return th[d.oWa3 + n * AD + j]; }, L.part);
        __syncthreads();
        for (int i = tid; i < B * AD; i += kThreads) {
            const int b = i / AD, j = i % AD;
            const float mu = tanhf(u.template part_sum<AD>(L.part, b, j) + th[d.oba3 + j]);
            L.mu[i] = mu;
            const float ao = mu * amax[j];
            L.aout[i] = ao;
            dv.tap_aout[(size_t)agent * RLC_MAX_BATCH * AD + i] = ao;
        }
        __syncthreads();

        // ================= step 5: dQ/da at the scaled action, updated critic (DDPG.py:91) =================
        // back through the critic's second layer norm in the accumulators (the image holds the actor's xhat); only
        // the A action rows of Wc2 are needed: a row-dot, not a GEMM
        u.fwd_gemm(acc, th + d.oWc2, HC, H1);
        u.template bias_add<AD>(acc, th + d.obc2, HC, L.aout, th + d.oWc2, d.arow0);
        u.ln_acc(acc, HC, st_mean, st_rs3);
        {
            float gm[NTW], bt[NTW], w3[NTW], wa[NTW][AD];
            const int NT = (HC + 15) >> 4;
#pragma unroll
            for (int i = 0; i < NTW; i++) {
                const int t = u.tile_of(i);
                const int n = 16 * t + u.c;
                const bool ok = t < NT && n < HC;
                gm[i] = ok ? th[d.oL3g + n] : 0.0f;
                bt[i] = ok ? th[d.oL3b + n] : 0.0f;
                w3[i] = ok ? th[d.oWc3 + n] : 0.0f;
#pragma unroll
                for (int j = 0; j < AD; j++) wa[i][j] = ok ? th[d.oWc2 + rlc_blk_index(d.arow0 + j, n, HC)] : 0.0f;
            }
            auto gq = [&](float xh, int i) { return xh * gm[i] + bt[i] > 0.0f ? w3[i] * gm[i] : 0.0f; };
            u.template row_reduce<2>(acc, HC, [&](float xh, int, int, int i, float (&e)[2]) {
                const float gv = gq(xh, i);
                e[0] = gv;
                e[1] = gv * xh;
            });
            __syncthreads();
            for (int b = tid; b < MB; b += kThreads) {
                st_m1[b] = u.template part_sum<2>(L.part, b, 0) / (float)HC;
                st_m2[b] = u.template part_sum<2>(L.part, b, 1) / (float)HC;
            }
            __syncthreads();
            u.template row_reduce<AD>(acc, HC, [&](float xh, int, int b, int i, float (&e)[AD]) {
                const float dzv = st_rs3[b] * (gq(xh, i) - st_m1[b] - xh * st_m2[b]);
#pragma unroll
                for (int j = 0; j < AD; j++) e[j] = dzv * wa[i][j];
            });
        }
        __syncthreads();
        for (int i = tid; i < B * AD; i += kThreads) {
            const int b = i / AD, j = i % AD;
            const float dqda = u.template part_sum<AD>(L.part, b, j);
            dv.tap_dqda[(size_t)agent * RLC_MAX_BATCH * AD + i] = dqda;
            const float mu = L.mu[i];
            L.dz[i] = -dqda * (1.0f - mu * mu);                         // grad_ys = -dQ/da on tanh output (Q3)
        }
        __syncthreads();

        // ================= step 6: actor step =================
        const float alpha_a = adam_alpha(lr_a, pw[0], pw[1]);
        {
            float gg, gb, go[2];
            float w3n[AD];
#pragma unroll
            for (int j = 0; j < AD; j++) w3n[j] = (tid & 255) < HA ? th[d.oWa3 + (tid & 255) * AD + j] : 0.0f;
            auto up = [&](int b, int) {
                float s = 0.0f;
#pragma unroll
                for (int j = 0; j < AD; j++) s += L.dz[b * AD + j] * w3n[j];
                return s;
            };
            col_grads(HA, th + d.oL2b, th + d.oL2g, up, std::integral_constant<int, AD>{}, L.dz, gg, gb, go);
            __syncthreads();
            float w3[4][AD];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < AD; j++) w3[i][j] = u.lane + 64 * i < HA ? th[d.oWa3 + (u.lane + 64 * i) * AD + j] : 0.0f;
            u.ln_bwd_rows(HA, th + d.oL2b, th + d.oL2g, st_rs2, [&](int r, int, int i) {
                float s = 0.0f;
#pragma unroll
                for (int j = 0; j < AD; j++) s += L.dz[r * AD + j] * w3[i][j];
                return s;
            });
            __syncthreads();
            const float gbias = col_sum(HA);
            const int n = tid & 255, half = tid >> 8;
            if (n < HA) {
                if (half == 0) {
#pragma unroll
                    for (int j = 0; j < AD; j++) U::adam_scalar(th, m_a, v_a, tt, tap_ga, d.oWa3 + n * AD + j, go[j], alpha_a, tau);
                    U::adam_scalar(th, m_a, v_a, tt, tap_ga, d.oba2 + n, gbias, alpha_a, tau);
                } else {
                    U::adam_scalar(th, m_a, v_a, tt, tap_ga, d.oL2g + n, gg, alpha_a, tau);
                    U::adam_scalar(th, m_a, v_a, tt, tap_ga, d.oL2b + n, gb, alpha_a, tau);
                }
            }
            if (u.wave >= kWaves - AD) {  // ba3[j]: sum_b dz[b][j], one wave per column
                const int j = kWaves - 1 - u.wave;
                float gr = 0.0f;
                for (int b = u.lane; b < MB; b += 64) gr += L.dz[b * AD + j];
                gr = ln_wave_sum(gr);
                if (u.lane == 0) U::adam_scalar(th, m_a, v_a, tt, tap_ga, d.oba3 + j, gr, alpha_a, tau);
            }
        }
        u.bwd_gemm_img(acc, th + d.oWa2, HA, H1);
        u.store_dh(acc, sc);
        __syncthreads();
        u.template wgrad_adam_img<0>(nullptr, HA, th + d.oWa2, m_a + d.oWa2, v_a + d.oWa2, alpha_a,
                                     tap_ga ? tap_ga + d.oWa2 : nullptr, tt + d.oWa2, tau);
        __syncthreads();
        first_layer_bwd(m_a, v_a, alpha_a, tap_ga, tt);
        if (tid == 0) { pw[0] *= 0.9f; pw[1] *= 0.999f; }
        __syncthreads();
    }
}

template <int MT, int AD>
int launch_ln(const RlcDev& dv, int first_agent, int n_agents, int n_updates, int source, const long long* idx_dev,
              int grad_taps, hipStream_t st, const RlcRollout* rollout, int q8_first) {
    const size_t lds = smem_carve_ln(dv.d, MT, nullptr, nullptr);
    RLC_REQUIRE(lds <= 160 * 1024, "layer-norm MFMA DDPG kernel needs %zu B of LDS (> 160 KiB)", lds);
    RLC_REQUIRE(dv.d.norm && !dv.d.sep && !rlc_mfma_wide(dv.d) && dv.d.A == AD && dv.d.B <= 16 * MT,
                "layer-norm MFMA DDPG kernel launched for dimensions it does not take");
    RLC_REQUIRE(dv.scratch && dv.scratch_stride >= (long long)dv.d.B * dv.d.H1, "layer-norm MFMA DDPG kernel needs the population's scratch");
    {
        // the carve must still hold part, r, g and idx back to back, and the stretch must hold the training step's scratch
        SmemLn L;
        smem_carve_ln(dv.d, MT, nullptr, &L);
        const size_t have = (size_t)((lds_u8*)L.idx - (lds_u8*)L.part) + sizeof(long long) * RLC_MAX_BATCH;
        const size_t need = sizeof(float) * (ddpg_policy_lds_floats(dv.d) + 4);
        RLC_REQUIRE(!rollout || (have == sizeof(float) * ln_step_scratch_floats(MT) && need <= have),
                    "layer-norm MFMA DDPG kernel: the on-device training step needs %zu B of LDS scratch, %zu B lie between the "
                    "row partials and the sample indices", need, have);
    }
    auto kern = rlc_ddpg_update_ln_mfma_kernel<MT, AD>;
    static bool attr_set = false;
    if (!attr_set) {
        RLC_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, dim3(n_agents), dim3(kThreads), lds, st, dv, first_agent, n_updates, source, idx_dev, grad_taps,
                       rollout, q8_first);
    RLC_HIP(hipGetLastError());
    return 0;
}

}  // namespace
