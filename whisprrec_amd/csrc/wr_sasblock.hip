// wr_sasblock.hip — K13: one whole SASRec TransformerLayer (reference src/utils/layers.py:8-86), forward and backward, fp32.
//
//   q, k, v = x Wq^T + bq, ...        S = q k^T / sqrt(d_k), causal        P = softmax(S - max over the WHOLE call)  (:54)
//   A = P v, a row whose exponentials all underflow is 0 (the isnan fill, :55)          C = LN1(drop1(A) + x)
//   H = relu(C W1^T + b1)             out = LN2(drop2(H W2^T + b2) + C)                  LayerNorm eps 1e-5, d_ff = D
//
// One workgroup of 256 threads works on one sequence at a time; everything of that sequence lives in LDS as [T][D + 1] slots
// (the odd stride keeps both the row-broadcast and the column access patterns free of bank conflicts).
//
//   forward, launch 1   q / k / v of every sequence -> workspace, the causal scores' maximum per workgroup -> workspace
//   forward, launch 2   every workgroup folds the workgroup maxima (at most 2,048 floats, the same order everywhere: the same
//                       value everywhere), then attention, LN1, feed-forward, LN2; workgroup 0 stores the maximum for the backward
//   backward, launch 1  a workgroup walks its sequences (b = wg, wg + G, ...): recomputes the forward of a sequence from x
//                       and the stored maximum, walks back through it, writes that sequence's gx and keeps the 5 D^2 + 9 D
//                       parameter gradients in registers; at the end they go to the workgroup's row of the partials
//   backward, launch 2  the partials folded in workgroup order
// Products x W^T take W transposed from an LDS slot (staged straight from the live parameter, coalesced); products dY W read
// W from global memory, where consecutive lanes already read consecutive floats.  No matrix cores: at T = 20 a sequence is
// 20 x 64 — the launch count was the cost, not the arithmetic.
//
// Dropout: counter-based keep mask over (seed, site, b, t, d) with the sampler's splitmix64 finaliser (mix64, wr_common.h):
//   key_site = mix64(seed ^ (site + 1) * 0x9E3779B97F4A7C15),  draw = mix64(key_site ^ (e * 0xD1B54A32D192ED03 + 1)) >> 40,
//   e = (b T + t) D + d;  kept iff draw >= floor(p 2^24), scaled by the fp32 1 / (1 - p).  Recomputed in the backward.
//
// Backward: the path through the global maximum is ignored (softmax is shift-invariant: it sums to zero in exact arithmetic).
// DEVIATION from the reference: a row zeroed by the NaN rule passes no gradient through its scores here; the reference's
// autograd produces NaN gradients for such a row.  That regime is outside the parity claim.
//
// No float atomics, every sum has a fixed order: same inputs and seed, same bits.  No allocation, no host round trip.
//
// Two masks, one code: the kernels are templates over CAUSAL.  CAUSAL (SASRec, wr_sasblock_fwd / _bwd): query i keeps keys
// j <= i.  !CAUSAL (ContraRec's BERT4RecEncoder, wr_sasblock_fwd_keys / _bwd_keys): every query i in 0..T-1 — the padded
// positions are ordinary queries — keeps keys j < key_len[b]; a key_len outside [1, T] is clamped before it bounds any loop and
// reported in err_word.  The mask is only the bound of the key loops (jend), workgroup-uniform in the second mode.
#include "wr_common.h"

namespace wr {

constexpr int kSasParams = 14;
constexpr int kSasFwdWg = 2048;    // workgroups of forward launch 1 = number of partial maxima
constexpr int kSasBwdWg = 512;     // workgroups of the backward = rows of the gradient partials
constexpr float kSasLnEps = 1e-5f;

enum { SP_WQ, SP_BQ, SP_WK, SP_BK, SP_WV, SP_BV, SP_G1, SP_BE1, SP_W1, SP_B1, SP_W2, SP_B2, SP_G2, SP_BE2 };

struct SasParams {
    const float *p[kSasParams];
};

struct SasDrop {
    uint64_t key[2];
    uint32_t thr;
    float scale;
    int on;
};

__device__ __forceinline__ float sas_drop(const SasDrop &dr, int site, uint64_t e) {
    if (!dr.on) return 1.0f;
    const uint32_t draw = (uint32_t)(mix64(dr.key[site] ^ (e * 0xD1B54A32D192ED03ull + 1ull)) >> 40);
    return draw >= dr.thr ? dr.scale : 0.0f;
}

// offset of parameter k in the packed gradient (D = d_ff): every block is a multiple of D floats
__host__ __device__ __forceinline__ int sas_off(int k, int D) {
    const int nw[kSasParams + 1] = {0, 1, 1, 2, 2, 3, 3, 3, 3, 4, 4, 5, 5, 5, 5};   // weight matrices before parameter k
    const int nv[kSasParams + 1] = {0, 0, 1, 1, 2, 2, 3, 4, 5, 5, 6, 6, 7, 8, 9};   // vectors before parameter k
    return nw[k] * D * D + nv[k] * D;
}

__device__ __forceinline__ float sas_block_max(float v, float *red) {
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();                                     // red may still be read from an earlier use
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// [T][D] rows of global memory <-> an LDS slot of stride D + 1
template <int D>
__device__ __forceinline__ void sas_load(const float *__restrict__ g, float *s, int T) {
    for (int e = threadIdx.x; e < T * D; e += kBlock) s[(e / D) * (D + 1) + (e % D)] = g[e];
}
template <int D>
__device__ __forceinline__ void sas_store(float *__restrict__ g, const float *s, int T) {
    for (int e = threadIdx.x; e < T * D; e += kBlock) g[e] = s[(e / D) * (D + 1) + (e % D)];
}

// sW[d][j] = W[j][d]: the operand of x W^T with consecutive lanes on consecutive output features
template <int D>
__device__ __forceinline__ void sas_stage_wt(const float *__restrict__ W, float *sW) {
    for (int e = threadIdx.x; e < D * D; e += kBlock) sW[(e % D) * (D + 1) + (e / D)] = W[e];
}

// out(t, c) = sum_k A[t][k] * Bm[k * ldb + c] for t < T, handed to epi(t, c, value).  A is an LDS slot; Bm is an LDS slot
// (ldb = D + 1) or a weight matrix in global memory (ldb = D).  Thread: column c = tid % D, rows tid / D + i * (256 / D).
template <int D, int TM, typename Epi>
__device__ __forceinline__ void sas_mm(const float *A, const float *Bm, int ldb, int T, Epi epi) {
    constexpr int LD = D + 1, RP = kBlock / D, NT = TM / RP;
    static_assert(TM % RP == 0, "row tile");
    const int c = threadIdx.x % D, r0 = threadIdx.x / D;
    // Every thread runs all NT row groups, those past T too: their operands lie inside the slot and their sums are dropped.
    // Skipping them (a workgroup-uniform test per group, rows clamped to T - 1) was measured: it costs the constant LDS
    // offsets of the unrolled loop, and the training step at T = 20 went from 2.34 to 2.61 ms (B = 2,048).
    float acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = 0.f;
#pragma unroll 4
    for (int k = 0; k < D; ++k) {
        const float w = Bm[k * ldb + c];
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[i] = fmaf(A[(r0 + i * RP) * LD + k], w, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int t = r0 + i * RP;
        if (t < T) epi(t, c, acc[i]);
    }
}

// acc(j, d) += sum_t dY[t][j] * A[t][d]: the weight gradient of y = A W^T.  Thread: d = tid % D, j = tid / D + k * (256 / D).
template <int D>
__device__ __forceinline__ void sas_wgrad(float (&acc)[D * D / kBlock], const float *dY, const float *A, int T) {
    constexpr int LD = D + 1, RP = kBlock / D, NJ = D * D / kBlock;
    const int d = threadIdx.x % D, j0 = threadIdx.x / D;
    for (int t = 0; t < T; ++t) {
        const float a = A[t * LD + d];
#pragma unroll
        for (int k = 0; k < NJ; ++k) acc[k] = fmaf(dY[t * LD + j0 + k * RP], a, acc[k]);
    }
}

template <int D>
__device__ __forceinline__ void sas_wgrad_store(const float (&acc)[D * D / kBlock], float *__restrict__ dst) {
    constexpr int RP = kBlock / D, NJ = D * D / kBlock;
    const int d = threadIdx.x % D, j0 = threadIdx.x / D;
#pragma unroll
    for (int k = 0; k < NJ; ++k) dst[(j0 + k * RP) * D + d] = acc[k];
}

// column sums over the T rows of a slot, by the threads c < D
template <int D>
__device__ __forceinline__ float sas_colsum(const float *s, int T, int c) {
    float v = 0.f;
    for (int t = 0; t < T; ++t) v += s[t * (D + 1) + c];
    return v;
}
template <int D>
__device__ __forceinline__ float sas_coldot(const float *a, const float *b, int T, int c) {
    float v = 0.f;
    for (int t = 0; t < T; ++t) v = fmaf(a[t * (D + 1) + c], b[t * (D + 1) + c], v);
    return v;
}

__device__ __forceinline__ float sas_dot(const float *a, const float *b, int n) {
    float s = 0.f;
    for (int c = 0; c < n; ++c) s = fmaf(a[c], b[c], s);
    return s;
}

// LayerNorm of one row (one thread): row <- (row - mean) * rstd, y (may be row itself, or NULL) <- that * gamma + beta
template <int D>
__device__ __forceinline__ float sas_ln_row(float *row, float *y, const float *__restrict__ gamma, const float *__restrict__ beta) {
    float s = 0.f;
#pragma unroll 8
    for (int c = 0; c < D; ++c) s += row[c];
    const float mu = s / (float)D;
    float v = 0.f;
#pragma unroll 8
    for (int c = 0; c < D; ++c) {
        const float d = row[c] - mu;
        v = fmaf(d, d, v);
    }
    const float rstd = 1.0f / sqrtf(v / (float)D + kSasLnEps);
#pragma unroll 8
    for (int c = 0; c < D; ++c) {
        const float xh = (row[c] - mu) * rstd;
        row[c] = xh;
        if (y != nullptr) y[c] = xh * gamma[c] + beta[c];
    }
    return rstd;
}

// backward of the normalisation of one row (one thread): g <- rstd * (g gamma - mean(g gamma) - xh * mean(g gamma xh))
template <int D>
__device__ __forceinline__ void sas_ln_row_bwd(float *g, const float *xh, const float *__restrict__ gamma, float rstd) {
    float a = 0.f, b = 0.f;
#pragma unroll 8
    for (int c = 0; c < D; ++c) {
        const float dxh = g[c] * gamma[c];
        a += dxh;
        b = fmaf(dxh, xh[c], b);
    }
    a /= (float)D;
    b /= (float)D;
#pragma unroll 8
    for (int c = 0; c < D; ++c) g[c] = rstd * (g[c] * gamma[c] - a - xh[c] * b);
}

// largest kept score of the sequence in sQ / sK over this thread's row (h, i), or -inf for a thread without a row
template <int D, bool CAUSAL>
__device__ __forceinline__ float sas_row_max(const float *sQ, const float *sK, int T, int H, int dk, float sqrt_dk, int len) {
    constexpr int LD = D + 1;
    float m = -INFINITY;
    const int r = threadIdx.x;
    if (r < H * T) {
        const int h = r / T, i = r % T;
        const float *q = sQ + i * LD + h * dk;
        const int jend = CAUSAL ? i + 1 : len;
        for (int j = 0; j < jend; ++j) m = fmaxf(m, sas_dot(q, sK + j * LD + h * dk, dk) / sqrt_dk);
    }
    return m;
}

// attention of one sequence: thread r = (h, i) owns one score row.  sA[i][h dk ..] = sum_j P_ij v_j, sZ[r] = sum_j exp
template <int D, bool CAUSAL>
__device__ __forceinline__ void sas_attn_fwd(const float *sQ, const float *sK, const float *sV, float *sA, float *sZ, int T, int H,
                                             int dk, float sqrt_dk, float gmax, int len) {
    constexpr int LD = D + 1;
    const int r = threadIdx.x;
    if (r >= H * T) return;
    const int h = r / T, i = r % T;
    const float *q = sQ + i * LD + h * dk;
    float *a = sA + i * LD + h * dk;
    for (int c = 0; c < dk; ++c) a[c] = 0.f;
    float Z = 0.f;
    const int jend = CAUSAL ? i + 1 : len;
    for (int j = 0; j < jend; ++j) {
        const float e = expf(sas_dot(q, sK + j * LD + h * dk, dk) / sqrt_dk - gmax);
        Z += e;
        const float *v = sV + j * LD + h * dk;
        for (int c = 0; c < dk; ++c) a[c] = fmaf(e, v[c], a[c]);
    }
    for (int c = 0; c < dk; ++c) a[c] = Z > 0.f ? a[c] / Z : 0.f;      // 0 / 0 in the reference, zeroed by its isnan fill
    sZ[r] = Z;
}

// key_len[b] clamped into [1, T]; a value outside is reported once per sequence (integer OR: order-free).  Causal: T, unused.
template <bool CAUSAL>
__device__ __forceinline__ int sas_key_len(const int64_t *__restrict__ key_len, int64_t b, int T, int32_t *__restrict__ err_word) {
    if constexpr (CAUSAL) return T;
    const int64_t l = key_len[b];
    const bool bad = l < 1 || l > (int64_t)T;
    if (bad && err_word != nullptr && threadIdx.x == 0) atomicOr(err_word, 1);
    return bad ? (l < 1 ? 1 : T) : (int)l;
}

// ------------------------------------------------------------------------------------------------ forward, launch 1
template <int D, int TM, bool CAUSAL>
__global__ __launch_bounds__(kBlock, TM <= 24 ? 2 : 1) void sas_fwd_pre_kernel(const float *__restrict__ x, int64_t B, int T, int H, SasParams P,
                                                             float sqrt_dk, float *__restrict__ qkv, float *__restrict__ wgmax,
                                                             const int64_t *__restrict__ key_len, int32_t *__restrict__ err_word) {
    constexpr int LD = D + 1;
    __shared__ float sX[TM * LD], sQ[TM * LD], sK[TM * LD], sW[D * LD], red[4];
    const int dk = D / H;
    float m = -INFINITY;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        __syncthreads();
        sas_load<D>(x + b * T * D, sX, T);
        float *dst = qkv + b * 3 * T * D;
        for (int w = 0; w < 3; ++w) {
            sas_stage_wt<D>(P.p[2 * w], sW);
            __syncthreads();
            const float *bias = P.p[2 * w + 1];
            float *s = w == 0 ? sQ : sK;
            sas_mm<D, TM>(sX, sW, LD, T, [&](int t, int c, float v) {
                v += bias[c];
                if (w < 2) s[t * LD + c] = v;
                dst[(w * T + t) * D + c] = v;
            });
            __syncthreads();
        }
        m = fmaxf(m, sas_row_max<D, CAUSAL>(sQ, sK, T, H, dk, sqrt_dk, sas_key_len<CAUSAL>(key_len, b, T, err_word)));
    }
    m = sas_block_max(m, red);
    if (threadIdx.x == 0) wgmax[blockIdx.x] = m;
}

// ------------------------------------------------------------------------------------------------ forward, launch 2
template <int D, int TM, bool CAUSAL>
__global__ __launch_bounds__(kBlock, TM <= 24 ? 2 : 1) void sas_fwd_main_kernel(const float *__restrict__ x, int64_t B, int T, int H, SasParams P,
                                                              float sqrt_dk, SasDrop dr, const float *__restrict__ qkv,
                                                              const float *__restrict__ wgmax, int n_max, float *__restrict__ out,
                                                              float *__restrict__ gmax_out, const int64_t *__restrict__ key_len) {
    constexpr int LD = D + 1;
    __shared__ float sQ[TM * LD], sK[TM * LD], sV[TM * LD], sA[TM * LD], sW[D * LD], sZ[kBlock], red[4];
    const int dk = D / H;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < n_max; i += kBlock) m = fmaxf(m, wgmax[i]);
    const float gmax = sas_block_max(m, red);
    if (blockIdx.x == 0 && threadIdx.x == 0) gmax_out[0] = gmax;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        __syncthreads();
        const float *src = qkv + b * 3 * T * D;
        sas_load<D>(src, sQ, T);
        sas_load<D>(src + T * D, sK, T);
        sas_load<D>(src + 2 * T * D, sV, T);
        __syncthreads();
        sas_attn_fwd<D, CAUSAL>(sQ, sK, sV, sA, sZ, T, H, dk, sqrt_dk, gmax, sas_key_len<CAUSAL>(key_len, b, T, nullptr));
        __syncthreads();
        const float *xb = x + b * T * D;
        for (int e = threadIdx.x; e < T * D; e += kBlock) {
            float &a = sA[(e / D) * LD + (e % D)];
            a = a * sas_drop(dr, 0, (uint64_t)(b * T * D + e)) + xb[e];
        }
        __syncthreads();
        if (threadIdx.x < T) sas_ln_row<D>(sA + threadIdx.x * LD, sA + threadIdx.x * LD, P.p[SP_G1], P.p[SP_BE1]);   // sA = C
        sas_stage_wt<D>(P.p[SP_W1], sW);
        __syncthreads();
        sas_mm<D, TM>(sA, sW, LD, T, [&](int t, int c, float v) { sK[t * LD + c] = fmaxf(v + P.p[SP_B1][c], 0.f); });   // sK = H
        __syncthreads();
        sas_stage_wt<D>(P.p[SP_W2], sW);
        __syncthreads();
        sas_mm<D, TM>(sK, sW, LD, T, [&](int t, int c, float v) {
            v += P.p[SP_B2][c];
            sV[t * LD + c] = v * sas_drop(dr, 1, (uint64_t)((b * T + t) * D + c)) + sA[t * LD + c];
        });
        __syncthreads();
        if (threadIdx.x < T) sas_ln_row<D>(sV + threadIdx.x * LD, sV + threadIdx.x * LD, P.p[SP_G2], P.p[SP_BE2]);
        __syncthreads();
        sas_store<D>(out + b * T * D, sV, T);
    }
}

// ------------------------------------------------------------------------------------------------ backward, launch 1
template <int D, int TM, bool CAUSAL>
__global__ __launch_bounds__(kBlock, TM <= 24 ? 2 : 1) void sas_bwd_kernel(const float *__restrict__ x, const float *__restrict__ gout, int64_t B, int T,
                                                         int H, SasParams P, float sqrt_dk, SasDrop dr,
                                                         const float *__restrict__ gmax_p, float *__restrict__ gx,
                                                         float *__restrict__ part, const int64_t *__restrict__ key_len,
                                                         int32_t *__restrict__ err_word) {
    constexpr int LD = D + 1, SLOT = TM * LD, ESLOT = (TM > D ? TM : D) * LD, NJ = D * D / kBlock;
    // slot:  s0 q   s1 k   s2 v   s3 xhat1 (A and y1 on the way; x again at the end)   s4 C, then dv   s5 H, then dk
    //        s6 y2 -> xhat2 -> d pre-activation -> dq   s7 x, then the gradient flowing back   s8 W^T staging, dO2, dA
    __shared__ float slots[8 * SLOT + ESLOT], sZ[kBlock], sDelta[kBlock], rstd1[TM], rstd2[TM];
    float *s0 = slots, *s1 = s0 + SLOT, *s2 = s1 + SLOT, *s3 = s2 + SLOT, *s4 = s3 + SLOT, *s5 = s4 + SLOT, *s6 = s5 + SLOT,
          *s7 = s6 + SLOT, *s8 = s7 + SLOT;
    const int dk = D / H, tid = threadIdx.x;
    const float gmax = gmax_p[0];
    float aq[NJ], ak[NJ], av[NJ], a1[NJ], a2[NJ];
#pragma unroll
    for (int k = 0; k < NJ; ++k) aq[k] = ak[k] = av[k] = a1[k] = a2[k] = 0.f;
    float cbq = 0.f, cbk = 0.f, cbv = 0.f, cg1 = 0.f, cbe1 = 0.f, cb1 = 0.f, cb2 = 0.f, cg2 = 0.f, cbe2 = 0.f;   // threads < D

    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const float *xb = x + b * T * D;
        const uint64_t e0 = (uint64_t)(b * T * D);
        const int len = sas_key_len<CAUSAL>(key_len, b, T, err_word);
        __syncthreads();
        // ---- the forward of this sequence again
        sas_load<D>(xb, s7, T);
        for (int w = 0; w < 3; ++w) {
            sas_stage_wt<D>(P.p[2 * w], s8);
            __syncthreads();
            const float *bias = P.p[2 * w + 1];
            float *s = w == 0 ? s0 : w == 1 ? s1 : s2;
            sas_mm<D, TM>(s7, s8, LD, T, [&](int t, int c, float v) { s[t * LD + c] = v + bias[c]; });
            __syncthreads();
        }
        sas_attn_fwd<D, CAUSAL>(s0, s1, s2, s3, sZ, T, H, dk, sqrt_dk, gmax, len);
        __syncthreads();
        for (int e = tid; e < T * D; e += kBlock) {
            const int o = (e / D) * LD + (e % D);
            s3[o] = s3[o] * sas_drop(dr, 0, e0 + e) + s7[o];
        }
        __syncthreads();
        if (tid < T) rstd1[tid] = sas_ln_row<D>(s3 + tid * LD, s4 + tid * LD, P.p[SP_G1], P.p[SP_BE1]);
        sas_stage_wt<D>(P.p[SP_W1], s8);
        __syncthreads();
        sas_mm<D, TM>(s4, s8, LD, T, [&](int t, int c, float v) { s5[t * LD + c] = fmaxf(v + P.p[SP_B1][c], 0.f); });
        __syncthreads();
        sas_stage_wt<D>(P.p[SP_W2], s8);
        __syncthreads();
        sas_mm<D, TM>(s5, s8, LD, T, [&](int t, int c, float v) {
            v += P.p[SP_B2][c];
            s6[t * LD + c] = v * sas_drop(dr, 1, e0 + (uint64_t)(t * D + c)) + s4[t * LD + c];
        });
        __syncthreads();
        if (tid < T) rstd2[tid] = sas_ln_row<D>(s6 + tid * LD, nullptr, nullptr, nullptr);
        // ---- LN2
        sas_load<D>(gout + b * T * D, s7, T);
        __syncthreads();
        if (tid < D) {
            cg2 += sas_coldot<D>(s7, s6, T, tid);
            cbe2 += sas_colsum<D>(s7, T, tid);
        }
        __syncthreads();
        if (tid < T) sas_ln_row_bwd<D>(s7 + tid * LD, s6 + tid * LD, P.p[SP_G2], rstd2[tid]);      // s7 = d(y2)
        __syncthreads();
        // ---- linear2, ReLU, linear1
        for (int e = tid; e < T * D; e += kBlock) {
            const int o = (e / D) * LD + (e % D);
            s8[o] = s7[o] * sas_drop(dr, 1, e0 + e);                                               // s8 = d(O2)
        }
        __syncthreads();
        sas_wgrad<D>(a2, s8, s5, T);
        if (tid < D) cb2 += sas_colsum<D>(s8, T, tid);
        sas_mm<D, TM>(s8, P.p[SP_W2], D, T, [&](int t, int c, float v) { s6[t * LD + c] = s5[t * LD + c] > 0.f ? v : 0.f; });
        __syncthreads();
        sas_wgrad<D>(a1, s6, s4, T);
        if (tid < D) cb1 += sas_colsum<D>(s6, T, tid);
        sas_mm<D, TM>(s6, P.p[SP_W1], D, T, [&](int t, int c, float v) { s7[t * LD + c] += v; });   // s7 = d(C)
        __syncthreads();
        // ---- LN1
        if (tid < D) {
            cg1 += sas_coldot<D>(s7, s3, T, tid);
            cbe1 += sas_colsum<D>(s7, T, tid);
        }
        __syncthreads();
        if (tid < T) sas_ln_row_bwd<D>(s7 + tid * LD, s3 + tid * LD, P.p[SP_G1], rstd1[tid]);      // s7 = d(y1): gx's residual part
        __syncthreads();
        for (int e = tid; e < T * D; e += kBlock) {
            const int o = (e / D) * LD + (e % D);
            s8[o] = s7[o] * sas_drop(dr, 0, e0 + e);                                               // s8 = d(A)
        }
        __syncthreads();
        // ---- attention.  Row pass: thread (h, i) -> delta_i = sum_j P_ij dP_ij and dq_i
        if (tid < H * T) {
            const int h = tid / T, i = tid % T, ho = h * dk;
            const float Z = sZ[tid];
            const float *q = s0 + i * LD + ho, *da = s8 + i * LD + ho;
            float *dq = s6 + i * LD + ho;
            for (int c = 0; c < dk; ++c) dq[c] = 0.f;
            float delta = 0.f;
            const int jend = CAUSAL ? i + 1 : len;
            if (Z > 0.f) {                                                  // a zeroed row passes nothing through its scores
                for (int j = 0; j < jend; ++j) {
                    const float p = expf(sas_dot(q, s1 + j * LD + ho, dk) / sqrt_dk - gmax) / Z;
                    delta = fmaf(p, sas_dot(da, s2 + j * LD + ho, dk), delta);
                }
                for (int j = 0; j < jend; ++j) {
                    const float *kj = s1 + j * LD + ho;
                    const float p = expf(sas_dot(q, kj, dk) / sqrt_dk - gmax) / Z;
                    const float ds = p * (sas_dot(da, s2 + j * LD + ho, dk) - delta) / sqrt_dk;
                    for (int c = 0; c < dk; ++c) dq[c] = fmaf(ds, kj[c], dq[c]);
                }
            }
            sDelta[tid] = delta;
        }
        __syncthreads();
        // column pass: thread (h, j) -> dk_j = sum_i dS_ij q_i (into s5), dv_j = sum_i P_ij dA_i (into s4)
        if (tid < H * T) {
            const int h = tid / T, j = tid % T, ho = h * dk;
            const float *kj = s1 + j * LD + ho, *vj = s2 + j * LD + ho;
            float *dkj = s5 + j * LD + ho, *dvj = s4 + j * LD + ho;
            for (int c = 0; c < dk; ++c) dkj[c] = dvj[c] = 0.f;
            for (int i = CAUSAL ? j : (j < len ? 0 : T); i < T; ++i) {     // the queries that keep key j
                const float Z = sZ[h * T + i];
                if (!(Z > 0.f)) continue;
                const float *q = s0 + i * LD + ho, *da = s8 + i * LD + ho;
                const float p = expf(sas_dot(q, kj, dk) / sqrt_dk - gmax) / Z;
                const float ds = p * (sas_dot(da, vj, dk) - sDelta[h * T + i]) / sqrt_dk;
                for (int c = 0; c < dk; ++c) {
                    dkj[c] = fmaf(ds, q[c], dkj[c]);
                    dvj[c] = fmaf(p, da[c], dvj[c]);
                }
            }
        }
        sas_load<D>(xb, s3, T);                                             // xhat1 is done with: x for the q / k / v weights
        __syncthreads();
        // ---- the three projections
        sas_wgrad<D>(aq, s6, s3, T);
        sas_wgrad<D>(ak, s5, s3, T);
        sas_wgrad<D>(av, s4, s3, T);
        if (tid < D) {
            cbq += sas_colsum<D>(s6, T, tid);
            cbk += sas_colsum<D>(s5, T, tid);
            cbv += sas_colsum<D>(s4, T, tid);
        }
        sas_mm<D, TM>(s6, P.p[SP_WQ], D, T, [&](int t, int c, float v) { s7[t * LD + c] += v; });
        sas_mm<D, TM>(s5, P.p[SP_WK], D, T, [&](int t, int c, float v) { s7[t * LD + c] += v; });
        sas_mm<D, TM>(s4, P.p[SP_WV], D, T, [&](int t, int c, float v) { s7[t * LD + c] += v; });
        __syncthreads();
        sas_store<D>(gx + b * T * D, s7, T);
    }
    float *row = part + (int64_t)blockIdx.x * (5 * D * D + 9 * D);
    sas_wgrad_store<D>(aq, row + sas_off(SP_WQ, D));
    sas_wgrad_store<D>(ak, row + sas_off(SP_WK, D));
    sas_wgrad_store<D>(av, row + sas_off(SP_WV, D));
    sas_wgrad_store<D>(a1, row + sas_off(SP_W1, D));
    sas_wgrad_store<D>(a2, row + sas_off(SP_W2, D));
    if (tid < D) {
        row[sas_off(SP_BQ, D) + tid] = cbq;
        row[sas_off(SP_BK, D) + tid] = cbk;
        row[sas_off(SP_BV, D) + tid] = cbv;
        row[sas_off(SP_G1, D) + tid] = cg1;
        row[sas_off(SP_BE1, D) + tid] = cbe1;
        row[sas_off(SP_B1, D) + tid] = cb1;
        row[sas_off(SP_B2, D) + tid] = cb2;
        row[sas_off(SP_G2, D) + tid] = cg2;
        row[sas_off(SP_BE2, D) + tid] = cbe2;
    }
}

// ------------------------------------------------------------------------------------------------ backward, launch 2
__global__ __launch_bounds__(kBlock) void sas_fold_kernel(const float *__restrict__ part, int n_part, int P, float *__restrict__ g) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= P) return;
    float v = 0.f;
    for (int w = 0; w < n_part; ++w) v += part[(int64_t)w * P + e];            // workgroup order
    g[e] = v;
}

// ------------------------------------------------------------------------------------------------ host side
struct SasLayout {
    int64_t wgmax, qkv, part, total;   // byte offsets
};

static void sas_layout(int64_t B, int32_t T, int32_t D, SasLayout &L) {
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t at = o; o += align_up(bytes, 256); return at; };
    L.wgmax = take((int64_t)kSasFwdWg * 4);
    L.qkv = take(B * 3 * T * D * 4);
    L.part = take((int64_t)kSasBwdWg * (5 * D * D + 9 * D) * 4);               // sized by the bound, not by min(B, bound)
    L.total = o;
}

static int32_t sas_check(const char *entry, int64_t B, int32_t T, int32_t D, int32_t d_ff, int32_t n_heads) {
    WR_REQUIRE(T >= 1 && B >= 1 && B <= (int64_t(1) << 24), WR_E_SHAPE, "%s: B=%lld / T=%d out of range (B in 1..2^24, T >= 1)", entry,
               (long long)B, T);
    WR_REQUIRE(wr_sasblock_supported(D, d_ff, n_heads, T), WR_E_RANGE,
               "%s supports D = d_ff in {32, 64}, n_heads in {1, 2, 4} with D / n_heads >= 8, T <= 64; got D=%d d_ff=%d n_heads=%d T=%d",
               entry, D, d_ff, n_heads, T);
    return WR_OK;
}

static int32_t sas_check_params(const char *entry, const float *const *params, SasParams &P) {
    WR_REQUIRE(params != nullptr, WR_E_NULL, "%s: params is NULL", entry);
    for (int k = 0; k < kSasParams; ++k) {
        WR_REQUIRE(params[k] != nullptr, WR_E_NULL, "%s: parameter %d is NULL", entry, k);
        WR_REQUIRE(aligned16(params[k]), WR_E_ALIGN, "%s: parameter %d is not 16-byte aligned", entry, k);
        P.p[k] = params[k];
    }
    return WR_OK;
}

static int32_t sas_drop_of(const char *entry, float p, uint64_t seed, int32_t training, SasDrop &dr) {
    WR_REQUIRE(p >= 0.f && p < 1.f, WR_E_RANGE, "%s: dropout p must lie in [0, 1)", entry);
    dr.on = (training != 0 && p > 0.f) ? 1 : 0;
    dr.key[0] = mix64(seed ^ (1ull * 0x9E3779B97F4A7C15ull));
    dr.key[1] = mix64(seed ^ (2ull * 0x9E3779B97F4A7C15ull));
    dr.thr = (uint32_t)((double)p * 16777216.0);
    dr.scale = 1.0f / (1.0f - p);
    return WR_OK;
}

#define WR_SAS_DISPATCH(D, T, CALL)                  \
    do {                                             \
        if ((D) == 64 && (T) <= 24) { CALL(64, 24); } \
        else if ((D) == 64) { CALL(64, 64); }         \
        else if ((T) <= 24) { CALL(32, 24); }         \
        else { CALL(32, 64); }                        \
    } while (0)

}  // namespace wr

using namespace wr;

template <bool CAUSAL>
static int32_t sas_fwd(const char *entry, const float *x, int64_t B, int32_t T, int32_t D, int32_t d_ff, int32_t n_heads,
                       const float *const *params, float p, uint64_t seed, int32_t training, const int64_t *key_len,
                       int32_t *err_word, float *out, float *gmax, void *workspace, int64_t workspace_bytes, void *stream_) {
    int32_t rc = sas_check(entry, B, T, D, d_ff, n_heads);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(x && out && gmax && (CAUSAL || key_len), WR_E_NULL, "%s: NULL argument", entry);
    WR_REQUIRE(aligned16(x) && aligned16(out), WR_E_ALIGN, "%s: x and out must be 16-byte aligned", entry);
    SasParams P;
    if ((rc = sas_check_params(entry, params, P)) != WR_OK) return rc;
    SasDrop dr;
    if ((rc = sas_drop_of(entry, p, seed, training, dr)) != WR_OK) return rc;
    SasLayout L;
    sas_layout(B, T, D, L);
    if ((rc = check_workspace(entry, workspace, workspace_bytes, L.total)) != WR_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    char *ws = reinterpret_cast<char *>(workspace);
    float *wgmax = reinterpret_cast<float *>(ws + L.wgmax), *qkv = reinterpret_cast<float *>(ws + L.qkv);
    const int n_max = (int)(B < kSasFwdWg ? B : kSasFwdWg);
    const float sqrt_dk = sqrtf((float)(D / n_heads));
#define WR_SAS_FWD(D_, TM_)                                                                                                   \
    do {                                                                                                                      \
        hipLaunchKernelGGL((sas_fwd_pre_kernel<D_, TM_, CAUSAL>), dim3(n_max), dim3(kBlock), 0, stream, x, B, T, n_heads, P, sqrt_dk, \
                           qkv, wgmax, key_len, err_word);                                                                    \
        WR_LAUNCH_CHECK("sas_fwd_pre_kernel");                                                                                \
        hipLaunchKernelGGL((sas_fwd_main_kernel<D_, TM_, CAUSAL>), dim3((unsigned)B), dim3(kBlock), 0, stream, x, B, T, n_heads, P, \
                           sqrt_dk, dr, qkv, wgmax, n_max, out, gmax, key_len);                                               \
        WR_LAUNCH_CHECK("sas_fwd_main_kernel");                                                                               \
    } while (0)
    WR_SAS_DISPATCH(D, T, WR_SAS_FWD);
#undef WR_SAS_FWD
    return WR_OK;
}

template <bool CAUSAL>
static int32_t sas_bwd(const char *entry, const float *x, const float *grad_out, int64_t B, int32_t T, int32_t D, int32_t d_ff,
                       int32_t n_heads, const float *const *params, float p, uint64_t seed, int32_t training,
                       const int64_t *key_len, int32_t *err_word, const float *gmax, float *gx, float *gparams, void *workspace,
                       int64_t workspace_bytes, void *stream_) {
    int32_t rc = sas_check(entry, B, T, D, d_ff, n_heads);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(x && grad_out && gmax && gx && gparams && (CAUSAL || key_len), WR_E_NULL, "%s: NULL argument", entry);
    WR_REQUIRE(aligned16(x) && aligned16(grad_out) && aligned16(gx) && aligned16(gparams), WR_E_ALIGN,
               "%s: x, grad_out, gx and gparams must be 16-byte aligned", entry);
    SasParams P;
    if ((rc = sas_check_params(entry, params, P)) != WR_OK) return rc;
    SasDrop dr;
    if ((rc = sas_drop_of(entry, p, seed, training, dr)) != WR_OK) return rc;
    SasLayout L;
    sas_layout(B, T, D, L);
    if ((rc = check_workspace(entry, workspace, workspace_bytes, L.total)) != WR_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    float *part = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + L.part);
    const int n_wg = (int)(B < kSasBwdWg ? B : kSasBwdWg), n_par = 5 * D * D + 9 * D;
    const float sqrt_dk = sqrtf((float)(D / n_heads));
#define WR_SAS_BWD(D_, TM_)                                                                                                    \
    hipLaunchKernelGGL((sas_bwd_kernel<D_, TM_, CAUSAL>), dim3(n_wg), dim3(kBlock), 0, stream, x, grad_out, B, T, n_heads, P, sqrt_dk, \
                       dr, gmax, gx, part, key_len, err_word)
    WR_SAS_DISPATCH(D, T, WR_SAS_BWD);
#undef WR_SAS_BWD
    WR_LAUNCH_CHECK("sas_bwd_kernel");
    hipLaunchKernelGGL(sas_fold_kernel, dim3((n_par + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, part, n_wg, n_par, gparams);
    WR_LAUNCH_CHECK("sas_fold_kernel");
    return WR_OK;
}

extern "C" {

int32_t wr_sasblock_supported(int32_t D, int32_t d_ff, int32_t n_heads, int32_t T) {
    const bool ok = (D == 32 || D == 64) && d_ff == D && (n_heads == 1 || n_heads == 2 || n_heads == 4) && D / n_heads >= 8 &&
                    T >= 1 && T <= 64;
    return ok ? 1 : 0;
}

int64_t wr_sasblock_workspace_bytes(int64_t B, int32_t T, int32_t D, int32_t d_ff, int32_t n_heads) {
    const int32_t rc = sas_check("wr_sasblock_workspace_bytes", B, T, D, d_ff, n_heads);
    if (rc != WR_OK) return rc;
    SasLayout L;
    sas_layout(B, T, D, L);
    return L.total;
}

int32_t wr_sasblock_fwd(const float *x, int64_t B, int32_t T, int32_t D, int32_t d_ff, int32_t n_heads, const float *const *params,
                        float p, uint64_t seed, int32_t training, float *out, float *gmax, void *workspace, int64_t workspace_bytes,
                        void *stream) {
    return sas_fwd<true>("wr_sasblock_fwd", x, B, T, D, d_ff, n_heads, params, p, seed, training, nullptr, nullptr, out, gmax,
                         workspace, workspace_bytes, stream);
}

int32_t wr_sasblock_bwd(const float *x, const float *grad_out, int64_t B, int32_t T, int32_t D, int32_t d_ff, int32_t n_heads,
                        const float *const *params, float p, uint64_t seed, int32_t training, const float *gmax, float *gx,
                        float *gparams, void *workspace, int64_t workspace_bytes, void *stream) {
    return sas_bwd<true>("wr_sasblock_bwd", x, grad_out, B, T, D, d_ff, n_heads, params, p, seed, training, nullptr, nullptr, gmax,
                         gx, gparams, workspace, workspace_bytes, stream);
}

int32_t wr_sasblock_fwd_keys(const float *x, int64_t B, int32_t T, int32_t D, int32_t d_ff, int32_t n_heads,
                             const float *const *params, float p, uint64_t seed, int32_t training, float *out, float *gmax,
                             void *workspace, int64_t workspace_bytes, void *stream, const int64_t *key_len, int32_t *err_word) {
    return sas_fwd<false>("wr_sasblock_fwd_keys", x, B, T, D, d_ff, n_heads, params, p, seed, training, key_len, err_word, out, gmax,
                          workspace, workspace_bytes, stream);
}

int32_t wr_sasblock_bwd_keys(const float *x, const float *grad_out, int64_t B, int32_t T, int32_t D, int32_t d_ff, int32_t n_heads,
                             const float *const *params, float p, uint64_t seed, int32_t training, const float *gmax, float *gx,
                             float *gparams, void *workspace, int64_t workspace_bytes, void *stream, const int64_t *key_len,
                             int32_t *err_word) {
    return sas_bwd<false>("wr_sasblock_bwd_keys", x, grad_out, B, T, D, d_ff, n_heads, params, p, seed, training, key_len, err_word,
                          gmax, gx, gparams, workspace, workspace_bytes, stream);
}

}  // extern "C"
