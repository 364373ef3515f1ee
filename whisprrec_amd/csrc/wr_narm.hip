// wr_narm.hip — K28: NARM's additive attention pooling (Li et al., CIKM 2017; whisprrec_amd/narm.py, --pool_native 1) of the
// states hs [B, T, H] of a GRU against a query state h_g [B, H], forward and backward, fp32.  For row b, len = clamp(lengths[b],
// 0, T):
//   q = A1 h_g[b]          u_t = q + A2 hs[b, t]          e_t = v . sigmoid(u_t)          c[b] = sum_{t < len} e_t hs[b, t]
// A1, A2 [A, H], v [A]; no softmax (NARM's own form).  len = 0 gives zeros and no gradient.  hs[b, t, :] is never read for
// t >= len.  Supported (narm_supported, the one source of the set): H in {32, 64}, A in {16, 32, 64}, T >= 1.
//
// A wave owns a row b (rows wave, wave + 4 G, ... of the launch's G workgroups) and walks it in chunks of NT = 64 / A steps:
// lane (tt = lane / A, a = lane % A) forms u[t0 + tt][a] from the chunk's states in the wave's own piece of LDS, the A lanes of
// a step sum e_t with xor shuffles, and lane k < H adds e_t hs[t][k] for the chunk's steps in ascending t.  A1, A2 (rows of H + 4
// words: a lane reading its row as float4 and the lanes reading one column are both conflict-free) and v stay in LDS for the
// launch, 35 KB at A = H = 64 (33 KB without the pad words).  The next chunk is fetched while this one computes.  Plain FMAs: at most A H = 4,096 per step,
// and the operands come from LDS — the matrix cores would bring nothing (see wr_gru.hip).  Only waves synchronise: the rows of a
// workgroup's waves have lengths of their own.
//
// Backward, one launch and a fold: sigmoid(u_t) is recomputed; per chunk, with de_t = g_c . hs_t and du[t][a] = de_t v_a s (1 - s):
//   g_hs[b, t, k] = e_t g_c[k] + sum_a du[t][a] A2[a][k]   (zeros for t >= len, every element written)
//   g_h_g[b, k]   = sum_a dq_a A1[a][k],  dq_a = sum_t du[t][a]
//   g_A2[a][:] += du[t][a] hs_t,   g_A1[a][:] += dq_a h_g[b],   g_v[a] += de_t s       in the lane's registers (2 H + 1) across
// all its rows.  Each wave folds its NT partial sums with shuffles and writes one slab [A H | A H | A]; the second launch sums
// the slabs in (workgroup, wave) order.  No float atomics, no [B, T, A] array in memory; grid and order depend on (B, T, H, A)
// alone: same inputs, same bits.
#include <math.h>

#include "wr_common.h"

namespace wr {

constexpr int kNarmWaves = kBlock / 64;      // rows a workgroup holds at a time
constexpr int kNarmWg = 64;                  // workgroups at most: 256 slabs of parameter-gradient partials in the backward

static inline bool narm_supported(int32_t H, int32_t A, int32_t T) {
    return (H == 32 || H == 64) && (A == 16 || A == 32 || A == 64) && T >= 1;
}
static inline int64_t narm_slab_words(int H, int A) { return (int64_t)2 * A * H + A; }

template <int H, int A>
struct NarmShape {
    static constexpr int LD = H + 4;                        // words per LDS row of A1 / A2 and of a chunk's states
    static constexpr int NT = 64 / A;                       // steps of a chunk
    static constexpr int CH4 = NT * H / 4;                  // float4 of a chunk's states (<= 64: one per lane)
    static constexpr int W_WORDS = 2 * A * LD + A;          // A1 | A2 | v
    static constexpr int FWD_WAVE_WORDS = NT * LD + H;               // a wave's piece of LDS, forward: hs chunk | h_g
    static constexpr int WAVE_WORDS = NT * LD + 2 * H + 64 + A;      // backward: hs chunk | h_g | g_c | du [NT][A] | dq [A]
    static constexpr int SLAB = 2 * A * H + A;
};

struct NarmParams {
    const float *hs, *h_g, *A1, *A2, *v;
    const int64_t *lengths;
    int64_t B;
    int T;
};

__device__ __forceinline__ float narm_sigmoid(float a) { return 1.0f / (1.0f + expf(-a)); }

// the lanes of one wave hand LDS words to each other
__device__ __forceinline__ void narm_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int H, int A>
__device__ __forceinline__ void narm_load_weights(const NarmParams &P, float *W1, float *W2, float *vs) {
    using S = NarmShape<H, A>;
    for (int idx = threadIdx.x; idx < A * H / 4; idx += kBlock) {
        const int row = idx / (H / 4), c = idx - row * (H / 4);
        *reinterpret_cast<float4 *>(W1 + row * S::LD + 4 * c) = reinterpret_cast<const float4 *>(P.A1)[idx];
        *reinterpret_cast<float4 *>(W2 + row * S::LD + 4 * c) = reinterpret_cast<const float4 *>(P.A2)[idx];
    }
    if (threadIdx.x < A) vs[threadIdx.x] = P.v[threadIdx.x];
}

__device__ __forceinline__ int narm_length(const NarmParams &P, int64_t b) {
    const int64_t l = P.lengths[b];
    return (int)(l < 0 ? 0 : (l > P.T ? P.T : l));
}

// sum over the A lanes of a step (every one of them gets it)
template <int A>
__device__ __forceinline__ float narm_sum_a(float x) {
#pragma unroll
    for (int off = 1; off < A; off <<= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// sum over the 64 / A lanes that hold the same a (every one of them gets it)
template <int A>
__device__ __forceinline__ float narm_sum_tt(float x) {
#pragma unroll
    for (int off = A; off < 64; off <<= 1) x += __shfl_xor(x, off, 64);
    return x;
}

template <int H, int A>
__global__ __launch_bounds__(kBlock) void narm_pool_fwd_kernel(NarmParams P, float *__restrict__ c) {
    using S = NarmShape<H, A>;
    __shared__ float4 narm_lds4[(S::W_WORDS + kNarmWaves * S::FWD_WAVE_WORDS) / 4];
    float *W1 = reinterpret_cast<float *>(narm_lds4), *W2 = W1 + A * S::LD, *vs = W2 + A * S::LD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = lane % A, tt = lane / A, T = P.T;
    float *hsb = W1 + S::W_WORDS + wave * S::FWD_WAVE_WORDS, *hg = hsb + S::NT * S::LD;
    narm_load_weights<H, A>(P, W1, W2, vs);
    __syncthreads();
    const float va = vs[a];
    const int tl = lane / (H / 4), cl = lane - tl * (H / 4);      // this lane's float4 of a chunk (lane < CH4)
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t b = (int64_t)blockIdx.x * kNarmWaves + wave; b < P.B; b += (int64_t)gridDim.x * kNarmWaves) {
        const int len = narm_length(P, b);
        narm_wave_sync();      // the last row's readers are done
        if (lane < H) hg[lane] = P.h_g[b * H + lane];
        narm_wave_sync();
        float q = 0.f;
#pragma unroll
        for (int k4 = 0; k4 < H / 4; ++k4) {
            const float4 w = *reinterpret_cast<const float4 *>(W1 + a * S::LD + 4 * k4);
            const float4 x = *reinterpret_cast<const float4 *>(hg + 4 * k4);
            q = fmaf(w.w, x.w, fmaf(w.z, x.z, fmaf(w.y, x.y, fmaf(w.x, x.x, q))));
        }
        const float4 *hp = reinterpret_cast<const float4 *>(P.hs + b * (int64_t)T * H) + lane;      // + t0 H / 4
        float4 nx = zero4;
        if (lane < S::CH4 && tl < len) nx = hp[0];
        float acc = 0.f;
        for (int t0 = 0; t0 < len; t0 += S::NT) {
            if (lane < S::CH4) *reinterpret_cast<float4 *>(hsb + tl * S::LD + 4 * cl) = nx;
            narm_wave_sync();      // the chunk's states are in LDS (zeros for the steps past the length)
            nx = zero4;
            if (lane < S::CH4 && t0 + S::NT + tl < len) nx = hp[(int64_t)(t0 + S::NT) * (H / 4)];
            float u = q;
#pragma unroll
            for (int k4 = 0; k4 < H / 4; ++k4) {
                const float4 w = *reinterpret_cast<const float4 *>(W2 + a * S::LD + 4 * k4);
                const float4 x = *reinterpret_cast<const float4 *>(hsb + tt * S::LD + 4 * k4);
                u = fmaf(w.w, x.w, fmaf(w.z, x.z, fmaf(w.y, x.y, fmaf(w.x, x.x, u))));
            }
            float es = 0.f;
            if (t0 + tt < len) es = va * narm_sigmoid(u);
            const float e = narm_sum_a<A>(es);
#pragma unroll
            for (int s = 0; s < S::NT; ++s) {
                const float et = __shfl(e, s * A, 64);
                if (lane < H) acc = fmaf(et, hsb[s * S::LD + lane], acc);
            }
            narm_wave_sync();      // every read of the chunk is done
        }
        if (lane < H) c[b * H + lane] = acc;
    }
}

template <int H, int A>
__global__ __launch_bounds__(kBlock) void narm_pool_bwd_kernel(NarmParams P, const float *__restrict__ g_c, float *__restrict__ g_hs,
                                                               float *__restrict__ g_h_g, float *__restrict__ slabs) {
    using S = NarmShape<H, A>;
    __shared__ float4 narm_lds4[(S::W_WORDS + kNarmWaves * S::WAVE_WORDS) / 4];
    float *W1 = reinterpret_cast<float *>(narm_lds4), *W2 = W1 + A * S::LD, *vs = W2 + A * S::LD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = lane % A, tt = lane / A, T = P.T;
    float *hsb = W1 + S::W_WORDS + wave * S::WAVE_WORDS, *hg = hsb + S::NT * S::LD, *gc = hg + H, *dub = gc + H, *dqb = dub + 64;
    narm_load_weights<H, A>(P, W1, W2, vs);
    __syncthreads();
    const float va = vs[a];
    const int tl = lane / (H / 4), cl = lane - tl * (H / 4);      // this lane's float4 of a chunk (lane < CH4)
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float acc1[H], acc2[H], accv = 0.f;      // this lane's sums for g_A1[a][:], g_A2[a][:], g_v[a] over its steps tt, tt + NT, ...
#pragma unroll
    for (int k = 0; k < H; ++k) acc1[k] = acc2[k] = 0.f;
    for (int64_t b = (int64_t)blockIdx.x * kNarmWaves + wave; b < P.B; b += (int64_t)gridDim.x * kNarmWaves) {
        const int len = narm_length(P, b);
        narm_wave_sync();      // the last row's readers are done
        if (lane < H) {
            hg[lane] = P.h_g[b * H + lane];
            gc[lane] = g_c[b * H + lane];
        }
        narm_wave_sync();
        float q = 0.f;
#pragma unroll
        for (int k4 = 0; k4 < H / 4; ++k4) {
            const float4 w = *reinterpret_cast<const float4 *>(W1 + a * S::LD + 4 * k4);
            const float4 x = *reinterpret_cast<const float4 *>(hg + 4 * k4);
            q = fmaf(w.w, x.w, fmaf(w.z, x.z, fmaf(w.y, x.y, fmaf(w.x, x.x, q))));
        }
        const float4 *hp = reinterpret_cast<const float4 *>(P.hs + b * (int64_t)T * H) + lane;      // + t0 H / 4
        float *gout = g_hs + b * (int64_t)T * H + lane;                                              // + t H
        float4 nx = zero4;
        if (lane < S::CH4 && tl < len) nx = hp[0];
        float dqp = 0.f;
        for (int t0 = 0; t0 < T; t0 += S::NT) {
            if (t0 >= len) {      // the same for the whole wave: steps the row does not take
                if (lane < H) {
#pragma unroll
                    for (int s = 0; s < S::NT; ++s)
                        if (t0 + s < T) gout[(int64_t)(t0 + s) * H] = 0.f;
                }
                continue;
            }
            if (lane < S::CH4) *reinterpret_cast<float4 *>(hsb + tl * S::LD + 4 * cl) = nx;
            narm_wave_sync();      // the chunk's states are in LDS (zeros for the steps past the length)
            nx = zero4;
            if (lane < S::CH4 && t0 + S::NT + tl < len) nx = hp[(int64_t)(t0 + S::NT) * (H / 4)];
            float u = q, de = 0.f;
#pragma unroll
            for (int k4 = 0; k4 < H / 4; ++k4) {
                const float4 w = *reinterpret_cast<const float4 *>(W2 + a * S::LD + 4 * k4);
                const float4 x = *reinterpret_cast<const float4 *>(hsb + tt * S::LD + 4 * k4);
                const float4 g = *reinterpret_cast<const float4 *>(gc + 4 * k4);
                u = fmaf(w.w, x.w, fmaf(w.z, x.z, fmaf(w.y, x.y, fmaf(w.x, x.x, u))));
                de = fmaf(g.w, x.w, fmaf(g.z, x.z, fmaf(g.y, x.y, fmaf(g.x, x.x, de))));
            }
            float es = 0.f, du = 0.f;
            if (t0 + tt < len) {
                const float s = narm_sigmoid(u);
                es = va * s;
                du = de * va * s * (1.0f - s);
                accv = fmaf(de, s, accv);
            }
            const float e = narm_sum_a<A>(es);
            dqp += du;
            dub[lane] = du;      // [tt][a]
#pragma unroll
            for (int k4 = 0; k4 < H / 4; ++k4) {
                const float4 x = *reinterpret_cast<const float4 *>(hsb + tt * S::LD + 4 * k4);
                acc2[4 * k4] = fmaf(du, x.x, acc2[4 * k4]);
                acc2[4 * k4 + 1] = fmaf(du, x.y, acc2[4 * k4 + 1]);
                acc2[4 * k4 + 2] = fmaf(du, x.z, acc2[4 * k4 + 2]);
                acc2[4 * k4 + 3] = fmaf(du, x.w, acc2[4 * k4 + 3]);
            }
            narm_wave_sync();      // du of the chunk is in LDS
#pragma unroll
            for (int s = 0; s < S::NT; ++s) {
                const float et = __shfl(e, s * A, 64);
                if (lane < H && t0 + s < T) {
                    float g = et * gc[lane];
#pragma unroll 8
                    for (int r = 0; r < A; ++r) g = fmaf(dub[s * A + r], W2[r * S::LD + lane], g);
                    gout[(int64_t)(t0 + s) * H] = t0 + s < len ? g : 0.f;
                }
            }
            narm_wave_sync();      // every read of the chunk and of du is done
        }
#pragma unroll
        for (int k4 = 0; k4 < H / 4; ++k4) {
            const float4 x = *reinterpret_cast<const float4 *>(hg + 4 * k4);
            acc1[4 * k4] = fmaf(dqp, x.x, acc1[4 * k4]);
            acc1[4 * k4 + 1] = fmaf(dqp, x.y, acc1[4 * k4 + 1]);
            acc1[4 * k4 + 2] = fmaf(dqp, x.z, acc1[4 * k4 + 2]);
            acc1[4 * k4 + 3] = fmaf(dqp, x.w, acc1[4 * k4 + 3]);
        }
        const float dq = narm_sum_tt<A>(dqp);
        if (tt == 0) dqb[a] = dq;
        narm_wave_sync();
        if (lane < H) {
            float g = 0.f;
#pragma unroll 8
            for (int r = 0; r < A; ++r) g = fmaf(dqb[r], W1[r * S::LD + lane], g);
            g_h_g[b * H + lane] = g;
        }
    }
    // this wave's slab: [A][H] | [A][H] | [A], the NT partial sums of an a folded first
    float *slab = slabs + ((int64_t)blockIdx.x * kNarmWaves + wave) * S::SLAB;
#pragma unroll
    for (int k = 0; k < H; ++k) {
        const float s1 = narm_sum_tt<A>(acc1[k]), s2 = narm_sum_tt<A>(acc2[k]);
        if (tt == 0) {
            slab[a * H + k] = s1;
            slab[A * H + a * H + k] = s2;
        }
    }
    const float sv = narm_sum_tt<A>(accv);
    if (tt == 0) slab[2 * A * H + a] = sv;
}

// element e of [g_A1 | g_A2 | g_v]: the slabs summed in (workgroup, wave) order, eight loads in flight
__global__ __launch_bounds__(kBlock) void narm_fold_kernel(const float *__restrict__ slabs, int n_slabs, int n_w, int n_v,
                                                            float *__restrict__ g_A1, float *__restrict__ g_A2, float *__restrict__ g_v) {
    const int total = 2 * n_w + n_v;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    float v = 0.f;
    int w = 0;
    for (; w + 8 <= n_slabs; w += 8) {
        float p[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u] = slabs[(int64_t)(w + u) * total + e];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += p[u];
    }
    for (; w < n_slabs; ++w) v += slabs[(int64_t)w * total + e];
    if (e < n_w) g_A1[e] = v;
    else if (e < 2 * n_w) g_A2[e - n_w] = v;
    else g_v[e - 2 * n_w] = v;
}

static int32_t narm_check(const char *entry, const float *hs, const float *h_g, const int64_t *lengths, const float *A1,
                          const float *A2, const float *v, int64_t B, int32_t T, int32_t H, int32_t A) {
    WR_REQUIRE(narm_supported(H, A, T), WR_E_RANGE, "%s supports H in {32, 64}, A in {16, 32, 64}, T >= 1; got H=%d A=%d T=%d", entry,
               H, A, T);
    WR_REQUIRE(hs && h_g && lengths && A1 && A2 && v, WR_E_NULL, "%s: NULL argument", entry);
    WR_REQUIRE(B >= 1 && B <= (int64_t(1) << 24), WR_E_SHAPE, "%s: B=%lld out of range (1..2^24)", entry, (long long)B);
    WR_REQUIRE(aligned16(hs) && aligned16(A1) && aligned16(A2), WR_E_ALIGN, "%s: hs, A1 and A2 must be 16-byte aligned", entry);
    return WR_OK;
}

static inline unsigned narm_grid(int64_t B) {
    const int64_t n = (B + kNarmWaves - 1) / kNarmWaves;
    return (unsigned)(n < kNarmWg ? n : kNarmWg);
}

#define WR_NARM_DISPATCH(H, A, CALL)                  \
    do {                                              \
        if ((H) == 64 && (A) == 16) { CALL(64, 16); } \
        else if ((H) == 64 && (A) == 32) { CALL(64, 32); } \
        else if ((H) == 64) { CALL(64, 64); }         \
        else if ((A) == 16) { CALL(32, 16); }         \
        else if ((A) == 32) { CALL(32, 32); }         \
        else { CALL(32, 64); }                        \
    } while (0)

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_narm_pool_supported(int32_t H, int32_t A, int32_t T) { return narm_supported(H, A, T) ? 1 : 0; }

int64_t wr_narm_pool_workspace_bytes(int64_t B, int32_t T, int32_t H, int32_t A) {
    WR_REQUIRE(narm_supported(H, A, T) && B >= 1 && B <= (int64_t(1) << 24), WR_E_RANGE,
               "wr_narm_pool_workspace_bytes supports H in {32, 64}, A in {16, 32, 64}, T >= 1, 1 <= B <= 2^24; got B=%lld T=%d H=%d "
               "A=%d", (long long)B, T, H, A);
    return align_up((int64_t)kNarmWg * kNarmWaves * narm_slab_words(H, A) * 4, 256);      // sized by the bound, not by B
}

int32_t wr_narm_pool_fwd(const float *hs, const float *h_g, const int64_t *lengths, const float *A1, const float *A2, const float *v,
                         int64_t B, int32_t T, int32_t H, int32_t A, float *c, void *stream_) {
    const char *entry = "wr_narm_pool_fwd";
    const int32_t rc = narm_check(entry, hs, h_g, lengths, A1, A2, v, B, T, H, A);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(c != nullptr, WR_E_NULL, "%s: NULL argument", entry);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const NarmParams P{hs, h_g, A1, A2, v, lengths, B, T};
    const unsigned grid = narm_grid(B);
#define WR_NARM_FWD(H_, A_) hipLaunchKernelGGL((narm_pool_fwd_kernel<H_, A_>), dim3(grid), dim3(kBlock), 0, stream, P, c)
    WR_NARM_DISPATCH(H, A, WR_NARM_FWD);
#undef WR_NARM_FWD
    WR_LAUNCH_CHECK("narm_pool_fwd_kernel");
    return WR_OK;
}

int32_t wr_narm_pool_bwd(const float *hs, const float *h_g, const int64_t *lengths, const float *A1, const float *A2, const float *v,
                         const float *g_c, int64_t B, int32_t T, int32_t H, int32_t A, float *g_hs, float *g_h_g, float *g_A1,
                         float *g_A2, float *g_v, void *workspace, int64_t workspace_bytes, void *stream_) {
    const char *entry = "wr_narm_pool_bwd";
    int32_t rc = narm_check(entry, hs, h_g, lengths, A1, A2, v, B, T, H, A);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(g_c && g_hs && g_h_g && g_A1 && g_A2 && g_v, WR_E_NULL, "%s: NULL argument", entry);
    if ((rc = check_workspace(entry, workspace, workspace_bytes, wr_narm_pool_workspace_bytes(B, T, H, A))) != WR_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const NarmParams P{hs, h_g, A1, A2, v, lengths, B, T};
    const unsigned grid = narm_grid(B);
    float *slabs = reinterpret_cast<float *>(workspace);
#define WR_NARM_BWD(H_, A_) \
    hipLaunchKernelGGL((narm_pool_bwd_kernel<H_, A_>), dim3(grid), dim3(kBlock), 0, stream, P, g_c, g_hs, g_h_g, slabs)
    WR_NARM_DISPATCH(H, A, WR_NARM_BWD);
#undef WR_NARM_BWD
    WR_LAUNCH_CHECK("narm_pool_bwd_kernel");
    const int n_w = A * H, total = 2 * n_w + A;
    hipLaunchKernelGGL(narm_fold_kernel, dim3((total + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, slabs,
                       (int)grid * kNarmWaves, n_w, A, g_A1, g_A2, g_v);
    WR_LAUNCH_CHECK("narm_fold_kernel");
    return WR_OK;
}

}  // extern "C"
