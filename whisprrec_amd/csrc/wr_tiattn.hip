// wr_tiattn.hip — K25: time-interval attention (reference src/utils/layers.py:105-146, TimeIntervalMultiHeadAttention after its
// projections), forward and backward, without the two gathered [B, T, T, D] arrays (inter_k, inter_v) in global memory.
//
// For sequence b with q, k, v [T, D] (the caller has added the position terms to k and v), timestamps t [T], scale m_b and the
// tables time_k, time_v [time_max + 1, D]; head h owns columns h d_k .. (h + 1) d_k - 1; for j <= i:
//   r_ij   = min(|t_i - t_j| / m_b, time_max)                 integer (floor) division in 64 bits
//   s_ij^h = <q_i^h, k_j^h + time_k[r_ij]^h> / sqrt(d_k)
//   p_i.^h = softmax_j s_i.^h
//   out_i^h = sum_j p_ij^h (v_j^h + time_v[r_ij]^h)
// Supported (ti_supported, the one source of the set): D in {32, 64}, n_heads in {1, 2, 4} with D / n_heads >= 8, 1 <= T <= 64,
// 1 <= time_max <= 2048 (the intervals travel as 12-bit fields of the sort keys, and the backward's workspace grows with it).
//
// One workgroup works on one sequence at a time.  q, k, v sit in LDS in the [T][D + 1] layout of the block kernels
// (wr_sasblock.hip), the intervals as one 16-bit value per pair (i, j <= i) and the probabilities of all heads as triangular
// rows [h][i (i + 1) / 2 + j]; the table rows are read from global memory (two tables of 513 x 64 floats stay in L2) while the
// scores and the weighted sums are formed.  Nothing with T^2 elements per sequence ever leaves the CU.
//
// The global maximum.  The reference subtracts the maximum over the WHOLE call before softmax (:143).  This kernel uses each
// row's own maximum: the two agree wherever the reference is finite (the argument of wr_if4rec.hip's header), and where a row's
// shifted exponentials all underflow the reference gives NaN (this layer has no isnan fill) and this kernel the ordinary softmax.
//
// Backward.  The forward of a sequence is recomputed; nothing is saved.  dq, dk, dv are written per sequence.  The table
// gradients
//   d time_k[r] += ds_ij^h q_i^h      d time_v[r] += p_ij^h d out_i^h       over every (b, h, i, j) with r_ij = r
// are T (T + 1) / 2 contributions per sequence that mostly land on two rows (interval 0 and interval time_max).  No float
// atomics: the pairs of a sequence are ordered by (r, i, j) with a bitonic sort of unique 24-bit keys in LDS, the runs of equal r
// are summed column by column in that order (one lane per column, all heads at once), and each run is added to the workgroup's
// OWN slab [2][time_max + 1][D] of the workspace — one writer per slab, sequences in ascending order.  A second launch folds the
// slabs in workgroup order (the scheme of sas_fold_kernel).  Every sum has a fixed order: same inputs, same bits.
//
// m_b < 1 is clamped to 1 and ORs 1 into err_word; no host round trip.
#include "wr_common.h"

namespace wr {

constexpr int kTiMaxT = 64, kTiMaxTimeMax = 2048;
constexpr int kTiFwdWg = 4096;   // forward: workgroups at most (they stride over the sequences)
constexpr int kTiBwdWg = 256;    // backward: slabs of table-gradient partials at most

static inline bool ti_supported(int32_t D, int32_t H, int32_t T, int32_t time_max) {
    return (D == 32 || D == 64) && (H == 1 || H == 2 || H == 4) && D / H >= 8 && T >= 1 && T <= kTiMaxT && time_max >= 1 &&
           time_max <= kTiMaxTimeMax;
}

__host__ __device__ __forceinline__ int ti_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

struct TiLds {
    long long *tm;            // [T] timestamps
    float *q, *k, *v, *go;    // [T][D + 1]
    float *P, *dS;            // [H][N] triangular rows
    unsigned short *r;        // [N] interval of pair i (i + 1) / 2 + j
    unsigned *keys;           // [pow2(N)] r << 12 | i << 6 | j, sorted
    unsigned short *segs;     // [n_seg + 1] first sorted position of each run of equal r
    int *scr;                 // [16]
};

// 4-byte words of dynamic LDS; at T = 64, D = 64, 4 heads: 87,936 B forward, 158,404 B backward
__host__ __device__ __forceinline__ int ti_lds_words(int D, int T, int H, bool bwd) {
    const int N = T * (T + 1) / 2, LDW = D + 1;
    int n = 2 * T + 3 * T * LDW + H * N + (N + 1) / 2 + 16;
    if (bwd) n += T * LDW + H * N + ti_pow2(N) + (N + 2) / 2;
    return n;
}

template <int D>
__device__ __forceinline__ TiLds ti_carve(float *lds, int T, int H, bool bwd) {
    constexpr int LDW = D + 1;
    const int N = T * (T + 1) / 2;
    TiLds L;
    L.tm = reinterpret_cast<long long *>(lds);            // first: the base is 16-byte aligned
    L.q = lds + 2 * T;
    L.k = L.q + T * LDW;
    L.v = L.k + T * LDW;
    L.P = L.v + T * LDW;
    float *p = L.P + H * N;
    L.r = reinterpret_cast<unsigned short *>(p);
    p += (N + 1) / 2;
    L.scr = reinterpret_cast<int *>(p);
    p += 16;
    L.go = L.dS = nullptr;
    L.keys = nullptr;
    L.segs = nullptr;
    if (bwd) {
        L.go = p;
        L.dS = L.go + T * LDW;
        p = L.dS + H * N;
        L.keys = reinterpret_cast<unsigned *>(p);
        p += ti_pow2(N);
        L.segs = reinterpret_cast<unsigned short *>(p);
    }
    return L;
}

struct TiParams {
    const float *q, *k, *v, *tk, *tv;
    const int64_t *times, *min_interval;
    int64_t B;
    int T, H, time_max;
    float scale;              // 1 / sqrt(d_k)
};

// pair number p = i (i + 1) / 2 + j  ->  (i, j), j <= i.  8 p + 1 <= 16,641 is exact in fp32 and the root is correctly rounded;
// the two comparisons take back a floor that landed one off.
__device__ __forceinline__ void ti_pair(int p, int &i, int &j) {
    i = (int)((__fsqrt_rn(8.f * (float)p + 1.f) - 1.f) * 0.5f);
    if (i * (i + 1) / 2 > p) --i;
    else if ((i + 1) * (i + 2) / 2 <= p) ++i;
    j = p - i * (i + 1) / 2;
}

__device__ __forceinline__ void ti_rows_to_lds(float *dst, const float *__restrict__ src, int T, int D, int LDW) {
    const int D4 = D / 4;
    for (int f = threadIdx.x; f < T * D4; f += kBlock) {
        const int t = f / D4, c = f - t * D4;
        const float4 x = reinterpret_cast<const float4 *>(src + (int64_t)t * D)[c];
        float *o = dst + t * LDW + 4 * c;
        o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = x.w;
    }
}

// <a[0..dk), b[0..dk) + tab[0..dk)> with a, b in LDS and tab a 16-byte aligned piece of a table row
__device__ __forceinline__ float ti_dot_shifted(const float *a, const float *b, const float *__restrict__ tab, int dk) {
    float s = 0.f;
    for (int d = 0; d < dk; d += 4) {
        const float4 t = *reinterpret_cast<const float4 *>(tab + d);
        s = fmaf(a[d], b[d] + t.x, s);
        s = fmaf(a[d + 1], b[d + 1] + t.y, s);
        s = fmaf(a[d + 2], b[d + 2] + t.z, s);
        s = fmaf(a[d + 3], b[d + 3] + t.w, s);
    }
    return s;
}

// q, k, v, the intervals and the probabilities of all heads of sequence b; ends with a barrier
template <int D>
__device__ __forceinline__ void ti_forward_seq(const TiLds &L, const TiParams &P, int64_t b, int32_t *__restrict__ err_word) {
    constexpr int LDW = D + 1;
    const int T = P.T, H = P.H, N = T * (T + 1) / 2, dk = D / H, tid = threadIdx.x;
    ti_rows_to_lds(L.q, P.q + b * T * D, T, D, LDW);
    ti_rows_to_lds(L.k, P.k + b * T * D, T, D, LDW);
    ti_rows_to_lds(L.v, P.v + b * T * D, T, D, LDW);
    if (tid < T) L.tm[tid] = P.times[b * T + tid];
    long long m = P.min_interval[b];
    if (m < 1) {                                          // clamped before it divides anything
        if (tid == 0 && err_word != nullptr) atomicOr(err_word, 1);
        m = 1;
    }
    __syncthreads();
    for (int p = tid; p < N; p += kBlock) {
        int i, j;
        ti_pair(p, i, j);
        const long long a = L.tm[i], c = L.tm[j];
        const unsigned long long gap = a > c ? (unsigned long long)a - (unsigned long long)c
                                             : (unsigned long long)c - (unsigned long long)a;
        const unsigned long long quo = gap / (unsigned long long)m;
        L.r[p] = (unsigned short)(quo > (unsigned long long)P.time_max ? (unsigned long long)P.time_max : quo);
    }
    __syncthreads();
    for (int e = tid; e < H * N; e += kBlock) {
        const int h = e / N, p = e - h * N;
        int i, j;
        ti_pair(p, i, j);
        const float s = ti_dot_shifted(L.q + i * LDW + h * dk, L.k + j * LDW + h * dk, P.tk + (int64_t)L.r[p] * D + h * dk, dk);
        L.P[e] = s * P.scale;
    }
    __syncthreads();
    for (int row = tid; row < H * T; row += kBlock) {    // softmax over j <= i with the row's own maximum
        const int h = row / T, i = row - h * T;
        float *s = L.P + h * N + i * (i + 1) / 2;
        float mx = s[0];
        for (int j = 1; j <= i; ++j) mx = fmaxf(mx, s[j]);
        float z = 0.f;
        for (int j = 0; j <= i; ++j) {
            const float e = expf(s[j] - mx);
            s[j] = e;
            z += e;
        }
        const float inv = 1.f / z;
        for (int j = 0; j <= i; ++j) s[j] *= inv;
    }
    __syncthreads();
}

template <int D>
__global__ __launch_bounds__(kBlock) void ti_fwd_kernel(TiParams P, float *__restrict__ out, int32_t *__restrict__ err_word) {
    extern __shared__ float ti_lds[];
    const TiLds L = ti_carve<D>(ti_lds, P.T, P.H, false);
    constexpr int LDW = D + 1;
    const int T = P.T, N = T * (T + 1) / 2, dk = D / P.H;
    for (int64_t b = blockIdx.x; b < P.B; b += gridDim.x) {
        ti_forward_seq<D>(L, P, b, err_word);
        for (int e = threadIdx.x; e < T * D; e += kBlock) {
            const int i = e / D, d = e - i * D, h = d / dk, row = i * (i + 1) / 2;
            const float *pr = L.P + h * N + row;
            const unsigned short *rr = L.r + row;
            float s = 0.f;
            for (int j = 0; j <= i; ++j) s = fmaf(pr[j], L.v[j * LDW + d] + P.tv[(int64_t)rr[j] * D + d], s);
            out[(b * T + i) * D + d] = s;
        }
        __syncthreads();
    }
}

// slab layout of one workgroup: [2 (time_k, time_v)][time_max + 1][D]
template <int D>
__global__ __launch_bounds__(kBlock) void ti_bwd_kernel(TiParams P, const float *__restrict__ g_out, float *__restrict__ gq,
                                                         float *__restrict__ gk, float *__restrict__ gv, float *__restrict__ slabs,
                                                         int32_t *__restrict__ err_word) {
    extern __shared__ float ti_lds[];
    const TiLds L = ti_carve<D>(ti_lds, P.T, P.H, true);
    constexpr int LDW = D + 1, NG = kBlock / D;
    const int T = P.T, H = P.H, N = T * (T + 1) / 2, NP2 = ti_pow2(N), dk = D / H, tid = threadIdx.x;
    const int64_t slab_floats = (int64_t)2 * (P.time_max + 1) * D;
    float *slab = slabs + (int64_t)blockIdx.x * slab_floats;
    for (int64_t f = tid; f < slab_floats / 4; f += kBlock) reinterpret_cast<float4 *>(slab)[f] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    for (int64_t b = blockIdx.x; b < P.B; b += gridDim.x) {
        ti_rows_to_lds(L.go, g_out + b * T * D, T, D, LDW);
        ti_forward_seq<D>(L, P, b, err_word);
        for (int e = tid; e < H * N; e += kBlock) {       // dL/dp_ij = <d out_i, v_j + time_v[r_ij]>
            const int h = e / N, p = e - h * N;
            int i, j;
            ti_pair(p, i, j);
            L.dS[e] = ti_dot_shifted(L.go + i * LDW + h * dk, L.v + j * LDW + h * dk, P.tv + (int64_t)L.r[p] * D + h * dk, dk);
        }
        __syncthreads();
        for (int row = tid; row < H * T; row += kBlock) {    // softmax backward, times 1 / sqrt(d_k): ds w.r.t. the plain products
            const int h = row / T, i = row - h * T, at = h * N + i * (i + 1) / 2;
            const float *pr = L.P + at;
            float *ds = L.dS + at;
            float dot = 0.f;
            for (int j = 0; j <= i; ++j) dot = fmaf(pr[j], ds[j], dot);
            for (int j = 0; j <= i; ++j) ds[j] = pr[j] * (ds[j] - dot) * P.scale;
        }
        // the sort keys of the pairs: r << 12 | i << 6 | j (unique), padding above every key
        for (int s = tid; s < NP2; s += kBlock) {
            unsigned key = 0xFFFFFFFFu;
            if (s < N) {
                int i, j;
                ti_pair(s, i, j);
                key = ((unsigned)L.r[s] << 12) | ((unsigned)i << 6) | (unsigned)j;
            }
            L.keys[s] = key;
        }
        __syncthreads();
        for (int e = tid; e < T * D; e += kBlock) {       // dq_i = sum_j ds_ij (k_j + time_k[r_ij])
            const int i = e / D, d = e - i * D, h = d / dk, row = i * (i + 1) / 2;
            const float *ds = L.dS + h * N + row;
            const unsigned short *rr = L.r + row;
            float s = 0.f;
            for (int j = 0; j <= i; ++j) s = fmaf(ds[j], L.k[j * LDW + d] + P.tk[(int64_t)rr[j] * D + d], s);
            gq[(b * T + i) * D + d] = s;
        }
        for (int e = tid; e < T * D; e += kBlock) {       // dk_j = sum_{i >= j} ds_ij q_i, dv_j = sum_{i >= j} p_ij d out_i
            const int j = e / D, d = e - j * D, h = d / dk;
            const float *ds = L.dS + h * N, *pr = L.P + h * N;
            float sk = 0.f, sv = 0.f;
            for (int i = j; i < T; ++i) {
                const int at = i * (i + 1) / 2 + j;
                sk = fmaf(ds[at], L.q[i * LDW + d], sk);
                sv = fmaf(pr[at], L.go[i * LDW + d], sv);
            }
            gk[(b * T + j) * D + d] = sk;
            gv[(b * T + j) * D + d] = sv;
        }
        // bitonic sort of the keys (ascending); nothing above reads or writes them
        for (int k = 2; k <= NP2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < NP2; t += kBlock) {
                    const int u = t ^ j;
                    if (u > t) {
                        const unsigned a = L.keys[t], c = L.keys[u];
                        if ((a > c) == ((t & k) == 0)) {
                            L.keys[t] = c;
                            L.keys[u] = a;
                        }
                    }
                }
                __syncthreads();
            }
        }
        // runs of equal r: thread t owns sorted positions [t per, (t + 1) per); an exclusive scan of the heads it holds
        const int per = (N + kBlock - 1) / kBlock, lo = tid * per, hi = lo + per < N ? lo + per : N;
        int cnt = 0;
        for (int s = lo; s < hi; ++s) cnt += (s == 0 || (L.keys[s] >> 12) != (L.keys[s - 1] >> 12)) ? 1 : 0;
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if ((tid & 63) >= o) incl += up;
        }
        if ((tid & 63) == 63) L.scr[tid >> 6] = incl;
        __syncthreads();
        int at = incl - cnt, n_seg = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) {
            if (w < (tid >> 6)) at += L.scr[w];
            n_seg += L.scr[w];
        }
        for (int s = lo; s < hi; ++s)
            if (s == 0 || (L.keys[s] >> 12) != (L.keys[s - 1] >> 12)) L.segs[at++] = (unsigned short)s;
        if (tid == 0) L.segs[n_seg] = (unsigned short)N;
        __syncthreads();
        // task 2 seg + tab: the run's sum in sorted order, lane d for column d, added to this workgroup's slab
        {
            const int g = tid / D, d = tid - g * D, h = d / dk;
            for (int t = g; t < 2 * n_seg; t += NG) {
                const int seg = t >> 1, tab = t & 1, s0 = L.segs[seg], s1 = L.segs[seg + 1];
                const int r = (int)(L.keys[s0] >> 12);
                float *dst = slab + ((int64_t)tab * (P.time_max + 1) + r) * D + d;
                const float old = *dst;
                const float *coef = (tab ? L.P : L.dS) + h * N;
                const float *vec = (tab ? L.go : L.q) + d;
                float acc = 0.f;
                for (int s = s0; s < s1; ++s) {
                    const unsigned key = L.keys[s];
                    const int i = (int)((key >> 6) & 63u), j = (int)(key & 63u);
                    acc = fmaf(coef[i * (i + 1) / 2 + j], vec[i * LDW], acc);
                }
                *dst = old + acc;
            }
        }
        __syncthreads();    // the next sequence rewrites LDS, and other lanes may own this sequence's slab rows then
    }
}

// element e of [d time_k | d time_v]: the slabs summed in workgroup order
__global__ __launch_bounds__(kBlock) void ti_fold_kernel(const float *__restrict__ slabs, int n_slabs, int n_tab, float *__restrict__ g_tk,
                                                          float *__restrict__ g_tv) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= 2 * n_tab) return;
    float v = 0.f;
    for (int w = 0; w < n_slabs; ++w) v += slabs[(int64_t)w * 2 * n_tab + e];
    if (e < n_tab) g_tk[e] = v;
    else g_tv[e - n_tab] = v;
}

static int32_t ti_check(const char *entry, const float *q, const float *k, const float *v, const int64_t *times,
                        const int64_t *min_interval, int64_t B, int32_t T, int32_t D, int32_t H, const float *time_k,
                        const float *time_v, int32_t time_max) {
    WR_REQUIRE(ti_supported(D, H, T, time_max), WR_E_RANGE,
               "%s supports D in {32, 64}, n_heads in {1, 2, 4} with D / n_heads >= 8, 1 <= T <= %d, 1 <= time_max <= %d; got D=%d "
               "n_heads=%d T=%d time_max=%d", entry, kTiMaxT, kTiMaxTimeMax, D, H, T, time_max);
    WR_REQUIRE(q && k && v && times && min_interval && time_k && time_v, WR_E_NULL, "%s: NULL argument", entry);
    WR_REQUIRE(B >= 1 && B <= (int64_t(1) << 24), WR_E_SHAPE, "%s: B=%lld out of range (1..2^24)", entry, (long long)B);
    WR_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(time_k) && aligned16(time_v), WR_E_ALIGN,
               "%s: q, k, v and the tables must be 16-byte aligned", entry);
    return WR_OK;
}

#define WR_TI_DISPATCH(D, CALL)          \
    do {                                 \
        if ((D) == 64) { CALL(64); }     \
        else { CALL(32); }               \
    } while (0)

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_ti_attention_supported(int32_t D, int32_t n_heads, int32_t T, int32_t time_max) {
    return ti_supported(D, n_heads, T, time_max) ? 1 : 0;
}

int64_t wr_ti_attention_workspace_bytes(int64_t B, int32_t T, int32_t D, int32_t n_heads, int32_t time_max) {
    WR_REQUIRE(ti_supported(D, n_heads, T, time_max) && B >= 1 && B <= (int64_t(1) << 24), WR_E_RANGE,
               "wr_ti_attention_workspace_bytes supports D in {32, 64}, n_heads in {1, 2, 4} with D / n_heads >= 8, 1 <= T <= %d, "
               "1 <= time_max <= %d, 1 <= B <= 2^24; got B=%lld D=%d n_heads=%d T=%d time_max=%d", kTiMaxT, kTiMaxTimeMax,
               (long long)B, D, n_heads, T, time_max);
    return align_up((int64_t)kTiBwdWg * 2 * (time_max + 1) * D * 4, 256);   // sized by the bound, not by min(B, bound)
}

int32_t wr_ti_attention_fwd(const float *q, const float *k, const float *v, const int64_t *times, const int64_t *min_interval,
                            int64_t B, int32_t T, int32_t D, int32_t n_heads, const float *time_k, const float *time_v,
                            int32_t time_max, float *out, int32_t *err_word, void *stream_) {
    const char *entry = "wr_ti_attention_fwd";
    const int32_t rc = ti_check(entry, q, k, v, times, min_interval, B, T, D, n_heads, time_k, time_v, time_max);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(out != nullptr, WR_E_NULL, "%s: NULL argument", entry);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const TiParams P{q, k, v, time_k, time_v, times, min_interval, B, T, n_heads, time_max, 1.0f / sqrtf((float)(D / n_heads))};
    const size_t lds = (size_t)ti_lds_words(D, T, n_heads, false) * 4;
    const unsigned grid = (unsigned)(B < kTiFwdWg ? B : kTiFwdWg);
#define WR_TI_FWD(D_)                                                                                                          \
    do {                                                                                                                       \
        if (lds > 64 * 1024)                                                                                                   \
            WR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ti_fwd_kernel<D_>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                       (int)lds));                                                                             \
        hipLaunchKernelGGL(ti_fwd_kernel<D_>, dim3(grid), dim3(kBlock), lds, stream, P, out, err_word);                        \
    } while (0)
    WR_TI_DISPATCH(D, WR_TI_FWD);
#undef WR_TI_FWD
    WR_LAUNCH_CHECK("ti_fwd_kernel");
    return WR_OK;
}

int32_t wr_ti_attention_bwd(const float *q, const float *k, const float *v, const int64_t *times, const int64_t *min_interval,
                            int64_t B, int32_t T, int32_t D, int32_t n_heads, const float *time_k, const float *time_v,
                            int32_t time_max, const float *g_out, float *gq, float *gk, float *gv, float *g_time_k,
                            float *g_time_v, int32_t *err_word, void *workspace, int64_t workspace_bytes, void *stream_) {
    const char *entry = "wr_ti_attention_bwd";
    int32_t rc = ti_check(entry, q, k, v, times, min_interval, B, T, D, n_heads, time_k, time_v, time_max);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(g_out && gq && gk && gv && g_time_k && g_time_v, WR_E_NULL, "%s: NULL argument", entry);
    WR_REQUIRE(aligned16(g_out), WR_E_ALIGN, "%s: g_out must be 16-byte aligned", entry);
    if ((rc = check_workspace(entry, workspace, workspace_bytes, wr_ti_attention_workspace_bytes(B, T, D, n_heads, time_max))) != WR_OK)
        return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const TiParams P{q, k, v, time_k, time_v, times, min_interval, B, T, n_heads, time_max, 1.0f / sqrtf((float)(D / n_heads))};
    const size_t lds = (size_t)ti_lds_words(D, T, n_heads, true) * 4;
    float *slabs = reinterpret_cast<float *>(workspace);
    const int n_wg = (int)(B < kTiBwdWg ? B : kTiBwdWg);
#define WR_TI_BWD(D_)                                                                                                          \
    do {                                                                                                                       \
        if (lds > 64 * 1024)                                                                                                   \
            WR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ti_bwd_kernel<D_>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                       (int)lds));                                                                             \
        hipLaunchKernelGGL(ti_bwd_kernel<D_>, dim3(n_wg), dim3(kBlock), lds, stream, P, g_out, gq, gk, gv, slabs, err_word);   \
    } while (0)
    WR_TI_DISPATCH(D, WR_TI_BWD);
#undef WR_TI_BWD
    WR_LAUNCH_CHECK("ti_bwd_kernel");
    const int n_tab = (time_max + 1) * D;
    hipLaunchKernelGGL(ti_fold_kernel, dim3((2 * n_tab + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, slabs, n_wg, n_tab, g_time_k,
                       g_time_v);
    WR_LAUNCH_CHECK("ti_fold_kernel");
    return WR_OK;
}

}  // extern "C"
