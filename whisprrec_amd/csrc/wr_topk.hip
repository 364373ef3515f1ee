// wr_topk.hip — top-K recommendation on the matrix cores without the [n, n_items] score matrix.
//
// The reference's (commented-out) save_rec_results (src/main.py:83-102) sorts each row of full_predict with the user's
// clicked items at -inf and keeps the first K.  Here the scores come from the same v_mfma_f32_32x32x2_f32 tiles as
// wr_rank_eval (wr_eval.hip): an exact k-ordered fp32 chain, so a returned score is bitwise equal to wr_rank_eval's
// target_score for that pair.  Each score is packed into one 64-bit key
//     key = (orderable(score) << 32) | (0xFFFFFFFF - item),
// so a single unsigned compare orders by score descending, then item ascending; key 0 is the padding (-1, -inf).
//
// Phase 1 (topk_scan_kernel*): a workgroup = 4 waves = 128 query rows x one item chunk.  Every row keeps the key of its
// current K-th best in LDS.  A tile score that does not beat it (after the first few tiles, nearly all of them) costs one
// compare.  The rest go to the row's staging area in the workspace, at positions given by a ballot (deterministic).  When a
// row's staging could overflow on the next tile, its wave sorts list + staging (bitonic, in registers across the 64 lanes),
// keeps the K best as the row's list and raises the threshold.  Items are visited in ascending order inside a chunk, so an
// item whose score only ties the threshold has the larger id and loses: the fast test is a strict compare of the score part.
// Phase 2 (topk_merge_kernel): one wave per row folds the chunk lists together with the same sort and decodes.
#include "wr_common.h"

namespace wr {

typedef float tk_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int kTopkRows = 128;              // query rows per workgroup (32 per wave)
constexpr int kTopkTile = 64;               // items per tile, register-operand kernel (double-buffered)
constexpr int kTopkTileG = 32;              // items per tile, LDS-operand kernel
constexpr int kTopkSlots = 256 * 2;         // 256 CUs x 2 resident workgroups of the register-operand kernel (<= 256 VGPRs)
constexpr int64_t kTopkMinChunk = 4096;     // items per chunk at least (fewer, longer chunks: fewer candidates and lists)
constexpr int64_t kTopkMaxChunks = 64;
constexpr int64_t kTopkWgCap = 8 * kTopkSlots;   // workgroups of one call at most when chunking (bounds the workspace)

// keys per (row, chunk) region: the row's list (k keys) followed by its staging area
static inline int topk_region(int k) { return k <= 128 ? 256 : 512; }

__device__ __forceinline__ uint32_t ord_of(float s) {
    const uint32_t u = __float_as_uint(s);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float score_of(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o); }
__device__ __forceinline__ u64 key_of(float s, int64_t item) {
    return ((u64)ord_of(s) << 32) | (u64)(0xFFFFFFFFu - (uint32_t)item);
}

__device__ __forceinline__ u64 shfl_xor64(u64 v, int m) {
    const int lo = __shfl_xor((int)(uint32_t)v, m, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((u64)(uint32_t)hi << 32) | (uint32_t)lo;
}

// Bitonic sort, descending, of the 64*E keys of a wave: key i = lane*E + e lives in v[e] of `lane`.
template <int E>
__device__ __forceinline__ void sort_desc(u64 (&v)[E], int lane) {
    constexpr int N = 64 * E;
#pragma unroll
    for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= E) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int i = lane * E + e;
                    const u64 p = shfl_xor64(v[e], j / E);
                    const bool want_max = ((i & j) == 0) == ((i & k) == 0);
                    v[e] = want_max ? (v[e] > p ? v[e] : p) : (v[e] < p ? v[e] : p);
                }
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if ((e & j) == 0) {
                        const int f = e | j;
                        const bool up = ((lane * E + e) & k) == 0;
                        const u64 a = v[e], b = v[f];
                        const u64 hi = a > b ? a : b, lo = a > b ? b : a;
                        v[e] = up ? hi : lo;
                        v[f] = up ? lo : hi;
                    }
                }
            }
        }
    }
}

// The whole wave: sort list (buf[0, k)) + staging (buf[k, k + cnt)), keep the k best as the new list, return the score part
// of the k-th key (the row's new threshold).
template <int E>
__device__ __forceinline__ uint32_t merge_row(u64 *buf, int k, int cnt, int lane) {
    u64 v[E];
    const int lim = k + cnt;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        v[e] = i < lim ? buf[i] : 0ull;
    }
    sort_desc<E>(v, lane);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        if (i < k) buf[i] = v[e];
    }
    const int t = k - 1;
    uint32_t h = 0;
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (e == t % E) h = (uint32_t)(v[e] >> 32);
    return (uint32_t)__shfl((int)h, t / E, 64);
}

// LDS and workspace written by one lane are read by the other lanes of the same wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Per-wave state of phase 1: the wave's 32 rows are wave*32 .. wave*32+31 of the workgroup; their regions start at
// `base` (row r at base + r * stride).
struct TopkRows {
    u64 *base;
    int64_t stride;
    unsigned *thr;   // [32] LDS: score part of the row's k-th key (0xFFFFFFFF: row past the end, never takes a candidate)
    int *cnt;        // [32] LDS: keys in the row's staging area
    int k, trigger, lane;
};

template <int E>
__device__ __forceinline__ void topk_init_rows(const TopkRows &w, int64_t e_first, int64_t n) {
    for (int r = 0; r < 32; ++r) {
        if (e_first + r >= n) break;
        u64 *b = w.base + r * w.stride;
        for (int j = w.lane; j < w.k; j += 64) b[j] = 0ull;
    }
}

// merge every row whose staging holds more than `above` keys
template <int E>
__device__ __forceinline__ void topk_merge_rows(const TopkRows &w, int above) {
    for (int r = 0; r < 32; ++r) {
        const int c = w.cnt[r];
        if (c > above) {
            const uint32_t t = merge_row<E>(w.base + r * w.stride, w.k, c, w.lane);
            if (w.lane == 0) {
                w.thr[r] = t;
                w.cnt[r] = 0;
            }
            wave_sync();
        }
    }
}

// One tile's C column blocks of 32 x 32 scores (this lane: rows (reg&3) + 8*(reg>>2) + 4*half, column j0 + 32c + col).
// masked(c, row) and the table end only matter when `plain` is false.
template <int C, int E, typename Masked>
__device__ __forceinline__ void topk_absorb(const TopkRows &w, const tk_f32x16 (&acc)[C], int64_t j0, bool plain,
                                            int64_t n_items, Masked masked) {
    const int col = w.lane & 31, half = w.lane >> 5;
    uint32_t th[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const uint4 t4 = *reinterpret_cast<const uint4 *>(&w.thr[8 * g + 4 * half]);
        th[4 * g] = t4.x; th[4 * g + 1] = t4.y; th[4 * g + 2] = t4.z; th[4 * g + 3] = t4.w;
    }
    auto cand = [&](int c, int reg) -> bool {
        bool ok = ord_of(acc[c][reg]) > th[reg];
        if (!plain) {
            const int row = (reg & 3) + 8 * (reg >> 2) + 4 * half;
            ok = ok && j0 + c * 32 + col < n_items && !masked(c, row);
        }
        return ok;
    };
    bool any = false;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
#pragma unroll
        for (int c = 0; c < C; ++c) any |= cand(c, reg);
    }
    if (__ballot(any) == 0ull) return;     // wave-uniform: the common case after the first tiles
    bool full = false;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * half;
        int cnt = w.cnt[row];
        u64 *dst = w.base + row * w.stride + w.k;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const bool p = cand(c, reg);
            const u64 b = __ballot(p);
            const uint32_t mine = half ? (uint32_t)(b >> 32) : (uint32_t)b;
            if (p) dst[cnt + __popc(mine & ((1u << col) - 1u))] = key_of(acc[c][reg], j0 + c * 32 + col);
            cnt += __popc(mine);
        }
        full |= cnt > w.trigger;
        if (col == 0) w.cnt[row] = cnt;               // a wave's LDS accesses complete in order: no fence for the counts
    }
    // The fence waits for every outstanding load, the next tile's prefetch included: only before a merge (rare), which
    // reads the keys the lanes just stored
    if (__ballot(full) != 0ull) {
        wave_sync();
        topk_merge_rows<E>(w, w.trigger);
    }
}

// Register-operand kernel, D = 2*KS in {8, 16, 32, 64}: the structure of eval_rank_kernel_rega (A in registers, item tiles
// of 64 double-buffered in LDS, per-row mask bitmaps with a per-slab `anymask` skip).
// 2 workgroups per CU: at 3 (<= 168 VGPRs) the staging and merge path spills to scratch.
template <int KS, int E>
__global__ __launch_bounds__(kBlock, 2) void topk_scan_kernel_rega(const float *__restrict__ U, const float *__restrict__ I,
                                                                 int64_t n_items, const int64_t *__restrict__ qu, int64_t n,
                                                                 const int64_t *__restrict__ mask_ptr,
                                                                 const int *__restrict__ mask_idx, int k, int64_t chunk,
                                                                 int nc, u64 *ws) {
    constexpr int D = 2 * KS, LDW = D + 1, D4 = D / 4, M = 64 * E;
    constexpr int NLOAD = (kTopkTile * D4 + kBlock - 1) / kBlock;
    __shared__ float it[2][kTopkTile * LDW];
    __shared__ unsigned rowmask[2][kTopkTile / 32][kTopkRows];
    __shared__ unsigned anymask[2][kBlock / 64];
    __shared__ __attribute__((aligned(16))) unsigned thr_s[kTopkRows];
    __shared__ int cnt_s[kTopkRows];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = lane & 31, half = lane >> 5;
    const int64_t e0 = (int64_t)blockIdx.x * kTopkRows;
    const int64_t c0 = (int64_t)blockIdx.y * chunk;
    const int64_t c1 = (c0 + chunk < n_items) ? c0 + chunk : n_items;
    TopkRows w;
    w.stride = (int64_t)nc * M;
    w.base = ws + ((e0 + wave * 32) * nc + blockIdx.y) * (int64_t)M;
    w.thr = thr_s + wave * 32;
    w.cnt = cnt_s + wave * 32;
    w.k = k;
    w.trigger = M - k - kTopkTile;
    w.lane = lane;
    if (threadIdx.x < kTopkRows) {
        thr_s[threadIdx.x] = (e0 + threadIdx.x < n) ? 0u : 0xFFFFFFFFu;
        cnt_s[threadIdx.x] = 0;
    }
    topk_init_rows<E>(w, e0 + wave * 32, n);
    float a[KS];
    {
        const int64_t e = e0 + wave * 32 + col;
        const float *urow = U + ((e < n) ? qu[e] : 0) * (int64_t)D + half;
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = (e < n) ? urow[2 * s] : 0.f;
    }
    int64_t cur = 0, cend = 0;
    if (threadIdx.x < kTopkRows && mask_ptr != nullptr && e0 + threadIdx.x < n) {
        const int64_t uu = qu[e0 + threadIdx.x];
        int64_t lo = mask_ptr[uu], hi = mask_ptr[uu + 1];
        cend = hi;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)mask_idx[mid] < c0) lo = mid + 1; else hi = mid;
        }
        cur = lo;
    }
    int nxt = (cur < cend) ? mask_idx[cur] : 0x7fffffff;
    float4 stage[NLOAD];
    auto fetch = [&](int64_t j0) {
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
            const int f = threadIdx.x + i * kBlock;
            const int r = f / D4, k4 = f - r * D4;
            stage[i] = (f < kTopkTile * D4 && j0 + r < n_items)
                           ? reinterpret_cast<const float4 *>(I + (j0 + r) * (int64_t)D)[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto deposit = [&](int buf, int64_t j0) {
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
            const int f = threadIdx.x + i * kBlock;
            if (f < kTopkTile * D4) {
                const int r = f / D4, k4 = f - r * D4;
                float *dst = &it[buf][r * LDW + 4 * k4];
                dst[0] = stage[i].x; dst[1] = stage[i].y; dst[2] = stage[i].z; dst[3] = stage[i].w;
            }
        }
        if (threadIdx.x < kTopkRows) {
            unsigned m[kTopkTile / 32];
#pragma unroll
            for (int c = 0; c < kTopkTile / 32; ++c) m[c] = 0;
            while ((int64_t)nxt < j0 + kTopkTile) {
                const int64_t d = (int64_t)nxt - j0;
                if (d >= 0) m[d >> 5] |= 1u << (unsigned)(d & 31);
                ++cur;
                nxt = (cur < cend) ? mask_idx[cur] : 0x7fffffff;
            }
            unsigned any = 0;
#pragma unroll
            for (int c = 0; c < kTopkTile / 32; ++c) {
                rowmask[buf][c][threadIdx.x] = m[c];
                any |= m[c];
            }
            const unsigned long long bal = __ballot(any != 0);
            if (lane == 0) {
                anymask[buf][2 * wave] = (unsigned)(bal & 0xffffffffull) != 0;
                anymask[buf][2 * wave + 1] = (unsigned)(bal >> 32) != 0;
            }
        }
    };
    fetch(c0);
    deposit(0, c0);
    __syncthreads();
    int buf = 0;
    for (int64_t j0 = c0; j0 < c1; j0 += kTopkTile, buf ^= 1) {
        const bool more = j0 + kTopkTile < c1;
        if (more) fetch(j0 + kTopkTile);
        {
            constexpr int C = kTopkTile / 32;
            const float *bcol = &it[buf][col * LDW + half];
            tk_f32x16 acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = tk_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
#pragma unroll
                for (int c = 0; c < C; ++c)
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bcol[c * 32 * LDW + 2 * s], acc[c], 0, 0, 0);
            }
            const bool plain = anymask[buf][wave] == 0 && j0 + kTopkTile <= n_items;
            const int b = buf;
            topk_absorb<C, E>(w, acc, j0, plain, n_items,
                              [&](int c, int row) { return ((rowmask[b][c][wave * 32 + row] >> col) & 1u) != 0; });
        }
        if (more) deposit(buf ^ 1, j0 + kTopkTile);
        __syncthreads();
    }
    wave_sync();
    topk_merge_rows<E>(w, 0);
}

// LDS-operand kernel for any other D (multiple of 4, <= 252): the structure of eval_rank_kernel (query rows and one
// 32-item tile staged in LDS with padded rows).
template <int E>
__global__ __launch_bounds__(kBlock) void topk_scan_kernel(const float *__restrict__ U, const float *__restrict__ I, int D,
                                                           int64_t n_items, const int64_t *__restrict__ qu, int64_t n,
                                                           const int64_t *__restrict__ mask_ptr,
                                                           const int *__restrict__ mask_idx, int k, int64_t chunk, int nc,
                                                           u64 *ws) {
    constexpr int M = 64 * E;
    extern __shared__ float lds[];
    const int ldw = D + 1;
    float *ue = lds;                                                    // [kTopkRows][ldw]
    float *it = lds + kTopkRows * ldw;                                  // [32][ldw]
    unsigned *rowmask = reinterpret_cast<unsigned *>(it + kTopkTileG * ldw);   // [kTopkRows]
    unsigned *thr_s = rowmask + kTopkRows;                              // [kTopkRows], 16-byte aligned: (160 ldw + 128) * 4
    int *cnt_s = reinterpret_cast<int *>(thr_s + kTopkRows);            // [kTopkRows]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = lane & 31, half = lane >> 5;
    const int64_t e0 = (int64_t)blockIdx.x * kTopkRows;
    const int64_t c0 = (int64_t)blockIdx.y * chunk;
    const int64_t c1 = (c0 + chunk < n_items) ? c0 + chunk : n_items;
    TopkRows w;
    w.stride = (int64_t)nc * M;
    w.base = ws + ((e0 + wave * 32) * nc + blockIdx.y) * (int64_t)M;
    w.thr = thr_s + wave * 32;
    w.cnt = cnt_s + wave * 32;
    w.k = k;
    w.trigger = M - k - kTopkTileG;
    w.lane = lane;
    if (threadIdx.x < kTopkRows) {
        thr_s[threadIdx.x] = (e0 + threadIdx.x < n) ? 0u : 0xFFFFFFFFu;
        cnt_s[threadIdx.x] = 0;
    }
    topk_init_rows<E>(w, e0 + wave * 32, n);
    for (int idx = threadIdx.x; idx < kTopkRows * D; idx += kBlock) {
        const int r = idx / D, kk = idx - r * D;
        const int64_t e = e0 + r;
        ue[r * ldw + kk] = (e < n) ? U[qu[e] * (int64_t)D + kk] : 0.f;
    }
    int64_t cur = 0, cend = 0;
    if (threadIdx.x < kTopkRows && mask_ptr != nullptr && e0 + threadIdx.x < n) {
        const int64_t uu = qu[e0 + threadIdx.x];
        int64_t lo = mask_ptr[uu], hi = mask_ptr[uu + 1];
        cend = hi;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)mask_idx[mid] < c0) lo = mid + 1; else hi = mid;
        }
        cur = lo;
    }
    const float *arow = ue + (wave * 32 + col) * ldw + half;
    const float *brow = it + col * ldw + half;
    for (int64_t j0 = c0; j0 < c1; j0 += kTopkTileG) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < kTopkTileG * D; idx += kBlock) {
            const int r = idx / D, kk = idx - r * D;
            it[r * ldw + kk] = (j0 + r < n_items) ? I[(j0 + r) * (int64_t)D + kk] : 0.f;
        }
        if (threadIdx.x < kTopkRows) {
            unsigned m = 0;
            while (cur < cend && (int64_t)mask_idx[cur] < j0 + kTopkTileG) {
                if ((int64_t)mask_idx[cur] >= j0) m |= 1u << (unsigned)(mask_idx[cur] - j0);
                ++cur;
            }
            rowmask[threadIdx.x] = m;
        }
        __syncthreads();
        tk_f32x16 acc[1];
        acc[0] = tk_f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int k0 = 0; k0 < D; k0 += 2) acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[k0], brow[k0], acc[0], 0, 0, 0);
        topk_absorb<1, E>(w, acc, j0, false, n_items,
                          [&](int, int row) { return ((rowmask[wave * 32 + row] >> col) & 1u) != 0; });
    }
    wave_sync();
    topk_merge_rows<E>(w, 0);
}

// Phase 2: one wave per row folds the row's nc chunk lists (k sorted keys each) into one and decodes it.  The lower half of
// the 64*E keys carries the running best, the upper half takes the next list; 64*E/2 >= k.
template <int E>
__global__ __launch_bounds__(kBlock) void topk_merge_kernel(const u64 *__restrict__ ws, int64_t n, int nc, int k,
                                                            int *__restrict__ out_item, float *__restrict__ out_score) {
    constexpr int M = 64 * E, H = M / 2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    if (q >= n) return;
    const u64 *base = ws + q * nc * (int64_t)M;
    u64 v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        v[e] = i < k ? base[i] : 0ull;
    }
    for (int c = 1; c < nc; ++c) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = lane * E + e;
            if (i >= H) v[e] = (i - H < k) ? base[(int64_t)c * M + (i - H)] : 0ull;
        }
        sort_desc<E>(v, lane);
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        if (i < k) {
            const u64 key = v[e];
            out_item[q * k + i] = (int)(0xFFFFFFFFu - (uint32_t)key);
            out_score[q * k + i] = key == 0ull ? -__builtin_inff() : score_of((uint32_t)(key >> 32));
        }
    }
}

static inline bool topk_rega_d(int32_t D) { return D == 64 || D == 32 || D == 16 || D == 8; }

// LDS-operand kernel: (128 + 32) rows of D + 1 floats, 128 mask words, 128 thresholds, 128 counts
static inline size_t topk_lds_generic(int32_t D) { return ((size_t)(kTopkRows + kTopkTileG) * (D + 1) + 3 * kTopkRows) * 4; }

// Chunks per call: enough workgroups to fill the chip in whole rounds (a workgroup runs for the length of its chunk, so a
// grid of 1.02 rounds takes 2), fewer when that does not pay 2 % (every chunk adds candidates and a list to merge).
static inline int64_t topk_max_chunks(int64_t n_items) {
    int64_t m = n_items / kTopkMinChunk;
    return m < 1 ? 1 : (m > kTopkMaxChunks ? kTopkMaxChunks : m);
}

static inline int64_t topk_chunks(int64_t n, int64_t n_items) {
    const int64_t rb = (n + kTopkRows - 1) / kTopkRows;
    int64_t cap = topk_max_chunks(n_items);
    const int64_t wg_cap = rb > kTopkWgCap ? 1 : kTopkWgCap / rb;
    if (cap > wg_cap) cap = wg_cap;
    if (cap < 1) cap = 1;
    int64_t best = 1;
    double best_cost = 1e300;
    for (int64_t nc = 1; nc <= cap; ++nc) {
        const double cost = (double)((rb * nc + kTopkSlots - 1) / kTopkSlots) / (double)nc;
        if (cost < best_cost * 0.98) {
            best_cost = cost;
            best = nc;
        }
    }
    return best;
}

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_topk_supported(int32_t D, int32_t k) {
    if (k < 1 || k > 256 || D < 4 || D % 4 != 0) return 0;
    return (topk_rega_d(D) || topk_lds_generic(D) <= 160 * 1024) ? 1 : 0;
}

int64_t wr_topk_workspace_bytes(int64_t n, int64_t n_items, int32_t D, int32_t k) {
    (void)D;
    if (n < 0 || n_items < 0 || k < 1 || k > 256) {
        set_error("topk_workspace_bytes: n=%lld n_items=%lld k=%d out of range", (long long)n, (long long)n_items, k);
        return WR_E_SHAPE;
    }
    // an upper bound of what topk_chunks picks that never decreases in n, n_items or k:
    // rb * nc <= min(rb * max_chunks(n_items), max(rb, kTopkWgCap)) regions of 128 rows
    const int64_t rb = (n + kTopkRows - 1) / kTopkRows;
    const int64_t a = rb * topk_max_chunks(n_items), b = rb > kTopkWgCap ? rb : kTopkWgCap;
    const int64_t regions = (a < b ? a : b) * kTopkRows;
    return regions * topk_region(k) * 8 + 256;
}

int32_t wr_topk_recommend(const float *user_mat, int64_t n_user_rows, const float *item_tab, int64_t n_items, int32_t D,
                          const int64_t *query_user, int64_t n, const int64_t *mask_ptr, const int32_t *mask_idx,
                          int32_t k, int32_t *out_item, float *out_score, void *workspace, int64_t workspace_bytes,
                          void *stream_) {
    int32_t rc;
    if ((rc = check_table(user_mat, n_user_rows, D, "user_mat")) != WR_OK) return rc;
    if ((rc = check_table(item_tab, n_items, D, "item_tab")) != WR_OK) return rc;
    WR_REQUIRE(query_user && out_item && out_score, WR_E_NULL, "topk_recommend: NULL argument");
    WR_REQUIRE((mask_ptr == nullptr) == (mask_idx == nullptr), WR_E_NULL, "topk_recommend: mask_ptr and mask_idx go together");
    WR_REQUIRE(n >= 0 && n < (int64_t(1) << 31), WR_E_SHAPE, "topk_recommend: n out of range");
    WR_REQUIRE(k >= 1 && k <= 256, WR_E_RANGE, "topk_recommend: k=%d must be in [1, 256]", k);
    WR_REQUIRE(wr_topk_supported(D, k), WR_E_RANGE,
               "topk_recommend supports D in {8,16,32,64} or a multiple of 4 up to 252 (LDS staging: %lld B needed, "
               "163840 B per workgroup); got D=%d", (long long)topk_lds_generic(D), D);
    const int64_t need = wr_topk_workspace_bytes(n, n_items, D, k);
    WR_REQUIRE(workspace != nullptr && workspace_bytes >= need, WR_E_WORKSPACE,
               "topk_recommend: workspace of %lld B, %lld B needed", (long long)workspace_bytes, (long long)need);
    WR_REQUIRE(aligned16(workspace), WR_E_ALIGN, "topk_recommend: workspace is not 16-byte aligned");
    if (n == 0) return WR_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    u64 *ws = reinterpret_cast<u64 *>(workspace);
    const int64_t tiles = (n_items + kTopkTile - 1) / kTopkTile;
    int64_t nc = topk_chunks(n, n_items);
    const int64_t chunk = (tiles + nc - 1) / nc * kTopkTile;     // whole tiles of both kernels
    nc = (n_items + chunk - 1) / chunk;
    const dim3 grid((unsigned)((n + kTopkRows - 1) / kTopkRows), (unsigned)nc);
    const bool big = k > 128;
    const int nci = (int)nc;
    if (topk_rega_d(D)) {
#define WR_TOPK_REGA(KS_, E_)                                                                                            \
    hipLaunchKernelGGL((topk_scan_kernel_rega<KS_, E_>), grid, dim3(kBlock), 0, stream, user_mat, item_tab, n_items, \
                       query_user, n, mask_ptr, mask_idx, k, chunk, nci, ws)
        if (D == 64) { if (big) WR_TOPK_REGA(32, 8); else WR_TOPK_REGA(32, 4); }
        else if (D == 32) { if (big) WR_TOPK_REGA(16, 8); else WR_TOPK_REGA(16, 4); }
        else if (D == 16) { if (big) WR_TOPK_REGA(8, 8); else WR_TOPK_REGA(8, 4); }
        else { if (big) WR_TOPK_REGA(4, 8); else WR_TOPK_REGA(4, 4); }
#undef WR_TOPK_REGA
    } else {
        const size_t lds = topk_lds_generic(D);
        const void *fn = big ? reinterpret_cast<const void *>(topk_scan_kernel<8>) : reinterpret_cast<const void *>(topk_scan_kernel<4>);
        if (lds > 64 * 1024) WR_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (big)
            hipLaunchKernelGGL(topk_scan_kernel<8>, grid, dim3(kBlock), lds, stream, user_mat, item_tab, D, n_items, query_user,
                               n, mask_ptr, mask_idx, k, chunk, nci, ws);
        else
            hipLaunchKernelGGL(topk_scan_kernel<4>, grid, dim3(kBlock), lds, stream, user_mat, item_tab, D, n_items, query_user,
                               n, mask_ptr, mask_idx, k, chunk, nci, ws);
    }
    WR_LAUNCH_CHECK("topk_scan_kernel");
    const dim3 mgrid((unsigned)((n + kBlock / 64 - 1) / (kBlock / 64)));
    if (big)
        hipLaunchKernelGGL(topk_merge_kernel<8>, mgrid, dim3(kBlock), 0, stream, ws, n, nci, k, out_item, out_score);
    else
        hipLaunchKernelGGL(topk_merge_kernel<4>, mgrid, dim3(kBlock), 0, stream, ws, n, nci, k, out_item, out_score);
    WR_LAUNCH_CHECK("topk_merge_kernel");
    return WR_OK;
}

}  // extern "C"
