// wr_topk.hip — top-K recommendation on the matrix cores without the [n, n_items] score matrix.
//
// The reference's (commented-out) save_rec_results (src/main.py:83-102) sorts each row of full_predict with the user's
// clicked items at -inf and keeps the first K.  Here the scores come from the same v_mfma_f32_32x32x2_f32 tiles as
// wr_rank_eval (the scan of wr_score_tiles.h): an exact k-ordered fp32 chain, so a returned score is bitwise equal to
// wr_rank_eval's target_score for that pair.  Each score is packed into one 64-bit key
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
//
// KQ query vectors per row (K23, multi-interest models: score = max over the row's KQ interests): the scans run over the
// n KQ query rows, and acc_row puts the KQ in {1, 2, 4} query rows of one EVALUATION row into KQ adjacent accumulator
// registers of one lane (the layout argument of K19, wr_eval.hip).  The consumer takes their maximum, so a lane holds 16/KQ
// evaluation rows, a wave 32/KQ, a workgroup 128/KQ, and everything per-row below (threshold, staging count, ballot position,
// workspace region, merge trigger) is per evaluation row.  One item yields at most one candidate per evaluation row, so the
// trigger arithmetic and the tie argument hold as they are.  KQ = 1 is the single-query kernel.
#include "wr_score_tiles.h"

namespace wr {

typedef unsigned long long u64;

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

// Per-wave state of phase 1: the wave's 32/KQ evaluation rows are wave*32/KQ .. of the workgroup's 128/KQ; their regions
// start at `base` (row r at base + r * stride).
struct TopkRows {
    u64 *base;
    int64_t stride;
    unsigned *thr;   // [32/KQ] LDS: score part of the row's k-th key (0xFFFFFFFF: row past the end, never takes a candidate)
    int *cnt;        // [32/KQ] LDS: keys in the row's staging area
    int k, trigger, lane;
};

// The scan kernels' prologue: the wave's view of the workgroup's thresholds and counts (thr_s, cnt_s: [kScoreRows] LDS, set
// here, visible after the scan's first barrier) and of its regions of M keys in the workspace, lists emptied.  A merge is
// due when a row's staging could overflow on the next tile of `tile` items.  n: evaluation rows (the scan sees n KQ).
template <int E, int KQ>
__device__ __forceinline__ TopkRows topk_rows(u64 *ws, int nc, int k, int tile, int64_t n, unsigned *thr_s, int *cnt_s) {
    constexpr int M = 64 * E, RW = 32 / KQ, RG = kScoreRows / KQ;     // evaluation rows per wave and per workgroup
    const int wave = threadIdx.x >> 6;
    const int64_t e0 = (int64_t)blockIdx.x * RG;
    TopkRows w;
    w.stride = (int64_t)nc * M;
    w.base = ws + ((e0 + wave * RW) * nc + blockIdx.y) * (int64_t)M;
    w.thr = thr_s + wave * RW;
    w.cnt = cnt_s + wave * RW;
    w.k = k;
    w.trigger = M - k - tile;
    w.lane = threadIdx.x & 63;
    if (threadIdx.x < RG) {
        thr_s[threadIdx.x] = (e0 + threadIdx.x < n) ? 0u : 0xFFFFFFFFu;
        cnt_s[threadIdx.x] = 0;
    }
    for (int r = 0; r < RW; ++r) {
        if (e0 + wave * RW + r >= n) break;
        u64 *b = w.base + r * w.stride;
        for (int j = w.lane; j < w.k; j += 64) b[j] = 0ull;
    }
    return w;
}

// merge every row whose staging holds more than `above` keys
template <int E, int KQ>
__device__ __forceinline__ void topk_merge_rows(const TopkRows &w, int above) {
    for (int r = 0; r < 32 / KQ; ++r) {
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

// The score scan's consumer.  One tile's C column blocks of 32 x 32 scores (this lane: query rows acc_row(reg, half), column
// j0 + 32c + col).  Group g of a lane = registers g KQ .. g KQ + KQ - 1 = the KQ interests of evaluation row
// acc_row(g KQ, half) / KQ of the wave; its score is their maximum.  masked(c, row) and the table end only matter when `plain`
// is false; the KQ query rows of a group share one mask list, the first one's is tested.
template <int E, int KQ, int C, typename Masked>
__device__ __forceinline__ void topk_absorb(const TopkRows &w, const f32x16 (&acc)[C], int64_t j0, bool plain,
                                            int64_t n_items, Masked masked) {
    constexpr int NG = 16 / KQ;
    const int col = w.lane & 31, half = w.lane >> 5;
    uint32_t th[NG];
    if constexpr (KQ == 1) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint4 t4 = *reinterpret_cast<const uint4 *>(&w.thr[8 * g + 4 * half]);
            th[4 * g] = t4.x; th[4 * g + 1] = t4.y; th[4 * g + 2] = t4.z; th[4 * g + 3] = t4.w;
        }
    } else {
#pragma unroll
        for (int g = 0; g < NG; ++g) th[g] = w.thr[acc_row(g * KQ, half) / KQ];
    }
    auto best = [&](int c, int g) -> float {
        float m = acc[c][g * KQ];
#pragma unroll
        for (int q = 1; q < KQ; ++q) m = fmaxf(m, acc[c][g * KQ + q]);
        return m;
    };
    auto cand = [&](int c, int g) -> bool {
        bool ok = ord_of(best(c, g)) > th[g];
        if (!plain) {
            const int row = acc_row(g * KQ, half);
            ok = ok && j0 + c * 32 + col < n_items && !masked(c, row);
        }
        return ok;
    };
    bool any = false;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
        for (int c = 0; c < C; ++c) any |= cand(c, g);
    }
    if (__ballot(any) == 0ull) return;     // wave-uniform: the common case after the first tiles
    bool full = false;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int row = acc_row(g * KQ, half) / KQ;   // the two halves hold different rows: each takes its own ballot half
        int cnt = w.cnt[row];
        u64 *dst = w.base + row * w.stride + w.k;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const bool p = cand(c, g);
            const u64 b = __ballot(p);
            const uint32_t mine = half ? (uint32_t)(b >> 32) : (uint32_t)b;
            if (p) dst[cnt + __popc(mine & ((1u << col) - 1u))] = key_of(best(c, g), j0 + c * 32 + col);
            cnt += __popc(mine);
        }
        full |= cnt > w.trigger;
        if (col == 0) w.cnt[row] = cnt;               // a wave's LDS accesses complete in order: no fence for the counts
    }
    // The fence waits for every outstanding load, the next tile's prefetch included: only before a merge (rare), which
    // reads the keys the lanes just stored
    if (__ballot(full) != 0ull) {
        wave_sync();
        topk_merge_rows<E, KQ>(w, w.trigger);
    }
}

// Register-operand kernel, D = 2*KS in {8, 16, 32, 64}.
// 2 workgroups per CU: at 3 (<= 168 VGPRs) the staging and merge path spills to scratch.
// n: evaluation rows; the scan runs over n KQ query rows (qrows is NULL when KQ > 1).
template <int KS, int E, int KQ>
__global__ __launch_bounds__(kBlock, 2) void topk_scan_kernel_rega(const float *__restrict__ U, const float *__restrict__ I,
                                                                 int64_t n_items, const int64_t *__restrict__ qrows,
                                                                 const int64_t *__restrict__ mrows, int64_t n,
                                                                 const int64_t *__restrict__ mask_ptr,
                                                                 const int *__restrict__ mask_idx, int k, int64_t chunk,
                                                                 int nc, u64 *ws) {
    __shared__ __attribute__((aligned(16))) unsigned thr_s[kScoreRows];
    __shared__ int cnt_s[kScoreRows];
    const TopkRows w = topk_rows<E, KQ>(ws, nc, k, kScoreTile, n, thr_s, cnt_s);
    score_scan_rega<KS>(U, I, n_items, qrows, mrows, n * KQ, mask_ptr, mask_idx, (int64_t)blockIdx.y * chunk, chunk,
                        [&](const auto &acc, int64_t j0, bool plain, auto masked) {
                            topk_absorb<E, KQ>(w, acc, j0, plain, n_items, masked);
                        });
    wave_sync();
    topk_merge_rows<E, KQ>(w, 0);
}

// LDS-operand kernel for any other D (multiple of 4, <= 252); thresholds and counts are the scan's side words.
template <int E, int KQ>
__global__ __launch_bounds__(kBlock) void topk_scan_kernel(const float *__restrict__ U, const float *__restrict__ I, int D,
                                                           int64_t n_items, const int64_t *__restrict__ qrows,
                                                           const int64_t *__restrict__ mrows, int64_t n,
                                                           const int64_t *__restrict__ mask_ptr,
                                                           const int *__restrict__ mask_idx, int k, int64_t chunk, int nc,
                                                           u64 *ws) {
    unsigned *thr_s = score_lds_side(D);                                // [kScoreRows]
    int *cnt_s = reinterpret_cast<int *>(thr_s + kScoreRows);           // [kScoreRows]
    const TopkRows w = topk_rows<E, KQ>(ws, nc, k, kScoreTileG, n, thr_s, cnt_s);
    score_scan_lds(U, I, D, n_items, qrows, mrows, n * KQ, mask_ptr, mask_idx, (int64_t)blockIdx.y * chunk, chunk,
                   [&](const auto &acc, int64_t j0, bool plain, auto masked) {
                       topk_absorb<E, KQ>(w, acc, j0, plain, n_items, masked);
                   });
    wave_sync();
    topk_merge_rows<E, KQ>(w, 0);
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

// LDS-operand kernel: (128 + 32) rows of D + 1 floats, 128 mask words, 128 thresholds, 128 counts
static inline size_t topk_lds_generic(int32_t D) { return score_lds_bytes(D, 3); }

// Chunks per call: enough workgroups to fill the chip in whole rounds (a workgroup runs for the length of its chunk, so a
// grid of 1.02 rounds takes 2), fewer when that does not pay 2 % (every chunk adds candidates and a list to merge).
static inline int64_t topk_max_chunks(int64_t n_items) {
    int64_t m = n_items / kTopkMinChunk;
    return m < 1 ? 1 : (m > kTopkMaxChunks ? kTopkMaxChunks : m);
}

static inline int64_t topk_chunks(int64_t n, int64_t n_items) {
    const int64_t rb = (n + kScoreRows - 1) / kScoreRows;
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

// K23's epilogue, one thread per (row, slot): the smallest q whose chain equals the returned score (the k-ordered fmaf chain
// is bitwise the MFMA's, as eval_target_multi_kernel relies on), -1 at padding.
template <int KQ>
__global__ __launch_bounds__(kBlock) void topk_interest_kernel(const float *__restrict__ Q, const float *__restrict__ I, int D,
                                                               int64_t n, int k, const int *__restrict__ out_item,
                                                               const float *__restrict__ out_score,
                                                               int *__restrict__ out_interest) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n * k) return;
    const int64_t e = t / k;
    const int item = out_item[t];
    int win = -1;
    if (item >= 0) {
        const float want = out_score[t];
        const float *b = I + (int64_t)item * D;
#pragma unroll
        for (int q = KQ - 1; q >= 0; --q) {
            const float *a = Q + (e * KQ + q) * (int64_t)D;
            float s = 0.f;
            for (int d = 0; d < D; ++d) s = fmaf(a[d], b[d], s);
            if (s == want) win = q;
        }
    }
    out_interest[t] = win;
}

// The launches behind wr_topk_recommend, wr_topk_recommend_rows (KQ = 1) and wr_topk_recommend_multi; arguments are checked by
// the entries.  n: evaluation rows; query row e KQ + q of query_mat is interest q of row e when KQ > 1 (qrows NULL).
template <int KQ>
static int32_t topk_launch(const float *query_mat, const float *item_tab, int64_t n_items, int32_t D, const int64_t *qrows,
                           const int64_t *mrows, int64_t n, const int64_t *mask_ptr, const int32_t *mask_idx, int32_t k,
                           int32_t *out_item, float *out_score, int32_t *out_interest, void *workspace, hipStream_t stream) {
    u64 *ws = reinterpret_cast<u64 *>(workspace);
    const int64_t tiles = (n_items + kScoreTile - 1) / kScoreTile;
    int64_t nc = topk_chunks(n * KQ, n_items);
    const int64_t chunk = (tiles + nc - 1) / nc * kScoreTile;     // whole tiles of both kernels
    nc = (n_items + chunk - 1) / chunk;
    const dim3 grid((unsigned)((n * KQ + kScoreRows - 1) / kScoreRows), (unsigned)nc);
    const bool big = k > 128;
    const int nci = (int)nc;
    if (score_rega_d(D)) {
#define WR_TOPK_REGA(KS_, E_)                                                                                            \
    hipLaunchKernelGGL((topk_scan_kernel_rega<KS_, E_, KQ>), grid, dim3(kBlock), 0, stream, query_mat, item_tab, n_items, qrows, \
                       mrows, n, mask_ptr, mask_idx, k, chunk, nci, ws)
#define WR_TOPK_REGA_K(KS_) do { if (big) WR_TOPK_REGA(KS_, 8); else WR_TOPK_REGA(KS_, 4); } while (0)
        WR_DISPATCH_KS(D, 4, 32, WR_TOPK_REGA_K);
#undef WR_TOPK_REGA_K
#undef WR_TOPK_REGA
    } else {
        const size_t lds = topk_lds_generic(D);
        const void *fn = big ? reinterpret_cast<const void *>(topk_scan_kernel<8, KQ>)
                             : reinterpret_cast<const void *>(topk_scan_kernel<4, KQ>);
        if (lds > 64 * 1024) WR_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (big)
            hipLaunchKernelGGL((topk_scan_kernel<8, KQ>), grid, dim3(kBlock), lds, stream, query_mat, item_tab, D, n_items, qrows,
                               mrows, n, mask_ptr, mask_idx, k, chunk, nci, ws);
        else
            hipLaunchKernelGGL((topk_scan_kernel<4, KQ>), grid, dim3(kBlock), lds, stream, query_mat, item_tab, D, n_items, qrows,
                               mrows, n, mask_ptr, mask_idx, k, chunk, nci, ws);
    }
    WR_LAUNCH_CHECK("topk_scan_kernel");
    const dim3 mgrid((unsigned)((n + kBlock / 64 - 1) / (kBlock / 64)));
    if (big)
        hipLaunchKernelGGL(topk_merge_kernel<8>, mgrid, dim3(kBlock), 0, stream, ws, n, nci, k, out_item, out_score);
    else
        hipLaunchKernelGGL(topk_merge_kernel<4>, mgrid, dim3(kBlock), 0, stream, ws, n, nci, k, out_item, out_score);
    WR_LAUNCH_CHECK("topk_merge_kernel");
    if (out_interest != nullptr) {
        hipLaunchKernelGGL(topk_interest_kernel<KQ>, dim3((unsigned)((n * k + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                           query_mat, item_tab, D, n, k, out_item, out_score, out_interest);
        WR_LAUNCH_CHECK("topk_interest_kernel");
    }
    return WR_OK;
}

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_topk_supported(int32_t D, int32_t k) {
    if (k < 1 || k > 256 || D < 4 || D % 4 != 0) return 0;
    return (score_rega_d(D) || topk_lds_generic(D) <= kLdsPerWorkgroup) ? 1 : 0;
}

// an upper bound of what topk_chunks picks that never decreases in n, n_items or k:
// rb * nc <= min(rb * max_chunks(n_items), max(rb, kTopkWgCap)) workgroups of 128 / KQ evaluation rows, rb = ceil(n KQ / 128)
static int64_t topk_workspace(int64_t n, int64_t n_items, int32_t KQ, int32_t k) {
    const int64_t rb = (n * KQ + kScoreRows - 1) / kScoreRows;
    const int64_t a = rb * topk_max_chunks(n_items), b = rb > kTopkWgCap ? rb : kTopkWgCap;
    const int64_t regions = (a < b ? a : b) * (kScoreRows / KQ);
    return regions * topk_region(k) * 8 + 256;
}

int64_t wr_topk_workspace_bytes(int64_t n, int64_t n_items, int32_t D, int32_t k) {
    (void)D;
    if (n < 0 || n_items < 0 || k < 1 || k > 256) {
        set_error("topk_workspace_bytes: n=%lld n_items=%lld k=%d out of range", (long long)n, (long long)n_items, k);
        return WR_E_SHAPE;
    }
    return topk_workspace(n, n_items, 1, k);
}

int32_t wr_topk_multi_supported(int32_t D, int32_t KQ, int32_t k) {
    return ((KQ == 1 || KQ == 2 || KQ == 4) && wr_topk_supported(D, k)) ? 1 : 0;
}

int64_t wr_topk_multi_workspace_bytes(int64_t n, int64_t n_items, int32_t D, int32_t KQ, int32_t k) {
    (void)D;
    if (n < 0 || n >= (int64_t(1) << 31) || n_items < 0 || k < 1 || k > 256 || !(KQ == 1 || KQ == 2 || KQ == 4)) {
        set_error("topk_multi_workspace_bytes: n=%lld n_items=%lld KQ=%d k=%d out of range", (long long)n, (long long)n_items, KQ,
                  k);
        return WR_E_SHAPE;
    }
    return topk_workspace(n, n_items, KQ, k);
}

// the checks the recommend entries share; `entry` starts the message.  KQ query rows per row (checked by the caller).
static int32_t topk_check(const char *entry, int64_t n, int64_t n_items, int32_t D, int32_t KQ, int32_t k, const void *workspace,
                          int64_t workspace_bytes) {
    WR_REQUIRE(n >= 0 && n < (int64_t(1) << 31) / KQ, WR_E_SHAPE, "%s: n out of range", entry);
    WR_REQUIRE(k >= 1 && k <= 256, WR_E_RANGE, "%s: k=%d must be in [1, 256]", entry, k);
    WR_REQUIRE(wr_topk_supported(D, k), WR_E_RANGE,
               "%s supports D in {8,16,32,64} or a multiple of 4 up to 252 (LDS staging: %lld B needed, "
               "163840 B per workgroup); got D=%d", entry, (long long)topk_lds_generic(D), D);
    const int64_t need = topk_workspace(n, n_items, KQ, k);
    WR_REQUIRE(workspace != nullptr && workspace_bytes >= need, WR_E_WORKSPACE,
               "%s: workspace of %lld B, %lld B needed", entry, (long long)workspace_bytes, (long long)need);
    WR_REQUIRE(aligned16(workspace), WR_E_ALIGN, "%s: workspace is not 16-byte aligned", entry);
    return WR_OK;
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
    if ((rc = topk_check("topk_recommend", n, n_items, D, 1, k, workspace, workspace_bytes)) != WR_OK) return rc;
    if (n == 0) return WR_OK;
    return topk_launch<1>(user_mat, item_tab, n_items, D, query_user, query_user, n, mask_ptr, mask_idx, k, out_item, out_score,
                          nullptr, workspace, reinterpret_cast<hipStream_t>(stream_));
}

int32_t wr_topk_recommend_rows(const float *query_mat, int64_t n_query_rows, const float *item_tab, int64_t n_items, int32_t D,
                               const int64_t *query_row, int64_t n, const int64_t *mask_row, int64_t n_mask_rows,
                               const int64_t *mask_ptr, const int32_t *mask_idx, int32_t k, int32_t *out_item,
                               float *out_score, void *workspace, int64_t workspace_bytes, void *stream_) {
    int32_t rc;
    if ((rc = check_table(query_mat, n_query_rows, D, "query_mat")) != WR_OK) return rc;
    if ((rc = check_table(item_tab, n_items, D, "item_tab")) != WR_OK) return rc;
    WR_REQUIRE(out_item && out_score, WR_E_NULL, "topk_recommend_rows: NULL argument");
    WR_REQUIRE((mask_ptr == nullptr) == (mask_idx == nullptr) && (mask_ptr == nullptr) == (mask_row == nullptr), WR_E_NULL,
               "topk_recommend_rows: mask_row, mask_ptr and mask_idx go together");
    WR_REQUIRE(mask_ptr == nullptr || n_mask_rows >= 1, WR_E_SHAPE, "topk_recommend_rows: n_mask_rows=%lld with a mask",
               (long long)n_mask_rows);
    if ((rc = topk_check("topk_recommend_rows", n, n_items, D, 1, k, workspace, workspace_bytes)) != WR_OK) return rc;
    WR_REQUIRE(query_row != nullptr || n <= n_query_rows, WR_E_SHAPE,
               "topk_recommend_rows: n=%lld rows but query_mat has %lld and no query_row is given", (long long)n,
               (long long)n_query_rows);
    if (n == 0) return WR_OK;
    return topk_launch<1>(query_mat, item_tab, n_items, D, query_row, mask_row, n, mask_ptr, mask_idx, k, out_item, out_score,
                          nullptr, workspace, reinterpret_cast<hipStream_t>(stream_));
}

int32_t wr_topk_recommend_multi(const float *query_mat, int64_t n_query_rows, const float *item_tab, int64_t n_items, int32_t D,
                                int32_t KQ, int64_t n, const int64_t *mask_row, int64_t n_mask_rows, const int64_t *mask_ptr,
                                const int32_t *mask_idx, int32_t k, int32_t *out_item, float *out_score, int32_t *out_interest,
                                void *workspace, int64_t workspace_bytes, void *stream_) {
    int32_t rc;
    WR_REQUIRE(KQ == 1 || KQ == 2 || KQ == 4, WR_E_RANGE, "topk_recommend_multi supports KQ in {1, 2, 4}; got KQ=%d", KQ);
    if ((rc = check_table(query_mat, n_query_rows, D, "query_mat")) != WR_OK) return rc;
    if ((rc = check_table(item_tab, n_items, D, "item_tab")) != WR_OK) return rc;
    WR_REQUIRE(out_item && out_score, WR_E_NULL, "topk_recommend_multi: NULL argument");
    WR_REQUIRE((mask_ptr == nullptr) == (mask_idx == nullptr) && (mask_ptr == nullptr) == (mask_row == nullptr), WR_E_NULL,
               "topk_recommend_multi: mask_row, mask_ptr and mask_idx go together");
    WR_REQUIRE(mask_ptr == nullptr || n_mask_rows >= 1, WR_E_SHAPE, "topk_recommend_multi: n_mask_rows=%lld with a mask",
               (long long)n_mask_rows);
    if ((rc = topk_check("topk_recommend_multi", n, n_items, D, KQ, k, workspace, workspace_bytes)) != WR_OK) return rc;
    WR_REQUIRE(n * KQ <= n_query_rows, WR_E_SHAPE, "topk_recommend_multi: n=%lld rows of %d queries but query_mat has %lld rows",
               (long long)n, KQ, (long long)n_query_rows);
    if (n == 0) return WR_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (KQ == 1)
        return topk_launch<1>(query_mat, item_tab, n_items, D, nullptr, mask_row, n, mask_ptr, mask_idx, k, out_item, out_score,
                              out_interest, workspace, stream);
    if (KQ == 2)
        return topk_launch<2>(query_mat, item_tab, n_items, D, nullptr, mask_row, n, mask_ptr, mask_idx, k, out_item, out_score,
                              out_interest, workspace, stream);
    return topk_launch<4>(query_mat, item_tab, n_items, D, nullptr, mask_row, n, mask_ptr, mask_idx, k, out_item, out_score,
                          out_interest, workspace, stream);
}

}  // extern "C"
