// wr_eval.hip — full-ranking evaluation without the [n_eval, n_items] host matrix.
//
// Reference: BaseRunner.interface + evaluate_method (src/helpers/BaseRunner.py:218-258, 50-92) with
// BPRMF/LightGCN.full_predict (src/models/general/BPRMF.py:82-91): scores = U[user] @ I^T for every item, the user's
// train/dev/test items set to -inf (BaseRunner.py:246-255), rank of the ground-truth = its position in the descending
// order.  Only the rank is needed by every metric (HR/NDCG/RECALL/PRECISION@k), and
//     rank_i = 1 + #{ j not masked for user_i : score(i, j) > score(i, target_i) }.
// This is the one GEMM-shaped piece of the path, so it runs on the matrix cores: v_mfma_f32_32x32x2_f32 (f32 in, f32
// accumulate = a k-ordered fmaf chain, MI355X_MICROARCH.md "Matrix cores"), one 32x32 score tile per wave per item tile,
// compared against the target score (computed with the same k-ordered chain, so the target's own column can never count)
// and counted in registers.  A workgroup = 4 waves = 128 evaluation rows sharing each item tile through LDS: the score
// scan of wr_score_tiles.h, with RankCount as its consumer.
#include "wr_score_tiles.h"

namespace wr {

constexpr int kEvalChunk = 2048; // items per workgroup along grid.y

// score of the ground-truth item, as the k-ordered fmaf chain the MFMA accumulates; qrows NULL: row i is its own query
__global__ __launch_bounds__(kBlock) void eval_target_kernel(const float *__restrict__ U, const float *__restrict__ I, int D,
                                                              const int64_t *__restrict__ qrows, const int64_t *__restrict__ et,
                                                              int64_t n, float *__restrict__ tscore) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *a = U + (qrows != nullptr ? qrows[i] : i) * (int64_t)D, *b = I + et[i] * (int64_t)D;
    float s = 0.f;
    for (int k = 0; k < D; ++k) s = fmaf(a[k], b[k], s);
    tscore[i] = s;
}

// Consumer of the score scan: per lane the 16 accumulator rows of its wave's 32-row slab, their target scores and the
// number of unmasked items that beat them.
struct RankCount {
    float trow[16];
    int cnt[16];
    int64_t e_first, n, n_items;   // first row of the slab
    int col, half;

    __device__ __forceinline__ RankCount(const float *__restrict__ tscore, int64_t n_, int64_t n_items_)
        : e_first((int64_t)blockIdx.x * kScoreRows + (threadIdx.x >> 6) * 32), n(n_), n_items(n_items_),
          col(threadIdx.x & 31), half((threadIdx.x & 63) >> 5) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int64_t e = e_first + acc_row(reg, half);
            trow[reg] = (e < n) ? tscore[e] : 3.4e38f;   // rows past the end never count
            cnt[reg] = 0;
        }
    }

    template <int C, typename Masked>
    __device__ __forceinline__ void operator()(const f32x16 (&acc)[C], int64_t j0, bool plain, Masked masked) {
        if (plain) {                                      // wave-uniform: nothing masked, tile inside the table
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
#pragma unroll
                for (int c = 0; c < C; ++c) cnt[reg] += acc[c][reg] > trow[reg] ? 1 : 0;
            }
        } else {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = acc_row(reg, half);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const bool ok = j0 + c * 32 + col < n_items;
                    const bool m = masked(c, row);          // read unconditionally: four rows' words in one LDS load
                    cnt[reg] += (ok && !m && acc[c][reg] > trow[reg]) ? 1 : 0;
                }
            }
        }
    }

    // sum over the 32 item columns (lanes of one half), one integer atomic per row and workgroup
    __device__ __forceinline__ void flush(int *__restrict__ rank_cnt) const {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            int v = cnt[reg];
            v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64);
            const int64_t e = e_first + acc_row(reg, half);
            if (col == 0 && e < n && v) atomicAdd(&rank_cnt[e], v);
        }
    }
};

// D outside {8, 16, 32, 64}: the LDS-operand scan
__global__ __launch_bounds__(kBlock) void eval_rank_kernel(const float *__restrict__ U, const float *__restrict__ I, int D,
                                                            int64_t n_items, const int64_t *__restrict__ qrows,
                                                            const int64_t *__restrict__ mrows,
                                                            const float *__restrict__ tscore, int64_t n,
                                                            const int64_t *__restrict__ mask_ptr, const int *__restrict__ mask_idx,
                                                            int *__restrict__ rank_cnt) {
    RankCount count(tscore, n, n_items);
    score_scan_lds(U, I, D, n_items, qrows, mrows, n, mask_ptr, mask_idx, (int64_t)blockIdx.y * kEvalChunk, kEvalChunk, count);
    count.flush(rank_cnt);
}

// D = 2*KS in {8, 16, 32, 64}: the register-operand scan.
// 3 workgroups per CU (<= 168 VGPRs, no spill): A/B on MI355X 2 / 3 / 4 per CU = 101 / 111 / 86 TFLOP/s at 100K x 100K x 64.
template <int KS>
__global__ __launch_bounds__(kBlock, 3) void eval_rank_kernel_rega(const float *__restrict__ U, const float *__restrict__ I,
                                                                 int64_t n_items, const int64_t *__restrict__ qrows,
                                                                 const int64_t *__restrict__ mrows,
                                                                 const float *__restrict__ tscore, int64_t n,
                                                                 const int64_t *__restrict__ mask_ptr,
                                                                 const int *__restrict__ mask_idx, int *__restrict__ rank_cnt) {
    RankCount count(tscore, n, n_items);
    score_scan_rega<KS>(U, I, n_items, qrows, mrows, n, mask_ptr, mask_idx, (int64_t)blockIdx.y * kEvalChunk, kEvalChunk, count);
    count.flush(rank_cnt);
}

// count -> rank.  A NaN target score compares false with every item and would come out of the count as rank 1: such a row
// ranks behind all n_items items instead, so it is a miss at every k ("Ties and non-finite scores").
__global__ __launch_bounds__(kBlock) void eval_finish_kernel(int *__restrict__ rank, const float *__restrict__ tscore,
                                                              int64_t n_items, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) rank[i] = (tscore[i] != tscore[i]) ? (int)(n_items + 1) : rank[i] + 1;
}

// The launches behind wr_rank_eval and wr_rank_eval_rows; arguments are checked by the entries.
static int32_t rank_eval_launch(const float *query_mat, const float *item_tab, int64_t n_items, int32_t D, const int64_t *qrows,
                                const int64_t *mrows, const int64_t *eval_target, int64_t n, const int64_t *mask_ptr,
                                const int32_t *mask_idx, int32_t *rank, float *target_score, hipStream_t stream) {
    WR_HIP(hipMemsetAsync(rank, 0, (size_t)n * 4, stream));
    hipLaunchKernelGGL(eval_target_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, query_mat, item_tab,
                       D, qrows, eval_target, n, target_score);
    WR_LAUNCH_CHECK("eval_target_kernel");
    const dim3 grid((unsigned)((n + kScoreRows - 1) / kScoreRows), (unsigned)((n_items + kEvalChunk - 1) / kEvalChunk));
    if (score_rega_d(D)) {   // A operand in registers, double-buffered item tiles
#define WR_EVAL_REGA(KS_)                                                                                             \
    hipLaunchKernelGGL(eval_rank_kernel_rega<KS_>, grid, dim3(kBlock), 0, stream, query_mat, item_tab, n_items, qrows, mrows, \
                       target_score, n, mask_ptr, mask_idx, rank)
        WR_DISPATCH_KS(D, 4, 32, WR_EVAL_REGA);
#undef WR_EVAL_REGA
    } else {
        const size_t lds = score_lds_bytes(D, 1);
        if (lds > 64 * 1024)
            WR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(eval_rank_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(eval_rank_kernel, grid, dim3(kBlock), lds, stream, query_mat, item_tab, D, n_items, qrows, mrows,
                           target_score, n, mask_ptr, mask_idx, rank);
    }
    WR_LAUNCH_CHECK("eval_rank_kernel");
    hipLaunchKernelGGL(eval_finish_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, rank,
                       target_score, n_items, n);
    WR_LAUNCH_CHECK("eval_finish_kernel");
    return WR_OK;
}

// ------------------------------------------------------------------------------------------------ K19: KQ queries per row
// A multi-interest model (IF4Rec) scores row e against item j with max_k <Q[e KQ + k], I[j]>.  The scans run unchanged over
// the n KQ query rows (query row e KQ + k = interest k of row e, its mask row repeated KQ times); only the consumer differs:
// acc_row(reg, half) = (reg & 3) + 8 (reg >> 2) + 4 half puts the KQ in {1, 2, 4} query rows of one evaluation row into KQ
// ADJACENT accumulator registers of one lane, so their maximum is taken in registers, compared with the row's target score
// and counted once.  128 rows per workgroup and 32 per wave are multiples of KQ: no group straddles a slab.

// target score = max over k of the k-ordered fmaf chain the MFMA accumulates: the target's own column equals it exactly
template <int KQ>
__global__ __launch_bounds__(kBlock) void eval_target_multi_kernel(const float *__restrict__ Q, const float *__restrict__ I, int D,
                                                                    const int64_t *__restrict__ et, int64_t n,
                                                                    float *__restrict__ tscore) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *b = I + et[i] * (int64_t)D;
    float best = 0.f;
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
        const float *a = Q + (i * KQ + q) * (int64_t)D;
        float s = 0.f;
        for (int k = 0; k < D; ++k) s = fmaf(a[k], b[k], s);
        best = q == 0 ? s : fmaxf(best, s);
    }
    tscore[i] = best;
}

template <int KQ>
struct RankCountMulti {
    static constexpr int NG = 16 / KQ;     // evaluation rows per lane
    float trow[NG];
    int cnt[NG];
    int64_t q_first, n, n_items;           // first QUERY row of the slab; n evaluation rows
    int col, half;

    __device__ __forceinline__ RankCountMulti(const float *__restrict__ tscore, int64_t n_, int64_t n_items_)
        : q_first((int64_t)blockIdx.x * kScoreRows + (threadIdx.x >> 6) * 32), n(n_), n_items(n_items_),
          col(threadIdx.x & 31), half((threadIdx.x & 63) >> 5) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int64_t e = (q_first + acc_row(g * KQ, half)) / KQ;
            trow[g] = (e < n) ? tscore[e] : 3.4e38f;   // rows past the end never count
            cnt[g] = 0;
        }
    }

    template <int C>
    __device__ __forceinline__ float best(const f32x16 (&acc)[C], int c, int g) const {
        float m = acc[c][g * KQ];
#pragma unroll
        for (int q = 1; q < KQ; ++q) m = fmaxf(m, acc[c][g * KQ + q]);
        return m;
    }

    template <int C, typename Masked>
    __device__ __forceinline__ void operator()(const f32x16 (&acc)[C], int64_t j0, bool plain, Masked masked) {
        if (plain) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
#pragma unroll
                for (int c = 0; c < C; ++c) cnt[g] += best<C>(acc, c, g) > trow[g] ? 1 : 0;
            }
        } else {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int row = acc_row(g * KQ, half);      // the KQ query rows of a group share one mask list
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const bool ok = j0 + c * 32 + col < n_items;
                    const bool m = masked(c, row);
                    cnt[g] += (ok && !m && best<C>(acc, c, g) > trow[g]) ? 1 : 0;
                }
            }
        }
    }

    __device__ __forceinline__ void flush(int *__restrict__ rank_cnt) const {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            int v = cnt[g];
            v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64);
            const int64_t e = (q_first + acc_row(g * KQ, half)) / KQ;
            if (col == 0 && e < n && v) atomicAdd(&rank_cnt[e], v);
        }
    }
};

template <int KQ>
__global__ __launch_bounds__(kBlock) void eval_rank_multi_kernel(const float *__restrict__ Q, const float *__restrict__ I, int D,
                                                                  int64_t n_items, const int64_t *__restrict__ mrows,
                                                                  const float *__restrict__ tscore, int64_t n,
                                                                  const int64_t *__restrict__ mask_ptr, const int *__restrict__ mask_idx,
                                                                  int *__restrict__ rank_cnt) {
    RankCountMulti<KQ> count(tscore, n, n_items);
    score_scan_lds(Q, I, D, n_items, nullptr, mrows, n * KQ, mask_ptr, mask_idx, (int64_t)blockIdx.y * kEvalChunk, kEvalChunk, count);
    count.flush(rank_cnt);
}

template <int KS, int KQ>
__global__ __launch_bounds__(kBlock, 3) void eval_rank_multi_kernel_rega(const float *__restrict__ Q, const float *__restrict__ I,
                                                                       int64_t n_items, const int64_t *__restrict__ mrows,
                                                                       const float *__restrict__ tscore, int64_t n,
                                                                       const int64_t *__restrict__ mask_ptr,
                                                                       const int *__restrict__ mask_idx, int *__restrict__ rank_cnt) {
    RankCountMulti<KQ> count(tscore, n, n_items);
    score_scan_rega<KS>(Q, I, n_items, nullptr, mrows, n * KQ, mask_ptr, mask_idx, (int64_t)blockIdx.y * kEvalChunk, kEvalChunk, count);
    count.flush(rank_cnt);
}

template <int KQ>
static int32_t rank_eval_multi_launch(const float *query_mat, const float *item_tab, int64_t n_items, int32_t D, const int64_t *mrows,
                                      const int64_t *eval_target, int64_t n, const int64_t *mask_ptr, const int32_t *mask_idx,
                                      int32_t *rank, float *target_score, hipStream_t stream) {
    WR_HIP(hipMemsetAsync(rank, 0, (size_t)n * 4, stream));
    hipLaunchKernelGGL(eval_target_multi_kernel<KQ>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, query_mat,
                       item_tab, D, eval_target, n, target_score);
    WR_LAUNCH_CHECK("eval_target_multi_kernel");
    const dim3 grid((unsigned)((n * KQ + kScoreRows - 1) / kScoreRows), (unsigned)((n_items + kEvalChunk - 1) / kEvalChunk));
    if (score_rega_d(D)) {
#define WR_EVAL_MULTI_REGA(KS_)                                                                                        \
    hipLaunchKernelGGL((eval_rank_multi_kernel_rega<KS_, KQ>), grid, dim3(kBlock), 0, stream, query_mat, item_tab, n_items, mrows, \
                       target_score, n, mask_ptr, mask_idx, rank)
        WR_DISPATCH_KS(D, 4, 32, WR_EVAL_MULTI_REGA);
#undef WR_EVAL_MULTI_REGA
    } else {
        const size_t lds = score_lds_bytes(D, 1);
        if (lds > 64 * 1024)
            WR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(eval_rank_multi_kernel<KQ>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(eval_rank_multi_kernel<KQ>, grid, dim3(kBlock), lds, stream, query_mat, item_tab, D, n_items, mrows,
                           target_score, n, mask_ptr, mask_idx, rank);
    }
    WR_LAUNCH_CHECK("eval_rank_multi_kernel");
    hipLaunchKernelGGL(eval_finish_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, rank,
                       target_score, n_items, n);
    WR_LAUNCH_CHECK("eval_finish_kernel");
    return WR_OK;
}

static inline bool rank_eval_d_ok(int32_t D) {
    return D >= 4 && D % 4 == 0 && (score_rega_d(D) || score_lds_bytes(D, 1) <= kLdsPerWorkgroup);
}

// D outside {8,16,32,64}: the LDS-operand kernel stages (128 + 32) rows of D + 1 floats + 128 bitmap words; a
// workgroup gets at most 160 KiB (163,840 B) on gfx950 -> D <= 252
#define WR_EVAL_REQUIRE_D(D_)                                                                                          \
    WR_REQUIRE(score_rega_d(D_) || score_lds_bytes(D_, 1) <= kLdsPerWorkgroup, WR_E_RANGE,                             \
               "rank_eval supports D <= 252 (LDS staging: %lld B needed, 163840 B per workgroup); got D=%d",           \
               (long long)score_lds_bytes(D_, 1), D_)

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_rank_eval(const float *user_mat, int64_t n_user_rows, const float *item_tab, int64_t n_items, int32_t D,
                     const int64_t *eval_user, const int64_t *eval_target, int64_t n, const int64_t *mask_ptr,
                     const int32_t *mask_idx, int32_t *rank, float *target_score, void *stream_) {
    int32_t rc;
    if ((rc = check_table(user_mat, n_user_rows, D, "user_mat")) != WR_OK) return rc;
    if ((rc = check_table(item_tab, n_items, D, "item_tab")) != WR_OK) return rc;
    WR_REQUIRE(eval_user && eval_target && rank && target_score, WR_E_NULL, "rank_eval: NULL argument");
    WR_REQUIRE((mask_ptr == nullptr) == (mask_idx == nullptr), WR_E_NULL, "rank_eval: mask_ptr and mask_idx go together");
    WR_REQUIRE(n >= 0 && n < (int64_t(1) << 31), WR_E_SHAPE, "rank_eval: n out of range");
    WR_EVAL_REQUIRE_D(D);
    if (n == 0) return WR_OK;
    return rank_eval_launch(user_mat, item_tab, n_items, D, eval_user, eval_user, eval_target, n, mask_ptr, mask_idx, rank,
                            target_score, reinterpret_cast<hipStream_t>(stream_));
}

int32_t wr_rank_eval_rows(const float *query_mat, int64_t n_query_rows, const float *item_tab, int64_t n_items, int32_t D,
                          const int64_t *query_row, const int64_t *eval_target, int64_t n, const int64_t *mask_row,
                          int64_t n_mask_rows, const int64_t *mask_ptr, const int32_t *mask_idx, int32_t *rank,
                          float *target_score, void *stream_) {
    int32_t rc;
    if ((rc = check_table(query_mat, n_query_rows, D, "query_mat")) != WR_OK) return rc;
    if ((rc = check_table(item_tab, n_items, D, "item_tab")) != WR_OK) return rc;
    WR_REQUIRE(eval_target && rank && target_score, WR_E_NULL, "rank_eval_rows: NULL argument");
    WR_REQUIRE((mask_ptr == nullptr) == (mask_idx == nullptr) && (mask_ptr == nullptr) == (mask_row == nullptr), WR_E_NULL,
               "rank_eval_rows: mask_row, mask_ptr and mask_idx go together");
    WR_REQUIRE(n >= 0 && n < (int64_t(1) << 31), WR_E_SHAPE, "rank_eval_rows: n out of range");
    WR_REQUIRE(query_row != nullptr || n <= n_query_rows, WR_E_SHAPE,
               "rank_eval_rows: n=%lld rows but query_mat has %lld and no query_row is given", (long long)n, (long long)n_query_rows);
    WR_REQUIRE(mask_ptr == nullptr || n_mask_rows >= 1, WR_E_SHAPE, "rank_eval_rows: n_mask_rows=%lld with a mask",
               (long long)n_mask_rows);
    WR_EVAL_REQUIRE_D(D);
    if (n == 0) return WR_OK;
    return rank_eval_launch(query_mat, item_tab, n_items, D, query_row, mask_row, eval_target, n, mask_ptr, mask_idx, rank,
                            target_score, reinterpret_cast<hipStream_t>(stream_));
}

int32_t wr_rank_eval_multi_supported(int32_t D, int32_t KQ) {
    return (rank_eval_d_ok(D) && (KQ == 1 || KQ == 2 || KQ == 4)) ? 1 : 0;
}

int32_t wr_rank_eval_multi(const float *query_mat, int64_t n_query_rows, const float *item_tab, int64_t n_items, int32_t D,
                           int32_t KQ, const int64_t *eval_target, int64_t n, const int64_t *mask_row, int64_t n_mask_rows,
                           const int64_t *mask_ptr, const int32_t *mask_idx, int32_t *rank, float *target_score, void *stream_) {
    int32_t rc;
    WR_REQUIRE(KQ == 1 || KQ == 2 || KQ == 4, WR_E_RANGE, "rank_eval_multi supports KQ in {1, 2, 4}; got KQ=%d", KQ);
    if ((rc = check_table(query_mat, n_query_rows, D, "query_mat")) != WR_OK) return rc;
    if ((rc = check_table(item_tab, n_items, D, "item_tab")) != WR_OK) return rc;
    WR_REQUIRE(eval_target && rank && target_score, WR_E_NULL, "rank_eval_multi: NULL argument");
    WR_REQUIRE((mask_ptr == nullptr) == (mask_idx == nullptr) && (mask_ptr == nullptr) == (mask_row == nullptr), WR_E_NULL,
               "rank_eval_multi: mask_row, mask_ptr and mask_idx go together");
    WR_REQUIRE(n >= 0 && n * KQ < (int64_t(1) << 31), WR_E_SHAPE, "rank_eval_multi: n out of range");
    WR_REQUIRE(n * KQ <= n_query_rows, WR_E_SHAPE, "rank_eval_multi: n=%lld rows of %d queries but query_mat has %lld rows",
               (long long)n, KQ, (long long)n_query_rows);
    WR_REQUIRE(mask_ptr == nullptr || n_mask_rows >= 1, WR_E_SHAPE, "rank_eval_multi: n_mask_rows=%lld with a mask",
               (long long)n_mask_rows);
    WR_EVAL_REQUIRE_D(D);
    if (n == 0) return WR_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (KQ == 1)
        return rank_eval_multi_launch<1>(query_mat, item_tab, n_items, D, mask_row, eval_target, n, mask_ptr, mask_idx, rank,
                                         target_score, stream);
    if (KQ == 2)
        return rank_eval_multi_launch<2>(query_mat, item_tab, n_items, D, mask_row, eval_target, n, mask_ptr, mask_idx, rank,
                                         target_score, stream);
    return rank_eval_multi_launch<4>(query_mat, item_tab, n_items, D, mask_row, eval_target, n, mask_ptr, mask_idx, rank,
                                     target_score, stream);
}

}  // extern "C"
