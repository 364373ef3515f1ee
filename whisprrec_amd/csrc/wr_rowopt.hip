// wr_rowopt.hip — row-lazy dense optimizers for a table whose gradient rows come from autograd (K22).
//
// The item table of a sequential model (reference src/models/sequential/SASRec.py:60,84,105-106) is looked up at a few
// thousand positions per step, yet torch.optim.Adam / SGD(weight_decay) (src/helpers/BaseRunner.py:120-124,199) move all of
// its rows at every step, and the backward of every lookup builds a zero [n_rows, D] table first.  wr_lazy.hip removed the
// table passes for BPRMF, whose step kernels know the batch; here the same exact replay is offered to any caller that holds
// (index, gradient row) pairs:
//   * gather     out[k,:] = row idx[k] AS OF step `upto`: the wave replays the zero-gradient steps the row missed in registers
//                and writes only `out`.  The table, the moments and last[] are read-only, so duplicates and concurrent readers
//                need no dedup, no atomics and no index work in the forward pass;
//   * sparse step  the step's positions in (row, position) order: one wave per run of equal rows sums the run's gradient rows
//                in position order (the association of wr_scatter_add_rows into a zero table), replays the row up to step t-1,
//                applies step t with the sum and writes w, m, v and last[row] = t.  No [n_rows, D] gradient exists anywhere;
//   * the rows nobody asked for are brought up to date by wr_adam_catchup_all / wr_sgd_catchup_all (wr_lazy.hip), whole or on a
//                rotating window (bounded lag).
// Element arithmetic and order are those of wr_adam_dense / wr_sgd_dense (adam_elem, adam_replay_elem, sgd_decay_elem of
// wr_common.h): after a catch-up the table and the moments hold the bits the dense kernels produce from the scatter-added
// gradient table.
//
// One wave per row, lane-strided elements (wr_lazy.hip): a wave's lanes replay the same number of steps, no divergence.
#include "wr_common.h"

namespace wr {

constexpr int kWave = 64;
constexpr int kGatherRowsPerWave = 4;         // positions a wave of the gather has in flight (big calls; wr_lazy.hip's choice)
constexpr int64_t kSmallGather = 32768;       // fewer positions: one per wave, more waves to spread the replays
constexpr int kRunFly = 16;                   // gradient rows of a run requested together, added in order

enum : int { kErrRow = 1, kErrPerm = 2 };     // bits of the device error word

__device__ __forceinline__ void report(int *__restrict__ err, int bit, int lane) {
    if (err != nullptr && lane == 0) atomicOr(err, bit);
}

// The R positions of a wave: row ids (-1: none, or outside the table — reported, never dereferenced) and their last steps.
template <int R>
__device__ __forceinline__ void gather_heads(const int64_t *__restrict__ idx, int64_t n, int64_t n_rows, int64_t k0,
                                             const int *__restrict__ last, int (&rows)[R], int (&from)[R],
                                             int *__restrict__ err, int lane) {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        int r = -1;
        if (k0 + j < n) {
            const int64_t id = idx[k0 + j];
            if (id < 0 || id >= n_rows) bad = true;
            else r = (int)id;
        }
        rows[j] = __builtin_amdgcn_readfirstlane(r);
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int f = (rows[j] >= 0 && last != nullptr) ? last[rows[j]] : 0;
        from[j] = __builtin_amdgcn_readfirstlane(f < 0 ? 0 : f);            // consts[] is never read before step 1
    }
    if (bad) report(err, kErrRow, lane);
}

template <bool L2, int R>
__global__ __launch_bounds__(kBlock) void gather_rows_lazy_kernel(const float *__restrict__ w, const float *__restrict__ m,
                                                                   const float *__restrict__ v, const int *__restrict__ last,
                                                                   int64_t n_rows, int D, const int64_t *__restrict__ idx,
                                                                   int64_t n, int upto, const float *__restrict__ consts,
                                                                   float l2, float b1, float b2, float eps,
                                                                   float *__restrict__ out, int *__restrict__ err) {
    const int lane = threadIdx.x % kWave;
    const int64_t k0 = ((int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave) * R;
    if (k0 >= n) return;
    const float2 *__restrict__ c2 = reinterpret_cast<const float2 *>(consts);
    int rows[R], from[R];
    gather_heads<R>(idx, n, n_rows, k0, last, rows, from, err, lane);
    for (int e = lane; e < D; e += kWave) {
        float ww[R], mm[R], vv[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            ww[j] = mm[j] = vv[j] = 0.f;
            if (rows[j] < 0) continue;
            const int64_t at = rows[j] * (int64_t)D + e;
            ww[j] = w[at];
            if (from[j] < upto) { mm[j] = m[at]; vv[j] = v[at]; }     // a current row needs no moments
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (k0 + j >= n) continue;
            if (rows[j] >= 0) adam_replay_elem<L2>(ww[j], mm[j], vv[j], from[j], upto, c2, l2, b1, b2, eps);
            out[(k0 + j) * (int64_t)D + e] = ww[j];                   // a position outside the table: zeros
        }
    }
}

template <int R>
__global__ __launch_bounds__(kBlock) void gather_rows_lazy_sgd_kernel(const float *__restrict__ w, const int *__restrict__ last,
                                                                       int64_t n_rows, int D, const int64_t *__restrict__ idx,
                                                                       int64_t n, int upto, float lr, float l2,
                                                                       float *__restrict__ out, int *__restrict__ err) {
    const int lane = threadIdx.x % kWave;
    const int64_t k0 = ((int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave) * R;
    if (k0 >= n) return;
    int rows[R], from[R];
    gather_heads<R>(idx, n, n_rows, k0, last, rows, from, err, lane);
    for (int e = lane; e < D; e += kWave) {
        float ww[R];
#pragma unroll
        for (int j = 0; j < R; ++j) ww[j] = rows[j] >= 0 ? w[rows[j] * (int64_t)D + e] : 0.f;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (k0 + j >= n) continue;
            if (rows[j] >= 0)
                for (int s = from[j]; s < upto; ++s) ww[j] = sgd_decay_elem(ww[j], lr, l2);
            out[(k0 + j) * (int64_t)D + e] = ww[j];
        }
    }
}

// Sort keys of a step's positions: the row id, or n_rows for an id outside the table (reported; such keys sort behind every
// row and no run of them is ever applied).  padding_idx keeps its id: its row takes the step with a zero gradient.
__global__ __launch_bounds__(kBlock) void sparse_keys_kernel(const int64_t *__restrict__ idx, int64_t n, int64_t n_rows,
                                                              int *__restrict__ keys, int *__restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t r = idx[i];
    const bool bad = r < 0 || r >= n_rows;
    keys[i] = bad ? (int)n_rows : (int)r;
    if (bad && err != nullptr) atomicOr(err, kErrRow);
}

// The wave of position q0 heads a run iff the key before it differs; -> its row, or -1.
__device__ __forceinline__ int run_head(const int *__restrict__ keys, int64_t q0, int64_t n_rows) {
    int row = keys[q0];
    if (q0 > 0 && keys[q0 - 1] == row) row = -1;
    if (row >= n_rows) row = -1;                       // the keys of ids outside the table
    return __builtin_amdgcn_readfirstlane(row);
}

// Element e of the sum of src[perm[q], :] over the run of `row` that starts at q0, in ascending q, from +0: the association of
// wr_scatter_add_rows into a zero table.  The wave's lanes fetch 64 (key, position) pairs of the run per trip, the positions
// are handed round, kRunFly gradient rows are requested together and added in order.  Every lane of the wave calls this
// (`active`: the lane holds an element); all branches are wave-uniform.
__device__ __forceinline__ float run_sum(const int *__restrict__ keys, const int64_t *__restrict__ perm, int64_t n, int64_t q0,
                                         int row, const float *__restrict__ src, int D, int e, bool active, int lane,
                                         int *__restrict__ err) {
    float acc = 0.f;
    for (int64_t qb = q0;; qb += kWave) {
        const int64_t q = qb + lane;
        const bool in = q < n && keys[q] == row;
        const unsigned long long mask = __ballot(in);
        const int cnt = ~mask == 0ull ? kWave : __builtin_ctzll(~mask);     // lanes 0 .. cnt-1 hold the run's next entries
        int64_t sp = (in && lane < cnt) ? perm[q] : 0;
        const bool bad = sp < 0 || sp >= n;                                 // never read outside src
        if (__ballot(bad) != 0ull) report(err, kErrPerm, lane);
        const int spi = bad ? -1 : (int)sp;
        for (int j = 0; j < cnt; j += kRunFly) {
            float x[kRunFly];
#pragma unroll
            for (int f = 0; f < kRunFly; ++f) {
                const int s = __shfl(spi, (j + f) & (kWave - 1), kWave);
                x[f] = (j + f < cnt && s >= 0 && active) ? src[s * (int64_t)D + e] : 0.f;
            }
#pragma unroll
            for (int f = 0; f < kRunFly; ++f)
                if (j + f < cnt) acc += x[f];
        }
        if (cnt < kWave) break;
    }
    return acc;
}

template <bool L2>
__global__ __launch_bounds__(kBlock) void adam_rows_sparse_kernel(float *__restrict__ w, float *__restrict__ m,
                                                                   float *__restrict__ v, int *__restrict__ last, int64_t n_rows,
                                                                   int D, const int *__restrict__ keys,
                                                                   const int64_t *__restrict__ perm, int64_t n,
                                                                   const float *__restrict__ src, int64_t padding_idx, int step,
                                                                   const float *__restrict__ consts, float l2, float b1,
                                                                   float b2, float eps, int *__restrict__ err) {
    const int lane = threadIdx.x % kWave;
    const int64_t q0 = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (q0 >= n) return;
    const int row = run_head(keys, q0, n_rows);
    if (row < 0) return;
    const float2 *__restrict__ c2 = reinterpret_cast<const float2 *>(consts);
    const int from = max(__builtin_amdgcn_readfirstlane(last[row]), 0);
    const bool pad = row == padding_idx;               // no gradient, but the row takes the step: it stays current
    const float2 k = c2[step];
    for (int e0 = 0; e0 < D; e0 += kWave) {
        const int e = e0 + lane;
        const bool active = e < D;
        const int64_t at = row * (int64_t)D + e;
        float ww = 0.f, mm = 0.f, vv = 0.f;
        if (active) { ww = w[at]; mm = m[at]; vv = v[at]; }
        const float g = pad ? 0.f : run_sum(keys, perm, n, q0, row, src, D, e, active, lane, err);
        if (!active) continue;
        adam_replay_elem<L2>(ww, mm, vv, from, step - 1, c2, l2, b1, b2, eps);
        adam_elem<L2>(ww, mm, vv, g, l2, b1, b2, eps, k.x, k.y);
        w[at] = ww; m[at] = mm; v[at] = vv;
    }
    if (lane == 0) last[row] = step;
}

// DECAY: l2 != 0 — the row replays the decays it missed, takes the step with g + l2*w and is marked; else w -= lr*g, no state.
template <bool DECAY>
__global__ __launch_bounds__(kBlock) void sgd_rows_sparse_kernel(float *__restrict__ w, int *__restrict__ last, int64_t n_rows,
                                                                  int D, const int *__restrict__ keys,
                                                                  const int64_t *__restrict__ perm, int64_t n,
                                                                  const float *__restrict__ src, int64_t padding_idx, int step,
                                                                  float lr, float l2, int *__restrict__ err) {
    const int lane = threadIdx.x % kWave;
    const int64_t q0 = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (q0 >= n) return;
    const int row = run_head(keys, q0, n_rows);
    if (row < 0) return;
    const bool pad = row == padding_idx;
    if (!DECAY && pad) return;                          // w - lr * 0
    const int from = DECAY ? max(__builtin_amdgcn_readfirstlane(last[row]), 0) : 0;
    for (int e0 = 0; e0 < D; e0 += kWave) {
        const int e = e0 + lane;
        const bool active = e < D;
        const int64_t at = row * (int64_t)D + e;
        float ww = active ? w[at] : 0.f;
        float g = pad ? 0.f : run_sum(keys, perm, n, q0, row, src, D, e, active, lane, err);
        if (!active) continue;
        if (DECAY) {
            for (int s = from; s < step - 1; ++s) ww = sgd_decay_elem(ww, lr, l2);
            g = fmaf(l2, ww, g);                        // wr_sgd_dense: g' = g + l2*w
        }
        ww -= lr * g;
        w[at] = ww;
    }
    if (DECAY && lane == 0) last[row] = step;
}

static inline unsigned waves_grid(int64_t n_waves) {
    const int64_t g = (n_waves + kBlock / kWave - 1) / (kBlock / kWave);
    return (unsigned)(g < 1 ? 1 : g);
}

static int32_t check_positions(const char *entry, const void *idx, int64_t n) {
    WR_REQUIRE(n >= 0 && n < (int64_t(1) << 31), WR_E_SHAPE, "%s: n=%lld out of range", entry, (long long)n);
    WR_REQUIRE(n == 0 || idx != nullptr, WR_E_NULL, "%s: the index array is NULL", entry);
    return WR_OK;
}

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_gather_rows_lazy(const float *tab, const float *exp_avg, const float *exp_avg_sq, const int32_t *last_step,
                            int64_t n_rows, int32_t D, const int64_t *idx, int64_t n, int64_t upto, const float *consts,
                            int64_t n_consts, float l2, float beta1, float beta2, float eps, float *out, int32_t *err_word,
                            void *stream_) {
    int32_t rc;
    if ((rc = check_tables({{tab, n_rows, "tab"}, {exp_avg, n_rows, "exp_avg"}, {exp_avg_sq, n_rows, "exp_avg_sq"}}, D)) != WR_OK)
        return rc;
    WR_REQUIRE(last_step != nullptr && consts != nullptr, WR_E_NULL, "last_step / consts is NULL");
    WR_REQUIRE(upto >= 0 && upto < n_consts && upto < INT32_MAX, WR_E_RANGE, "step %lld outside the consts table (%lld entries)",
               (long long)upto, (long long)n_consts);
    if ((rc = check_positions("wr_gather_rows_lazy", idx, n)) != WR_OK) return rc;
    if (n == 0) return WR_OK;
    WR_REQUIRE(out != nullptr, WR_E_NULL, "out is NULL");
    const bool small = n < kSmallGather;
    auto kern = small ? (l2 != 0.f ? gather_rows_lazy_kernel<true, 1> : gather_rows_lazy_kernel<false, 1>)
                      : (l2 != 0.f ? gather_rows_lazy_kernel<true, kGatherRowsPerWave>
                                   : gather_rows_lazy_kernel<false, kGatherRowsPerWave>);
    const int R = small ? 1 : kGatherRowsPerWave;
    hipLaunchKernelGGL(kern, dim3(waves_grid((n + R - 1) / R)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream_), tab,
                       exp_avg, exp_avg_sq, last_step, n_rows, D, idx, n, (int)upto, consts, l2, beta1, beta2, eps, out, err_word);
    WR_LAUNCH_CHECK("gather_rows_lazy_kernel");
    return WR_OK;
}

int32_t wr_gather_rows_lazy_sgd(const float *tab, const int32_t *last_step, int64_t n_rows, int32_t D, const int64_t *idx,
                                int64_t n, int64_t upto, float lr, float l2, float *out, int32_t *err_word, void *stream_) {
    int32_t rc;
    if ((rc = check_table(tab, n_rows, D, "tab")) != WR_OK) return rc;
    WR_REQUIRE(last_step != nullptr, WR_E_NULL, "last_step is NULL");
    WR_REQUIRE(upto >= 0 && upto < INT32_MAX, WR_E_RANGE, "step must be >= 0");
    if ((rc = check_positions("wr_gather_rows_lazy_sgd", idx, n)) != WR_OK) return rc;
    if (n == 0) return WR_OK;
    WR_REQUIRE(out != nullptr, WR_E_NULL, "out is NULL");
    const bool small = n < kSmallGather;
    const int R = small ? 1 : kGatherRowsPerWave;
    hipLaunchKernelGGL(small ? gather_rows_lazy_sgd_kernel<1> : gather_rows_lazy_sgd_kernel<kGatherRowsPerWave>,
                       dim3(waves_grid((n + R - 1) / R)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream_), tab, last_step,
                       n_rows, D, idx, n, (int)upto, lr, l2, out, err_word);
    WR_LAUNCH_CHECK("gather_rows_lazy_sgd_kernel");
    return WR_OK;
}

int32_t wr_rows_sparse_keys(const int64_t *idx, int64_t n, int64_t n_rows, int32_t *keys, int32_t *err_word, void *stream_) {
    int32_t rc;
    if ((rc = check_positions("wr_rows_sparse_keys", idx, n)) != WR_OK) return rc;
    WR_REQUIRE(n_rows > 0 && n_rows < (int64_t(1) << 31), WR_E_SHAPE, "n_rows=%lld out of range", (long long)n_rows);
    if (n == 0) return WR_OK;
    WR_REQUIRE(keys != nullptr, WR_E_NULL, "keys is NULL");
    hipLaunchKernelGGL(sparse_keys_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream_), idx, n, n_rows, keys, err_word);
    WR_LAUNCH_CHECK("sparse_keys_kernel");
    return WR_OK;
}

int32_t wr_adam_rows_sparse(float *tab, float *exp_avg, float *exp_avg_sq, int32_t *last_step, int64_t n_rows, int32_t D,
                            const int32_t *sorted_rows, const int64_t *perm, int64_t n, const float *src, int64_t padding_idx,
                            int64_t adam_step, const float *consts, int64_t n_consts, float l2, float beta1, float beta2,
                            float eps, int32_t *err_word, void *stream_) {
    int32_t rc;
    if ((rc = check_tables({{tab, n_rows, "tab"}, {exp_avg, n_rows, "exp_avg"}, {exp_avg_sq, n_rows, "exp_avg_sq"}}, D)) != WR_OK)
        return rc;
    WR_REQUIRE(last_step != nullptr && consts != nullptr, WR_E_NULL, "last_step / consts is NULL");
    WR_REQUIRE(adam_step >= 1 && adam_step < n_consts && adam_step < INT32_MAX, WR_E_RANGE,
               "adam_step %lld outside the consts table (%lld entries)", (long long)adam_step, (long long)n_consts);
    if ((rc = check_positions("wr_adam_rows_sparse", sorted_rows, n)) != WR_OK) return rc;
    if (n == 0) return WR_OK;
    WR_REQUIRE(perm != nullptr && src != nullptr, WR_E_NULL, "perm / src is NULL");
    hipLaunchKernelGGL(l2 != 0.f ? adam_rows_sparse_kernel<true> : adam_rows_sparse_kernel<false>, dim3(waves_grid(n)),
                       dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream_), tab, exp_avg, exp_avg_sq, last_step, n_rows, D,
                       sorted_rows, perm, n, src, padding_idx, (int)adam_step, consts, l2, beta1, beta2, eps, err_word);
    WR_LAUNCH_CHECK("adam_rows_sparse_kernel");
    return WR_OK;
}

int32_t wr_sgd_rows_sparse(float *tab, int32_t *last_step, int64_t n_rows, int32_t D, const int32_t *sorted_rows,
                           const int64_t *perm, int64_t n, const float *src, int64_t padding_idx, int64_t step, float lr,
                           float l2, int32_t *err_word, void *stream_) {
    int32_t rc;
    if ((rc = check_table(tab, n_rows, D, "tab")) != WR_OK) return rc;
    WR_REQUIRE(l2 == 0.f || last_step != nullptr, WR_E_NULL, "last_step is NULL");
    WR_REQUIRE(step >= 1 && step < INT32_MAX, WR_E_RANGE, "step must be >= 1");
    if ((rc = check_positions("wr_sgd_rows_sparse", sorted_rows, n)) != WR_OK) return rc;
    if (n == 0) return WR_OK;
    WR_REQUIRE(perm != nullptr && src != nullptr, WR_E_NULL, "perm / src is NULL");
    hipLaunchKernelGGL(l2 != 0.f ? sgd_rows_sparse_kernel<true> : sgd_rows_sparse_kernel<false>, dim3(waves_grid(n)), dim3(kBlock),
                       0, reinterpret_cast<hipStream_t>(stream_), tab, last_step, n_rows, D, sorted_rows, perm, n, src, padding_idx,
                       (int)step, lr, l2, err_word);
    WR_LAUNCH_CHECK("sgd_rows_sparse_kernel");
    return WR_OK;
}

}  // extern "C"
