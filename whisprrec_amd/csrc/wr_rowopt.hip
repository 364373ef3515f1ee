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
//
// K24 (further down): the same three operations for a PAIR of tables, BUIR's online table and the target that follows it by a
// momentum update after every optimizer step — the replay of a missed step is "zero-gradient step, then target update".
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

// ------------------------------------------------------------------------------------------------ K24: online + target pair
// BUIR's tables (reference src/models/general/BUIR.py:69-72): after every optimizer step the target follows the online table
// by tgt = tgt*mom + w*(1 - mom).  A row that no step names still moves twice per step — the optimizer with a zero gradient,
// then the momentum update towards the row's NEW w — so the replay of one missed step is exactly that pair, step by step (no
// closed form: w changes under Adam and under weight decay).  last[row] = s: the row has had s optimizer steps AND s target
// updates.  Same three operations as above, on (w, tgt) together.
struct EmaOpt {
    const float2 *c2;                          // Adam: {step_size, 1/sqrt(bias_correction2)} per step; SGD: unused
    float lr, l2, b1, b2, eps, mom, one_minus_mom;
};

// Steps from+1 .. upto of one element with a zero gradient, each followed by its target update.  Adam fetches the constants of
// four steps together, as adam_replay_elem does.
template <bool ADAM, bool L2>
__device__ __forceinline__ void ema_replay_elem(float &w, float &m, float &v, float &t, int from, int upto, const EmaOpt &o) {
    if (ADAM) {
        auto replay = [&](float2 k) {
            if (L2) adam_elem<true>(w, m, v, 0.f, o.l2, o.b1, o.b2, o.eps, k.x, k.y);
            else adam_elem_zero_grad(w, m, v, o.b1, o.b2, o.eps, k.x, k.y);
            t = ema_elem(t, w, o.mom, o.one_minus_mom);
        };
        int s = from + 1;
        for (; s + 3 <= upto; s += 4) {
            const float2 k0 = o.c2[s], k1 = o.c2[s + 1], k2 = o.c2[s + 2], k3 = o.c2[s + 3];
            replay(k0); replay(k1); replay(k2); replay(k3);
        }
        for (; s <= upto; ++s) replay(o.c2[s]);
    } else {
        for (int s = from; s < upto; ++s) {
            if (L2) w = sgd_decay_elem(w, o.lr, o.l2);             // l2 == 0: w stays, the target still moves
            t = ema_elem(t, w, o.mom, o.one_minus_mom);
        }
    }
}

template <bool ADAM, bool L2, int R>
__global__ __launch_bounds__(kBlock) void gather_rows_ema_kernel(const float *__restrict__ w, const float *__restrict__ tgt,
                                                                  const float *__restrict__ m, const float *__restrict__ v,
                                                                  const int *__restrict__ last, int64_t n_rows, int D,
                                                                  const int64_t *__restrict__ idx, int64_t n, int upto, EmaOpt o,
                                                                  float *__restrict__ out_w, float *__restrict__ out_t,
                                                                  int *__restrict__ err) {
    const int lane = threadIdx.x % kWave;
    const int64_t k0 = ((int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave) * R;
    if (k0 >= n) return;
    int rows[R], from[R];
    gather_heads<R>(idx, n, n_rows, k0, last, rows, from, err, lane);
    for (int e = lane; e < D; e += kWave) {
        float ww[R], tt[R], mm[R], vv[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            ww[j] = tt[j] = mm[j] = vv[j] = 0.f;
            if (rows[j] < 0) continue;
            const int64_t at = rows[j] * (int64_t)D + e;
            ww[j] = w[at];
            tt[j] = tgt[at];
            if (ADAM && from[j] < upto) { mm[j] = m[at]; vv[j] = v[at]; }     // a current row needs no moments
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (k0 + j >= n) continue;
            if (rows[j] >= 0) ema_replay_elem<ADAM, L2>(ww[j], mm[j], vv[j], tt[j], from[j], upto, o);
            out_w[(k0 + j) * (int64_t)D + e] = ww[j];                         // a position outside the table: zeros
            out_t[(k0 + j) * (int64_t)D + e] = tt[j];
        }
    }
}

template <bool ADAM, bool L2>
__global__ __launch_bounds__(kBlock) void rows_sparse_ema_kernel(float *__restrict__ w, float *__restrict__ tgt,
                                                                  float *__restrict__ m, float *__restrict__ v,
                                                                  int *__restrict__ last, int64_t n_rows, int D,
                                                                  const int *__restrict__ keys, const int64_t *__restrict__ perm,
                                                                  int64_t n, const float *__restrict__ src, int step, EmaOpt o,
                                                                  int *__restrict__ err) {
    const int lane = threadIdx.x % kWave;
    const int64_t q0 = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (q0 >= n) return;
    const int row = run_head(keys, q0, n_rows);
    if (row < 0) return;
    const int from = max(__builtin_amdgcn_readfirstlane(last[row]), 0);
    float2 k = make_float2(0.f, 0.f);
    if (ADAM) k = o.c2[step];
    for (int e0 = 0; e0 < D; e0 += kWave) {
        const int e = e0 + lane;
        const bool active = e < D;
        const int64_t at = row * (int64_t)D + e;
        float ww = 0.f, tt = 0.f, mm = 0.f, vv = 0.f;
        if (active) {
            ww = w[at]; tt = tgt[at];
            if (ADAM) { mm = m[at]; vv = v[at]; }
        }
        float g = run_sum(keys, perm, n, q0, row, src, D, e, active, lane, err);
        if (!active) continue;
        ema_replay_elem<ADAM, L2>(ww, mm, vv, tt, from, step - 1, o);
        if (ADAM) {
            adam_elem<L2>(ww, mm, vv, g, o.l2, o.b1, o.b2, o.eps, k.x, k.y);
            m[at] = mm; v[at] = vv;
        } else {
            if (L2) g = fmaf(o.l2, ww, g);              // wr_sgd_dense: g' = g + l2*w
            ww -= o.lr * g;
        }
        tt = ema_elem(tt, ww, o.mom, o.one_minus_mom);  // the target update of step `step` sees the stepped row
        w[at] = ww; tgt[at] = tt;
    }
    if (lane == 0) last[row] = step;
}

// Rows [0, n_rows) of the arrays handed in (a window: pointers offset to its first row) up to step `upto`, zero gradients.
template <bool ADAM, bool L2, int R>
__global__ __launch_bounds__(kBlock) void catchup_ema_kernel(float *__restrict__ w, float *__restrict__ tgt, float *__restrict__ m,
                                                              float *__restrict__ v, int *__restrict__ last, int64_t n_rows, int D,
                                                              int upto, EmaOpt o) {
    const int lane = threadIdx.x % kWave;
    const int64_t stride = (int64_t)gridDim.x * (kBlock / kWave) * R;
    for (int64_t r0 = ((int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave) * R; r0 < n_rows; r0 += stride) {
        int64_t rows[R];
        int from[R];
#pragma unroll
        for (int j = 0; j < R; ++j) from[j] = r0 + j < n_rows ? last[r0 + j] : upto;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            from[j] = max(__builtin_amdgcn_readfirstlane(from[j]), 0);
            rows[j] = (r0 + j < n_rows && from[j] < upto) ? r0 + j : -1;        // a current row is not touched
        }
        for (int e = lane; e < D; e += kWave) {
            float ww[R], tt[R], mm[R], vv[R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                ww[j] = tt[j] = mm[j] = vv[j] = 0.f;
                if (rows[j] < 0) continue;
                const int64_t at = rows[j] * (int64_t)D + e;
                ww[j] = w[at]; tt[j] = tgt[at];
                if (ADAM) { mm[j] = m[at]; vv[j] = v[at]; }
            }
#pragma unroll
            for (int j = 0; j < R; ++j) {
                if (rows[j] < 0) continue;
                const int64_t at = rows[j] * (int64_t)D + e;
                ema_replay_elem<ADAM, L2>(ww[j], mm[j], vv[j], tt[j], from[j], upto, o);
                if (ADAM || L2) w[at] = ww[j];
                if (ADAM) { m[at] = mm[j]; v[at] = vv[j]; }
                tgt[at] = tt[j];
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < R; ++j)
                if (rows[j] >= 0) last[rows[j]] = upto;
        }
    }
}

static inline unsigned waves_grid(int64_t n_waves) {
    const int64_t g = (n_waves + kBlock / kWave - 1) / (kBlock / kWave);
    return (unsigned)(g < 1 ? 1 : g);
}
static inline unsigned catchup_grid(int64_t n_rows, int R) {
    const int64_t per = kBlock / kWave * R;
    const int64_t g = (n_rows + per - 1) / per, cap = 256 * 32;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

static int32_t check_ema_pair(const char *entry, const void *tab, const void *tgt, const void *m, const void *v, bool adam,
                              const void *last, int64_t n_rows, int32_t D, float mom, float one_minus_mom) {
    int32_t rc;
    if ((rc = check_tables({{tab, n_rows, "tab"}, {tgt, n_rows, "target"}}, D)) != WR_OK) return rc;
    if (adam && (rc = check_tables({{m, n_rows, "exp_avg"}, {v, n_rows, "exp_avg_sq"}}, D)) != WR_OK) return rc;
    WR_REQUIRE(last != nullptr, WR_E_NULL, "%s: last_step is NULL", entry);
    WR_REQUIRE(mom >= 0.f && mom <= 1.f && one_minus_mom >= 0.f && one_minus_mom <= 1.f, WR_E_RANGE,
               "%s: momentum %g / %g outside [0, 1]", entry, (double)mom, (double)one_minus_mom);
    return WR_OK;
}

// <ADAM, L2> x R in {1, kGatherRowsPerWave}: the launches of the three pair operations
#define WR_EMA_DISPATCH(ADAM_, l2_, LAUNCH)                      \
    do {                                                         \
        if ((l2_) != 0.f) { LAUNCH(ADAM_, true); }               \
        else { LAUNCH(ADAM_, false); }                           \
    } while (0)

template <bool ADAM>
static int32_t gather_rows_ema(const float *tab, const float *tgt, const float *m, const float *v, const int32_t *last,
                               int64_t n_rows, int32_t D, const int64_t *idx, int64_t n, int64_t upto, const EmaOpt &o,
                               float *out_w, float *out_t, int32_t *err_word, hipStream_t stream) {
    const bool small = n < kSmallGather;
    const unsigned grid = waves_grid(small ? n : (n + kGatherRowsPerWave - 1) / kGatherRowsPerWave);
#define WR_LAUNCH(A_, L_)                                                                                                     \
    do {                                                                                                                      \
        if (small)                                                                                                            \
            hipLaunchKernelGGL((gather_rows_ema_kernel<A_, L_, 1>), dim3(grid), dim3(kBlock), 0, stream, tab, tgt, m, v, last, \
                               n_rows, D, idx, n, (int)upto, o, out_w, out_t, err_word);                                      \
        else                                                                                                                  \
            hipLaunchKernelGGL((gather_rows_ema_kernel<A_, L_, kGatherRowsPerWave>), dim3(grid), dim3(kBlock), 0, stream, tab, \
                               tgt, m, v, last, n_rows, D, idx, n, (int)upto, o, out_w, out_t, err_word);                     \
    } while (0)
    WR_EMA_DISPATCH(ADAM, o.l2, WR_LAUNCH);
#undef WR_LAUNCH
    WR_LAUNCH_CHECK("gather_rows_ema_kernel");
    return WR_OK;
}

template <bool ADAM>
static int32_t rows_sparse_ema(float *tab, float *tgt, float *m, float *v, int32_t *last, int64_t n_rows, int32_t D,
                               const int32_t *keys, const int64_t *perm, int64_t n, const float *src, int64_t step,
                               const EmaOpt &o, int32_t *err_word, hipStream_t stream) {
#define WR_LAUNCH(A_, L_)                                                                                                        \
    hipLaunchKernelGGL((rows_sparse_ema_kernel<A_, L_>), dim3(waves_grid(n)), dim3(kBlock), 0, stream, tab, tgt, m, v, last, n_rows, \
                       D, keys, perm, n, src, (int)step, o, err_word)
    WR_EMA_DISPATCH(ADAM, o.l2, WR_LAUNCH);
#undef WR_LAUNCH
    WR_LAUNCH_CHECK("rows_sparse_ema_kernel");
    return WR_OK;
}

template <bool ADAM>
static int32_t catchup_ema(float *tab, float *tgt, float *m, float *v, int32_t *last, int64_t n_rows, int32_t D, int64_t upto,
                           const EmaOpt &o, hipStream_t stream) {
    const bool small = n_rows < kSmallGather;       // a window of rows (bounded lag): one wave per row
#define WR_LAUNCH(A_, L_)                                                                                                       \
    do {                                                                                                                        \
        if (small)                                                                                                              \
            hipLaunchKernelGGL((catchup_ema_kernel<A_, L_, 1>), dim3(catchup_grid(n_rows, 1)), dim3(kBlock), 0, stream, tab, tgt, \
                               m, v, last, n_rows, D, (int)upto, o);                                                            \
        else                                                                                                                    \
            hipLaunchKernelGGL((catchup_ema_kernel<A_, L_, kGatherRowsPerWave>), dim3(catchup_grid(n_rows, kGatherRowsPerWave)), \
                               dim3(kBlock), 0, stream, tab, tgt, m, v, last, n_rows, D, (int)upto, o);                         \
    } while (0)
    WR_EMA_DISPATCH(ADAM, o.l2, WR_LAUNCH);
#undef WR_LAUNCH
    WR_LAUNCH_CHECK("catchup_ema_kernel");
    return WR_OK;
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

// ---- K24: the pair (online table, target table)
int32_t wr_gather_rows_ema(const float *tab, const float *target, const float *exp_avg, const float *exp_avg_sq,
                           const int32_t *last_step, int64_t n_rows, int32_t D, const int64_t *idx, int64_t n, int64_t upto,
                           const float *consts, int64_t n_consts, float l2, float beta1, float beta2, float eps, float mom,
                           float one_minus_mom, float *out_tab, float *out_target, int32_t *err_word, void *stream_) {
    int32_t rc;
    if ((rc = check_ema_pair("wr_gather_rows_ema", tab, target, exp_avg, exp_avg_sq, true, last_step, n_rows, D, mom,
                             one_minus_mom)) != WR_OK)
        return rc;
    WR_REQUIRE(consts != nullptr, WR_E_NULL, "consts is NULL");
    WR_REQUIRE(upto >= 0 && upto < n_consts && upto < INT32_MAX, WR_E_RANGE, "step %lld outside the consts table (%lld entries)",
               (long long)upto, (long long)n_consts);
    if ((rc = check_positions("wr_gather_rows_ema", idx, n)) != WR_OK) return rc;
    if (n == 0) return WR_OK;
    WR_REQUIRE(out_tab != nullptr && out_target != nullptr, WR_E_NULL, "out_tab / out_target is NULL");
    const EmaOpt o{reinterpret_cast<const float2 *>(consts), 0.f, l2, beta1, beta2, eps, mom, one_minus_mom};
    return gather_rows_ema<true>(tab, target, exp_avg, exp_avg_sq, last_step, n_rows, D, idx, n, upto, o, out_tab, out_target,
                                 err_word, reinterpret_cast<hipStream_t>(stream_));
}

int32_t wr_gather_rows_ema_sgd(const float *tab, const float *target, const int32_t *last_step, int64_t n_rows, int32_t D,
                               const int64_t *idx, int64_t n, int64_t upto, float lr, float l2, float mom, float one_minus_mom,
                               float *out_tab, float *out_target, int32_t *err_word, void *stream_) {
    int32_t rc;
    if ((rc = check_ema_pair("wr_gather_rows_ema_sgd", tab, target, nullptr, nullptr, false, last_step, n_rows, D, mom,
                             one_minus_mom)) != WR_OK)
        return rc;
    WR_REQUIRE(upto >= 0 && upto < INT32_MAX, WR_E_RANGE, "step must be >= 0");
    if ((rc = check_positions("wr_gather_rows_ema_sgd", idx, n)) != WR_OK) return rc;
    if (n == 0) return WR_OK;
    WR_REQUIRE(out_tab != nullptr && out_target != nullptr, WR_E_NULL, "out_tab / out_target is NULL");
    const EmaOpt o{nullptr, lr, l2, 0.f, 0.f, 0.f, mom, one_minus_mom};
    return gather_rows_ema<false>(tab, target, nullptr, nullptr, last_step, n_rows, D, idx, n, upto, o, out_tab, out_target,
                                  err_word, reinterpret_cast<hipStream_t>(stream_));
}

int32_t wr_adam_rows_sparse_ema(float *tab, float *target, float *exp_avg, float *exp_avg_sq, int32_t *last_step, int64_t n_rows,
                                int32_t D, const int32_t *sorted_rows, const int64_t *perm, int64_t n, const float *src,
                                int64_t adam_step, const float *consts, int64_t n_consts, float l2, float beta1, float beta2,
                                float eps, float mom, float one_minus_mom, int32_t *err_word, void *stream_) {
    int32_t rc;
    if ((rc = check_ema_pair("wr_adam_rows_sparse_ema", tab, target, exp_avg, exp_avg_sq, true, last_step, n_rows, D, mom,
                             one_minus_mom)) != WR_OK)
        return rc;
    WR_REQUIRE(consts != nullptr, WR_E_NULL, "consts is NULL");
    WR_REQUIRE(adam_step >= 1 && adam_step < n_consts && adam_step < INT32_MAX, WR_E_RANGE,
               "adam_step %lld outside the consts table (%lld entries)", (long long)adam_step, (long long)n_consts);
    if ((rc = check_positions("wr_adam_rows_sparse_ema", sorted_rows, n)) != WR_OK) return rc;
    if (n == 0) return WR_OK;
    WR_REQUIRE(perm != nullptr && src != nullptr, WR_E_NULL, "perm / src is NULL");
    const EmaOpt o{reinterpret_cast<const float2 *>(consts), 0.f, l2, beta1, beta2, eps, mom, one_minus_mom};
    return rows_sparse_ema<true>(tab, target, exp_avg, exp_avg_sq, last_step, n_rows, D, sorted_rows, perm, n, src, adam_step, o,
                                 err_word, reinterpret_cast<hipStream_t>(stream_));
}

int32_t wr_sgd_rows_sparse_ema(float *tab, float *target, int32_t *last_step, int64_t n_rows, int32_t D,
                               const int32_t *sorted_rows, const int64_t *perm, int64_t n, const float *src, int64_t step, float lr,
                               float l2, float mom, float one_minus_mom, int32_t *err_word, void *stream_) {
    int32_t rc;
    if ((rc = check_ema_pair("wr_sgd_rows_sparse_ema", tab, target, nullptr, nullptr, false, last_step, n_rows, D, mom,
                             one_minus_mom)) != WR_OK)
        return rc;
    WR_REQUIRE(step >= 1 && step < INT32_MAX, WR_E_RANGE, "step must be >= 1");
    if ((rc = check_positions("wr_sgd_rows_sparse_ema", sorted_rows, n)) != WR_OK) return rc;
    if (n == 0) return WR_OK;
    WR_REQUIRE(perm != nullptr && src != nullptr, WR_E_NULL, "perm / src is NULL");
    const EmaOpt o{nullptr, lr, l2, 0.f, 0.f, 0.f, mom, one_minus_mom};
    return rows_sparse_ema<false>(tab, target, nullptr, nullptr, last_step, n_rows, D, sorted_rows, perm, n, src, step, o, err_word,
                                  reinterpret_cast<hipStream_t>(stream_));
}

int32_t wr_adam_catchup_ema(float *tab, float *target, float *exp_avg, float *exp_avg_sq, int32_t *last_step, int64_t n_rows,
                            int32_t D, int64_t adam_step, const float *consts, int64_t n_consts, float l2, float beta1,
                            float beta2, float eps, float mom, float one_minus_mom, void *stream_) {
    int32_t rc;
    if ((rc = check_ema_pair("wr_adam_catchup_ema", tab, target, exp_avg, exp_avg_sq, true, last_step, n_rows, D, mom,
                             one_minus_mom)) != WR_OK)
        return rc;
    WR_REQUIRE(consts != nullptr, WR_E_NULL, "consts is NULL");
    WR_REQUIRE(adam_step >= 0 && adam_step < n_consts && adam_step < INT32_MAX, WR_E_RANGE,
               "adam_step %lld outside the consts table (%lld entries)", (long long)adam_step, (long long)n_consts);
    const EmaOpt o{reinterpret_cast<const float2 *>(consts), 0.f, l2, beta1, beta2, eps, mom, one_minus_mom};
    return catchup_ema<true>(tab, target, exp_avg, exp_avg_sq, last_step, n_rows, D, adam_step, o,
                             reinterpret_cast<hipStream_t>(stream_));
}

int32_t wr_sgd_catchup_ema(float *tab, float *target, int32_t *last_step, int64_t n_rows, int32_t D, int64_t step, float lr,
                           float l2, float mom, float one_minus_mom, void *stream_) {
    int32_t rc;
    if ((rc = check_ema_pair("wr_sgd_catchup_ema", tab, target, nullptr, nullptr, false, last_step, n_rows, D, mom,
                             one_minus_mom)) != WR_OK)
        return rc;
    WR_REQUIRE(step >= 0 && step < INT32_MAX, WR_E_RANGE, "step must be >= 0");
    const EmaOpt o{nullptr, lr, l2, 0.f, 0.f, 0.f, mom, one_minus_mom};
    return catchup_ema<false>(tab, target, nullptr, nullptr, last_step, n_rows, D, step, o, reinterpret_cast<hipStream_t>(stream_));
}

}  // extern "C"
