// wr_rowopt.hip — row-lazy dense optimizers for a table whose gradient rows come from autograd (K22, K24).
//
// A table that is looked up at a few thousand positions per step is still moved in all of its rows by torch.optim.Adam /
// SGD(weight_decay) at every step (reference src/helpers/BaseRunner.py:120-124,199), and the backward of every lookup builds
// a zero [n_rows, D] table first.  wr_lazy.hip removed the table passes for BPRMF, whose step kernels know the batch; here the
// same exact replay is offered to any caller that holds (index, gradient row) pairs.  last[row] = s: the row has had s steps.
//
// One kernel family <ADAM, L2, EMA> with two faces:
//   EMA = false  ONE table — the item table of a sequential model (reference src/models/sequential/SASRec.py:60,84,105-106).
//                The replay of a missed step is the optimizer step with a zero gradient.
//   EMA = true   a PAIR — BUIR's online table and the target that follows it by tgt = tgt*mom + w*(1 - mom) after every
//                optimizer step (reference src/models/general/BUIR.py:69-72).  A row that no step names still moves twice per
//                step, so the replay of a missed step is "zero-gradient step, then target update towards the row's NEW w", step
//                by step (no closed form: w changes under Adam and under weight decay); last[row] counts both together.
// and three operations:
//   * gather     out[k,:] = row idx[k] AS OF step `upto`: the wave replays the steps the row missed in registers and writes
//                only `out` (both rows of a pair).  The tables, the moments and last[] are read-only, so duplicates and
//                concurrent readers need no dedup, no atomics and no index work in the forward pass;
//   * sparse step  the step's positions in (row, position) order: one wave per run of equal rows sums the run's gradient rows
//                in position order (the association of wr_scatter_add_rows into a zero table), replays the row up to step t-1,
//                applies step t with the sum (a pair: then the target update of step t) and writes w, m, v, (tgt) and
//                last[row] = t.  No [n_rows, D] gradient exists anywhere;
//   * catch-up   the rows nobody asked for, whole or on a rotating window (bounded lag): wr_adam_catchup_all /
//                wr_sgd_catchup_all of wr_lazy.hip for one table, catchup_ema_kernel here for a pair.
// Element arithmetic and order are those of wr_adam_dense / wr_sgd_dense / wr_ema_update (adam_elem, adam_replay_elem,
// sgd_decay_elem, ema_elem of wr_common.h): after a catch-up the tables and the moments hold the bits the dense kernels
// produce from the scatter-added gradient table.
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

// The optimizer of a call, by value.  Adam reads c2, l2, b1, b2, eps; SGD lr, l2; a pair also mom, one_minus_mom.
// The gather and the sparse step take c2 once more as a __restrict__ argument of their own and replay through that: they store
// while they replay, and only a pointer known not to alias their stores is read with scalar loads (one table under Adam had
// them; through the struct it measured 3 % on the step of a 1 M-row table).  The pair's catch-up reads o.c2 as it always did:
// with scalar loads its R = 4 forms need 102 SGPRs and lose a wave of occupancy.
struct RowOpt {
    const float2 *c2;                          // Adam: {step_size, 1/sqrt(bias_correction2)} per step; SGD: unused
    float lr, l2, b1, b2, eps, mom, one_minus_mom;
};
static RowOpt adam_opt(const float *consts, float l2, float b1, float b2, float eps, float mom = 0.f, float one_minus_mom = 0.f) {
    return {reinterpret_cast<const float2 *>(consts), 0.f, l2, b1, b2, eps, mom, one_minus_mom};
}
static RowOpt sgd_opt(float lr, float l2, float mom = 0.f, float one_minus_mom = 0.f) {
    return {nullptr, lr, l2, 0.f, 0.f, 0.f, mom, one_minus_mom};
}

// Steps from+1 .. upto of one element with a zero gradient, under EMA each followed by its target update.  One table under
// Adam: adam_replay_elem itself, which wr_lazy.hip's catch-up uses; a pair fetches the constants of four steps together as it
// does.  SGD with l2 == 0: w stays — a pair's target still moves.
template <bool ADAM, bool L2, bool EMA>
__device__ __forceinline__ void replay_elem(float &w, float &m, float &v, float &t, int from, int upto,
                                            const float2 *__restrict__ c2, const RowOpt &o) {
    if (ADAM && !EMA) {
        adam_replay_elem<L2>(w, m, v, from, upto, c2, o.l2, o.b1, o.b2, o.eps);
    } else if (ADAM) {
        auto replay = [&](float2 k) {
            if (L2) adam_elem<true>(w, m, v, 0.f, o.l2, o.b1, o.b2, o.eps, k.x, k.y);
            else adam_elem_zero_grad(w, m, v, o.b1, o.b2, o.eps, k.x, k.y);
            t = ema_elem(t, w, o.mom, o.one_minus_mom);
        };
        int s = from + 1;
        for (; s + 3 <= upto; s += 4) {
            const float2 k0 = c2[s], k1 = c2[s + 1], k2 = c2[s + 2], k3 = c2[s + 3];
            replay(k0); replay(k1); replay(k2); replay(k3);
        }
        for (; s <= upto; ++s) replay(c2[s]);
    } else {
        for (int s = from; s < upto; ++s) {
            if (L2) w = sgd_decay_elem(w, o.lr, o.l2);
            if (EMA) t = ema_elem(t, w, o.mom, o.one_minus_mom);
        }
    }
}

// tgt / out_t: a pair's target (EMA) only.
template <bool ADAM, bool L2, bool EMA, int R>
__global__ __launch_bounds__(kBlock) void gather_rows_kernel(const float *__restrict__ w, const float *__restrict__ tgt,
                                                              const float *__restrict__ m, const float *__restrict__ v,
                                                              const int *__restrict__ last, int64_t n_rows, int D,
                                                              const int64_t *__restrict__ idx, int64_t n, int upto,
                                                              const float2 *__restrict__ c2, RowOpt o,
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
            if (EMA) tt[j] = tgt[at];
            if (ADAM && from[j] < upto) { mm[j] = m[at]; vv[j] = v[at]; }     // a current row needs no moments
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (k0 + j >= n) continue;
            if (rows[j] >= 0) replay_elem<ADAM, L2, EMA>(ww[j], mm[j], vv[j], tt[j], from[j], upto, c2, o);
            out_w[(k0 + j) * (int64_t)D + e] = ww[j];                         // a position outside the table: zeros
            if (EMA) out_t[(k0 + j) * (int64_t)D + e] = tt[j];
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

// A run of padding_idx (-1: none; a pair passes -1 and is not tested) contributes no gradient but takes the step: its row stays
// current.  Without
// state (SGD, l2 == 0, one table: an untouched row never moves) `last` is neither read nor written and may be NULL.
template <bool ADAM, bool L2, bool EMA>
__global__ __launch_bounds__(kBlock) void rows_sparse_kernel(float *__restrict__ w, float *__restrict__ tgt, float *__restrict__ m,
                                                              float *__restrict__ v, int *__restrict__ last, int64_t n_rows, int D,
                                                              const int *__restrict__ keys, const int64_t *__restrict__ perm,
                                                              int64_t n, const float *__restrict__ src, int64_t padding_idx,
                                                              int step, const float2 *__restrict__ c2, RowOpt o,
                                                              int *__restrict__ err) {
    constexpr bool STATE = ADAM || L2 || EMA;
    const int lane = threadIdx.x % kWave;
    const int64_t q0 = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (q0 >= n) return;
    const int row = run_head(keys, q0, n_rows);
    if (row < 0) return;
    const bool pad = !EMA && row == padding_idx;        // a pair has no padding row: no test in its forms
    if (!STATE && pad) return;                          // w - lr * 0
    const int from = STATE ? max(__builtin_amdgcn_readfirstlane(last[row]), 0) : 0;
    float2 k = make_float2(0.f, 0.f);
    if (ADAM) k = c2[step];
    for (int e0 = 0; e0 < D; e0 += kWave) {
        const int e = e0 + lane;
        const bool active = e < D;
        const int64_t at = row * (int64_t)D + e;
        float ww = 0.f, tt = 0.f, mm = 0.f, vv = 0.f;
        if (active) {
            ww = w[at];
            if (EMA) tt = tgt[at];
            if (ADAM) { mm = m[at]; vv = v[at]; }
        }
        float g = pad ? 0.f : run_sum(keys, perm, n, q0, row, src, D, e, active, lane, err);
        if (!active) continue;
        replay_elem<ADAM, L2, EMA>(ww, mm, vv, tt, from, step - 1, c2, o);
        if (ADAM) {
            adam_elem<L2>(ww, mm, vv, g, o.l2, o.b1, o.b2, o.eps, k.x, k.y);
            m[at] = mm; v[at] = vv;
        } else {
            if (L2) g = fmaf(o.l2, ww, g);              // wr_sgd_dense: g' = g + l2*w
            ww -= o.lr * g;
        }
        if (EMA) tt = ema_elem(tt, ww, o.mom, o.one_minus_mom);        // the target update of step `step` sees the stepped row
        w[at] = ww;
        if (EMA) tgt[at] = tt;
    }
    if (STATE && lane == 0) last[row] = step;
}

// A pair's catch-up: rows [0, n_rows) of the arrays handed in (a window: pointers offset to its first row) up to step `upto`,
// zero gradients.
template <bool ADAM, bool L2, int R>
__global__ __launch_bounds__(kBlock) void catchup_ema_kernel(float *__restrict__ w, float *__restrict__ tgt, float *__restrict__ m,
                                                              float *__restrict__ v, int *__restrict__ last, int64_t n_rows, int D,
                                                              int upto, RowOpt o) {
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
                replay_elem<ADAM, L2, true>(ww[j], mm[j], vv[j], tt[j], from[j], upto, o.c2, o);
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

// What every entry checks first, in this order: the tables of its face, last[], a pair's momentum, Adam's constants table,
// and that `step` lies in [first_step, n_consts) (SGD: >= first_step).
template <bool ADAM, bool EMA>
static int32_t check_state(const char *entry, const void *tab, const void *tgt, const void *m, const void *v, const void *last,
                           bool need_last, int64_t n_rows, int32_t D, const RowOpt &o, int64_t n_consts, int64_t step,
                           int64_t first_step) {
    int32_t rc;
    if ((rc = check_table(tab, n_rows, D, "tab")) != WR_OK) return rc;
    if (EMA && (rc = check_table(tgt, n_rows, D, "target")) != WR_OK) return rc;
    if (ADAM && (rc = check_tables({{m, n_rows, "exp_avg"}, {v, n_rows, "exp_avg_sq"}}, D)) != WR_OK) return rc;
    WR_REQUIRE(!need_last || last != nullptr, WR_E_NULL, "%s: last_step is NULL", entry);
    WR_REQUIRE(!EMA || (o.mom >= 0.f && o.mom <= 1.f && o.one_minus_mom >= 0.f && o.one_minus_mom <= 1.f), WR_E_RANGE,
               "%s: momentum %g / %g outside [0, 1]", entry, (double)o.mom, (double)o.one_minus_mom);
    WR_REQUIRE(!ADAM || o.c2 != nullptr, WR_E_NULL, "%s: consts is NULL", entry);
    WR_REQUIRE(step >= first_step && step < INT32_MAX && (!ADAM || step < n_consts), WR_E_RANGE,
               "%s: step %lld outside [%lld, %lld)", entry, (long long)step, (long long)first_step,
               (long long)(ADAM ? n_consts : (int64_t)INT32_MAX));
    return WR_OK;
}

static int32_t check_positions(const char *entry, const void *idx, int64_t n) {
    WR_REQUIRE(n >= 0 && n < (int64_t(1) << 31), WR_E_SHAPE, "%s: n=%lld out of range", entry, (long long)n);
    WR_REQUIRE(n == 0 || idx != nullptr, WR_E_NULL, "%s: the index array is NULL", entry);
    return WR_OK;
}

// The one place where a face <ADAM, EMA>, l2 and the size of a call pick a kernel instance: launch(Form<ADAM, L2, EMA, R>{}).
// small: one row per wave (R = 1), else kGatherRowsPerWave; the sparse step has no R and passes true.
template <bool ADAM_, bool L2_, bool EMA_, int R_>
struct Form {
    static constexpr bool ADAM = ADAM_, L2 = L2_, EMA = EMA_;
    static constexpr int R = R_;
};
template <bool ADAM, bool EMA, typename Launch>
static void for_form(bool l2, bool small, Launch &&launch) {
    if (l2) {
        if (small) launch(Form<ADAM, true, EMA, 1>{});
        else launch(Form<ADAM, true, EMA, kGatherRowsPerWave>{});
    } else {
        if (small) launch(Form<ADAM, false, EMA, 1>{});
        else launch(Form<ADAM, false, EMA, kGatherRowsPerWave>{});
    }
}

// The rest of a gather entry after check_state.  l2: whether the replay decays (SGD on one table always does, as its kernel
// always did; its <false, false, false> forms are never launched).
template <bool ADAM, bool EMA>
static int32_t gather_rows(const char *entry, const float *tab, const float *tgt, const float *m, const float *v,
                           const int32_t *last, int64_t n_rows, int32_t D, const int64_t *idx, int64_t n, int64_t upto, bool l2,
                           const RowOpt &o, float *out_w, float *out_t, int32_t *err_word, void *stream_) {
    int32_t rc;
    if ((rc = check_positions(entry, idx, n)) != WR_OK) return rc;
    if (n == 0) return WR_OK;
    WR_REQUIRE(out_w != nullptr && (!EMA || out_t != nullptr), WR_E_NULL, "%s: an output array is NULL", entry);
    for_form<ADAM, EMA>(l2, n < kSmallGather, [&](auto f) {
        using F = decltype(f);
        hipLaunchKernelGGL((gather_rows_kernel<F::ADAM, F::L2, F::EMA, F::R>), dim3(waves_grid((n + F::R - 1) / F::R)),
                           dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream_), tab, tgt, m, v, last, n_rows, D, idx, n,
                           (int)upto, o.c2, o, out_w, out_t, err_word);
    });
    WR_LAUNCH_CHECK("gather_rows_kernel");
    return WR_OK;
}

// The rest of a sparse-step entry after check_state.
template <bool ADAM, bool EMA>
static int32_t rows_sparse(const char *entry, float *tab, float *tgt, float *m, float *v, int32_t *last, int64_t n_rows, int32_t D,
                           const int32_t *keys, const int64_t *perm, int64_t n, const float *src, int64_t padding_idx,
                           int64_t step, const RowOpt &o, int32_t *err_word, void *stream_) {
    int32_t rc;
    if ((rc = check_positions(entry, keys, n)) != WR_OK) return rc;
    if (n == 0) return WR_OK;
    WR_REQUIRE(perm != nullptr && src != nullptr, WR_E_NULL, "%s: perm / src is NULL", entry);
    for_form<ADAM, EMA>(o.l2 != 0.f, true, [&](auto f) {
        using F = decltype(f);
        hipLaunchKernelGGL((rows_sparse_kernel<F::ADAM, F::L2, F::EMA>), dim3(waves_grid(n)), dim3(kBlock), 0,
                           reinterpret_cast<hipStream_t>(stream_), tab, tgt, m, v, last, n_rows, D, keys, perm, n, src,
                           padding_idx, (int)step, o.c2, o, err_word);
    });
    WR_LAUNCH_CHECK("rows_sparse_kernel");
    return WR_OK;
}

// The rest of a pair's catch-up entry after check_state.  A window of rows (bounded lag) is small: one wave per row.
template <bool ADAM>
static int32_t catchup_ema(float *tab, float *tgt, float *m, float *v, int32_t *last, int64_t n_rows, int32_t D, int64_t upto,
                           const RowOpt &o, void *stream_) {
    for_form<ADAM, true>(o.l2 != 0.f, n_rows < kSmallGather, [&](auto f) {
        using F = decltype(f);
        hipLaunchKernelGGL((catchup_ema_kernel<F::ADAM, F::L2, F::R>), dim3(catchup_grid(n_rows, F::R)), dim3(kBlock), 0,
                           reinterpret_cast<hipStream_t>(stream_), tab, tgt, m, v, last, n_rows, D, (int)upto, o);
    });
    WR_LAUNCH_CHECK("catchup_ema_kernel");
    return WR_OK;
}

}  // namespace wr

using namespace wr;

extern "C" {

// ---- one table
int32_t wr_gather_rows_lazy(const float *tab, const float *exp_avg, const float *exp_avg_sq, const int32_t *last_step,
                            int64_t n_rows, int32_t D, const int64_t *idx, int64_t n, int64_t upto, const float *consts,
                            int64_t n_consts, float l2, float beta1, float beta2, float eps, float *out, int32_t *err_word,
                            void *stream_) {
    const char *entry = "wr_gather_rows_lazy";
    const RowOpt o = adam_opt(consts, l2, beta1, beta2, eps);
    const int32_t rc = check_state<true, false>(entry, tab, nullptr, exp_avg, exp_avg_sq, last_step, true,
                                                n_rows, D, o, n_consts, upto, 0);
    if (rc != WR_OK) return rc;
    return gather_rows<true, false>(entry, tab, nullptr, exp_avg, exp_avg_sq, last_step, n_rows, D, idx, n, upto, l2 != 0.f, o, out,
                                    nullptr, err_word, stream_);
}

int32_t wr_gather_rows_lazy_sgd(const float *tab, const int32_t *last_step, int64_t n_rows, int32_t D, const int64_t *idx,
                                int64_t n, int64_t upto, float lr, float l2, float *out, int32_t *err_word, void *stream_) {
    const char *entry = "wr_gather_rows_lazy_sgd";
    const RowOpt o = sgd_opt(lr, l2);
    const int32_t rc = check_state<false, false>(entry, tab, nullptr, nullptr, nullptr, last_step, true, n_rows, D, o, 0, upto, 0);
    if (rc != WR_OK) return rc;
    return gather_rows<false, false>(entry, tab, nullptr, nullptr, nullptr, last_step, n_rows, D, idx, n, upto, true, o, out,
                                     nullptr, err_word, stream_);
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
    const char *entry = "wr_adam_rows_sparse";
    const RowOpt o = adam_opt(consts, l2, beta1, beta2, eps);
    const int32_t rc = check_state<true, false>(entry, tab, nullptr, exp_avg, exp_avg_sq, last_step, true,
                                                n_rows, D, o, n_consts, adam_step, 1);
    if (rc != WR_OK) return rc;
    return rows_sparse<true, false>(entry, tab, nullptr, exp_avg, exp_avg_sq, last_step, n_rows, D, sorted_rows, perm, n, src,
                                    padding_idx, adam_step, o, err_word, stream_);
}

int32_t wr_sgd_rows_sparse(float *tab, int32_t *last_step, int64_t n_rows, int32_t D, const int32_t *sorted_rows,
                           const int64_t *perm, int64_t n, const float *src, int64_t padding_idx, int64_t step, float lr,
                           float l2, int32_t *err_word, void *stream_) {
    const char *entry = "wr_sgd_rows_sparse";
    const RowOpt o = sgd_opt(lr, l2);
    const int32_t rc = check_state<false, false>(entry, tab, nullptr, nullptr, nullptr, last_step, l2 != 0.f,
                                                 n_rows, D, o, 0, step, 1);
    if (rc != WR_OK) return rc;
    return rows_sparse<false, false>(entry, tab, nullptr, nullptr, nullptr, last_step, n_rows, D, sorted_rows, perm, n, src,
                                     padding_idx, step, o, err_word, stream_);
}

// ---- a pair (online table, target table): no padding row
int32_t wr_gather_rows_ema(const float *tab, const float *target, const float *exp_avg, const float *exp_avg_sq,
                           const int32_t *last_step, int64_t n_rows, int32_t D, const int64_t *idx, int64_t n, int64_t upto,
                           const float *consts, int64_t n_consts, float l2, float beta1, float beta2, float eps, float mom,
                           float one_minus_mom, float *out_tab, float *out_target, int32_t *err_word, void *stream_) {
    const char *entry = "wr_gather_rows_ema";
    const RowOpt o = adam_opt(consts, l2, beta1, beta2, eps, mom, one_minus_mom);
    const int32_t rc = check_state<true, true>(entry, tab, target, exp_avg, exp_avg_sq, last_step, true,
                                               n_rows, D, o, n_consts, upto, 0);
    if (rc != WR_OK) return rc;
    return gather_rows<true, true>(entry, tab, target, exp_avg, exp_avg_sq, last_step, n_rows, D, idx, n, upto, l2 != 0.f, o,
                                   out_tab, out_target, err_word, stream_);
}

int32_t wr_gather_rows_ema_sgd(const float *tab, const float *target, const int32_t *last_step, int64_t n_rows, int32_t D,
                               const int64_t *idx, int64_t n, int64_t upto, float lr, float l2, float mom, float one_minus_mom,
                               float *out_tab, float *out_target, int32_t *err_word, void *stream_) {
    const char *entry = "wr_gather_rows_ema_sgd";
    const RowOpt o = sgd_opt(lr, l2, mom, one_minus_mom);
    const int32_t rc = check_state<false, true>(entry, tab, target, nullptr, nullptr, last_step, true, n_rows, D, o, 0, upto, 0);
    if (rc != WR_OK) return rc;
    return gather_rows<false, true>(entry, tab, target, nullptr, nullptr, last_step, n_rows, D, idx, n, upto, l2 != 0.f, o, out_tab,
                                    out_target, err_word, stream_);
}

int32_t wr_adam_rows_sparse_ema(float *tab, float *target, float *exp_avg, float *exp_avg_sq, int32_t *last_step, int64_t n_rows,
                                int32_t D, const int32_t *sorted_rows, const int64_t *perm, int64_t n, const float *src,
                                int64_t adam_step, const float *consts, int64_t n_consts, float l2, float beta1, float beta2,
                                float eps, float mom, float one_minus_mom, int32_t *err_word, void *stream_) {
    const char *entry = "wr_adam_rows_sparse_ema";
    const RowOpt o = adam_opt(consts, l2, beta1, beta2, eps, mom, one_minus_mom);
    const int32_t rc = check_state<true, true>(entry, tab, target, exp_avg, exp_avg_sq, last_step, true,
                                               n_rows, D, o, n_consts, adam_step, 1);
    if (rc != WR_OK) return rc;
    return rows_sparse<true, true>(entry, tab, target, exp_avg, exp_avg_sq, last_step, n_rows, D, sorted_rows, perm, n, src, -1,
                                   adam_step, o, err_word, stream_);
}

int32_t wr_sgd_rows_sparse_ema(float *tab, float *target, int32_t *last_step, int64_t n_rows, int32_t D,
                               const int32_t *sorted_rows, const int64_t *perm, int64_t n, const float *src, int64_t step, float lr,
                               float l2, float mom, float one_minus_mom, int32_t *err_word, void *stream_) {
    const char *entry = "wr_sgd_rows_sparse_ema";
    const RowOpt o = sgd_opt(lr, l2, mom, one_minus_mom);
    const int32_t rc = check_state<false, true>(entry, tab, target, nullptr, nullptr, last_step, true, n_rows, D, o, 0, step, 1);
    if (rc != WR_OK) return rc;
    return rows_sparse<false, true>(entry, tab, target, nullptr, nullptr, last_step, n_rows, D, sorted_rows, perm, n, src, -1, step,
                                    o, err_word, stream_);
}

int32_t wr_adam_catchup_ema(float *tab, float *target, float *exp_avg, float *exp_avg_sq, int32_t *last_step, int64_t n_rows,
                            int32_t D, int64_t adam_step, const float *consts, int64_t n_consts, float l2, float beta1,
                            float beta2, float eps, float mom, float one_minus_mom, void *stream_) {
    const RowOpt o = adam_opt(consts, l2, beta1, beta2, eps, mom, one_minus_mom);
    const int32_t rc = check_state<true, true>("wr_adam_catchup_ema", tab, target, exp_avg, exp_avg_sq, last_step, true,
                                               n_rows, D, o,
                                               n_consts, adam_step, 0);
    if (rc != WR_OK) return rc;
    return catchup_ema<true>(tab, target, exp_avg, exp_avg_sq, last_step, n_rows, D, adam_step, o, stream_);
}

int32_t wr_sgd_catchup_ema(float *tab, float *target, int32_t *last_step, int64_t n_rows, int32_t D, int64_t step, float lr,
                           float l2, float mom, float one_minus_mom, void *stream_) {
    const RowOpt o = sgd_opt(lr, l2, mom, one_minus_mom);
    const int32_t rc = check_state<false, true>("wr_sgd_catchup_ema", tab, target, nullptr, nullptr, last_step, true,
                                                n_rows, D, o, 0,
                                                step, 0);
    if (rc != WR_OK) return rc;
    return catchup_ema<false>(tab, target, nullptr, nullptr, last_step, n_rows, D, step, o, stream_);
}

}  // extern "C"
