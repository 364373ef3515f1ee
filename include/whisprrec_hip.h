/*
 * whisprrec_hip.h — C-ABI of libwhisprrec_hip.so: the MI355X (gfx950) implementation of WhisprRec's
 * embedding-CF training hot path.
 *
 * The reference (HeyWeCome/WhisprRec) is pure Python and has no FFI; its "operator boundary" for this
 * path is the chain of PyTorch calls cited per entry point below (paths relative to the reference
 * root).  A maintainer binds this library with ctypes (INTEGRATION.md shows the stub); every symbol is
 * plain C: raw device pointers, sizes, a hipStream_t passed as void*.
 *
 * Conventions
 *   - return value: 0 = ok, <0 = argument error (WR_E_*), >0 = hipError_t of the failing HIP call.
 *     wr_last_error() returns a thread-local, human-readable message for the last non-zero return.
 *   - ownership: every table / index / output / workspace buffer is allocated and owned by the caller
 *     (e.g. a PyTorch-ROCm tensor, passed as tensor.data_ptr()).  The library allocates nothing.
 *   - asynchrony: every call only enqueues work on `stream` (hipStream_t; NULL = default stream) and
 *     returns; no call synchronises the device.  Calls on one stream execute in order.
 *   - tables are row-major fp32 [n_rows, D], rows contiguous (row stride = D floats), 16-byte aligned
 *     base.  D must be a multiple of 4 and <= 1024.
 *   - indices at the reference boundary are int64 (src/models/BaseModel.py:121); the sorted "plan"
 *     arrays produced and consumed inside the library are int32.
 *   - semantics are batch-synchronous: every gradient of a step is computed from the pre-step tables
 *     (src/helpers/BaseRunner.py:197-199), duplicates inside a batch are summed, and results do not
 *     depend on scheduling (no float atomics: bitwise reproducible run to run).
 */
#ifndef WHISPRREC_HIP_H
#define WHISPRREC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WR_ABI_VERSION 1

#define WR_OK 0
#define WR_E_NULL (-1)     /* required pointer is NULL            */
#define WR_E_SHAPE (-2)    /* bad size / D / batch                */
#define WR_E_WORKSPACE (-3)/* workspace too small                 */
#define WR_E_ALIGN (-4)    /* pointer not 16-byte aligned         */
#define WR_E_RANGE (-5)    /* value out of supported range        */

int32_t wr_abi_version(void);
const char *wr_last_error(void);
/* number of CUs, wavefront size and gcnArchName of the current device (sanity: expects gfx950) */
int32_t wr_device_info(int32_t *n_cu, int32_t *wave_size, char *arch, int32_t arch_len);

/* ---------------------------------------------------------------------------------------------------
 * K1-K3  BPRMF.predict forward  — src/models/general/BPRMF.py:69-80, src/utils/loss.py:37-39
 *   pos[b] = <U[u_b], I[p_b]>, neg[b] = <U[u_b], I[n_b]>, loss = -mean(log(1e-10 + sigmoid(pos-neg)))
 *   coef[b] = dloss/dpos[b]  (what loss.backward(), BaseRunner.py:198, feeds the three gathers)
 * pos_score / neg_score / coef may be NULL.  loss: 1 float on device.
 * workspace: >= wr_bpr_fwd_workspace_bytes(B) bytes.
 * Also serves LightGCN.predict (LightGCN.py:156-163) and SASRec.predict (SASRec.py:105-111) on
 * propagated / encoded rows: `user_tab` is then any [n_users, D] fp32 matrix.
 * --------------------------------------------------------------------------------------------------- */
int64_t wr_bpr_fwd_workspace_bytes(int64_t B);
int32_t wr_bpr_fwd(const float *user_tab, int64_t n_users, const float *item_tab, int64_t n_items, int32_t D,
                   const int64_t *u, const int64_t *p, const int64_t *n, int64_t B, float *pos_score, float *neg_score,
                   float *coef, float *loss, void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Batch plan — the on-device counterpart of DataLoader batching (BaseRunner.py:188-193) +
 * collate_batch (BaseModel.py:96-127) for the fused step: for each consecutive batch of `batch_size`
 * triplets (last one may be short, no drop_last — BaseRunner.py:201), triplets are stably sorted by
 * user and the 2*B (item, source) occurrences are stably sorted by item, so that each table row of a
 * step has exactly one owner.
 *   tu,tp,tn [n]  : triplets of batch k at [k*batch_size, ...), sorted by user; bit 31 of tp[t] / tn[t] is
 *                   set when that item row has more than one occurrence in the batch (row = low 31 bits)
 *   torig    [n]  : original position (0..n) of each sorted triplet (may be NULL)
 *   oc_item  [2n] : occurrences of batch k at [2*k*batch_size, ...), sorted by item row
 *   oc_src   [2n] : (local sorted triplet index << 1) | (1 if the occurrence is the NEGATIVE item)
 * Index inputs are int64 (reference layout) or int32.  Every index is range-checked on device against
 * n_users / n_items; *err_flag (int32 on device, caller-zeroed) is set to 1 on violation.
 * --------------------------------------------------------------------------------------------------- */
int64_t wr_bprmf_plan_workspace_bytes(int64_t n_triplets, int64_t batch_size, int64_t n_users, int64_t n_items);
int32_t wr_bprmf_plan_build_i64(const int64_t *u, const int64_t *p, const int64_t *n, int64_t n_triplets,
                                int64_t batch_size, int64_t n_users, int64_t n_items, int32_t *tu, int32_t *tp,
                                int32_t *tn, int32_t *torig, int32_t *oc_item, int32_t *oc_src, int32_t *err_flag,
                                void *workspace, int64_t workspace_bytes, void *stream);
int32_t wr_bprmf_plan_build_i32(const int32_t *u, const int32_t *p, const int32_t *n, int64_t n_triplets,
                                int64_t batch_size, int64_t n_users, int64_t n_items, int32_t *tu, int32_t *tp,
                                int32_t *tn, int32_t *torig, int32_t *oc_item, int32_t *oc_src, int32_t *err_flag,
                                void *workspace, int64_t workspace_bytes, void *stream);

/* Small batches (batch_size <= wr_bprmf_plan_small_max_batch() = 4,096; the reference's default is 2,048): the plan of a
 * batch is built by ONE workgroup in LDS, one launch for all batches, no workspace, nothing to read back but err_flag — the
 * builder of the LightGCN step (a plan per optimizer step, hipGraph-capturable).  Tables small enough for one LDS counter
 * per row (8 * max(n_users, n_items) + 16 * P bytes <= 128 KB, P = batch size rounded up to a power of two: ml-scale) take a
 * counting sort (count, scan, scatter, order every row's segment by position); the others two bitonic sorts of unique
 * composites.  Either way the arrays are wr_bprmf_plan_build_*'s, bit for bit.  WR_PLAN_SMALL=bitonic in the environment
 * keeps the sorting form (A/B runs). */
int64_t wr_bprmf_plan_small_max_batch(void);
int32_t wr_bprmf_plan_build_small_i64(const int64_t *u, const int64_t *p, const int64_t *n, int64_t n_triplets,
                                      int64_t batch_size, int64_t n_users, int64_t n_items, int32_t *tu, int32_t *tp,
                                      int32_t *tn, int32_t *torig, int32_t *oc_item, int32_t *oc_src, int32_t *err_flag,
                                      void *stream);
int32_t wr_bprmf_plan_build_small_i32(const int32_t *u, const int32_t *p, const int32_t *n, int64_t n_triplets,
                                      int64_t batch_size, int64_t n_users, int64_t n_items, int32_t *tu, int32_t *tp,
                                      int32_t *tn, int32_t *torig, int32_t *oc_item, int32_t *oc_src, int32_t *err_flag,
                                      void *stream);

/* Hand-written builder producing bit-identical plan arrays: bucket scatter + per-bucket LDS bitonic sort (one HBM
 * round trip per pair instead of the radix sort's four).  Applies when wr_bprmf_plan_fast_workspace_bytes(...) > 0
 * (batch sizes up to ~1 M, any table size).  flags: int32[2] on device, caller-zeroed; flags[0] = index out of range (as err_flag
 * above), flags[1] = a bucket overflowed (heavily skewed ids) -> the plan is INVALID and the caller must rebuild it
 * with wr_bprmf_plan_build_*.  Asynchronous like every other call; the caller reads the flags after the stream work. */
int64_t wr_bprmf_plan_fast_workspace_bytes(int64_t n_triplets, int64_t batch_size, int64_t n_users, int64_t n_items);
int32_t wr_bprmf_plan_build_fast_i64(const int64_t *u, const int64_t *p, const int64_t *n, int64_t n_triplets,
                                     int64_t batch_size, int64_t n_users, int64_t n_items, int32_t *tu, int32_t *tp,
                                     int32_t *tn, int32_t *torig, int32_t *oc_item, int32_t *oc_src, int32_t *flags,
                                     void *workspace, int64_t workspace_bytes, void *stream);
int32_t wr_bprmf_plan_build_fast_i32(const int32_t *u, const int32_t *p, const int32_t *n, int64_t n_triplets,
                                     int64_t batch_size, int64_t n_users, int64_t n_items, int32_t *tu, int32_t *tp,
                                     int32_t *tn, int32_t *torig, int32_t *oc_item, int32_t *oc_src, int32_t *flags,
                                     void *workspace, int64_t workspace_bytes, void *stream);

/* wr_bprmf_plan_build_fast_* that also writes, per batch, the bitmap "item row has several occurrences in the batch"
 * (bitmap [n_batches * ceil(n_items/32)], zeroed and filled here): the workgroup that sorts a bucket of item rows owns the
 * bucket's bitmap words, so no global atomics are needed (wr_bprmf_plan_overlap_marks spends one per such occurrence).
 * Applies to equal-width buckets spanning whole bitmap words: wr_bprmf_plan_fast_marks_supported() == 1 (WR_E_RANGE
 * otherwise).  After a bucket overflow (flags[1]) the bitmap is as incomplete as the plan. */
int32_t wr_bprmf_plan_fast_marks_supported(int64_t n_triplets, int64_t batch_size, int64_t n_users, int64_t n_items);
int32_t wr_bprmf_plan_build_fast_marks_i64(const int64_t *u, const int64_t *p, const int64_t *n, int64_t n_triplets,
                                           int64_t batch_size, int64_t n_users, int64_t n_items, int32_t *tu, int32_t *tp,
                                           int32_t *tn, int32_t *torig, int32_t *oc_item, int32_t *oc_src, int32_t *flags,
                                           void *workspace, int64_t workspace_bytes, int32_t *bitmap, void *stream);
int32_t wr_bprmf_plan_build_fast_marks_i32(const int32_t *u, const int32_t *p, const int32_t *n, int64_t n_triplets,
                                           int64_t batch_size, int64_t n_users, int64_t n_items, int32_t *tu, int32_t *tp,
                                           int32_t *tn, int32_t *torig, int32_t *oc_item, int32_t *oc_src, int32_t *flags,
                                           void *workspace, int64_t workspace_bytes, int32_t *bitmap, void *stream);

/* Bucket map for the hand-written plan builder on skewed ids.  The builder's first stage appends every triplet (item
 * occurrence) to a (batch, row-range) bucket of FIXED capacity (twice the mean load + 64).  Without a map the ranges have
 * equal width, and popularity-skewed ids overflow them (flags[1], rebuild with wr_bprmf_plan_build_*).  A map makes the
 * ranges equal in expected LOAD instead: row_bucket[row] & 0xffff is the bucket of the row (buckets ascend with the rows,
 * so the plan arrays are the same, bit for bit); a row heavy enough to fill a bucket on its own owns row_bucket[row] >> 16
 * consecutive sub-buckets that split its occurrences by position in the batch.  Per bucket: first row, number of rows,
 * and for the sub-buckets of a heavy row (index among them) | (their number << 16), else 0.  All arrays on the device.
 * whisprrec_amd/hip_ops.py (BucketMap) derives a map from an epoch's id columns; either side may be NULL (equal widths). */
typedef struct wr_bucket_side {
    int32_t n_buckets;             /* 1..1024 */
    const int32_t *row_bucket;     /* [n_rows] */
    const int32_t *bucket_start;   /* [n_buckets] */
    const int32_t *bucket_rows;    /* [n_buckets] */
    const int32_t *bucket_sub;     /* [n_buckets] */
} wr_bucket_side;

int64_t wr_bprmf_plan_fast_mapped_workspace_bytes(int64_t n_triplets, int64_t batch_size, int64_t n_users, int64_t n_items,
                                                  int32_t n_buckets_users, int32_t n_buckets_items);
int32_t wr_bprmf_plan_build_fast_mapped_i64(const int64_t *u, const int64_t *p, const int64_t *n, int64_t n_triplets,
                                            int64_t batch_size, int64_t n_users, int64_t n_items,
                                            const wr_bucket_side *map_users, const wr_bucket_side *map_items, int32_t *tu,
                                            int32_t *tp, int32_t *tn, int32_t *torig, int32_t *oc_item, int32_t *oc_src,
                                            int32_t *flags, void *workspace, int64_t workspace_bytes, void *stream);
int32_t wr_bprmf_plan_build_fast_mapped_i32(const int32_t *u, const int32_t *p, const int32_t *n, int64_t n_triplets,
                                            int64_t batch_size, int64_t n_users, int64_t n_items,
                                            const wr_bucket_side *map_users, const wr_bucket_side *map_items, int32_t *tu,
                                            int32_t *tp, int32_t *tn, int32_t *torig, int32_t *oc_item, int32_t *oc_src,
                                            int32_t *flags, void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Epoch preparation on the device — GeneralModel.Dataset.actions_before_epoch (src/models/BaseModel.py:167-177):
 * one negative per training row, uniform over [1, n_items) (item 0 is never drawn, :168), redrawn while it is in the
 * user's train set (:172-174).  clicked_ptr int64 [n_users+1] / clicked_idx int32 (ascending per user) is the CSR of
 * train_clicked_set.  Counter-based generator keyed by (seed, epoch, row, attempt): rows are independent, the result
 * is reproducible and equals oracle.sample_negatives_counter bit for bit; it is NOT NumPy's MT19937 stream (the
 * bit-exact NumPy sampler stays available on the host for small-scale parity).  err_flag (int32, device, caller-
 * zeroed): 1 = user id out of range, 2 = some user has clicked every item.
 * --------------------------------------------------------------------------------------------------- */
int32_t wr_sample_negatives_i64(const int64_t *users, int64_t n, int64_t n_users, int64_t n_items, const int64_t *clicked_ptr,
                                const int32_t *clicked_idx, uint64_t seed, uint64_t epoch, int64_t *neg_items,
                                int32_t *err_flag, void *stream);
int32_t wr_sample_negatives_i32(const int32_t *users, int64_t n, int64_t n_users, int64_t n_items, const int64_t *clicked_ptr,
                                const int32_t *clicked_idx, uint64_t seed, uint64_t epoch, int32_t *neg_items,
                                int32_t *err_flag, void *stream);

/* Sampler and shuffle fused, for a RANGE [first, first + count) of the epoch's output rows (batch order): output row i takes
 * source row j = perm(i) of (users, items) and the negative wr_sample_negatives draws for row j — bit for bit the columns of
 * wr_sample_negatives followed by wr_epoch_shuffle (same seed, epoch), no intermediate array.  out_* [count] receive rows
 * first.. (the caller passes pointers to that position); order_out [count] (may be NULL) the source rows.  The step stream
 * prepares plan chunk c+1's rows this way beside chunk c's steps (hip_ops.PipelinedSgd, `prep`). */
int32_t wr_epoch_prepare_range_i64(const int64_t *users, const int64_t *items, int64_t n, int64_t n_users, int64_t n_items,
                                   const int64_t *clicked_ptr, const int32_t *clicked_idx, uint64_t seed, uint64_t epoch,
                                   int64_t first, int64_t count, int64_t *out_users, int64_t *out_pos, int64_t *out_neg,
                                   int64_t *order_out, int32_t *err_flag, void *stream);
int32_t wr_epoch_prepare_range_i32(const int32_t *users, const int32_t *items, int64_t n, int64_t n_users, int64_t n_items,
                                   const int64_t *clicked_ptr, const int32_t *clicked_idx, uint64_t seed, uint64_t epoch,
                                   int64_t first, int64_t count, int32_t *out_users, int32_t *out_pos, int32_t *out_neg,
                                   int64_t *order_out, int32_t *err_flag, void *stream);

/* The same membership test — "has this user clicked this item" (BaseModel.py:172-174) — against a HASH SET of the (user, item)
 * pairs instead of the per-user lists: open addressing with linear probing over 64-bit keys (user << 32 | item), capacity a
 * power of two, at most a third full.  One test then reads one random 64-byte sector where the binary search reads ~7: the
 * sampler is bound by that traffic at 100 M rows.  Same answers, hence the same negatives, bit for bit.
 *   wr_pairset_capacity(n_pairs)  -> entries (uint64 each) the table needs;
 *   wr_pairset_build              fills `table` [capacity] from the clicked lists (once per training frame);
 *                                 err_flag (may be NULL) is set to 3 if the table was too small;
 *   wr_sample_negatives_set_*, wr_epoch_prepare_range_set_*   the two entry points above with the set in place of the lists. */
int64_t wr_pairset_capacity(int64_t n_pairs);
int32_t wr_pairset_build(const int64_t *clicked_ptr, const int32_t *clicked_idx, int64_t n_users, uint64_t *table,
                         int64_t capacity, int32_t *err_flag, void *stream);
int32_t wr_sample_negatives_set_i64(const int64_t *users, int64_t n, int64_t n_users, int64_t n_items, const uint64_t *pair_table,
                                    int64_t pair_capacity, uint64_t seed, uint64_t epoch, int64_t *neg_items,
                                    int32_t *err_flag, void *stream);
int32_t wr_sample_negatives_set_i32(const int32_t *users, int64_t n, int64_t n_users, int64_t n_items, const uint64_t *pair_table,
                                    int64_t pair_capacity, uint64_t seed, uint64_t epoch, int32_t *neg_items,
                                    int32_t *err_flag, void *stream);
int32_t wr_epoch_prepare_range_set_i64(const int64_t *users, const int64_t *items, int64_t n, int64_t n_users, int64_t n_items,
                                       const uint64_t *pair_table, int64_t pair_capacity, uint64_t seed, uint64_t epoch,
                                       int64_t first, int64_t count, int64_t *out_users, int64_t *out_pos, int64_t *out_neg,
                                       int64_t *order_out, int32_t *err_flag, void *stream);
int32_t wr_epoch_prepare_range_set_i32(const int32_t *users, const int32_t *items, int64_t n, int64_t n_users, int64_t n_items,
                                       const uint64_t *pair_table, int64_t pair_capacity, uint64_t seed, uint64_t epoch,
                                       int64_t first, int64_t count, int32_t *out_users, int32_t *out_pos, int32_t *out_neg,
                                       int64_t *order_out, int32_t *err_flag, void *stream);

/* wr_epoch_prepare_range_set_* with the source rows PACKED, one 8-byte word (user << 32) | item per interaction (built once
 * per training frame): one random memory sector per output row for the source instead of two — the kernel is bound by its
 * random sectors (source row + membership probe).  Same columns, bit for bit. */
int32_t wr_epoch_prepare_range_packed_i64(const uint64_t *packed_rows, int64_t n, int64_t n_users, int64_t n_items,
                                          const uint64_t *pair_table, int64_t pair_capacity, uint64_t seed, uint64_t epoch,
                                          int64_t first, int64_t count, int64_t *out_users, int64_t *out_pos, int64_t *out_neg,
                                          int64_t *order_out, int32_t *err_flag, void *stream);
int32_t wr_epoch_prepare_range_packed_i32(const uint64_t *packed_rows, int64_t n, int64_t n_users, int64_t n_items,
                                          const uint64_t *pair_table, int64_t pair_capacity, uint64_t seed, uint64_t epoch,
                                          int64_t first, int64_t count, int32_t *out_users, int32_t *out_pos, int32_t *out_neg,
                                          int64_t *order_out, int32_t *err_flag, void *stream);

/* Epoch shuffle on the device — the row order DataLoader(shuffle=True) gives an epoch (src/helpers/BaseRunner.py:188-193):
 * out_k[i] = col_k[perm(i)] for up to three index columns (NULL pairs are skipped), order_out[i] = perm(i) if not NULL.
 * perm is a keyed bijection of [0, n) evaluated per row (alternating Feistel network on ceil(log2 n) bits, splitmix64
 * round function keyed by (seed, epoch), cycle walking): no sort and no order array are needed.  Reproducible, equal to
 * oracle.epoch_permutation bit for bit; NOT the reference's torch.randperm stream (the bit-exact host path stays
 * available, whisprrec_amd/runner.py epoch_order).  Outputs must not alias inputs. */
int32_t wr_epoch_shuffle_i64(const int64_t *col0, const int64_t *col1, const int64_t *col2, int64_t n, uint64_t seed,
                             uint64_t epoch, int64_t *out0, int64_t *out1, int64_t *out2, int64_t *order_out, void *stream);
int32_t wr_epoch_shuffle_i32(const int32_t *col0, const int32_t *col1, const int32_t *col2, int64_t n, uint64_t seed,
                             uint64_t epoch, int32_t *out0, int32_t *out1, int32_t *out2, int64_t *order_out, void *stream);

/* Long runs ("hot rows": a table row with more than 32 occurrences in one batch, e.g. power-law ids).  Optional second
 * part of a plan: every such run is cut into pieces of at most 256 positions so that the step can work on a hot row with
 * many workgroups instead of one 16-lane team (still in a fixed order: reproducible).  Two sides: kind 0 = item rows (runs of
 * oc_item, 2*B positions per batch), kind 1 = user rows (runs of tu, B positions per batch).  Arrays are per batch with the
 * capacities of wr_bprmf_hot_caps(batch_size, kind): piece_q/piece_len [n_batches*cap_pieces] (start inside the batch,
 * length), run_q/run_first/run_np [n_batches*cap_runs] (head position, first piece, piece count).  counts: int32
 * [n_batches*4] on the DEVICE, caller-zeroed: item pieces, item runs, user pieces, user runs per batch.  The caller copies
 * `counts` to the host (it sizes the extra launches) and hands everything to the step calls through wr_hot_runs (NULL = none:
 * long runs are then walked sequentially by one team — correct, but slow on skewed data). */
typedef struct wr_hot_runs {
    const int32_t *piece_q, *piece_len, *run_q, *run_first, *run_np;             /* device, item side */
    const int32_t *u_piece_q, *u_piece_len, *u_run_q, *u_run_first, *u_run_np;   /* device, user side */
    const int32_t *counts_host;                                                   /* HOST, 4 per batch */
    int64_t cap_pieces, cap_runs, cap_u_pieces, cap_u_runs;
} wr_hot_runs;
void wr_bprmf_hot_caps(int64_t batch_size, int32_t kind, int64_t *cap_pieces, int64_t *cap_runs);
int32_t wr_bprmf_plan_hot_runs(const int32_t *keys, int32_t kind, int64_t n_triplets, int64_t batch_size, int32_t *piece_q,
                               int32_t *piece_len, int32_t *run_q, int32_t *run_first, int32_t *run_np, int32_t *counts,
                               void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K1-K5 fused  One BaseRunner.fit iteration for BPRMF with torch.optim.SGD —
 *   zero_grad -> predict -> backward -> step  (BaseRunner.py:196-199, optimizer per :120-124)
 * Two kernels: (A) one 16-lane team per user row: gathers U[u], I[p], I[n], BPR loss + coefficient,
 * user-row gradient reduced over the user's triplets, U[u] updated in place, c_b*U[u] stashed;
 * (B) one team per item row: sums the stashed contributions of its occurrences, I[r] updated in place.
 *   w <- w - lr * (g + l2*w)  for rows in the batch.  Rows NOT in the batch are not touched here: with
 *   l2 != 0 call wr_sgd_decay_untouched afterwards (dense torch.optim.SGD weight_decay semantics).
 * stamp_u / stamp_i (int32 [n_rows], may be NULL when l2 == 0): set to step_id for rows in the batch.
 * loss_out: 1 float on device (may be NULL).  workspace >= wr_bprmf_step_workspace_bytes(B, D).
 * --------------------------------------------------------------------------------------------------- */
int64_t wr_bprmf_step_workspace_bytes(int64_t B, int32_t D);
int32_t wr_bprmf_step_sgd(float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D,
                          const int32_t *tu, const int32_t *tp, const int32_t *tn, const int32_t *oc_item,
                          const int32_t *oc_src, int64_t B, float lr, float l2, int32_t *stamp_u, int32_t *stamp_i,
                          int32_t step_id, float *loss_out, const wr_hot_runs *hot, void *workspace,
                          int64_t workspace_bytes, void *stream);

/* Runs consecutive steps over batches [first_batch, first_batch + n_batches) of a plan built with
 * `batch_size` over `n_triplets` triplets (the native inner loop of BaseRunner.fit, BaseRunner.py:194-200).
 * loss_out[k] receives the loss of batch first_batch + k (may be NULL).  l2 must be 0 here.
 * phase_events (may be NULL): 4*n_batches hipEvent_t handles, any of them NULL (per-kernel timing).  For step k, events
 * 4k / 4k+1 are attached to the first / last kernel of the user phase as that dispatch's start / stop event, 4k+2 / 4k+3
 * likewise for the item phase: they carry the kernels' own timestamps (what rocprofv3 --kernel-trace reports) and no
 * marker packet is queued.  elapsed(4k, 4k+1) is the user phase of step k, elapsed(4k+1, 4k+3) launch to launch. */
int32_t wr_bprmf_run_sgd(float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D,
                         const int32_t *tu, const int32_t *tp, const int32_t *tn, const int32_t *oc_item,
                         const int32_t *oc_src, int64_t n_triplets, int64_t batch_size, int64_t first_batch,
                         int64_t n_batches, float lr, float *loss_out, void *const *phase_events, const wr_hot_runs *hot,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* Chained step stream — the same consecutive steps as wr_bprmf_run_sgd (BaseRunner.py:194-200, l2 = 0, no hot rows) with
 * ONE launch per step on ONE stream: the item phase of step k-1 rides, as extra workgroups, in the launch that carries the
 * user phase of step k.  The runs of batch k that read an item row that item phase rewrites (the plan's deferred runs,
 * wr_bprmf_plan_overlap_marks) are taken by a few workgroups that first wait, inside the launch, for a counter the item
 * workgroups add to after their (write-through) row stores; every other run needs no ordering.  Every table row keeps one
 * writer per step and its summation order: tables bit-identical to wr_bprmf_run_sgd's; the loss of a step differs by the
 * association of its partial sums only (fixed by the plan, bitwise reproducible).
 *   tdef  [n_batches_of_plan * ceil(batch_size/32)] : per batch, bit t%32 of word t/32 = the run headed at sorted position
 *         t is deferred;  def_q [n_batches_of_plan * def_cap] : those positions, ascending;
 *   def_count_host (HOST memory, one int32 per batch of the plan) : their number.  A step whose batch has more than
 *         min(def_cap, def_limit) deferred runs (small item tables: almost every run) is issued as the two ordinary
 *         launches; the first step of a call always is, and the call ends with an ordinary item-phase launch — on return
 *         the stream holds complete steps only.
 *   phase_events (may be NULL): 4 handles per step as for wr_bprmf_run_sgd; [4k], [4k+1] are attached to the launch that
 *         carries the user phase of step k, [4k+2], [4k+3] to a separate item-phase launch of step k where there is one.
 *   workspace >= 2 * wr_bprmf_step_workspace_bytes(batch_size, D).
 *   sync: wr_bprmf_chain_sync_words(n_batches) int32 words of device memory, 16-byte aligned, owned by the caller: one
 *         (sharded) counter per step from word 0 (zeroed by the call) and, at word sync_words - 4, a sticky word the kernels set when a
 *         bounded wait expired (zero it once when allocating; non-zero afterwards = the run is invalid).
 * Rows must be whole 128-byte lines: D % 32 == 0 and both tables 128-byte aligned (wr_bprmf_chain_supported; WR_E_ALIGN). */
int32_t wr_bprmf_chain_supported(const float *user_tab, const float *item_tab, int32_t D);
int64_t wr_bprmf_chain_sync_words(int64_t n_batches);
int32_t wr_bprmf_run_sgd_chain(float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D,
                               const int32_t *tu, const int32_t *tp, const int32_t *tn, const int32_t *oc_item,
                               const int32_t *oc_src, int64_t n_triplets, int64_t batch_size, int64_t first_batch,
                               int64_t n_batches, float lr, float *loss_out, const int32_t *tdef, const int32_t *def_q,
                               const int32_t *def_count_host, int64_t def_cap, int64_t def_limit, void *const *phase_events,
                               void *workspace, int64_t workspace_bytes, int32_t *sync, int64_t sync_words, void *stream);

/* Step stream WITHOUT a per-batch sort (wr_group.hip) — the same consecutive steps as wr_bprmf_run_sgd
 * (src/helpers/BaseRunner.py:194-200: zero_grad / predict / backward / SGD.step per batch, l2 = 0), one launch per step.
 * The reference loop does no per-batch index work; neither does this path beyond GROUPING what recurs in a batch:
 *   wr_group_plan_build    leaves the triplets (u, p, n: int32, batch order) where they are and writes, per batch, four
 *       flag bits per triplet (user shared in the batch / positive item shared / negative item shared / an item row is
 *       rewritten by the batch before) and the shared occurrences only, sorted by (row, position), as lists.  `plan` holds
 *       wr_group_plan_words(...) int32 words (0: shape not supported — batch_size > 131,072), 16-byte aligned, caller-owned.
 *       plan[0] != 0: an id was out of range (nn.Embedding would raise IndexError); plan[1] != 0: a list overflowed
 *       (tables small against the batch, or popularity-skewed ids) — the plan is NOT usable, build a sorted plan instead;
 *       plan[2] != 0: some row has more than 64 occurrences in a batch (usable, but slow: prefer the sorted plan's hot-row
 *       path).  Tables beyond 2^21 rows are hashed into 2^21 bits: a collision makes a row look shared, never the reverse.
 *   wr_bprmf_run_sgd_group  the steps of batches [first_batch, first_batch + n_batches) of that plan; `u, p, n` are the
 *       arrays the plan was built from.  The item rows with several occurrences in batch k are rewritten by workgroups
 *       that ride in the launch of step k+1 (write-through stores + an in-launch counter hand-off, as wr_bprmf_run_sgd_chain);
 *       the call ends with a launch of its own for the last batch's, so the stream holds complete steps on return.
 *       Every table row has one writer per step and a fixed summation order (bitwise reproducible); the order differs from
 *       the sorted plan's, so tables agree with wr_bprmf_run_sgd to rounding (1e-7 relative), not bit for bit.
 *       events (may be NULL): 2 handles per step, start / stop of the launch that carries step k's triplets.
 *       workspace >= wr_bprmf_group_workspace_bytes(batch_size, D); sync: wr_bprmf_group_sync_words(n_batches) int32 words,
 *       16-byte aligned; word sync_words - 4 is the sticky "a bounded wait expired" word (zero it once when allocating).
 *       Rows must be whole 128-byte lines (wr_bprmf_group_supported; WR_E_ALIGN otherwise). */
int64_t wr_group_plan_words(int64_t n_triplets, int64_t batch_size, int64_t n_users, int64_t n_items);
/* out[16] = {n_batches, flag words per batch, user ranges, item ranges, user hash mask, item hash mask, and the offsets (in
 * int32 words from `plan`) of: flags [nb][fw][4], user list lengths [nb][R_u], item list lengths [nb][R_i], user list rows,
 * user list sources, item list rows, item list sources [nb][R][cap]; total words; cap of a user segment; cap of an item
 * segment} — for tools and tests */
int32_t wr_group_plan_layout(int64_t n_triplets, int64_t batch_size, int64_t n_users, int64_t n_items, int64_t *out);
/* int64 index columns (the reference's batch layout, src/models/BaseModel.py:96-127) -> the int32 columns the group plan
 * and its step read; ids outside [0, 2^31) become -1 (reported by the plan as out of range). */
int32_t wr_narrow_ids_i64(const int64_t *u, const int64_t *p, const int64_t *n, int32_t *u32, int32_t *p32, int32_t *n32,
                          int64_t count, void *stream);
int32_t wr_group_plan_build(const int32_t *u, const int32_t *p, const int32_t *n, int64_t n_triplets, int64_t batch_size,
                            int64_t n_users, int64_t n_items, int32_t *plan, int64_t plan_words, void *stream);
int64_t wr_bprmf_group_workspace_bytes(int64_t batch_size, int32_t D);
int64_t wr_bprmf_group_sync_words(int64_t n_batches);
int32_t wr_bprmf_group_supported(const float *user_tab, const float *item_tab, int32_t D);
int32_t wr_bprmf_run_sgd_group(float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D,
                               const int32_t *u, const int32_t *p, const int32_t *n, int64_t n_triplets, int64_t batch_size,
                               const int32_t *plan, int64_t plan_words, int64_t first_batch, int64_t n_batches, float lr,
                               float *loss_out, void *const *events, void *workspace, int64_t workspace_bytes, int32_t *sync,
                               int64_t sync_words, void *stream);

/* Plan-time marks for wr_bprmf_run_sgd_chain (index work only; call after the plan build, on the same stream).
 *   bitmap [n_batches * ceil(n_items/32)] (out): per batch, bit r = item row r has several occurrences in the batch;
 *   prev_bitmap: that bitmap of the batch BEFORE this plan's first batch, or NULL (then the first batch defers nothing);
 *   tdef, def_q as above (out); def_count [n_batches] (out, device): deferred runs per batch — may exceed def_cap, in which
 *   case only the first def_cap positions were stored and the caller must use wr_bprmf_run_sgd for this plan.
 * Every index is range-checked: safe on a plan whose hand-written builder reported a bucket overflow. */
int32_t wr_bprmf_plan_overlap_marks(const int32_t *tu, const int32_t *tp, const int32_t *tn, int64_t n_triplets,
                                    int64_t batch_size, int64_t n_items, const int32_t *prev_bitmap, int32_t *bitmap,
                                    int32_t *tdef, int32_t *def_q, int64_t def_cap, int32_t *def_count, void *stream);

/* The second half of wr_bprmf_plan_overlap_marks for a `bitmap` that is already complete (written by
 * wr_bprmf_plan_build_fast_marks_*): deferred-run mask, list and counts only. */
int32_t wr_bprmf_plan_overlap_deferred(const int32_t *tu, const int32_t *tp, const int32_t *tn, int64_t n_triplets,
                                       int64_t batch_size, int64_t n_items, const int32_t *prev_bitmap, const int32_t *bitmap,
                                       int32_t *tdef, int32_t *def_q, int64_t def_cap, int32_t *def_count, void *stream);

/* Same two kernels in gradient-emitting mode: instead of updating the tables, writes the reduced
 * gradient rows (embedding_dense_backward of BaseRunner.py:198) to grad_u[r,:] / grad_i[r,:] for rows in
 * the batch and sets stamp[r] = step_id.  Rows not in the batch are not written: a consumer treats
 * stamp[r] != step_id as a zero gradient row (wr_adam_dense / wr_sgd_dense below).  stamp_u / stamp_i may be
 * NULL (a caller that zero-filled grad_u / grad_i and reads them densely). */
int32_t wr_bprmf_grads(const float *user_tab, int64_t n_users, const float *item_tab, int64_t n_items, int32_t D,
                       const int32_t *tu, const int32_t *tp, const int32_t *tn, const int32_t *oc_item,
                       const int32_t *oc_src, int64_t B, float *grad_u, float *grad_i, int32_t *stamp_u,
                       int32_t *stamp_i, int32_t step_id, float *loss_out, const wr_hot_runs *hot, void *workspace,
                       int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K5  optimizers over a whole table — torch.optim.{SGD,Adam}.step as built at BaseRunner.py:120-124.
 * grad rows are valid where stamp[r] == step_id and are zero elsewhere (stamp == NULL: all rows valid).
 * --------------------------------------------------------------------------------------------------- */
/* w <- w - lr*l2*w for rows with stamp[r] != step_id (completes weight decay after wr_bprmf_step_sgd) */
int32_t wr_sgd_decay_untouched(float *tab, int64_t n_rows, int32_t D, const int32_t *stamp, int32_t step_id, float lr,
                               float l2, void *stream);
/* g' = g + l2*w ; w <- w - lr*g' */
int32_t wr_sgd_dense(float *tab, int64_t n_rows, int32_t D, const float *grad, const int32_t *stamp, int32_t step_id,
                     float lr, float l2, void *stream);
/* Adam (amsgrad off): g' = g + l2*w; m = lerp(m,g',1-b1); v = b2 v + (1-b2) g'^2;
 * w <- w - lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps);  t = adam_step (1-based) */
int32_t wr_adam_dense(float *tab, float *exp_avg, float *exp_avg_sq, int64_t n_rows, int32_t D, const float *grad,
                      const int32_t *stamp, int32_t step_id, int64_t adam_step, float lr, float l2, float beta1,
                      float beta2, float eps, void *stream);

/* wr_adam_dense with the step number in device memory (consts as for wr_adam_rows_lazy: consts[2t] = lr/(1-beta1^t),
 * consts[2t+1] = 1/sqrt(1-beta2^t); t = step_dev[0], 1-based, must be < n_consts): the launch has no step-dependent
 * argument, so a hipGraph that captured a whole training step can be replayed; wr_counter_add advances the counter inside the
 * same graph.  All rows take the gradient (no stamps). */
int32_t wr_adam_dense_dev(float *tab, float *exp_avg, float *exp_avg_sq, int64_t n_rows, int32_t D, const float *grad,
                          const float *consts, int64_t n_consts, const int32_t *step_dev, float l2, float beta1, float beta2,
                          float eps, void *stream);

/* wr_adam_dense_dev for two tables of the same width in ONE launch (a model's user and item embeddings; one graph node and
 * one launch latency fewer per step).  Same arithmetic per element. */
int32_t wr_adam_dense_dev_pair(float *tab_a, float *exp_avg_a, float *exp_avg_sq_a, int64_t n_rows_a, const float *grad_a,
                               float *tab_b, float *exp_avg_b, float *exp_avg_sq_b, int64_t n_rows_b, const float *grad_b,
                               int32_t D, const float *consts, int64_t n_consts, const int32_t *step_dev, float l2,
                               float beta1, float beta2, float eps, void *stream);
int32_t wr_counter_add(int32_t *counter, int32_t delta, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K5 (lazy, exact)  The same optimizers without the table passes.  torch.optim.Adam / SGD(weight_decay) move every
 * row at every step (BaseRunner.py:120-124,199); between two batches that contain it a row's trajectory depends on
 * the row alone, so it is replayed when the row is next needed: last_step[r] = number of the last optimizer step
 * applied to row r (0 = none).  Same element arithmetic, order and per-step bias corrections as wr_adam_dense /
 * wr_sgd_dense: the tables come out bit-identical to the dense kernels'.
 *   step t of a batch:  wr_*_rows_lazy(grad = NULL) on the batch's rows  ->  gradients (wr_bprmf_grads / the fused SGD
 *   step)  ->  wr_adam_rows_lazy(grad) ;  before evaluation / checkpoint: wr_*_catchup_all.
 * keys: row ids of one batch with equal ids adjacent (the plan's tu / oc_item arrays); each distinct row is done once.
 * consts: device array, consts[2s] = lr/(1-beta1^s), consts[2s+1] = 1/sqrt(1-beta2^s) for s < n_consts (fill a host
 * copy with wr_adam_consts — the expressions wr_adam_dense evaluates on the host).
 * --------------------------------------------------------------------------------------------------- */
int32_t wr_adam_consts(int64_t first_step, int64_t n_steps, float lr, float beta1, float beta2, float *consts_host);
/* grad == NULL: replay the rows up to step adam_step-1.  grad != NULL ([n_rows, D], rows of the batch valid): replay
 * up to adam_step-1 if still needed, then apply step adam_step with the gradient row. */
int32_t wr_adam_rows_lazy(float *tab, float *exp_avg, float *exp_avg_sq, int32_t *last_step, int64_t n_rows, int32_t D,
                          const int32_t *keys, int64_t n_keys, const float *grad, int64_t adam_step, const float *consts,
                          int64_t n_consts, float l2, float beta1, float beta2, float eps, void *stream);
/* every row up to and including step adam_step (zero gradients) */
int32_t wr_adam_catchup_all(float *tab, float *exp_avg, float *exp_avg_sq, int32_t *last_step, int64_t n_rows, int32_t D,
                            int64_t adam_step, const float *consts, int64_t n_consts, float l2, float beta1, float beta2,
                            float eps, void *stream);
/* SGD weight decay: replay w <- w - lr*l2*w on the batch's rows up to step-1 and mark them as done for `step` (the fused
 * step wr_bprmf_step_sgd applies step `step` itself, decay included, to exactly these rows).  lr and l2 must not have
 * changed since the rows' last step (call wr_sgd_catchup_all before changing them). */
int32_t wr_sgd_rows_lazy(float *tab, int32_t *last_step, int64_t n_rows, int32_t D, const int32_t *keys, int64_t n_keys,
                         int64_t step, float lr, float l2, void *stream);
int32_t wr_sgd_catchup_all(float *tab, int32_t *last_step, int64_t n_rows, int32_t D, int64_t step, float lr, float l2,
                           void *stream);

/* One Adam step on one batch with the update fused into the step kernels (the fused SGD step's two kernels with Adam where
 * they apply SGD): the team that finishes a row reads its two moment rows, takes torch.optim.Adam's step (adam_elem, the
 * arithmetic of wr_adam_dense) and writes weights and moments back; no gradient table.  Every row of the batch must be up to
 * date through adam_step - 1 (wr_adam_rows_lazy with grad = NULL first); last_* [n_rows] become adam_step for those rows. */
int32_t wr_bprmf_step_adam(float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D, float *m_u,
                           float *v_u, float *m_i, float *v_i, int32_t *last_u, int32_t *last_i, const int32_t *tu,
                           const int32_t *tp, const int32_t *tn, const int32_t *oc_item, const int32_t *oc_src, int64_t B,
                           int64_t adam_step, float lr, float l2, float beta1, float beta2, float eps, float *loss_out,
                           const wr_hot_runs *hot, void *workspace, int64_t workspace_bytes, void *stream);
/* torch.optim.Adagrad (kind = 1) / torch.optim.Adadelta (kind = 2) with weight_decay = 0 fused into the step kernels, for
 * n_batches consecutive batches of a plan (the reference eval's --optimizer into torch.optim.<name>(params, lr,
 * weight_decay=l2), src/helpers/BaseRunner.py:34-37,120-124).  With a zero gradient neither optimizer moves a weight, so the
 * tables are always current: no catch-up before the gradients, no flush before evaluation.
 *   Adagrad : s1_* = state_sum tables (s2_*, last_* unused, may be NULL); exactly sparse.  eps = 1e-10 in torch.
 *   Adadelta: s1_* = square_avg, s2_* = acc_delta, last_* [n_rows] int32 = step of the row's last update (0 initially): a
 *             missed step multiplies both state rows by rho, replayed by the finisher before step t.  rho 0.9, eps 1e-6.
 * step0 = optimizer step number of the first batch (1-based).  Hot rows are handled (pieces + combine) like in the SGD step. */
int32_t wr_bprmf_run_stateful(int32_t kind, float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D,
                              float *s1_u, float *s2_u, float *s1_i, float *s2_i, int32_t *last_u, int32_t *last_i,
                              const int32_t *tu, const int32_t *tp, const int32_t *tn, const int32_t *oc_item,
                              const int32_t *oc_src, int64_t n_triplets, int64_t batch_size, int64_t first_batch,
                              int64_t n_batches, int64_t step0, float lr, float rho, float eps, float *loss_out,
                              const wr_hot_runs *hot, void *workspace, int64_t workspace_bytes, void *stream);
/* The same step with the catch-up FOLDED into the row loads: rows need NOT be up to date — every team that loads a row
 * replays the missed zero-gradient steps last[row]+1 .. adam_step-1 on its register copy (consts: the table of
 * wr_adam_consts, entries 0..adam_step), the finisher applies step adam_step and writes weights and moments once: 3 row
 * reads + 3 row writes per touched row instead of the 12 transfers of wr_adam_rows_lazy + wr_bprmf_step_adam.  Same bits
 * as the dense optimizer.  Batches with hot rows are refused (WR_E_RANGE): use the separate catch-up for those. */
int32_t wr_bprmf_step_adam_folded(float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D, float *m_u,
                                  float *v_u, float *m_i, float *v_i, int32_t *last_u, int32_t *last_i, const int32_t *tu,
                                  const int32_t *tp, const int32_t *tn, const int32_t *oc_item, const int32_t *oc_src,
                                  int64_t B, int64_t adam_step, float lr, const float *consts, int64_t n_consts, float l2,
                                  float beta1, float beta2, float eps, float *loss_out, void *workspace,
                                  int64_t workspace_bytes, void *stream);
/* wr_bprmf_run_adam_lazy with wr_bprmf_step_adam_folded for every batch without hot rows (same arguments, same results) */
int32_t wr_bprmf_run_adam_folded(float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D, float *m_u,
                                 float *v_u, float *m_i, float *v_i, int32_t *last_u, int32_t *last_i, const int32_t *tu,
                                 const int32_t *tp, const int32_t *tn, const int32_t *oc_item, const int32_t *oc_src,
                                 int64_t n_triplets, int64_t batch_size, int64_t first_batch, int64_t n_batches,
                                 int64_t adam_step0, float lr, const float *consts, int64_t n_consts, float l2, float beta1,
                                 float beta2, float eps, float *loss_out, const wr_hot_runs *hot, void *workspace,
                                 int64_t workspace_bytes, void *stream);
/* wr_bprmf_run_adam_folded as ONE launch per step (round 3): the item phase of step k-1 — the rows that recur in batch k-1:
 * weights, both moments and the step stamp, stored write-through — rides in the launch of step k's user phase; the user runs
 * of batch k that read such a row wait for it inside the launch (the chained launch of wr_bprmf_run_sgd_chain, same marks:
 * tdef / def_q / def_count_host / def_cap / def_limit from wr_bprmf_plan_overlap_deferred).  No batch of the range may have
 * hot rows (the caller takes wr_bprmf_run_adam_folded for such plans).  workspace: 2 x wr_bprmf_step_workspace_bytes; sync:
 * wr_bprmf_chain_sync_words(n_batches).  Same bits as the dense optimizer. */
int32_t wr_bprmf_run_adam_folded_chain(float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D,
                                       float *m_u, float *v_u, float *m_i, float *v_i, int32_t *last_u, int32_t *last_i,
                                       const int32_t *tu, const int32_t *tp, const int32_t *tn, const int32_t *oc_item,
                                       const int32_t *oc_src, int64_t n_triplets, int64_t batch_size, int64_t first_batch,
                                       int64_t n_batches, int64_t adam_step0, float lr, const float *consts, int64_t n_consts,
                                       float l2, float beta1, float beta2, float eps, float *loss_out, const int32_t *tdef,
                                       const int32_t *def_q, const int32_t *def_count_host, int64_t def_cap, int64_t def_limit,
                                       void *workspace, int64_t workspace_bytes, int32_t *sync, int64_t sync_words,
                                       void *stream);
/* wr_bprmf_run_adam_lazy with a bounded lag: before every step a rotating window of ceil(rows / max_lag) consecutive rows
 * of each table is brought to the previous step (wr_adam_catchup_all on the sub-range), so that no row ever misses more
 * than max_lag steps and the replays of a batch's rows stay short (small batches on big tables: a geometric tail of
 * thousands of missed steps otherwise makes every catch-up launch wait for its unluckiest wave).  Same bits as the dense
 * optimizer.  sweep_pos (HOST memory, in/out): [0] next user row, [1] next item row of the window; start at {0, 0}. */
int32_t wr_bprmf_run_adam_lazy_bounded(float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D,
                                       float *m_u, float *v_u, float *m_i, float *v_i, int32_t *last_u, int32_t *last_i,
                                       const int32_t *tu, const int32_t *tp, const int32_t *tn, const int32_t *oc_item,
                                       const int32_t *oc_src, int64_t n_triplets, int64_t batch_size, int64_t first_batch,
                                       int64_t n_batches, int64_t adam_step0, float lr, const float *consts, int64_t n_consts,
                                       float l2, float beta1, float beta2, float eps, float *loss_out, const wr_hot_runs *hot,
                                       int64_t max_lag, int64_t *sweep_pos, void *workspace, int64_t workspace_bytes,
                                       void *stream);
/* The bounded-lag forms of wr_bprmf_run_sgd_lazy and wr_bprmf_run_stateful (Adadelta), as wr_bprmf_run_adam_lazy_bounded:
 * a rotating window of ceil(rows / max_lag) rows per table takes the zero-gradient steps it missed before every step
 * (wr_sgd_catchup_all / wr_adadelta_decay_all on the sub-range).  Same bits as without the window. */
int32_t wr_bprmf_run_sgd_lazy_bounded(float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D,
                                      int32_t *last_u, int32_t *last_i, int32_t *stamp_u, int32_t *stamp_i, int32_t step_id0,
                                      const int32_t *tu, const int32_t *tp, const int32_t *tn, const int32_t *oc_item,
                                      const int32_t *oc_src, int64_t n_triplets, int64_t batch_size, int64_t first_batch,
                                      int64_t n_batches, int64_t step0, float lr, float l2, float *loss_out,
                                      const wr_hot_runs *hot, int64_t max_lag, int64_t *sweep_pos, void *workspace,
                                      int64_t workspace_bytes, void *stream);
int32_t wr_bprmf_run_stateful_bounded(int32_t kind, float *user_tab, int64_t n_users, float *item_tab, int64_t n_items,
                                      int32_t D, float *s1_u, float *s2_u, float *s1_i, float *s2_i, int32_t *last_u,
                                      int32_t *last_i, const int32_t *tu, const int32_t *tp, const int32_t *tn,
                                      const int32_t *oc_item, const int32_t *oc_src, int64_t n_triplets, int64_t batch_size,
                                      int64_t first_batch, int64_t n_batches, int64_t step0, float lr, float rho, float eps,
                                      float *loss_out, const wr_hot_runs *hot, int64_t max_lag, int64_t *sweep_pos,
                                      void *workspace, int64_t workspace_bytes, void *stream);
/* Adadelta's zero-gradient steps on rows [0, n_rows): both state rows times rho once per missed step (step - last_step[r]
 * multiplications), last_step[r] = step. */
int32_t wr_adadelta_decay_all(float *square_avg, float *acc_delta, int32_t *last_step, int64_t n_rows, int32_t D, int64_t step,
                              float rho, void *stream);
/* n_batches consecutive optimizer steps over batches [first_batch, first_batch + n_batches) of a plan, issued from native
 * code (the inner loop of BaseRunner.fit, BaseRunner.py:196-199, with the lazy optimizers): per batch
 *   Adam:  wr_adam_rows_lazy(NULL) on U and I rows -> wr_bprmf_step_adam (gradients + Adam on the rows it finishes);
 *   SGD + weight decay:  wr_sgd_rows_lazy on U and I rows -> wr_bprmf_step_sgd.
 * adam_step0 / step0 = optimizer step number of the first batch (1-based); step_id0 = stamp id of the first batch;
 * loss_out[k] receives batch k's loss (may be NULL). */
int32_t wr_bprmf_run_adam_lazy(float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D, float *m_u,
                               float *v_u, float *m_i, float *v_i, int32_t *last_u, int32_t *last_i, const int32_t *tu,
                               const int32_t *tp, const int32_t *tn, const int32_t *oc_item, const int32_t *oc_src,
                               int64_t n_triplets, int64_t batch_size, int64_t first_batch, int64_t n_batches,
                               int64_t adam_step0, float lr, const float *consts, int64_t n_consts, float l2, float beta1,
                               float beta2, float eps, float *loss_out, const wr_hot_runs *hot, void *workspace,
                               int64_t workspace_bytes, void *stream);
int32_t wr_bprmf_run_sgd_lazy(float *user_tab, int64_t n_users, float *item_tab, int64_t n_items, int32_t D, int32_t *last_u,
                              int32_t *last_i, int32_t *stamp_u, int32_t *stamp_i, int32_t step_id0, const int32_t *tu,
                              const int32_t *tp, const int32_t *tn, const int32_t *oc_item, const int32_t *oc_src,
                              int64_t n_triplets, int64_t batch_size, int64_t first_batch, int64_t n_batches, int64_t step0,
                              float lr, float l2, float *loss_out, const wr_hot_runs *hot, void *workspace,
                              int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K9  nn.Embedding forward / embedding_dense_backward with padding_idx —
 *     src/models/sequential/SASRec.py:60,84,105-106; also the row-exchange primitive of the
 *     row-sharded multi-GPU step.
 * out[k,:] = tab[idx[k],:]                                        (gather; padding rows are read as stored)
 * grad[idx[k],:] += src[k,:] for idx[k] != padding_idx            (deterministic: one writer per row, position order)
 * --------------------------------------------------------------------------------------------------- */
int32_t wr_gather_rows(const float *tab, int64_t n_rows, int32_t D, const int64_t *idx, int64_t n, float *out,
                       void *stream);
int64_t wr_scatter_add_workspace_bytes(int64_t n, int64_t n_rows);
int32_t wr_scatter_add_rows(float *grad, int64_t n_rows, int32_t D, const int64_t *idx, const float *src, int64_t n,
                            int64_t padding_idx, float alpha, void *workspace, int64_t workspace_bytes, void *stream);

/* The same scatter-add through a ROW PLAN instead of a sort of the positions (wr_scatter.hip; tables of any size, segments
 * of at most 2^18 positions).  The plan is index work only, so a caller that knows the indices of several calls ahead — the
 * row-sharded step knows the rows it will serve for a whole chunk of steps — builds ONE plan for all of them (segment s =
 * idx[s * seg_stride .. + seg_len[s]), seg_len on the device or NULL = every segment full) and applies segment after
 * segment: one launch per call.  Per segment: a flag bit per position (its row recurs in the segment) and the recurring
 * positions ordered by (row, position); rows that occur once are added in place, runs are summed in position order (the
 * bits of wr_scatter_add_rows).  plan[1] != 0 after a build: some range of rows held more than 8,192 recurring positions and
 * is summed by brute force (slow, exact).  wr_scatter_add_rows itself takes this path for tables beyond 16,383 rows.
 * wr_scatter_plan_words returns 0 when the plan does not apply (segments longer than 2^18 positions). */
int64_t wr_scatter_plan_words(int64_t n_segments, int64_t seg_stride, int64_t n_rows);
int32_t wr_scatter_plan_build(const int64_t *idx, int64_t n_segments, int64_t seg_stride, const int32_t *seg_len, int64_t n_rows,
                              int64_t padding_idx, int32_t *plan, int64_t plan_words, void *stream);
int32_t wr_scatter_add_planned(float *table, int64_t n_rows, int32_t D, const int64_t *idx, int64_t n_segments,
                               int64_t seg_stride, int64_t segment, int64_t n, int64_t padding_idx, const float *src,
                               float alpha, const int32_t *plan, int64_t plan_words, void *stream);

/* tab[sorted_rows[q], :] += alpha * sum of src[perm[q'], :] over the run of equal sorted_rows (rows ascending; the
 * order was fixed when the exchange was planned, so the sum is reproducible).  Entries >= n_rows are skipped.
 * Owner-side application of gradient rows received from other shards (alpha = -lr for SGD). */
int32_t wr_apply_rows_sorted(float *tab, int64_t n_rows, int32_t D, const int32_t *sorted_rows, const int32_t *perm,
                             const float *src, int64_t n, float alpha, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Row-sharded step (multi-GPU) on a SORTED batch plan — the form for batches the group plan does not take (popularity-skewed
 * ids, shards small against the batch; wr_bprmf_shard_step_group is the usual one): the same two kernels with the user rows
 * of this shard updated in place (SGD, l2 = 0).  `item_rows` [n_rows, D] = the shard's own item rows [0, n_local_items),
 * rewritten in place, followed by the rows received from their owners for this step (tp/tn/oc_item hold row ids into
 * it); `grad_slots` [n_rows - n_local_items, D] receives the reduced gradient row of every received row (to be returned
 * to the owners).  The loss term and coefficient are scaled by 1/global_batch (the mean runs over all shards' triplets);
 * loss_partial = this shard's share.
 * --------------------------------------------------------------------------------------------------- */
int32_t wr_bprmf_shard_step(float *user_shard, int64_t n_user_rows, float *item_rows, int64_t n_rows, int64_t n_local_items,
                            int32_t D, const int32_t *tu, const int32_t *tp, const int32_t *tn, const int32_t *oc_item,
                            const int32_t *oc_src, int64_t B, int64_t global_batch, float lr, float *grad_slots,
                            float *loss_partial, const wr_hot_runs *hot, void *workspace, int64_t workspace_bytes,
                            void *stream);

/* Row-sharded step without a per-batch sort (whisprrec_amd/sharded.py; wr_shard.hip + wr_group.hip) — ONE BaseRunner.fit
 * iteration (src/helpers/BaseRunner.py:196-199) over the union of the ranks' batches, negatives from ALL items
 * (src/models/BaseModel.py:168,174).  Item row i lives on rank i % world at local row i / world; a rank owns the users of its
 * triplets.  A rank's LOCAL item rows are read and rewritten in its shard in place; REMOTE ones are received from their
 * owners into rows [n_local_items, n_local_items + slots) of the same buffer (`item_ext`) and their gradient rows go back.
 *   wr_shard_route   index work for a chunk of batches: vu / vp / vn = the triplets with local user rows and "virtual" item
 *       ids (local row, or n_local_items + slot; a step's distinct remote items get slots 0, 1, ... in ascending (owner, row)
 *       order); send_rows [world][n_batches][list_cap] / send_cnt [world][n_batches] = per owner and batch the requested
 *       local rows (ascending) and their number — exchanged by two fixed-size all-to-alls.  rows_per_owner: a multiple of
 *       32 with world * rows_per_owner >= n_items.  err[0] != 0: an id out of range or a user of another rank; err[1] != 0:
 *       a request list beyond list_cap.
 *   wr_shard_pack    after the exchange (recv_rows / recv_cnt in the same layout, indexed by requester): per batch the rows
 *       to serve, requester by requester (serve_rows [n_batches][serve_stride], int64) and where each requester's rows
 *       start (serve_off [n_batches][world + 1]).  err[0] != 0: a peer asked for a row this shard does not have.
 *   wr_bprmf_shard_step_group   batch `batch` of a group plan built on (vu, vp, vn) with n_items = n_ext_rows: user rows and
 *       local item rows updated in place (SGD, l2 = 0), grad_slots[s] = the summed gradient row of slot s; coefficients and
 *       the loss share are scaled by 1 / global_batch.  Two launches (the triplets, then the batch's own tiles).
 *       workspace / sync as for wr_bprmf_run_sgd_group (sync: at least wr_bprmf_group_sync_words(1) words). */
int32_t wr_shard_route(const int32_t *u, const int32_t *p, const int32_t *n, int64_t n_triplets, int64_t batch_size, int32_t world,
                       int32_t rank, int64_t n_users, int64_t n_items, int64_t rows_per_owner, int64_t n_local_items,
                       int64_t list_cap, int32_t *vu, int32_t *vp, int32_t *vn, int32_t *send_rows, int32_t *send_cnt,
                       int32_t *err, void *stream);
int32_t wr_shard_pack(const int32_t *recv_rows, const int32_t *recv_cnt, int64_t n_batches, int32_t world, int64_t list_cap,
                      int64_t n_local_items, int64_t *serve_rows, int64_t serve_stride, int32_t *serve_off, int32_t *err,
                      void *stream);
int32_t wr_bprmf_shard_step_group(float *user_shard, int64_t n_user_rows, float *item_ext, int64_t n_ext_rows,
                                  int64_t n_local_items, int32_t D, const int32_t *vu, const int32_t *vp, const int32_t *vn,
                                  int64_t n_triplets, int64_t batch_size, const int32_t *plan, int64_t plan_words, int64_t batch,
                                  int64_t global_batch, float lr, float *grad_slots, float *loss_partial, void *workspace,
                                  int64_t workspace_bytes, int32_t *sync, int64_t sync_words, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K6-K7  LightGCN propagation — src/models/general/LightGCN.py:134-148
 *   Y = A X for the CSR form of the normalised bipartite adjacency (the reference multiplies the dense
 *   form of the same matrix, LightGCN.py:120,139).  If acc != NULL: acc += Y fused (running layer sum
 *   for the mean over layers, LightGCN.py:142-143).  row_ptr int64 [n_rows+1], col int32, val fp32.
 * --------------------------------------------------------------------------------------------------- */
int32_t wr_spmm_csr(int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const float *val, const float *X,
                    int32_t D, float *Y, float *acc, void *stream);
/* Load-balanced form for power-law graphs: the rows are pre-cut (once, on the host: the adjacency is static) into
 * consecutive chunks of at most L non-zeros; chunk c covers non-zeros [chunk_ptr[c], chunk_ptr[c+1]) of row chunk_row[c],
 * every row has at least one (possibly empty) chunk, the chunks of a row are consecutive.  partials: fp32 [n_chunks, D]
 * scratch.  Rows with several chunks are summed in chunk order (reproducible). */
int32_t wr_spmm_csr_chunked(int64_t n_rows, int64_t n_chunks, const int64_t *chunk_ptr, const int32_t *chunk_row,
                            const int32_t *col, const float *val, const float *X, int32_t D, float *Y, float *acc,
                            float *partials, void *stream);

/* Hybrid product for graphs with a dense head (popular items): the block (all users) x (head items) of the adjacency and
 * its transpose are kept DENSE and multiplied on the matrix cores (v_mfma_f32_32x32x2_f32, exact fp32), the rest stays on
 * the chunked CSR kernels.  Per 32-row output tile the dense block is stored as A_T[tile][k][32] (value of tile row r and
 * column k at [k][r], zeros included), k = 0..K_pad-1 with cols[k] the node id of column k (padding columns: -1 —
 * they contribute exact zeros whatever X holds — or any valid node with zero values); rows[tile*32 + r] is the node id of tile row r (-1: padding row).  K_pad is cut into splits of
 * k_per_split columns (a multiple of 64, at most 1024), one workgroup each; with one split the tile is written to Y (acc must be NULL:
 * such rows also have a CSR part, which adds the layer sum), with several the split tiles go to `partials`
 * (wr_spmm_dense_partials_bytes) and are added in split order, then Y[row] is written and acc[row] += it.  D in
 * {32, 64, 96, 128}.  Summation order differs from CSR order: results agree with wr_spmm_csr to fp32 rounding (1e-6
 * relative on unit-scale data), and are bitwise reproducible.
 * wr_spmm_csr_chunked_modes: the CSR part — row_mode[row] (int8): 0 = write Y[row] (and acc), 1 = ADD to the Y[row] the
 * dense tiles wrote before (then acc), 2 = skip the row (it belongs to the dense tiles). */
int64_t wr_spmm_dense_partials_bytes(int64_t n_tiles, int64_t K_pad, int64_t k_per_split, int32_t D);
typedef struct wr_dense_group {
    const float *A_T;        /* [n_tiles][K_pad][32] */
    const int32_t *cols;     /* [K_pad] node id of column k */
    const int32_t *rows;     /* [n_tiles*32] node id of tile row r, -1 = padding */
    float *partials;         /* >= wr_spmm_dense_partials_bytes(...) when K_pad > k_per_split, else may be NULL */
    int64_t K_pad, k_per_split, n_tiles;
} wr_dense_group;
/* One launch for both tile groups of the hybrid product (either may be NULL): `unsplit` (K_pad == k_per_split: tiles written
 * straight to Y; acc is NOT touched for them) and `split` (K_pad > k_per_split: split tiles to its partials, then Y and acc). */
int32_t wr_spmm_dense_tiles(const wr_dense_group *unsplit, const wr_dense_group *split, const float *X, int64_t n_nodes,
                            int32_t D, float *Y, float *acc, void *stream);
int32_t wr_spmm_csr_chunked_modes(int64_t n_rows, int64_t n_chunks, const int64_t *chunk_ptr, const int32_t *chunk_row,
                                  const int32_t *col, const float *val, const float *X, int32_t D, float *Y, float *acc,
                                  float *partials, const int8_t *row_mode, void *stream);
/* The same product with the number of combine levels chosen by the caller (row_mode may be NULL): 2 = chunks of a row are
 * first added inside aligned groups of 16 chunk slots, then the group leaders (a hub row with hundreds of chunks is not one
 * team's chain of hundreds of dependent adds); 1 = the row's first chunk adds all the others itself — one launch less,
 * right while no row has more than a few dozen chunks.  The summation order (hence the rounding) differs between the two;
 * each is fixed and reproducible.
 * acc (may be NULL) is the running layer sum: acc[r] = (base[r] + Y[r]) * acc_scale with base = acc, or = X when
 * acc_from_x != 0 (first layer: no copy of the input into acc beforehand); acc_scale = 1 except for the last layer's
 * 1 / (layers + 1) (LightGCN.py:142-143: mean over the layers). */
int32_t wr_spmm_csr_chunked_levels(int64_t n_rows, int64_t n_chunks, const int64_t *chunk_ptr, const int32_t *chunk_row,
                                   const int32_t *col, const float *val, const float *X, int32_t D, float *Y, float *acc,
                                   float *partials, const int8_t *row_mode, int32_t levels, int32_t acc_from_x,
                                   float acc_scale, void *stream);

/* The same product (one combine level) in ONE launch: the chunk of a cut row that finishes last adds the row's partials
 * itself (in chunk order: the bits of the two-launch form) instead of a combine launch doing it.  row_span[2r], [2r + 1]:
 * first chunk and number of chunks of row r; counters: n_rows words, zero before the first call (every call leaves them
 * zero).  Rows must be whole 128-byte lines: wr_spmm_fused_supported(D, partials) != 0 (D % 32 == 0, partials 128-byte
 * aligned); rows cut into more than a few dozen chunks are better served by the two-level form. */
int32_t wr_spmm_fused_supported(int32_t D, const float *partials);
int32_t wr_spmm_csr_chunked_fused(int64_t n_rows, int64_t n_chunks, const int64_t *chunk_ptr, const int32_t *chunk_row,
                                  const int32_t *row_span, const int32_t *col, const float *val, const float *X, int32_t D,
                                  float *Y, float *acc, float *partials, const int8_t *row_mode, int32_t acc_from_x,
                                  float acc_scale, uint32_t *counters, void *stream);
/* out = alpha * x  /  y += alpha * x  over numel floats (layer-mean scaling, gradient accumulation) */
int32_t wr_axpy(float *y, const float *x, int64_t numel, float alpha, int32_t overwrite, void *stream);
/* EmbLoss pieces (src/utils/loss.py:94-98): sq[0..2] = sum of squares of the gathered U[u], I[p], I[n] blocks */
int32_t wr_embloss_sumsq(const float *user_tab, const float *item_tab, int32_t D, const int64_t *u, const int64_t *p,
                         const int64_t *n, int64_t B, float *sq3, void *workspace, int64_t workspace_bytes,
                         void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K10  Full-ranking evaluation — BaseRunner.interface + evaluate_method (src/helpers/BaseRunner.py:218-258, 50-92) over
 *      full_predict (src/models/general/BPRMF.py:82-91), without materialising the [n, n_items] score matrix:
 *   rank[i] = 1 + #{ j not in mask(eval_user[i]) : <user_mat[eval_user[i]], item_tab[j]>  >  target_score[i] }
 *   target_score[i] = <user_mat[eval_user[i]], item_tab[eval_target[i]]>
 *   A NaN target_score[i] (a diverged model) compares false with every item: such a row gets rank[i] = n_items + 1, behind
 *   everything, in wr_rank_eval_rows and wr_rank_eval_multi alike.  A NaN score of another item never counts.
 * mask_ptr int64 [n_user_rows+1] / mask_idx int32 (ascending per user): the user's train + dev + test items, which the
 * reference sets to -inf (BaseRunner.py:246-255); both NULL = no masking (--test_all 0).  Scores are computed on the matrix
 * cores with v_mfma_f32_32x32x2_f32 (exact fp32 k-ordered fma chain).  rank: int32 [n]; target_score: fp32 [n] (output).
 * --------------------------------------------------------------------------------------------------- */
int32_t wr_rank_eval(const float *user_mat, int64_t n_user_rows, const float *item_tab, int64_t n_items, int32_t D,
                     const int64_t *eval_user, const int64_t *eval_target, int64_t n, const int64_t *mask_ptr,
                     const int32_t *mask_idx, int32_t *rank, float *target_score, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K11  Top-K recommendation: for each query row q, the k unmasked items with the largest
 *   score(q, j) = <user_mat[query_user[q]], item_tab[j]>, ordered by score descending, ties by item id ascending.
 * The reference's save_rec_results (src/main.py:83-102, commented out there) over full_predict, without the [n, n_items]
 * score matrix.
 *   - Scores: the fp32 k-ordered chain of v_mfma_f32_32x32x2_f32 over k = 0..D-1 that wr_rank_eval computes: a returned
 *     score is bitwise equal to wr_rank_eval's target_score for that (user, item) pair.
 *   - Masking: mask_ptr int64 [n_user_rows+1] / mask_idx int32, ascending per user, as for wr_rank_eval; both NULL = no
 *     mask.  A masked item is never returned.
 *   - Order: score descending, then item id ascending (a stable descending sort).
 *   - Padding: a row with fewer than k unmasked items ends with out_item = -1, out_score = -inf.
 *   - out_item int32 [n, k], out_score fp32 [n, k], row-major.  1 <= k <= 256; D in {8, 16, 32, 64} (A operand in
 *     registers) or a multiple of 4 up to 252 (A operand in LDS) — the set wr_rank_eval takes (wr_topk_supported).
 *   - workspace >= wr_topk_workspace_bytes(n, n_items, D, k) bytes, 16-byte aligned; that bound never decreases as n,
 *     n_items or k grow.  Argument errors (WR_E_*) are reported before anything is launched.
 *   - Bitwise reproducible (no float atomics); no host round trip: capturable into a hipGraph.
 * Two launches: a scoring kernel per (128 query rows, item chunk) that keeps each row's K best keys in the workspace, then a
 * merge of the chunk lists per row. */
int32_t wr_topk_supported(int32_t D, int32_t k);
int64_t wr_topk_workspace_bytes(int64_t n, int64_t n_items, int32_t D, int32_t k);
int32_t wr_topk_recommend(const float *user_mat, int64_t n_user_rows, const float *item_tab, int64_t n_items, int32_t D,
                          const int64_t *query_user, int64_t n, const int64_t *mask_ptr, const int32_t *mask_idx,
                          int32_t k, int32_t *out_item, float *out_score, void *workspace, int64_t workspace_bytes,
                          void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K14  Ranking evaluation and top-K with one query vector PER ROW — sequential models (SASRec: the query of row e is
 *      the encoder's output for row e's own history, BaseRunner.py:229-236 over SASRec.full_predict), where the row that
 *      scores and the row that masks are two different things:
 *   score(e, j)     = <query_mat[q(e)], item_tab[j]>,   q(e) = query_row[e], or e itself when query_row is NULL
 *   mask of row e   = the list of row mask_row[e] of the CSR mask_ptr int64 [n_mask_rows+1] / mask_idx int32 (ascending
 *                     per list) — the user of row e; several rows may share one list
 *   wr_rank_eval_rows:       rank[e] = 1 + #{ j not masked for e : score(e, j) > target_score[e] },
 *                            target_score[e] = score(e, eval_target[e])                          (as wr_rank_eval, K10)
 *   wr_topk_recommend_rows:  the k best unmasked items of every row                            (as wr_topk_recommend, K11)
 *   - Same kernels as K10 / K11 (those entries pass their one index array for both roles): the same fp32 k-ordered
 *     v_mfma_f32_32x32x2_f32 chain, so with query_mat[q(e)] = user_mat[u] and mask_row[e] = u every output is bitwise that of
 *     wr_rank_eval / wr_topk_recommend, and a returned top-K score is bitwise the target_score of that (row, item) pair.
 *   - mask_row, mask_ptr and mask_idx are all NULL (no mask) or all non-NULL.  query_row == NULL requires n <= n_query_rows.
 *   - D: the set wr_rank_eval / wr_topk_supported take.  Workspace of the top-K entry: wr_topk_workspace_bytes(n, n_items,
 *     D, k) as it is (it depends on nothing else).  Order, ties and padding of the top-K entry: score descending, then item
 *     id ascending, then -1 / -inf.
 *   - Ids (query_row, eval_target, mask_row) are trusted exactly as wr_rank_eval trusts eval_user and eval_target: they are
 *     not range-checked on the device, the caller passes ids inside [0, n_query_rows), [0, n_items), [0, n_mask_rows).
 *   - Argument errors (WR_E_*) are reported before anything is launched.
 * --------------------------------------------------------------------------------------------------- */
int32_t wr_rank_eval_rows(const float *query_mat, int64_t n_query_rows, const float *item_tab, int64_t n_items, int32_t D,
                          const int64_t *query_row /* NULL: row e */, const int64_t *eval_target, int64_t n,
                          const int64_t *mask_row, int64_t n_mask_rows, const int64_t *mask_ptr, const int32_t *mask_idx,
                          int32_t *rank, float *target_score, void *stream);
int32_t wr_topk_recommend_rows(const float *query_mat, int64_t n_query_rows, const float *item_tab, int64_t n_items, int32_t D,
                               const int64_t *query_row /* NULL: row e */, int64_t n, const int64_t *mask_row,
                               int64_t n_mask_rows, const int64_t *mask_ptr, const int32_t *mask_idx, int32_t k,
                               int32_t *out_item, float *out_score, void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K12  InfoNCE loss and gradient of ONE side (users or items) of SGL's calc_ssl_loss (src/models/general/SGL.py:196-230,
 *      the formula at :213-220), without the [B, n_rows] score matrix.  A = view 1, Bm = view 2, both [n_rows, D] fp32
 *      row-major; idx int64 [B], duplicates allowed:
 *   q_b  = A[idx_b] / max(|A[idx_b]|, 1e-12)        k_j = Bm[j] / max(|Bm[j]|, 1e-12)                     (F.normalize)
 *   s_bj = <q_b, k_j> / tau
 *   loss = weight * sum_b ( log sum_j exp(s_bj)  -  <q_b, k_idx_b> / tau ),   j over ALL n_rows rows
 *   gA   = d loss / d A    non-zero only on the rows named by idx, duplicates summed
 *   gB   = d loss / d Bm   dense: every row receives sum_b softmax_bj q_b / tau back through its normalisation, the rows
 *                          named by idx additionally -q_b / tau
 *   - loss [1] on the device: loss_out = (accumulate ? loss_in : 0) + this side's loss.  gA / gB [n_rows, D] are fully
 *     written (gA is zero outside the batch rows); both NULL = loss only, and that loss has the bits of the full call's.
 *     A, Bm, gA, gB may point into the middle of a larger contiguous table (16-byte aligned).
 *   - Scores: the fp32 k-ordered chain of v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate), as wr_rank_eval.  The products
 *     softmax x rows run on the same instruction.
 *   - eps rule: a row with |x| < 1e-12 follows F.normalize's clamped branch in both directions: y = x / 1e-12 and
 *     d loss / d x = g / 1e-12 with no projection term.
 *   - tau domain: any finite tau > 0.  Cosines are bounded, so the kernels sum exp((c - 1) / tau), which lies in (0, 1],
 *     and add 1 / tau back after the log; there is no running maximum and nothing overflows.  The reference's own
 *     exp(c / tau) overflows fp32 below tau ~ 0.0113, so parity is claimed for tau >= 0.02 only; far below that a row's
 *     whole sum can underflow.
 *   - Determinism: no float atomics.  Item chunks and row blocks go to partials that are folded in chunk order, the loss
 *     terms in a fixed order, and the rows of a duplicated id are summed in ascending batch position by one writer
 *     (a scan of idx per duplicated row: cheap while duplicates are few, quadratic in B when B >> n_rows).  Same inputs,
 *     same bits — loss, gA and gB.
 *   - Bad ids: an id outside [0, n_rows) is clamped to the nearest row, never dereferenced, and err_word[0] |= 1
 *     (err_word may be NULL; the caller clears it).
 *   - D in {32, 64, 128} (wr_infonce_supported); any other value is refused before a launch, like every argument error.
 *   - workspace >= wr_infonce_workspace_bytes(n_rows, B, D), 16-byte aligned.  The bound grows with n_rows * D, with B * D
 *     and with a fixed number of [row, D] chunk partials — never with B * n_rows — and never decreases as n_rows or B grow.
 *   - No host round trip, no allocation: capturable into a hipGraph. */
int32_t wr_infonce_supported(int32_t D);
int64_t wr_infonce_workspace_bytes(int64_t n_rows, int64_t B, int32_t D);
int32_t wr_infonce_loss_grad(const float *A, const float *Bm, int64_t n_rows, int32_t D, const int64_t *idx, int64_t B,
                             float tau, float weight, float *loss, int32_t accumulate, float *gA, float *gB,
                             int32_t *err_word, void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K13  One whole SASRec TransformerLayer (src/utils/layers.py:8-86; whisprrec_amd/sasrec.py::_Block), forward and backward,
 *      fp32.  x, out, grad_out, gx are [B, T, D] row-major.  `params` is a HOST array of 14 device pointers to the live
 *      parameter storages in _Block.state_dict() order — q / k / v linear (weight [D, D], bias [D]), layer_norm1 (weight,
 *      bias), linear1 (weight [d_ff, D], bias), linear2 (weight [D, d_ff], bias), layer_norm2 (weight, bias) — read where they
 *      are: no packing copy.  No output projection, post-norm residuals, LayerNorm eps 1e-5:
 *   q, k, v = x W^T + b;  S = q k^T / sqrt(D / n_heads) per head, causal mask only (padded positions are ordinary tokens)
 *   P = softmax(S - m), m the maximum of S over the WHOLE [B, h, T, T] tensor of the call (layers.py:54), not the row's
 *   A = P v;  C = LN1(drop(A) + x);  out = LN2(drop(relu(C W1^T + b1) W2^T + b2) + C)
 *   - Zeroed rows: a score row whose exponentials all underflow is 0 / 0 in the reference and set to 0 by its isnan fill
 *     (:55); here such a row's attention output is 0 as well and the position sees only its residual.
 *   - Backward: gx and the 14 parameter gradients, packed in gparams in the same order (5 D^2 + 9 D floats, every block
 *     starts at a multiple of D floats); fully written.  The path through the maximum m is ignored: softmax is
 *     shift-invariant, that path sums to zero in exact arithmetic.  DEVIATION: a zeroed row passes no gradient through its
 *     scores, where the reference's autograd yields NaN gradients; that regime is outside the parity claim.
 *   - gmax [1] on the device: the forward stores m, the backward of the same call reads it (it recomputes the forward of a
 *     sequence from x; nothing else is saved).
 *   - Dropout at two sites (0: after attention, 1: after the feed-forward), active iff training != 0 and p > 0; p in [0, 1).
 *     Counter-based keep mask with the splitmix64 finaliser mix64 of the negative sampler, never stored:
 *       key = mix64(seed ^ (site + 1) * 0x9E3779B97F4A7C15);  draw = mix64(key ^ (e * 0xD1B54A32D192ED03 + 1)) >> 40,
 *       e = (b T + t) D + d;  kept iff draw >= floor(p * 2^24), kept elements scaled by the fp32 1 / (1 - p).
 *     Same distribution as torch's dropout, not its Philox stream.  The backward must be given the forward's p, seed, training.
 *   - Determinism: no float atomics.  The maximum is a fold of per-workgroup maxima in index order; parameter gradients go to
 *     per-workgroup partials that are folded in workgroup order.  Same inputs and seed, same bits — out, gx, gparams.
 *   - Supported (wr_sasblock_supported): D = d_ff in {32, 64}, n_heads in {1, 2, 4} with D / n_heads >= 8, 1 <= T <= 64;
 *     B in 1 .. 2^24.  Anything else, a NULL or misaligned (16 B) pointer or a short workspace is refused with WR_E_* before
 *     anything is launched.
 *   - workspace >= wr_sasblock_workspace_bytes(B, T, D, d_ff, n_heads), 16-byte aligned: q / k / v of the call (12 B T D bytes)
 *     plus a fixed number of maxima and gradient partials; never decreases as B or T grow.  The forward and the backward of one
 *     call may share it with other calls on the same stream.
 *   - Launches: forward 2 (projections + maxima; the rest), backward 2 (all sequences; fold of the partials).  No allocation,
 *     no host round trip. */
int32_t wr_sasblock_supported(int32_t D, int32_t d_ff, int32_t n_heads, int32_t T);
int64_t wr_sasblock_workspace_bytes(int64_t B, int32_t T, int32_t D, int32_t d_ff, int32_t n_heads);
int32_t wr_sasblock_fwd(const float *x, int64_t B, int32_t T, int32_t D, int32_t d_ff, int32_t n_heads,
                        const float *const *params, float p, uint64_t seed, int32_t training, float *out, float *gmax,
                        void *workspace, int64_t workspace_bytes, void *stream);
int32_t wr_sasblock_bwd(const float *x, const float *grad_out, int64_t B, int32_t T, int32_t D, int32_t d_ff, int32_t n_heads,
                        const float *const *params, float p, uint64_t seed, int32_t training, const float *gmax, float *gx,
                        float *gparams, void *workspace, int64_t workspace_bytes, void *stream);
/* K13 with a key-length mask instead of the causal one (ContraRec's BERT4RecEncoder, src/models/sequential/ContraRec.py:216-233:
 * attn_mask = valid_mask.view(B, 1, 1, T)).  The arguments of wr_sasblock_fwd / _bwd plus key_len (int64 [B] on the device) and
 * err_word (may be NULL; the caller clears it).  The score of query i against key j is kept iff j < key_len[b], for EVERY query
 * i in 0..T-1: padded query positions are ordinary queries.  Everything else is the K13 contract unchanged — the call-wide
 * maximum over the kept scores, the zeroed-row rule, the dropout sites, no float atomics, fixed fold orders, same bits from run to
 * run, no allocation, no host round trip, the supported shapes, argument errors refused before any launch.
 *   - A key_len outside [1, T] is clamped into it before it bounds any loop, and err_word[0] |= 1.
 *   - The causal entry points are the same templates with the loop bound j <= i: their results are unchanged. */
int32_t wr_sasblock_fwd_keys(const float *x, int64_t B, int32_t T, int32_t D, int32_t d_ff, int32_t n_heads,
                             const float *const *params, float p, uint64_t seed, int32_t training, float *out, float *gmax,
                             void *workspace, int64_t workspace_bytes, void *stream, const int64_t *key_len, int32_t *err_word);
int32_t wr_sasblock_bwd_keys(const float *x, const float *grad_out, int64_t B, int32_t T, int32_t D, int32_t d_ff,
                             int32_t n_heads, const float *const *params, float p, uint64_t seed, int32_t training,
                             const float *gmax, float *gx, float *gparams, void *workspace, int64_t workspace_bytes, void *stream,
                             const int64_t *key_len, int32_t *err_word);

/* ---------------------------------------------------------------------------------------------------
 * K15  Supervised contrastive loss of ContraRec (ContraLoss, src/models/sequential/ContraRec.py:141-204) and its gradient,
 *      without any [2B, 2B] array.  F is [2B, D] fp32 row-major, raw and unnormalised: rows 0..B-1 are view a, rows B..2B-1
 *      view b; labels int64 [B], row r has label labels[r mod B].  With N = 2B and z_i = F_i / max(|F_i|, 1e-12):
 *   s_ij = <z_i, z_j> / tau        m_i = max_j s_ij (diagonal included)        l_ij = s_ij - 2 m_i   (the reference subtracts the
 *   E_i  = sum_{j != i} exp(l_ij)                                                                    row maximum twice, :181-182)
 *   P_i  = { j != i : label_j == label_i }        c_i = |P_i| + 1e-10
 *   loss = weight * (1/N) * sum_i (-tau / c_i) * sum_{j in P_i} ( l_ij - log(E_i + 1e-10) )
 *   gF   = d loss / d F with m_i held constant:  G_ij = (-tau/N) ( [j in P_i] / c_i - (|P_i| / c_i) exp(l_ij) / (E_i + 1e-10) )
 *          for j != i, 0 on the diagonal;  gz = weight (G + G^T) z / tau;  gF_i = (gz_i - <gz_i, z_i> z_i) / |F_i|
 *          (a row with |F_i| < 1e-12 follows K12's eps rule: gF_i = gz_i / 1e-12)
 *   - loss [1] on the device: loss_out = (accumulate ? loss_in : 0) + this loss.  gF [2B, D] is fully written; NULL = loss
 *     only, and that loss has the bits of the full call's.
 *   - Scores: the fp32 k-ordered chain of v_mfma_f32_32x32x2_f32 from wr_score_tiles.h with the normalised rows as both
 *     operands, so s_ij and s_ji have the same bits.  Pass 1 leaves m_i, sum_{j != i} exp(s_ij - 1/tau), |P_i| and
 *     sum_{j in P_i} s_ij per row; pass 2 rebuilds each tile, forms G_ij + G_ji from the statistics of its row and its column
 *     and multiplies by z on the same instruction.
 *   - tau domain: finite tau > 0 is accepted; parity is claimed for tau >= 0.05.  Cosines are bounded, so the exponentials
 *     are taken as e_ij = exp(s_ij - 1/tau) in (0, ~1]; with r_i = exp(1/tau - 2 m_i), exp(l_ij) = e_ij r_i and the 1e-10 joins
 *     the row's sum as 1e-10 / r_i ~ 1e-10 e^{1/tau}.  Below that domain: the reference's own exp(l_ij) ~ exp(-3/tau) of a
 *     dissimilar pair leaves the normal fp32 range under tau ~ 0.034 and e_ij under tau ~ 0.023 (such terms count as 0, the loss
 *     tends to (-tau / c_i) sum_P (l_ij - log 1e-10), here as there); under tau ~ 0.009 1e-10 / r_i overflows and the loss is inf.
 *   - Determinism: no float atomics; column chunks go to partials folded in chunk order, the N row terms in a fixed
 *     order.  Same inputs, same bits.
 *   - D in {32, 64, 128} (wr_supcon_supported), 1 <= B, 2B <= 2^15; anything else, a NULL or misaligned (16 B) pointer or a
 *     short workspace is refused before any launch.  err_word is reserved (labels are compared, never used as indices: no
 *     value is out of range); it may be NULL and is not written.
 *   - workspace >= wr_supcon_workspace_bytes(B, D), 16-byte aligned: the normalised rows, per-row statistics and a bounded
 *     number of [row, D] chunk partials — never N x N.
 *   - No host round trip, no allocation: capturable into a hipGraph. */
int32_t wr_supcon_supported(int32_t D);
int64_t wr_supcon_workspace_bytes(int64_t B, int32_t D);
int32_t wr_supcon_loss_grad(const float *F, int64_t B, int32_t D, const int64_t *labels, float tau, float *loss,
                            int32_t accumulate, float weight, float *gF, int32_t *err_word, void *workspace,
                            int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K16  BUIR's bootstrap loss (src/models/general/BUIR.py:76-97) and every gradient of it in one call.  The four tables are
 *      [n_users | n_items, D] fp32 row-major, W [D, D] (nn.Linear: out x in) and b [D] the shared predictor, users / items
 *      int64 [B].  For sample k with online rows x_u, x_i and target rows t_u, t_i, p = W x + b, z^ = z / max(|z|, 1e-12):
 *   l_k  = 4 - 2 <p_u^, t_i^> - 2 <p_i^, t_u^>        loss = mean_k l_k
 *   g_pu = (-2/B) (t_i^ - p_u^ <p_u^, t_i^>) / |p_u|  (g_pi likewise)        gU[k] = W^T g_pu,  gI[k] = W^T g_pi
 *   gW   = sum_k g_pu x_u^T + g_pi x_i^T               gb = sum_k g_pu + g_pi
 *   - Targets are constants.  gU / gI [B, D] are PER-SAMPLE gradients w.r.t. the gathered online rows (a row that occurs twice
 *     has two entries: scatter-add them for the dense table gradient); gW [D, D], gb [D], loss [1] are fully written.
 *     gU == NULL: loss only (gI, gW, gb are then ignored), with the bits of the full call's loss.
 *   - A predictor output with |p| < 1e-12 is divided by 1e-12 instead of |p| and keeps the projection term: torch passes no
 *     gradient through the clamped norm there.  That regime is not claimed; a zero TARGET row is exact (term 2, gradient 0).
 *   - The three products ([2B, D] x [D, D] forward, the row gradients, the weight gradient) are fp32 k-ordered chains of
 *     v_mfma_f32_32x32x2_f32 (wr_score_tiles.h); rows are gathered straight from the tables, no [B, D] copies.
 *   - Determinism: no float atomics.  Workgroup w (128 samples) writes its partial gW, gb and loss sum into the workspace; a
 *     second launch folds the partials in workgroup order.  The grid depends on (B, D) only: same inputs, same bits on any
 *     device.
 *   - An id outside [0, n_users) / [0, n_items) is clamped into the table and ORs 1 into err_word (int32 on the device, may be
 *     NULL; the caller clears and reads it): no fault follows from an unsafe id.
 *   - D in {32, 64, 128} (wr_buir_supported), 1 <= B <= 2^22; anything else, a NULL or misaligned (16 B) pointer or a short
 *     workspace (< wr_buir_workspace_bytes(B, D), 16-byte aligned) is refused before any launch.
 *   - No host round trip, no allocation. */
int32_t wr_buir_supported(int32_t D);
int64_t wr_buir_workspace_bytes(int64_t B, int32_t D);
int32_t wr_buir_loss_grad(const float *user_online, const float *item_online, const float *user_target,
                          const float *item_target, int64_t n_users, int64_t n_items, int32_t D, const float *W, const float *b,
                          const int64_t *users, const int64_t *items, int64_t B, float *loss, float *gU, float *gI, float *gW,
                          float *gb, int32_t *err_word, void *workspace, int64_t workspace_bytes, void *stream);

/* K17  BUIR's momentum update of a target table (BUIR.py:69-74), in place and in one pass of 16-byte accesses:
 *      t[i] = t[i] * m + o[i] * one_minus_m, i < n — two products and one sum, each rounded (never contracted to an FMA), which
 *      is what torch's `t * m + o * (1. - m)` computes; the caller forms 1 - m in double and narrows it.  Every element is
 *      rewritten (t m + t (1 - m) is not t in fp32).  t and o 16-byte aligned, n >= 1. */
int32_t wr_ema_update(float *t, const float *o, int64_t n, float m, float one_minus_m, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K18  IF4Rec's interest pooling (src/models/sequential/IF4Rec.py:87-103), forward and backward, without the [B, T, D] gather
 *      or the [B, K, T, D] product in global memory.  item_tab [n_items, D], pos_tab [n_pos_rows, D] or NULL (add_pos 0),
 *      history int64 [B, T], W1 [A, D], b1 [A], W2 [K, A], b2 [K] (nn.Linear: out x in), all fp32 row-major:
 *   valid[t] = history[b][t] > 0              hp[t] = item_tab[history[b][t]] + pos_tab[t]
 *   s[k][t]  = b2[k] + <W2[k], leaky_relu(W1 hp[t] + b1, 0.01)> for valid t, -inf otherwise
 *   p[k][.]  = softmax_t s[k][.]   (a row with no valid entry: all 0, the reference's NaN rule)
 *   out[b][k] = sum_t p[k][t] hp[t]                                                                    out [B, K, D]
 *   - Supported (wr_interest_pool_supported): D in {32, 64, 128}, 1 <= A <= 32, 1 <= K <= 8, 1 <= T <= 64, 1 <= B <= 2^24;
 *     n_pos_rows >= T.  Anything else, a NULL or misaligned (16 B) table or a short workspace is refused before any launch.
 *   - The softmax subtracts each row's own maximum, not the reference's maximum over the whole call: softmax is invariant under
 *     the shift, the results differ by the rounding of s - max only (wr_if4rec.hip, file header).
 *   - wr_interest_pool_fwd: one launch.  A sequence's valid rows are gathered once into LDS; padded positions are not read.
 *   - wr_interest_pool_bwd: g_out [B, K, D] -> g_hp [B, T, D] (gradient w.r.t. item row + position row, exactly 0 at masked
 *     positions; scatter-add it for the item-table gradient), gW1 [A, D], gb1 [A], gW2 [K, A], gb2 [K] and gpos [n_pos_rows, D]
 *     (NULL iff pos_tab is NULL; rows at or past T are written as zeros), all fully written.  The forward is recomputed from
 *     the ids.  Workgroup w accumulates the parameter gradients of sequences w, w + G, ... (G = min(B, 512)) in registers and
 *     writes one row of partials; a second launch folds the rows in workgroup order.  No float atomics: same inputs, same
 *     bits.  A row zeroed by the NaN rule passes no gradient (autograd would pass NaN), the deviation K13 documents.
 *   - An id outside [0, n_items) is clamped into the table before it addresses anything and ORs 1 into err_word (int32 on the
 *     device, may be NULL; the caller clears and reads it).
 *   - workspace >= wr_interest_pool_workspace_bytes(B, D, A, K, T), 16-byte aligned (backward only).  No host round trip, no
 *     allocation. */
int32_t wr_interest_pool_supported(int32_t D, int32_t A, int32_t K, int32_t T);
int64_t wr_interest_pool_workspace_bytes(int64_t B, int32_t D, int32_t A, int32_t K, int32_t T);
int32_t wr_interest_pool_fwd(const float *item_tab, int64_t n_items, const float *pos_tab, int64_t n_pos_rows, int32_t D,
                             const int64_t *history, int64_t B, int32_t T, const float *W1, const float *b1, const float *W2,
                             const float *b2, int32_t A, int32_t K, float *out, int32_t *err_word, void *stream);
int32_t wr_interest_pool_bwd(const float *item_tab, int64_t n_items, const float *pos_tab, int64_t n_pos_rows, int32_t D,
                             const int64_t *history, int64_t B, int32_t T, const float *W1, const float *b1, const float *W2,
                             const float *b2, int32_t A, int32_t K, const float *g_out, float *g_hp, float *gW1, float *gb1,
                             float *gW2, float *gb2, float *gpos, int32_t *err_word, void *workspace, int64_t workspace_bytes,
                             void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K19  Ranking evaluation with KQ query vectors per row — multi-interest models (IF4Rec.py:117-118):
 *   score(e, j)     = max_{k < KQ} <query_mat[e KQ + k], item_tab[j]>                        query_mat [n KQ, D]
 *   rank[e]         = 1 + #{ j not masked for e : score(e, j) > target_score[e] },   target_score[e] = score(e, eval_target[e])
 *   - The scans of K10 / K14 run unchanged over the n KQ query rows; a consumer takes the maximum of the KQ adjacent accumulator
 *     registers that hold one row's interests and counts once per row.  Each <.,.> is the fp32 k-ordered chain of
 *     v_mfma_f32_32x32x2_f32, target_score is the maximum of the same chains: the target's own column never counts.
 *   - mask_row int64 [n KQ]: the mask list of QUERY row r = e KQ + k, i.e. row e's entry repeated KQ times (the caller repeats
 *     it on the device); mask_row, mask_ptr and mask_idx are all NULL or all non-NULL.  Ids are trusted as in K14.
 *   - KQ in {1, 2, 4} and the D of wr_rank_eval (wr_rank_eval_multi_supported); KQ = 8 would cross the half-wave.  With KQ = 1
 *     every output is bitwise that of wr_rank_eval_rows without query_row.  wr_rank_eval / wr_rank_eval_rows do not change.
 *   - Argument errors (WR_E_*) are reported before anything is launched. */
int32_t wr_rank_eval_multi_supported(int32_t D, int32_t KQ);
int32_t wr_rank_eval_multi(const float *query_mat, int64_t n_query_rows, const float *item_tab, int64_t n_items, int32_t D,
                           int32_t KQ, const int64_t *eval_target, int64_t n, const int64_t *mask_row, int64_t n_mask_rows,
                           const int64_t *mask_ptr, const int32_t *mask_idx, int32_t *rank, float *target_score, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K23  Top-K recommendation with KQ query vectors per row — multi-interest models (IF4Rec), the selection side of K19:
 *   score(e, j) = max_{q < KQ} <query_mat[e KQ + q], item_tab[j]>                              query_mat [n KQ, D]
 *   out         = the k unmasked items of every evaluation row e with the largest score(e, j)
 *   - Scores: each <.,.> is the fp32 k-ordered chain of v_mfma_f32_32x32x2_f32; a returned score is bitwise wr_rank_eval_multi's
 *     target_score for that (row, item) pair.
 *   - Order, ties, padding and masking are K11's: score descending, then item id ascending; a row with fewer than k unmasked
 *     items ends with -1 / -inf; a masked item is never returned.  out_item int32 [n, k], out_score fp32 [n, k].
 *   - The scans of K11 run unchanged over the n KQ query rows; as in K19 mask_row int64 [n KQ] holds row e's entry repeated KQ
 *     times (the caller repeats it on the device), and mask_row, mask_ptr and mask_idx are all NULL or all non-NULL.  The
 *     consumer takes the maximum of the KQ adjacent accumulator registers that hold one row's interests (the layout argument
 *     of K19), so a lane holds 16/KQ evaluation rows, a wave 32/KQ, a workgroup 128/KQ, and threshold, staging count, ballot
 *     position, workspace region and merge trigger are per EVALUATION row: one item yields at most one candidate per row.
 *   - out_interest int32 [n, k], may be NULL: the smallest q whose chain equals the returned score, -1 at padding.  A small
 *     epilogue launch, one thread per (row, slot), recomputes the KQ fmaf chains (bitwise the MFMA's, as K19's target score).
 *   - KQ in {1, 2, 4} (KQ = 8 would cross the half-wave), D and k as for wr_topk_supported (wr_topk_multi_supported).  With
 *     KQ = 1 the kernels are those of wr_topk_recommend_rows without query_row and every output has its bits.
 *   - workspace >= wr_topk_multi_workspace_bytes(n, n_items, D, KQ, k), 16-byte aligned; the bound never decreases as n,
 *     n_items or k grow, and with KQ = 1 it is wr_topk_workspace_bytes.  n KQ < 2^31, n KQ <= n_query_rows.
 *   - Argument errors (WR_E_*) are reported before anything is launched.  No host round trip, no float atomics: bitwise
 *     reproducible. */
int32_t wr_topk_multi_supported(int32_t D, int32_t KQ, int32_t k);
int64_t wr_topk_multi_workspace_bytes(int64_t n, int64_t n_items, int32_t D, int32_t KQ, int32_t k);
int32_t wr_topk_recommend_multi(const float *query_mat, int64_t n_query_rows, const float *item_tab, int64_t n_items,
                                int32_t D, int32_t KQ, int64_t n, const int64_t *mask_row, int64_t n_mask_rows,
                                const int64_t *mask_ptr, const int32_t *mask_idx, int32_t k, int32_t *out_item,
                                float *out_score, int32_t *out_interest /* may be NULL */, void *workspace,
                                int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K20 SGL's augmented graph views (src/utils/augmentor.py:33-111, csr2tensor of src/models/general/SGL.py:105-146) built on
 *      the device from a resident BASE: the directed edge list (rows, cols) int32 [n_edges] of the symmetric adjacency over
 *      n_nodes nodes, sorted by (row, col) without duplicates; mirror int32 [n_edges], the position of (cols[e], rows[e]);
 *      bchunk_ptr int64 [n_bchunks + 1], the base rows cut into chunks of at most 64 edges that never cross a row, every row
 *      owning at least one (an empty one for an empty row), in row order; row_first_chunk int64 [n_nodes + 1], the first
 *      chunk of each row (entry n_nodes = n_bchunks); dis_tab fp32 [n_dis], (c + 1e-10)^-1/2 for c = 0 .. n_dis - 1, host-built,
 *      n_dis > the largest base degree.
 *   selection  perm = the keyed bijection of wr_epoch_shuffle with key (seed, stream id in the epoch slot).
 *              WR_VIEW_EDGE_DROP: edge e is kept iff perm_{stream_id0}(e) < n_select (n_select edges survive; stream_id1 unused).
 *              WR_VIEW_NODE_DROP: row node v is dropped iff perm_{stream_id0}(v) < n_select, column node v iff
 *              perm_{stream_id1}(v) < n_select; an edge is kept iff neither its row node nor its column node is dropped.
 *   view       forward CSR: the kept edges in base order; transposed CSR: row a lists b iff edge (b, a) is kept, ascending;
 *              val(a, b) = dis_tab[cnt[a]] * dis_tab[cnt[b]] with cnt = kept edges per ROW of the forward view (one fp32
 *              multiply: bitwise the host's norm_csr / transpose_csr for the same kept set).
 *   Three calls per view with two scans by the caller between them; nothing is read back inside any of them:
 *   - wr_sgl_view_count: the keep flags into the workspace, then cnt_fwd / cnt_bwd int32 [n_bchunks], the kept edges of each
 *     base chunk in the forward / the transposed view.  The caller scans both into scan_* int64 [n_bchunks + 1] (exclusive,
 *     entry 0 = 0; the last entry is the view's nnz).
 *   - wr_sgl_view_rows: row_ptr_fwd / row_ptr_bwd int64 [n_nodes + 1] from the scans.
 *   - wr_sgl_view_fill: col int32 / val fp32 [nnz] of both directions (NULL allowed where nnz = 0) from the SAME workspace the
 *     count call filled.  nnz_* are the sizes of the arrays: nothing is stored at or past them.
 *   - workspace >= wr_sgl_views_workspace_bytes(n_nodes, n_edges), 16-byte aligned.  n_edges, n_nodes in [1, 2^31); a size, a
 *     kind or an n_select outside its range, a NULL array or a short workspace is refused (WR_E_*) before any launch.
 *   - err_word (int32 on the device, may be NULL; the caller clears and reads it) receives bits for base arrays that
 *     contradict the contract (1 node id, 2 chunk table, 4 mirror, 8 degree past dis_tab, 16 scan past nnz); such an element is
 *     skipped or clamped, never addressed.
 *   - Deterministic: no float atomics, one writer per output element.  No allocation.
 *   Chunk tables of the load-balanced product (wr_spmm_csr_chunked*) for a device row_ptr int64 [n_rows + 1]:
 *   - wr_spmm_chunks_count: per[r] = max(1, ceil(deg_r / max_nnz)) int64 [n_rows]; max_per (int32, zeroed by the caller) receives
 *     the largest.  The caller scans per into chunk_first int64 [n_rows + 1] (exclusive; the last entry is n_chunks).
 *   - wr_spmm_chunks_fill: chunk_ptr int64 [n_chunks + 1] (chunk k of row r starts at row_ptr[r] + k max_nnz; the last entry is
 *     row_ptr[n_rows]) and chunk_row int32 [n_chunks]. */
#define WR_VIEW_EDGE_DROP 0
#define WR_VIEW_NODE_DROP 1
int64_t wr_sgl_views_workspace_bytes(int64_t n_nodes, int64_t n_edges);
int32_t wr_sgl_view_count(int32_t kind, const int32_t *rows, const int32_t *cols, const int32_t *mirror, int64_t n_edges,
                          int64_t n_nodes, const int64_t *bchunk_ptr, int64_t n_bchunks, int64_t n_select, uint64_t seed,
                          uint64_t stream_id0, uint64_t stream_id1, int32_t *cnt_fwd, int32_t *cnt_bwd, int32_t *err_word,
                          void *workspace, int64_t workspace_bytes, void *stream);
int32_t wr_sgl_view_rows(const int64_t *row_first_chunk, int64_t n_nodes, int64_t n_bchunks, const int64_t *scan_fwd,
                         const int64_t *scan_bwd, int64_t *row_ptr_fwd, int64_t *row_ptr_bwd, void *stream);
int32_t wr_sgl_view_fill(const int32_t *rows, const int32_t *cols, const int32_t *mirror, int64_t n_edges, int64_t n_nodes,
                         const int64_t *bchunk_ptr, int64_t n_bchunks, const int64_t *scan_fwd, const int64_t *scan_bwd,
                         const int64_t *row_ptr_fwd, const float *dis_tab, int64_t n_dis, int32_t *col_fwd, float *val_fwd,
                         int64_t nnz_fwd, int32_t *col_bwd, float *val_bwd, int64_t nnz_bwd, int32_t *err_word,
                         const void *workspace, int64_t workspace_bytes, void *stream);
int32_t wr_spmm_chunks_count(const int64_t *row_ptr, int64_t n_rows, int32_t max_nnz, int64_t *per, int32_t *max_per,
                             void *stream);
int32_t wr_spmm_chunks_fill(const int64_t *row_ptr, int64_t n_rows, int32_t max_nnz, const int64_t *chunk_first, int64_t n_chunks,
                            int64_t *chunk_ptr, int32_t *chunk_row, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K21  ContraRec's two augmented views of a batch of histories (ContraRec.Dataset.augment / mask_op / reorder_op, reference
 *      src/models/sequential/ContraRec.py:107-129) drawn on the device: the reference's distribution, not NumPy's stream.
 *   hist int64 [n_rows, T] left-aligned, zero-padded histories; lengths int64 [n_rows]; rows int64 [B], the dataset row ids of
 *   the batch (any order, repeats allowed); out_a / out_b int64 [B, T], the two views, 0 at every position t >= L.
 *   Per (row, view): with probability 1/2 mask, otherwise reorder; ratio ~ Beta(beta_a, beta_b), sel = int(L * ratio) in
 *   float64, truncated (sel <= L - 1).  mask: a uniform subset of sel of the L positions becomes mask_token.  reorder: start
 *   uniform on [0, L - sel], the window [start, start + sel) permuted uniformly (sel of 0 or 1 leaves the row unchanged).
 *   - Generator: counter-based on the splitmix64 finaliser, keyed by (seed, epoch, dataset row id, view) and a domain constant
 *     of its own; no state.  A row's views depend on neither the batch it arrives in nor its position there.
 *   - Beta(a, b) for integer a, b is the a-th smallest of a + b - 1 uniforms (exact); subset and permutation come from ranking
 *     64-bit position keys by (key, index) (exact up to key ties, 2^-64 per pair, broken by index); start is the high half of
 *     draw * (L - sel + 1), within 2^-58 (total variation) of uniform.
 *   - 1 <= T <= 64, beta_a, beta_b >= 1, beta_a + beta_b - 1 <= 15 (wr_seq_augment_supported); n_rows >= 1, 0 <= B < 2^31.  A
 *     NULL array, an unsupported shape or a size out of range is refused (WR_E_*) before any launch.
 *   - err_word (int32 on the device, may be NULL; the caller clears and reads it): bit 1 a length outside [1, T] (clamped before
 *     it bounds anything), bit 2 a row id outside [0, n_rows) (its two output rows are zeros).  Nothing is read out of bounds.
 *   - Deterministic: one writer per output element.  One launch, no workspace, no allocation, no host round trip. */
int32_t wr_seq_augment_supported(int32_t T, int32_t beta_a, int32_t beta_b);
int32_t wr_seq_augment(const int64_t *hist, const int64_t *lengths, int64_t n_rows, int32_t T, const int64_t *rows, int64_t B,
                       int64_t mask_token, int32_t beta_a, int32_t beta_b, uint64_t seed, uint64_t epoch, int64_t *out_a,
                       int64_t *out_b, int32_t *err_word, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K22  Row-lazy dense optimizers for a table whose gradient rows come from autograd — the item table of the sequential models
 *      (nn.Embedding lookups of src/models/sequential/SASRec.py:60,84,105-106 under torch.optim.Adam / SGD(weight_decay),
 *      src/helpers/BaseRunner.py:120-124,199).  K5 (lazy, exact) without the BPR step kernels: tab / exp_avg / exp_avg_sq /
 *      last_step / consts as there (last_step[r] = number of the last optimizer step applied to row r).
 *   - Gather: out[k,:] = row idx[k] as the dense optimizer holds it after step `upto` — the zero-gradient steps last_step[r]+1 ..
 *     upto are replayed in registers.  Nothing but `out` is written: duplicates in idx and concurrent readers are free.
 *   - Sparse step: sorted_rows int32 [n] = the step's row ids ascending (wr_rows_sparse_keys, then a STABLE sort by key), perm
 *     int64 [n] = the position of every entry in the concatenation of the step's lookups, src [n, D] the gradient rows in that
 *     order.  Per run of equal rows, one wave: g = src[perm[q],:] summed over the run in ascending q starting from +0 (the
 *     association of wr_scatter_add_rows into a zero table), replay of the row through step - 1, the step itself with g, then
 *     w / m / v and last_step[row] = step are written.  A run of padding_idx contributes no gradient but takes the step with
 *     g = 0 (SASRec gathers row 0 at every padded position: the row stays current).  wr_sgd_rows_sparse: l2 == 0: w -= lr*g on
 *     the rows with a gradient, last_step unused (may be NULL); l2 != 0: missed decays, then g' = g + l2*w; w -= lr*g'.
 *   - Same element arithmetic and order as wr_adam_dense / wr_sgd_dense: after wr_*_catchup_all the tables hold the bits of
 *     "zero table, wr_scatter_add_rows, wr_*_dense" repeated step by step.  One writer per row, no float atomics, no [n_rows, D]
 *     temporary.  Rows no step names are advanced by wr_*_catchup_all, whole or on a window (pointers offset to its first row).
 *   - idx int64; 0 <= n < 2^31; upto / step < n_consts.  An id outside [0, n_rows) is never dereferenced: the gather writes a
 *     zero row for it, wr_rows_sparse_keys gives it the key n_rows (sorted last, never applied); a perm entry outside [0, n)
 *     contributes nothing.  err_word (int32 on the device, may be NULL; the caller clears and reads it): bit 1 a row id
 *     outside the table, bit 2 a perm entry outside [0, n).  No workspace, no allocation, no host round trip. */
int32_t wr_gather_rows_lazy(const float *tab, const float *exp_avg, const float *exp_avg_sq, const int32_t *last_step,
                            int64_t n_rows, int32_t D, const int64_t *idx, int64_t n, int64_t upto, const float *consts,
                            int64_t n_consts, float l2, float beta1, float beta2, float eps, float *out, int32_t *err_word,
                            void *stream);
int32_t wr_gather_rows_lazy_sgd(const float *tab, const int32_t *last_step, int64_t n_rows, int32_t D, const int64_t *idx,
                                int64_t n, int64_t upto, float lr, float l2, float *out, int32_t *err_word, void *stream);
int32_t wr_rows_sparse_keys(const int64_t *idx, int64_t n, int64_t n_rows, int32_t *keys, int32_t *err_word, void *stream);
int32_t wr_adam_rows_sparse(float *tab, float *exp_avg, float *exp_avg_sq, int32_t *last_step, int64_t n_rows, int32_t D,
                            const int32_t *sorted_rows, const int64_t *perm, int64_t n, const float *src, int64_t padding_idx,
                            int64_t adam_step, const float *consts, int64_t n_consts, float l2, float beta1, float beta2,
                            float eps, int32_t *err_word, void *stream);
int32_t wr_sgd_rows_sparse(float *tab, int32_t *last_step, int64_t n_rows, int32_t D, const int32_t *sorted_rows,
                           const int64_t *perm, int64_t n, const float *src, int64_t padding_idx, int64_t step, float lr,
                           float l2, int32_t *err_word, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K24  K22 for a PAIR (online table `tab`, target table `target`) — BUIR's tables (src/models/general/BUIR.py:69-72): after every
 *      optimizer step the target follows by target = target*mom + tab*one_minus_mom (the arithmetic of wr_ema_update, K17).
 *      One last_step per row: last_step[r] = s means row r has had exactly s optimizer steps AND s target updates, in the dense
 *      order "step 1, update 1, step 2, update 2, ...".  The replay of one missed step is the zero-gradient optimizer step, then
 *      the target update with the row's new value; under SGD with l2 == 0 the online row stays and the target still moves.
 *   - Gather: out_tab[k,:] / out_target[k,:] = row idx[k] of both tables as of step `upto`; nothing else is written.
 *   - Sparse step: sorted_rows / perm / src as for K22 (wr_rows_sparse_keys + a stable sort); no padding row.  Per run of equal
 *     rows, one wave: the run's sum (ascending position, from +0), replay through step - 1, the step with the sum, the target
 *     update of that step, then tab, (exp_avg, exp_avg_sq,) target and last_step[row] = step are written.
 *   - Catch-up: rows [0, n_rows) of the arrays handed in (pointers offset to a window's first row) up to the given step.
 *   - After a catch-up of the whole table, tab / exp_avg / exp_avg_sq / target hold the bits of "zero table, wr_scatter_add_rows,
 *     wr_adam_dense / wr_sgd_dense, wr_ema_update" repeated step by step.  One writer per row, no float atomics, no [n_rows, D]
 *     temporary, no workspace, no allocation, no host round trip.
 *   - tab, target, exp_avg, exp_avg_sq: 16-byte aligned, 0 < n_rows < 2^31, D a multiple of 4 in [4, 1024] (as K22; the tests
 *     cover 20, 64 and 128); idx int64, 0 <= n < 2^31; upto / step < n_consts (Adam); mom, one_minus_mom in [0, 1].  Anything else
 *     is refused (WR_E_*) before any launch.  err_word (int32 on the device, may be NULL; the caller clears and reads it): bit 1
 *     a row id outside [0, n_rows) — never dereferenced: the gather writes two zero rows, the step skips it —, bit 2 a perm
 *     entry outside [0, n) (contributes nothing). */
int32_t wr_gather_rows_ema(const float *tab, const float *target, const float *exp_avg, const float *exp_avg_sq,
                           const int32_t *last_step, int64_t n_rows, int32_t D, const int64_t *idx, int64_t n, int64_t upto,
                           const float *consts, int64_t n_consts, float l2, float beta1, float beta2, float eps, float mom,
                           float one_minus_mom, float *out_tab, float *out_target, int32_t *err_word, void *stream);
int32_t wr_gather_rows_ema_sgd(const float *tab, const float *target, const int32_t *last_step, int64_t n_rows, int32_t D,
                               const int64_t *idx, int64_t n, int64_t upto, float lr, float l2, float mom, float one_minus_mom,
                               float *out_tab, float *out_target, int32_t *err_word, void *stream);
int32_t wr_adam_rows_sparse_ema(float *tab, float *target, float *exp_avg, float *exp_avg_sq, int32_t *last_step, int64_t n_rows,
                                int32_t D, const int32_t *sorted_rows, const int64_t *perm, int64_t n, const float *src,
                                int64_t adam_step, const float *consts, int64_t n_consts, float l2, float beta1, float beta2,
                                float eps, float mom, float one_minus_mom, int32_t *err_word, void *stream);
int32_t wr_sgd_rows_sparse_ema(float *tab, float *target, int32_t *last_step, int64_t n_rows, int32_t D,
                               const int32_t *sorted_rows, const int64_t *perm, int64_t n, const float *src, int64_t step, float lr,
                               float l2, float mom, float one_minus_mom, int32_t *err_word, void *stream);
int32_t wr_adam_catchup_ema(float *tab, float *target, float *exp_avg, float *exp_avg_sq, int32_t *last_step, int64_t n_rows,
                            int32_t D, int64_t adam_step, const float *consts, int64_t n_consts, float l2, float beta1,
                            float beta2, float eps, float mom, float one_minus_mom, void *stream);
int32_t wr_sgd_catchup_ema(float *tab, float *target, int32_t *last_step, int64_t n_rows, int32_t D, int64_t step, float lr,
                           float l2, float mom, float one_minus_mom, void *stream);

/* LightGCN.predict's per-batch tail in two launches (src/models/general/LightGCN.py:156-175, src/utils/loss.py:37-39,94-98):
 *   loss[0] = mean_b( -log(1e-10 + sigmoid(<Ua[u_b], Ia[p_b]> - <Ua[u_b], Ia[n_b]>)) )
 *             + reg_weight * (||U0[u]||_F + ||I0[p]||_F + ||I0[n]||_F) / B
 * with Ua / Ia the propagated tables and U0 / I0 the ego tables; sq3[3] receives the three sums of squares (the backward pass
 * needs them: wr_embloss_grad).  Partials are folded in a fixed order: bitwise reproducible. */
int64_t wr_lightgcn_loss_workspace_bytes(int64_t B);
int32_t wr_lightgcn_loss(const float *user_all, const float *item_all, const float *user_ego, const float *item_ego,
                         int64_t n_users, int64_t n_items, int32_t D, const int64_t *u, const int64_t *p, const int64_t *n,
                         int64_t B, float reg_weight, float *loss, float *sq3, void *workspace, int64_t workspace_bytes,
                         void *stream);
/* Backward of EmbLoss for one planned batch: grad_user[u,:] += m_u * w/(B*sqrt(sq3[0])) * user_tab[u,:] for a user with m_u
 * triplets in the batch; grad_item[r,:] += (m_pos * w/(B*sqrt(sq3[1])) + m_neg * w/(B*sqrt(sq3[2]))) * item_tab[r,:].
 * tu / oc_item / oc_src are the plan arrays of that batch (oc_item must hold plain row ids), sq3 the device output of
 * wr_embloss_sumsq: no host round trip. */
int32_t wr_embloss_grad(const float *user_tab, const float *item_tab, int32_t D, const int32_t *tu, const int32_t *oc_item,
                        const int32_t *oc_src, int64_t B, const float *sq3, float reg_weight, float *grad_user,
                        float *grad_item, void *stream);

/* LightGCN.predict + its backward as ONE call (src/models/general/LightGCN.py:134-175; loss.backward() of
 * src/helpers/BaseRunner.py:198): propagation of cat(user_tab, item_tab) through `n_layers` products with the chunked CSR
 * adjacency (layer mean folded in; `levels` as for wr_spmm_csr_chunked_levels), BPR + reg_weight * EmbLoss -> loss[0] (shape
 * (1,) like the reference's), and the dense gradient of that loss w.r.t. both tables -> grad [n_users + n_items, D] (user
 * rows first).  The same kernels, in the same order, that the separate entry points run: same bits.  B <=
 * wr_bprmf_plan_small_max_batch().  trusted_indices != 0: u / p / n were range-checked by the caller (no error flag is
 * written); else err_flag[0] != 0 reports an id out of range.  No host round trip: capturable into a hipGraph. */
int64_t wr_lightgcn_step_workspace_bytes(int64_t n_users, int64_t n_items, int32_t D, int64_t n_chunks, int64_t B);
int32_t wr_lightgcn_step(const float *user_tab, const float *item_tab, int64_t n_users, int64_t n_items, int32_t D,
                         int64_t n_chunks, const int64_t *chunk_ptr, const int32_t *chunk_row, const int32_t *col,
                         const float *val, int32_t levels, int32_t n_layers, const int64_t *u, const int64_t *p, const int64_t *n,
                         int64_t B, float reg_weight, int32_t trusted_indices, float *loss, float *grad, int32_t *err_flag,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K25 — time-interval attention (reference src/utils/layers.py:105-146 after the projections), forward and backward, without
 * the gathered [B, T, T, D] arrays.  q, k, v fp32 [B, T, D] (position terms already added to k and v), times int64 [B, T],
 * min_interval int64 [B], time_k / time_v fp32 [time_max + 1, D]; head h owns columns h d_k .. (h + 1) d_k - 1; for j <= i:
 *   r_ij = min(|t_i - t_j| / m_b, time_max)   (64-bit integer division)      s_ij = <q_i, k_j + time_k[r_ij]> / sqrt(d_k)
 *   p_i. = softmax_j s_i.                                                      out_i = sum_j p_ij (v_j + time_v[r_ij])
 *   - Supported (wr_ti_attention_supported): D in {32, 64}, n_heads in {1, 2, 4} with D / n_heads >= 8, 1 <= T <= 64,
 *     1 <= time_max <= 2048 (the intervals are 12-bit fields of the backward's sort keys), 1 <= B <= 2^24.  Anything else, a
 *     NULL or misaligned (16 B) pointer or a short workspace is refused (WR_E_*) with the numbers before any launch.
 *   - The softmax subtracts each row's own maximum, not the reference's maximum over the whole call: equal wherever the
 *     reference is finite; where a row's shifted exponentials all underflow the reference gives NaN, this the plain softmax.
 *   - wr_ti_attention_fwd: one launch; nothing with T^2 elements per sequence is written to memory.
 *   - wr_ti_attention_bwd: g_out [B, T, D] -> gq, gk, gv [B, T, D], g_time_k, g_time_v [time_max + 1, D], all fully written.
 *     The forward is recomputed.  Two launches: every workgroup orders the pairs of a sequence by (r, i, j) in LDS, sums each
 *     run of equal r in that order and adds it to its own slab [2][time_max + 1][D] of the workspace (sequences w, w + G, ...,
 *     G = min(B, 256)); the second launch folds the slabs in workgroup order.  No float atomics: same inputs, same bits.
 *   - min_interval[b] < 1 is clamped to 1 and ORs 1 into err_word (int32 on the device, may be NULL; the caller clears and
 *     reads it).
 *   - workspace >= wr_ti_attention_workspace_bytes(B, T, D, n_heads, time_max), 16-byte aligned (backward only): 256 slabs,
 *     independent of B and T.  No host round trip, no allocation. */
int32_t wr_ti_attention_supported(int32_t D, int32_t n_heads, int32_t T, int32_t time_max);
int64_t wr_ti_attention_workspace_bytes(int64_t B, int32_t T, int32_t D, int32_t n_heads, int32_t time_max);
int32_t wr_ti_attention_fwd(const float *q, const float *k, const float *v, const int64_t *times, const int64_t *min_interval,
                            int64_t B, int32_t T, int32_t D, int32_t n_heads, const float *time_k, const float *time_v,
                            int32_t time_max, float *out, int32_t *err_word, void *stream);
int32_t wr_ti_attention_bwd(const float *q, const float *k, const float *v, const int64_t *times, const int64_t *min_interval,
                            int64_t B, int32_t T, int32_t D, int32_t n_heads, const float *time_k, const float *time_v,
                            int32_t time_max, const float *g_out, float *gq, float *gk, float *gv, float *g_time_k,
                            float *g_time_v, int32_t *err_word, void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K26  Softmax cross-entropy of B query rows against the whole item table, loss and both gradients, without the
 *      [B, n_items] logit matrix (whisprrec_amd/softmax_loss.py, --train_loss softmax --softmax_native 1), fp32.
 *      Q [B, D] queries, E [n_items, D] item table, target [B] int64; the classes are the items first_class .. n_items - 1
 *      (first_class = 1: item 0 is padding and no class):
 *   s_bj  = <Q[b], E[j]>                                  (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain started at 0)
 *   loss  = (accumulate ? loss : 0) + weight * sum_b ( log sum_j exp(s_bj) - s_b,target_b )
 *   gQ[b] = weight * ( sum_j p_bj E[j] - E[target_b] )                p_bj = exp(s_bj) / sum_j' exp(s_bj')
 *   gE[j] = weight * sum_b ( p_bj - [j == target_b] ) Q[b]            for j >= first_class; rows below are written as zeros
 *   - The log-sum-exp subtracts the row's true maximum and is exact for any finite scores; the maximum and the shifted
 *     sum are kept apart, so a row with scores of size 150 loses no more bits than one with scores of size 1.
 *   - weight = 1 / B gives the mean.  gQ == gE == NULL: loss only, the same loss bits.  gQ [B, D] and gE [n_items, D] are
 *     fully written; a target named by many rows costs nothing extra (no owner table, no scatter, no memset).
 *   - Determinism: no float atomics.  Item chunks and query chunks go to partials folded in chunk order, the loss terms in
 *     a fixed order.  Same inputs, same bits — loss, gQ and gE.
 *   - Bad targets: a target outside [first_class, n_items) is clamped to the nearest class, never dereferenced, and
 *     err_word[0] |= 1 (err_word may be NULL; the caller clears it).
 *   - D in {32, 64, 128} (wr_softmax_ce_supported); any other value, first_class outside [0, n_items), a NULL or misaligned
 *     (16 B) pointer or a short workspace is refused before a launch.
 *   - workspace >= wr_softmax_ce_workspace_bytes(n_items, B, D), 16-byte aligned.  The bound grows with max(n_items, B) * D
 *     and a fixed number of [row, D] chunk partials — never with B * n_items — and never decreases as n_items or B grow.
 *   - No host round trip, no allocation: capturable into a hipGraph. */
int32_t wr_softmax_ce_supported(int32_t D);
int64_t wr_softmax_ce_workspace_bytes(int64_t n_items, int64_t B, int32_t D);
int32_t wr_softmax_ce_loss_grad(const float *Q, int64_t B, const float *E, int64_t n_items, int32_t D, const int64_t *target,
                                int64_t first_class, float weight, float *loss, int32_t accumulate, float *gQ, float *gE,
                                int32_t *err_word, void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K27 — one-layer GRU over left-aligned, zero-padded histories with a length per row (whisprrec_amd/gru4rec.py, --gru_native 1),
 * forward and backward, fp32.  x [B, T, E], lengths int64 [B], w_ih [3H, E], w_hh [3H, H], b_ih, b_hh [3H]; torch's cell and
 * gate order (r, z, n), h_0 = 0:
 *   r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)      z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
 *   n = tanh(W_in x + b_in + r * (W_hn h + b_hn))   h' = (1 - z) * n + z * h
 *   - Row b takes its first len_b = min(max(lengths[b], 0), T) steps and is frozen afterwards: h_last[b] [H] is its state after
 *     step len_b - 1.  A length of 0 (or below) gives h_last[b] = 0 and no gradient from that row; a length above T acts as T.
 *     x[b, t, :] is never read for t >= len_b (it may hold anything, NaN included).
 *   - Supported (wr_gru_supported): E, H in {32, 64} in any combination, T >= 1 without an upper limit (x_t is streamed),
 *     1 <= B <= 2^24.  Anything else, a NULL or misaligned (16 B) pointer or a short workspace is refused (WR_E_*) with the
 *     numbers before any launch.
 *   - wr_gru_fwd: one launch; both weight matrices and the h of a 16-row tile stay on chip for the whole walk.  hs != NULL:
 *     every step's h_t is stored to hs [B, T, H] (the frozen value for t >= len_b), the one activation wr_gru_bwd reads;
 *     hs == NULL (inference): nothing but h_last is written.
 *   - wr_gru_bwd: g_last [B, H] -> gx [B, T, E] (exactly zero for t >= len_b), g_w_ih, g_w_hh, g_b_ih, g_b_hh, all fully
 *     written.  The gates are recomputed from x_t and hs[t - 1].  Two launches: the reverse walk keeps the parameter gradients of
 *     its tiles (tiles w, w + G, ..., G = min(ceil(B / 16), 256)) in registers across all t and writes them once to its own slab
 *     of the workspace; the second launch folds the slabs in workgroup order.  No float atomics: same inputs, same bits.
 *   - workspace >= wr_gru_workspace_bytes(B, T, E, H), 16-byte aligned (backward only): 256 slabs of 3H (E + H) + 6H floats,
 *     independent of B and T.  No host round trip, no allocation. */
int32_t wr_gru_supported(int32_t E, int32_t H, int32_t T);
int64_t wr_gru_workspace_bytes(int64_t B, int32_t T, int32_t E, int32_t H);
int32_t wr_gru_fwd(const float *x, const int64_t *lengths, const float *w_ih, const float *w_hh, const float *b_ih,
                   const float *b_hh, int64_t B, int32_t T, int32_t E, int32_t H, float *h_last, float *hs, void *stream);
int32_t wr_gru_bwd(const float *x, const int64_t *lengths, const float *w_ih, const float *w_hh, const float *b_ih,
                   const float *b_hh, const float *hs, const float *g_last, int64_t B, int32_t T, int32_t E, int32_t H, float *gx,
                   float *g_w_ih, float *g_w_hh, float *g_b_ih, float *g_b_hh, void *workspace, int64_t workspace_bytes,
                   void *stream);

/* K27, the whole output sequence (hip_ops.gru_seq: NARM's local encoder, the lower layers of a stacked GRU4Rec).  The same
 * walk, shapes, refusals and workspace as wr_gru_fwd / _bwd; compile-time variants of the same kernels.
 *   - wr_gru_seq_fwd: hs [B, T, H] is the result: every step's state for t < len_b and EXACTLY ZERO for t >= len_b
 *     (pad_packed_sequence's form, not the frozen state wr_gru_fwd stores).  For t < len_b the bits are wr_gru_fwd's.
 *   - wr_gru_seq_bwd: hs as wr_gru_seq_fwd wrote it; g_hs [B, T, H] enters at every step: g_hs[b, t, :] is added to dh before
 *     step t's gate gradients, for t < len_b only; g_hs[b, t, :] is never read for t >= len_b.  g_last [B, H] (may be NULL:
 *     none) is a gradient of the state after step len_b - 1 on top.  Outputs, launches and reproducibility as wr_gru_bwd. */
int32_t wr_gru_seq_fwd(const float *x, const int64_t *lengths, const float *w_ih, const float *w_hh, const float *b_ih,
                       const float *b_hh, int64_t B, int32_t T, int32_t E, int32_t H, float *hs, void *stream);
int32_t wr_gru_seq_bwd(const float *x, const int64_t *lengths, const float *w_ih, const float *w_hh, const float *b_ih,
                       const float *b_hh, const float *hs, const float *g_hs, const float *g_last, int64_t B, int32_t T, int32_t E,
                       int32_t H, float *gx, float *g_w_ih, float *g_w_hh, float *g_b_ih, float *g_b_hh, void *workspace,
                       int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K28 — NARM's additive attention pooling (whisprrec_amd/narm.py, --pool_native 1), forward and backward, fp32.
 * hs [B, T, H], h_g [B, H], lengths int64 [B], A1, A2 [A, H], v [A]; for row b, len = min(max(lengths[b], 0), T):
 *   q = A1 h_g[b]     u_t = q + A2 hs[b, t]     e_t = v . sigmoid(u_t)     c[b] = sum_{t < len} e_t hs[b, t]      (no softmax)
 *   - len = 0 gives c[b] = 0 and no gradient from the row.  hs[b, t, :] is never read for t >= len.
 *   - Supported (wr_narm_pool_supported): H in {32, 64}, A in {16, 32, 64}, T >= 1, 1 <= B <= 2^24.  Anything else, a NULL or
 *     misaligned (16 B: hs, A1, A2) pointer or a short workspace is refused (WR_E_*) with the numbers before any launch.
 *   - wr_narm_pool_fwd: one launch, c [B, H]; A1, A2 and v stay in LDS; nothing is kept for the backward.
 *   - wr_narm_pool_bwd: g_c [B, H] -> g_hs [B, T, H] (exactly zero for t >= len, every element written), g_h_g [B, H], g_A1,
 *     g_A2 [A, H], g_v [A], all fully written.  sigmoid(u_t) is recomputed; no [B, T, A] array in memory.  Two launches: each
 *     wave keeps the parameter gradients of its rows in registers and writes one slab; the second launch folds the slabs in
 *     (workgroup, wave) order.  No float atomics: same inputs, same bits.
 *   - workspace >= wr_narm_pool_workspace_bytes(B, T, H, A), 16-byte aligned (backward only): 256 slabs of 2 A H + A floats,
 *     independent of B and T. */
int32_t wr_narm_pool_supported(int32_t H, int32_t A, int32_t T);
int64_t wr_narm_pool_workspace_bytes(int64_t B, int32_t T, int32_t H, int32_t A);
int32_t wr_narm_pool_fwd(const float *hs, const float *h_g, const int64_t *lengths, const float *A1, const float *A2, const float *v,
                         int64_t B, int32_t T, int32_t H, int32_t A, float *c, void *stream);
int32_t wr_narm_pool_bwd(const float *hs, const float *h_g, const int64_t *lengths, const float *A1, const float *A2, const float *v,
                         const float *g_c, int64_t B, int32_t T, int32_t H, int32_t A, float *g_hs, float *g_h_g, float *g_A1,
                         float *g_A2, float *g_v, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WHISPRREC_HIP_H */
