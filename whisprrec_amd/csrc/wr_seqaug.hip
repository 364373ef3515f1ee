// wr_seqaug.hip — K21: ContraRec's two augmented views of every history of a batch, drawn on the device.
//
// Device counterpart of ContraRec.Dataset.augment / mask_op / reorder_op (reference src/models/sequential/ContraRec.py:107-129,
// whisprrec_amd/contrarec.py restates them on the host): per (row, view), with probability 1/2 mask, otherwise reorder; both
// draw ratio ~ Beta(a, b) and take sel = int(L * ratio) in float64, truncated.  mask: a uniform subset of sel of the L positions
// becomes mask_token.  reorder: start uniform on [0, L - sel], the window [start, start + sel) permuted uniformly.  The same
// distribution, NOT NumPy's stream.
//
// Generator: counter-based on mix64, no state.  key_epoch = mix64(mix64(seed ^ epoch * 0x9E3779B97F4A7C15) ^ kAugDomain) (the
// domain constant keeps these values apart from the epoch shuffle's and the negative sampler's, which start from the same
// (seed, epoch) word), key = mix64(key_epoch ^ ((2 row + view) * 0xD1B54A32D192ED03 + 1)) with the DATASET row id, and
// draw(c) = mix64(key + (c + 1) * 0x9E3779B97F4A7C15): a row's views depend on (seed, epoch, row, view) alone, never on the
// batch.  Counters: 0 the op (unit > 0.5 -> mask, as `np.random.rand() > 0.5`), 1 .. a + b - 1 the uniforms of the Beta draw,
// 16 + t the key of position t, 80 the start.  unit(d) = (d >> 11) * 2^-53 in double.
//   Beta     exact for integer a, b: the a-th smallest of a + b - 1 iid U(0, 1) is Beta(a, b).  Lane l < a + b - 1 holds uniform l,
//            ranks it by (value, index) against the others, and the lane of rank a - 1 broadcasts its value.
//   subset / permutation   every position gets a 64-bit key; positions are ranked by (key, index) inside [0, L) (mask) or inside
//            the window (reorder).  iid keys with a fixed tie-break rank as a uniform permutation, so "rank < sel" is a uniform
//            sel-subset and out[t] = src[start + rank(t)] a uniform permutation of the window — at every size, which the Feistel
//            bijection of wr_shuffle.h is not on 2 to 8 elements.
//   start    the high 64 bits of draw * (L - sel + 1): every value's probability is within 2^-64 of 1 / (L - sel + 1), the total
//            variation from uniform below 65 * 2^-65 < 2^-58.
// Shape: T <= 64, one 64-lane wave per row, lane = position, both views in turn; four rows per workgroup.  The two rank loops
// read other lanes' registers with __shfl (at most 15 + 64 iterations of one or two ds_bpermute): no LDS, no barrier, no
// atomics but the error word.  Every output element is written by exactly one lane: same arguments, same bits.
// A length outside [1, T] is clamped before it bounds anything (err bit 1); a row id outside [0, n_rows) gives a zero row (err
// bit 2).  hist is read at [row, t] for t < min(L, T) only.
#include "wr_common.h"

namespace wr {

constexpr uint64_t kAugDomain = 0x5345514155473231ull;      // "SEQAUG21"
constexpr int kAugMaxT = 64;
constexpr int kAugMaxUniforms = 15;                         // a + b - 1
constexpr int kAugKeyCounter = 16;                          // + position
constexpr int kAugStartCounter = kAugKeyCounter + kAugMaxT;
constexpr int kAugRowsPerBlock = kBlock / 64;

__host__ __device__ __forceinline__ uint64_t aug_draw(uint64_t key, uint64_t counter) {
    return mix64(key + (counter + 1ull) * 0x9E3779B97F4A7C15ull);
}
__device__ __forceinline__ double aug_unit(uint64_t draw) { return (double)(draw >> 11) * 0x1.0p-53; }

static inline bool seq_augment_ok(int32_t T, int32_t a, int32_t b) {
    return T >= 1 && T <= kAugMaxT && a >= 1 && b >= 1 && a <= kAugMaxUniforms && b <= kAugMaxUniforms &&
           a + b - 1 <= kAugMaxUniforms;
}

__global__ __launch_bounds__(kBlock) void seq_augment_kernel(const int64_t *__restrict__ hist, const int64_t *__restrict__ lengths,
                                                              int64_t n_rows, int T, const int64_t *__restrict__ rows, int64_t B,
                                                              int64_t mask_token, int beta_a, int n_unif, uint64_t key_epoch,
                                                              int64_t *__restrict__ out_a, int64_t *__restrict__ out_b,
                                                              int32_t *__restrict__ err) {
    const int64_t b = (int64_t)blockIdx.x * kAugRowsPerBlock + (threadIdx.x >> 6);      // wave-uniform
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const bool in_T = lane < T;
    const int64_t row = rows[b];
    if (row < 0 || row >= n_rows) {
        if (lane == 0 && err) atomicOr(err, 2);
        if (in_T) {
            out_a[b * T + lane] = 0;
            out_b[b * T + lane] = 0;
        }
        return;
    }
    const int64_t len_raw = lengths[row];
    if ((len_raw < 1 || len_raw > T) && lane == 0 && err) atomicOr(err, 1);
    const int L = len_raw < 1 ? 1 : (len_raw > T ? T : (int)len_raw);
    const int64_t item = lane < L ? hist[row * T + lane] : 0;
    for (int view = 0; view < 2; ++view) {
        const uint64_t key = mix64(key_epoch ^ (((uint64_t)row * 2ull + (uint64_t)view) * 0xD1B54A32D192ED03ull + 1ull));
        const bool do_mask = aug_unit(aug_draw(key, 0)) > 0.5;
        // ratio ~ Beta(a, b): the a-th smallest of the n_unif uniforms held by lanes 0 .. n_unif - 1
        const double u = aug_unit(aug_draw(key, 1 + (lane < n_unif ? lane : 0)));
        int u_rank = 0;
        for (int j = 0; j < n_unif; ++j) {
            const double uj = __shfl(u, j, 64);
            u_rank += (uj < u || (uj == u && j < lane)) ? 1 : 0;
        }
        const unsigned long long hit = __ballot(lane < n_unif && u_rank == beta_a - 1);
        const int holder = hit ? __ffsll(hit) - 1 : 0;                               // exactly one lane holds rank a - 1
        const double ratio = __shfl(u, holder, 64);
        const int sel = (int)((double)L * ratio);                                    // <= L - 1: ratio <= 1 - 2^-53
        const int start = (int)__umul64hi(aug_draw(key, kAugStartCounter), (uint64_t)(L - sel + 1));
        const int lo = do_mask ? 0 : start, hi = do_mask ? L : start + sel;          // the positions ranked against each other
        const uint64_t k = aug_draw(key, kAugKeyCounter + lane);
        int rank = 0;
        for (int j = lo; j < hi; ++j) {
            const uint64_t kj = __shfl(k, j, 64);
            rank += (kj < k || (kj == k && j < lane)) ? 1 : 0;
        }
        int64_t v;
        if (do_mask) {
            v = (lane < L && rank < sel) ? mask_token : item;
        } else {
            const int from = (lane >= lo && lane < hi) ? start + rank : lane;
            v = __shfl(item, from, 64);
        }
        if (in_T) (view == 0 ? out_a : out_b)[b * T + lane] = v;
    }
}

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_seq_augment_supported(int32_t T, int32_t beta_a, int32_t beta_b) { return seq_augment_ok(T, beta_a, beta_b) ? 1 : 0; }

int32_t wr_seq_augment(const int64_t *hist, const int64_t *lengths, int64_t n_rows, int32_t T, const int64_t *rows, int64_t B,
                       int64_t mask_token, int32_t beta_a, int32_t beta_b, uint64_t seed, uint64_t epoch, int64_t *out_a,
                       int64_t *out_b, int32_t *err_word, void *stream) {
    WR_REQUIRE(hist && lengths && rows && out_a && out_b, WR_E_NULL, "wr_seq_augment: NULL argument");
    WR_REQUIRE(seq_augment_ok(T, beta_a, beta_b), WR_E_RANGE,
               "wr_seq_augment: T=%d, beta=(%d, %d) not supported (1 <= T <= %d, a, b >= 1, a + b - 1 <= %d)", (int)T, (int)beta_a,
               (int)beta_b, kAugMaxT, kAugMaxUniforms);
    WR_REQUIRE(n_rows >= 1 && n_rows < (int64_t(1) << 40) && B >= 0 && B < (int64_t(1) << 31), WR_E_SHAPE,
               "wr_seq_augment: n_rows=%lld, B=%lld out of range", (long long)n_rows, (long long)B);
    if (B == 0) return WR_OK;
    const uint64_t key_epoch = mix64(mix64(seed ^ (epoch * 0x9E3779B97F4A7C15ull)) ^ kAugDomain);
    const unsigned blocks = (unsigned)((B + kAugRowsPerBlock - 1) / kAugRowsPerBlock);
    hipLaunchKernelGGL(seq_augment_kernel, dim3(blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), hist, lengths,
                       n_rows, (int)T, rows, B, mask_token, (int)beta_a, (int)(beta_a + beta_b - 1), key_epoch, out_a, out_b,
                       err_word);
    WR_LAUNCH_CHECK("seq_augment_kernel");
    return WR_OK;
}

}  // extern "C"
