// wr_softmax.hip — K26: softmax cross-entropy of B query rows against the whole item table, loss and both gradients, without
// the [B, n_items] logit matrix.
//
// What it restates (the stock lines of whisprrec_amd/softmax_loss.py, --softmax_native 0):
//     logits = Q @ E.t();  logits[:, :first_class] = -inf;  loss = weight * sum_b cross_entropy(logits[b], target[b])
// Raw dot products are unbounded, so unlike K12 a true maximum is carried: the scores exist only as 32x32 accumulator tiles of
// v_mfma_f32_32x32x2_f32 (the k-ordered chain of wr_score_tiles.h) inside the streamed pair pass of wr_pair_pass.h.
//
//   pass 0      128 queries per workgroup resident, 64-row item tiles streamed.  Every lane keeps a running (max, sum exp) of
//               the scores it sees and rescales its sum when a larger score arrives; the two half-waves fold at the end; one
//               (m, z) pair per (query, item chunk).  No gradient product: this pass is the whole loss-only path
//   rows        per query: the chunk pairs merged in chunk order -> m_b, 1 / Z_b (Z_b = sum_j exp(s_bj - m_b)); the target is
//               clamped into [first_class, n_items) and reported; loss term (m_b - s_b,target) + log Z_b.  m_b and Z_b stay
//               apart: folded into one float lse_b, every probability would inherit the rounding of a number of size |m_b|
//   loss        the B terms folded by one workgroup in a fixed order (pair_loss_kernel)
//   pass 1      queries resident again: w_bj = exp(s_bj - m_b) / Z_b - [j == target_b], gQ partials = sum_j w_bj E[j] on the
//               matrix cores (the transposed score tile is already the A operand)
//   pass 2      128 items resident, queries streamed with (m_i, 1 / Z_i, target_i) beside every tile:
//               w_ij = exp(s - m_i) / Z_i - [e == target_i], gE partials = sum_i w_ij Q[i]
//   folds       chunk partials summed in chunk order, scaled by weight, every row of gQ and gE written once
// The positive term rides in the weight of its own pair: no owner table, no duplicate list, no scatter, no memset, and a
// target named many times costs nothing extra.  Items below first_class and streamed rows past a chunk's end weigh 0, so
// rows j < first_class of gE come out as exact zeros.
// No float atomics anywhere: every sum has a fixed order, the results are bitwise reproducible.  No host round trip.
#include "wr_pair_pass.h"

namespace wr {

constexpr int64_t kSmxTargetWg = 1024;    // workgroups a pass aims at when it splits the streamed side into chunks (K12's)
constexpr float kLog2e = 1.44269504088896341f;
constexpr float kNegInf = -__builtin_huge_valf();

// exp(d) for d <= 0 (and 0 for d = -inf): the difference is formed before the scaling, so a pair near the maximum keeps its bits
__device__ __forceinline__ float smx_exp(float d) { return __builtin_amdgcn_exp2f(d * kLog2e); }

// ------------------------------------------------------------------------------------------------ pass 0: (max, sum exp)
// The policies are local structs of their kernels (wr_pair_pass.h says why).
template <int KS, int TS>
__global__ __launch_bounds__(kBlock, 2) void smx_lse_pass_kernel(const float *__restrict__ Q, int64_t B, const float *__restrict__ E,
                                                                int64_t n, int first_class, int64_t chunk_rows,
                                                                float *__restrict__ mpart, float *__restrict__ zpart) {
    struct Policy {
        int first_class;
        float *__restrict__ mpart;
        float *__restrict__ zpart;
        int c1 = 0;
        float m = kNegInf, z = 0.f;

        __device__ __forceinline__ void start(int64_t, int64_t, int64_t c1_) { c1 = (int)c1_; }
        __device__ __forceinline__ void fetch_side(int64_t, bool) {}
        __device__ __forceinline__ void deposit_side(int) {}
        __device__ __forceinline__ float weight(float s, int tr, int64_t j0, int64_t, int) {
            const int j = (int)j0 + tr;
            if (j >= first_class && j < c1) {
                if (s > m) {                                             // rare after the first tiles; exp(-inf) = 0 starts it
                    z *= smx_exp(m - s);
                    m = s;
                }
                z += smx_exp(s - m);
            }
            return s;
        }
        __device__ __forceinline__ void finish(int64_t e, int64_t nr, int half) {
            const float mo = __shfl_xor(m, 32, 64), zo = __shfl_xor(z, 32, 64);
            const float M = fmaxf(m, mo);
            const float f = (M == kNegInf) ? 0.f : M;                    // a chunk with no class: (-inf, 0), no NaN on the way
            if (half == 0 && e < nr) {                                   // half-wave 0's term first
                mpart[(int64_t)blockIdx.y * nr + e] = M;
                zpart[(int64_t)blockIdx.y * nr + e] = z * smx_exp(m - f) + zo * smx_exp(mo - f);
            }
        }
    } P{first_class, mpart, zpart};
    pair_pass<KS, TS, false>(P, Q, B, E, n, chunk_rows, nullptr);
}

// ------------------------------------------------------------------------------------------------ rows
// Per query, a team of 16 lanes: merge the chunk pairs in chunk order, clamp the target, the loss term
__global__ __launch_bounds__(kBlock) void smx_row_kernel(int64_t B, int D, int64_t n, int first_class, int64_t chunks,
                                                         const float *__restrict__ mpart, const float *__restrict__ zpart,
                                                         const float *__restrict__ Q, const float *__restrict__ E,
                                                         const int64_t *__restrict__ target, float *__restrict__ mrow,
                                                         float *__restrict__ invz, int *__restrict__ ctgt,
                                                         float *__restrict__ lterm, int32_t *__restrict__ err_word) {
    const int64_t t = (int64_t)blockIdx.x * kNceTeamsPerBlock + (threadIdx.x / kNceTeam);
    const int l = threadIdx.x & (kNceTeam - 1);
    const bool live = t < B;
    const int64_t b = live ? t : 0;
    float M = kNegInf;
    for (int64_t c = 0; c < chunks; ++c) M = fmaxf(M, mpart[c * B + b]);
    float Z = 0.f;
    for (int64_t c = 0; c < chunks; ++c) Z += zpart[c * B + b] * expf(mpart[c * B + b] - M);    // chunk order
    int64_t id = target[b];
    const bool bad = id < (int64_t)first_class || id >= n;
    if (bad) id = id < (int64_t)first_class ? (int64_t)first_class : n - 1;     // never dereferenced out of range
    const float pos = nce_dot(nce_load(Q + b * (int64_t)D, D / 4, l), nce_load(E + id * (int64_t)D, D / 4, l));
    if (live && l == 0) {
        if (bad && err_word != nullptr) atomicOr(err_word, 1);
        mrow[b] = M;
        invz[b] = 1.0f / Z;
        ctgt[b] = (int)id;
        lterm[b] = (M - pos) + logf(Z);                                  // log sum_j exp(s_bj) - s_b,target
    }
}

// ------------------------------------------------------------------------------------------------ pass 1: queries resident
template <int KS, int TS>
__global__ __launch_bounds__(kBlock, 2) void smx_q_pass_kernel(const float *__restrict__ Q, int64_t B, const float *__restrict__ E,
                                                              int64_t n, int first_class, const float *__restrict__ mrow,
                                                              const float *__restrict__ invz, const int *__restrict__ ctgt,
                                                              int64_t chunk_rows, float *__restrict__ part) {
    struct Policy {
        int first_class;
        const float *__restrict__ mrow;
        const float *__restrict__ invz;
        const int *__restrict__ ctgt;
        int c1 = 0, tg = -1;
        float mm = 0.f, iz = 0.f;

        __device__ __forceinline__ void start(int64_t e, int64_t nr, int64_t c1_) {
            c1 = (int)c1_;
            if (e < nr) {
                mm = mrow[e];
                iz = invz[e];
                tg = ctgt[e];
            }
        }
        __device__ __forceinline__ void fetch_side(int64_t, bool) {}
        __device__ __forceinline__ void deposit_side(int) {}
        __device__ __forceinline__ float weight(float s, int tr, int64_t j0, int64_t, int) {
            const int j = (int)j0 + tr;
            const float w = smx_exp(s - mm) * iz - (j == tg ? 1.0f : 0.f);
            return (j >= first_class && j < c1) ? w : 0.f;               // a select: an excluded pair's exp may be inf
        }
        __device__ __forceinline__ void finish(int64_t, int64_t, int) {}
    } P{first_class, mrow, invz, ctgt};
    pair_pass<KS, TS, true>(P, Q, B, E, n, chunk_rows, part);
}

// ------------------------------------------------------------------------------------------------ pass 2: items resident
template <int KS, int TS>
__global__ __launch_bounds__(kBlock, 2) void smx_e_pass_kernel(const float *__restrict__ E, int64_t n, const float *__restrict__ Q,
                                                              int64_t B, int first_class, const float *__restrict__ mrow,
                                                              const float *__restrict__ invz, const int *__restrict__ ctgt,
                                                              int64_t chunk_rows, float *__restrict__ part) {
    __shared__ float sm[2][TS], sz[2][TS];                              // (m_i, 1 / Z_i, target_i) of every row of the two tiles
    __shared__ int st[2][TS];
    struct Policy {
        int first_class;
        const float *__restrict__ mrow;
        const float *__restrict__ invz;
        const int *__restrict__ ctgt;
        float stm = 0.f, stz = 0.f;
        int stt = -1, ei = -2;

        __device__ __forceinline__ void start(int64_t e, int64_t nr, int64_t) {
            ei = (e >= (int64_t)first_class && e < nr) ? (int)e : -2;     // -2: the lane's item is no class (or no row)
        }
        __device__ __forceinline__ void fetch_side(int64_t r, bool in) {
            stm = in ? mrow[r] : 0.f;
            stz = in ? invz[r] : 0.f;                                    // a row past the chunk's end: exp(0 - 0) * 0
            stt = in ? ctgt[r] : -1;
        }
        __device__ __forceinline__ void deposit_side(int buf) {
            sm[buf][threadIdx.x] = stm;
            sz[buf][threadIdx.x] = stz;
            st[buf][threadIdx.x] = stt;
        }
        __device__ __forceinline__ float weight(float s, int tr, int64_t, int64_t, int buf) {
            const float w = smx_exp(s - sm[buf][tr]) * sz[buf][tr] - (st[buf][tr] == ei ? 1.0f : 0.f);
            return ei >= 0 ? w : 0.f;
        }
        __device__ __forceinline__ void finish(int64_t, int64_t, int) {}
    } P{first_class, mrow, invz, ctgt};
    pair_pass<KS, TS, true>(P, E, n, Q, B, chunk_rows, part);
}

// ------------------------------------------------------------------------------------------------ folds
// Per resident row: the chunk partials part[chunk][row][:] summed in chunk order, scaled, g[row] written once
__global__ __launch_bounds__(kBlock) void smx_fold_kernel(int64_t n, int D, int64_t chunks, const float *__restrict__ part,
                                                          float scale, float *__restrict__ g) {
    const int64_t j = (int64_t)blockIdx.x * kNceTeamsPerBlock + (threadIdx.x / kNceTeam);
    const int l = threadIdx.x & (kNceTeam - 1);
    if (j >= n) return;
    const int D4 = D / 4;
    NceRow H;
    H.v[0] = H.v[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t c = 0; c < chunks; ++c) nce_add(H, nce_load(part + (c * n + j) * (int64_t)D, D4, l));
    nce_store(g + j * (int64_t)D, D4, l, nce_axpby(H, scale, H, 0.f));
}

// ------------------------------------------------------------------------------------------------ host side
// The partials are sized by the bound of pair_chunks, not by the split itself: every term is non-decreasing in n and in B.
struct SmxWs {
    float *mpart, *zpart, *part, *mrow, *invz, *lterm;
    int *ctgt;
    int64_t total;
};

static SmxWs smx_carve(void *workspace, int64_t n, int64_t B, int32_t D) {
    const int64_t part_rows = kSmxTargetWg * kPairRows + 2 * kPairRows + (n > B ? n : B);
    const int64_t z_rows = kSmxTargetWg * kPairRows + 2 * kPairRows + B;
    Carver c(workspace);
    SmxWs W;
    W.mpart = c.take<float>(z_rows);
    W.zpart = c.take<float>(z_rows);
    W.part = c.take<float>(part_rows * D);
    W.mrow = c.take<float>(B);
    W.invz = c.take<float>(B);
    W.lterm = c.take<float>(B);
    W.ctgt = c.take<int>(B);
    W.total = c.bytes;
    return W;
}

// item and query numbers are compared as ints, a tile past the last row included
static inline bool smx_shape_ok(int64_t n, int64_t B) {
    return n > 0 && n < (int64_t(1) << 31) - 2 * kPairRows && B > 0 && B < (int64_t(1) << 31) - 2 * kPairRows;
}

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_softmax_ce_supported(int32_t D) { return (D == 32 || D == 64 || D == 128) ? 1 : 0; }

int64_t wr_softmax_ce_workspace_bytes(int64_t n_items, int64_t B, int32_t D) {
    WR_REQUIRE(wr_softmax_ce_supported(D), WR_E_RANGE, "softmax_ce supports D in {32, 64, 128}; got D=%d", D);
    WR_REQUIRE(smx_shape_ok(n_items, B), WR_E_SHAPE, "softmax_ce: n_items=%lld / B=%lld out of range", (long long)n_items,
               (long long)B);
    return smx_carve(nullptr, n_items, B, D).total;
}

int32_t wr_softmax_ce_loss_grad(const float *Q, int64_t B, const float *E, int64_t n_items, int32_t D, const int64_t *target,
                                int64_t first_class, float weight, float *loss, int32_t accumulate, float *gQ, float *gE,
                                int32_t *err_word, void *workspace, int64_t workspace_bytes, void *stream_) {
    WR_REQUIRE(wr_softmax_ce_supported(D), WR_E_RANGE, "softmax_ce supports D in {32, 64, 128}; got D=%d", D);
    WR_REQUIRE(smx_shape_ok(n_items, B), WR_E_SHAPE, "softmax_ce: n_items=%lld / B=%lld out of range", (long long)n_items,
               (long long)B);
    WR_REQUIRE(first_class >= 0 && first_class < n_items, WR_E_RANGE, "softmax_ce: first_class=%lld leaves no class among %lld items",
               (long long)first_class, (long long)n_items);
    WR_REQUIRE(Q && E && target && loss, WR_E_NULL, "softmax_ce: NULL argument");
    WR_REQUIRE((gQ == nullptr) == (gE == nullptr), WR_E_NULL, "softmax_ce: gQ and gE go together (both NULL = loss only)");
    WR_REQUIRE(aligned16(Q) && aligned16(E) && aligned16(gQ) && aligned16(gE), WR_E_ALIGN,
               "softmax_ce: Q, E, gQ and gE must be 16-byte aligned");
    const SmxWs W = smx_carve(workspace, n_items, B, D);
    const int32_t rc = check_workspace("wr_softmax_ce_loss_grad", workspace, workspace_bytes, W.total);
    if (rc != WR_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int TS = pair_tile(D);
    const int fc = (int)first_class;
    const unsigned grid_n = (unsigned)((n_items + kNceTeamsPerBlock - 1) / kNceTeamsPerBlock);
    const unsigned grid_b = (unsigned)((B + kNceTeamsPerBlock - 1) / kNceTeamsPerBlock);

    int64_t chunks, chunk_rows;
    pair_chunks(B, n_items, TS, kSmxTargetWg, chunks, chunk_rows);
    const dim3 grid_q((unsigned)((B + kPairRows - 1) / kPairRows), (unsigned)chunks);
#define WR_SMX_LSE(KS_)                                                                                               \
    hipLaunchKernelGGL((smx_lse_pass_kernel<KS_, pair_tile(2 * (KS_))>), grid_q, dim3(kBlock), 0, stream, Q, B, E, n_items, fc, \
                       chunk_rows, W.mpart, W.zpart)
    WR_DISPATCH_KS(D, 16, 64, WR_SMX_LSE);
#undef WR_SMX_LSE
    WR_LAUNCH_CHECK("smx_lse_pass_kernel");
    hipLaunchKernelGGL(smx_row_kernel, dim3(grid_b), dim3(kBlock), 0, stream, B, D, n_items, fc, chunks, W.mpart, W.zpart, Q, E,
                       target, W.mrow, W.invz, W.ctgt, W.lterm, err_word);
    WR_LAUNCH_CHECK("smx_row_kernel");
    hipLaunchKernelGGL(pair_loss_kernel, dim3(1), dim3(kBlock), 0, stream, W.lterm, B, weight, accumulate, loss);
    WR_LAUNCH_CHECK("pair_loss_kernel");
    if (gQ == nullptr) return WR_OK;

#define WR_SMX_Q(KS_)                                                                                                 \
    hipLaunchKernelGGL((smx_q_pass_kernel<KS_, pair_tile(2 * (KS_))>), grid_q, dim3(kBlock), 0, stream, Q, B, E, n_items, fc,   \
                       W.mrow, W.invz, W.ctgt, chunk_rows, W.part)
    WR_DISPATCH_KS(D, 16, 64, WR_SMX_Q);
#undef WR_SMX_Q
    WR_LAUNCH_CHECK("smx_q_pass_kernel");
    hipLaunchKernelGGL(smx_fold_kernel, dim3(grid_b), dim3(kBlock), 0, stream, B, D, chunks, W.part, weight, gQ);
    WR_LAUNCH_CHECK("smx_fold_kernel (queries)");

    pair_chunks(n_items, B, TS, kSmxTargetWg, chunks, chunk_rows);
    const dim3 grid_e((unsigned)((n_items + kPairRows - 1) / kPairRows), (unsigned)chunks);
#define WR_SMX_E(KS_)                                                                                                 \
    hipLaunchKernelGGL((smx_e_pass_kernel<KS_, pair_tile(2 * (KS_))>), grid_e, dim3(kBlock), 0, stream, E, n_items, Q, B, fc,   \
                       W.mrow, W.invz, W.ctgt, chunk_rows, W.part)
    WR_DISPATCH_KS(D, 16, 64, WR_SMX_E);
#undef WR_SMX_E
    WR_LAUNCH_CHECK("smx_e_pass_kernel");
    hipLaunchKernelGGL(smx_fold_kernel, dim3(grid_n), dim3(kBlock), 0, stream, n_items, D, chunks, W.part, weight, gE);
    WR_LAUNCH_CHECK("smx_fold_kernel (items)");
    return WR_OK;
}

}  // extern "C"
