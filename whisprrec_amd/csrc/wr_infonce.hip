// wr_infonce.hip — InfoNCE loss and gradient of one side of SGL's calc_ssl_loss without the [B, n] score matrix.
//
// Reference: calc_ssl_loss (src/models/general/SGL.py:196-230): the batch rows of view 1 and ALL rows of view 2 are
// L2-normalised (F.normalize, eps 1e-12), every batch row is scored against every row of view 2, and
//     loss = weight * sum_b ( log sum_j exp(<q_b, k_j> / tau)  -  <q_b, k_idx_b> / tau ).
// The reference forms e1.matmul(all2.T) and lets autograd keep it and its exp alive.  Here the scores exist only as 32x32
// accumulator tiles of v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: the k-ordered fma chain of wr_score_tiles.h):
//
//   prep        k_j = Bm[j] / max(|Bm[j]|, eps) for every row (workspace, [n, D]) and q_b likewise for the batch rows; ids
//               outside [0, n) are clamped and reported; owner[id] = first batch position that names the row
//   pass 1      128 batch rows per workgroup stay in registers, 64-row tiles of k stream through LDS (double-buffered, one
//               barrier per tile).  Cosines are bounded, so e_bj = exp((c_bj - 1) / tau) needs no running maximum: it lies in
//               (0, 1] for every tau > 0, and 1/tau is added back after the log.  Per (row, item chunk): sum_j e_bj and
//               sum_j e_bj k_j — the second product runs on the matrix cores too: the score tile is computed TRANSPOSED
//               (streamed rows x resident rows), which leaves every lane holding the weights of its own resident row in the
//               operand layout of the next MFMA, without a trip through LDS
//   reduce q    chunk partials folded in chunk order -> Z_b, the loss terms, d loss / d q_b, back through the normalisation
//   loss        the B terms folded by one workgroup in a fixed order
//   pass 2      the same kernel with the roles swapped: 128 rows of k resident, the batch rows q_b streamed with the scale
//               1/Z_b, giving sum_b softmax_bj q_b per row of k
//   reduce k    chunk partials folded, back through the normalisation of Bm[j], every row of gB written once
//   scatter     rows named by the batch: gA[id] = sum of the per-position gradients, gB[id] += sum of the positive terms, by
//               the owner position, in ascending position order
// No float atomics anywhere: every sum has a fixed order, the results are bitwise reproducible.  No host round trip.
#include "wr_pair_pass.h"

namespace wr {

constexpr int64_t kNceTargetWg = 1024;    // workgroups a pass aims at when it splits the streamed side into chunks

// ------------------------------------------------------------------------------------------------ prep
__global__ __launch_bounds__(kBlock) void nce_prep_k_kernel(const float *__restrict__ Bm, int64_t n, int D, float *__restrict__ Kn,
                                                            float *__restrict__ invB, int *__restrict__ owner) {
    const int64_t t = (int64_t)blockIdx.x * kNceTeamsPerBlock + (threadIdx.x / kNceTeam);
    const int l = threadIdx.x & (kNceTeam - 1);
    const bool live = t < n;
    const int64_t j = live ? t : 0;
    float inv;
    const NceRow k = nce_normalize(nce_load(Bm + j * (int64_t)D, D / 4, l), inv);
    if (!live) return;
    nce_store(Kn + j * (int64_t)D, D / 4, l, k);
    if (l == 0) {
        invB[j] = inv;
        owner[j] = 0x7fffffff;
    }
}

__global__ __launch_bounds__(kBlock) void nce_prep_q_kernel(const float *__restrict__ A, int64_t n, int D,
                                                            const int64_t *__restrict__ idx, int64_t B, float *__restrict__ Q,
                                                            float *__restrict__ invA, int64_t *__restrict__ cidx,
                                                            int *__restrict__ owner, int *__restrict__ dup,
                                                            int32_t *__restrict__ err_word) {
    const int64_t t = (int64_t)blockIdx.x * kNceTeamsPerBlock + (threadIdx.x / kNceTeam);
    const int l = threadIdx.x & (kNceTeam - 1);
    const bool live = t < B;
    const int64_t b = live ? t : 0;
    int64_t id = idx[b];
    const bool bad = id < 0 || id >= n;
    if (bad) id = id < 0 ? 0 : n - 1;                       // never dereferenced out of range
    float inv;
    const NceRow q = nce_normalize(nce_load(A + id * (int64_t)D, D / 4, l), inv);
    if (!live) return;
    nce_store(Q + b * (int64_t)D, D / 4, l, q);
    if (l == 0) {
        if (bad && err_word != nullptr) atomicOr(err_word, 1);
        invA[b] = inv;
        cidx[b] = id;
        dup[b] = 0;
        atomicMin(&owner[id], (int)b);                       // integer atomic: the result does not depend on the order
    }
}

// ------------------------------------------------------------------------------------------------ the two GEMM passes
// pair_pass (wr_pair_pass.h) with the softmax weights: for the streamed row i and the resident row j,
//     w_ij = exp2((s - 1) * escale) * tscale[i],     zpart[chunk][j] = sum_i w_ij     (zpart may be NULL)
// over the streamed rows i of the chunk blockIdx.y.  tscale NULL = 1.  Streamed rows past the end weigh 0.
// The policy is a local struct of the kernel so that it names the kernel's LDS array itself: reached through a pointer member the
// same reads compile to other address arithmetic and five more VGPRs in the gradient pass.
template <int KS, int TS, bool GRAD>
__global__ __launch_bounds__(kBlock, 2) void nce_pass_kernel(const float *__restrict__ R, int64_t nr, const float *__restrict__ T,
                                                            int64_t nt, const float *__restrict__ tscale, float escale,
                                                            int64_t chunk_rows, float *__restrict__ part,
                                                            float *__restrict__ zpart) {
    __shared__ float sc[2][TS];                                         // the scale of every row of the two tiles
    struct Policy {
        const float *__restrict__ tscale;
        float escale;
        float *__restrict__ zpart;
        float sstage = 0.f, z = 0.f;

        __device__ __forceinline__ void start(int64_t, int64_t, int64_t) {}
        __device__ __forceinline__ void fetch_side(int64_t r, bool in) { sstage = in ? (tscale != nullptr ? tscale[r] : 1.0f) : 0.f; }
        __device__ __forceinline__ void deposit_side(int buf) { sc[buf][threadIdx.x] = sstage; }
        __device__ __forceinline__ float weight(float s, int tr, int64_t, int64_t, int buf) {
            const float w = __builtin_amdgcn_exp2f((s - 1.0f) * escale) * sc[buf][tr];
            z += w;
            return w;
        }
        __device__ __forceinline__ void finish(int64_t e, int64_t nr, int half) {
            z += __shfl_xor(z, 32, 64);
            if (zpart != nullptr && half == 0) {
                if (e < nr) zpart[(int64_t)blockIdx.y * nr + e] = z;
            }
        }
    } P{tscale, escale, zpart};
    pair_pass<KS, TS, GRAD>(P, R, nr, T, nt, chunk_rows, part);
}

// ------------------------------------------------------------------------------------------------ reductions
// Per batch position: Z_b, the loss term, and (grad) the two per-position gradient rows
//   growA[b] = d loss / d A[idx_b]  of this position alone,   growB[b] = the positive term's share of d loss / d Bm[idx_b]
__global__ __launch_bounds__(kBlock) void nce_reduce_q_kernel(int64_t B, int D, int64_t chunks, const float *__restrict__ zpart,
                                                              const float *__restrict__ part, const float *__restrict__ Q,
                                                              const float *__restrict__ invA, const float *__restrict__ Kn,
                                                              const float *__restrict__ invB, const int64_t *__restrict__ cidx,
                                                              const int *__restrict__ owner, int *__restrict__ dup, float wtau,
                                                              float inv_tau, float *__restrict__ invZ, float *__restrict__ lterm,
                                                              float *__restrict__ growA, float *__restrict__ growB, int grad) {
    const int64_t t = (int64_t)blockIdx.x * kNceTeamsPerBlock + (threadIdx.x / kNceTeam);
    const int l = threadIdx.x & (kNceTeam - 1);
    const bool live = t < B;
    const int64_t b = live ? t : 0;
    const int D4 = D / 4;
    float Z = 0.f;
    for (int64_t c = 0; c < chunks; ++c) Z += zpart[c * B + b];         // chunk order
    const int64_t id = cidx[b];
    const NceRow q = nce_load(Q + b * (int64_t)D, D4, l);
    const NceRow kp = nce_load(Kn + id * (int64_t)D, D4, l);
    const float pos = nce_dot(q, kp);
    const float iz = 1.0f / Z;
    if (live && l == 0) {
        lterm[b] = (logf(Z) + inv_tau) - pos * inv_tau;                 // log sum_j exp(s_bj) - s_b,idx_b
        invZ[b] = iz;
    }
    if (!grad) return;
    NceRow G;
    G.v[0] = G.v[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t c = 0; c < chunks; ++c) nce_add(G, nce_load(part + (c * B + b) * (int64_t)D, D4, l));
    // d loss / d q_b = (weight / tau) * (sum_j softmax_bj k_j - k_idx_b)
    const NceRow gq = nce_axpby(G, wtau * iz, kp, -wtau);
    const NceRow ga = nce_bwd(gq, q, invA[b]);
    // positive term of d loss / d k_idx_b = -(weight / tau) q_b, back through the normalisation of Bm[idx_b]
    const NceRow gk = nce_axpby(q, -wtau, q, 0.f);
    const NceRow gb = nce_bwd(gk, kp, invB[id]);
    if (!live) return;
    nce_store(growA + b * (int64_t)D, D4, l, ga);
    nce_store(growB + b * (int64_t)D, D4, l, gb);
    if (l == 0) {
        const int o = owner[id];
        if ((int64_t)o != b) dup[o] = 1;                                 // same value from every writer
    }
}

// Rows named by the batch.  The owner of a row (its first position) sums the per-position rows of every position that
// names it, in ascending position order, and is the only writer of that row: gA[id] = sum, gB[id] += sum.
__global__ __launch_bounds__(kBlock) void nce_scatter_kernel(int64_t B, int D, const int64_t *__restrict__ cidx,
                                                             const int *__restrict__ owner, const int *__restrict__ dup,
                                                             const float *__restrict__ growA, const float *__restrict__ growB,
                                                             float *__restrict__ gA, float *__restrict__ gB) {
    const int team = threadIdx.x / kNceTeam;
    const int64_t t = (int64_t)blockIdx.x * kNceTeamsPerBlock + team;
    const int l = threadIdx.x & (kNceTeam - 1);
    const bool live = t < B;
    const int64_t b = live ? t : 0;
    const int D4 = D / 4;
    const int64_t id = cidx[b];
    const bool own = live && (int64_t)owner[id] == b;
    const bool shared = own && dup[b] != 0;
    NceRow sa = nce_load(growA + b * (int64_t)D, D4, l), sb = nce_load(growB + b * (int64_t)D, D4, l);
    if (__any(shared)) {                                                 // wave-uniform: some row of this wave recurs
        const int64_t want = shared ? id : -1;
        const unsigned sh = (unsigned)((team & 3) * kNceTeam);          // this team's 16 bits of the wave's ballot
        for (int64_t base = 0; base < B; base += kNceTeam) {
            const int64_t p = base + l;
            const bool hit = p < B && p > b && cidx[p] == want;
            unsigned m = (unsigned)(__ballot(hit) >> sh) & 0xffffu;
            while (m) {                                                  // ascending positions
                const int64_t pp = base + (__ffs(m) - 1);
                m &= m - 1;
                nce_add(sa, nce_load(growA + pp * (int64_t)D, D4, l));
                nce_add(sb, nce_load(growB + pp * (int64_t)D, D4, l));
            }
        }
    }
    if (!own) return;
    nce_store(gA + id * (int64_t)D, D4, l, sa);
    NceRow cur = nce_load(gB + id * (int64_t)D, D4, l);
    nce_add(cur, sb);
    nce_store(gB + id * (int64_t)D, D4, l, cur);
}

// ------------------------------------------------------------------------------------------------ host side
// The partials are sized by the bound of pair_chunks, not by the split itself: every term is non-decreasing in n and in B.
struct NceWs {
    float *Kn, *invB;
    int *owner;
    float *Q, *invA;
    int64_t *cidx;
    int *dup;
    float *zpart, *part, *invZ, *lterm, *growA, *growB;
    int64_t total;
};

static NceWs nce_carve(void *workspace, int64_t n, int64_t B, int32_t D) {
    const int64_t part_rows = kNceTargetWg * kPairRows + 2 * kPairRows + (n > B ? n : B);
    const int64_t z_rows = kNceTargetWg * kPairRows + 2 * kPairRows + B;
    Carver c(workspace);
    NceWs W;
    W.Kn = c.take<float>(n * D);
    W.invB = c.take<float>(n);
    W.owner = c.take<int>(n);
    W.Q = c.take<float>(B * D);
    W.invA = c.take<float>(B);
    W.cidx = c.take<int64_t>(B);
    W.dup = c.take<int>(B);
    W.zpart = c.take<float>(z_rows);
    W.part = c.take<float>(part_rows * D);
    W.invZ = c.take<float>(B);
    W.lterm = c.take<float>(B);
    W.growA = c.take<float>(B * D);
    W.growB = c.take<float>(B * D);
    W.total = c.bytes;
    return W;
}

static inline bool nce_shape_ok(int64_t n, int64_t B) {
    return n > 0 && n < (int64_t(1) << 31) && B > 0 && B < (int64_t(1) << 31);
}

template <bool GRAD>
static void nce_launch_pass(int32_t D, dim3 grid, hipStream_t stream, const float *R, int64_t nr, const float *T, int64_t nt,
                            const float *tscale, float escale, int64_t chunk_rows, float *part, float *zpart) {
#define WR_NCE_PASS(KS_)                                                                                              \
    hipLaunchKernelGGL((nce_pass_kernel<KS_, pair_tile(2 * (KS_)), GRAD>), grid, dim3(kBlock), 0, stream, R, nr, T, nt, tscale, \
                       escale, chunk_rows, part, zpart)
    WR_DISPATCH_KS(D, 16, 64, WR_NCE_PASS);
#undef WR_NCE_PASS
}

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_infonce_supported(int32_t D) { return (D == 32 || D == 64 || D == 128) ? 1 : 0; }

int64_t wr_infonce_workspace_bytes(int64_t n_rows, int64_t B, int32_t D) {
    WR_REQUIRE(wr_infonce_supported(D), WR_E_RANGE, "infonce supports D in {32, 64, 128}; got D=%d", D);
    WR_REQUIRE(nce_shape_ok(n_rows, B), WR_E_SHAPE, "infonce: n_rows=%lld / B=%lld out of range", (long long)n_rows, (long long)B);
    return nce_carve(nullptr, n_rows, B, D).total;
}

int32_t wr_infonce_loss_grad(const float *A, const float *Bm, int64_t n_rows, int32_t D, const int64_t *idx, int64_t B, float tau,
                             float weight, float *loss, int32_t accumulate, float *gA, float *gB, int32_t *err_word,
                             void *workspace, int64_t workspace_bytes, void *stream_) {
    WR_REQUIRE(wr_infonce_supported(D), WR_E_RANGE, "infonce supports D in {32, 64, 128}; got D=%d", D);
    WR_REQUIRE(nce_shape_ok(n_rows, B), WR_E_SHAPE, "infonce: n_rows=%lld / B=%lld out of range", (long long)n_rows, (long long)B);
    WR_REQUIRE(A && Bm && idx && loss, WR_E_NULL, "infonce: NULL argument");
    WR_REQUIRE((gA == nullptr) == (gB == nullptr), WR_E_NULL, "infonce: gA and gB go together (both NULL = loss only)");
    WR_REQUIRE(aligned16(A) && aligned16(Bm) && aligned16(gA) && aligned16(gB), WR_E_ALIGN, "infonce: tables must be 16-byte aligned");
    WR_REQUIRE(tau > 0.f && tau == tau && tau <= 3.0e38f, WR_E_RANGE, "infonce: tau must be positive and finite");
    const NceWs W = nce_carve(workspace, n_rows, B, D);
    const int32_t rc = check_workspace("wr_infonce_loss_grad", workspace, workspace_bytes, W.total);
    if (rc != WR_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const bool grad = gA != nullptr;
    const int TS = pair_tile(D);
    const float inv_tau = 1.0f / tau, wtau = weight / tau, escale = 1.44269504088896341f / tau;
    const unsigned grid_n = (unsigned)((n_rows + kNceTeamsPerBlock - 1) / kNceTeamsPerBlock);
    const unsigned grid_b = (unsigned)((B + kNceTeamsPerBlock - 1) / kNceTeamsPerBlock);

    hipLaunchKernelGGL(nce_prep_k_kernel, dim3(grid_n), dim3(kBlock), 0, stream, Bm, n_rows, D, W.Kn, W.invB, W.owner);
    WR_LAUNCH_CHECK("nce_prep_k_kernel");
    hipLaunchKernelGGL(nce_prep_q_kernel, dim3(grid_b), dim3(kBlock), 0, stream, A, n_rows, D, idx, B, W.Q, W.invA, W.cidx, W.owner,
                       W.dup, err_word);
    WR_LAUNCH_CHECK("nce_prep_q_kernel");
    int64_t chunks, chunk_rows;
    pair_chunks(B, n_rows, TS, kNceTargetWg, chunks, chunk_rows);
    {
        const dim3 grid((unsigned)((B + kPairRows - 1) / kPairRows), (unsigned)chunks);
        if (grad) nce_launch_pass<true>(D, grid, stream, W.Q, B, W.Kn, n_rows, nullptr, escale, chunk_rows, W.part, W.zpart);
        else nce_launch_pass<false>(D, grid, stream, W.Q, B, W.Kn, n_rows, nullptr, escale, chunk_rows, W.part, W.zpart);
        WR_LAUNCH_CHECK("nce_pass_kernel (queries)");
    }
    hipLaunchKernelGGL(nce_reduce_q_kernel, dim3(grid_b), dim3(kBlock), 0, stream, B, D, chunks, W.zpart, W.part, W.Q, W.invA, W.Kn,
                       W.invB, W.cidx, W.owner, W.dup, wtau, inv_tau, W.invZ, W.lterm, W.growA, W.growB, grad ? 1 : 0);
    WR_LAUNCH_CHECK("nce_reduce_q_kernel");
    hipLaunchKernelGGL(pair_loss_kernel, dim3(1), dim3(kBlock), 0, stream, W.lterm, B, weight, accumulate, loss);
    WR_LAUNCH_CHECK("pair_loss_kernel");
    if (!grad) return WR_OK;
    pair_chunks(n_rows, B, TS, kNceTargetWg, chunks, chunk_rows);
    {
        const dim3 grid((unsigned)((n_rows + kPairRows - 1) / kPairRows), (unsigned)chunks);
        nce_launch_pass<true>(D, grid, stream, W.Kn, n_rows, W.Q, B, W.invZ, escale, chunk_rows, W.part, nullptr);
        WR_LAUNCH_CHECK("nce_pass_kernel (items)");
    }
    // per row of Bm: sum_b softmax_bj q_b, scaled by weight / tau, back through the normalisation of Bm[j]
    hipLaunchKernelGGL(pair_grad_kernel, dim3(grid_n), dim3(kBlock), 0, stream, n_rows, D, chunks, W.part, W.Kn, W.invB, wtau, gB);
    WR_LAUNCH_CHECK("pair_grad_kernel (items)");
    WR_HIP(hipMemsetAsync(gA, 0, (size_t)n_rows * D * 4, stream));
    hipLaunchKernelGGL(nce_scatter_kernel, dim3(grid_b), dim3(kBlock), 0, stream, B, D, W.cidx, W.owner, W.dup, W.growA, W.growB, gA,
                       gB);
    WR_LAUNCH_CHECK("nce_scatter_kernel");
    return WR_OK;
}

}  // extern "C"
