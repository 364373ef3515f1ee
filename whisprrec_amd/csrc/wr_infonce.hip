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
#include "wr_row_team.h"
#include "wr_score_tiles.h"

namespace wr {

constexpr int kNceRows = kScoreRows;      // resident rows per workgroup (32 per wave)
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
// Resident rows R [nr, D] (128 per workgroup, 32 per wave, in registers as the B operand), streamed rows T [nt, D] in tiles
// of TS through LDS as the A operand:  s = <T[i], R[j]> (k-ordered chain),  w_ij = exp2((s - 1) * escale) * tscale[i],
//     zpart[chunk][j]    = sum_i w_ij                      (zpart may be NULL)
//     part[chunk][j][:]  = sum_i w_ij * T[i][:]            (GRAD only)
// over the streamed rows i of the chunk blockIdx.y.  tscale NULL = 1.  Streamed rows past the end weigh 0.
template <int KS, int TS, bool GRAD>
__global__ __launch_bounds__(kBlock, 2) void nce_pass_kernel(const float *__restrict__ R, int64_t nr, const float *__restrict__ T,
                                                            int64_t nt, const float *__restrict__ tscale, float escale,
                                                            int64_t chunk_rows, float *__restrict__ part,
                                                            float *__restrict__ zpart) {
    constexpr int D = 2 * KS, LDW = D + 1, C = TS / 32, NB = D / 32;
    __shared__ float it[2][TS * LDW];
    __shared__ float sc[2][TS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = lane & 31, half = lane >> 5;
    const int64_t e0 = (int64_t)blockIdx.x * kNceRows;
    const int64_t c0 = (int64_t)blockIdx.y * chunk_rows;
    const int64_t c1 = (c0 + chunk_rows < nt) ? c0 + chunk_rows : nt;
    // B[k = 2s + (lane>>5)][j = lane&31] of this wave's slab of resident rows
    float a[KS];
    {
        const int64_t e = e0 + wave * 32 + col;
        const float *rrow = R + ((e < nr) ? e : 0) * (int64_t)D + half;
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = (e < nr) ? rrow[2 * s] : 0.f;
    }
    f32x16 out[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) out[b] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float z = 0.f;
    TileStager<D, TS> stager;
    float sstage = 0.f;
    auto fetch = [&](int64_t j0) {
        stager.fetch(T, j0, c1);
        if (threadIdx.x < TS) {
            const int64_t r = j0 + threadIdx.x;
            sstage = (r < c1) ? (tscale != nullptr ? tscale[r] : 1.0f) : 0.f;
        }
    };
    auto deposit = [&](int buf) {
        stager.deposit(it[buf]);
        if (threadIdx.x < TS) sc[buf][threadIdx.x] = sstage;
    };
    fetch(c0);
    deposit(0);
    __syncthreads();
    int buf = 0;
    for (int64_t j0 = c0; j0 < c1; j0 += TS, buf ^= 1) {
        const bool more = j0 + TS < c1;
        if (more) fetch(j0 + TS);                                       // global loads fly while the matrix cores work
        // acc[c][reg] = score(streamed row c*32 + acc_row(reg, half), resident row lane&31)
        f32x16 acc[C];
        score_tiles<KS, C, LDW, true>(a, &it[buf][col * LDW + half], acc);   // A[i = lane&31][k = 2s + (lane>>5)] of block 0
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float w = __builtin_amdgcn_exp2f((acc[c][reg] - 1.0f) * escale) * sc[buf][c * 32 + acc_row(reg, half)];
                z += w;
                acc[c][reg] = w;
            }
        }
        if constexpr (GRAD) {
            // out[j][d] += sum_i w_ij T[i][d]: step `reg` of the k loop pairs the two streamed rows the two half-waves
            // hold in accumulator register `reg` — the weights are already where the A operand wants them
#pragma unroll
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    // B[k = half][j = d = lane&31 (+ 32 b)]
                    const float *brow = &it[buf][(c * 32 + acc_row(reg, half)) * LDW + col];
#pragma unroll
                    for (int b = 0; b < NB; ++b)
                        out[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[c][reg], brow[b * 32], out[b], 0, 0, 0);
                }
            }
        }
        if (more) deposit(buf ^ 1);                                     // the other buffer was last read one barrier ago
        __syncthreads();
    }
    z += __shfl_xor(z, 32, 64);                                         // the two half-waves hold disjoint streamed rows
    if (zpart != nullptr && half == 0) {
        const int64_t e = e0 + wave * 32 + col;
        if (e < nr) zpart[(int64_t)blockIdx.y * nr + e] = z;
    }
    if constexpr (GRAD) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int64_t e = e0 + wave * 32 + acc_row(reg, half);
                if (e < nr) part[((int64_t)blockIdx.y * nr + e) * D + b * 32 + col] = out[b][reg];
            }
        }
    }
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

__global__ __launch_bounds__(kBlock) void nce_loss_kernel(const float *__restrict__ lterm, int64_t B, float weight, int accumulate,
                                                          float *__restrict__ loss) {
    __shared__ float scratch[kBlock / 64];
    float v = 0.f;
    for (int64_t i = threadIdx.x; i < B; i += kBlock) v += lterm[i];
    const float r = block_sum(v, scratch);
    if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + weight * r;
}

// Per row of Bm: fold the chunk partials of sum_b softmax_bj q_b, scale by weight / tau, back through the normalisation
__global__ __launch_bounds__(kBlock) void nce_reduce_k_kernel(int64_t n, int D, int64_t chunks, const float *__restrict__ part,
                                                              const float *__restrict__ Kn, const float *__restrict__ invB,
                                                              float wtau, float *__restrict__ gB) {
    const int64_t t = (int64_t)blockIdx.x * kNceTeamsPerBlock + (threadIdx.x / kNceTeam);
    const int l = threadIdx.x & (kNceTeam - 1);
    const bool live = t < n;
    const int64_t j = live ? t : 0;
    const int D4 = D / 4;
    NceRow H;
    H.v[0] = H.v[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t c = 0; c < chunks; ++c) nce_add(H, nce_load(part + (c * n + j) * (int64_t)D, D4, l));
    const NceRow k = nce_load(Kn + j * (int64_t)D, D4, l);
    const NceRow g = nce_bwd(nce_axpby(H, wtau, H, 0.f), k, invB[j]);
    if (live) nce_store(gB + j * (int64_t)D, D4, l, g);
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
static inline int nce_tile(int D) { return D <= 64 ? 64 : 32; }

// split of the streamed side (nt rows) of a pass with nr resident rows: chunks * nr <= kNceTargetWg * kNceRows + nr + kNceRows
static void nce_chunks(int64_t nr, int64_t nt, int TS, int64_t &chunks, int64_t &chunk_rows) {
    const int64_t rb = (nr + kNceRows - 1) / kNceRows, tiles = (nt + TS - 1) / TS;
    const int64_t want = (kNceTargetWg + rb - 1) / rb;
    const int64_t ch = tiles < want ? tiles : want;
    const int64_t tpc = (tiles + ch - 1) / ch;
    chunks = (tiles + tpc - 1) / tpc;
    chunk_rows = tpc * TS;
}

struct NceLayout {
    int64_t Kn, invB, owner, Q, invA, cidx, dup, zpart, part, invZ, lterm, growA, growB, total;   // byte offsets
};

static void nce_layout(int64_t n, int64_t B, int32_t D, NceLayout &L) {
    // every term is non-decreasing in n and in B; the partials are sized by the bound of nce_chunks, not by the split itself
    const int64_t part_rows = kNceTargetWg * kNceRows + 2 * kNceRows + (n > B ? n : B);
    const int64_t z_rows = kNceTargetWg * kNceRows + 2 * kNceRows + B;
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t at = o; o += align_up(bytes, 256); return at; };
    L.Kn = take(n * D * 4);
    L.invB = take(n * 4);
    L.owner = take(n * 4);
    L.Q = take(B * D * 4);
    L.invA = take(B * 4);
    L.cidx = take(B * 8);
    L.dup = take(B * 4);
    L.zpart = take(z_rows * 4);
    L.part = take(part_rows * D * 4);
    L.invZ = take(B * 4);
    L.lterm = take(B * 4);
    L.growA = take(B * D * 4);
    L.growB = take(B * D * 4);
    L.total = o;
}

static inline bool nce_shape_ok(int64_t n, int64_t B) {
    return n > 0 && n < (int64_t(1) << 31) && B > 0 && B < (int64_t(1) << 31);
}

template <bool GRAD>
static void nce_launch_pass(int32_t D, dim3 grid, hipStream_t stream, const float *R, int64_t nr, const float *T, int64_t nt,
                            const float *tscale, float escale, int64_t chunk_rows, float *part, float *zpart) {
#define WR_NCE_PASS(KS_)                                                                                              \
    hipLaunchKernelGGL((nce_pass_kernel<KS_, ((KS_) <= 32 ? 64 : 32), GRAD>), grid, dim3(kBlock), 0, stream, R, nr, T, nt, tscale, \
                       escale, chunk_rows, part, zpart)
    WR_DISPATCH_KS(D, 16, 64, WR_NCE_PASS);                             // the tile height is nce_tile(D)
#undef WR_NCE_PASS
}

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_infonce_supported(int32_t D) { return (D == 32 || D == 64 || D == 128) ? 1 : 0; }

int64_t wr_infonce_workspace_bytes(int64_t n_rows, int64_t B, int32_t D) {
    WR_REQUIRE(wr_infonce_supported(D), WR_E_RANGE, "infonce supports D in {32, 64, 128}; got D=%d", D);
    WR_REQUIRE(nce_shape_ok(n_rows, B), WR_E_SHAPE, "infonce: n_rows=%lld / B=%lld out of range", (long long)n_rows, (long long)B);
    NceLayout L;
    nce_layout(n_rows, B, D, L);
    return L.total;
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
    NceLayout L;
    nce_layout(n_rows, B, D, L);
    WR_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= L.total, WR_E_WORKSPACE, "infonce workspace %lld B < %lld B",
               (long long)workspace_bytes, (long long)L.total);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    char *ws = reinterpret_cast<char *>(workspace);
    float *Kn = reinterpret_cast<float *>(ws + L.Kn), *invB = reinterpret_cast<float *>(ws + L.invB);
    int *owner = reinterpret_cast<int *>(ws + L.owner), *dup = reinterpret_cast<int *>(ws + L.dup);
    float *Q = reinterpret_cast<float *>(ws + L.Q), *invA = reinterpret_cast<float *>(ws + L.invA);
    int64_t *cidx = reinterpret_cast<int64_t *>(ws + L.cidx);
    float *zpart = reinterpret_cast<float *>(ws + L.zpart), *part = reinterpret_cast<float *>(ws + L.part);
    float *invZ = reinterpret_cast<float *>(ws + L.invZ), *lterm = reinterpret_cast<float *>(ws + L.lterm);
    float *growA = reinterpret_cast<float *>(ws + L.growA), *growB = reinterpret_cast<float *>(ws + L.growB);
    const bool grad = gA != nullptr;
    const int TS = nce_tile(D);
    const float inv_tau = 1.0f / tau, wtau = weight / tau, escale = 1.44269504088896341f / tau;
    const unsigned grid_n = (unsigned)((n_rows + kNceTeamsPerBlock - 1) / kNceTeamsPerBlock);
    const unsigned grid_b = (unsigned)((B + kNceTeamsPerBlock - 1) / kNceTeamsPerBlock);

    hipLaunchKernelGGL(nce_prep_k_kernel, dim3(grid_n), dim3(kBlock), 0, stream, Bm, n_rows, D, Kn, invB, owner);
    WR_LAUNCH_CHECK("nce_prep_k_kernel");
    hipLaunchKernelGGL(nce_prep_q_kernel, dim3(grid_b), dim3(kBlock), 0, stream, A, n_rows, D, idx, B, Q, invA, cidx, owner, dup,
                       err_word);
    WR_LAUNCH_CHECK("nce_prep_q_kernel");
    int64_t chunks, chunk_rows;
    nce_chunks(B, n_rows, TS, chunks, chunk_rows);
    {
        const dim3 grid((unsigned)((B + kNceRows - 1) / kNceRows), (unsigned)chunks);
        if (grad) nce_launch_pass<true>(D, grid, stream, Q, B, Kn, n_rows, nullptr, escale, chunk_rows, part, zpart);
        else nce_launch_pass<false>(D, grid, stream, Q, B, Kn, n_rows, nullptr, escale, chunk_rows, part, zpart);
        WR_LAUNCH_CHECK("nce_pass_kernel (queries)");
    }
    hipLaunchKernelGGL(nce_reduce_q_kernel, dim3(grid_b), dim3(kBlock), 0, stream, B, D, chunks, zpart, part, Q, invA, Kn, invB, cidx,
                       owner, dup, wtau, inv_tau, invZ, lterm, growA, growB, grad ? 1 : 0);
    WR_LAUNCH_CHECK("nce_reduce_q_kernel");
    hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(kBlock), 0, stream, lterm, B, weight, accumulate, loss);
    WR_LAUNCH_CHECK("nce_loss_kernel");
    if (!grad) return WR_OK;
    nce_chunks(n_rows, B, TS, chunks, chunk_rows);
    {
        const dim3 grid((unsigned)((n_rows + kNceRows - 1) / kNceRows), (unsigned)chunks);
        nce_launch_pass<true>(D, grid, stream, Kn, n_rows, Q, B, invZ, escale, chunk_rows, part, nullptr);
        WR_LAUNCH_CHECK("nce_pass_kernel (items)");
    }
    hipLaunchKernelGGL(nce_reduce_k_kernel, dim3(grid_n), dim3(kBlock), 0, stream, n_rows, D, chunks, part, Kn, invB, wtau, gB);
    WR_LAUNCH_CHECK("nce_reduce_k_kernel");
    WR_HIP(hipMemsetAsync(gA, 0, (size_t)n_rows * D * 4, stream));
    hipLaunchKernelGGL(nce_scatter_kernel, dim3(grid_b), dim3(kBlock), 0, stream, B, D, cidx, owner, dup, growA, growB, gA, gB);
    WR_LAUNCH_CHECK("nce_scatter_kernel");
    return WR_OK;
}

}  // extern "C"
