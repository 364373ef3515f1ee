// wr_supcon.hip — K15: ContraRec's supervised contrastive loss (ContraLoss, reference src/models/sequential/ContraRec.py:141-204)
// and its gradient without any [N, N] array, N = 2B rows of the two augmented views.
//
// The reference as written, z = F.normalize(F):
//     s_ij = <z_i, z_j> / tau,  m_i = max_j s_ij (diagonal included),  l_ij = s_ij - 2 m_i   (the maximum is subtracted twice: the
//     in-place sub_ at :181 and the detach at :182),  E_i = sum_{j != i} exp(l_ij),  P_i = { j != i : label_j == label_i },
//     loss = weight / N * sum_i (-tau / (|P_i| + 1e-10)) * sum_{j in P_i} (l_ij - log(E_i + 1e-10))
// Neither the double shift nor the 1e-10 is cosmetic: exp(l_ij) ~ exp(-1/tau) is 2e-9 at tau = 0.05, the size of the 1e-10.
//
// The scores exist only as 32x32 accumulator tiles of v_mfma_f32_32x32x2_f32 (score_tiles of wr_score_tiles.h) with the
// normalised rows as both operands: the k-ordered chain commutes in its two rows, so s_ij and s_ji have the same bits.
//
//   prep      z_i = F_i / max(|F_i|, eps), the signed reciprocal norm, label_i = labels[i mod B]
//   pass 1    128 rows per workgroup stay in registers, 64- (D = 128: 32-) row tiles of z stream through LDS, double-buffered as
//             in K12.  Cosines are bounded, so e_ij = exp((c_ij - 1) / tau) in (0, ~1] needs no running maximum.  Per (row,
//             column chunk): max_j c_ij, sum_{j != i} e_ij, |P_i|, sum_{j in P_i} c_ij
//   stats     chunk partials folded in chunk order -> m_i and, with r_i = exp(1/tau - 2 m_i) (exp(l_ij) = e_ij r_i), the sum
//             d_i = sum e_ij + 1e-10 / r_i = (E_i + 1e-10) / r_i, the row's loss term and the two coefficients of its gradient:
//             a_i = 1 / c_i, b_i = (|P_i| / c_i) / d_i
//   loss      the N terms folded by one workgroup in a fixed order
//   pass 2    the tiles again; (G_ij + G_ji) N / (-tau) = [j in P_i] (a_i + a_j) - e_ij (b_i + b_j) from the row's and the column's
//             statistics, zero on the diagonal, times z on the matrix cores (the transposed tile leaves the weights in the operand
//             layout of the next MFMA, as K12's softmax-times-rows product)
//   grad      chunk partials folded in chunk order, scaled by -weight / N, back through the normalisation
// m_i is a constant of the gradient (the closed form of the header).  No float atomics, every sum has a fixed order: same
// inputs, same bits; loss-only runs the same kernels up to `loss`.  No host round trip, no allocation.
#include "wr_row_team.h"
#include "wr_score_tiles.h"

namespace wr {

constexpr int kSupRows = kScoreRows;     // resident rows per workgroup (32 per wave)
constexpr int64_t kSupTargetWg = 512;    // workgroups a pass aims at when it splits the streamed side into chunks
constexpr int64_t kSupMaxRows = 1 << 15;
constexpr float kSupEps = 1e-10f;        // the reference's two + 1e-10

// ------------------------------------------------------------------------------------------------ prep
__global__ __launch_bounds__(kBlock) void sup_prep_kernel(const float *__restrict__ F, int64_t N, int64_t B, int D,
                                                          const int64_t *__restrict__ labels, float *__restrict__ Z,
                                                          float *__restrict__ inv, int64_t *__restrict__ lab) {
    const int64_t t = (int64_t)blockIdx.x * kNceTeamsPerBlock + (threadIdx.x / kNceTeam);
    const int l = threadIdx.x & (kNceTeam - 1);
    const bool live = t < N;
    const int64_t i = live ? t : 0;
    float iv;
    const NceRow z = nce_normalize(nce_load(F + i * (int64_t)D, D / 4, l), iv);
    if (!live) return;
    nce_store(Z + i * (int64_t)D, D / 4, l, z);
    if (l == 0) {
        inv[i] = iv;
        lab[i] = labels[i >= B ? i - B : i];
    }
}

// ------------------------------------------------------------------------------------------------ the two tile passes
// Resident rows i (128 per workgroup, 32 per wave, in registers as the B operand) against the streamed rows j of the column
// chunk blockIdx.y, in tiles of TS through LDS as the A operand: c = <Z[j], Z[i]>, e = exp2((c - 1) * escale).
//   !GRAD   stat[chunk][0..3][i] = max_j c,  sum_{j != i} e,  |{j != i : lab_j == lab_i}|,  sum over those j of c
//    GRAD   part[chunk][i][:]    = sum_{j != i} ([lab_j == lab_i] (ra_i + ra_j) - e (rb_i + rb_j)) Z[j][:]
template <int KS, int TS, bool GRAD>
__global__ __launch_bounds__(kBlock, 2) void sup_pass_kernel(const float *__restrict__ Z, int64_t N, const int64_t *__restrict__ lab,
                                                            const float *__restrict__ ra, const float *__restrict__ rb, float escale,
                                                            int64_t chunk_rows, float *__restrict__ stat, float *__restrict__ part) {
    constexpr int D = 2 * KS, LDW = D + 1, C = TS / 32, NB = D / 32;
    __shared__ float it[2][TS * LDW];
    __shared__ int64_t sl[2][TS];
    __shared__ float sa[2][TS], sb[2][TS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = lane & 31, half = lane >> 5;
    const int64_t e0 = (int64_t)blockIdx.x * kSupRows;
    const int64_t c0 = (int64_t)blockIdx.y * chunk_rows;
    const int64_t c1 = (c0 + chunk_rows < N) ? c0 + chunk_rows : N;
    const int64_t e = e0 + wave * 32 + col;                             // this lane's resident row
    const int64_t er = e < N ? e : 0;
    // B[k = 2s + (lane>>5)][j = lane&31] of this wave's slab of resident rows
    float a[KS];
    {
        const float *rrow = Z + er * (int64_t)D + half;
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = (e < N) ? rrow[2 * s] : 0.f;
    }
    const int64_t mylab = lab[er];
    const float ai = GRAD ? ra[er] : 0.f, bi = GRAD ? rb[er] : 0.f;
    f32x16 out[GRAD ? NB : 1];
#pragma unroll
    for (int b = 0; b < (GRAD ? NB : 1); ++b) out[b] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float cmax = -INFINITY, esum = 0.f, cnt = 0.f, cpos = 0.f;
    TileStager<D, TS> stager;
    int64_t lstage = 0;
    float astage = 0.f, bstage = 0.f;
    auto fetch = [&](int64_t j0) {
        stager.fetch(Z, j0, c1);
        if (threadIdx.x < TS) {
            const int64_t r = j0 + threadIdx.x;
            const bool in = r < c1;
            lstage = lab[in ? r : 0];
            if constexpr (GRAD) {
                astage = in ? ra[r] : 0.f;
                bstage = in ? rb[r] : 0.f;
            }
        }
    };
    auto deposit = [&](int buf) {
        stager.deposit(it[buf]);
        if (threadIdx.x < TS) {
            sl[buf][threadIdx.x] = lstage;
            if constexpr (GRAD) {
                sa[buf][threadIdx.x] = astage;
                sb[buf][threadIdx.x] = bstage;
            }
        }
    };
    fetch(c0);
    deposit(0);
    __syncthreads();
    int buf = 0;
    for (int64_t j0 = c0; j0 < c1; j0 += TS, buf ^= 1) {
        const bool more = j0 + TS < c1;
        if (more) fetch(j0 + TS);                                       // global loads fly while the matrix cores work
        // acc[c][reg] = <streamed row c*32 + acc_row(reg, half), resident row lane&31>
        f32x16 acc[C];
        score_tiles<KS, C, LDW, true>(a, &it[buf][col * LDW + half], acc);
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int tr = c * 32 + acc_row(reg, half);
                const int jr = (int)j0 + tr;                            // N <= 2^15: row numbers fit an int
                const float cs = acc[c][reg];
                const bool valid = jr < (int)c1;                        // rows past the chunk's end are zero rows: dropped
                const bool off = valid && jr != (int)e;
                const bool same = off && sl[buf][tr] == mylab;
                const float ex = __builtin_amdgcn_exp2f((cs - 1.0f) * escale);
                if constexpr (GRAD) {
                    float w = same ? ai + sa[buf][tr] : 0.f;
                    w -= ex * (bi + sb[buf][tr]);
                    acc[c][reg] = off ? w : 0.f;
                } else {
                    cmax = fmaxf(cmax, valid ? cs : -INFINITY);
                    esum += off ? ex : 0.f;
                    cnt += same ? 1.0f : 0.f;
                    cpos += same ? cs : 0.f;
                }
            }
        }
        if constexpr (GRAD) {
            // out[i][d] += sum_j w_ij Z[j][d]: step `reg` of the k loop pairs the two streamed rows the two half-waves hold in
            // accumulator register `reg`
#pragma unroll
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const float *brow = &it[buf][(c * 32 + acc_row(reg, half)) * LDW + col];   // B[k = half][d = lane&31 (+ 32 b)]
#pragma unroll
                    for (int b = 0; b < NB; ++b)
                        out[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[c][reg], brow[b * 32], out[b], 0, 0, 0);
                }
            }
        }
        if (more) deposit(buf ^ 1);                                     // the other buffer was last read one barrier ago
        __syncthreads();
    }
    if constexpr (GRAD) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int64_t r = e0 + wave * 32 + acc_row(reg, half);
                if (r < N) part[((int64_t)blockIdx.y * N + r) * D + b * 32 + col] = out[b][reg];
            }
        }
    } else {
        // the two half-waves hold disjoint streamed rows of the same resident row
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
        esum += __shfl_xor(esum, 32, 64);
        cnt += __shfl_xor(cnt, 32, 64);
        cpos += __shfl_xor(cpos, 32, 64);
        if (half == 0 && e < N) {
            float *st = stat + (int64_t)blockIdx.y * 4 * N + e;
            st[0] = cmax;
            st[N] = esum;
            st[2 * N] = cnt;
            st[3 * N] = cpos;
        }
    }
}

// Per row: the chunk partials folded in chunk order, the row's loss term and gradient coefficients
__global__ __launch_bounds__(kBlock) void sup_stats_kernel(int64_t N, int64_t chunks, const float *__restrict__ stat, float tau,
                                                           float *__restrict__ lterm, float *__restrict__ ra, float *__restrict__ rb) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    float cmax = -INFINITY, esum = 0.f, cnt = 0.f, cpos = 0.f;
    for (int64_t c = 0; c < chunks; ++c) {
        const float *st = stat + c * 4 * N + i;
        cmax = fmaxf(cmax, st[0]);
        esum += st[N];
        cnt += st[2 * N];
        cpos += st[3 * N];
    }
    // exp(l_ij) = e_ij r with r = exp(1/tau - 2 m_i), so E_i + 1e-10 = r (sum e_ij + 1e-10 / r) and
    // l_ij - log(E_i + 1e-10) = (c_ij - 1) / tau - log(sum e_ij + 1e-10 / r): the two 2 m_i cancel on paper, not in fp32
    const float m = cmax / tau;
    const float den = esum + kSupEps * expf(2.0f * m - 1.0f / tau);
    const float ci = cnt + kSupEps;
    lterm[i] = (-tau / ci) * ((cpos - cnt) / tau - cnt * logf(den));
    ra[i] = 1.0f / ci;
    rb[i] = (cnt / ci) / den;
}

__global__ __launch_bounds__(kBlock) void sup_loss_kernel(const float *__restrict__ lterm, int64_t N, float scale, int accumulate,
                                                          float *__restrict__ loss) {
    __shared__ float scratch[kBlock / 64];
    float v = 0.f;
    for (int64_t i = threadIdx.x; i < N; i += kBlock) v += lterm[i];
    const float r = block_sum(v, scratch);
    if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + scale * r;
}

// Per row: fold the chunk partials of sum_j w_ij z_j, scale by -weight / N, back through the normalisation of F_i
__global__ __launch_bounds__(kBlock) void sup_grad_kernel(int64_t N, int D, int64_t chunks, const float *__restrict__ part,
                                                          const float *__restrict__ Z, const float *__restrict__ inv, float scale,
                                                          float *__restrict__ gF) {
    const int64_t t = (int64_t)blockIdx.x * kNceTeamsPerBlock + (threadIdx.x / kNceTeam);
    const int l = threadIdx.x & (kNceTeam - 1);
    const bool live = t < N;
    const int64_t i = live ? t : 0;
    const int D4 = D / 4;
    NceRow H;
    H.v[0] = H.v[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t c = 0; c < chunks; ++c) nce_add(H, nce_load(part + (c * N + i) * (int64_t)D, D4, l));
    const NceRow z = nce_load(Z + i * (int64_t)D, D4, l);
    const NceRow g = nce_bwd(nce_axpby(H, scale, H, 0.f), z, inv[i]);
    if (live) nce_store(gF + i * (int64_t)D, D4, l, g);
}

// ------------------------------------------------------------------------------------------------ host side
static inline int sup_tile(int D) { return D <= 64 ? 64 : 32; }

// split of the N streamed rows into column chunks: a function of N and D alone
static void sup_chunks(int64_t N, int TS, int64_t &chunks, int64_t &chunk_rows) {
    const int64_t rb = (N + kSupRows - 1) / kSupRows, tiles = (N + TS - 1) / TS;
    const int64_t want = (kSupTargetWg + rb - 1) / rb;
    const int64_t ch = tiles < want ? tiles : want;
    const int64_t tpc = (tiles + ch - 1) / ch;
    chunks = (tiles + tpc - 1) / tpc;
    chunk_rows = tpc * TS;
}

struct SupLayout {
    int64_t Z, inv, lab, stat, lterm, ra, rb, part, total;   // byte offsets
};

static void sup_layout(int64_t N, int32_t D, SupLayout &L) {
    int64_t chunks, chunk_rows;
    sup_chunks(N, sup_tile(D), chunks, chunk_rows);
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t at = o; o += align_up(bytes, 256); return at; };
    L.Z = take(N * D * 4);
    L.inv = take(N * 4);
    L.lab = take(N * 8);
    L.stat = take(chunks * 4 * N * 4);
    L.lterm = take(N * 4);
    L.ra = take(N * 4);
    L.rb = take(N * 4);
    L.part = take(chunks * N * D * 4);
    L.total = o;
}

static int32_t sup_check(const char *entry, int64_t B, int32_t D) {
    WR_REQUIRE(wr_supcon_supported(D), WR_E_RANGE, "%s supports D in {32, 64, 128}; got D=%d", entry, D);
    WR_REQUIRE(B >= 1 && 2 * B <= kSupMaxRows, WR_E_SHAPE, "%s: B=%lld out of range (1 <= B, 2 B <= 2^15)", entry, (long long)B);
    return WR_OK;
}

template <bool GRAD>
static void sup_launch_pass(int32_t D, dim3 grid, hipStream_t stream, const float *Z, int64_t N, const int64_t *lab, const float *ra,
                            const float *rb, float escale, int64_t chunk_rows, float *stat, float *part) {
#define WR_SUP_PASS(KS_)                                                                                                    \
    hipLaunchKernelGGL((sup_pass_kernel<KS_, ((KS_) <= 32 ? 64 : 32), GRAD>), grid, dim3(kBlock), 0, stream, Z, N, lab, ra, rb, escale, \
                       chunk_rows, stat, part)
    WR_DISPATCH_KS(D, 16, 64, WR_SUP_PASS);                             // the tile height is sup_tile(D)
#undef WR_SUP_PASS
}

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_supcon_supported(int32_t D) { return (D == 32 || D == 64 || D == 128) ? 1 : 0; }

int64_t wr_supcon_workspace_bytes(int64_t B, int32_t D) {
    const int32_t rc = sup_check("wr_supcon_workspace_bytes", B, D);
    if (rc != WR_OK) return rc;
    SupLayout L;
    sup_layout(2 * B, D, L);
    return L.total;
}

int32_t wr_supcon_loss_grad(const float *F, int64_t B, int32_t D, const int64_t *labels, float tau, float *loss, int32_t accumulate,
                            float weight, float *gF, int32_t *err_word, void *workspace, int64_t workspace_bytes, void *stream_) {
    int32_t rc = sup_check("wr_supcon_loss_grad", B, D);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(F && labels && loss, WR_E_NULL, "wr_supcon_loss_grad: NULL argument");
    WR_REQUIRE(aligned16(F) && aligned16(gF), WR_E_ALIGN, "wr_supcon_loss_grad: F and gF must be 16-byte aligned");
    WR_REQUIRE(tau > 0.f && tau == tau && tau <= 3.0e38f, WR_E_RANGE, "wr_supcon_loss_grad: tau must be positive and finite");
    (void)err_word;                                                     // reserved: labels are compared, never dereferenced
    const int64_t N = 2 * B;
    SupLayout L;
    sup_layout(N, D, L);
    if ((rc = check_workspace("wr_supcon_loss_grad", workspace, workspace_bytes, L.total)) != WR_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    char *ws = reinterpret_cast<char *>(workspace);
    float *Z = reinterpret_cast<float *>(ws + L.Z), *inv = reinterpret_cast<float *>(ws + L.inv);
    int64_t *lab = reinterpret_cast<int64_t *>(ws + L.lab);
    float *stat = reinterpret_cast<float *>(ws + L.stat), *lterm = reinterpret_cast<float *>(ws + L.lterm);
    float *ra = reinterpret_cast<float *>(ws + L.ra), *rb = reinterpret_cast<float *>(ws + L.rb);
    float *part = reinterpret_cast<float *>(ws + L.part);
    const float escale = 1.44269504088896341f / tau;
    int64_t chunks, chunk_rows;
    sup_chunks(N, sup_tile(D), chunks, chunk_rows);
    const unsigned grid_team = (unsigned)((N + kNceTeamsPerBlock - 1) / kNceTeamsPerBlock);
    const dim3 grid((unsigned)((N + kSupRows - 1) / kSupRows), (unsigned)chunks);

    hipLaunchKernelGGL(sup_prep_kernel, dim3(grid_team), dim3(kBlock), 0, stream, F, N, B, D, labels, Z, inv, lab);
    WR_LAUNCH_CHECK("sup_prep_kernel");
    sup_launch_pass<false>(D, grid, stream, Z, N, lab, nullptr, nullptr, escale, chunk_rows, stat, nullptr);
    WR_LAUNCH_CHECK("sup_pass_kernel (statistics)");
    hipLaunchKernelGGL(sup_stats_kernel, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, N, chunks, stat, tau,
                       lterm, ra, rb);
    WR_LAUNCH_CHECK("sup_stats_kernel");
    hipLaunchKernelGGL(sup_loss_kernel, dim3(1), dim3(kBlock), 0, stream, lterm, N, weight / (float)N, accumulate, loss);
    WR_LAUNCH_CHECK("sup_loss_kernel");
    if (gF == nullptr) return WR_OK;
    sup_launch_pass<true>(D, grid, stream, Z, N, lab, ra, rb, escale, chunk_rows, nullptr, part);
    WR_LAUNCH_CHECK("sup_pass_kernel (gradient)");
    hipLaunchKernelGGL(sup_grad_kernel, dim3(grid_team), dim3(kBlock), 0, stream, N, D, chunks, part, Z, inv, -weight / (float)N, gF);
    WR_LAUNCH_CHECK("sup_grad_kernel");
    return WR_OK;
}

}  // extern "C"
