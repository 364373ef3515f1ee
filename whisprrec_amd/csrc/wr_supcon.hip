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
#include "wr_pair_pass.h"

namespace wr {

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
// pair_pass (wr_pair_pass.h) with Z as both sides: resident rows i against the streamed rows j of the column chunk blockIdx.y,
// c = <Z[j], Z[i]>, e = exp2((c - 1) * escale).
//   !GRAD   stat[chunk][0..3][i] = max_j c,  sum_{j != i} e,  |{j != i : lab_j == lab_i}|,  sum over those j of c
//    GRAD   part[chunk][i][:]    = sum_{j != i} ([lab_j == lab_i] (ra_i + ra_j) - e (rb_i + rb_j)) Z[j][:]
// The policy is a local struct of the kernel so that it names the kernel's LDS arrays itself (as in wr_infonce.hip).
template <int KS, int TS, bool GRAD>
__global__ __launch_bounds__(kBlock, 2) void sup_pass_kernel(const float *__restrict__ Z, int64_t N, const int64_t *__restrict__ lab,
                                                            const float *__restrict__ ra, const float *__restrict__ rb, float escale,
                                                            int64_t chunk_rows, float *__restrict__ stat, float *__restrict__ part) {
    __shared__ int64_t sl[2][TS];                                       // label and (GRAD) coefficients of every row of the
    __shared__ float sa[2][TS], sb[2][TS];                              // two tiles
    struct Policy {
        const int64_t *__restrict__ lab;
        const float *__restrict__ ra, *__restrict__ rb;
        float escale;
        float *__restrict__ stat;
        int bound = 0;                                                      // end of the chunk.  N <= 2^15: row numbers fit an int
        int64_t mylab = 0;                                                  // of the lane's resident row, as ai and bi
        float ai = 0.f, bi = 0.f;
        int64_t lstage = 0;
        float astage = 0.f, bstage = 0.f;
        float cmax = -INFINITY, esum = 0.f, cnt = 0.f, cpos = 0.f;

        __device__ __forceinline__ void start(int64_t e, int64_t N, int64_t c1) {
            const int64_t er = e < N ? e : 0;
            bound = (int)c1;
            mylab = lab[er];
            if constexpr (GRAD) {
                ai = ra[er];
                bi = rb[er];
            }
        }
        __device__ __forceinline__ void fetch_side(int64_t r, bool in) {
            lstage = lab[in ? r : 0];
            if constexpr (GRAD) {
                astage = in ? ra[r] : 0.f;
                bstage = in ? rb[r] : 0.f;
            }
        }
        __device__ __forceinline__ void deposit_side(int buf) {
            sl[buf][threadIdx.x] = lstage;
            if constexpr (GRAD) {
                sa[buf][threadIdx.x] = astage;
                sb[buf][threadIdx.x] = bstage;
            }
        }
        __device__ __forceinline__ float weight(float cs, int tr, int64_t j0, int64_t e, int buf) {
            const int jr = (int)j0 + tr;
            const bool valid = jr < bound;                                  // rows past the chunk's end are zero rows: dropped
            const bool off = valid && jr != (int)e;
            const bool same = off && sl[buf][tr] == mylab;
            const float ex = __builtin_amdgcn_exp2f((cs - 1.0f) * escale);
            if constexpr (GRAD) {
                float w = same ? ai + sa[buf][tr] : 0.f;
                w -= ex * (bi + sb[buf][tr]);
                return off ? w : 0.f;
            } else {
                cmax = fmaxf(cmax, valid ? cs : -INFINITY);
                esum += off ? ex : 0.f;
                cnt += same ? 1.0f : 0.f;
                cpos += same ? cs : 0.f;
                return cs;                                                  // no product follows the statistics pass
            }
        }
        __device__ __forceinline__ void finish(int64_t e, int64_t N, int half) {
            if constexpr (!GRAD) {
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
    } P{lab, ra, rb, escale, stat};
    pair_pass<KS, TS, GRAD>(P, Z, N, Z, N, chunk_rows, part);
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

// ------------------------------------------------------------------------------------------------ host side
struct SupWs {
    float *Z, *inv;
    int64_t *lab;
    float *stat, *lterm, *ra, *rb, *part;
    int64_t chunks, chunk_rows;              // the split of the N streamed rows into column chunks: a function of N and D alone
    int64_t total;
};

static SupWs sup_carve(void *workspace, int64_t N, int32_t D) {
    Carver c(workspace);
    SupWs W;
    pair_chunks(N, N, pair_tile(D), kSupTargetWg, W.chunks, W.chunk_rows);
    W.Z = c.take<float>(N * D);
    W.inv = c.take<float>(N);
    W.lab = c.take<int64_t>(N);
    W.stat = c.take<float>(W.chunks * 4 * N);
    W.lterm = c.take<float>(N);
    W.ra = c.take<float>(N);
    W.rb = c.take<float>(N);
    W.part = c.take<float>(W.chunks * N * D);
    W.total = c.bytes;
    return W;
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
    hipLaunchKernelGGL((sup_pass_kernel<KS_, pair_tile(2 * (KS_)), GRAD>), grid, dim3(kBlock), 0, stream, Z, N, lab, ra, rb, escale, \
                       chunk_rows, stat, part)
    WR_DISPATCH_KS(D, 16, 64, WR_SUP_PASS);
#undef WR_SUP_PASS
}

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_supcon_supported(int32_t D) { return (D == 32 || D == 64 || D == 128) ? 1 : 0; }

int64_t wr_supcon_workspace_bytes(int64_t B, int32_t D) {
    const int32_t rc = sup_check("wr_supcon_workspace_bytes", B, D);
    if (rc != WR_OK) return rc;
    return sup_carve(nullptr, 2 * B, D).total;
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
    const SupWs W = sup_carve(workspace, N, D);
    if ((rc = check_workspace("wr_supcon_loss_grad", workspace, workspace_bytes, W.total)) != WR_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const float escale = 1.44269504088896341f / tau;
    const unsigned grid_team = (unsigned)((N + kNceTeamsPerBlock - 1) / kNceTeamsPerBlock);
    const dim3 grid((unsigned)((N + kPairRows - 1) / kPairRows), (unsigned)W.chunks);

    hipLaunchKernelGGL(sup_prep_kernel, dim3(grid_team), dim3(kBlock), 0, stream, F, N, B, D, labels, W.Z, W.inv, W.lab);
    WR_LAUNCH_CHECK("sup_prep_kernel");
    sup_launch_pass<false>(D, grid, stream, W.Z, N, W.lab, nullptr, nullptr, escale, W.chunk_rows, W.stat, nullptr);
    WR_LAUNCH_CHECK("sup_pass_kernel (statistics)");
    hipLaunchKernelGGL(sup_stats_kernel, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, N, W.chunks, W.stat, tau,
                       W.lterm, W.ra, W.rb);
    WR_LAUNCH_CHECK("sup_stats_kernel");
    hipLaunchKernelGGL(pair_loss_kernel, dim3(1), dim3(kBlock), 0, stream, W.lterm, N, weight / (float)N, accumulate, loss);
    WR_LAUNCH_CHECK("pair_loss_kernel");
    if (gF == nullptr) return WR_OK;
    sup_launch_pass<true>(D, grid, stream, W.Z, N, W.lab, W.ra, W.rb, escale, W.chunk_rows, nullptr, W.part);
    WR_LAUNCH_CHECK("sup_pass_kernel (gradient)");
    // per row: sum_j w_ij z_j, scaled by -weight / N, back through the normalisation of F_i
    hipLaunchKernelGGL(pair_grad_kernel, dim3(grid_team), dim3(kBlock), 0, stream, N, D, W.chunks, W.part, W.Z, W.inv,
                       -weight / (float)N, gF);
    WR_LAUNCH_CHECK("pair_grad_kernel");
    return WR_OK;
}

}  // extern "C"
