// wr_buir.hip — K16: BUIR's bootstrap loss (reference src/models/general/BUIR.py:76-97) with every gradient of it in one call,
// and K17: the momentum update of the target tables (BUIR.py:69-74).
//
// K16.  For sample k with online rows x_u, x_i, target rows t_u, t_i and the shared predictor p = W x + b:
//     c_ui = <p_u, t_i> / (max(|p_u|, eps) max(|t_i|, eps)),  c_iu likewise,  l_k = 4 - 2 c_ui - 2 c_iu,  loss = mean l_k
//     g_p  = (-2/B) (t^ - p^ c) / |p| = alpha t - beta p,  alpha = (-2/B) / (max(|p|, eps) max(|t|, eps)),  beta = (-2/B) c / max(|p|, eps)^2
//     g_x  = W^T g_p,   gW = sum_k g_pu x_u^T + g_pi x_i^T,   gb = sum_k g_pu + g_pi
// Targets are constants.  A row with |p| < eps takes the same two coefficients (torch's clamp passes no gradient to the norm
// there): that regime is not claimed.
//
// A wave owns a slab of 32 samples, a workgroup 128; W sits in LDS, rows padded to D + 1.  All three products are
// v_mfma_f32_32x32x2_f32 chains (tile layout: wr_score_tiles.h), the online rows read straight from the tables in the k loops:
//   phase 1, per side   P^T = W X^T  (tile rows = output features, tile column = the lane's sample): the per-sample sums |p|^2,
//                       <p, t>, |t|^2 run down the registers of a lane; the tile is rewritten as g_p and, rows being the summed
//                       index, is the A operand of g_x = g_p^T W as it stands (an accumulator tile as the next operand)
//   phase 2, per 32 output features   P = X W^T with the two operands swapped — the same fmaf chains, so the same bits — gives
//                       the tile with samples down the registers; rewritten as g_p from the coefficients phase 1 left in
//                       LDS it is the A operand of gW = g_p^T X, both sides into one accumulator; gb is its column sum
// The four waves' gW / gb are folded through LDS in wave order and written as the workgroup's partial; a second launch folds
// the partials in workgroup order.  No float atomics, the grid is a function of (B, D): same inputs, same bits, on any device.
#include "wr_row_team.h"
#include "wr_score_tiles.h"

namespace wr {

constexpr int kBuirRows = kScoreRows;             // samples per workgroup (32 per wave)
constexpr int64_t kBuirMaxBatch = int64_t(1) << 22;
constexpr int kBuirFoldElems = 16;                // output elements per workgroup of the fold launch
constexpr int kBuirFoldSlices = kBlock / kBuirFoldElems;

// floats of one workgroup's partial: gW [D, D], gb [D], the sum of the loss terms
static inline int64_t buir_partial_floats(int32_t D) { return (int64_t)D * D + D + 1; }
static inline int64_t buir_workgroups(int64_t B) { return (B + kBuirRows - 1) / kBuirRows; }

__device__ __forceinline__ int buir_clamp_id(int64_t v, int64_t n, bool &bad) {
    bad = v < 0 || v >= n;
    return (int)(v < 0 ? 0 : (v >= n ? n - 1 : v));
}

template <int KS, bool GRAD>
__global__ __launch_bounds__(kBlock, (KS == 64 ? 1 : 2)) void buir_kernel(const float *__restrict__ Uo, const float *__restrict__ Io,
                                                      const float *__restrict__ Ut, const float *__restrict__ It, int64_t n_users,
                                                      int64_t n_items, const float *__restrict__ W, const float *__restrict__ bias,
                                                      const int64_t *__restrict__ users, const int64_t *__restrict__ items, int64_t B,
                                                      float neg2_over_b, float *__restrict__ gU, float *__restrict__ gI,
                                                      float *__restrict__ part, int32_t *__restrict__ err_word) {
    constexpr int D = 2 * KS, LDW = D + 1, NB = D / 32;
    __shared__ float sW[D * LDW];
    __shared__ float sb[D];
    __shared__ int sid[2][kBuirRows];                 // clamped user / item id of every sample of the workgroup
    __shared__ float coef[2][kBuirRows][2];           // alpha, beta of the user-side and the item-side predictor output
    __shared__ float fold[GRAD ? 3 : 1][GRAD ? 32 * D : 1];
    __shared__ float foldb[3][32];
    __shared__ float scratch[kBlock / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = lane & 31, half = lane >> 5;
    const int64_t k0 = (int64_t)blockIdx.x * kBuirRows;
    const int slot = wave * 32 + col;                 // this lane's sample inside the workgroup
    const int64_t sample = k0 + slot;
    const bool valid = sample < B;

    for (int idx = threadIdx.x; idx < D * D; idx += kBlock) {
        const int o = idx / D, k = idx - o * D;
        sW[o * LDW + k] = W[idx];
    }
    if (threadIdx.x < D) sb[threadIdx.x] = bias[threadIdx.x];
    bool bad_u = false, bad_i = false;
    const int uid = buir_clamp_id(valid ? users[sample] : 0, n_users, bad_u);
    const int iid = buir_clamp_id(valid ? items[sample] : 0, n_items, bad_i);
    if ((bad_u || bad_i) && half == 0 && err_word != nullptr) atomicOr(err_word, 1);
    if (half == 0) {
        sid[0][slot] = uid;
        sid[1][slot] = iid;
    }
    // element k = 2s + (lane>>5) of the online rows of the lane's sample: the X operand of both orientations, read in the k
    // loop itself (a second visit finds the row in cache); a lane past the batch takes zeros
    const float *xur = Uo + (int64_t)uid * D + half, *xir = Io + (int64_t)iid * D + half;
    __syncthreads();

    // ---------------------------------------------------------------------------------------- phase 1
    float lterm = 0.f;
    auto side = [&](const float *__restrict__ xr, const float *__restrict__ trow, int which, float *__restrict__ gX) {
        // acc[ob][reg] = p[o = 32 ob + acc_row(reg, half)] of sample `col`, before the bias: A[i = o][k] = W, B[k][j = sample] = X
        f32x16 acc[NB];
#pragma unroll
        for (int ob = 0; ob < NB; ++ob) acc[ob] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 8
        for (int s = 0; s < KS; ++s) {
            const float xv = valid ? xr[2 * s] : 0.f;
#pragma unroll
            for (int ob = 0; ob < NB; ++ob)
                acc[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(sW[(ob * 32 + col) * LDW + 2 * s + half], xv, acc[ob], 0, 0, 0);
        }
        float pp = 0.f, pt = 0.f, tt = 0.f;
#pragma unroll
        for (int ob = 0; ob < NB; ++ob) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = ob * 32 + 8 * q + 4 * half;                // acc_row(4 q, half): registers 4q .. 4q+3 are o .. o+3
                const float4 t4 = valid ? *reinterpret_cast<const float4 *>(trow + o) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float tv[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = acc[ob][4 * q + r] + sb[o + r];
                    acc[ob][4 * q + r] = p;
                    pp += p * p;
                    pt += p * tv[r];
                    tt += tv[r] * tv[r];
                }
            }
        }
        pp += __shfl_xor(pp, 32, 64);
        pt += __shfl_xor(pt, 32, 64);
        tt += __shfl_xor(tt, 32, 64);
        const float mp = fmaxf(sqrtf(pp), kNceEps), mt = fmaxf(sqrtf(tt), kNceEps);
        const float c = (pt / mp) / mt;
        const float alpha = valid ? (neg2_over_b / mp) / mt : 0.f;
        const float beta = valid ? ((neg2_over_b * c) / mp) / mp : 0.f;
        if (valid && half == 0) lterm += 2.0f - 2.0f * c;
        if constexpr (GRAD) {
            if (half == 0) {
                coef[which][slot][0] = alpha;
                coef[which][slot][1] = beta;
            }
#pragma unroll
            for (int ob = 0; ob < NB; ++ob) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int o = ob * 32 + 8 * q + 4 * half;
                    const float4 t4 = valid ? *reinterpret_cast<const float4 *>(trow + o) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float tv[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[ob][4 * q + r] = alpha * tv[r] - beta * acc[ob][4 * q + r];
                }
            }
            // g_x[sample][k'] = sum_o g_p[o][sample] W[o][k']: step `reg` pairs the two output features that the two half-waves
            // hold in accumulator register `reg`
#pragma unroll 1
            for (int kb = 0; kb < NB; ++kb) {
                f32x16 out = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int ob = 0; ob < NB; ++ob) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg)
                        out = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[ob][reg], sW[(ob * 32 + acc_row(reg, half)) * LDW + kb * 32 + col],
                                                                   out, 0, 0, 0);
                }
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int64_t r = k0 + wave * 32 + acc_row(reg, half);
                    if (r < B) gX[r * (int64_t)D + kb * 32 + col] = out[reg];
                }
            }
        }
    };
    side(xur, It + (int64_t)iid * D, 0, gU);         // the user's prediction against the item's target row
    side(xir, Ut + (int64_t)uid * D, 1, gI);
    {
        const float r = block_sum(lterm, scratch);  // holds a barrier: coef and sid are visible to phase 2
        if (threadIdx.x == 0) part[(int64_t)blockIdx.x * ((int64_t)D * D + D + 1) + (int64_t)D * D + D] = r;
    }

    // ---------------------------------------------------------------------------------------- phase 2
    if constexpr (GRAD) {
        float *mine = part + (int64_t)blockIdx.x * ((int64_t)D * D + D + 1);
#pragma unroll 1
        for (int ob = 0; ob < NB; ++ob) {
            f32x16 accw[NB];
#pragma unroll
            for (int kb = 0; kb < NB; ++kb) accw[kb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            float gbv = 0.f;
            const int o = ob * 32 + col;                                  // this lane's output feature
            auto side2 = [&](const float *__restrict__ xr, const float *__restrict__ T, const float *__restrict__ X, int which) {
                // p2[reg] = p[o] of sample acc_row(reg, half) of the slab, before the bias: A[i = sample][k] = X, B[k][j = o] = W
                f32x16 p2 = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 8
                for (int s = 0; s < KS; ++s)
                    p2 = __builtin_amdgcn_mfma_f32_32x32x2f32(valid ? xr[2 * s] : 0.f, sW[o * LDW + 2 * s + half], p2, 0, 0, 0);
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int sl = wave * 32 + acc_row(reg, half);
                    const bool live = k0 + sl < B;
                    const float alpha = coef[which][sl][0], beta = coef[which][sl][1];
                    const float t = T[(int64_t)sid[which ^ 1][sl] * D + o];
                    const float p = p2[reg] + sb[o];
                    const float g = live ? alpha * t - beta * p : 0.f;
                    gbv += g;
                    const float *xrow = X + (int64_t)sid[which][sl] * D + col;
#pragma unroll
                    for (int kb = 0; kb < NB; ++kb)
                        accw[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(g, xrow[kb * 32], accw[kb], 0, 0, 0);
                }
            };
            side2(xur, It, Uo, 0);
            side2(xir, Ut, Io, 1);
            gbv += __shfl_xor(gbv, 32, 64);
            // accw[kb][reg] = this wave's share of gW[32 ob + acc_row(reg, half)][32 kb + col]; folded in wave order
            if (wave > 0) {
#pragma unroll
                for (int kb = 0; kb < NB; ++kb) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) fold[wave - 1][acc_row(reg, half) * D + kb * 32 + col] = accw[kb][reg];
                }
                if (half == 0) foldb[wave - 1][col] = gbv;
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int w = 0; w < 3; ++w) {
#pragma unroll
                    for (int kb = 0; kb < NB; ++kb) {
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) accw[kb][reg] += fold[w][acc_row(reg, half) * D + kb * 32 + col];
                    }
                    gbv += foldb[w][col];
                }
#pragma unroll
                for (int kb = 0; kb < NB; ++kb) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) mine[(ob * 32 + acc_row(reg, half)) * D + kb * 32 + col] = accw[kb][reg];
                }
                if (half == 0) mine[D * D + o] = gbv;
            }
            __syncthreads();
        }
    }
}

// out element e = sum over the workgroups' partials of element e0 + e, in workgroup order: slice q of a thread group takes a
// contiguous range of workgroups, the slices are added in slice order.  Elements: gW (D*D), gb (D), the loss sum (scaled).
__global__ __launch_bounds__(kBlock) void buir_fold_kernel(const float *__restrict__ part, int64_t n_wg, int64_t stride, int64_t e0,
                                                           int64_t n_elems, int64_t dd, int64_t d, float loss_scale,
                                                           float *__restrict__ gW, float *__restrict__ gb, float *__restrict__ loss) {
    __shared__ float sl[kBuirFoldSlices][kBuirFoldElems];
    const int el = threadIdx.x % kBuirFoldElems, q = threadIdx.x / kBuirFoldElems;
    const int64_t e = e0 + (int64_t)blockIdx.x * kBuirFoldElems + el;
    const bool live = e < e0 + n_elems;
    const int64_t per = (n_wg + kBuirFoldSlices - 1) / kBuirFoldSlices;
    const int64_t w0 = q * per, w1 = (w0 + per < n_wg) ? w0 + per : n_wg;
    float a = 0.f;
    if (live) {
#pragma unroll 8
        for (int64_t w = w0; w < w1; ++w) a += part[w * stride + e];
    }
    sl[q][el] = a;
    __syncthreads();
    if (q == 0 && live) {
        float r = 0.f;
#pragma unroll
        for (int s = 0; s < kBuirFoldSlices; ++s) r += sl[s][el];
        if (e < dd) gW[e] = r;
        else if (e < dd + d) gb[e - dd] = r;
        else loss[0] = r * loss_scale;
    }
}

// K17: t = t m + o (1 - m), three roundings (ema_elem of wr_common.h, shared with the row replays of wr_rowopt.hip)
__global__ __launch_bounds__(kBlock) void ema_kernel(float *__restrict__ t, const float *__restrict__ o, int64_t n, float m,
                                                     float one_minus_m) {
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
        float4 a = reinterpret_cast<float4 *>(t)[i];
        const float4 b = reinterpret_cast<const float4 *>(o)[i];
        a.x = ema_elem(a.x, b.x, m, one_minus_m);
        a.y = ema_elem(a.y, b.y, m, one_minus_m);
        a.z = ema_elem(a.z, b.z, m, one_minus_m);
        a.w = ema_elem(a.w, b.w, m, one_minus_m);
        reinterpret_cast<float4 *>(t)[i] = a;
    }
    if (blockIdx.x == 0) {
        const int64_t i = (n4 << 2) + threadIdx.x;                        // fewer than 4 elements past the last whole float4
        if (i < n) t[i] = ema_elem(t[i], o[i], m, one_minus_m);
    }
}

static int32_t buir_check(const char *entry, int64_t B, int32_t D) {
    WR_REQUIRE(wr_buir_supported(D), WR_E_RANGE, "%s supports D in {32, 64, 128}; got D=%d", entry, D);
    WR_REQUIRE(B >= 1 && B <= kBuirMaxBatch, WR_E_SHAPE, "%s: B=%lld out of range (1 <= B <= 2^22)", entry, (long long)B);
    return WR_OK;
}

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_buir_supported(int32_t D) { return (D == 32 || D == 64 || D == 128) ? 1 : 0; }

int64_t wr_buir_workspace_bytes(int64_t B, int32_t D) {
    const int32_t rc = buir_check("wr_buir_workspace_bytes", B, D);
    if (rc != WR_OK) return rc;
    return align_up(buir_workgroups(B) * buir_partial_floats(D) * 4, 256);
}

int32_t wr_buir_loss_grad(const float *user_online, const float *item_online, const float *user_target, const float *item_target,
                          int64_t n_users, int64_t n_items, int32_t D, const float *W, const float *b, const int64_t *users,
                          const int64_t *items, int64_t B, float *loss, float *gU, float *gI, float *gW, float *gb,
                          int32_t *err_word, void *workspace, int64_t workspace_bytes, void *stream_) {
    int32_t rc = buir_check("wr_buir_loss_grad", B, D);
    if (rc != WR_OK) return rc;
    rc = check_tables({{user_online, n_users, "user_online"}, {user_target, n_users, "user_target"},
                       {item_online, n_items, "item_online"}, {item_target, n_items, "item_target"}}, D);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(W && b && users && items && loss, WR_E_NULL, "wr_buir_loss_grad: NULL argument");
    const bool grad = gU != nullptr;
    WR_REQUIRE(!grad || (gI && gW && gb), WR_E_NULL, "wr_buir_loss_grad: gU without gI, gW or gb");
    WR_REQUIRE(aligned16(W) && aligned16(gU) && aligned16(gI) && aligned16(gW), WR_E_ALIGN,
               "wr_buir_loss_grad: W, gU, gI and gW must be 16-byte aligned");
    const int64_t n_wg = buir_workgroups(B), stride = buir_partial_floats(D);
    if ((rc = check_workspace("wr_buir_loss_grad", workspace, workspace_bytes, align_up(n_wg * stride * 4, 256))) != WR_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    float *part = reinterpret_cast<float *>(workspace);
    const float neg2_over_b = -2.0f / (float)B;
#define WR_BUIR_LAUNCH(KS_)                                                                                                      \
    do {                                                                                                                         \
        if (grad)                                                                                                                \
            hipLaunchKernelGGL((buir_kernel<KS_, true>), dim3((unsigned)n_wg), dim3(kBlock), 0, stream, user_online, item_online, \
                               user_target, item_target, n_users, n_items, W, b, users, items, B, neg2_over_b, gU, gI, part,     \
                               err_word);                                                                                        \
        else                                                                                                                     \
            hipLaunchKernelGGL((buir_kernel<KS_, false>), dim3((unsigned)n_wg), dim3(kBlock), 0, stream, user_online, item_online, \
                               user_target, item_target, n_users, n_items, W, b, users, items, B, neg2_over_b, gU, gI, part,     \
                               err_word);                                                                                        \
    } while (0)
    WR_DISPATCH_KS(D, 16, 64, WR_BUIR_LAUNCH);
#undef WR_BUIR_LAUNCH
    WR_LAUNCH_CHECK("buir_kernel");
    const int64_t dd = (int64_t)D * D;
    const int64_t e0 = grad ? 0 : dd + D, n_elems = grad ? stride : 1;
    hipLaunchKernelGGL(buir_fold_kernel, dim3((unsigned)((n_elems + kBuirFoldElems - 1) / kBuirFoldElems)), dim3(kBlock), 0, stream,
                       part, n_wg, stride, e0, n_elems, dd, (int64_t)D, 1.0f / (float)B, gW, gb, loss);
    WR_LAUNCH_CHECK("buir_fold_kernel");
    return WR_OK;
}

int32_t wr_ema_update(float *t, const float *o, int64_t n, float m, float one_minus_m, void *stream_) {
    WR_REQUIRE(t && o, WR_E_NULL, "wr_ema_update: NULL argument");
    WR_REQUIRE(n >= 1 && n < (int64_t(1) << 40), WR_E_SHAPE, "wr_ema_update: n=%lld out of range", (long long)n);
    WR_REQUIRE(aligned16(t) && aligned16(o), WR_E_ALIGN, "wr_ema_update: t and o must be 16-byte aligned");
    const int64_t n4 = n >> 2;
    int64_t blocks = (n4 + kBlock - 1) / kBlock;
    if (blocks < 1) blocks = 1;
    if (blocks > (1 << 20)) blocks = 1 << 20;
    hipLaunchKernelGGL(ema_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream_), t, o, n, m,
                       one_minus_m);
    WR_LAUNCH_CHECK("ema_kernel");
    return WR_OK;
}

}  // extern "C"
