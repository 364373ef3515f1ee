// wr_pair_pass.h — the streamed pair pass shared by wr_infonce.hip (K12) and wr_supcon.hip (K15), and the host and row-kernel
// pieces around it.
//
// A pass pairs every resident row with every streamed row of one chunk: kPairRows resident rows per workgroup stay in
// registers (32 per wave), the streamed rows go through LDS in double-buffered tiles of TS, one barrier per tile.  The scores
// exist only as TRANSPOSED accumulator tiles (streamed rows x resident rows, score_tiles of wr_score_tiles.h), which leaves
// every lane holding the weights of its own resident row in the A-operand layout of the next MFMA: weights x streamed rows
// runs on the matrix cores without a trip through LDS.  What a loss adds is a policy (a struct of the .hip file, resolved at
// compile time):
//   start(e, nr, c1)          before the first tile: the lane's resident row e (a real row if e < nr) and the chunk's end c1
//   fetch_side(r, in)         threads below TS: load the side values of streamed row r into registers (`in`: r is inside the chunk)
//   deposit_side(buf)         threads below TS: store them beside tile `buf`
//   weight(s, tr, j0, e, buf) the score s of streamed row j0 + tr (row tr of tile `buf`, which starts at row j0) against the
//                             lane's resident row e -> the weight of that pair; the policy accumulates its own per-row
//                             statistics here
//   finish(e, nr, half)       after the last tile: fold the two half-waves (they hold disjoint streamed rows of the same
//                             resident row) and store what the loss keeps beside `part`
// Define the policy as a LOCAL struct of the kernel, after the kernel's __shared__ side arrays, so that its methods name those
// arrays themselves.  Reached through pointer or reference members the same LDS reads compile to other address arithmetic
// (3 to 5 more VGPRs in the InfoNCE gradient pass).  weight() gets j0 and tr apart, not their sum, so that a policy whose
// row numbers fit an int (SupCon: N <= 2^15) can compare them as `(int)j0 + tr`.
// No float atomics: every sum has a fixed order.
#pragma once
#include "wr_row_team.h"
#include "wr_score_tiles.h"

namespace wr {

constexpr int kPairRows = kScoreRows;     // resident rows per workgroup (32 per wave)

// Resident rows R [nr, D] as the B operand, streamed rows T [nt, D] of the chunk blockIdx.y as the A operand:
//     w_ij = P.weight(<T[i], R[j]>, ...)  (k-ordered chain),   part[chunk][j][:] = sum_i w_ij * T[i][:]   (GRAD only)
// Streamed rows past the chunk's end are zero rows; the policy gives them weight 0.  Static LDS: 2 tiles.
template <int KS, int TS, bool GRAD, typename Policy>
__device__ __forceinline__ void pair_pass(Policy &P, const float *R, int64_t nr, const float *T, int64_t nt, int64_t chunk_rows,
                                          float *part) {
    constexpr int D = 2 * KS, LDW = D + 1, C = TS / 32, NB = D / 32;
    __shared__ float it[2][TS * LDW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = lane & 31, half = lane >> 5;
    const int64_t e0 = (int64_t)blockIdx.x * kPairRows;
    const int64_t c0 = (int64_t)blockIdx.y * chunk_rows;
    const int64_t c1 = (c0 + chunk_rows < nt) ? c0 + chunk_rows : nt;
    const int64_t e = e0 + wave * 32 + col;
    // B[k = 2s + (lane>>5)][j = lane&31] of this wave's slab of resident rows
    float a[KS];
    {
        const float *rrow = R + ((e < nr) ? e : 0) * (int64_t)D + half;
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = (e < nr) ? rrow[2 * s] : 0.f;
    }
    P.start(e, nr, c1);
    f32x16 out[GRAD ? NB : 1];
#pragma unroll
    for (int b = 0; b < (GRAD ? NB : 1); ++b) out[b] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    TileStager<D, TS> stager;
    auto fetch = [&](int64_t j0) {
        stager.fetch(T, j0, c1);
        if (threadIdx.x < TS) P.fetch_side(j0 + threadIdx.x, j0 + threadIdx.x < c1);
    };
    auto deposit = [&](int buf) {
        stager.deposit(it[buf]);
        if (threadIdx.x < TS) P.deposit_side(buf);
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
                const int tr = c * 32 + acc_row(reg, half);
                acc[c][reg] = P.weight(acc[c][reg], tr, j0, e, buf);
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
    P.finish(e, nr, half);
    if constexpr (GRAD) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int64_t r = e0 + wave * 32 + acc_row(reg, half);
                if (r < nr) part[((int64_t)blockIdx.y * nr + r) * D + b * 32 + col] = out[b][reg];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ row kernels
// loss = (accumulate ? loss : 0) + scale * sum of the n terms, folded by one workgroup in a fixed order
static __global__ __launch_bounds__(kBlock) void pair_loss_kernel(const float *__restrict__ lterm, int64_t n, float scale,
                                                                  int accumulate, float *__restrict__ loss) {
    __shared__ float scratch[kBlock / 64];
    float v = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) v += lterm[i];
    const float r = block_sum(v, scratch);
    if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + scale * r;
}

// Per resident row: fold the chunk partials part[chunk][row][:] in chunk order, scale, back through the normalisation that
// made Y[row] (signed reciprocal norm inv[row]), store g[row]
static __global__ __launch_bounds__(kBlock) void pair_grad_kernel(int64_t n, int D, int64_t chunks, const float *__restrict__ part,
                                                                  const float *__restrict__ Y, const float *__restrict__ inv,
                                                                  float scale, float *__restrict__ g) {
    const int64_t t = (int64_t)blockIdx.x * kNceTeamsPerBlock + (threadIdx.x / kNceTeam);
    const int l = threadIdx.x & (kNceTeam - 1);
    const bool live = t < n;
    const int64_t j = live ? t : 0;
    const int D4 = D / 4;
    NceRow H;
    H.v[0] = H.v[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t c = 0; c < chunks; ++c) nce_add(H, nce_load(part + (c * n + j) * (int64_t)D, D4, l));
    const NceRow y = nce_load(Y + j * (int64_t)D, D4, l);
    const NceRow r = nce_bwd(nce_axpby(H, scale, H, 0.f), y, inv[j]);
    if (live) nce_store(g + j * (int64_t)D, D4, l, r);
}

// ------------------------------------------------------------------------------------------------ host side
// height of a streamed tile: two tiles of D + 1 padded rows stay near 33 KiB of LDS
static constexpr int pair_tile(int D) { return D <= 64 ? 64 : 32; }

// Split of the nt streamed rows of a pass with nr resident rows into chunks of whole tiles, aiming at target_wg workgroups:
// chunks * nr <= target_wg * kPairRows + nr + kPairRows.  The split fixes the order of the sums.
static void pair_chunks(int64_t nr, int64_t nt, int TS, int64_t target_wg, int64_t &chunks, int64_t &chunk_rows) {
    const int64_t rb = (nr + kPairRows - 1) / kPairRows, tiles = (nt + TS - 1) / TS;
    const int64_t want = (target_wg + rb - 1) / rb;
    const int64_t ch = tiles < want ? tiles : want;
    const int64_t tpc = (tiles + ch - 1) / ch;
    chunks = (tiles + tpc - 1) / tpc;
    chunk_rows = tpc * TS;
}

// Carves typed arrays out of a workspace in 256-byte steps.  With a NULL base the pointers are NULL and `bytes` ends as the
// size the workspace needs: one function lays the workspace out and sizes it.
struct Carver {
    char *base;
    int64_t bytes = 0;
    explicit Carver(void *workspace) : base(static_cast<char *>(workspace)) {}
    template <typename T>
    T *take(int64_t count) {
        T *p = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
        bytes += align_up(count * (int64_t)sizeof(T), 256);
        return p;
    }
};

}  // namespace wr
