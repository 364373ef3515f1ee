// wr_score_tiles.h — the score tiles on the matrix cores.  The two scans: wr_eval.hip and wr_topk.hip.  TileStager, score_tiles
// and acc_row without a scan: the streamed pair pass of wr_pair_pass.h (wr_infonce.hip, wr_supcon.hip).  The tile layout
// (f32x16, acc_row) and WR_DISPATCH_KS alone: wr_buir.hip.
//
// scores = rows x items^T on the matrix cores: v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate = a k-ordered fmaf chain
// started at 0, MI355X_MICROARCH.md "Matrix cores"), one 32x32 tile per wave and 32-item column block.  A workgroup =
// 4 waves = kScoreRows rows sharing each item tile through LDS; the scores never leave the accumulator registers, a
// per-tile consumer takes them from there.  Two scans:
//   score_scan_rega  D = 2*KS in {8, 16, 32, 64}: a wave's 32 rows stay in KS registers as the A operand, item tiles of
//                    kScoreTile rows are double-buffered in LDS (the next tile's global loads fly while the current one
//                    feeds the matrix cores), one barrier per tile
//   score_scan_lds   any other D: the rows and one tile of kScoreTileG items in dynamic LDS, two barriers per tile
// Both take two row arrays, because a row has two roles that sequential models keep apart: qrows[e] is the row of the
// query matrix that row e scores with (NULL: row e itself), mrows[e] the row of the mask CSR that hides items from it (read
// only when a mask is given).  Factor models pass their user ids for both.
// Consumer contract (both scans), consume(acc, j0, plain, masked):
//   acc[c][reg]      score of row acc_row(reg, lane >> 5) of the wave's slab against item j0 + 32 c + (lane & 31)
//   plain            wave-uniform.  True: no row of the slab has a masked item in the tile and the whole tile lies inside
//                    the table, so neither has to be tested.  False says nothing (score_scan_lds never claims it)
//   masked(c, row)   is item j0 + 32 c + (lane & 31) masked for row `row` of the slab; valid until the consumer returns
//   columns at or past n_items hold the score of an all-zero item row and must be dropped (j0 + 32 c + col < n_items)
//   rows at or past n hold the scores of an all-zero row and have empty bitmaps: the consumer's own per-row state must
//   keep them from counting
#pragma once
#include "wr_common.h"

namespace wr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kScoreRows = 128;   // rows per workgroup (32 per wave)
constexpr int kScoreTile = 64;    // items per tile, register-operand scan
constexpr int kScoreTileG = 32;   // items per tile, LDS-operand scan

// row inside the 32x32 tile that accumulator register `reg` of a lane in half-wave `half` holds (its column: lane & 31)
__device__ __forceinline__ constexpr int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// One tile of TS rows of D floats on its way from a row-major table into LDS rows padded to D + 1 floats (conflict-free
// column reads): fetch() issues the global loads into registers, deposit() stores them once the tile's buffer is free.
template <int D, int TS>
struct TileStager {
    static constexpr int LDW = D + 1, D4 = D / 4;
    static constexpr int NLOAD = (TS * D4 + kBlock - 1) / kBlock;        // float4 loads per thread and tile
    float4 stage[NLOAD];

    // rows j0 .. j0 + TS - 1 of T; rows at or past `bound` read as zeros
    __device__ __forceinline__ void fetch(const float *__restrict__ T, int64_t j0, int64_t bound) {
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
            const int f = threadIdx.x + i * kBlock;
            const int r = f / D4, k4 = f - r * D4;
            stage[i] = (f < TS * D4 && j0 + r < bound)
                           ? reinterpret_cast<const float4 *>(T + (j0 + r) * (int64_t)D)[k4] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __device__ __forceinline__ void deposit(float *tile) const {          // tile: [TS][LDW]
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
            const int f = threadIdx.x + i * kBlock;
            if (f < TS * D4) {
                const int r = f / D4, k4 = f - r * D4;
                float *dst = &tile[r * LDW + 4 * k4];
                dst[0] = stage[i].x; dst[1] = stage[i].y; dst[2] = stage[i].z; dst[3] = stage[i].w;
            }
        }
    }
};

// Thread t < kScoreRows walks the ascending mask list (CSR: mask_ptr / mask_idx) of row e0 + t along the item chunk.  The
// next masked item waits in a register: a tile without masked items (almost all of them) costs no memory access.
struct MaskCursor {
    const int *idx;
    int64_t cur = 0, cend = 0;
    int nxt = 0x7fffffff;

    // positioned at the first masked item >= c0 of row e (mask row mrows[e]); no list, or e >= n: an empty one
    __device__ __forceinline__ MaskCursor(const int64_t *__restrict__ mask_ptr, const int *__restrict__ mask_idx,
                                          const int64_t *__restrict__ mrows, int64_t e, int64_t n, int64_t c0)
        : idx(mask_idx) {
        if (threadIdx.x < kScoreRows && mask_ptr != nullptr && e < n) {
            const int64_t uu = mrows[e];
            int64_t lo = mask_ptr[uu], hi = mask_ptr[uu + 1];
            cend = hi;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if ((int64_t)mask_idx[mid] < c0) lo = mid + 1; else hi = mid;
            }
            cur = lo;
            load();
        }
    }
    __device__ __forceinline__ void load() { nxt = (cur < cend) ? idx[cur] : 0x7fffffff; }

    // bitmaps of the row's masked items among j0 .. j0 + 32 C - 1 (tiles are visited in ascending order); word c goes to
    // out[c * kScoreRows].  Returns the OR of the words.
    template <int C>
    __device__ __forceinline__ unsigned advance(int64_t j0, unsigned *out) {
        unsigned m[C];
#pragma unroll
        for (int c = 0; c < C; ++c) m[c] = 0;
        while ((int64_t)nxt < j0 + 32 * C) {
            const int64_t d = (int64_t)nxt - j0;
            if (d >= 0) m[d >> 5] |= 1u << (unsigned)(d & 31);
            ++cur;
            load();
        }
        unsigned any = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            out[c * kScoreRows] = m[c];
            any |= m[c];
        }
        return any;
    }

    // anymask[w] = does any row of slab w have a masked item in the tile?  Called by the threads below kScoreRows: rows
    // 0..127 sit in waves 0 and 1, slab w = rows 32w..32w+31 = lanes 32(w&1).. of wave w>>1
    static __device__ __forceinline__ void publish_any(unsigned any, unsigned *anymask) {
        const unsigned long long bal = __ballot(any != 0);
        if ((threadIdx.x & 63) == 0) {
            const int wave = threadIdx.x >> 6;
            anymask[2 * wave] = (unsigned)(bal & 0xffffffffull) != 0;
            anymask[2 * wave + 1] = (unsigned)(bal >> 32) != 0;
        }
    }
};

// acc[c] = the 32x32 product of the 32 rows held in registers (r[s]: element k = 2s + (lane>>5) of row lane&31) with rows
// 32c .. 32c+31 of the LDS tile (t: element `lane>>5` of row `lane&31` of block 0, rows LDW apart), s ascending, one MFMA per
// k-pair.  The C column blocks are independent accumulator chains: a dependent MFMA waits for its predecessor's result,
// an independent one issues right behind it.  STREAM_A: the tile is the A operand (acc rows = tile rows, acc column = the
// register row) instead of B (acc rows = register rows, acc column = tile row).
template <int KS, int C, int LDW, bool STREAM_A>
__device__ __forceinline__ void score_tiles(const float (&r)[KS], const float *t, f32x16 (&acc)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float v = t[c * 32 * LDW + 2 * s];
            acc[c] = STREAM_A ? __builtin_amdgcn_mfma_f32_32x32x2f32(v, r[s], acc[c], 0, 0, 0)
                              : __builtin_amdgcn_mfma_f32_32x32x2f32(r[s], v, acc[c], 0, 0, 0);
        }
    }
}

// the same chain for one tile with both operands in LDS and D known at run time
__device__ __forceinline__ void score_tile_lds(const float *arow, const float *brow, int D, f32x16 &acc) {
    acc = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k0 = 0; k0 < D; k0 += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[k0], brow[k0], acc, 0, 0, 0);
}

// Register-operand scan of the items c0 .. min(c0 + chunk, n_items) - 1 against the rows U[qrows[e]] (qrows NULL: U[e]),
// e = blockIdx.x * kScoreRows + 0..127 (e < n), masked by the lists of mrows[e].
// Static LDS: 2 tiles, 2 x 2 x 128 bitmap words, 2 x 4 slab flags.
template <int KS, typename Consumer>
__device__ __forceinline__ void score_scan_rega(const float *__restrict__ U, const float *__restrict__ I, int64_t n_items,
                                                const int64_t *__restrict__ qrows, const int64_t *__restrict__ mrows,
                                                int64_t n, const int64_t *__restrict__ mask_ptr,
                                                const int *__restrict__ mask_idx, int64_t c0, int64_t chunk,
                                                Consumer &&consume) {
    constexpr int D = 2 * KS, LDW = D + 1, C = kScoreTile / 32;
    __shared__ float it[2][kScoreTile * LDW];
    __shared__ unsigned rowmask[2][C][kScoreRows];
    __shared__ unsigned anymask[2][kBlock / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = lane & 31, half = lane >> 5;
    const int64_t e0 = (int64_t)blockIdx.x * kScoreRows;
    const int64_t c1 = (c0 + chunk < n_items) ? c0 + chunk : n_items;
    // A[i = lane&31][k = 2s + (lane>>5)] of this wave's slab
    float a[KS];
    {
        const int64_t e = e0 + wave * 32 + col;
        const float *urow = U + ((e < n) ? (qrows != nullptr ? qrows[e] : e) : 0) * (int64_t)D + half;
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = (e < n) ? urow[2 * s] : 0.f;
    }
    MaskCursor cursor(mask_ptr, mask_idx, mrows, e0 + threadIdx.x, n, c0);
    TileStager<D, kScoreTile> stager;
    auto deposit = [&](int buf, int64_t j0) {
        stager.deposit(it[buf]);
        if (threadIdx.x < kScoreRows)
            MaskCursor::publish_any(cursor.advance<C>(j0, &rowmask[buf][0][threadIdx.x]), anymask[buf]);
    };
    stager.fetch(I, c0, n_items);
    deposit(0, c0);
    __syncthreads();
    int buf = 0;
    for (int64_t j0 = c0; j0 < c1; j0 += kScoreTile, buf ^= 1) {
        const bool more = j0 + kScoreTile < c1;
        if (more) stager.fetch(I, j0 + kScoreTile, n_items);    // global loads fly while the matrix cores work
        {
            f32x16 acc[C];
            // B[k = 2s + (lane>>5)][j = lane&31] of block 0
            score_tiles<KS, C, LDW, false>(a, &it[buf][col * LDW + half], acc);
            const bool plain = anymask[buf][wave] == 0 && j0 + kScoreTile <= n_items;
            const int b = buf;
            consume(acc, j0, plain, [&](int c, int row) { return ((rowmask[b][c][wave * 32 + row] >> col) & 1u) != 0; });
        }
        if (more) deposit(buf ^ 1, j0 + kScoreTile);            // the other buffer was last read one barrier ago
        __syncthreads();
    }
}

// LDS-operand scan, same arguments plus D (a multiple of 4).  Dynamic LDS: [kScoreRows][D + 1] rows, [kScoreTileG][D + 1]
// items, kScoreRows bitmap words, then the consumer's own words (score_lds_side); score_lds_bytes() sizes it.  State the
// consumer sets up before the call is visible to all waves at the first tile.
template <typename Consumer>
__device__ __forceinline__ void score_scan_lds(const float *__restrict__ U, const float *__restrict__ I, int D, int64_t n_items,
                                               const int64_t *__restrict__ qrows, const int64_t *__restrict__ mrows,
                                               int64_t n, const int64_t *__restrict__ mask_ptr,
                                               const int *__restrict__ mask_idx, int64_t c0, int64_t chunk,
                                               Consumer &&consume) {
    extern __shared__ float lds[];
    const int ldw = D + 1;
    float *ue = lds;                                                    // [kScoreRows][ldw]
    float *it = lds + kScoreRows * ldw;                                 // [kScoreTileG][ldw]
    unsigned *rowmask = reinterpret_cast<unsigned *>(it + kScoreTileG * ldw);   // [kScoreRows]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = lane & 31, half = lane >> 5;
    const int64_t e0 = (int64_t)blockIdx.x * kScoreRows;
    const int64_t c1 = (c0 + chunk < n_items) ? c0 + chunk : n_items;
    for (int idx = threadIdx.x; idx < kScoreRows * D; idx += kBlock) {
        const int r = idx / D, k = idx - r * D;
        const int64_t e = e0 + r;
        ue[r * ldw + k] = (e < n) ? U[(qrows != nullptr ? qrows[e] : e) * (int64_t)D + k] : 0.f;
    }
    MaskCursor cursor(mask_ptr, mask_idx, mrows, e0 + threadIdx.x, n, c0);
    const float *arow = ue + (wave * 32 + col) * ldw + half;            // A[i = lane&31][k = lane>>5]
    const float *brow = it + col * ldw + half;                          // B[k = lane>>5][j = lane&31]
    for (int64_t j0 = c0; j0 < c1; j0 += kScoreTileG) {
        __syncthreads();                                                // previous tile fully consumed (and ue staged)
        for (int idx = threadIdx.x; idx < kScoreTileG * D; idx += kBlock) {
            const int r = idx / D, k = idx - r * D;
            it[r * ldw + k] = (j0 + r < n_items) ? I[(j0 + r) * (int64_t)D + k] : 0.f;
        }
        if (threadIdx.x < kScoreRows) cursor.advance<1>(j0, &rowmask[threadIdx.x]);
        __syncthreads();
        f32x16 acc[1];
        score_tile_lds(arow, brow, D, acc[0]);
        consume(acc, j0, false, [&](int, int row) { return ((rowmask[wave * 32 + row] >> col) & 1u) != 0; });
    }
}

// the consumer's side words of score_scan_lds (16-byte aligned: (160 (D + 1) + 128) * 4 with D a multiple of 4)
__device__ __forceinline__ unsigned *score_lds_side(int D) {
    extern __shared__ float lds[];
    return reinterpret_cast<unsigned *>(lds + (kScoreRows + kScoreTileG) * (D + 1)) + kScoreRows;
}

// ------------------------------------------------------------------------------------------------ host side
constexpr size_t kLdsPerWorkgroup = 160 * 1024;   // gfx950

static inline bool score_rega_d(int32_t D) { return D == 64 || D == 32 || D == 16 || D == 8; }

// dynamic LDS of score_scan_lds with `side_words` words per row (the bitmap word and the consumer's): <= 160 KiB up to D = 252
static inline size_t score_lds_bytes(int32_t D, int side_words) {
    return ((size_t)(kScoreRows + kScoreTileG) * (D + 1) + (size_t)side_words * kScoreRows) * 4;
}

// WR_DISPATCH_KS(D, KS_LO, KS_HI, launch): launch(KS) for the power of two KS in [KS_LO, KS_HI] with D == 2 * KS.  Sizes
// outside the range are not instantiated; the caller has checked D.
#define WR_KS_CASE_(D_, LO_, HI_, KS_, launch_)                                                                        \
    if constexpr ((KS_) >= (LO_) && (KS_) <= (HI_)) {                                                                  \
        if ((D_) == 2 * (KS_)) { launch_(KS_); }                                                                       \
    }
#define WR_DISPATCH_KS(D_, LO_, HI_, launch_)                                                                          \
    do {                                                                                                               \
        WR_KS_CASE_(D_, LO_, HI_, 64, launch_)                                                                         \
        WR_KS_CASE_(D_, LO_, HI_, 32, launch_)                                                                         \
        WR_KS_CASE_(D_, LO_, HI_, 16, launch_)                                                                         \
        WR_KS_CASE_(D_, LO_, HI_, 8, launch_)                                                                          \
        WR_KS_CASE_(D_, LO_, HI_, 4, launch_)                                                                          \
    } while (0)

}  // namespace wr
