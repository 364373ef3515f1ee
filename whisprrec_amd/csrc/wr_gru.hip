// wr_gru.hip — K27: a one-layer GRU over left-aligned, zero-padded histories x [B, T, E] with a length per row, forward and
// backward (whisprrec_amd/gru4rec.py, --gru_native 1).  torch's cell, gate order r, z, n, h_0 = 0:
//   r  = sigmoid(W_ir x + b_ir + W_hr h + b_hr)          z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
//   n  = tanh(W_in x + b_in + r * (W_hn h + b_hn))       h' = (1 - z) * n + z * h
// Row b takes its first len_b = clamp(lengths[b], 0, T) steps; after them its h is frozen, so h_last[b] is the state after step
// len_b - 1 (zeros for len_b = 0).  x[b, t, :] is never read for t >= len_b.
// Supported (gru_supported, the one source of the set): E, H in {32, 64} in any combination, T >= 1.  At H = 128 W_hh alone is
// 196 KB, beyond the 160 KiB of LDS.
//
// Forward, one launch.  A workgroup owns tiles of 16 rows (tiles wg, wg + G, ...) and walks t = 0 .. T - 1.  Both weight
// matrices sit in LDS for the whole launch, row-major with rows of E + 4 / H + 4 words: lane j reading row j as float4 and lane
// k reading column k of one row are both free of bank conflicts, so the forward (a thread owns gate column j) and the backward's
// transposed products (a thread owns input column k) share ONE image: 102 KB at E = H = 64.  Thread (j, g) owns column j of the
// three gates for the rows g RPT .. g RPT + RPT - 1 of the tile (RPT = 4 at H = 64, 2 at H = 32); x_t and h of the tile are
// broadcast reads.  Plain FMAs: fp32 MFMA runs at the vector rate on gfx950 and the operands already come from LDS.  x_{t+1}
// is fetched while step t is computed.  hs != NULL: every h_t goes to hs [B, T, H] (frozen values after len_b) — the only
// activation the backward wants.
//
// Backward, two launches.  The reverse walk t = T - 1 .. 0 over the same tiles recomputes the step's gates from x_t and
// hs[t - 1], forms the four pre-activation gradients [16][4H] in LDS, then dh_{t-1} through W_hh (kept in the registers of the
// thread that owns (row, j)), gx[b, t, :] through W_ih (zeros for t >= len_b, every element written), and adds the step's
// outer products to the workgroup's parameter-gradient accumulators: 3H (E + H) / 256 per thread (96 at E = H = 64) + 2 bias
// sums, in registers across all t and all tiles of the workgroup.  Each workgroup writes its accumulators once to its own slab
// [3H E | 3H H | 3H | 3H] of the workspace; the second launch folds the slabs in workgroup order.  No float atomics; grid, walk
// and fold order depend on (B, T, E, H) alone: same inputs, same bits.
//
// The whole output sequence (wr_gru_seq_fwd / _bwd; NARM's local encoder, the lower layers of a stacked GRU4Rec) is a compile-time
// variant of both kernels, SEQ: the forward's hs is then the result and zero for t >= len_b; the backward adds g_hs[b, t, :] to dh
// before step t's gate gradients (t < len_b only, step t - 1's values fetched while step t computes: RPT registers more).  The
// SEQ = false instantiations hold no trace of it: their instruction streams are the ones from before the variant existed.
#include <math.h>

#include "wr_common.h"

namespace wr {

constexpr int kGruRows = 16;      // rows of a tile
constexpr int kGruFwdWg = 1024;   // forward: workgroups at most (they stride over the tiles)
constexpr int kGruBwdWg = 256;    // backward: slabs of parameter-gradient partials at most

static inline bool gru_supported(int32_t E, int32_t H, int32_t T) { return (E == 32 || E == 64) && (H == 32 || H == 64) && T >= 1; }

template <int E, int H>
struct GruShape {
    static constexpr int LDI = E + 4, LDH = H + 4;          // words per LDS row of W_ih / W_hh
    static constexpr int NG = kBlock / H, RPT = kGruRows / NG;     // gate mapping: thread (j = tid % H, g = tid / H), RPT rows
    static constexpr int NGX = kBlock / E, RPX = kGruRows / NGX;   // gx mapping: thread (k = tid % E, g = tid / E), RPX rows
    static constexpr int XV = kGruRows * E / 4, HV = kGruRows * H / 4;   // float4 of a tile's x_t / h_t
    static constexpr int CI = 3 * H * E / kBlock, CH = 3 * H * H / kBlock;   // accumulators per thread for g_w_ih / g_w_hh
    static constexpr int W_WORDS = 3 * H * LDI + 3 * H * LDH;
    static constexpr int SLAB = 3 * H * E + 3 * H * H + 6 * H;
};

static inline int64_t gru_slab_words(int E, int H) { return (int64_t)3 * H * E + 3 * H * H + 6 * H; }      // GruShape::SLAB
// dynamic LDS: the two weight images, x_t and h of a tile, its 16 lengths and, backward, the gate gradients [16][4H]
static inline int64_t gru_lds_bytes(int E, int H, bool bwd) {
    return (int64_t)4 * (3 * H * (E + 4) + 3 * H * (H + 4) + kGruRows * E + kGruRows * H + kGruRows + (bwd ? kGruRows * 4 * H : 0));
}

struct GruParams {
    const float *x, *w_ih, *w_hh, *b_ih, *b_hh;
    const int64_t *lengths;
    int64_t B;
    int T;
};

__device__ __forceinline__ float gru_sigmoid(float a) { return 1.0f / (1.0f + expf(-a)); }

// both weight matrices -> LDS rows of LDI / LDH words
template <int E, int H>
__device__ __forceinline__ void gru_load_weights(const GruParams &P, float *Wi, float *Wh) {
    using S = GruShape<E, H>;
    for (int idx = threadIdx.x; idx < 3 * H * E / 4; idx += kBlock) {
        const int row = idx / (E / 4), c = idx - row * (E / 4);
        *reinterpret_cast<float4 *>(Wi + row * S::LDI + 4 * c) = reinterpret_cast<const float4 *>(P.w_ih)[idx];
    }
    for (int idx = threadIdx.x; idx < 3 * H * H / 4; idx += kBlock) {
        const int row = idx / (H / 4), c = idx - row * (H / 4);
        *reinterpret_cast<float4 *>(Wh + row * S::LDH + 4 * c) = reinterpret_cast<const float4 *>(P.w_hh)[idx];
    }
}

// the tile's clamped lengths -> len_s, rows past B as length 0; returns the tile's largest (after a barrier)
__device__ __forceinline__ int gru_tile_lengths(const GruParams &P, int64_t b0, int *len_s) {
    if (threadIdx.x < kGruRows) {
        const int64_t b = b0 + threadIdx.x;
        int64_t l = b < P.B ? P.lengths[b] : 0;
        l = l < 0 ? 0 : (l > P.T ? P.T : l);
        len_s[threadIdx.x] = (int)l;
    }
    __syncthreads();
    int m = 0;
#pragma unroll
    for (int r = 0; r < kGruRows; ++r) m = max(m, len_s[r]);
    return m;
}

// The pre-activations of gate column j for the thread's RPT rows: ar / az start at the sums of both biases, ain at b_in, ahn at
// b_hn; the input part is added first (k ascending), then the hidden part.
template <int E, int H>
__device__ __forceinline__ void gru_gate_sums(const float *Wi, const float *Wh, const float *xs, const float *hh, int j, int row0,
                                              float (&ar)[GruShape<E, H>::RPT], float (&az)[GruShape<E, H>::RPT],
                                              float (&ain)[GruShape<E, H>::RPT], float (&ahn)[GruShape<E, H>::RPT]) {
    using S = GruShape<E, H>;
#pragma unroll 4
    for (int k4 = 0; k4 < E / 4; ++k4) {
        const float4 wr_ = *reinterpret_cast<const float4 *>(Wi + j * S::LDI + 4 * k4);
        const float4 wz = *reinterpret_cast<const float4 *>(Wi + (H + j) * S::LDI + 4 * k4);
        const float4 wn = *reinterpret_cast<const float4 *>(Wi + (2 * H + j) * S::LDI + 4 * k4);
#pragma unroll
        for (int i = 0; i < S::RPT; ++i) {
            const float4 v = *reinterpret_cast<const float4 *>(xs + (row0 + i) * E + 4 * k4);
            ar[i] = fmaf(wr_.w, v.w, fmaf(wr_.z, v.z, fmaf(wr_.y, v.y, fmaf(wr_.x, v.x, ar[i]))));
            az[i] = fmaf(wz.w, v.w, fmaf(wz.z, v.z, fmaf(wz.y, v.y, fmaf(wz.x, v.x, az[i]))));
            ain[i] = fmaf(wn.w, v.w, fmaf(wn.z, v.z, fmaf(wn.y, v.y, fmaf(wn.x, v.x, ain[i]))));
        }
    }
#pragma unroll 4
    for (int k4 = 0; k4 < H / 4; ++k4) {
        const float4 wr_ = *reinterpret_cast<const float4 *>(Wh + j * S::LDH + 4 * k4);
        const float4 wz = *reinterpret_cast<const float4 *>(Wh + (H + j) * S::LDH + 4 * k4);
        const float4 wn = *reinterpret_cast<const float4 *>(Wh + (2 * H + j) * S::LDH + 4 * k4);
#pragma unroll
        for (int i = 0; i < S::RPT; ++i) {
            const float4 v = *reinterpret_cast<const float4 *>(hh + (row0 + i) * H + 4 * k4);
            ar[i] = fmaf(wr_.w, v.w, fmaf(wr_.z, v.z, fmaf(wr_.y, v.y, fmaf(wr_.x, v.x, ar[i]))));
            az[i] = fmaf(wz.w, v.w, fmaf(wz.z, v.z, fmaf(wz.y, v.y, fmaf(wz.x, v.x, az[i]))));
            ahn[i] = fmaf(wn.w, v.w, fmaf(wn.z, v.z, fmaf(wn.y, v.y, fmaf(wn.x, v.x, ahn[i]))));
        }
    }
}

// SEQ (wr_gru_seq_fwd): hs is the result, zero for t >= len_b (pad_packed_sequence's form), and h_last is not written.
template <int E, int H, bool SEQ = false>
__global__ __launch_bounds__(kBlock) void gru_fwd_kernel(GruParams P, float *__restrict__ h_last, float *__restrict__ hs) {
    using S = GruShape<E, H>;
    extern __shared__ float4 gru_lds4[];
    float *Wi = reinterpret_cast<float *>(gru_lds4), *Wh = Wi + 3 * H * S::LDI, *xs = Wi + S::W_WORDS, *hh = xs + kGruRows * E;
    int *len_s = reinterpret_cast<int *>(hh + kGruRows * H);
    const int tid = threadIdx.x, j = tid % H, row0 = (tid / H) * S::RPT, T = P.T;
    gru_load_weights<E, H>(P, Wi, Wh);
    const float br = P.b_ih[j] + P.b_hh[j], bz = P.b_ih[H + j] + P.b_hh[H + j], bin = P.b_ih[2 * H + j], bhn = P.b_hh[2 * H + j];
    const int xrow = tid / (E / 4), xc = tid - xrow * (E / 4);      // this thread's float4 of a tile's x_t (tid < XV)
    const int64_t n_tiles = (P.B + kGruRows - 1) / kGruRows;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * kGruRows;
        __syncthreads();      // the weights are in place; the last tile's readers are done
        const int maxlen = gru_tile_lengths(P, b0, len_s);
        for (int idx = tid; idx < kGruRows * H; idx += kBlock) hh[idx] = 0.f;
        int lr[S::RPT];
        float hreg[S::RPT];
#pragma unroll
        for (int i = 0; i < S::RPT; ++i) {
            lr[i] = len_s[row0 + i];
            hreg[i] = 0.f;
        }
        const int xlen = tid < S::XV ? len_s[xrow] : 0;
        const float4 *xp = reinterpret_cast<const float4 *>(P.x + (b0 + xrow) * (int64_t)T * E) + xc;      // + t E / 4
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 xn = zero4;
        if (0 < xlen) xn = xp[0];
        for (int t = 0; t < T; ++t) {
            if (t < maxlen) {      // the same for the whole workgroup
                if (tid < S::XV) *reinterpret_cast<float4 *>(xs + xrow * E + 4 * xc) = xn;
                __syncthreads();      // x_t and h_{t-1} are in LDS
                xn = zero4;      // (an if, not a ?: between a load and a constant: that form puts the constant on the stack)
                if (t + 1 < xlen) xn = xp[(int64_t)(t + 1) * (E / 4)];
                float ar[S::RPT], az[S::RPT], ain[S::RPT], ahn[S::RPT];
#pragma unroll
                for (int i = 0; i < S::RPT; ++i) {
                    ar[i] = br;
                    az[i] = bz;
                    ain[i] = bin;
                    ahn[i] = bhn;
                }
                gru_gate_sums<E, H>(Wi, Wh, xs, hh, j, row0, ar, az, ain, ahn);
#pragma unroll
                for (int i = 0; i < S::RPT; ++i) {
                    const float r = gru_sigmoid(ar[i]), z = gru_sigmoid(az[i]);
                    const float n = tanhf(fmaf(r, ahn[i], ain[i]));
                    const float hn = fmaf(z, hreg[i], (1.0f - z) * n);
                    if (t < lr[i]) hreg[i] = hn;
                }
                __syncthreads();      // every read of h_{t-1} is done
#pragma unroll
                for (int i = 0; i < S::RPT; ++i) hh[(row0 + i) * H + j] = hreg[i];
            }
            if constexpr (SEQ) {
#pragma unroll
                for (int i = 0; i < S::RPT; ++i)
                    if (b0 + row0 + i < P.B) hs[((b0 + row0 + i) * T + t) * H + j] = t < lr[i] ? hreg[i] : 0.f;
            } else if (hs != nullptr) {
#pragma unroll
                for (int i = 0; i < S::RPT; ++i)
                    if (b0 + row0 + i < P.B) hs[((b0 + row0 + i) * T + t) * H + j] = hreg[i];
            }
        }
        if constexpr (!SEQ) {
#pragma unroll
            for (int i = 0; i < S::RPT; ++i)
                if (b0 + row0 + i < P.B) h_last[(b0 + row0 + i) * H + j] = hreg[i];
        }
    }
}

// SEQ (wr_gru_seq_bwd): a gradient enters at every step: g_hs[b, t, j] is added to dh before step t's gate gradients, for
// t < len_b only (the padding of g_hs is never read); step t - 1's values are fetched while step t computes.  g_last may be NULL.
// hs is then wr_gru_seq_fwd's (zero past the length): the walk reads hs[b, t - 1] for t < len_b alone, so either form serves.
// g_hs is the last argument, unused and NULL without SEQ: the arguments before it sit where they always did.  (A shared
// __device__ body behind two __global__ entries was tried: the compiler then schedules the SEQ = false kernels differently.)
template <int E, int H, bool SEQ = false>
__global__ __launch_bounds__(kBlock) void gru_bwd_kernel(GruParams P, const float *__restrict__ hs, const float *__restrict__ g_last,
                                                         float *__restrict__ gx, float *__restrict__ slabs,
                                                         const float *__restrict__ g_hs) {
    using S = GruShape<E, H>;
    extern __shared__ float4 gru_lds4[];
    float *Wi = reinterpret_cast<float *>(gru_lds4), *Wh = Wi + 3 * H * S::LDI, *xs = Wi + S::W_WORDS, *hp = xs + kGruRows * E;
    int *len_s = reinterpret_cast<int *>(hp + kGruRows * H);
    float *dG = reinterpret_cast<float *>(len_s + kGruRows);      // [16][4H]: d ar | d az | d ain | d ahn
    const int tid = threadIdx.x, j = tid % H, row0 = (tid / H) * S::RPT, T = P.T;
    const int kx = tid % E, rowx0 = (tid / E) * S::RPX;                  // gx: column kx of RPX rows
    const int ci0 = (tid / E) * S::CI, ch0 = (tid / H) * S::CH;          // first gate row of this thread's accumulators
    gru_load_weights<E, H>(P, Wi, Wh);
    const float br = P.b_ih[j] + P.b_hh[j], bz = P.b_ih[H + j] + P.b_hh[H + j], bin = P.b_ih[2 * H + j], bhn = P.b_hh[2 * H + j];
    const int xrow = tid / (E / 4), xc = tid - xrow * (E / 4);      // this thread's float4 of a tile's x_t (tid < XV)
    const int hrow = tid / (H / 4), hc = tid - hrow * (H / 4);      // ... and of its h_{t-1} (tid < HV)
    float acc_i[S::CI], acc_h[S::CH], accb_i = 0.f, accb_h = 0.f;
#pragma unroll
    for (int c = 0; c < S::CI; ++c) acc_i[c] = 0.f;
#pragma unroll
    for (int c = 0; c < S::CH; ++c) acc_h[c] = 0.f;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t n_tiles = (P.B + kGruRows - 1) / kGruRows;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * kGruRows;
        __syncthreads();      // the weights are in place; the last tile's readers are done
        const int maxlen = gru_tile_lengths(P, b0, len_s);
        int lr[S::RPT], lx[S::RPX];
        float dh[S::RPT];
#pragma unroll
        for (int i = 0; i < S::RPT; ++i) {
            lr[i] = len_s[row0 + i];
            if constexpr (SEQ) {
                dh[i] = 0.f;
                if (g_last != nullptr && b0 + row0 + i < P.B) dh[i] = g_last[(b0 + row0 + i) * H + j];
            } else {
                dh[i] = b0 + row0 + i < P.B ? g_last[(b0 + row0 + i) * H + j] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < S::RPX; ++i) lx[i] = len_s[rowx0 + i];
        const int xlen = tid < S::XV ? len_s[xrow] : 0, hlen = tid < S::HV ? len_s[hrow] : 0;
        const float4 *xp = reinterpret_cast<const float4 *>(P.x + (b0 + xrow) * (int64_t)T * E) + xc;      // + t E / 4
        const float4 *hsp = reinterpret_cast<const float4 *>(hs + (b0 + hrow) * (int64_t)T * H) + hc;      // + t H / 4
        float4 *gxz = reinterpret_cast<float4 *>(gx + (b0 + xrow) * (int64_t)T * E) + xc;
        for (int t = T - 1; t >= maxlen; --t)      // steps no row of the tile takes
            if (tid < S::XV && b0 + xrow < P.B) gxz[(int64_t)t * (E / 4)] = zero4;
        float4 xn = zero4, hn = zero4;
        if (maxlen > 0) {
            const int t = maxlen - 1;
            if (t < xlen) xn = xp[(int64_t)t * (E / 4)];
            if (t < hlen && t > 0) hn = hsp[(int64_t)(t - 1) * (H / 4)];
        }
        float gn[SEQ ? S::RPT : 1];      // SEQ: g_hs[row][t][j] of the step about to run (rows past their length: 0, unread)
        const float *ghp = nullptr;
        (void)gn;
        (void)ghp;
        if constexpr (SEQ) {
            ghp = g_hs + ((b0 + row0) * (int64_t)T) * H + j;      // + (i T + t) H
#pragma unroll
            for (int i = 0; i < S::RPT; ++i) {
                gn[i] = 0.f;
                if (maxlen > 0 && maxlen - 1 < lr[i]) gn[i] = ghp[((int64_t)i * T + (maxlen - 1)) * H];      // maxlen = 0: no step
            }
        }
        for (int t = maxlen - 1; t >= 0; --t) {
            if (tid < S::XV) *reinterpret_cast<float4 *>(xs + xrow * E + 4 * xc) = xn;
            if (tid < S::HV) *reinterpret_cast<float4 *>(hp + hrow * H + 4 * hc) = hn;
            __syncthreads();      // x_t and h_{t-1} are in LDS (zeros for the rows past their length)
            xn = zero4;
            hn = zero4;
            if (t >= 1 && t - 1 < xlen) xn = xp[(int64_t)(t - 1) * (E / 4)];
            if (t >= 2 && t - 1 < hlen) hn = hsp[(int64_t)(t - 2) * (H / 4)];
            if constexpr (SEQ) {
#pragma unroll
                for (int i = 0; i < S::RPT; ++i) {
                    if (t < lr[i]) dh[i] += gn[i];
                    gn[i] = 0.f;
                    if (t >= 1 && t - 1 < lr[i]) gn[i] = ghp[((int64_t)i * T + (t - 1)) * H];
                }
            }
            {      // the step's gates again, and the four pre-activation gradients
                float ar[S::RPT], az[S::RPT], ain[S::RPT], ahn[S::RPT];
#pragma unroll
                for (int i = 0; i < S::RPT; ++i) {
                    ar[i] = br;
                    az[i] = bz;
                    ain[i] = bin;
                    ahn[i] = bhn;
                }
                gru_gate_sums<E, H>(Wi, Wh, xs, hp, j, row0, ar, az, ain, ahn);
#pragma unroll
                for (int i = 0; i < S::RPT; ++i) {
                    float d_ar = 0.f, d_az = 0.f, d_ain = 0.f, d_ahn = 0.f;
                    if (t < lr[i]) {
                        const float r = gru_sigmoid(ar[i]), z = gru_sigmoid(az[i]);
                        const float n = tanhf(fmaf(r, ahn[i], ain[i]));
                        const float hprev = hp[(row0 + i) * H + j];
                        d_ain = dh[i] * (1.0f - z) * (1.0f - n * n);
                        d_ahn = d_ain * r;
                        d_ar = d_ain * ahn[i] * r * (1.0f - r);
                        d_az = dh[i] * (hprev - n) * z * (1.0f - z);
                        dh[i] = dh[i] * z;      // the direct path; the path through the gates is added below
                    }
                    float *d = dG + (row0 + i) * 4 * H + j;
                    d[0] = d_ar;
                    d[H] = d_az;
                    d[2 * H] = d_ain;
                    d[3 * H] = d_ahn;
                }
            }
            __syncthreads();      // dG is complete
            // dh_{t-1}[row][j] += sum_q d ar[row][q] W_hr[q][j] + d az[row][q] W_hz[q][j] + d ahn[row][q] W_hn[q][j]
#pragma unroll
            for (int gate = 0; gate < 3; ++gate) {
                const float *w = Wh + gate * H * S::LDH + j;
                const float *d = dG + row0 * 4 * H + (gate == 2 ? 3 : gate) * H;
#pragma unroll 4
                for (int q4 = 0; q4 < H / 4; ++q4) {
                    const float w0 = w[(4 * q4) * S::LDH], w1 = w[(4 * q4 + 1) * S::LDH], w2 = w[(4 * q4 + 2) * S::LDH],
                                w3 = w[(4 * q4 + 3) * S::LDH];
#pragma unroll
                    for (int i = 0; i < S::RPT; ++i) {
                        const float4 v = *reinterpret_cast<const float4 *>(d + i * 4 * H + 4 * q4);
                        dh[i] = fmaf(v.w, w3, fmaf(v.z, w2, fmaf(v.y, w1, fmaf(v.x, w0, dh[i]))));
                    }
                }
            }
            // gx[row][k] = sum_q d ar[row][q] W_ir[q][k] + d az[row][q] W_iz[q][k] + d ain[row][q] W_in[q][k]
            {
                float g[S::RPX];
#pragma unroll
                for (int i = 0; i < S::RPX; ++i) g[i] = 0.f;
#pragma unroll
                for (int gate = 0; gate < 3; ++gate) {
                    const float *w = Wi + gate * H * S::LDI + kx;
                    const float *d = dG + rowx0 * 4 * H + gate * H;
#pragma unroll 4
                    for (int q4 = 0; q4 < H / 4; ++q4) {
                        const float w0 = w[(4 * q4) * S::LDI], w1 = w[(4 * q4 + 1) * S::LDI], w2 = w[(4 * q4 + 2) * S::LDI],
                                    w3 = w[(4 * q4 + 3) * S::LDI];
#pragma unroll
                        for (int i = 0; i < S::RPX; ++i) {
                            const float4 v = *reinterpret_cast<const float4 *>(d + i * 4 * H + 4 * q4);
                            g[i] = fmaf(v.w, w3, fmaf(v.z, w2, fmaf(v.y, w1, fmaf(v.x, w0, g[i]))));
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < S::RPX; ++i)
                    if (b0 + rowx0 + i < P.B) gx[((b0 + rowx0 + i) * T + t) * E + kx] = t < lx[i] ? g[i] : 0.f;
            }
            // the step's outer products, rows in ascending order (the rows past their length add exact zeros)
#pragma unroll 2
            for (int r = 0; r < kGruRows; ++r) {
                const float xv = xs[r * E + kx], hv = hp[r * H + j];
                const float *d = dG + r * 4 * H;
#pragma unroll
                for (int c = 0; c < S::CI / 4; ++c) {
                    const float4 v = *reinterpret_cast<const float4 *>(d + ci0 + 4 * c);
                    acc_i[4 * c] = fmaf(v.x, xv, acc_i[4 * c]);
                    acc_i[4 * c + 1] = fmaf(v.y, xv, acc_i[4 * c + 1]);
                    acc_i[4 * c + 2] = fmaf(v.z, xv, acc_i[4 * c + 2]);
                    acc_i[4 * c + 3] = fmaf(v.w, xv, acc_i[4 * c + 3]);
                }
#pragma unroll
                for (int c = 0; c < S::CH / 4; ++c) {
                    const int q = ch0 + 4 * c;      // gate row of W_hh; its n rows read d ahn
                    const float4 v = *reinterpret_cast<const float4 *>(d + (q < 2 * H ? q : q + H));
                    acc_h[4 * c] = fmaf(v.x, hv, acc_h[4 * c]);
                    acc_h[4 * c + 1] = fmaf(v.y, hv, acc_h[4 * c + 1]);
                    acc_h[4 * c + 2] = fmaf(v.z, hv, acc_h[4 * c + 2]);
                    acc_h[4 * c + 3] = fmaf(v.w, hv, acc_h[4 * c + 3]);
                }
                if (tid < 3 * H) {
                    accb_i += d[tid];
                    accb_h += d[tid < 2 * H ? tid : tid + H];
                }
            }
            __syncthreads();      // every read of x_t, h_{t-1} and dG is done
        }
    }
    // this workgroup's slab: [3H][E] | [3H][H] | [3H] | [3H]
    float *slab = slabs + (int64_t)blockIdx.x * S::SLAB;
#pragma unroll
    for (int c = 0; c < S::CI; ++c) slab[(ci0 + c) * E + kx] = acc_i[c];
#pragma unroll
    for (int c = 0; c < S::CH; ++c) slab[3 * H * E + (ch0 + c) * H + j] = acc_h[c];
    if (tid < 3 * H) {
        slab[3 * H * E + 3 * H * H + tid] = accb_i;
        slab[3 * H * E + 3 * H * H + 3 * H + tid] = accb_h;
    }
}

// element e of [g_w_ih | g_w_hh | g_b_ih | g_b_hh]: the slabs summed in workgroup order, eight loads in flight
__global__ __launch_bounds__(kBlock) void gru_fold_kernel(const float *__restrict__ slabs, int n_slabs, int n_wi, int n_wh, int n_b,
                                                           float *__restrict__ g_w_ih, float *__restrict__ g_w_hh,
                                                           float *__restrict__ g_b_ih, float *__restrict__ g_b_hh) {
    const int total = n_wi + n_wh + 2 * n_b;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    float v = 0.f;
    int w = 0;
    for (; w + 8 <= n_slabs; w += 8) {
        float p[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u] = slabs[(int64_t)(w + u) * total + e];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += p[u];
    }
    for (; w < n_slabs; ++w) v += slabs[(int64_t)w * total + e];
    if (e < n_wi) g_w_ih[e] = v;
    else if (e < n_wi + n_wh) g_w_hh[e - n_wi] = v;
    else if (e < n_wi + n_wh + n_b) g_b_ih[e - n_wi - n_wh] = v;
    else g_b_hh[e - n_wi - n_wh - n_b] = v;
}

static int32_t gru_check(const char *entry, const float *x, const int64_t *lengths, const float *w_ih, const float *w_hh,
                         const float *b_ih, const float *b_hh, int64_t B, int32_t T, int32_t E, int32_t H) {
    WR_REQUIRE(gru_supported(E, H, T), WR_E_RANGE, "%s supports E in {32, 64}, H in {32, 64}, T >= 1; got E=%d H=%d T=%d", entry, E,
               H, T);
    WR_REQUIRE(x && lengths && w_ih && w_hh && b_ih && b_hh, WR_E_NULL, "%s: NULL argument", entry);
    WR_REQUIRE(B >= 1 && B <= (int64_t(1) << 24), WR_E_SHAPE, "%s: B=%lld out of range (1..2^24)", entry, (long long)B);
    WR_REQUIRE(aligned16(x) && aligned16(w_ih) && aligned16(w_hh), WR_E_ALIGN, "%s: x, w_ih and w_hh must be 16-byte aligned", entry);
    return WR_OK;
}

#define WR_GRU_DISPATCH(E, H, CALL)                   \
    do {                                              \
        if ((E) == 64 && (H) == 64) { CALL(64, 64); } \
        else if ((E) == 64) { CALL(64, 32); }         \
        else if ((H) == 64) { CALL(32, 64); }         \
        else { CALL(32, 32); }                        \
    } while (0)

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_gru_supported(int32_t E, int32_t H, int32_t T) { return gru_supported(E, H, T) ? 1 : 0; }

int64_t wr_gru_workspace_bytes(int64_t B, int32_t T, int32_t E, int32_t H) {
    WR_REQUIRE(gru_supported(E, H, T) && B >= 1 && B <= (int64_t(1) << 24), WR_E_RANGE,
               "wr_gru_workspace_bytes supports E in {32, 64}, H in {32, 64}, T >= 1, 1 <= B <= 2^24; got B=%lld T=%d E=%d H=%d",
               (long long)B, T, E, H);
    return align_up((int64_t)kGruBwdWg * gru_slab_words(E, H) * 4, 256);      // sized by the bound, not by the tiles of B
}

int32_t wr_gru_fwd(const float *x, const int64_t *lengths, const float *w_ih, const float *w_hh, const float *b_ih,
                   const float *b_hh, int64_t B, int32_t T, int32_t E, int32_t H, float *h_last, float *hs, void *stream_) {
    const char *entry = "wr_gru_fwd";
    const int32_t rc = gru_check(entry, x, lengths, w_ih, w_hh, b_ih, b_hh, B, T, E, H);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(h_last != nullptr, WR_E_NULL, "%s: NULL argument", entry);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const GruParams P{x, w_ih, w_hh, b_ih, b_hh, lengths, B, T};
    const size_t lds = (size_t)gru_lds_bytes(E, H, false);
    const int64_t n_tiles = (B + kGruRows - 1) / kGruRows;
    const unsigned grid = (unsigned)(n_tiles < kGruFwdWg ? n_tiles : kGruFwdWg);
#define WR_GRU_FWD(E_, H_)                                                                                                         \
    do {                                                                                                                           \
        if (lds > 64 * 1024)                                                                                                       \
            WR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(gru_fwd_kernel<E_, H_>),                                     \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                     \
        hipLaunchKernelGGL((gru_fwd_kernel<E_, H_>), dim3(grid), dim3(kBlock), lds, stream, P, h_last, hs);                        \
    } while (0)
    WR_GRU_DISPATCH(E, H, WR_GRU_FWD);
#undef WR_GRU_FWD
    WR_LAUNCH_CHECK("gru_fwd_kernel");
    return WR_OK;
}

int32_t wr_gru_bwd(const float *x, const int64_t *lengths, const float *w_ih, const float *w_hh, const float *b_ih,
                   const float *b_hh, const float *hs, const float *g_last, int64_t B, int32_t T, int32_t E, int32_t H, float *gx,
                   float *g_w_ih, float *g_w_hh, float *g_b_ih, float *g_b_hh, void *workspace, int64_t workspace_bytes,
                   void *stream_) {
    const char *entry = "wr_gru_bwd";
    int32_t rc = gru_check(entry, x, lengths, w_ih, w_hh, b_ih, b_hh, B, T, E, H);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(hs && g_last && gx && g_w_ih && g_w_hh && g_b_ih && g_b_hh, WR_E_NULL, "%s: NULL argument", entry);
    WR_REQUIRE(aligned16(hs) && aligned16(gx), WR_E_ALIGN, "%s: hs and gx must be 16-byte aligned", entry);
    if ((rc = check_workspace(entry, workspace, workspace_bytes, wr_gru_workspace_bytes(B, T, E, H))) != WR_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const GruParams P{x, w_ih, w_hh, b_ih, b_hh, lengths, B, T};
    const size_t lds = (size_t)gru_lds_bytes(E, H, true);
    float *slabs = reinterpret_cast<float *>(workspace);
    const int64_t n_tiles = (B + kGruRows - 1) / kGruRows;
    const int n_wg = (int)(n_tiles < kGruBwdWg ? n_tiles : kGruBwdWg);
#define WR_GRU_BWD(E_, H_)                                                                                                         \
    do {                                                                                                                           \
        if (lds > 64 * 1024)                                                                                                       \
            WR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(gru_bwd_kernel<E_, H_>),                                     \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                     \
        hipLaunchKernelGGL((gru_bwd_kernel<E_, H_>), dim3(n_wg), dim3(kBlock), lds, stream, P, hs, g_last, gx, slabs,              \
                           (const float *)nullptr);                                                                                \
    } while (0)
    WR_GRU_DISPATCH(E, H, WR_GRU_BWD);
#undef WR_GRU_BWD
    WR_LAUNCH_CHECK("gru_bwd_kernel");
    const int n_wi = 3 * H * E, n_wh = 3 * H * H, n_b = 3 * H, total = n_wi + n_wh + 2 * n_b;
    hipLaunchKernelGGL(gru_fold_kernel, dim3((total + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, slabs, n_wg, n_wi, n_wh, n_b,
                       g_w_ih, g_w_hh, g_b_ih, g_b_hh);
    WR_LAUNCH_CHECK("gru_fold_kernel");
    return WR_OK;
}

int32_t wr_gru_seq_fwd(const float *x, const int64_t *lengths, const float *w_ih, const float *w_hh, const float *b_ih,
                       const float *b_hh, int64_t B, int32_t T, int32_t E, int32_t H, float *hs, void *stream_) {
    const char *entry = "wr_gru_seq_fwd";
    const int32_t rc = gru_check(entry, x, lengths, w_ih, w_hh, b_ih, b_hh, B, T, E, H);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(hs != nullptr, WR_E_NULL, "%s: NULL argument", entry);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const GruParams P{x, w_ih, w_hh, b_ih, b_hh, lengths, B, T};
    const size_t lds = (size_t)gru_lds_bytes(E, H, false);
    const int64_t n_tiles = (B + kGruRows - 1) / kGruRows;
    const unsigned grid = (unsigned)(n_tiles < kGruFwdWg ? n_tiles : kGruFwdWg);
#define WR_GRU_SEQ_FWD(E_, H_)                                                                                                     \
    do {                                                                                                                           \
        if (lds > 64 * 1024)                                                                                                       \
            WR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(gru_fwd_kernel<E_, H_, true>),                               \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                     \
        hipLaunchKernelGGL((gru_fwd_kernel<E_, H_, true>), dim3(grid), dim3(kBlock), lds, stream, P, (float *)nullptr, hs);        \
    } while (0)
    WR_GRU_DISPATCH(E, H, WR_GRU_SEQ_FWD);
#undef WR_GRU_SEQ_FWD
    WR_LAUNCH_CHECK("gru_fwd_kernel (seq)");
    return WR_OK;
}

int32_t wr_gru_seq_bwd(const float *x, const int64_t *lengths, const float *w_ih, const float *w_hh, const float *b_ih,
                       const float *b_hh, const float *hs, const float *g_hs, const float *g_last, int64_t B, int32_t T, int32_t E,
                       int32_t H, float *gx, float *g_w_ih, float *g_w_hh, float *g_b_ih, float *g_b_hh, void *workspace,
                       int64_t workspace_bytes, void *stream_) {
    const char *entry = "wr_gru_seq_bwd";
    int32_t rc = gru_check(entry, x, lengths, w_ih, w_hh, b_ih, b_hh, B, T, E, H);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(hs && g_hs && gx && g_w_ih && g_w_hh && g_b_ih && g_b_hh, WR_E_NULL, "%s: NULL argument", entry);      // g_last may be
    WR_REQUIRE(aligned16(hs) && aligned16(gx), WR_E_ALIGN, "%s: hs and gx must be 16-byte aligned", entry);
    if ((rc = check_workspace(entry, workspace, workspace_bytes, wr_gru_workspace_bytes(B, T, E, H))) != WR_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const GruParams P{x, w_ih, w_hh, b_ih, b_hh, lengths, B, T};
    const size_t lds = (size_t)gru_lds_bytes(E, H, true);
    float *slabs = reinterpret_cast<float *>(workspace);
    const int64_t n_tiles = (B + kGruRows - 1) / kGruRows;
    const int n_wg = (int)(n_tiles < kGruBwdWg ? n_tiles : kGruBwdWg);
#define WR_GRU_SEQ_BWD(E_, H_)                                                                                                     \
    do {                                                                                                                           \
        if (lds > 64 * 1024)                                                                                                       \
            WR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(gru_bwd_kernel<E_, H_, true>),                               \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                     \
        hipLaunchKernelGGL((gru_bwd_kernel<E_, H_, true>), dim3(n_wg), dim3(kBlock), lds, stream, P, hs, g_last, gx, slabs, g_hs); \
    } while (0)
    WR_GRU_DISPATCH(E, H, WR_GRU_SEQ_BWD);
#undef WR_GRU_SEQ_BWD
    WR_LAUNCH_CHECK("gru_bwd_kernel (seq)");
    const int n_wi = 3 * H * E, n_wh = 3 * H * H, n_b = 3 * H, total = n_wi + n_wh + 2 * n_b;
    hipLaunchKernelGGL(gru_fold_kernel, dim3((total + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, slabs, n_wg, n_wi, n_wh, n_b,
                       g_w_ih, g_w_hh, g_b_ih, g_b_hh);
    WR_LAUNCH_CHECK("gru_fold_kernel");
    return WR_OK;
}

}  // extern "C"
