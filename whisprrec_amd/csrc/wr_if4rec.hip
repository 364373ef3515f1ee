// wr_if4rec.hip — K18: IF4Rec's interest pooling (reference src/models/sequential/IF4Rec.py:87-103), forward and backward,
// without the [B, T, D] gather and the [B, K, T, D] product in global memory.
//
// For sequence b with history ids h[t] (t < T), item table E, position table P (NULL: add_pos 0), W1 [A, D], b1 [A], W2 [K, A],
// b2 [K]:
//   valid[t] = h[t] > 0                                   hp[t] = E[h[t]] + P[t]          (position t for a valid entry, :91)
//   s[k][t]  = b2[k] + <W2[k], leaky_relu(W1 hp[t] + b1)>  for valid t, -inf otherwise   (:97-98)
//   p[k][.]  = softmax over t of s[k][.], an all-masked row -> 0                          (:100-101)
//   out[k]   = sum_t p[k][t] hp[t]                                                        (:102)
// Supported (ip_supported, the one source of the set): D in {32, 64, 128}, 1 <= A <= 32, 1 <= K <= 8, 1 <= T <= 64.
//
// One workgroup works on one sequence at a time: its valid rows are gathered ONCE into LDS in the [T][D + 1] layout of the block
// kernels (wr_sasblock.hip; conflict-free column reads), padded positions are not gathered (their rows are zeros with weight
// zero), and hidden layer, scores, softmax and the K weighted sums are computed from there.
//
// The global maximum.  The reference subtracts the maximum over the WHOLE call before softmax (:100).  Softmax is invariant
// under a shift, and torch's softmax subtracts each row's own maximum again, so the reference computes
// exp((s - g) - (m_row - g)): the shift changes nothing but the rounding of s - g (an absolute error of one ulp of |s - g| in
// the exponent) and can neither cause nor cure an underflow.  This kernel uses each (b, k) row's own maximum, exp(s - m_row):
// no second launch, no fold across workgroups.  The tolerance of the tests is measured on the stock path, which does the
// global shift, on cases with a large score spread.
//
// Backward.  The forward of a sequence is recomputed from the ids; nothing is saved.  g_hp [B, T, D] is the gradient w.r.t.
// item row + position row (exactly 0 at masked positions).  Parameter gradients (W1, b1, W2, b2, the position rows 0..T-1) are
// accumulated per workgroup in registers over its sequences b = wg, wg + G, ... (G = min(B, kIpBwdWg)), written as one row of
// partials per workgroup and folded in workgroup order by a second launch (the scheme of sas_bwd_kernel / sas_fold_kernel): no
// float atomics, every sum has a fixed order, same inputs -> same bits on any device.  The path through the maximum is
// ignored (its derivative is zero), and a row zeroed by the NaN rule passes no gradient where autograd would pass NaN: the
// deviation K13 documents for its own NaN rule.
//
// An id outside [0, n_items) is clamped before it addresses anything and ORs 1 into err_word; no host round trip.
#include "wr_common.h"

namespace wr {

constexpr int kIpMaxT = 64, kIpMaxA = 32, kIpMaxK = 8;
constexpr int kIpFwdWg = 4096;   // forward: workgroups at most (they stride over the sequences)
constexpr int kIpBwdWg = 512;    // backward: rows of partials at most
constexpr float kIpLeaky = 0.01f;   // F.leaky_relu's default slope

static inline bool ip_supported(int32_t D, int32_t A, int32_t K, int32_t T) {
    return (D == 32 || D == 64 || D == 128) && A >= 1 && A <= kIpMaxA && K >= 1 && K <= kIpMaxK && T >= 1 && T <= kIpMaxT;
}

// floats of one row of partials: gW1 | gb1 | gW2 | gb2 | position rows 0..T-1
static inline int64_t ip_main_params(int32_t D, int32_t A, int32_t K) { return (int64_t)A * D + A + (int64_t)K * A + K; }
static inline int64_t ip_partial_floats(int32_t D, int32_t A, int32_t K, int32_t T) { return ip_main_params(D, A, K) + (int64_t)T * D; }

struct IpLds {
    float *hp, *w1, *hs, *sc, *w2, *b1, *b2, *gi, *ds, *dh;
    int *ids;
};

// dynamic LDS: hp [T][D+1], w1 [A][D+1], hs [T][A+1], sc [K][64], w2 [K][A], b1 [A], b2 [K], ids [T]; backward adds gi [K][D+1],
// ds [K][64], dh [T][A+1]
__host__ __device__ __forceinline__ int ip_lds_floats(int D, int T, int A, int K, bool bwd) {
    int n = T * (D + 1) + A * (D + 1) + T * (A + 1) + K * 64 + K * A + A + K + T;
    if (bwd) n += K * (D + 1) + K * 64 + T * (A + 1);
    return n;
}

template <int D>
__device__ __forceinline__ IpLds ip_carve(float *lds, int T, int A, int K) {
    IpLds L;
    L.hp = lds;
    L.w1 = L.hp + T * (D + 1);
    L.hs = L.w1 + A * (D + 1);
    L.sc = L.hs + T * (A + 1);
    L.w2 = L.sc + K * 64;
    L.b1 = L.w2 + K * A;
    L.b2 = L.b1 + A;
    L.ids = reinterpret_cast<int *>(L.b2 + K);
    L.gi = L.b2 + K + T;
    L.ds = L.gi + K * (D + 1);
    L.dh = L.ds + K * 64;
    return L;
}

struct IpParams {
    const float *item, *pos, *W1, *b1, *W2, *b2;
    const int64_t *hist;
    int64_t n_items, B;
    int T, A, K;
};

__device__ __forceinline__ float ip_leaky(float x) { return x > 0.f ? x : x * kIpLeaky; }

__device__ __forceinline__ float ip_wave_max(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

template <int D>
__device__ __forceinline__ void ip_load_params(const IpLds &L, const IpParams &P) {
    for (int i = threadIdx.x; i < P.A * D; i += kBlock) {
        const int a = i / D, d = i - a * D;
        L.w1[a * (D + 1) + d] = P.W1[i];
    }
    for (int i = threadIdx.x; i < P.K * P.A; i += kBlock) L.w2[i] = P.W2[i];
    for (int i = threadIdx.x; i < P.A; i += kBlock) L.b1[i] = P.b1[i];
    for (int i = threadIdx.x; i < P.K; i += kBlock) L.b2[i] = P.b2[i];
}

// ids -> hp, hs (the hidden layer before leaky_relu), sc (the probabilities) of sequence b; ends with a barrier
template <int D>
__device__ __forceinline__ void ip_forward_seq(const IpLds &L, const IpParams &P, int64_t b, int32_t *__restrict__ err_word) {
    constexpr int LDW = D + 1, D4 = D / 4;
    const int T = P.T, A = P.A, K = P.K, tid = threadIdx.x;
    if (tid < T) {
        int64_t id = P.hist[b * T + tid];
        if (id < 0 || id >= P.n_items) {                  // clamped before it addresses anything
            if (err_word != nullptr) atomicOr(err_word, 1);
            id = id < 0 ? 0 : P.n_items - 1;
        }
        L.ids[tid] = id > 0 ? (int)id : -1;               // the mask is history > 0
    }
    __syncthreads();
    for (int f = tid; f < T * D4; f += kBlock) {
        const int t = f / D4, c = f - t * D4;
        const int id = L.ids[t];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (id >= 0) {                                    // padded positions are not gathered
            v = reinterpret_cast<const float4 *>(P.item + (int64_t)id * D)[c];
            if (P.pos != nullptr) {
                const float4 q = reinterpret_cast<const float4 *>(P.pos + (int64_t)t * D)[c];
                v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
            }
        }
        float *dst = &L.hp[t * LDW + 4 * c];
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
    __syncthreads();
    for (int i = tid; i < T * A; i += kBlock) {
        const int t = i / A, a = i - t * A;
        const float *x = L.hp + t * LDW, *w = L.w1 + a * LDW;
        float s = 0.f;
#pragma unroll 8
        for (int d = 0; d < D; ++d) s = fmaf(x[d], w[d], s);
        L.hs[t * (A + 1) + a] = s + L.b1[a];
    }
    __syncthreads();
    for (int i = tid; i < K * T; i += kBlock) {
        const int k = i / T, t = i - k * T;
        float s = -INFINITY;
        if (L.ids[t] >= 0) {
            s = 0.f;
            for (int a = 0; a < A; ++a) s = fmaf(ip_leaky(L.hs[t * (A + 1) + a]), L.w2[k * A + a], s);
            s += L.b2[k];
        }
        L.sc[k * 64 + t] = s;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int k = wave; k < K; k += kBlock / 64) {         // one wave per row: softmax over t with the row's own maximum
        const float v = lane < T ? L.sc[k * 64 + lane] : -INFINITY;
        const float m = ip_wave_max(v);
        float p = 0.f;
        if (m > -INFINITY) {                              // wave-uniform; an all-masked row keeps p = 0 (the NaN rule)
            const float e = v > -INFINITY ? expf(v - m) : 0.f;
            p = e / wave_sum(e);
        }
        if (lane < T) L.sc[k * 64 + lane] = p;
    }
    __syncthreads();
}

template <int D>
__global__ __launch_bounds__(kBlock) void ip_fwd_kernel(IpParams P, float *__restrict__ out, int32_t *__restrict__ err_word) {
    extern __shared__ float ip_lds[];
    const IpLds L = ip_carve<D>(ip_lds, P.T, P.A, P.K);
    constexpr int LDW = D + 1;
    const int T = P.T, K = P.K;
    ip_load_params<D>(L, P);
    for (int64_t b = blockIdx.x; b < P.B; b += gridDim.x) {
        ip_forward_seq<D>(L, P, b, err_word);
        for (int i = threadIdx.x; i < K * D; i += kBlock) {
            const int k = i / D, d = i - k * D;
            float s = 0.f;
            for (int t = 0; t < T; ++t) s = fmaf(L.sc[k * 64 + t], L.hp[t * LDW + d], s);
            out[(b * K + k) * D + d] = s;
        }
        __syncthreads();
    }
}

template <int D>
__global__ __launch_bounds__(kBlock) void ip_bwd_kernel(IpParams P, const float *__restrict__ g_out, float *__restrict__ g_hp,
                                                         float *__restrict__ part, int32_t *__restrict__ err_word) {
    extern __shared__ float ip_lds[];
    const IpLds L = ip_carve<D>(ip_lds, P.T, P.A, P.K);
    constexpr int LDW = D + 1;
    constexpr int NW = kIpMaxA * D / kBlock;              // gW1 elements per thread at most
    constexpr int NP = kIpMaxT * D / kBlock;              // g_hp / position-row elements per thread at most
    const int T = P.T, A = P.A, K = P.K, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    float accW1[NW], accP[NP], accW2 = 0.f, accB1 = 0.f, accB2 = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) accW1[i] = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) accP[i] = 0.f;
    ip_load_params<D>(L, P);
    for (int64_t b = blockIdx.x; b < P.B; b += gridDim.x) {
        ip_forward_seq<D>(L, P, b, err_word);
        for (int i = tid; i < K * D; i += kBlock) {
            const int k = i / D, d = i - k * D;
            L.gi[k * LDW + d] = g_out[(b * K + k) * D + d];
        }
        __syncthreads();
        for (int i = tid; i < K * T; i += kBlock) {       // dL/dp[k][t] = <g_out[k], hp[t]>
            const int k = i / T, t = i - k * T;
            float s = 0.f;
            if (L.ids[t] >= 0) {
                const float *x = L.hp + t * LDW, *g = L.gi + k * LDW;
#pragma unroll 8
                for (int d = 0; d < D; ++d) s = fmaf(g[d], x[d], s);
            }
            L.ds[k * 64 + t] = s;
        }
        __syncthreads();
        for (int k = wave; k < K; k += kBlock / 64) {     // softmax backward: ds = p (dp - <p, dp>)
            const float p = lane < T ? L.sc[k * 64 + lane] : 0.f;
            const float dp = lane < T ? L.ds[k * 64 + lane] : 0.f;
            const float dot = wave_sum(p * dp);
            if (lane < T) L.ds[k * 64 + lane] = p * (dp - dot);
        }
        __syncthreads();
        for (int i = tid; i < T * A; i += kBlock) {       // through W2 and leaky_relu
            const int t = i / A, a = i - t * A;
            float s = 0.f;
            for (int k = 0; k < K; ++k) s = fmaf(L.ds[k * 64 + t], L.w2[k * A + a], s);
            L.dh[t * (A + 1) + a] = s * (L.hs[t * (A + 1) + a] > 0.f ? 1.f : kIpLeaky);
        }
        if (tid < K * A) {
            const int k = tid / A, a = tid - k * A;
            float s = 0.f;
            for (int t = 0; t < T; ++t) s = fmaf(L.ds[k * 64 + t], ip_leaky(L.hs[t * (A + 1) + a]), s);
            accW2 += s;
        }
        if (tid < K) {
            float s = 0.f;
            for (int t = 0; t < T; ++t) s += L.ds[tid * 64 + t];
            accB2 += s;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NP; ++i) {                    // g_hp[t] = sum_k p[k][t] g_out[k] + W1^T dh[t]
            const int idx = tid + i * kBlock;
            if (idx < T * D) {
                const int t = idx / D, d = idx - t * D;
                float v = 0.f;
                if (L.ids[t] >= 0) {
                    for (int k = 0; k < K; ++k) v = fmaf(L.sc[k * 64 + t], L.gi[k * LDW + d], v);
                    for (int a = 0; a < A; ++a) v = fmaf(L.dh[t * (A + 1) + a], L.w1[a * LDW + d], v);
                }
                g_hp[(b * T + t) * D + d] = v;            // exactly 0 at a masked position
                accP[i] += v;
            }
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int idx = tid + i * kBlock;
            if (idx < A * D) {
                const int a = idx / D, d = idx - a * D;
                float s = 0.f;
                for (int t = 0; t < T; ++t) s = fmaf(L.dh[t * (A + 1) + a], L.hp[t * LDW + d], s);
                accW1[i] += s;
            }
        }
        if (tid < A) {
            float s = 0.f;
            for (int t = 0; t < T; ++t) s += L.dh[t * (A + 1) + tid];
            accB1 += s;
        }
        __syncthreads();
    }
    // one row of partials per workgroup: gW1 | gb1 | gW2 | gb2 | position rows
    float *row = part + (int64_t)blockIdx.x * (A * D + A + K * A + K + T * D);
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int idx = tid + i * kBlock;
        if (idx < A * D) row[idx] = accW1[i];
    }
    row += A * D;
    if (tid < A) row[tid] = accB1;
    row += A;
    if (tid < K * A) row[tid] = accW2;
    row += K * A;
    if (tid < K) row[tid] = accB2;
    row += K;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int idx = tid + i * kBlock;
        if (idx < T * D) row[idx] = accP[i];
    }
}

// element e of [gW1 | gb1 | gW2 | gb2 | gpos]: the partials summed in workgroup order; position rows at or past T are zero
__global__ __launch_bounds__(kBlock) void ip_fold_kernel(const float *__restrict__ part, int n_part, int P, int n_w1, int n_b1, int n_w2,
                                                          int n_b2, int n_pos_used, int n_pos_all, float *__restrict__ gW1,
                                                          float *__restrict__ gb1, float *__restrict__ gW2, float *__restrict__ gb2,
                                                          float *__restrict__ gpos) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    const int n_main = n_w1 + n_b1 + n_w2 + n_b2;
    if (e >= n_main + n_pos_all) return;
    float v = 0.f;
    if (e < n_main + n_pos_used)
        for (int w = 0; w < n_part; ++w) v += part[(int64_t)w * P + e];
    if (e < n_w1) gW1[e] = v;
    else if (e < n_w1 + n_b1) gb1[e - n_w1] = v;
    else if (e < n_w1 + n_b1 + n_w2) gW2[e - n_w1 - n_b1] = v;
    else if (e < n_main) gb2[e - n_w1 - n_b1 - n_w2] = v;
    else gpos[e - n_main] = v;
}

static int32_t ip_check(const char *entry, const float *item_tab, int64_t n_items, const float *pos_tab, int64_t n_pos_rows, int32_t D,
                        const int64_t *history, int64_t B, int32_t T, const float *W1, const float *b1, const float *W2,
                        const float *b2, int32_t A, int32_t K) {
    WR_REQUIRE(ip_supported(D, A, K, T), WR_E_RANGE,
               "%s supports D in {32, 64, 128}, 1 <= A <= 32, 1 <= K <= 8, 1 <= T <= 64; got D=%d A=%d K=%d T=%d", entry, D, A, K, T);
    WR_REQUIRE(item_tab && history && W1 && b1 && W2 && b2, WR_E_NULL, "%s: NULL argument", entry);
    WR_REQUIRE(n_items >= 1 && n_items < (int64_t(1) << 31), WR_E_SHAPE, "%s: n_items=%lld out of range", entry, (long long)n_items);
    WR_REQUIRE(B >= 1 && B <= (int64_t(1) << 24), WR_E_SHAPE, "%s: B=%lld out of range (1..2^24)", entry, (long long)B);
    WR_REQUIRE(pos_tab == nullptr || n_pos_rows >= T, WR_E_SHAPE, "%s: the position table has %lld rows for T=%d", entry,
               (long long)n_pos_rows, T);
    WR_REQUIRE(pos_tab == nullptr || n_pos_rows <= 4096, WR_E_SHAPE, "%s: the position table has %lld rows (4096 at most)", entry,
               (long long)n_pos_rows);
    WR_REQUIRE(aligned16(item_tab) && aligned16(pos_tab), WR_E_ALIGN, "%s: the tables must be 16-byte aligned", entry);
    return WR_OK;
}

#define WR_IP_DISPATCH(D, CALL)          \
    do {                                 \
        if ((D) == 64) { CALL(64); }     \
        else if ((D) == 32) { CALL(32); } \
        else { CALL(128); }              \
    } while (0)

}  // namespace wr

using namespace wr;

extern "C" {

int32_t wr_interest_pool_supported(int32_t D, int32_t A, int32_t K, int32_t T) { return ip_supported(D, A, K, T) ? 1 : 0; }

int64_t wr_interest_pool_workspace_bytes(int64_t B, int32_t D, int32_t A, int32_t K, int32_t T) {
    WR_REQUIRE(ip_supported(D, A, K, T) && B >= 1 && B <= (int64_t(1) << 24), WR_E_RANGE,
               "wr_interest_pool_workspace_bytes supports D in {32, 64, 128}, 1 <= A <= 32, 1 <= K <= 8, 1 <= T <= 64, 1 <= B <= 2^24; "
               "got B=%lld D=%d A=%d K=%d T=%d", (long long)B, D, A, K, T);
    return align_up((int64_t)kIpBwdWg * ip_partial_floats(D, A, K, T) * 4, 256);   // sized by the bound, not by min(B, bound)
}

int32_t wr_interest_pool_fwd(const float *item_tab, int64_t n_items, const float *pos_tab, int64_t n_pos_rows, int32_t D,
                             const int64_t *history, int64_t B, int32_t T, const float *W1, const float *b1, const float *W2,
                             const float *b2, int32_t A, int32_t K, float *out, int32_t *err_word, void *stream_) {
    const char *entry = "wr_interest_pool_fwd";
    const int32_t rc = ip_check(entry, item_tab, n_items, pos_tab, n_pos_rows, D, history, B, T, W1, b1, W2, b2, A, K);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(out != nullptr, WR_E_NULL, "%s: NULL argument", entry);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const IpParams P{item_tab, pos_tab, W1, b1, W2, b2, history, n_items, B, T, A, K};
    const size_t lds = (size_t)ip_lds_floats(D, T, A, K, false) * 4;      // <= 61,472 B
    const unsigned grid = (unsigned)(B < kIpFwdWg ? B : kIpFwdWg);
#define WR_IP_FWD(D_) hipLaunchKernelGGL(ip_fwd_kernel<D_>, dim3(grid), dim3(kBlock), lds, stream, P, out, err_word)
    WR_IP_DISPATCH(D, WR_IP_FWD);
#undef WR_IP_FWD
    WR_LAUNCH_CHECK("ip_fwd_kernel");
    return WR_OK;
}

int32_t wr_interest_pool_bwd(const float *item_tab, int64_t n_items, const float *pos_tab, int64_t n_pos_rows, int32_t D,
                             const int64_t *history, int64_t B, int32_t T, const float *W1, const float *b1, const float *W2,
                             const float *b2, int32_t A, int32_t K, const float *g_out, float *g_hp, float *gW1, float *gb1,
                             float *gW2, float *gb2, float *gpos, int32_t *err_word, void *workspace, int64_t workspace_bytes,
                             void *stream_) {
    const char *entry = "wr_interest_pool_bwd";
    int32_t rc = ip_check(entry, item_tab, n_items, pos_tab, n_pos_rows, D, history, B, T, W1, b1, W2, b2, A, K);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(g_out && g_hp && gW1 && gb1 && gW2 && gb2, WR_E_NULL, "%s: NULL argument", entry);
    WR_REQUIRE((pos_tab == nullptr) == (gpos == nullptr), WR_E_NULL, "%s: gpos goes with pos_tab", entry);
    if ((rc = check_workspace(entry, workspace, workspace_bytes, wr_interest_pool_workspace_bytes(B, D, A, K, T))) != WR_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const IpParams P{item_tab, pos_tab, W1, b1, W2, b2, history, n_items, B, T, A, K};
    const size_t lds = (size_t)ip_lds_floats(D, T, A, K, true) * 4;       // <= 76,096 B
    float *part = reinterpret_cast<float *>(workspace);
    const int n_wg = (int)(B < kIpBwdWg ? B : kIpBwdWg);
#define WR_IP_BWD(D_)                                                                                                          \
    do {                                                                                                                       \
        if (lds > 64 * 1024)                                                                                                   \
            WR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ip_bwd_kernel<D_>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                       (int)lds));                                                                             \
        hipLaunchKernelGGL(ip_bwd_kernel<D_>, dim3(n_wg), dim3(kBlock), lds, stream, P, g_out, g_hp, part, err_word);          \
    } while (0)
    WR_IP_DISPATCH(D, WR_IP_BWD);
#undef WR_IP_BWD
    WR_LAUNCH_CHECK("ip_bwd_kernel");
    const int n_pos_used = gpos != nullptr ? T * D : 0, n_pos_all = gpos != nullptr ? (int)n_pos_rows * D : 0;
    const int n_out = (int)ip_main_params(D, A, K) + n_pos_all;
    hipLaunchKernelGGL(ip_fold_kernel, dim3((n_out + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, part, n_wg,
                       (int)ip_partial_floats(D, A, K, T), A * D, A, K * A, K, n_pos_used, n_pos_all, gW1, gb1, gW2, gb2, gpos);
    WR_LAUNCH_CHECK("ip_fold_kernel");
    return WR_OK;
}

}  // extern "C"
