// wr_views.hip — SGL's two augmented graph views, forward and transposed, and their chunk tables, built on the device.
//
// Device counterpart of augmentor.edge_dropout / node_dropout + csr2tensor (reference src/utils/augmentor.py:33-111,
// src/models/general/SGL.py:105-146) as whisprrec_amd/sgl.py restates them on the host (edge_dropout_edges / node_dropout_edges,
// norm_csr, transpose_csr) and of hip_ops.spmm_chunks.  The host path draws an exact-size uniform subset with random.sample
// and sorts twice per view; here the subset is "element e is selected iff perm(e) < n_select" with the keyed bijection of
// wr_shuffle.h — the same distribution (a uniform bijection maps a fixed set of n_select positions to a uniform subset of
// that size), NOT the reference's `random` stream — and, because the base edge list is sorted by (row, col), a
// view's CSR is a stream compaction of it:
//   keep     one flag byte per base edge (ED: the edge's own draw; ND: neither its row node nor its column node is dropped)
//   count    one wave per 64-edge chunk of the BASE list (chunks never cross a row, every row owns at least one): ballot and
//            popcount of keep[e] (forward view) and of keep[mirror[e]] (transposed view: row a lists b iff (b, a) was kept)
//   scan     by the caller over the chunk counts (the chunks are in row-major order: a chunk's scanned value is its write
//            offset, a row's first chunk gives the view's row_ptr)
//   fill     same grid; the in-chunk position is the ballot prefix; val = dis_tab[cnt[a]] * dis_tab[cnt[b]], one fp32
//            multiply of two entries of the host-built table, so the bits are norm_csr's.  The product is the same for an edge
//            and its mirror (fp32 multiplication commutes), which is what transpose_csr copies.
// Deterministic: no float atomics, every output element has one writer.  Stores of one wave go to consecutive int32 / fp32
// slots (the kept lanes of a chunk are compacted), loads of rows / cols / keep are lane-consecutive; keep[mirror[e]],
// row_ptr[a], row_ptr[b] and dis_tab[.] are gathers that stay in L2 (1 B per edge, 8 B per node, 4 B per degree).
// The 8-round hash chain (16 64-bit multiplies per evaluation, ~2 evaluations with cycle walking) is pure VALU work on a
// handful of registers: no LDS, far below 64 VGPRs, so the flag kernels run at full occupancy (8 waves per SIMD) and are
// bound by issue slots, 1-2 us per million elements.
#include "wr_common.h"
#include "wr_shuffle.h"

namespace wr {

constexpr int kViewChunk = 64;                      // base edges per wave: one ballot
constexpr int kWavesPerBlock = kBlock / 64;

static inline int64_t views_flag_offset(int64_t n_edges) { return align_up(n_edges, 16); }

__device__ __forceinline__ void flag_err(int32_t *err, int32_t bit) {
    if (err) atomicOr(err, bit);
}

// ND: flags[v] = row node v dropped, flags[N + v] = column node v dropped (two independent bijections)
__global__ __launch_bounds__(kBlock) void node_drop_kernel(int64_t n_nodes, unsigned bits, uint64_t key_rows, uint64_t key_cols,
                                                            uint64_t n_drop, uint8_t *__restrict__ flags) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= n_nodes) return;
    flags[v] = shuffle_index((uint64_t)v, (uint64_t)n_nodes, bits, key_rows) < n_drop ? 1 : 0;
    flags[n_nodes + v] = shuffle_index((uint64_t)v, (uint64_t)n_nodes, bits, key_cols) < n_drop ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void edge_keep_ed_kernel(int64_t n_edges, unsigned bits, uint64_t key, uint64_t n_keep,
                                                               uint8_t *__restrict__ keep) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_edges) return;
    keep[e] = shuffle_index((uint64_t)e, (uint64_t)n_edges, bits, key) < n_keep ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void edge_keep_nd_kernel(const int32_t *__restrict__ rows, const int32_t *__restrict__ cols,
                                                               int64_t n_edges, int64_t n_nodes, const uint8_t *__restrict__ flags,
                                                               uint8_t *__restrict__ keep, int32_t *__restrict__ err) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_edges) return;
    const int64_t a = rows[e], b = cols[e];
    if (a < 0 || a >= n_nodes || b < 0 || b >= n_nodes) {
        flag_err(err, 1);
        keep[e] = 0;
        return;
    }
    keep[e] = (flags[a] | flags[n_nodes + b]) ? 0 : 1;
}

// the base edges [lo, lo + len) of one chunk; a malformed table yields an empty chunk and a flag, never an address
__device__ __forceinline__ void chunk_span(const int64_t *__restrict__ bptr, int64_t chunk, int64_t n_edges, int64_t &lo, int &len,
                                           int32_t *err) {
    lo = bptr[chunk];
    const int64_t hi = bptr[chunk + 1];
    if (lo < 0 || hi < lo || hi > n_edges || hi - lo > kViewChunk) {
        flag_err(err, 2);
        lo = 0;
        len = 0;
        return;
    }
    len = (int)(hi - lo);
}

__device__ __forceinline__ int64_t mirror_of(const int32_t *__restrict__ mirror, int64_t e, int64_t n_edges, int32_t *err) {
    const int64_t m = mirror[e];
    if (m < 0 || m >= n_edges) {
        flag_err(err, 4);
        return e;
    }
    return m;
}

__global__ __launch_bounds__(kBlock) void view_count_kernel(const int32_t *__restrict__ mirror, const uint8_t *__restrict__ keep,
                                                             int64_t n_edges, const int64_t *__restrict__ bptr, int64_t n_bchunks,
                                                             int32_t *__restrict__ cnt_fwd, int32_t *__restrict__ cnt_bwd,
                                                             int32_t *__restrict__ err) {
    const int64_t chunk = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);     // wave-uniform
    if (chunk >= n_bchunks) return;
    const int lane = threadIdx.x & 63;
    int64_t lo;
    int len;
    chunk_span(bptr, chunk, n_edges, lo, len, err);
    bool kf = false, kb = false;
    if (lane < len) {
        const int64_t e = lo + lane;
        kf = keep[e] != 0;
        kb = keep[mirror_of(mirror, e, n_edges, err)] != 0;
    }
    const unsigned long long mf = __ballot(kf), mb = __ballot(kb);
    if (lane == 0) {
        cnt_fwd[chunk] = __popcll(mf);
        cnt_bwd[chunk] = __popcll(mb);
    }
}

// row_ptr of both directions: the scanned count of the row's first base chunk (entry n_nodes: of the end, the view's nnz)
__global__ __launch_bounds__(kBlock) void view_rows_kernel(const int64_t *__restrict__ row_first_chunk, int64_t n_nodes,
                                                            int64_t n_bchunks, const int64_t *__restrict__ scan_fwd,
                                                            const int64_t *__restrict__ scan_bwd, int64_t *__restrict__ rp_fwd,
                                                            int64_t *__restrict__ rp_bwd) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r > n_nodes) return;
    int64_t c = row_first_chunk[r];
    c = c < 0 ? 0 : (c > n_bchunks ? n_bchunks : c);
    rp_fwd[r] = scan_fwd[c];
    rp_bwd[r] = scan_bwd[c];
}

__global__ __launch_bounds__(kBlock) void view_fill_kernel(const int32_t *__restrict__ rows, const int32_t *__restrict__ cols,
                                                            const int32_t *__restrict__ mirror, const uint8_t *__restrict__ keep,
                                                            int64_t n_edges, int64_t n_nodes, const int64_t *__restrict__ bptr,
                                                            int64_t n_bchunks, const int64_t *__restrict__ scan_fwd,
                                                            const int64_t *__restrict__ scan_bwd, const int64_t *__restrict__ rp_fwd,
                                                            const float *__restrict__ dis_tab, int64_t n_dis,
                                                            int32_t *__restrict__ col_fwd, float *__restrict__ val_fwd, int64_t nnz_fwd,
                                                            int32_t *__restrict__ col_bwd, float *__restrict__ val_bwd, int64_t nnz_bwd,
                                                            int32_t *__restrict__ err) {
    const int64_t chunk = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);     // wave-uniform
    if (chunk >= n_bchunks) return;
    const int lane = threadIdx.x & 63;
    int64_t lo;
    int len;
    chunk_span(bptr, chunk, n_edges, lo, len, err);
    bool kf = false, kb = false;
    int64_t a = 0, b = 0;
    if (lane < len) {
        const int64_t e = lo + lane;
        a = rows[e];
        b = cols[e];
        if (a < 0 || a >= n_nodes || b < 0 || b >= n_nodes) {
            flag_err(err, 1);
            a = b = 0;
        } else {
            kf = keep[e] != 0;
            kb = keep[mirror_of(mirror, e, n_edges, err)] != 0;
        }
    }
    const unsigned long long mf = __ballot(kf), mb = __ballot(kb);
    if (!(kf || kb)) return;
    // kept row edges of the two end nodes in THIS view (forward counts on both sides, as norm_csr's row sums)
    int64_t ca = rp_fwd[a + 1] - rp_fwd[a], cb = rp_fwd[b + 1] - rp_fwd[b];
    if (ca < 0 || ca >= n_dis || cb < 0 || cb >= n_dis) {
        flag_err(err, 8);
        ca = ca < 0 ? 0 : (ca >= n_dis ? n_dis - 1 : ca);
        cb = cb < 0 ? 0 : (cb >= n_dis ? n_dis - 1 : cb);
    }
    const float v = dis_tab[ca] * dis_tab[cb];
    const unsigned long long below = (1ull << lane) - 1ull;
    if (kf) {
        const int64_t pos = scan_fwd[chunk] + __popcll(mf & below);
        if (pos >= 0 && pos < nnz_fwd) {
            col_fwd[pos] = (int32_t)b;
            val_fwd[pos] = v;
        } else {
            flag_err(err, 16);
        }
    }
    if (kb) {
        const int64_t pos = scan_bwd[chunk] + __popcll(mb & below);
        if (pos >= 0 && pos < nnz_bwd) {
            col_bwd[pos] = (int32_t)b;
            val_bwd[pos] = v;
        } else {
            flag_err(err, 16);
        }
    }
}

// ----------------------------------------------------------------------------------------------- chunk tables
// hip_ops.spmm_chunks on the device: per = max(1, ceil(deg / max_nnz)) chunks per row, chunk k of row r starts at
// row_ptr[r] + k * max_nnz.
__global__ __launch_bounds__(kBlock) void chunks_count_kernel(const int64_t *__restrict__ row_ptr, int64_t n_rows, int32_t max_nnz,
                                                               int64_t *__restrict__ per, int32_t *__restrict__ max_per) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t p = 0;
    if (r < n_rows) {
        int64_t deg = row_ptr[r + 1] - row_ptr[r];
        if (deg < 0) deg = 0;
        const int64_t q = (deg + max_nnz - 1) / max_nnz;
        p = (int32_t)(q < 1 ? 1 : (q > 0x7fffffff ? 0x7fffffff : q));
        per[r] = p;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(p, off, 64);
        p = o > p ? o : p;
    }
    if ((threadIdx.x & 63) == 0 && p > 0) atomicMax(max_per, p);
}

__global__ __launch_bounds__(kBlock) void chunks_fill_kernel(const int64_t *__restrict__ row_ptr, int64_t n_rows, int32_t max_nnz,
                                                              const int64_t *__restrict__ chunk_first, int64_t n_chunks,
                                                              int64_t *__restrict__ chunk_ptr, int32_t *__restrict__ chunk_row) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t first = chunk_first[r], end = chunk_first[r + 1], start = row_ptr[r];
    for (int64_t k = first; k < end; ++k) {
        if (k < 0 || k >= n_chunks) break;                     // a scan that does not match n_chunks never addresses past it
        chunk_ptr[k] = start + (k - first) * max_nnz;
        chunk_row[k] = (int32_t)r;
    }
    if (r == n_rows - 1) chunk_ptr[n_chunks] = row_ptr[n_rows];
}

static inline unsigned blocks_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

static int32_t check_view_sizes(const char *entry, int64_t n_edges, int64_t n_nodes, int64_t n_bchunks) {
    WR_REQUIRE(n_edges >= 1 && n_edges < (int64_t(1) << 31) && n_nodes >= 1 && n_nodes < (int64_t(1) << 31), WR_E_SHAPE,
               "%s: n_edges=%lld, n_nodes=%lld must lie in [1, 2^31)", entry, (long long)n_edges, (long long)n_nodes);
    WR_REQUIRE(n_bchunks >= n_nodes && n_bchunks <= n_edges + n_nodes, WR_E_SHAPE,
               "%s: %lld base chunks for %lld rows and %lld edges (every row owns at least one chunk of at most %d edges)", entry,
               (long long)n_bchunks, (long long)n_nodes, (long long)n_edges, kViewChunk);
    return WR_OK;
}

}  // namespace wr

using namespace wr;

extern "C" {

int64_t wr_sgl_views_workspace_bytes(int64_t n_nodes, int64_t n_edges) {
    if (n_edges < 1 || n_edges >= (int64_t(1) << 31) || n_nodes < 1 || n_nodes >= (int64_t(1) << 31)) {
        set_error("wr_sgl_views_workspace_bytes: n_edges=%lld, n_nodes=%lld must lie in [1, 2^31)", (long long)n_edges,
                  (long long)n_nodes);
        return WR_E_SHAPE;
    }
    return views_flag_offset(n_edges) + align_up(2 * n_nodes, 16);
}

int32_t wr_sgl_view_count(int32_t kind, const int32_t *rows, const int32_t *cols, const int32_t *mirror, int64_t n_edges,
                          int64_t n_nodes, const int64_t *bchunk_ptr, int64_t n_bchunks, int64_t n_select, uint64_t seed,
                          uint64_t stream_id0, uint64_t stream_id1, int32_t *cnt_fwd, int32_t *cnt_bwd, int32_t *err_word,
                          void *workspace, int64_t workspace_bytes, void *stream_) {
    WR_REQUIRE(rows && cols && mirror && bchunk_ptr && cnt_fwd && cnt_bwd, WR_E_NULL, "wr_sgl_view_count: NULL argument");
    WR_REQUIRE(kind == WR_VIEW_EDGE_DROP || kind == WR_VIEW_NODE_DROP, WR_E_RANGE, "wr_sgl_view_count: kind %d is neither edge (0) "
               "nor node (1) dropout", (int)kind);
    int32_t rc = check_view_sizes("wr_sgl_view_count", n_edges, n_nodes, n_bchunks);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(n_select >= 0 && n_select <= (kind == WR_VIEW_EDGE_DROP ? n_edges : n_nodes), WR_E_RANGE,
               "wr_sgl_view_count: n_select=%lld outside [0, %lld]", (long long)n_select,
               (long long)(kind == WR_VIEW_EDGE_DROP ? n_edges : n_nodes));
    rc = check_workspace("wr_sgl_view_count", workspace, workspace_bytes, wr_sgl_views_workspace_bytes(n_nodes, n_edges));
    if (rc != WR_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    uint8_t *keep = static_cast<uint8_t *>(workspace);
    if (kind == WR_VIEW_EDGE_DROP) {
        hipLaunchKernelGGL(edge_keep_ed_kernel, dim3(blocks_for(n_edges, kBlock)), dim3(kBlock), 0, stream, n_edges,
                           shuffle_bits(n_edges), shuffle_key(seed, stream_id0), (uint64_t)n_select, keep);
        WR_LAUNCH_CHECK("edge_keep_ed_kernel");
    } else {
        uint8_t *flags = keep + views_flag_offset(n_edges);
        hipLaunchKernelGGL(node_drop_kernel, dim3(blocks_for(n_nodes, kBlock)), dim3(kBlock), 0, stream, n_nodes,
                           shuffle_bits(n_nodes), shuffle_key(seed, stream_id0), shuffle_key(seed, stream_id1), (uint64_t)n_select,
                           flags);
        WR_LAUNCH_CHECK("node_drop_kernel");
        hipLaunchKernelGGL(edge_keep_nd_kernel, dim3(blocks_for(n_edges, kBlock)), dim3(kBlock), 0, stream, rows, cols, n_edges,
                           n_nodes, flags, keep, err_word);
        WR_LAUNCH_CHECK("edge_keep_nd_kernel");
    }
    hipLaunchKernelGGL(view_count_kernel, dim3(blocks_for(n_bchunks, kWavesPerBlock)), dim3(kBlock), 0, stream, mirror, keep,
                       n_edges, bchunk_ptr, n_bchunks, cnt_fwd, cnt_bwd, err_word);
    WR_LAUNCH_CHECK("view_count_kernel");
    return WR_OK;
}

int32_t wr_sgl_view_rows(const int64_t *row_first_chunk, int64_t n_nodes, int64_t n_bchunks, const int64_t *scan_fwd,
                         const int64_t *scan_bwd, int64_t *row_ptr_fwd, int64_t *row_ptr_bwd, void *stream) {
    WR_REQUIRE(row_first_chunk && scan_fwd && scan_bwd && row_ptr_fwd && row_ptr_bwd, WR_E_NULL, "wr_sgl_view_rows: NULL argument");
    WR_REQUIRE(n_nodes >= 1 && n_nodes < (int64_t(1) << 31) && n_bchunks >= n_nodes && n_bchunks < (int64_t(1) << 32), WR_E_SHAPE,
               "wr_sgl_view_rows: n_nodes=%lld, n_bchunks=%lld out of range", (long long)n_nodes, (long long)n_bchunks);
    hipLaunchKernelGGL(view_rows_kernel, dim3(blocks_for(n_nodes + 1, kBlock)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       row_first_chunk, n_nodes, n_bchunks, scan_fwd, scan_bwd, row_ptr_fwd, row_ptr_bwd);
    WR_LAUNCH_CHECK("view_rows_kernel");
    return WR_OK;
}

int32_t wr_sgl_view_fill(const int32_t *rows, const int32_t *cols, const int32_t *mirror, int64_t n_edges, int64_t n_nodes,
                         const int64_t *bchunk_ptr, int64_t n_bchunks, const int64_t *scan_fwd, const int64_t *scan_bwd,
                         const int64_t *row_ptr_fwd, const float *dis_tab, int64_t n_dis, int32_t *col_fwd, float *val_fwd,
                         int64_t nnz_fwd, int32_t *col_bwd, float *val_bwd, int64_t nnz_bwd, int32_t *err_word,
                         const void *workspace, int64_t workspace_bytes, void *stream) {
    WR_REQUIRE(rows && cols && mirror && bchunk_ptr && scan_fwd && scan_bwd && row_ptr_fwd && dis_tab, WR_E_NULL,
               "wr_sgl_view_fill: NULL argument");
    const int32_t rc = check_view_sizes("wr_sgl_view_fill", n_edges, n_nodes, n_bchunks);
    if (rc != WR_OK) return rc;
    WR_REQUIRE(n_dis >= 1 && nnz_fwd >= 0 && nnz_fwd <= n_edges && nnz_bwd >= 0 && nnz_bwd <= n_edges, WR_E_SHAPE,
               "wr_sgl_view_fill: n_dis=%lld, nnz=%lld / %lld out of range", (long long)n_dis, (long long)nnz_fwd, (long long)nnz_bwd);
    WR_REQUIRE((nnz_fwd == 0 || (col_fwd && val_fwd)) && (nnz_bwd == 0 || (col_bwd && val_bwd)), WR_E_NULL,
               "wr_sgl_view_fill: col / val of a non-empty view is NULL");
    WR_REQUIRE(workspace && workspace_bytes >= wr_sgl_views_workspace_bytes(n_nodes, n_edges), WR_E_WORKSPACE,
               "wr_sgl_view_fill: workspace %lld B < %lld B (the one wr_sgl_view_count filled)", (long long)workspace_bytes,
               (long long)wr_sgl_views_workspace_bytes(n_nodes, n_edges));
    hipLaunchKernelGGL(view_fill_kernel, dim3(blocks_for(n_bchunks, kWavesPerBlock)), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), rows, cols, mirror, static_cast<const uint8_t *>(workspace), n_edges,
                       n_nodes, bchunk_ptr, n_bchunks, scan_fwd, scan_bwd, row_ptr_fwd, dis_tab, n_dis, col_fwd, val_fwd, nnz_fwd,
                       col_bwd, val_bwd, nnz_bwd, err_word);
    WR_LAUNCH_CHECK("view_fill_kernel");
    return WR_OK;
}

int32_t wr_spmm_chunks_count(const int64_t *row_ptr, int64_t n_rows, int32_t max_nnz, int64_t *per, int32_t *max_per,
                             void *stream) {
    WR_REQUIRE(row_ptr && per && max_per, WR_E_NULL, "wr_spmm_chunks_count: NULL argument");
    WR_REQUIRE(n_rows >= 1 && n_rows < (int64_t(1) << 31) && max_nnz >= 1, WR_E_SHAPE,
               "wr_spmm_chunks_count: n_rows=%lld, max_nnz=%d out of range", (long long)n_rows, (int)max_nnz);
    hipLaunchKernelGGL(chunks_count_kernel, dim3(blocks_for(n_rows, kBlock)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       row_ptr, n_rows, max_nnz, per, max_per);
    WR_LAUNCH_CHECK("chunks_count_kernel");
    return WR_OK;
}

int32_t wr_spmm_chunks_fill(const int64_t *row_ptr, int64_t n_rows, int32_t max_nnz, const int64_t *chunk_first, int64_t n_chunks,
                            int64_t *chunk_ptr, int32_t *chunk_row, void *stream) {
    WR_REQUIRE(row_ptr && chunk_first && chunk_ptr && chunk_row, WR_E_NULL, "wr_spmm_chunks_fill: NULL argument");
    WR_REQUIRE(n_rows >= 1 && n_rows < (int64_t(1) << 31) && max_nnz >= 1 && n_chunks >= n_rows, WR_E_SHAPE,
               "wr_spmm_chunks_fill: n_rows=%lld, max_nnz=%d, n_chunks=%lld out of range", (long long)n_rows, (int)max_nnz,
               (long long)n_chunks);
    hipLaunchKernelGGL(chunks_fill_kernel, dim3(blocks_for(n_rows, kBlock)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       row_ptr, n_rows, max_nnz, chunk_first, n_chunks, chunk_ptr, chunk_row);
    WR_LAUNCH_CHECK("chunks_fill_kernel");
    return WR_OK;
}

}  // extern "C"
