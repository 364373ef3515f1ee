// wr_row_team.h — one row of D <= 128 floats held by a team of 16 lanes, and F.normalize (eps 1e-12) forward and backward on
// such rows: the row kernels of wr_infonce.hip (K12) and wr_supcon.hip (K15).
#pragma once
#include "wr_common.h"

namespace wr {

constexpr float kNceEps = 1e-12f;         // F.normalize's eps
constexpr int kNceTeam = 16;              // lanes per row in the row kernels
constexpr int kNceTeamsPerBlock = kBlock / kNceTeam;

__device__ __forceinline__ float nce_team_sum(float v) {
    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
    return v;
}

// One row of D <= 128 floats over a team of 16 lanes: lane l holds float4 chunks l and l + 16 (those below D / 4).
struct NceRow {
    float4 v[2];
};

__device__ __forceinline__ NceRow nce_load(const float *__restrict__ p, int D4, int l) {
    NceRow r;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = l + k * kNceTeam;
        r.v[k] = (c < D4) ? reinterpret_cast<const float4 *>(p)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return r;
}

__device__ __forceinline__ void nce_store(float *__restrict__ p, int D4, int l, const NceRow &r) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = l + k * kNceTeam;
        if (c < D4) reinterpret_cast<float4 *>(p)[c] = r.v[k];
    }
}

__device__ __forceinline__ float nce_dot(const NceRow &a, const NceRow &b) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        s = fmaf(a.v[k].x, b.v[k].x, s); s = fmaf(a.v[k].y, b.v[k].y, s);
        s = fmaf(a.v[k].z, b.v[k].z, s); s = fmaf(a.v[k].w, b.v[k].w, s);
    }
    return nce_team_sum(s);
}

// r = a * s + b * t, element-wise
__device__ __forceinline__ NceRow nce_axpby(const NceRow &a, float s, const NceRow &b, float t) {
    NceRow r;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        r.v[k].x = a.v[k].x * s + b.v[k].x * t; r.v[k].y = a.v[k].y * s + b.v[k].y * t;
        r.v[k].z = a.v[k].z * s + b.v[k].z * t; r.v[k].w = a.v[k].w * s + b.v[k].w * t;
    }
    return r;
}

__device__ __forceinline__ void nce_add(NceRow &a, const NceRow &b) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        a.v[k].x += b.v[k].x; a.v[k].y += b.v[k].y; a.v[k].z += b.v[k].z; a.v[k].w += b.v[k].w;
    }
}

// x / max(|x|, eps) and the signed reciprocal that the backward pass needs: inv > 0 for a row with |x| >= eps, and -1/eps
// for a clamped row (F.normalize's clamp_min passes no gradient to the norm there: the backward is g / eps, no projection).
__device__ __forceinline__ NceRow nce_normalize(const NceRow &x, float &inv_signed) {
    const float nrm = sqrtf(nce_dot(x, x));
    const float inv = 1.0f / fmaxf(nrm, kNceEps);
    inv_signed = nrm < kNceEps ? -inv : inv;
    NceRow zero;
    zero.v[0] = zero.v[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    return nce_axpby(x, inv, zero, 0.f);
}

// gradient w.r.t. x of y = x / max(|x|, eps), given g = d loss / d y, y and the signed reciprocal:
// (g - y <y, g>) / |x| for a regular row, g / eps for a clamped one
__device__ __forceinline__ NceRow nce_bwd(const NceRow &g, const NceRow &y, float inv_signed) {
    const float dt = nce_dot(y, g);                                      // every lane of the team takes part
    if (inv_signed < 0.f) return nce_axpby(g, -inv_signed, y, 0.f);
    NceRow t = nce_axpby(g, 1.0f, y, -dt);
    return nce_axpby(t, inv_signed, y, 0.f);
}

}  // namespace wr
