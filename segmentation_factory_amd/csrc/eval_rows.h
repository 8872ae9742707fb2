// What the evaluation kernels with classes on lanes share (eval_msf.hip, eval_slide.hip, and through loss_geom.h the arg max kernels
// of loss.hip): a wave's slice of an image's pixels, the reductions over a pixel's lane group, the arg max of a class row spread over
// the group and the counting of one (label, prediction) pair.
#pragma once
#include "common.h"

// The pixels [p0, p1) of an image's npix that this wave walks: contiguous slices, 4 waves per workgroup, gridDim.x workgroups per image
__device__ __forceinline__ void wave_pixel_range(int64_t npix, int64_t& p0, int64_t& p1) {
    const int64_t nw = (int64_t)gridDim.x * 4;
    const int64_t per = (npix + nw - 1) / nw;
    const int64_t wid = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    p0 = wid * per; p1 = p0 + per < npix ? p0 + per : npix;
}

// reductions over the GW lanes of a pixel's group (every lane of the wave active); GW == 64: wave-uniform result
template <int GW> __device__ __forceinline__ float grp_max(float v) { return GW == 64 ? wave_max_all(v) : wave_max(v, GW); }
template <int GW> __device__ __forceinline__ float grp_sum(float v) { return GW == 64 ? wave_sum_all(v) : wave_sum(v, GW); }

// arg max of a class row held as S[s] = class cl + 64 s on the group's lane cl: the lowest class index attaining the maximum
// (wave_argmax of loss.hip, per group); 0 on an all-NaN row.  Every lane of the wave active; the result is the same on every lane of
// the group.
template <int NS, int GW> __device__ __forceinline__ int grp_argmax(const float (&S)[NS], int cl, int C) {
    float zs[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) zs[s] = cl + 64 * s < C ? S[s] : -INFINITY;
    float mx = zs[0];
#pragma unroll
    for (int s = 1; s < NS; ++s) mx = fmaxf(mx, zs[s]);
    mx = grp_max<GW>(mx);
    float cand = -1e9f;                                           // -(index): the lowest index is the maximum of the negated ones
#pragma unroll
    for (int s = NS - 1; s >= 0; --s) if (zs[s] == mx) cand = -(float)(cl + 64 * s);
    const int bi = (int)(-grp_max<GW>(cand));
    return bi < C ? bi : 0;
}

// one pixel's count in both confusion matrices: mat at [t][best] where 0 <= t < C, hist the same except t == ignore_label; a label outside
// [0, C) that is not ignore_label sets flag bit 0 and is counted nowhere (the reference's bincount shape check fails there)
__device__ __forceinline__ void eval_count(int64_t t, int best, int C, int64_t ignore_label, unsigned long long* __restrict__ mat,
                                           unsigned long long* __restrict__ hist, int* __restrict__ flag) {
    const bool in_mat = t >= 0 && t < C;
    if (in_mat) atomicAdd(mat + t * C + best, 1ull);
    if (t != ignore_label) {
        if (in_mat) atomicAdd(hist + t * C + best, 1ull);
        else atomicOr(flag, 1);
    }
}
