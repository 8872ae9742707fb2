// Multi-scale + flip SLIDING-WINDOW evaluation: per (scale, flip) pair the mean over the low-resolution logit maps of the overlapping
// crops of the scaled image, resampled to the label size, softmaxed and summed over the pairs; arg max of the sum and both confusion
// matrices, in one kernel (segf_msf_slide_argmax_confmat, include/segfac.h).
//   mmseg's aug_test with mode='slide' -- SegFormer's multi-scale Cityscapes figures (crop 1024, stride 768 over 1024 x 2048 at scales
//   0.5 ... 1.75, each mirrored) and most multi-scale ADE20K / VOC figures (crop 512, stride 341).  Done with tensors that is, per
//   scale and flip, a full-resolution [C, ch, cw] fp32 map per window, a [C, Hs, Ws] accumulator at the SCALED size (488 MB per image
//   at scale 1.75 of Cityscapes), its resize to the label size, a softmax map and a running sum.  Here a pixel's class row of a window
//   set is built from the low-resolution NHWC rows alone: the (at most four) outer taps of the resize from (Hs, Ws) to (H, W), at each
//   tap the window mean of eval_slide.hip, the four means combined in ATen's order, then the softmax + sum of eval_msf.hip.
// Layout of the work: that of the two siblings -- classes on lanes, one GROUP of GW lanes per pixel (GW = 64 with NS = ceil(C / 64)
// class slots per lane, or GW = 32 / 16 for C <= 32 / 16), a wave walks a contiguous pixel range of one image; the loops over the sets
// and over a set's taps are wave-uniform.  The covering-window loops depend on the pixel, so for GW < 64 they diverge between the
// groups of a wave: nothing that crosses lanes sits inside them -- the softmax reductions run once per set, on the complete logit row,
// with every lane active.  The per-set descriptors travel BY VALUE in the kernel argument (MsfSlideSets, 1 KB): no device table, no
// upload, no host synchronisation, so the call can be captured into a hipGraph.
// The tap and window arithmetic is a commented COPY of slide_argmax_confmat_kernel's and msf_argmax_confmat_kernel's, not shared code:
// moving code between these kernels lets the compiler fuse a b + c d differently and changes result bits of the two siblings.
#include "eval_rows.h"

struct MsfSlideSet { const void* p; int64_t ldl; int Hs, Ws, ch, cw, sh, sw, h, w, ny, nx, flip, pad; };
struct MsfSlideSets { MsfSlideSet m[SEGF_MSF_MAX_MAPS]; };

#define MSFS_THREADS 256

// the window grid of one axis (slide_count of eval_slide.hip): n = max(L - c + s - 1, 0) / s + 1 windows, origin of window i = min(i s, L - c)
static inline int msfs_count(int L, int c, int s) { const int d = L - c + s - 1; return (d > 0 ? d : 0) / s + 1; }

// M[s] = the mean over the windows of set `st` that cover the scaled pixel (Y, X) of the bilinear sample of each window's map at the
// local pixel, class cl + 64 s: the arithmetic of slide_argmax_confmat_kernel -- ascending (i, j), fp32 sum in that order, a true IEEE
// division by the cover count.  No lane reads another lane's value: safe inside divergent control flow.
template <typename T, int NS>
__device__ __forceinline__ void window_mean(const MsfSlideSet& st, const T* __restrict__ img0, int Y, int X, int cl, int C, float (&M)[NS]) {
    const int64_t map_elems = (int64_t)st.h * st.w * st.ldl;                 // one window's map
    const bool direct = st.h == st.ch && st.w == st.cw;
    // first window of each axis that reaches the pixel; never past the last window, which ends at the border
    const int i0 = Y >= st.ch ? (Y - st.ch) / st.sh + 1 : 0;
    const int j0 = X >= st.cw ? (X - st.cw) / st.sw + 1 : 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) M[s] = 0.f;
    int cover = 0;
    for (int i = i0; i < st.ny; ++i) {
        const int yo = min(i * st.sh, st.Hs - st.ch);
        if (yo > Y) break;                                       // origins are monotone: no later window covers the pixel
        int y0, y1; float ly;
        if (direct) { y0 = y1 = Y - yo; ly = 0.f; }
        else bilinear_src(Y - yo, st.h, st.ch, 0, y0, y1, ly);
        for (int j = j0; j < st.nx; ++j) {
            const int xo = min(j * st.sw, st.Ws - st.cw);
            if (xo > X) break;
            const T* img = img0 + (int64_t)(i * st.nx + j) * map_elems;
            if (direct) {                                        // same size: the row itself
                const T* r = img + ((int64_t)y0 * st.w + (X - xo)) * st.ldl;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int c = cl + 64 * s;
                    M[s] += ldf<T>(r + (c < C ? c : C - 1));                  // clamped index: every load unconditional
                }
            } else {
                int x0, x1; float lx;
                bilinear_src(X - xo, st.w, st.cw, 0, x0, x1, lx);
                const T* r00 = img + ((int64_t)y0 * st.w + x0) * st.ldl;
                const T* r01 = img + ((int64_t)y0 * st.w + x1) * st.ldl;
                const T* r10 = img + ((int64_t)y1 * st.w + x0) * st.ldl;
                const T* r11 = img + ((int64_t)y1 * st.w + x1) * st.ldl;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int c = cl + 64 * s, ci = c < C ? c : C - 1;
                    M[s] += bilinear_aten(ldf<T>(r00 + ci), ldf<T>(r01 + ci), ldf<T>(r10 + ci), ldf<T>(r11 + ci), ly, lx);
                }
            }
            ++cover;
        }
    }
    const float fn = (float)cover;                               // >= 1: the grid covers every pixel of the scaled image
#pragma unroll
    for (int s = 0; s < NS; ++s) M[s] = __fdiv_rn(M[s], fn);
}

template <typename T, int NS, int GW>
__global__ void __launch_bounds__(MSFS_THREADS) msf_slide_argmax_confmat_kernel(MsfSlideSets sets, int n, int C, int H, int W,
                                                                                 const int64_t* __restrict__ target, int64_t ignore_label,
                                                                                 unsigned long long* __restrict__ mat,
                                                                                 unsigned long long* __restrict__ hist,
                                                                                 int* __restrict__ flag, int64_t* __restrict__ pred_out,
                                                                                 float* __restrict__ prob_out, int64_t ldp) {
    static_assert(GW == 64 || NS == 1, "sub-wave groups hold one class per lane");
    constexpr int G = 64 / GW;                                   // pixels per wave and step
    const int lane = threadIdx.x & 63;
    const int grp = lane / GW, cl = lane - grp * GW;             // this lane's pixel of the step, its class (slot 0)
    const int b = blockIdx.y;
    const int64_t npix = (int64_t)H * W;
    static_assert(MSFS_THREADS == 256, "wave_pixel_range: 4 waves per workgroup");
    int64_t p0, p1;
    wave_pixel_range(npix, p0, p1);
    const int64_t* tg = target ? target + (int64_t)b * npix : nullptr;
    const bool want_all = pred_out != nullptr || prob_out != nullptr;       // every pixel's row is needed, counted or not
    for (int64_t base = p0; base < p1; base += G) {
        const bool live = base + grp < p1;
        const int64_t p = live ? base + grp : p1 - 1;            // a group past the end recomputes the last pixel and writes nothing
        int64_t t = ignore_label;
        if (tg) t = tg[p];
        const bool in_mat = t >= 0 && t < C;
        // counted nowhere (label == ignore_label outside [0, C)) and no output wanted: the pixel is skipped as argmax_confmat_kernel does
        const bool need = live && (want_all || (tg != nullptr && (in_mat || t != ignore_label)));
        if (__builtin_amdgcn_ballot_w64(need) == 0) continue;    // wave-uniform
        const int Y = (int)(p / W), X = (int)(p - (int64_t)Y * W);
        float S[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) S[s] = 0.f;
        for (int k = 0; k < n; ++k) {                            // wave-uniform
            const MsfSlideSet st = sets.m[k];
            const T* img0 = (const T*)st.p + (int64_t)b * st.ny * st.nx * ((int64_t)st.h * st.w * st.ldl);    // window 0 of image b
            float z[NS];
            if (st.Hs == H && st.Ws == W) {                      // same size: the mean at the (mirrored) pixel itself
                window_mean<T, NS>(st, img0, Y, st.flip ? st.Ws - 1 - X : X, cl, C, z);
            } else {
                int y0, y1, x0, x1; float ly, lx;
                bilinear_src(Y, st.Hs, H, 0, y0, y1, ly);
                bilinear_src(X, st.Ws, W, 0, x0, x1, lx);
                // a mirrored set is read at the mirrored tap columns with the SAME weights: exactly the sample of the un-mirrored mean map
                if (st.flip) { x0 = st.Ws - 1 - x0; x1 = st.Ws - 1 - x1; }
                // bilinear_aten(M00, M01, M10, M11, ly, lx), one tap's mean alive at a time: its operations in its order --
                // fma(M11, w11, fma(M10, w10, fma(M00, w00, M01 * w01)))
                const float wy0 = 1.f - ly, wx0 = 1.f - lx;
                float M[NS];
                window_mean<T, NS>(st, img0, y0, x1, cl, C, M);
                const float w01 = __fmul_rn(wy0, lx);
#pragma unroll
                for (int s = 0; s < NS; ++s) z[s] = __fmul_rn(M[s], w01);
                window_mean<T, NS>(st, img0, y0, x0, cl, C, M);
                const float w00 = __fmul_rn(wy0, wx0);
#pragma unroll
                for (int s = 0; s < NS; ++s) z[s] = __fmaf_rn(M[s], w00, z[s]);
                window_mean<T, NS>(st, img0, y1, x0, cl, C, M);
                const float w10 = __fmul_rn(ly, wx0);
#pragma unroll
                for (int s = 0; s < NS; ++s) z[s] = __fmaf_rn(M[s], w10, z[s]);
                window_mean<T, NS>(st, img0, y1, x1, cl, C, M);
                const float w11 = __fmul_rn(ly, lx);
#pragma unroll
                for (int s = 0; s < NS; ++s) z[s] = __fmaf_rn(M[s], w11, z[s]);
            }
            // the set's logit row is complete and the groups of the wave have reconverged: softmax over the group's lanes
            // (max-subtracted, fp32, as msf_argmax_confmat_kernel); empty class slots hold -inf -> exp = 0
#pragma unroll
            for (int s = 0; s < NS; ++s) z[s] = cl + 64 * s < C ? z[s] : -INFINITY;
            float mx = z[0];
#pragma unroll
            for (int s = 1; s < NS; ++s) mx = fmaxf(mx, z[s]);
            mx = grp_max<GW>(mx);
            float e[NS], sum = 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s) { e[s] = __expf(z[s] - mx); sum += e[s]; }
            sum = grp_sum<GW>(sum);
            const float inv = __builtin_amdgcn_rcpf(sum);        // 1 ulp; sum is in [1, C]
#pragma unroll
            for (int s = 0; s < NS; ++s) S[s] += e[s] * inv;
        }
        const int best = grp_argmax<NS, GW>(S, cl, C);           // lowest class index attaining the maximum; 0 on an all-NaN row
        if (need) {
            const int64_t q = (int64_t)b * npix + p;
            if (prob_out) {
#pragma unroll
                for (int s = 0; s < NS; ++s)
                    if (cl + 64 * s < C) prob_out[q * ldp + cl + 64 * s] = S[s];
            }
            if (cl == 0) {
                if (pred_out) pred_out[q] = best;
                if (tg) eval_count(t, best, C, ignore_label, mat, hist, flag);
            }
        }
    }
}

// geom[8 k ..] = Hs, Ws, ch, cw, sh, sw, h, w of set k
static bool msfs_shape_ok(int B, int C, int n, const int* geom, int H, int W) {
    if (n < 1 || n > SEGF_MSF_MAX_MAPS || C < 1 || C > 192 || B < 1 || B > 65535 || H < 1 || W < 1 || !geom) return false;
    for (int k = 0; k < n; ++k) {
        const int* g = geom + 8 * k;
        if (!(g[4] >= 1 && g[4] <= g[2] && g[2] <= g[0] && g[5] >= 1 && g[5] <= g[3] && g[3] <= g[1]) || g[6] < 1 || g[7] < 1) return false;
    }
    return true;
}

extern "C" int segf_msf_slide_supported(int dt, int B, int C, int n, const int* geom, int H, int W) {
    return (dt == SEGF_F32 || dt == SEGF_BF16) && msfs_shape_ok(B, C, n, geom, H, W) ? 1 : 0;
}

extern "C" int segf_msf_slide_argmax_confmat(int dt, int B, int C, int n, void** logits, const int* geom, const int64_t* ldl,
                                             const int* flip, int H, int W, const int64_t* target, int64_t ignore_label, int64_t* mat,
                                             int64_t* hist, int32_t* flag, int64_t* pred_out, float* prob_out, int64_t ldp, void* stream) {
    if (!msfs_shape_ok(B, C, n, geom, H, W) || !logits || !ldl || !flip) return SEGF_ERR_SHAPE;
    if (prob_out && ldp < C) return SEGF_ERR_SHAPE;
    MsfSlideSets sets;
    for (int k = 0; k < SEGF_MSF_MAX_MAPS; ++k) {
        const int j = k < n ? k : 0;                              // unused entries repeat set 0 (never read: the loop stops at n)
        const int* g = geom + 8 * j;
        if (!logits[j] || ldl[j] < C) return SEGF_ERR_SHAPE;
        sets.m[k] = MsfSlideSet{logits[j], ldl[j], g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], msfs_count(g[0], g[2], g[4]),
                                msfs_count(g[1], g[3], g[5]), flip[j] ? 1 : 0, 0};
    }
    if (dt != SEGF_F32 && dt != SEGF_BF16) return SEGF_ERR_DTYPE;
    hipStream_t st = (hipStream_t)stream;
    // a wave owns a contiguous pixel range of one image; ~2048 workgroups in all (8 waves per SIMD in flight cover the tap loads'
    // latency), never more waves than groups of pixels
    const int64_t npix = (int64_t)H * W;
    const int gw = C > 32 ? 64 : (C > 16 ? 32 : 16);
    int64_t nblk = cdiv64(npix, (int64_t)(MSFS_THREADS / 64) * (64 / gw) * 8);
    const int64_t cap = 2048 / B > 16 ? 2048 / B : 16;
    if (nblk > cap) nblk = cap;
    if (nblk < 1) nblk = 1;
    const dim3 grid((unsigned)nblk, (unsigned)B);
    unsigned long long* m = (unsigned long long*)mat;
    unsigned long long* hs = (unsigned long long*)hist;
#define CALL(NS, GW) hipLaunchKernelGGL((msf_slide_argmax_confmat_kernel<T, NS, GW>), grid, dim3(MSFS_THREADS), 0, st, sets, n, C, H, W,   \
                                        target, ignore_label, m, hs, (int*)flag, pred_out, prob_out, ldp)
    SEGF_DISPATCH_DT(dt, T, {
        if (gw == 16) CALL(1, 16);
        else if (gw == 32) CALL(1, 32);
        else if (C <= 64) CALL(1, 64);
        else if (C <= 128) CALL(2, 64);
        else CALL(3, 64);
    })
#undef CALL
    SEGF_CHECK_LAUNCH();
    return 0;
}
