// Sliding-window evaluation: resample + mean over the low-resolution logit maps of overlapping crops, arg max of the mean and both
// confusion matrices, in one kernel (segf_slide_argmax_confmat, include/segfac.h).
//   The published Cityscapes figures of SegFormer (crop 1024, stride 768 over 1024 x 2048) and most ADE20K / VOC configurations
//   (crop 512, stride 341) are sliding-window numbers (mmseg's slide_inference): the model runs on overlapping ch x cw crops, every
//   crop's logits are resized to the crop, the logits of overlapping crops are averaged and the arg max of the mean is scored.  Done
//   with tensors that is one full-resolution [C, ch, cw] fp32 map per window plus a [C, H, W] accumulator and a count map per image.
//   Here a pixel's class row is resampled straight from the low-resolution NHWC rows of every window that covers it (bilinear_src +
//   bilinear_aten, as msf_argmax_confmat_kernel does), added into per-lane fp32 accumulators in window order and divided by the cover
//   count; only the prediction / the counts (and, on request, the mean row) are written.
// Layout of the work: that of eval_msf.hip -- classes on lanes, one GROUP of GW lanes per pixel (GW = 64 with NS = ceil(C / 64) class
// slots per lane, or GW = 32 / 16 for C <= 32 / 16), a wave walks a contiguous pixel range of one image.  The loop over maps is a loop
// over the covering windows: the window grid is regular, so the covering range of an axis is arithmetic on the pixel coordinate (no
// table; the call can be captured), wave-uniform for GW = 64.  Nothing floating-point crosses lanes: two runs give the same bits.
#include "eval_rows.h"

#define SLIDE_THREADS 256

// the window grid of one axis: n = max(L - c + s - 1, 0) / s + 1 windows, origin of window i = min(i s, L - c)
static inline int slide_count(int L, int c, int s) { const int d = L - c + s - 1; return (d > 0 ? d : 0) / s + 1; }

template <typename T, int NS, int GW>
__global__ void __launch_bounds__(SLIDE_THREADS) slide_argmax_confmat_kernel(const T* __restrict__ logits, int64_t ldl, int C, int H, int W,
                                                                              int ch, int cw, int sh, int sw, int ny, int nx, int h, int w,
                                                                              const int64_t* __restrict__ target, int64_t ignore_label,
                                                                              unsigned long long* __restrict__ mat,
                                                                              unsigned long long* __restrict__ hist, int* __restrict__ flag,
                                                                              int64_t* __restrict__ pred_out, float* __restrict__ mean_out,
                                                                              int64_t ldm) {
    static_assert(GW == 64 || NS == 1, "sub-wave groups hold one class per lane");
    constexpr int G = 64 / GW;                                   // pixels per wave and step
    const int lane = threadIdx.x & 63;
    const int grp = lane / GW, cl = lane - grp * GW;             // this lane's pixel of the step, its class (slot 0)
    const int b = blockIdx.y;
    const int64_t npix = (int64_t)H * W;
    static_assert(SLIDE_THREADS == 256, "wave_pixel_range: 4 waves per workgroup");
    int64_t p0, p1;
    wave_pixel_range(npix, p0, p1);
    const int64_t* tg = target ? target + (int64_t)b * npix : nullptr;
    const bool want_all = pred_out != nullptr || mean_out != nullptr;       // every pixel's row is needed, counted or not
    const int64_t map_elems = (int64_t)h * w * ldl;                          // one window's map
    const T* img0 = logits + (int64_t)b * ny * nx * map_elems;               // window 0 of image b
    const bool direct = h == ch && w == cw;
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
        // first window of each axis that reaches the pixel: origins i s (the last one moved back to L - c) and size c give
        // i >= (Y - ch) / sh + 1 for Y >= ch; never past the last window, which ends at the border
        const int i0 = Y >= ch ? (Y - ch) / sh + 1 : 0;
        const int j0 = X >= cw ? (X - cw) / sw + 1 : 0;
        float S[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) S[s] = 0.f;
        int cover = 0;
        for (int i = i0; i < ny; ++i) {
            const int yo = min(i * sh, H - ch);
            if (yo > Y) break;                                   // origins are monotone: no later window covers the pixel
            int y0, y1; float ly;
            if (direct) { y0 = y1 = Y - yo; ly = 0.f; }
            else bilinear_src(Y - yo, h, ch, 0, y0, y1, ly);
            for (int j = j0; j < nx; ++j) {
                const int xo = min(j * sw, W - cw);
                if (xo > X) break;
                const T* img = img0 + (int64_t)(i * nx + j) * map_elems;
                if (direct) {                                    // same size: the row itself
                    const T* r = img + ((int64_t)y0 * w + (X - xo)) * ldl;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int c = cl + 64 * s;
                        S[s] += ldf<T>(r + (c < C ? c : C - 1));              // clamped index: every load unconditional
                    }
                } else {
                    int x0, x1; float lx;
                    bilinear_src(X - xo, w, cw, 0, x0, x1, lx);
                    const T* r00 = img + ((int64_t)y0 * w + x0) * ldl;
                    const T* r01 = img + ((int64_t)y0 * w + x1) * ldl;
                    const T* r10 = img + ((int64_t)y1 * w + x0) * ldl;
                    const T* r11 = img + ((int64_t)y1 * w + x1) * ldl;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int c = cl + 64 * s, ci = c < C ? c : C - 1;
                        S[s] += bilinear_aten(ldf<T>(r00 + ci), ldf<T>(r01 + ci), ldf<T>(r10 + ci), ldf<T>(r11 + ci), ly, lx);
                    }
                }
                ++cover;
            }
        }
        // mean: a true IEEE division (a pixel covered once keeps its sample bit for bit), not v_rcp
        const float fn = (float)cover;
#pragma unroll
        for (int s = 0; s < NS; ++s) S[s] = __fdiv_rn(S[s], fn);
        const int best = grp_argmax<NS, GW>(S, cl, C);           // lowest class index attaining the maximum; 0 on an all-NaN row
        if (need) {
            const int64_t q = (int64_t)b * npix + p;
            if (mean_out) {
#pragma unroll
                for (int s = 0; s < NS; ++s)
                    if (cl + 64 * s < C) mean_out[q * ldm + cl + 64 * s] = S[s];
            }
            if (cl == 0) {
                if (pred_out) pred_out[q] = best;
                if (tg) eval_count(t, best, C, ignore_label, mat, hist, flag);
            }
        }
    }
}

static bool slide_grid_ok(int H, int W, int ch, int cw, int sh, int sw) {
    return sh >= 1 && sh <= ch && ch <= H && sw >= 1 && sw <= cw && cw <= W;
}

static bool slide_shape_ok(int B, int C, int H, int W, int ch, int cw, int sh, int sw, int h, int w) {
    return C >= 1 && C <= 192 && B >= 1 && B <= 65535 && H >= 1 && W >= 1 && h >= 1 && w >= 1 && slide_grid_ok(H, W, ch, cw, sh, sw);
}

extern "C" int segf_slide_grid(int H, int W, int ch, int cw, int sh, int sw, int* ny, int* nx) {
    if (!slide_grid_ok(H, W, ch, cw, sh, sw) || !ny || !nx) return SEGF_ERR_SHAPE;
    *ny = slide_count(H, ch, sh);
    *nx = slide_count(W, cw, sw);
    return 0;
}

extern "C" int segf_slide_supported(int dt, int B, int C, int H, int W, int ch, int cw, int sh, int sw, int h, int w) {
    return (dt == SEGF_F32 || dt == SEGF_BF16) && slide_shape_ok(B, C, H, W, ch, cw, sh, sw, h, w) ? 1 : 0;
}

extern "C" int segf_slide_argmax_confmat(int dt, int B, int C, int H, int W, int ch, int cw, int sh, int sw, int h, int w,
                                         const void* logits, int64_t ldl, const int64_t* target, int64_t ignore_label, int64_t* mat,
                                         int64_t* hist, int32_t* flag, int64_t* pred_out, float* mean_out, int64_t ldm, void* stream) {
    if (!slide_shape_ok(B, C, H, W, ch, cw, sh, sw, h, w) || !logits || ldl < C) return SEGF_ERR_SHAPE;
    if (mean_out && ldm < C) return SEGF_ERR_SHAPE;
    if (dt != SEGF_F32 && dt != SEGF_BF16) return SEGF_ERR_DTYPE;
    hipStream_t st = (hipStream_t)stream;
    const int ny = slide_count(H, ch, sh), nx = slide_count(W, cw, sw);
    // a wave owns a contiguous pixel range of one image; ~2048 workgroups in all (8 waves per SIMD in flight cover the tap loads'
    // latency), never more waves than groups of pixels
    const int64_t npix = (int64_t)H * W;
    const int gw = C > 32 ? 64 : (C > 16 ? 32 : 16);
    int64_t nblk = cdiv64(npix, (int64_t)(SLIDE_THREADS / 64) * (64 / gw) * 8);
    const int64_t cap = 2048 / B > 16 ? 2048 / B : 16;
    if (nblk > cap) nblk = cap;
    if (nblk < 1) nblk = 1;
    const dim3 grid((unsigned)nblk, (unsigned)B);
    unsigned long long* m = (unsigned long long*)mat;
    unsigned long long* hs = (unsigned long long*)hist;
#define CALL(NS, GW) hipLaunchKernelGGL((slide_argmax_confmat_kernel<T, NS, GW>), grid, dim3(SLIDE_THREADS), 0, st, (const T*)logits, ldl, \
                                        C, H, W, ch, cw, sh, sw, ny, nx, h, w, target, ignore_label, m, hs, (int*)flag, pred_out,         \
                                        mean_out, ldm)
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
