// Multi-scale + flip evaluation: resample + softmax + sum over n low-resolution logit maps, arg max of the summed probabilities and
// both confusion matrices, in one kernel (segf_msf_argmax_confmat, include/segfac.h).
//   The published mIoU figures of SegFormer / UPerNet / DeepLabV3 are "MSF" numbers: the model runs on the image at scales 0.5 ...
//   1.75, each also mirrored, every output is resized to the label size and softmaxed, the 2 S probability maps are summed and the
//   arg max of the sum is scored.  Done with tensors that is 2 S full-resolution [C, H, W] fp32 maps plus an accumulator per image
//   (157 MB each at C = 150, 512^2).  Here a pixel's class row of every map is resampled straight from the low-resolution NHWC rows
//   (the arithmetic of the generic path of pixel_logits<T, NS, true> in loss_geom.h: bilinear_src + bilinear_aten), softmaxed across the
//   lanes and added into per-lane fp32 accumulators; only the prediction / the counts (and, on request, the summed row) are written.
// Layout of the work: classes on lanes, one GROUP of GW lanes per pixel -- GW = 64 with NS = ceil(C / 64) class slots per lane, or,
// for C <= 32 / C <= 16, GW = 32 / 16 so that a wave carries 2 / 4 pixels (a 19-class row would otherwise leave 45 of 64 lanes idle
// through every instruction).  A wave walks a contiguous pixel range of one image and loops over the maps per pixel, in map order:
// S = p_0 + p_1 + ... is the same sequence of fp32 additions on every run, and nothing floating-point is accumulated across lanes
// or workgroups except the fixed-shape butterfly of the softmax denominator -- two runs give the same bits.  Counts are integer
// atomics (eval_count of eval_rows.h).  The per-map descriptors travel BY VALUE in the kernel argument (MsfMaps, 512 bytes): no
// device table, no upload, no host synchronisation, so the call can be captured into a hipGraph.
#include "eval_rows.h"

struct MsfMap { const void* p; int64_t ldl; int h, w, flip, pad; };
struct MsfMaps { MsfMap m[SEGF_MSF_MAX_MAPS]; };

#define MSF_THREADS 256

template <typename T, int NS, int GW>
__global__ void __launch_bounds__(MSF_THREADS) msf_argmax_confmat_kernel(MsfMaps maps, int n, int C, int H, int W,
                                                                          const int64_t* __restrict__ target, int64_t ignore_label,
                                                                          unsigned long long* __restrict__ mat,
                                                                          unsigned long long* __restrict__ hist, int* __restrict__ flag,
                                                                          int64_t* __restrict__ pred_out, float* __restrict__ prob_out,
                                                                          int64_t ldp) {
    static_assert(GW == 64 || NS == 1, "sub-wave groups hold one class per lane");
    constexpr int G = 64 / GW;                                   // pixels per wave and step
    const int lane = threadIdx.x & 63;
    const int grp = lane / GW, cl = lane - grp * GW;             // this lane's pixel of the step, its class (slot 0)
    const int b = blockIdx.y;
    const int64_t npix = (int64_t)H * W;
    static_assert(MSF_THREADS == 256, "wave_pixel_range: 4 waves per workgroup");
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
        for (int k = 0; k < n; ++k) {
            const MsfMap mp = maps.m[k];
            const T* img = (const T*)mp.p + (int64_t)b * mp.h * mp.w * mp.ldl;
            float z[NS];
            if (mp.h == H && mp.w == W) {                        // same size: the row itself
                const int xs = mp.flip ? mp.w - 1 - X : X;
                const T* r = img + ((int64_t)Y * mp.w + xs) * mp.ldl;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int c = cl + 64 * s;
                    const float v = ldf<T>(r + (c < C ? c : C - 1));       // clamped index: every load unconditional
                    z[s] = c < C ? v : -INFINITY;
                }
            } else {
                int y0, y1, x0, x1; float ly, lx;
                bilinear_src(Y, mp.h, H, 0, y0, y1, ly);
                bilinear_src(X, mp.w, W, 0, x0, x1, lx);
                // a mirrored map is read at the mirrored tap columns with the SAME weights: exactly the sample of the un-mirrored map
                if (mp.flip) { x0 = mp.w - 1 - x0; x1 = mp.w - 1 - x1; }
                const T* r00 = img + ((int64_t)y0 * mp.w + x0) * mp.ldl;
                const T* r01 = img + ((int64_t)y0 * mp.w + x1) * mp.ldl;
                const T* r10 = img + ((int64_t)y1 * mp.w + x0) * mp.ldl;
                const T* r11 = img + ((int64_t)y1 * mp.w + x1) * mp.ldl;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int c = cl + 64 * s, ci = c < C ? c : C - 1;
                    const float v = bilinear_aten(ldf<T>(r00 + ci), ldf<T>(r01 + ci), ldf<T>(r10 + ci), ldf<T>(r11 + ci), ly, lx);
                    z[s] = c < C ? v : -INFINITY;
                }
            }
            // softmax over the group's lanes (max-subtracted, fp32); empty class slots hold -inf -> exp = 0
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

static bool msf_shape_ok(int B, int C, int n, const int* hw, int H, int W) {
    if (n < 1 || n > SEGF_MSF_MAX_MAPS || C < 1 || C > 192 || B < 1 || B > 65535 || H < 1 || W < 1 || !hw) return false;
    for (int k = 0; k < n; ++k)
        if (hw[2 * k] < 1 || hw[2 * k + 1] < 1) return false;
    return true;
}

extern "C" int segf_msf_supported(int dt, int B, int C, int n, const int* hw, int H, int W) {
    return (dt == SEGF_F32 || dt == SEGF_BF16) && msf_shape_ok(B, C, n, hw, H, W) ? 1 : 0;
}

extern "C" int segf_msf_argmax_confmat(int dt, int B, int C, int n, void** logits, const int* hw, const int64_t* ldl, const int* flip,
                                       int H, int W, const int64_t* target, int64_t ignore_label, int64_t* mat, int64_t* hist,
                                       int32_t* flag, int64_t* pred_out, float* prob_out, int64_t ldp, void* stream) {
    if (!msf_shape_ok(B, C, n, hw, H, W) || !logits || !ldl || !flip) return SEGF_ERR_SHAPE;
    if (prob_out && ldp < C) return SEGF_ERR_SHAPE;
    MsfMaps maps;
    for (int k = 0; k < SEGF_MSF_MAX_MAPS; ++k) {
        const int j = k < n ? k : 0;                              // unused entries repeat map 0 (never read: the loop stops at n)
        if (ldl[j] < C) return SEGF_ERR_SHAPE;
        maps.m[k] = MsfMap{logits[j], ldl[j], hw[2 * j], hw[2 * j + 1], flip[j] ? 1 : 0, 0};
    }
    if (dt != SEGF_F32 && dt != SEGF_BF16) return SEGF_ERR_DTYPE;
    hipStream_t st = (hipStream_t)stream;
    // a wave owns a contiguous pixel range of one image; ~2048 workgroups in all (8 waves per SIMD in flight cover the tap loads'
    // latency), never more waves than groups of pixels
    const int64_t npix = (int64_t)H * W;
    const int gw = C > 32 ? 64 : (C > 16 ? 32 : 16);
    int64_t nblk = cdiv64(npix, (int64_t)(MSF_THREADS / 64) * (64 / gw) * 8);
    const int64_t cap = 2048 / B > 16 ? 2048 / B : 16;
    if (nblk > cap) nblk = cap;
    if (nblk < 1) nblk = 1;
    const dim3 grid((unsigned)nblk, (unsigned)B);
    unsigned long long* m = (unsigned long long*)mat;
    unsigned long long* hs = (unsigned long long*)hist;
#define CALL(NS, GW) hipLaunchKernelGGL((msf_argmax_confmat_kernel<T, NS, GW>), grid, dim3(MSF_THREADS), 0, st, maps, n, C, H, W, target, \
                                        ignore_label, m, hs, (int*)flag, pred_out, prob_out, ldp)
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
