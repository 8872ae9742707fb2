// Device-side input pipeline: the reference's per-sample CPU transforms as gfx950 kernels over decoded
// uint8 images that already live in HBM.
//   train: ExtRandomCrop -> ExtColorJitter -> ExtRandomHorizontalFlip -> ExtToTensor -> ExtNormalize
//          (datasets/build_datasets.py:14-22; datasets/extra_transform.py:319-392, 426-509, 196-214, 259-281, 288-313)
//   train with scale augmentation: ExtRandomScale -> ExtRandomCrop(pad_if_needed) in front of the same stack
//          (extra_transform.py:75-96, 319-392), the resize evaluated for the crop window only (segf_input_train_scaled)
//   val:   ExtResize -> ExtToTensor -> ExtNormalize                      (build_datasets.py:24-29; extra_transform.py:395-419)
// plus the label table + widening of the dataset classes (datasets/ade.py:122-124, cityscapes.py:159, coco_stuff.py:95-100).
// The arithmetic is Pillow's (the transforms act on PIL images): ImagingBlend in C float with truncation / clipping, rgb2l =
// (R*19595 + G*38470 + B*7471 + 0x8000) >> 16, the contrast mean int(sum / count + 0.5) in double, ImagingResample's two
// 22-bit fixed-point passes, ImagingScaleAffine's accumulated nearest index -- all integer / uint8 results are bit-exact, and
// the float tail ((u8 / 255) / 255 - mean) / std (quirk Q11: the second / 255) is four IEEE float32 operations, evaluated once
// per (channel, byte value) into an LDS table.  This file is compiled with -ffp-contract=off: a fused multiply-add anywhere in
// it would change results.  The random draws are made on the host in the reference's order (transforms.py); kernels only see
// their values.  HBM-bound: 4 bytes read, 20 bytes written per output pixel (fp32 NCHW image + int64 label).
#include "common.h"

namespace {

constexpr int OP_BRIGHTNESS = 1, OP_CONTRAST = 2, OP_SATURATION = 3;

__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Blend.c: (UINT8)(deg + alpha * (v - deg)); outside [0, 1] the value is clipped first.  One formula covers alpha == 0 / 1 (exact)
// and the interpolating range (the result lies between deg and v, so the clip never acts there).
__device__ __forceinline__ int blend1(int deg, int v, float a) {
    const float t = __fadd_rn((float)deg, __fmul_rn(a, (float)(v - deg)));
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// applies the jitter operations of `order` (2 bits per step, 0 = end) to one pixel; stops BEFORE the contrast step when
// `until_contrast` (the luma sum that defines the contrast mean is taken over the image at that point)
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ void jitter(int& r, int& g, int& b, int order, const float (&f)[3], int cmean) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int op = (order >> (2 * k)) & 3;
        if (op == 0) break;
        if (op == OP_CONTRAST && UNTIL_CONTRAST) break;
        const int l = luma(r, g, b);
        const int dr = op == OP_BRIGHTNESS ? 0 : (op == OP_CONTRAST ? cmean : l);
        r = blend1(dr, r, f[k]); g = blend1(dr, g, f[k]); b = blend1(dr, b, f[k]);
    }
}

__device__ __forceinline__ bool has_contrast(int order) {
    return (order & 3) == OP_CONTRAST || ((order >> 2) & 3) == OP_CONTRAST || ((order >> 4) & 3) == OP_CONTRAST;
}

// PX consecutive OUTPUT pixels (x0 .. x0+PX-1 of output row y) of a sample: source pixel of output x is
// (top + y, left + (flip ? W-1-x : x)); outside the source image the crop reads 0 (Image.crop).  The fast path fetches the 12
// image bytes / 4 label bytes of an in-range run as aligned dwords + v_alignbyte (the run starts at an arbitrary byte).
template <int PX, bool WANT_LBL>
__device__ __forceinline__ void load_run(const segf_input_sample& s, int y, int x0, int W, int (&rgb)[PX][3], int (&lb)[PX]) {
    const int sy = s.top + y;
    const int cs = s.flip ? s.left + W - PX - x0 : s.left + x0;          // first SOURCE column of the run (ascending)
    int src[PX][3], sl[PX];
    if (PX == 4 && sy < s.src_h && cs + 4 <= s.src_w) {
        const uintptr_t p = (uintptr_t)s.img + (uintptr_t)sy * s.img_stride + (uintptr_t)cs * 3;
        const uintptr_t base = p & ~(uintptr_t)3, last = (p + 11) & ~(uintptr_t)3;
        const unsigned sh = (unsigned)(p & 3);
        const unsigned w0 = *(const unsigned*)base, w1 = *(const unsigned*)(base + 4), w2 = *(const unsigned*)(base + 8);
        const unsigned w3 = *(const unsigned*)(base + 12 <= last ? base + 12 : last);     // never past the dword of the last byte
        const unsigned d0 = __builtin_amdgcn_alignbyte(w1, w0, sh), d1 = __builtin_amdgcn_alignbyte(w2, w1, sh),
                       d2 = __builtin_amdgcn_alignbyte(w3, w2, sh);
        src[0][0] = d0 & 255; src[0][1] = (d0 >> 8) & 255; src[0][2] = (d0 >> 16) & 255;
        src[1][0] = d0 >> 24; src[1][1] = d1 & 255; src[1][2] = (d1 >> 8) & 255;
        src[2][0] = (d1 >> 16) & 255; src[2][1] = d1 >> 24; src[2][2] = d2 & 255;
        src[3][0] = (d2 >> 8) & 255; src[3][1] = (d2 >> 16) & 255; src[3][2] = d2 >> 24;
        if (WANT_LBL) {
            const uintptr_t q = (uintptr_t)s.lbl + (uintptr_t)sy * s.lbl_stride + (uintptr_t)cs;
            const uintptr_t qb = q & ~(uintptr_t)3, ql = (q + 3) & ~(uintptr_t)3;
            const unsigned l0 = *(const unsigned*)qb, l1 = *(const unsigned*)(qb + 4 <= ql ? qb + 4 : ql);
            const unsigned d = __builtin_amdgcn_alignbyte(l1, l0, (unsigned)(q & 3));
            sl[0] = d & 255; sl[1] = (d >> 8) & 255; sl[2] = (d >> 16) & 255; sl[3] = d >> 24;
        }
    } else {
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const int sx = cs + k;
            const bool in = sy < s.src_h && sx < s.src_w && sx >= 0;
            const uint8_t* p = s.img + (int64_t)(in ? sy : 0) * s.img_stride + (int64_t)(in ? sx : 0) * 3;
            const int r = p[0], g = p[1], b = p[2];
            src[k][0] = in ? r : 0; src[k][1] = in ? g : 0; src[k][2] = in ? b : 0;
            if (WANT_LBL) {
                const int l = s.lbl[(int64_t)(in ? sy : 0) * s.lbl_stride + (in ? sx : 0)];
                sl[k] = in ? l : 0;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const int j = s.flip ? PX - 1 - k : k;
        rgb[k][0] = src[j][0]; rgb[k][1] = src[j][1]; rgb[k][2] = src[j][2];
        lb[k] = WANT_LBL ? sl[j] : 0;
    }
}

// lsum[b] = sum over the crop of luma(pixel after the jitter steps that precede the contrast step): ImageStat.Stat(convert('L')).sum
template <int PX>
__global__ void __launch_bounds__(256) input_lsum_kernel(const segf_input_sample* __restrict__ samples, int H, int W,
                                                         unsigned long long* __restrict__ lsum) {
    const segf_input_sample s = samples[blockIdx.y];
    if (!has_contrast(s.order)) return;
    const int runs_per_row = W / PX, total = H * runs_per_row;
    const float f[3] = {s.factor[0], s.factor[1], s.factor[2]};
    unsigned acc = 0;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int y = idx / runs_per_row, x0 = (idx - y * runs_per_row) * PX;
        int rgb[PX][3], lb[PX];
        load_run<PX, false>(s, y, x0, W, rgb, lb);
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            jitter<true>(rgb[k][0], rgb[k][1], rgb[k][2], s.order, f, 0);
            acc += (unsigned)luma(rgb[k][0], rgb[k][1], rgb[k][2]);
        }
    }
    unsigned long long a64 = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a64 += __shfl_xor(a64, o, 64);
    if ((threadIdx.x & 63) == 0 && a64) atomicAdd(&lsum[blockIdx.y], a64);     // integer sum: order-independent, exact
}

// the float tail of one (channel, byte value): ExtToTensor's v / 255, ExtNormalize's / 255 again, (t - mean) / std
__device__ __forceinline__ float norm_value(int v, float mean, float sd) {
    return __fdiv_rn(__fsub_rn(__fdiv_rn(__fdiv_rn((float)v, 255.f), 255.f), mean), sd);
}

template <int PX>
__global__ void __launch_bounds__(256) input_train_kernel(const segf_input_sample* __restrict__ samples, int H, int W,
                                                          const unsigned long long* __restrict__ lsum,
                                                          const float* __restrict__ mean, const float* __restrict__ stdv,
                                                          const int64_t* __restrict__ lut, float* __restrict__ out_img,
                                                          int64_t* __restrict__ out_lbl) {
    __shared__ float nrm[3][256];
    __shared__ int64_t llut[256];
    for (int i = threadIdx.x; i < 768; i += 256) nrm[i >> 8][i & 255] = norm_value(i & 255, mean[i >> 8], stdv[i >> 8]);
    llut[threadIdx.x] = lut ? lut[threadIdx.x] : (int64_t)threadIdx.x;
    const int b = blockIdx.y;
    const segf_input_sample s = samples[b];
    // ImageEnhance.Contrast: mean = int(sum / count + 0.5), Python floats = IEEE doubles
    const int cmean = has_contrast(s.order) ? (int)((double)lsum[b] / (double)((int64_t)H * W) + 0.5) : 0;
    const float f[3] = {s.factor[0], s.factor[1], s.factor[2]};
    __syncthreads();
    const int runs_per_row = W / PX, total = H * runs_per_row;
    const int64_t plane = (int64_t)H * W;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int y = idx / runs_per_row, x0 = (idx - y * runs_per_row) * PX;
        int rgb[PX][3], lb[PX];
        load_run<PX, true>(s, y, x0, W, rgb, lb);
        float o[3][PX];
        int64_t ol[PX];
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            jitter<false>(rgb[k][0], rgb[k][1], rgb[k][2], s.order, f, cmean);
            o[0][k] = nrm[0][rgb[k][0]]; o[1][k] = nrm[1][rgb[k][1]]; o[2][k] = nrm[2][rgb[k][2]];
            ol[k] = llut[lb[k]];
        }
        const int64_t pix = (int64_t)y * W + x0;
        float* oi = out_img + (int64_t)b * 3 * plane + pix;
        int64_t* olp = out_lbl + (int64_t)b * plane + pix;
        if (PX == 4) {
#pragma unroll
            for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(oi + c * plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
            *reinterpret_cast<longlong2*>(olp) = make_longlong2(ol[0], ol[1]);
            *reinterpret_cast<longlong2*>(olp + 2) = make_longlong2(ol[2], ol[3]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) oi[c * plane] = o[c][0];
            olp[0] = ol[0];
        }
    }
}

// ---- validation: Pillow's resize ----------------------------------------------------------------------------------------------
constexpr int PRECISION_BITS = 32 - 8 - 2;

__host__ __device__ inline int resample_ksize(int in_size, int out_size) {
    double fs = (double)in_size / (double)out_size;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(fs) * 2 + 1;
}

// Resample.c precompute_coeffs + normalize_coeffs_8bpc (bilinear filter, support 1) for output index xx
// -> bounds2[0..1] = (first tap, tap count), kk[0..ksize) = this output index' own coefficients
__device__ void coeffs_at(int xx, int in_size, int out_size, int ksize, int* __restrict__ bounds2, int* __restrict__ kk) {
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs, ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        double a = (x + xmin - center + 0.5) * ss;
        if (a < 0.0) a = -a;
        ww += a < 1.0 ? 1.0 - a : 0.0;
    }
    for (int x = 0; x < ksize; ++x) {
        double w = 0.0;
        if (x < xmax) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            w = a < 1.0 ? 1.0 - a : 0.0;
            if (ww != 0.0) w /= ww;
        }
        kk[x] = w < 0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
    }
    bounds2[0] = xmin;
    bounds2[1] = xmax;
}
__device__ void coeffs_for(int xx, int in_size, int out_size, int ksize, int* __restrict__ bounds, int* __restrict__ kk) {
    coeffs_at(xx, in_size, out_size, ksize, bounds + 2 * xx, kk + (int64_t)xx * ksize);
}

// Geometry.c ImagingScaleAffine (nearest): xo = a * 0.5; per output pixel xin = (int)xo; xo += a  (accumulated in double)
__device__ void nearest_table(int n_in, int n_out, int* __restrict__ tab) {
    const double a = (double)n_in / (double)n_out;
    double xo = a * 0.5;
    for (int i = 0; i < n_out; ++i) {
        int v = (int)xo;
        tab[i] = v < 0 ? 0 : (v >= n_in ? n_in - 1 : v);
        xo += a;
    }
}

struct ValTables { int *hb, *hk, *vb, *vk, *nx, *ny; uint8_t* tmp; int ksw, ksh; };

__host__ __device__ inline int64_t val_tables(void* ws, int src_h, int src_w, int out_h, int out_w, ValTables* t) {
    const int ksw = resample_ksize(src_w, out_w), ksh = resample_ksize(src_h, out_h);
    int64_t n = 0;
    int* base = (int*)ws;
    int* hb = base + n; n += 2 * (int64_t)out_w;
    int* hk = base + n; n += (int64_t)out_w * ksw;
    int* vb = base + n; n += 2 * (int64_t)out_h;
    int* vk = base + n; n += (int64_t)out_h * ksh;
    int* nx = base + n; n += out_w;
    int* ny = base + n; n += out_h;
    n = (n + 3) & ~(int64_t)3;
    if (t) { t->hb = hb; t->hk = hk; t->vb = vb; t->vk = vk; t->nx = nx; t->ny = ny; t->tmp = (uint8_t*)(base + n); t->ksw = ksw; t->ksh = ksh; }
    return n * 4 + (int64_t)src_h * out_w * 3;
}

__global__ void __launch_bounds__(256) input_val_tables_kernel(int src_h, int src_w, int out_h, int out_w, ValTables t) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < out_w) coeffs_for(g, src_w, out_w, t.ksw, t.hb, t.hk);
    if (g < out_h) coeffs_for(g, src_h, out_h, t.ksh, t.vb, t.vk);
    if (g == 0) nearest_table(src_w, out_w, t.nx);
    if (g == 1) nearest_table(src_h, out_h, t.ny);
}

// horizontal pass: tmp[y][xx][c] = clip8((2^21 + sum_k src[y][xmin + k][c] * coef[xx][k]) >> 22)
__global__ void __launch_bounds__(256) input_val_hpass_kernel(const uint8_t* __restrict__ img, int64_t img_stride, int src_h, int out_w,
                                                              ValTables t) {
    const int64_t total = (int64_t)src_h * out_w;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int y = (int)(idx / out_w), xx = (int)(idx - (int64_t)y * out_w);
        const int xmin = t.hb[2 * xx], n = t.hb[2 * xx + 1];
        const int* k = t.hk + (int64_t)xx * t.ksw;
        const uint8_t* p = img + (int64_t)y * img_stride + (int64_t)xmin * 3;
        int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
        for (int x = 0; x < n; ++x) { const int kv = k[x]; s0 += p[3 * x] * kv; s1 += p[3 * x + 1] * kv; s2 += p[3 * x + 2] * kv; }
        uint8_t* o = t.tmp + idx * 3;
        s0 >>= PRECISION_BITS; s1 >>= PRECISION_BITS; s2 >>= PRECISION_BITS;
        o[0] = (uint8_t)(s0 < 0 ? 0 : (s0 > 255 ? 255 : s0));
        o[1] = (uint8_t)(s1 < 0 ? 0 : (s1 > 255 ? 255 : s1));
        o[2] = (uint8_t)(s2 < 0 ? 0 : (s2 > 255 ? 255 : s2));
    }
}

// vertical pass + float tail + nearest-resized label through the table
__global__ void __launch_bounds__(256) input_val_vpass_kernel(const uint8_t* __restrict__ lbl, int64_t lbl_stride, int out_h, int out_w,
                                                              ValTables t, const float* __restrict__ mean, const float* __restrict__ stdv,
                                                              const int64_t* __restrict__ lut, float* __restrict__ out_img,
                                                              int64_t* __restrict__ out_lbl) {
    __shared__ float nrm[3][256];
    for (int i = threadIdx.x; i < 768; i += 256) nrm[i >> 8][i & 255] = norm_value(i & 255, mean[i >> 8], stdv[i >> 8]);
    __syncthreads();
    const int64_t total = (int64_t)out_h * out_w;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int yy = (int)(idx / out_w), xx = (int)(idx - (int64_t)yy * out_w);
        const int ymin = t.vb[2 * yy], n = t.vb[2 * yy + 1];
        const int* k = t.vk + (int64_t)yy * t.ksh;
        const uint8_t* p = t.tmp + ((int64_t)ymin * out_w + xx) * 3;
        int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
        for (int y = 0; y < n; ++y) {
            const int kv = k[y];
            const uint8_t* q = p + (int64_t)y * out_w * 3;
            s0 += q[0] * kv; s1 += q[1] * kv; s2 += q[2] * kv;
        }
        s0 >>= PRECISION_BITS; s1 >>= PRECISION_BITS; s2 >>= PRECISION_BITS;
        s0 = s0 < 0 ? 0 : (s0 > 255 ? 255 : s0); s1 = s1 < 0 ? 0 : (s1 > 255 ? 255 : s1); s2 = s2 < 0 ? 0 : (s2 > 255 ? 255 : s2);
        out_img[idx] = nrm[0][s0]; out_img[total + idx] = nrm[1][s1]; out_img[2 * total + idx] = nrm[2][s2];
        const int l = lbl[(int64_t)t.ny[yy] * lbl_stride + t.nx[xx]];
        out_lbl[idx] = lut ? lut[l] : (int64_t)l;
    }
}

// ---- training with scale augmentation: ExtRandomScale -> ExtRandomCrop(pad_if_needed) computed for the crop window only -----------
// nearest_table's entry `idx` alone: the same chain of double additions from output index 0 (Pillow's bits), nothing stored on the way.
// The first `uniform` (<= idx) of them are counted by a value that is the same for the whole workgroup: scalar loop control, no
// divergence; only the remainder (< 256 for neighbouring lanes) differs by lane.
__device__ int nearest_at(int n_in, int n_out, int idx, int uniform) {
    const double a = (double)n_in / (double)n_out;
    double xo = a * 0.5;
#pragma unroll 8
    for (int i = 0; i < uniform; ++i) xo += a;
    for (int i = uniform; i < idx; ++i) xo += a;
    const int v = (int)xo;
    return v < 0 ? 0 : (v >= n_in ? n_in - 1 : v);
}

// Workspace of segf_input_train_scaled, every part 16-byte aligned: the plain records and luma sums that the unchanged train kernels
// read, the scaled records, per sample the tables of its W crop columns and H crop rows ([2W] column bounds, [W][kmax] column
// coefficients, [2H] row bounds, [H][kmax] row coefficients, [W] + [H] nearest source indices), and the staged uint8 crops.
struct ScaledWs {
    segf_input_sample* recs; unsigned long long* lsum; segf_input_scaled_sample* srecs; int* tabs; uint8_t *img, *lbl;
    int64_t per;                                                          // ints of one sample's tables
};

inline int64_t scaled_ws(void* ws, int B, int H, int W, int kmax, ScaledWs* t) {
    auto up16 = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
    const int64_t per = ((int64_t)(W + H) * (3 + kmax) + 3) & ~(int64_t)3;
    const int64_t o_recs = 0, o_lsum = o_recs + up16((int64_t)B * sizeof(segf_input_sample)), o_srecs = o_lsum + up16((int64_t)B * 8),
                  o_tabs = o_srecs + up16((int64_t)B * sizeof(segf_input_scaled_sample)), o_img = o_tabs + (int64_t)B * per * 4,
                  o_lbl = o_img + up16((int64_t)B * H * W * 3), end = o_lbl + up16((int64_t)B * H * W);
    if (t) {
        uint8_t* p = (uint8_t*)ws;
        t->recs = (segf_input_sample*)(p + o_recs); t->lsum = (unsigned long long*)(p + o_lsum);
        t->srecs = (segf_input_scaled_sample*)(p + o_srecs); t->tabs = (int*)(p + o_tabs); t->img = p + o_img; t->lbl = p + o_lbl;
        t->per = per;
    }
    return end;
}

struct ScaledTabs { int *hb, *hk, *vb, *vk, *nx, *ny; };
__device__ __forceinline__ ScaledTabs scaled_tabs(const ScaledWs& t, int b, int H, int W, int kmax) {
    int* p = t.tabs + (int64_t)b * t.per;
    ScaledTabs r;
    r.hb = p; r.hk = r.hb + 2 * W; r.vb = r.hk + (int64_t)W * kmax; r.vk = r.vb + 2 * H; r.nx = r.vk + (int64_t)H * kmax; r.ny = r.nx + W;
    return r;
}

// one thread per crop column and crop row of a sample (grid.y = sample): crop column x is resized column left + x; outside the resized
// image it has no taps.  Thread 0 also writes the plain record through which the train kernels read the staged crop.
__global__ void __launch_bounds__(256) input_scale_tables_kernel(int H, int W, int kmax, ScaledWs t) {
    const int b = blockIdx.y, g = blockIdx.x * 256 + threadIdx.x;
    const segf_input_scaled_sample s = t.srecs[b];
    const ScaledTabs tb = scaled_tabs(t, b, H, W, kmax);
    if (g < W) {
        const int rx = s.left + g, first = s.left + (int)blockIdx.x * 256;     // first: resized column of this workgroup's lane 0
        int* hb = tb.hb + 2 * g;
        if (rx >= 0 && rx < s.res_w) {
            coeffs_at(rx, s.src_w, s.res_w, resample_ksize(s.src_w, s.res_w), hb, tb.hk + (int64_t)g * kmax);
            tb.nx[g] = nearest_at(s.src_w, s.res_w, rx, first < 0 ? 0 : first);
        } else {
            hb[0] = 0; hb[1] = 0;
            tb.nx[g] = 0;
        }
    }
    if (g < H) {
        const int ry = s.top + g, first_y = s.top + (int)blockIdx.x * 256;
        int* vb = tb.vb + 2 * g;
        if (ry >= 0 && ry < s.res_h) {
            coeffs_at(ry, s.src_h, s.res_h, resample_ksize(s.src_h, s.res_h), vb, tb.vk + (int64_t)g * kmax);
            tb.ny[g] = nearest_at(s.src_h, s.res_h, ry, first_y < 0 ? 0 : first_y);
        } else {
            vb[0] = 0; vb[1] = 0;
            tb.ny[g] = 0;
        }
    }
    if (g == 0) {
        segf_input_sample r;
        r.img = t.img + (int64_t)b * H * W * 3; r.lbl = t.lbl + (int64_t)b * H * W;
        r.img_stride = (int64_t)W * 3; r.lbl_stride = W;
        r.src_h = H; r.src_w = W; r.top = 0; r.left = 0;
        r.flip = s.flip; r.order = s.order;
        r.factor[0] = s.factor[0]; r.factor[1] = s.factor[1]; r.factor[2] = s.factor[2];
        r.reserved = 0;
        t.recs[b] = r;
    }
}

__device__ __forceinline__ int clip8(int v) { v >>= PRECISION_BITS; return v < 0 ? 0 : (v > 255 ? 255 : v); }

// PX consecutive crop pixels per thread -> the staged uint8 crop.  A pixel inside the resized image is ImagingResample's vertical pass
// over the horizontal-pass values of its (at most kmax) source rows, each of those formed here from its (at most kmax) source pixels
// and rounded / clipped to uint8 as Pillow's intermediate image is; outside, the pad fill.  The tap loops are counted: a form with
// the horizontal taps unrolled to a fixed 3 / 5 / 7 (absent taps re-reading tap 0 with coefficient 0) measured 1.3 - 1.55 x SLOWER --
// the kernel is bound by the number of byte loads it issues, not by their latency.
template <int PX>
__global__ void __launch_bounds__(256) input_scale_crop_kernel(int H, int W, int kmax, ScaledWs t) {
    const int b = blockIdx.y;
    const segf_input_scaled_sample s = t.srecs[b];
    const ScaledTabs tb = scaled_tabs(t, b, H, W, kmax);
    uint8_t* oimg = t.img + (int64_t)b * H * W * 3;
    uint8_t* olbl = t.lbl + (int64_t)b * H * W;
    const int runs_per_row = W / PX, total = H * runs_per_row;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int y = idx / runs_per_row, x0 = (idx - y * runs_per_row) * PX;
        const int ry = s.top + y;
        int v[PX][3], l[PX];
#pragma unroll
        for (int k = 0; k < PX; ++k) { v[k][0] = 0; v[k][1] = 0; v[k][2] = 0; l[k] = s.label_fill & 255; }
        if (ry >= 0 && ry < s.res_h) {
            const int ymin = tb.vb[2 * y], nrow = tb.vb[2 * y + 1];
            const int* kv = tb.vk + (int64_t)y * kmax;
            const uint8_t* lrow = s.lbl + (int64_t)tb.ny[y] * s.lbl_stride;
            int xmin[PX], ncol[PX], acc[PX][3];
            bool in[PX];
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                const int rx = s.left + x0 + k;
                in[k] = rx >= 0 && rx < s.res_w;
                xmin[k] = tb.hb[2 * (x0 + k)]; ncol[k] = in[k] ? tb.hb[2 * (x0 + k) + 1] : 0;
                acc[k][0] = acc[k][1] = acc[k][2] = 1 << (PRECISION_BITS - 1);
            }
            for (int j = 0; j < nrow; ++j) {
                const uint8_t* prow = s.img + (int64_t)(ymin + j) * s.img_stride;
                const int kvj = kv[j];
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const int* kh = tb.hk + (int64_t)(x0 + k) * kmax;
                    const uint8_t* p = prow + (int64_t)xmin[k] * 3;
                    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
                    for (int i = 0; i < ncol[k]; ++i) { const int c = kh[i]; s0 += p[3 * i] * c; s1 += p[3 * i + 1] * c; s2 += p[3 * i + 2] * c; }
                    acc[k][0] += clip8(s0) * kvj; acc[k][1] += clip8(s1) * kvj; acc[k][2] += clip8(s2) * kvj;
                }
            }
#pragma unroll
            for (int k = 0; k < PX; ++k)
                if (in[k]) {
                    v[k][0] = clip8(acc[k][0]); v[k][1] = clip8(acc[k][1]); v[k][2] = clip8(acc[k][2]);
                    l[k] = lrow[tb.nx[x0 + k]];
                }
        }
        const int64_t pix = (int64_t)y * W + x0;
        if (PX == 4) {                                     // W % 4 == 0: 12 image bytes at a multiple of 12, 4 label bytes at a multiple of 4
            unsigned* o = reinterpret_cast<unsigned*>(oimg + pix * 3);
            const unsigned d0 = v[0][0] | v[0][1] << 8 | v[0][2] << 16 | (unsigned)v[1][0] << 24,
                           d1 = v[1][1] | v[1][2] << 8 | v[2][0] << 16 | (unsigned)v[2][1] << 24,
                           d2 = v[2][2] | v[3][0] << 8 | v[3][1] << 16 | (unsigned)v[3][2] << 24;
            o[0] = d0; o[1] = d1; o[2] = d2;
            *reinterpret_cast<unsigned*>(olbl + pix) = l[0] | l[1] << 8 | l[2] << 16 | (unsigned)l[3] << 24;
        } else {
            oimg[pix * 3] = (uint8_t)v[0][0]; oimg[pix * 3 + 1] = (uint8_t)v[0][1]; oimg[pix * 3 + 2] = (uint8_t)v[0][2];
            olbl[pix] = (uint8_t)l[0];
        }
    }
}

// ---- class-balanced crop choice: the rule of include/segfac.h (segf_input_crop_select) ---------------------------------------------
// One workgroup of 16 waves per sample walks the candidate windows IN ORDER and stops at the first that passes, so a batch whose
// first windows pass reads each label once, and nothing but the chosen index leaves the workgroup: no workspace, no second launch,
// no host read.  Counting: a lane takes 16 consecutive window pixels of one row and forms runs of equal bytes in registers; label
// maps are piecewise constant, so almost every lane ends with ONE run, and when the 64 runs of a wave carry the same value (the
// all-road window, where every lane would hit the same counter) they are summed across the wave by shuffles and added once.
// Anything else goes to the wave's OWN 256 raw-value counters in LDS by ds_add_u32, one add per run.  The counters are integers:
// the verdict does not depend on the order of the adds.  At the end of a window the 16 x 256 counters are merged, raw values that
// label_lut maps to one class are added up, and the test itself is one double division.
constexpr int SEL_THREADS = 1024, SEL_WAVES = SEL_THREADS / 64, SEL_SEG = 16;

struct SelectShared {
    unsigned hist[SEL_WAVES][256];                                        // per wave, per raw uint8 value
    long long cls[256];                                                   // label_lut (identity when null)
    unsigned raw[256];                                                    // the merged counters of the window
    unsigned ncls, maxc, sum;                                             // over the counted classes
};

// The final run (cur, run) of every lane of a wave -> the wave's counters.  Called by all 64 lanes; lanes without work carry
// run == 0, and they are the LAST lanes of the wave (work indices ascend with the lane), so lane 0's value stands for the wave.
__device__ __forceinline__ void select_flush(unsigned* __restrict__ h, int cur, int run) {
    const int first = __shfl(cur, 0, 64);
    if (__all(run == 0 || cur == first)) {
        int s = run;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&h[first], (unsigned)s);
    } else if (run) {
        atomicAdd(&h[cur], (unsigned)run);
    }
}

// Counts one H x W window.  load(y, x0, n, d): the raw labels of window pixels (y, x0 .. x0 + n - 1), n <= 16, one per byte of d[4]
// (bytes past n are zero).
template <class Load>
__device__ __forceinline__ void select_count(unsigned* __restrict__ h, int H, int W, const Load& load) {
    const int segs = (W + SEL_SEG - 1) / SEL_SEG;
    const int64_t total = (int64_t)H * segs;
    for (int64_t base = 0; base < total; base += SEL_THREADS) {           // workgroup-uniform trip count: select_flush needs whole waves
        const int64_t idx = base + threadIdx.x;
        int cur = -1, run = 0;
        if (idx < total) {
            const int y = (int)(idx / segs), x0 = (int)(idx - (int64_t)y * segs) * SEL_SEG;
            const int n = W - x0 < SEL_SEG ? W - x0 : SEL_SEG;
            unsigned d[4];
            load(y, x0, n, d);
            cur = (int)(d[0] & 255u);
            const unsigned rep = (unsigned)cur * 0x01010101u;
            if (n == SEL_SEG && d[0] == rep && d[1] == rep && d[2] == rep && d[3] == rep) {
                run = SEL_SEG;
            } else {
                run = 1;
#pragma unroll
                for (int k = 1; k < SEL_SEG; ++k)
                    if (k < n) {
                        const int v = (int)((d[k >> 2] >> (8 * (k & 3))) & 255u);
                        if (v == cur) ++run;
                        else { atomicAdd(&h[cur], (unsigned)run); cur = v; run = 1; }
                    }
            }
        }
        select_flush(h, cur, run);
    }
}

// unscaled stack: window pixel (y, x) is lbl[top + y][left + x], raw 0 outside the source (Image.crop)
struct SelectPlainLoad {
    const uint8_t* lbl; int64_t stride; int src_h, src_w; int64_t top, left;
    __device__ __forceinline__ void operator()(int y, int x0, int n, unsigned (&d)[4]) const {
        d[0] = d[1] = d[2] = d[3] = 0;
        const int64_t sy = top + y, cs = left + x0;
        if (sy < 0 || sy >= src_h || cs + n <= 0 || cs >= src_w) return;
        const uint8_t* row = lbl + sy * stride;
        if (n == SEL_SEG && cs >= 0 && cs + SEL_SEG <= src_w) {           // 16 bytes from any byte address: aligned dwords + v_alignbyte
            const uintptr_t q = (uintptr_t)row + (uintptr_t)cs;
            const uintptr_t qb = q & ~(uintptr_t)3, ql = (q + 15) & ~(uintptr_t)3;      // ql >= qb + 12
            const unsigned sh = (unsigned)(q & 3);
            const unsigned w0 = *(const unsigned*)qb, w1 = *(const unsigned*)(qb + 4), w2 = *(const unsigned*)(qb + 8),
                           w3 = *(const unsigned*)(qb + 12);
            const unsigned w4 = *(const unsigned*)(qb + 16 <= ql ? qb + 16 : ql);         // never past the dword of the last byte
            d[0] = __builtin_amdgcn_alignbyte(w1, w0, sh); d[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
            d[2] = __builtin_amdgcn_alignbyte(w3, w2, sh); d[3] = __builtin_amdgcn_alignbyte(w4, w3, sh);
        } else {
#pragma unroll
            for (int k = 0; k < SEL_SEG; ++k) {
                const int64_t sx = cs + k;
                const bool in = k < n && sx >= 0 && sx < src_w;
                const unsigned v = row[in ? sx : 0];                      // (cs + n > 0 and cs < src_w: column 0 exists)
                d[k >> 2] |= (in ? v : 0u) << (8 * (k & 3));
            }
        }
    }
};

// scaled stack: window pixel (y, x) is the NEAREST-resized label at resized (top + y, left + x) = lbl[ny[y]][nx[x]]; a table entry
// of -1 says that the row / column lies outside the resized image, where the pad fill stands
struct SelectScaledLoad {
    const uint8_t* lbl; int64_t stride; const int *nx, *ny; unsigned fill;
    __device__ __forceinline__ void operator()(int y, int x0, int n, unsigned (&d)[4]) const {
        d[0] = d[1] = d[2] = d[3] = 0;
        const int sy = ny[y];
        const uint8_t* row = lbl + (int64_t)(sy < 0 ? 0 : sy) * stride;
#pragma unroll
        for (int k = 0; k < SEL_SEG; ++k) {
            const int sx = k < n ? nx[x0 + k] : -1;
            const bool in = sy >= 0 && sx >= 0;
            const unsigned v = row[in ? sx : 0];
            d[k >> 2] |= (k < n ? (in ? v : fill) : 0u) << (8 * (k & 3));
        }
    }
};

__device__ __forceinline__ void select_init(SelectShared& sh, const int64_t* __restrict__ lut) {
    for (int i = threadIdx.x; i < SEL_WAVES * 256; i += SEL_THREADS) (&sh.hist[0][0])[i] = 0;
    if (threadIdx.x < 256) sh.cls[threadIdx.x] = lut ? (long long)lut[threadIdx.x] : (long long)threadIdx.x;
    __syncthreads();
}

// The verdict of the window just counted, the same value in every thread; leaves the counters zeroed for the next window.
__device__ __forceinline__ bool select_passes(SelectShared& sh, long long ignore_class, double max_ratio) {
    const int t = threadIdx.x;
    __syncthreads();
    if (t < 256) {
        unsigned n = 0;
#pragma unroll
        for (int w = 0; w < SEL_WAVES; ++w) n += sh.hist[w][t];
        sh.raw[t] = n;
    }
    if (t == 0) { sh.ncls = 0; sh.maxc = 0; sh.sum = 0; }
    __syncthreads();
    if (t < 256 && sh.raw[t] != 0 && sh.cls[t] != ignore_class) {
        // the class of raw value t is counted by the FIRST raw value present in the window that the table maps to it
        const long long c = sh.cls[t];
        unsigned tot = 0;
        bool rep = true;
        for (int u = 0; u < 256; ++u)
            if (sh.cls[u] == c) {
                if (u < t && sh.raw[u] != 0) rep = false;
                tot += sh.raw[u];
            }
        if (rep) { atomicAdd(&sh.ncls, 1u); atomicMax(&sh.maxc, tot); atomicAdd(&sh.sum, tot); }
    }
    for (int i = t; i < SEL_WAVES * 256; i += SEL_THREADS) (&sh.hist[0][0])[i] = 0;
    __syncthreads();
    // numpy's np.max(cnt) / np.sum(cnt) < cat_max_ratio: int64 / int64 is a float64 division; no division without two classes
    return sh.ncls >= 2u && (double)sh.maxc / (double)sh.sum < max_ratio;
}

__global__ void __launch_bounds__(SEL_THREADS) input_crop_select_kernel(segf_input_sample* samples, const int32_t* __restrict__ cand,
                                                                        int K, int H, int W, double max_ratio,
                                                                        const int64_t* __restrict__ lut, long long ignore_class,
                                                                        int32_t* __restrict__ chosen) {
    __shared__ SelectShared sh;
    const int b = blockIdx.x;
    const int32_t* cd = cand + (int64_t)b * K * 2;
    int pick = K - 1;
    if (K > 1) {
        const segf_input_sample s = samples[b];
        select_init(sh, lut);
        for (int k = 0; k < K - 1; ++k) {
            if (k > 0 && cd[2 * k] == cd[2 * k - 2] && cd[2 * k + 1] == cd[2 * k - 1]) continue;      // the window that has just failed
            select_count(sh.hist[threadIdx.x >> 6], H, W, SelectPlainLoad{s.lbl, s.lbl_stride, s.src_h, s.src_w, cd[2 * k], cd[2 * k + 1]});
            if (select_passes(sh, ignore_class, max_ratio)) { pick = k; break; }
        }
    }
    if (threadIdx.x == 0) {
        samples[b].top = cd[2 * pick];
        samples[b].left = cd[2 * pick + 1];
        if (chosen) chosen[b] = pick;
    }
}

// nearest_at's wave-uniform part for a lane at resized index `r`: the index of the wave's lane 0 (never negative), so that only the
// last < 64 additions of the chain are counted per lane, as input_scale_tables_kernel keeps them under 256
__device__ __forceinline__ int select_chain_base(int r) {
    const int r0 = __builtin_amdgcn_readfirstlane(r - (int)(threadIdx.x & 63));
    return r0 < 0 ? 0 : r0;
}

// the scaled stack's form: the nearest-index tables of a candidate's W columns and H rows go where input_scale_tables_kernel will put
// those of the chosen window afterwards (the same chain of double additions, nearest_at), then the window is counted through them
__global__ void __launch_bounds__(SEL_THREADS) input_scale_select_kernel(int H, int W, int kmax, ScaledWs t, const int32_t* __restrict__ cand,
                                                                         int K, double max_ratio, const int64_t* __restrict__ lut,
                                                                         long long ignore_class, int32_t* __restrict__ chosen) {
    __shared__ SelectShared sh;
    const int b = blockIdx.x;
    const int32_t* cd = cand + (int64_t)b * K * 2;
    int pick = K - 1;
    if (K > 1) {
        const segf_input_scaled_sample s = t.srecs[b];
        const ScaledTabs tb = scaled_tabs(t, b, H, W, kmax);
        select_init(sh, lut);
        for (int k = 0; k < K - 1; ++k) {
            const int top = cd[2 * k], left = cd[2 * k + 1];
            if (k > 0 && top == cd[2 * k - 2] && left == cd[2 * k - 1]) continue;
            for (int g = threadIdx.x; g < W; g += SEL_THREADS) {
                const int rx = left + g;
                tb.nx[g] = rx >= 0 && rx < s.res_w ? nearest_at(s.src_w, s.res_w, rx, select_chain_base(left + g)) : -1;
            }
            for (int g = threadIdx.x; g < H; g += SEL_THREADS) {
                const int ry = top + g;
                tb.ny[g] = ry >= 0 && ry < s.res_h ? nearest_at(s.src_h, s.res_h, ry, select_chain_base(top + g)) : -1;
            }
            __syncthreads();                                              // the tables are read by the whole workgroup
            select_count(sh.hist[threadIdx.x >> 6], H, W, SelectScaledLoad{s.lbl, s.lbl_stride, tb.nx, tb.ny, (unsigned)(s.label_fill & 255)});
            if (select_passes(sh, ignore_class, max_ratio)) { pick = k; break; }
        }
    }
    if (threadIdx.x == 0) {
        t.srecs[b].top = cd[2 * pick];
        t.srecs[b].left = cd[2 * pick + 1];
        if (chosen) chosen[b] = pick;
    }
}

inline bool select_args_ok(int K, double max_ratio) { return K >= 1 && K <= 32 && max_ratio > 0.0 && max_ratio <= 1.0; }   // NaN fails

// the launches of segf_input_train (arguments already checked): zero the luma sums, sum, transform
int launch_input_train(const segf_input_sample* samples, int B, int H, int W, uint64_t* lsum_ws, const float* mean3, const float* std3,
                       const int64_t* label_lut, float* out_img, int64_t* out_lbl, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const bool px4 = W % 4 == 0;
    const int64_t runs = (int64_t)H * (px4 ? W / 4 : W);
    // enough workgroups to fill 256 CUs several times over even at batch 1; grid.y = sample
    const int bx = (int)imin64(cdiv64(runs, 256), B >= 64 ? 64 : 1024);
    int rc = segf_zero(lsum_ws, (int64_t)B * 8, stream);
    if (rc) return rc;
    if (px4) {
        hipLaunchKernelGGL(input_lsum_kernel<4>, dim3(bx, B), dim3(256), 0, st, samples, H, W, (unsigned long long*)lsum_ws);
        hipLaunchKernelGGL(input_train_kernel<4>, dim3(bx, B), dim3(256), 0, st, samples, H, W, (const unsigned long long*)lsum_ws,
                           mean3, std3, label_lut, out_img, out_lbl);
    } else {
        hipLaunchKernelGGL(input_lsum_kernel<1>, dim3(bx, B), dim3(256), 0, st, samples, H, W, (unsigned long long*)lsum_ws);
        hipLaunchKernelGGL(input_train_kernel<1>, dim3(bx, B), dim3(256), 0, st, samples, H, W, (const unsigned long long*)lsum_ws,
                           mean3, std3, label_lut, out_img, out_lbl);
    }
    SEGF_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int segf_input_train(const segf_input_sample* samples, int B, int H, int W, uint64_t* lsum_ws, const float* mean3,
                                const float* std3, const int64_t* label_lut, float* out_img, int64_t* out_lbl, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    if (!samples || !lsum_ws || !mean3 || !std3 || !out_img || !out_lbl) return SEGF_ERR_SHAPE;
    if ((int64_t)H * W > (int64_t)1 << 30) return SEGF_ERR_SHAPE;
    if (((uintptr_t)out_img | (uintptr_t)out_lbl | (uintptr_t)lsum_ws | (uintptr_t)samples) % 16 != 0) return SEGF_ERR_SHAPE;
    return launch_input_train(samples, B, H, W, lsum_ws, mean3, std3, label_lut, out_img, out_lbl, stream);
}

extern "C" int64_t segf_input_train_scaled_ws(int B, int H, int W, int kmax) {
    if (B <= 0 || H <= 0 || W <= 0 || kmax < 3 || (int64_t)H * W > (int64_t)1 << 30) return 0;
    return scaled_ws(nullptr, B, H, W, kmax, nullptr);
}

namespace {

// what segf_input_train_scaled refuses (include/segfac.h); 0 when the arguments stand
int check_scaled(const segf_input_scaled_sample* samples, int B, int H, int W, int kmax, const void* ws, const float* mean3,
                 const float* std3, const float* out_img, const int64_t* out_lbl) {
    if (!samples || !ws || !mean3 || !std3 || !out_img || !out_lbl) return SEGF_ERR_SHAPE;
    if ((int64_t)H * W > (int64_t)1 << 30 || kmax < 3 || B > 65535) return SEGF_ERR_SHAPE;
    if (((uintptr_t)out_img | (uintptr_t)out_lbl | (uintptr_t)ws) % 16 != 0) return SEGF_ERR_SHAPE;
    const int big = 1 << 30;
    for (int b = 0; b < B; ++b) {
        const segf_input_scaled_sample& s = samples[b];
        if (!s.img || !s.lbl || s.src_h < 1 || s.src_w < 1 || s.res_h < 1 || s.res_w < 1 || s.res_h > big || s.res_w > big)
            return SEGF_ERR_SHAPE;
        if (s.img_stride < (int64_t)s.src_w * 3 || s.lbl_stride < s.src_w) return SEGF_ERR_SHAPE;
        if (s.top > big || s.top < -big || s.left > big || s.left < -big) return SEGF_ERR_SHAPE;
        if (resample_ksize(s.src_h, s.res_h) > kmax || resample_ksize(s.src_w, s.res_w) > kmax) return SEGF_ERR_SHAPE;
    }
    return 0;
}

// the kernels of segf_input_train_scaled over records that already stand in ws
int launch_scaled(const ScaledWs& t, int B, int H, int W, int kmax, const float* mean3, const float* std3, const int64_t* label_lut,
                  float* out_img, int64_t* out_lbl, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const bool px4 = W % 4 == 0;
    const int nt = W > H ? W : H;
    hipLaunchKernelGGL(input_scale_tables_kernel, dim3((int)cdiv64(nt, 256), B), dim3(256), 0, st, H, W, kmax, t);
    const int bx = (int)imin64(cdiv64((int64_t)H * (px4 ? W / 4 : W), 256), B >= 64 ? 64 : 1024);
    if (px4) hipLaunchKernelGGL(input_scale_crop_kernel<4>, dim3(bx, B), dim3(256), 0, st, H, W, kmax, t);
    else hipLaunchKernelGGL(input_scale_crop_kernel<1>, dim3(bx, B), dim3(256), 0, st, H, W, kmax, t);
    SEGF_CHECK_LAUNCH();
    return launch_input_train(t.recs, B, H, W, (uint64_t*)t.lsum, mean3, std3, label_lut, out_img, out_lbl, stream);
}

}  // namespace

extern "C" int segf_input_train_scaled(const segf_input_scaled_sample* samples, int B, int H, int W, int kmax, void* ws,
                                       const float* mean3, const float* std3, const int64_t* label_lut, float* out_img,
                                       int64_t* out_lbl, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const int rc = check_scaled(samples, B, H, W, kmax, ws, mean3, std3, out_img, out_lbl);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    ScaledWs t;
    scaled_ws(ws, B, H, W, kmax, &t);
    if (!segf_trace().dry) {
        hipError_t e = hipMemcpyAsync(t.srecs, samples, (size_t)B * sizeof(segf_input_scaled_sample), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);                 // the caller's array is free again on return
        if (e != hipSuccess) return (int)e;
    }
    return launch_scaled(t, B, H, W, kmax, mean3, std3, label_lut, out_img, out_lbl, stream);
}

extern "C" int segf_input_crop_select(segf_input_sample* samples, const int32_t* cand, int B, int K, int H, int W, double max_ratio,
                                      const int64_t* label_lut, int64_t ignore_class, int32_t* chosen, void* stream) {
    if (!select_args_ok(K, max_ratio) || !samples || !cand) return SEGF_ERR_SHAPE;
    if ((int64_t)H * W > (int64_t)1 << 30 || (uintptr_t)samples % 16 != 0 || (uintptr_t)cand % 4 != 0) return SEGF_ERR_SHAPE;
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    hipLaunchKernelGGL(input_crop_select_kernel, dim3(B), dim3(SEL_THREADS), 0, (hipStream_t)stream, samples, cand, K, H, W, max_ratio,
                       label_lut, (long long)ignore_class, chosen);
    SEGF_CHECK_LAUNCH();
    return 0;
}

// the workspace of segf_input_train_scaled with the [B][K][2] candidates behind it
extern "C" int64_t segf_input_train_scaled_select_ws(int B, int H, int W, int kmax, int K) {
    const int64_t base = segf_input_train_scaled_ws(B, H, W, kmax);
    if (base == 0 || K < 1 || K > 32) return 0;
    return base + (((int64_t)B * K * 8 + 15) & ~(int64_t)15);
}

extern "C" int segf_input_train_scaled_select(const segf_input_scaled_sample* samples, const int32_t* cand, int K, double max_ratio,
                                              int64_t ignore_class, int32_t* chosen, int B, int H, int W, int kmax, void* ws,
                                              const float* mean3, const float* std3, const int64_t* label_lut, float* out_img,
                                              int64_t* out_lbl, void* stream) {
    if (!select_args_ok(K, max_ratio) || !cand) return SEGF_ERR_SHAPE;
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const int rc = check_scaled(samples, B, H, W, kmax, ws, mean3, std3, out_img, out_lbl);
    if (rc) return rc;
    const int big = 1 << 30;
    for (int64_t i = 0; i < (int64_t)B * K * 2; ++i)
        if (cand[i] > big || cand[i] < -big) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    ScaledWs t;
    const int64_t base = scaled_ws(ws, B, H, W, kmax, &t);
    int32_t* dcand = (int32_t*)((uint8_t*)ws + base);
    if (!segf_trace().dry) {
        hipError_t e = hipMemcpyAsync(t.srecs, samples, (size_t)B * sizeof(segf_input_scaled_sample), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(dcand, cand, (size_t)B * K * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);                 // both host arrays are free again on return
        if (e != hipSuccess) return (int)e;
    }
    // the selection first: the coefficient tables depend on the window it writes into the uploaded records
    hipLaunchKernelGGL(input_scale_select_kernel, dim3(B), dim3(SEL_THREADS), 0, st, H, W, kmax, t, (const int32_t*)dcand, K, max_ratio,
                       label_lut, (long long)ignore_class, chosen);
    SEGF_CHECK_LAUNCH();
    return launch_scaled(t, B, H, W, kmax, mean3, std3, label_lut, out_img, out_lbl, stream);
}

// ---- single-image inference (estimate_model.py:85-97): T.Resize((nH, nW)) on the uint8 CHW tensor + x / 255 + Normalize -----------
// torchvision 0.15.2 (environment.yml:22) resizes a TENSOR through torch.nn.functional.interpolate(bilinear, align_corners=False,
// antialias=False) on the float32 cast, rounds (half to even) and casts back to uint8.  ATen's arithmetic (UpSampleKernel.cpp):
// scale = in / out in float; src = scale * (dst + 0.5) - 0.5 clamped at 0; i0 = (int) src, l1 = src - i0, l0 = 1 - l1,
// i1 = min(i0 + 1, in - 1); out = wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11) -- IEEE float32, no contraction
// (this file is built with -ffp-contract=off).  Then (u8 / 255 - mean) / std.
__global__ void __launch_bounds__(256) infer_preprocess_kernel(const uint8_t* __restrict__ img, int src_h, int src_w, int out_h, int out_w,
                                                               float sy, float sx, const float* __restrict__ mean3,
                                                               const float* __restrict__ std3, float* __restrict__ out) {
    const int64_t n = (int64_t)out_h * out_w;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int oy = (int)(i / out_w), ox = (int)(i - (int64_t)oy * out_w);
        float fy = __fsub_rn(__fmul_rn(sy, __fadd_rn((float)oy, 0.5f)), 0.5f), fx = __fsub_rn(__fmul_rn(sx, __fadd_rn((float)ox, 0.5f)), 0.5f);
        fy = fy < 0.f ? 0.f : fy; fx = fx < 0.f ? 0.f : fx;
        int y0 = (int)fy, x0 = (int)fx;
        y0 = y0 > src_h - 1 ? src_h - 1 : y0; x0 = x0 > src_w - 1 ? src_w - 1 : x0;
        const int y1 = y0 + 1 < src_h ? y0 + 1 : src_h - 1, x1 = x0 + 1 < src_w ? x0 + 1 : src_w - 1;
        float ly1 = __fsub_rn(fy, (float)y0), lx1 = __fsub_rn(fx, (float)x0);
        ly1 = ly1 < 0.f ? 0.f : (ly1 > 1.f ? 1.f : ly1); lx1 = lx1 < 0.f ? 0.f : (lx1 > 1.f ? 1.f : lx1);
        const float ly0 = __fsub_rn(1.f, ly1), lx0 = __fsub_rn(1.f, lx1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint8_t* p = img + (int64_t)c * src_h * src_w;
            const float v00 = (float)p[(int64_t)y0 * src_w + x0], v01 = (float)p[(int64_t)y0 * src_w + x1];
            const float v10 = (float)p[(int64_t)y1 * src_w + x0], v11 = (float)p[(int64_t)y1 * src_w + x1];
            const float top = __fadd_rn(__fmul_rn(lx0, v00), __fmul_rn(lx1, v01)), bot = __fadd_rn(__fmul_rn(lx0, v10), __fmul_rn(lx1, v11));
            float v = __fadd_rn(__fmul_rn(ly0, top), __fmul_rn(ly1, bot));
            v = rintf(v);                                                  // torch.round: half to even
            v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);                   // (the uint8 cast)
            out[(int64_t)c * n + i] = __fdiv_rn(__fsub_rn(__fdiv_rn(v, 255.f), mean3[c]), std3[c]);
        }
    }
}
extern "C" int segf_infer_preprocess(const uint8_t* img, int src_h, int src_w, int out_h, int out_w, const float* mean3, const float* std3,
                                     float* out, void* stream) {
    if (src_h <= 0 || src_w <= 0 || out_h <= 0 || out_w <= 0 || !img || !mean3 || !std3 || !out) return SEGF_ERR_SHAPE;
    const float sy = (float)src_h / (float)out_h, sx = (float)src_w / (float)out_w;
    const int blocks = (int)imin64(cdiv64((int64_t)out_h * out_w, 256), 4096);
    hipLaunchKernelGGL(infer_preprocess_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, img, src_h, src_w, out_h, out_w, sy, sx,
                       mean3, std3, out);
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t segf_input_val_ws(int src_h, int src_w, int out_h, int out_w) {
    if (src_h <= 0 || src_w <= 0 || out_h <= 0 || out_w <= 0) return 0;
    return val_tables(nullptr, src_h, src_w, out_h, out_w, nullptr);
}

extern "C" int segf_input_val(const uint8_t* img, int64_t img_stride, const uint8_t* lbl, int64_t lbl_stride, int src_h, int src_w,
                              int out_h, int out_w, void* ws, const float* mean3, const float* std3, const int64_t* label_lut,
                              float* out_img, int64_t* out_lbl, void* stream) {
    if (src_h <= 0 || src_w <= 0 || out_h <= 0 || out_w <= 0) return SEGF_ERR_SHAPE;
    if (!img || !lbl || !ws || !mean3 || !std3 || !out_img || !out_lbl) return SEGF_ERR_SHAPE;
    if ((uintptr_t)ws % 16 != 0) return SEGF_ERR_WORKSPACE;
    if (img_stride < (int64_t)src_w * 3 || lbl_stride < src_w) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    ValTables t;
    val_tables(ws, src_h, src_w, out_h, out_w, &t);
    const int nt = out_w > out_h ? out_w : out_h;
    hipLaunchKernelGGL(input_val_tables_kernel, dim3((int)cdiv64(nt < 2 ? 2 : nt, 256)), dim3(256), 0, st, src_h, src_w, out_h, out_w, t);
    hipLaunchKernelGGL(input_val_hpass_kernel, dim3((int)imin64(cdiv64((int64_t)src_h * out_w, 256), 8192)), dim3(256), 0, st, img,
                       img_stride, src_h, out_w, t);
    hipLaunchKernelGGL(input_val_vpass_kernel, dim3((int)imin64(cdiv64((int64_t)out_h * out_w, 256), 8192)), dim3(256), 0, st, lbl,
                       lbl_stride, out_h, out_w, t, mean3, std3, label_lut, out_img, out_lbl);
    SEGF_CHECK_LAUNCH();
    return 0;
}
