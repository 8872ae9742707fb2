// LayerNorm (rows = tokens, wave-shuffle statistics) and BatchNorm2d-on-NHWC (column statistics).
// HBM-bound streaming kernels: each activation is read once per pass with 16-B lane accesses.
//   LayerNorm: reference nn.LayerNorm in models/backbones/mit.py:107,129,136-140 (eps 1e-5) and the
//              channels-first LayerNorm of convnext.py:8-23 / convnextv2.py:40-66 (eps 1e-6).
//   BatchNorm: ConvModule of heads/segformer.py:21-29, layers/conv_module.py:4-9, mobilenetv2.py:5-11.
#include <type_traits>

#include "colreduce.h"

// ---- LayerNorm -----------------------------------------------------------------------------------------
// A row is spread over LPR = 2^lpr_log2 lanes (8 elements per lane per step, VPT steps); a wave handles
// 64/LPR rows at once.  Two-pass statistics in registers (mean, then centred variance), fp32.
// Patch-major token order of a spatial-reduction convolution's im2col matrix (mit.py:47, k = s = sr): token (b, y, x) of a [B, H, W] map
// is row ((b Ho + y / sr) Wo + x / sr) of the matrix and chunk (y % sr, x % sr) of that row -- a PERMUTATION of the token rows.  With W
// and sr powers of two (H a multiple of sr): t = r >> lw = b H + y, x = r & (W - 1).
__device__ __forceinline__ int64_t patch_row(int64_t r, int lw, int ls) {
    const int64_t t = r >> lw, x = r & (((int64_t)1 << lw) - 1), sm = ((int64_t)1 << ls) - 1;
    return ((((t >> ls) << (lw - ls)) + (x >> ls)) << (2 * ls)) + ((t & sm) << ls) + (x & sm);
}
template <typename T, int VPT>
__global__ void __launch_bounds__(256) ln_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, T* __restrict__ y,
                                                      float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                      int64_t rows, int C, float eps, int lpr_log2,
                                                      T* __restrict__ y2 /*nullable: the same rows in patch-major order*/, int lw, int ls) {
    const int lpr = 1 << lpr_log2;
    const int lane = threadIdx.x & 63;
    const int sub = lane & (lpr - 1), rin = lane >> lpr_log2;
    const int rows_per_wave = 64 >> lpr_log2;
    const int64_t wave_global = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    float g[VPT][8], b[VPT][8];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int c0 = (sub + i * lpr) * 8;
        if (c0 < C) { load8f(gamma + c0, g[i]); load8f(beta + c0, b[i]); }
    }
    const float invC = 1.f / (float)C;
    for (int64_t rbase = wave_global * rows_per_wave; rbase < rows; rbase += nwaves * rows_per_wave) {
        const int64_t r = rbase + rin;
        const bool rv = r < rows;
        float v[VPT][8];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int c0 = (sub + i * lpr) * 8;
            if (rv && c0 < C) {
                load8<T>(x + r * C + c0, v[i]);
#pragma unroll
                for (int j = 0; j < 8; ++j) s += v[i][j];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
            }
        }
        s = wave_sum(s, lpr);
        const float mu = s * invC;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int c0 = (sub + i * lpr) * 8;
            if (c0 < C) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mu; q += d * d; }
            }
        }
        q = wave_sum(q, lpr);
        const float rs = rsqrtf(q * invC + eps);
        if (rv) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int c0 = (sub + i * lpr) * 8;
                if (c0 < C) {
                    float o[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mu) * rs * g[i][j] + b[i][j];
                    store8<T>(y + r * C + c0, o);
                    if (y2) store8<T>(y2 + patch_row(r, lw, ls) * C + c0, o);
                }
            }
            if (sub == 0) { mean_out[r] = mu; rstd_out[r] = rs; }
        }
    }
}

#define LN_BWD_MAX_BLOCKS 1024      // 4 workgroups per CU (one per CU left the HBM pipe half empty: 2.7 TB/s at 2M x 32)
template <typename T, int VPT>
__global__ void __launch_bounds__(256) ln_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                      const T* __restrict__ dy2 /*nullable: second consumer's gradient, added to dy*/,
                                                      const T* __restrict__ dres /*nullable: residual-path gradient, added to dx*/,
                                                      const float* __restrict__ gamma, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, T* __restrict__ dx,
                                                      float* __restrict__ partial /*[grid][2][C]*/, int64_t rows, int C,
                                                      int lpr_log2, const float* __restrict__ rsc /*nullable: per-row-group scale of a second output*/,
                                                      float inv_rpg, T* __restrict__ dxs /*dxs = (T) dx * rsc[row / rpg]: the DropPath backward of dx's consumer*/,
                                                      int lw /*>= 0: dy2 is stored in patch-major row order (patch_row)*/, int ls) {
    extern __shared__ float lds[];   // [4 waves][2][C]
    const int lpr = 1 << lpr_log2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (lpr - 1), rin = lane >> lpr_log2;
    const int rows_per_wave = 64 >> lpr_log2;
    const int64_t wave_global = (int64_t)blockIdx.x * 4 + wave;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    float g[VPT][8], dg[VPT][8], db[VPT][8];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int c0 = (sub + i * lpr) * 8;
        if (c0 < C) load8f(gamma + c0, g[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) { dg[i][j] = 0.f; db[i][j] = 0.f; }
    }
    const float invC = 1.f / (float)C;
    for (int64_t rbase = wave_global * rows_per_wave; rbase < rows; rbase += nwaves * rows_per_wave) {
        const int64_t r = rbase + rin;
        const bool rv = r < rows;
        const int64_t rc = rv ? r : rows - 1;          // rows past the end: clamped loads, contributions masked below
        const float mu = mean[rc], rs = rv ? rstd[rc] : 0.f;
        float xh[VPT][8], gy[VPT][8];
        float s1 = 0.f, s2 = 0.f;
        Raw8<T> rx[VPT], rd[VPT], rd2[VPT], rr[VPT];
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int c0 = (sub + i * lpr) * 8, cc = c0 < C ? c0 : 0;
            rx[i] = load8_raw<T>(x + rc * C + cc);
            rd[i] = load8_raw<T>(dy + rc * C + cc);
            if (dy2) rd2[i] = load8_raw<T>(dy2 + (lw >= 0 ? patch_row(rc, lw, ls) : rc) * C + cc);          // workgroup-uniform branches: the loads stay batched
            if (dres) rr[i] = load8_raw<T>(dres + rc * C + cc);
        }
        SEGF_LOADS_ISSUED();
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int c0 = (sub + i * lpr) * 8;
            if (rv && c0 < C) {
                float xv[8], dv[8];
                unpack8(rx[i], xv);
                unpack8(rd[i], dv);
                if (dy2) {
                    float d2[8];
                    unpack8(rd2[i], d2);
#pragma unroll
                    for (int j = 0; j < 8; ++j) dv[j] += d2[j];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    xh[i][j] = (xv[j] - mu) * rs;
                    dg[i][j] += dv[j] * xh[i][j];
                    db[i][j] += dv[j];
                    gy[i][j] = dv[j] * g[i][j];
                    s1 += gy[i][j];
                    s2 += gy[i][j] * xh[i][j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) { xh[i][j] = 0.f; gy[i][j] = 0.f; }
            }
        }
        s1 = wave_sum(s1, lpr) * invC;
        s2 = wave_sum(s2, lpr) * invC;
        if (rv) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int c0 = (sub + i * lpr) * 8;
                if (c0 < C) {
                    float o[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[j] = rs * (gy[i][j] - s1 - xh[i][j] * s2);
                    if (dres) {
                        float rv8[8];
                        unpack8(rr[i], rv8);
#pragma unroll
                        for (int j = 0; j < 8; ++j) o[j] += rv8[j];
                    }
                    store8<T>(dx + r * C + c0, o);
                    if (dxs) {
                        // what segf_scale_rows computes from the STORED dx (DropPath backward, drop_path.py:18-25): the value rounded to T first.
                        // row / rpg through the reciprocal: exact below 2^22 rows (host-checked)
                        const float sc = rsc[(int)(((float)r + 0.5f) * inv_rpg)];
#pragma unroll
                        for (int j = 0; j < 8; ++j) o[j] = round_to<T>(o[j]) * sc;
                        store8<T>(dxs + r * C + c0, o);
                    }
                }
            }
        }
    }
    // reduce dgamma / dbeta: across the row lanes of the wave (xor offsets >= lpr), then across waves via LDS
#pragma unroll
    for (int i = 0; i < VPT; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float a = dg[i][j], c = db[i][j];
            for (int o = 32; o >= lpr; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
            dg[i][j] = a; db[i][j] = c;
        }
    if (rin == 0) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int c0 = (sub + i * lpr) * 8;
            if (c0 < C) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    lds[(wave * 2 + 0) * C + c0 + j] = dg[i][j];
                    lds[(wave * 2 + 1) * C + c0 + j] = db[i][j];
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        const int which = i / C, c = i - which * C;
        float s = 0.f;
        for (int w = 0; w < 4; ++w) s += lds[(w * 2 + which) * C + c];
        partial[((int64_t)blockIdx.x * 2 + which) * C + c] = s;
    }
}

template <typename T>
static void ln_fwd_launch(int vpt, int blocks, hipStream_t st, const T* x, const float* gamma, const float* beta, T* y,
                          float* mean, float* rstd, int64_t rows, int C, float eps, int lpr_log2, T* y2, int lw, int ls) {
#define LN_F(V) hipLaunchKernelGGL((ln_fwd_kernel<T, V>), dim3(blocks), dim3(256), 0, st, x, gamma, beta, y, mean, rstd, rows, C, eps, lpr_log2, y2, lw, ls)
    if (vpt == 1) LN_F(1); else if (vpt == 2) LN_F(2); else if (vpt == 3) LN_F(3); else if (vpt == 4) LN_F(4); else if (vpt == 5) LN_F(5); else LN_F(6);
#undef LN_F
}
template <typename T>
static void ln_bwd_launch(int vpt, int blocks, size_t shm, hipStream_t st, const T* x, const T* dy, const T* dy2, const T* dres, const float* gamma,
                          const float* mean, const float* rstd, T* dx, float* ws, int64_t rows, int C, int lpr_log2, const float* rsc,
                          float inv_rpg, T* dxs, int lw, int ls) {
#define LN_B(V) hipLaunchKernelGGL((ln_bwd_kernel<T, V>), dim3(blocks), dim3(256), shm, st, x, dy, dy2, dres, gamma, mean, rstd, dx, ws, rows, C, lpr_log2, rsc, inv_rpg, dxs, lw, ls)
    // C in (2048, 3072] (convnextv2_huge's 2816-wide last stage): six chunks per lane and 96 KB of dynamic LDS -- above the 64 KB
    // a kernel gets by default, so the limit is raised on the function first (160 KB per CU on gfx950)
#define LN_B_BIG(V) do { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ln_bwd_kernel<T, V>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm); LN_B(V); } while (0)
    if (vpt == 1) LN_B(1); else if (vpt == 2) LN_B(2); else if (vpt == 3) LN_B(3); else if (vpt == 4) LN_B(4); else if (vpt == 5) LN_B_BIG(5); else LN_B_BIG(6);
#undef LN_B_BIG
#undef LN_B
}

static inline int ln_plan(int C, int& lpr_log2) {
    const int nchunk = C / 8;
    lpr_log2 = 0;
    while ((1 << lpr_log2) < nchunk && lpr_log2 < 6) ++lpr_log2;
    return (nchunk + (1 << lpr_log2) - 1) >> lpr_log2;   // VPT
}

extern "C" int segf_layernorm_fwd_patch(int dt, int64_t rows, int C, const void* x, const float* gamma, const float* beta, float eps, void* y,
                                        float* mean, float* rstd, void* y2, int log2_w, int log2_sr, void* stream);
static int patch_geom_ok(int64_t rows, int log2_w, int log2_sr) {
    return log2_sr >= 1 && log2_w >= log2_sr && log2_w <= 20 && ((rows >> log2_w) << log2_w) == rows && ((rows >> log2_w) & (((int64_t)1 << log2_sr) - 1)) == 0;
}
extern "C" int segf_layernorm_fwd(int dt, int64_t rows, int C, const void* x, const float* gamma, const float* beta,
                                  float eps, void* y, float* mean, float* rstd, void* stream) {
    return segf_layernorm_fwd_patch(dt, rows, C, x, gamma, beta, eps, y, mean, rstd, nullptr, 0, 0, stream);
}
// ... with a second copy y2 of the output in the PATCH-MAJOR row order of a k = s = sr convolution's im2col matrix (mit.py:47): y2 viewed as
// [rows / sr^2][sr^2 C] IS that matrix (no segf_im2col pass over y).  The map width W = 2^log2_w and sr = 2^log2_sr; rows % (W sr) == 0.
extern "C" int segf_layernorm_fwd_patch(int dt, int64_t rows, int C, const void* x, const float* gamma, const float* beta, float eps, void* y,
                                        float* mean, float* rstd, void* y2, int log2_w, int log2_sr, void* stream) {
    if (rows <= 0) return 0;
    if (y2 && (!patch_geom_ok(rows, log2_w, log2_sr) || ((uintptr_t)y2 % 16))) return SEGF_ERR_SHAPE;
    if (C <= 0 || C % 8 != 0 || C > 3072) return SEGF_ERR_SHAPE;
    if (((uintptr_t)x % 16) || ((uintptr_t)y % 16) || ((uintptr_t)gamma % 16) || ((uintptr_t)beta % 16)) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    int lpr_log2;
    const int vpt = ln_plan(C, lpr_log2);
    const int rows_per_block = 4 * (64 >> lpr_log2);
    const int blocks = (int)imin64(cdiv64(rows, rows_per_block), 4096);
    SEGF_DISPATCH_DT(dt, T, { ln_fwd_launch<T>(vpt, blocks, st, (const T*)x, gamma, beta, (T*)y, mean, rstd, rows, C, eps, lpr_log2, (T*)y2, log2_w, log2_sr); })
    SEGF_CHECK_LAUNCH();
    return 0;
}

static inline int ln_bwd_blocks(int64_t rows, int C) {
    int lpr_log2;
    ln_plan(C, lpr_log2);
    const int rows_per_block = 4 * (64 >> lpr_log2);
    const int64_t b4 = cdiv64(rows, (int64_t)rows_per_block * 4);
    // few rows (the stage-3 / 4 maps at the reference's default batch of 4, train_gpu.py:71): one row group per wave instead of four --
    // the launch is a chain of dependent load rounds on a fraction of the chip, and four rounds cost 10 us where one costs 6
    if (b4 < 256) return (int)imin64(cdiv64(rows, (int64_t)rows_per_block), LN_BWD_MAX_BLOCKS);
    return (int)imin64(b4, LN_BWD_MAX_BLOCKS);
}
extern "C" int64_t segf_layernorm_bwd_ws(int64_t rows, int C) { return (int64_t)ln_bwd_blocks(rows, C) * 2 * C; }

extern "C" int segf_layernorm_bwd_fused(int dt, int64_t rows, int C, const void* x, const void* dy, const void* dy2, const void* dres,
                                        const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                                        float* dbeta, float* ws, void* stream);
extern "C" int segf_layernorm_bwd_scaled(int dt, int64_t rows, int C, const void* x, const void* dy, const void* dy2, const void* dres,
                                         const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                                         float* dbeta, float* ws, const float* rscale, int64_t rows_per_group, void* dxs, void* stream);
extern "C" int segf_layernorm_bwd_patch(int dt, int64_t rows, int C, const void* x, const void* dy, const void* dy2, const void* dres,
                                        const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                                        float* dbeta, float* ws, const float* rscale, int64_t rows_per_group, void* dxs, int log2_w,
                                        int log2_sr, void* stream);
extern "C" int segf_layernorm_bwd(int dt, int64_t rows, int C, const void* x, const void* dy, const float* gamma,
                                  const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta,
                                  float* ws, void* stream) {
    return segf_layernorm_bwd_fused(dt, rows, C, x, dy, nullptr, nullptr, gamma, mean, rstd, dx, dgamma, dbeta, ws, stream);
}
extern "C" int segf_layernorm_bwd_fused(int dt, int64_t rows, int C, const void* x, const void* dy, const void* dy2, const void* dres,
                                        const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                                        float* dbeta, float* ws, void* stream) {
    return segf_layernorm_bwd_scaled(dt, rows, C, x, dy, dy2, dres, gamma, mean, rstd, dx, dgamma, dbeta, ws, nullptr, 1, nullptr, stream);
}
// ... with a second output dxs[r][c] = (T) dx[r][c] * rscale[r / rows_per_group]: when dx's consumer is the backward of a residual branch
// `x + DropPath(f(.))` (mit.py:143-146), its first step is exactly this row scaling of the incoming gradient (one launch per branch)
extern "C" int segf_layernorm_bwd_scaled(int dt, int64_t rows, int C, const void* x, const void* dy, const void* dy2, const void* dres,
                                         const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                                         float* dbeta, float* ws, const float* rscale, int64_t rows_per_group, void* dxs, void* stream) {
    return segf_layernorm_bwd_patch(dt, rows, C, x, dy, dy2, dres, gamma, mean, rstd, dx, dgamma, dbeta, ws, rscale, rows_per_group, dxs, -1, 0, stream);
}
// ... with dy2 stored in the patch-major row order of segf_layernorm_fwd_patch's y2 (log2_w >= 0): the gradient of that second output, as the
// data-gradient product of the convolution leaves it (no segf_col2im pass)
extern "C" int segf_layernorm_bwd_patch(int dt, int64_t rows, int C, const void* x, const void* dy, const void* dy2, const void* dres,
                                        const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                                        float* dbeta, float* ws, const float* rscale, int64_t rows_per_group, void* dxs, int log2_w,
                                        int log2_sr, void* stream) {
    if (rows <= 0) return 0;
    if (log2_w >= 0 && (!dy2 || !patch_geom_ok(rows, log2_w, log2_sr))) return SEGF_ERR_SHAPE;
    if ((rscale != nullptr) != (dxs != nullptr)) return SEGF_ERR_SHAPE;
    if (rscale && (rows_per_group <= 0 || rows >= (1ll << 22) || ((uintptr_t)dxs % 16))) return SEGF_ERR_SHAPE;
    if (((uintptr_t)dy2 % 16) || ((uintptr_t)dres % 16)) return SEGF_ERR_SHAPE;
    if (C <= 0 || C % 8 != 0 || C > 3072) return SEGF_ERR_SHAPE;
    if (!ws) return SEGF_ERR_WORKSPACE;
    if (dgamma && dbeta != dgamma + C) return SEGF_ERR_SHAPE;   // dgamma and dbeta are one [2][C] fp32 buffer (NULL: deferred finalize)
    hipStream_t st = (hipStream_t)stream;
    int lpr_log2;
    const int vpt = ln_plan(C, lpr_log2);
    const int blocks = ln_bwd_blocks(rows, C);
    const size_t shm = (size_t)4 * 2 * C * sizeof(float);
    const float inv_rpg = rscale ? 1.0f / (float)rows_per_group : 0.f;
    SEGF_DISPATCH_DT(dt, T, { ln_bwd_launch<T>(vpt, blocks, shm, st, (const T*)x, (const T*)dy, (const T*)dy2, (const T*)dres, gamma, mean, rstd, (T*)dx, ws, rows, C, lpr_log2, rscale, inv_rpg, (T*)dxs, log2_w, log2_sr); })
    SEGF_CHECK_LAUNCH();
    if (!dgamma) return 0;                       // deferred: the caller finalizes ws later (segf_colreduce_finalize_grouped)
    const int64_t n = 2 * (int64_t)C;
    colreduce_finalize_launch(ws, blocks, n, dgamma, st);
    SEGF_CHECK_LAUNCH();
    return 0;
}
extern "C" int segf_layernorm_bwd_blocks(int64_t rows, int C) { return rows > 0 ? ln_bwd_blocks(rows, C) : 0; }
extern "C" int segf_colreduce_finalize_grouped(int n, const SegfFinalizeItem* items, void* stream) {
    if (n <= 0) return 0;
    if (!items) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    ColreduceGroup g;
    g.n = 0; g.start[0] = 0;
    for (int i = 0; i < n; ++i) {
        const SegfFinalizeItem& it = items[i];
        if (it.len <= 0 || it.nblk <= 0) continue;
        if (!it.partial || !it.out) return SEGF_ERR_SHAPE;
        const int k = g.n;
        if (it.scatter_c < 0 || (it.scatter_c > 0 && it.len != 10 * (int64_t)it.scatter_c)) return SEGF_ERR_SHAPE;
        g.partial[k] = it.partial; g.out[k] = it.out; g.nblk[k] = it.nblk; g.len[k] = it.len; g.scatter_c[k] = it.scatter_c;
        g.start[k + 1] = g.start[k] + (unsigned)cdiv64(it.len, CRF_OUT);
        if (++g.n == CRF_GROUP_MAX || i == n - 1) {
            hipLaunchKernelGGL(colreduce_finalize_group_kernel, dim3(g.start[g.n]), dim3(CRF_OUT * CRF_SL), 0, st, g);
            SEGF_CHECK_LAUNCH();
            g.n = 0;
        }
    }
    if (g.n > 0) {
        hipLaunchKernelGGL(colreduce_finalize_group_kernel, dim3(g.start[g.n]), dim3(CRF_OUT * CRF_SL), 0, st, g);
        SEGF_CHECK_LAUNCH();
    }
    return 0;
}

// ---- fc1 data gradient + LayerNorm backward + fc1 weight / bias gradient in ONE streaming pass ------------------------------
// The backward of `norm2 -> mlp.fc1` of a MiT block (mit.py:98,136-146) at C = 32 / 64, hidden width H = 4 C, as three launches reads
// the hidden-width gradient dh twice and writes + re-reads the C-wide product dy = dh W1.  Here a
// workgroup walks tiles of 64 token rows; the dh and y (saved LayerNorm output) rows of a tile are staged ONCE in LDS and
//   * wave w forms dy^T = W1^T dh^T for its 16 tokens with the MFMA sequence of the kernel that forms it today (C = 32:
//     gemm_skinny_kernel<1, 4, 2>, one chain over K ascending; C = 64: gemm_skinny_k_kernel<1, 2, 4>, four K-quarter chains
//     from zero added in the order 0..3 -- or, below the row count from which segf_gemm takes that kernel, the one chain of the
//     128-tile kernel: `ksplit`), rounds it to bf16 once, and applies ln_bwd_kernel's arithmetic to the rounded
//     values: lane (mi, g) holds features 32 q + 8 g .. + 7 of token mi, so a token's chunks sit 16 lanes apart and the row
//     sums run over them in wave_sum's pairing (xor 1, xor 2 on the chunk index, then xor 4 = the lane's own second chunk);
//   * wave w accumulates rows [H / 4 w, H / 4 (w + 1)) of dW1 += dh^T y and db1 += colsum(dh) over all 64 tokens, both
//     operands read transposed from the staged tiles (ds_read_b64_tr_b16), as gemm_dw_skinny_kernel does.
// dW1, db1, dgamma, dbeta leave as per-workgroup fp32 partials (fixed order, no atomics) for the column-reduction finalize.
// The next tile's rows are in flight in registers meanwhile; rows past the end: clamped loads, zeroed
// staging (no contribution to dW1 / db1), masked LayerNorm sums and stores.
#define LNL_MAX_BLOCKS 512          // 2 workgroups per CU (75 KB of LDS each at C = 64)
typedef __attribute__((ext_vector_type(8))) __bf16 lnl_bf16x8;
typedef __attribute__((ext_vector_type(4))) float lnl_f32x4;
typedef __attribute__((ext_vector_type(4))) short lnl_s16x4;
typedef __attribute__((ext_vector_type(8))) short lnl_s16x8;
typedef uint32_t lnl_u32x4 __attribute__((ext_vector_type(4)));
// 32 tokens x 16 features of a staged token-major tile as an MFMA fragment with the TOKENS along k (gemm.hip: frag_tok_tr)
__device__ __forceinline__ lnl_bf16x8 lnl_frag_tok_tr(const unsigned char* tile, int rowbytes, int cb, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const unsigned char* a0 = tile + (8 * g + q) * rowbytes + (cb + 4 * p) * 2;
    const lnl_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) lnl_s16x4*)a0);
    const lnl_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) lnl_s16x4*)(a0 + 4 * rowbytes));
    const lnl_s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(lnl_bf16x8, v);
}
// ln_bwd_kernel's per-chunk arithmetic for dx as that kernel's machine code performs it (the compiler keeps gy = dv * g and
// gy * xh as rounded products and contracts gy - s1 - xh * s2 and the residual addition into fused multiply-adds): contraction is
// off here and the fused operations are spelled out, so that the two kernels agree bit for bit whatever the optimiser would
// choose for this one.
// (xh and gy are formed twice, before and after the row sums, by the same operations on the same values: 32 registers fewer
// across the sums at C = 64)
__device__ __forceinline__ void lnl_chunk_sums(const float (&xv)[8], const float (&dv)[8], const float (&g)[8], float mu, float rs,
                                               float (&xh)[8], float& s1, float& s2) {
#pragma clang fp contract(off)
    s1 = 0.f; s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        xh[j] = (xv[j] - mu) * rs;
        const float gy = dv[j] * g[j];
        s1 = s1 + gy;
        const float p = gy * xh[j];
        s2 = s2 + p;
    }
}
__device__ __forceinline__ void lnl_chunk_out(const float (&xv)[8], const float (&dv)[8], const float (&g)[8], float mu, float s1, float s2,
                                              float rs, bool has_res, const float (&res)[8], float (&o)[8]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float xh = (xv[j] - mu) * rs;
        const float gy = dv[j] * g[j];
        const float t = __builtin_fmaf(-s2, xh, gy - s1);
        o[j] = has_res ? __builtin_fmaf(rs, t, res[j]) : rs * t;
    }
}
__device__ __forceinline__ void lnl_unpack8(const lnl_u32x4 u, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[2 * j] = __uint_as_float(u[j] << 16); v[2 * j + 1] = __uint_as_float(u[j] & 0xffff0000u); }
}
__device__ __forceinline__ lnl_u32x4 lnl_pack8(const float (&v)[8]) {
    lnl_u32x4 u;
    u[0] = pack2bf(v[0], v[1]); u[1] = pack2bf(v[2], v[3]); u[2] = pack2bf(v[4], v[5]); u[3] = pack2bf(v[6], v[7]);
    return u;
}
// The same pass in three more forms (template arguments behind KS; the three-argument-less spelling is the form above):
//   YX   the LayerNorm output is not read but REBUILT from the x rows, mean, rstd the kernel loads anyway: y = bf16(fma(gamma, xh, beta)) with
//        xh = (x - mean) * rstd -- ln_fwd_kernel's operations (its gfx950 code: subtract, multiply, one fused multiply-add, one rounding), so
//        the staged tile holds the bits that kernel stored and dW1 does not change.  The wave's 16 token rows go to LDS behind the LayerNorm
//        phase (one more barrier per tile); nothing else is staged for y.
//   HM   hidden width H = HM * C: 4 (mlp.fc1) or 1 (the attention's q Linear behind norm1, mit.py:45,143: ONE row of W fragments, one chain over
//        K = C; the wave's share of dW is one 16-row tile -- at C = 32 the four waves take the four 16 x 16 tiles of the [32][32] output)
//   FAN  a second consumer's gradient dy2 (norm1's patch-major output feeding the spatial-reduction convolution: rows in patch_row order when
//        lw >= 0) is added to the bf16-rounded dy on load, in fp32, exactly as ln_bwd_kernel adds its dy2.
template <int KS, int HM = 4> struct LnlGeom {
    static constexpr int C = 32 * KS, H = HM * C;
    static constexpr int RD = 2 * H + 16, RY = 2 * C + 16;               // staged row bytes (+16: bank spread)
    static constexpr int KSTEPS = H / 32;
    static constexpr int NFRAG = 2 * KS * KSTEPS;                        // W1 fragments of 1 KB: [2 KS feature tiles][H / 32 k-steps]
    static constexpr int OFF_Y = 64 * RD, OFF_W = OFF_Y + 64 * RY, OFF_G = OFF_W + 1024 * NFRAG, LDS_BYTES = OFF_G + 8 * C;   // gamma | beta
};
__device__ __forceinline__ void lnl_chunk_y(const float (&xh)[8], const float (&g)[8], const float (&b)[8], float (&o)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = __builtin_fmaf(g[j], xh[j], b[j]);
}
template <int KS, bool YX = false, int HM = 4, bool FAN = false>
__global__ void __launch_bounds__(256, 2) ln_linear_bwd_kernel(const bf16_t* __restrict__ dh, const bf16_t* __restrict__ w1 /*[H][C]*/,
                                                                const bf16_t* __restrict__ x, const bf16_t* __restrict__ y,
                                                                const bf16_t* __restrict__ dres /*nullable*/, const float* __restrict__ gamma,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                bf16_t* __restrict__ dx, const float* __restrict__ rsc /*nullable*/, uint32_t rpg,
                                                                bf16_t* __restrict__ dxs, bf16_t* __restrict__ dyo /*nullable: the fc1 data gradient*/,
                                                                float* __restrict__ pw /*[grid][H][C]*/, float* __restrict__ pb /*[grid][H]*/,
                                                                float* __restrict__ pg /*[grid][2][C]*/, int64_t rows,
                                                                int ksplit /*C = 64: K-quarter partials (else one chain over K)*/,
                                                                const float* __restrict__ beta /*YX*/, const bf16_t* __restrict__ dy2 /*FAN*/, int lw, int ls) {
    typedef LnlGeom<KS, HM> G;
    constexpr int C = G::C, H = G::H, RD = G::RD, RY = G::RY, KSTEPS = G::KSTEPS;
    constexpr int NT = 2 * KS;                                           // 16-feature tiles of dy
    constexpr int NQ = (KS == 1 || HM == 1) ? 1 : 4, SPQ = HM == 1 ? KS : (KS == 1 ? 4 : 2);           // accumulation chains over K and 32-steps per chain
    constexpr int ND = H / 32, NY = KS;                                  // 16-byte chunks per thread of a staged dh / y tile
    constexpr bool QUAD = HM == 1 && KS == 1;                            // H / 4 = 8 rows per wave would split a tile: wave -> (row tile, column tile)
    constexpr int NI = HM == 1 ? 1 : NT, NJ = QUAD ? 1 : NT;             // the wave's block of dW1 in 16 x 16 tiles
    extern __shared__ __attribute__((aligned(16))) unsigned char lnl_lds[];
    unsigned char* dhs = lnl_lds;
    unsigned char* ys = lnl_lds + G::OFF_Y;
    unsigned char* wl = lnl_lds + G::OFF_W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mi = lane & 15, g = lane >> 4;
    // W1 fragments in LDS, fragment (nt, ks) at 1 KB * (nt * 4 KS + ks): MFMA row i of tile nt carries feature
    // 32 (nt >> 1) + 8 (i >> 2) + 4 (nt & 1) + (i & 3) and lane group g the k rows 32 ks + 8 g .. + 7 (gemm_skinny_kernel, LAYOUT 1)
    for (int f = wave; f < G::NFRAG; f += 4) {
        const int nt = f / KSTEPS, ks = f - nt * KSTEPS;
        const int n = 32 * (nt >> 1) + 8 * (mi >> 2) + 4 * (nt & 1) + (mi & 3);
        lnl_s16x8 w;
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = (short)w1[(32 * ks + 8 * g + j) * C + n];
        *reinterpret_cast<lnl_s16x8*>(wl + 1024 * f + 16 * lane) = w;
    }
    float* gml = reinterpret_cast<float*>(lnl_lds + G::OFF_G);           // gamma, read back per tile (16 registers fewer at C = 64)
    if (tid < C) gml[tid] = gamma[tid];
    float* btl = gml + C;
    if (YX && tid < C) btl[tid] = beta[tid];
    const int rowbase = QUAD ? 16 * (wave >> 1) : (H / 4) * wave, jbase = QUAD ? (wave & 1) : 0;
    // dgamma / dbeta: a token's 16 lanes (one DPP row) sum each of the lane group's 8 KS features per tile, and lane mi keeps
    // the running sum of feature 32 (mi >> 3) + 8 g + (mi & 7) -- two accumulators per lane instead of 16 KS
    float accg = 0.f, accb = 0.f;
    // this wave's [H / 4 x C] block of dW1; its db1 rows share ONE accumulator tile: row tile i is multiplied by a B fragment
    // whose column i is all ones, so column i of the tile collects colsum(dh) of rows 16 i .. 16 i + 15
    lnl_f32x4 aw[NI][NJ], ab = lnl_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) aw[i][j] = lnl_f32x4{0.f, 0.f, 0.f, 0.f};
    float bz = 0.f;                                                      // the absent bias of the data-gradient product (acc + 0, as that kernel adds it)
    asm volatile("" : "+v"(bz));
    const float invC = 1.f / (float)C;
    const int64_t ntiles = (rows + 63) >> 6;
    // staging: pass i of a thread takes chunk (tid % chunks per row) of row tid / (chunks per row) + i * (rows per pass) -- one
    // column offset and one LDS address per thread, so that nothing per pass is kept across the loop
    constexpr int CPD = H / 8, RPD = 256 / CPD, CPY = C / 8, RPY = 256 / CPY;
    // Global addresses are a tile-uniform base (scalar registers) plus a 32-bit lane offset of the row within the tile, clamped
    // to the tile's last existing row.
    const int drow = tid / CPD, yrow = tid / CPY, dcol = 8 * (tid % CPD), ycol = 8 * (tid % CPY);
    unsigned char* dst_d = dhs + drow * RD + 2 * dcol;
    unsigned char* dst_y = ys + yrow * RY + 2 * ycol;
    lnl_u32x4 rd[ND], ry[NY];
    auto tile_last = [&](int64_t t) { const int64_t rem = rows - 1 - (t << 6); return (int)(rem < 63 ? rem : 63); };
    auto load_tile = [&](int64_t t) {
        const bf16_t* dht = dh + (t << 6) * H;
        const bf16_t* yt = y + (t << 6) * C;
        const int last = tile_last(t);
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const int lr = drow + RPD * i < last ? drow + RPD * i : last;
            rd[i] = *reinterpret_cast<const lnl_u32x4*>(dht + (uint32_t)(lr * H + dcol));
        }
        if (!YX) {
#pragma unroll
            for (int i = 0; i < NY; ++i) {
                const int lr = yrow + RPY * i < last ? yrow + RPY * i : last;
                ry[i] = *reinterpret_cast<const lnl_u32x4*>(yt + (uint32_t)(lr * C + ycol));
            }
        }
    };
    int64_t tile = blockIdx.x;
    if (tile < ntiles) load_tile(tile);
    for (; tile < ntiles; tile += gridDim.x) {
        const int64_t r0 = tile << 6;
        __syncthreads();                                                 // the previous tile's fragment reads (and the W1 fill) are complete
        const lnl_u32x4 zero4 = {0u, 0u, 0u, 0u};
        const int last = tile_last(tile);
#pragma unroll
        for (int i = 0; i < ND; ++i) *reinterpret_cast<lnl_u32x4*>(dst_d + RPD * i * RD) = drow + RPD * i <= last ? rd[i] : zero4;
        if (!YX) {
#pragma unroll
            for (int i = 0; i < NY; ++i) *reinterpret_cast<lnl_u32x4*>(dst_y + RPY * i * RY) = yrow + RPY * i <= last ? ry[i] : zero4;
        }
        // this tile's LayerNorm operands of the lane's token
        const int lrow = 16 * wave + mi;
        const bool rv = lrow <= last;
        const int lrc = rv ? lrow : last;
        const uint32_t eo = (uint32_t)(lrc * C + 8 * g);                 // the lane's first chunk, elements from the tile's first row
        const bf16_t* xt = x + r0 * C;
        const bf16_t* rt = dres + r0 * C;
        lnl_u32x4 rx[KS], rr[KS], r2[KS];
        const bf16_t* d2t = nullptr;
        if (FAN) d2t = lw >= 0 ? dy2 + patch_row(r0 + lrc, lw, ls) * C + 8 * g : dy2 + r0 * C + eo;
#pragma unroll
        for (int q = 0; q < KS; ++q) {
            rx[q] = *reinterpret_cast<const lnl_u32x4*>(xt + (eo + 32 * q));
            if (dres) rr[q] = *reinterpret_cast<const lnl_u32x4*>(rt + (eo + 32 * q));
            if (FAN) r2[q] = *reinterpret_cast<const lnl_u32x4*>(d2t + 32 * q);
        }
        const float mu = (mean + r0)[lrc], rs = rv ? (rstd + r0)[lrc] : 0.f;
        float sc = 0.f;
        if (dxs) sc = rsc[(uint32_t)(r0 + lrc) / rpg];
        // The next tile's rows (unconditional: the last one re-reads).  C = 32 requests them here, a whole tile ahead; at C = 64 the 40
        // registers they land in are not free across the two phases below (the kernel spilled), so there they are requested
        // behind the LayerNorm phase and land during the weight-gradient products and the other workgroup's turn.
        const int64_t nxt = tile + gridDim.x < ntiles ? tile + gridDim.x : tile;
        if (KS == 1) load_tile(nxt);
        SEGF_LOADS_ISSUED();
        __syncthreads();
        // ---- data gradient of the wave's 16 tokens: dy^T = W1^T dh^T, the dh rows as the B operand as they lie
        float dyv[KS][8];
        {
            lnl_f32x4 sum[NT];
            const unsigned char* brow = dhs + (16 * wave + mi) * RD + 16 * g;
            // (a rolled loop over the K quarters: unrolled, the scheduler lifts all 32 fragment reads of C = 64 above the first product
            // and the kernel spills)
#pragma unroll 1
            for (int kq = 0; kq < NQ; ++kq) {
                lnl_bf16x8 xa[SPQ];
#pragma unroll
                for (int s = 0; s < SPQ; ++s) xa[s] = *reinterpret_cast<const lnl_bf16x8*>(brow + 64 * (kq * SPQ + s));
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    lnl_f32x4 a = lnl_f32x4{0.f, 0.f, 0.f, 0.f};
                    if (kq != 0 && !ksplit) a = sum[nt];                 // one chain over all of K
#pragma unroll
                    for (int s = 0; s < SPQ; ++s) {
                        const lnl_bf16x8 wf = *reinterpret_cast<const lnl_bf16x8*>(wl + 1024 * (nt * KSTEPS + kq * SPQ + s) + 16 * lane);
                        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xa[s], a, 0, 0, 0);
                    }
                    if (kq == 0 || !ksplit) sum[nt] = a; else sum[nt] = sum[nt] + a;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < KS; ++q)
#pragma unroll
                for (int rr_ = 0; rr_ < 4; ++rr_) { dyv[q][rr_] = sum[2 * q][rr_] + bz; dyv[q][4 + rr_] = sum[2 * q + 1][rr_] + bz; }
        }
        // ---- LayerNorm backward on the bf16-rounded dy
        {
            lnl_u32x4 dp[KS];
            float s1[KS], s2[KS];
#pragma unroll
            for (int q = 0; q < KS; ++q) {
                dp[q] = lnl_pack8(dyv[q]);
                if (dyo && rv) *reinterpret_cast<lnl_u32x4*>(dyo + r0 * C + (eo + 32 * q)) = dp[q];
                if (!rv) dp[q] = lnl_u32x4{0u, 0u, 0u, 0u};              // (rs == 0 too: xh = 0, nothing reaches dgamma / dbeta)
                float xv[8], dv[8], gm[8], xh[8];
                lnl_unpack8(rx[q], xv);
                lnl_unpack8(dp[q], dv);
                if (FAN) {
                    if (!rv) r2[q] = lnl_u32x4{0u, 0u, 0u, 0u};
                    float d2[8];
                    lnl_unpack8(r2[q], d2);
#pragma unroll
                    for (int j = 0; j < 8; ++j) dv[j] = dv[j] + d2[j];
                }
                load8f(gml + 32 * q + 8 * g, gm);
                lnl_chunk_sums(xv, dv, gm, mu, rs, xh, s1[q], s2[q]);
                if (YX) {
                    // the lane's chunk of y into the staged tile (zero rows past the end, as the staging of a stored y leaves them)
                    float bt[8], yv[8];
                    load8f(btl + 32 * q + 8 * g, bt);
                    lnl_chunk_y(xh, gm, bt, yv);
                    *reinterpret_cast<lnl_u32x4*>(ys + lrow * RY + 2 * (32 * q + 8 * g)) = rv ? lnl_pack8(yv) : lnl_u32x4{0u, 0u, 0u, 0u};
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float ag = wave_sum(dv[j] * xh[j], 16), abt = wave_sum(dv[j], 16);
                    if (mi == 8 * q + j) { accg += ag; accb += abt; }
                }
                s1[q] += __shfl_xor(s1[q], 16, 64); s1[q] += __shfl_xor(s1[q], 32, 64);
                s2[q] += __shfl_xor(s2[q], 16, 64); s2[q] += __shfl_xor(s2[q], 32, 64);
                __builtin_amdgcn_sched_barrier(0);
            }
            float t1 = s1[0], t2 = s2[0];
            if (KS == 2) { t1 += s1[KS - 1]; t2 += s2[KS - 1]; }
            t1 *= invC; t2 *= invC;
#pragma unroll
            for (int q = 0; q < KS; ++q) {
                float xv[8], dv[8], gm[8], o[8], res[8];
                lnl_unpack8(rx[q], xv);
                lnl_unpack8(dp[q], dv);
                if (FAN) {
                    float d2[8];
                    lnl_unpack8(r2[q], d2);
#pragma unroll
                    for (int j = 0; j < 8; ++j) dv[j] = dv[j] + d2[j];
                }
                load8f(gml + 32 * q + 8 * g, gm);
                if (dres) lnl_unpack8(rr[q], res);
                else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) res[j] = 0.f;
                }
                lnl_chunk_out(xv, dv, gm, mu, t1, t2, rs, dres != nullptr, res, o);
                const lnl_u32x4 op = lnl_pack8(o);
                if (rv) *reinterpret_cast<lnl_u32x4*>(dx + r0 * C + (eo + 32 * q)) = op;
                if (dxs) {
                    float ov[8];
                    lnl_unpack8(op, ov);                                 // the STORED dx (rounded), as segf_scale_rows reads it
#pragma unroll
                    for (int j = 0; j < 8; ++j) ov[j] *= sc;
                    if (rv) *reinterpret_cast<lnl_u32x4*>(dxs + r0 * C + (eo + 32 * q)) = lnl_pack8(ov);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (KS != 1) load_tile(nxt);
        if (YX) __syncthreads();                                         // the four waves' rows of y are staged
        __builtin_amdgcn_sched_barrier(0);
        // ---- dW1 += dh^T y, db1 += colsum(dh): rows [H / 4 wave, + H / 4) over the tile's 64 tokens (two k-steps of 32)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            lnl_bf16x8 fa[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                fa[i] = lnl_frag_tok_tr(dhs + kk * 32 * RD, RD, rowbase + 16 * i, lane);
                uint32_t one2 = mi == i ? 0x3f803f80u : 0u;
                asm volatile("" : "+v"(one2));                           // (built here: kept across the loop the four selectors are 16 registers)
                const lnl_u32x4 sel = {one2, one2, one2, one2};
                ab = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], __builtin_bit_cast(lnl_bf16x8, sel), ab, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const lnl_bf16x8 fb = lnl_frag_tok_tr(ys + kk * 32 * RY, RY, 16 * (jbase + j), lane);
#pragma unroll
                for (int i = 0; i < NI; ++i) aw[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb, aw[i][j], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // ---- partials.  accumulator (i, j): rows H / 4 wave + 16 i + 4 g + r, column 16 j + mi
    float* pwb = pw + (int64_t)blockIdx.x * H * C;
    float* pbb = pb + (int64_t)blockIdx.x * H;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
#pragma unroll
        for (int rr_ = 0; rr_ < 4; ++rr_) {
            const int m = rowbase + 16 * i + 4 * g + rr_;
#pragma unroll
            for (int j = 0; j < NJ; ++j) pwb[m * C + 16 * (jbase + j) + mi] = aw[i][j][rr_];
        }
    }
    if (mi < NI && jbase == 0) {                                         // (QUAD: the two waves of a row tile hold the same column sums)
#pragma unroll
        for (int rr_ = 0; rr_ < 4; ++rr_) pbb[rowbase + 16 * mi + 4 * g + rr_] = ab[rr_];
    }
    // dgamma / dbeta: across the waves through LDS in fixed order
    __syncthreads();
    float* red = reinterpret_cast<float*>(dhs);                          // [4 waves][2][C]
    if (mi < 8 * KS) {
        red[(wave * 2 + 0) * C + 32 * (mi >> 3) + 8 * g + (mi & 7)] = accg;
        red[(wave * 2 + 1) * C + 32 * (mi >> 3) + 8 * g + (mi & 7)] = accb;
    }
    __syncthreads();
    if (tid < 2 * C) {
        float s = 0.f;
        for (int w = 0; w < 4; ++w) s += red[w * 2 * C + tid];
        pg[(int64_t)blockIdx.x * 2 * C + tid] = s;
    }
}

static inline int lnl_blocks(int64_t rows) { return (int)imin64(cdiv64(rows, 64), LNL_MAX_BLOCKS); }
// The shapes the fused form exists for and the sizes the policy sends to it (SEGFAC_LN_LINEAR_BWD_FUSED: 0 never, 1 from 131072 token
// rows on -- the recorded batch-4 step keeps its three launches --, 2 wherever the shape has the kernel)
extern "C" int segf_layernorm_linear_bwd_supported(int dt, int64_t rows, int C, int N) {
    const int pol = POL(ln_linear_bwd_fused);
    if (pol <= 0 || dt != SEGF_BF16 || (C != 32 && C != 64) || N != 4 * C) return 0;
    if (rows <= 0 || rows > 0x7fffffffll) return 0;
    return (pol >= 2 || rows >= 131072) ? 1 : 0;
}
extern "C" int segf_layernorm_linear_bwd_blocks(int64_t rows) { return rows > 0 ? lnl_blocks(rows) : 0; }
extern "C" int64_t segf_layernorm_linear_bwd_ws(int64_t rows, int C, int N) {
    return rows > 0 ? (int64_t)lnl_blocks(rows) * ((int64_t)N * C + N + 2 * C) : 0;
}
// The general entry point: N = 4 C or N = C, y nullable (NULL: rebuilt from x, mean, rstd, gamma and beta -- the forward then keeps no y),
// dy2 nullable (a second consumer's gradient of the LayerNorm output, in patch-major row order when log2_w >= 0, in token order otherwise).
extern "C" int segf_layernorm_linear_bwd_ex_supported(int dt, int64_t rows, int C, int N) {
    const int pol = POL(ln_linear_bwd_fused);
    if (pol <= 0 || dt != SEGF_BF16 || (C != 32 && C != 64) || (N != 4 * C && N != C)) return 0;
    if (rows <= 0 || rows > 0x7fffffffll) return 0;
    return (pol >= 2 || rows >= 131072) ? 1 : 0;
}
extern "C" int segf_layernorm_linear_bwd_ex(int dt, int64_t rows, int C, int N, const void* dh, const void* w1, const void* x, const void* y,
                                            const float* beta, const void* dy2, int log2_w, int log2_sr, const void* dres, const float* gamma,
                                            const float* mean, const float* rstd, void* dx, const float* rscale, int64_t rows_per_group, void* dxs,
                                            void* dy_out, float* dw1, float* db1, float* dgamma, float* dbeta, float* ws, void* stream) {
    if (dt != SEGF_BF16) return SEGF_ERR_DTYPE;
    if ((C != 32 && C != 64) || (N != 4 * C && N != C) || rows <= 0 || rows > 0x7fffffffll) return SEGF_ERR_SHAPE;
    if (y ? N != 4 * C : !beta) return SEGF_ERR_SHAPE;                   // a stored y: the norm2 -> fc1 form only
    if (dy2 && N != C) return SEGF_ERR_SHAPE;                            // the fan-in: norm1 -> q only (at C = 64 the hidden-width form has no registers for it)
    if (dy2 && log2_w >= 0 && !patch_geom_ok(rows, log2_w, log2_sr)) return SEGF_ERR_SHAPE;
    if ((rscale != nullptr) != (dxs != nullptr)) return SEGF_ERR_SHAPE;
    if (rscale && (rows_per_group <= 0 || rows_per_group > 0x7fffffffll)) return SEGF_ERR_SHAPE;
    if (((uintptr_t)dh % 16) || ((uintptr_t)w1 % 2) || ((uintptr_t)x % 16) || ((uintptr_t)y % 16) || ((uintptr_t)dres % 16) || ((uintptr_t)dy2 % 16) ||
        ((uintptr_t)gamma % 16) || ((uintptr_t)beta % 16) || ((uintptr_t)dx % 16) || ((uintptr_t)dxs % 16) || ((uintptr_t)dy_out % 16)) return SEGF_ERR_SHAPE;
    if (!ws) return SEGF_ERR_WORKSPACE;
    const bool now = dw1 != nullptr;                                     // NULL: deferred finalize (segf_colreduce_finalize_grouped on the three partial blocks)
    if (now ? (!db1 || !dgamma || dbeta != dgamma + C) : (db1 || dgamma || dbeta)) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = lnl_blocks(rows);
    float* pw = ws;
    float* pb = pw + (int64_t)blocks * N * C;
    float* pg = pb + (int64_t)blocks * N;
    const uint32_t rpg = rscale ? (uint32_t)rows_per_group : 1u;
    // the order in which segf_gemm (layout 1) sums K = 256 at this row count: gemm_skinny_k_kernel's quarters from 65536 rows on
    // (gemm.hip: gemm_skinny_k_ok), one chain on the 128-tile kernel below.  K = C <= 64 (N == C) is one chain at every row count.
    const int ksplit = N == 4 * C && C == 64 && rows >= 65536 && !POL(gemm_no_skinny_k) && !POL(gemm_no_skinny);
    const int lw = dy2 ? log2_w : -1;
    // C = 64 stages 75 KB: above the 64 KB a kernel gets by default, so the limit is raised on the function, once per device
#define LNL_GO(LDSB, ...) do { \
        static int lds_dev = -1; \
        int dev = -1; \
        if (LDSB > 65536 && !segf_trace().dry && hipGetDevice(&dev) == hipSuccess && dev != lds_dev) { \
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&__VA_ARGS__), hipFuncAttributeMaxDynamicSharedMemorySize, LDSB) != hipSuccess) return SEGF_ERR_SHAPE; \
            lds_dev = dev; \
        } \
        hipLaunchKernelGGL((__VA_ARGS__), dim3(blocks), dim3(256), LDSB, st, (const bf16_t*)dh, (const bf16_t*)w1, (const bf16_t*)x, \
                           (const bf16_t*)y, (const bf16_t*)dres, gamma, mean, rstd, (bf16_t*)dx, rscale, rpg, (bf16_t*)dxs, (bf16_t*)dy_out, pw, pb, pg, rows, ksplit, \
                           beta, (const bf16_t*)dy2, lw, log2_sr); } while (0)
#define LNL(KS_) LNL_GO((LnlGeom<KS_>::LDS_BYTES), ln_linear_bwd_kernel<KS_>)
#define LNLX(KS_, HM_, FAN_) LNL_GO((LnlGeom<KS_, HM_>::LDS_BYTES), ln_linear_bwd_kernel<KS_, true, HM_, FAN_>)
    if (y) { if (C == 32) LNL(1); else LNL(2); }
    else if (N == 4 * C) { if (C == 32) LNLX(1, 4, false); else LNLX(2, 4, false); }
    else {
        if (dy2) { if (C == 32) LNLX(1, 1, true); else LNLX(2, 1, true); }
        else { if (C == 32) LNLX(1, 1, false); else LNLX(2, 1, false); }
    }
#undef LNLX
#undef LNL
#undef LNL_GO
    SEGF_CHECK_LAUNCH();
    if (!now) return 0;
    colreduce_finalize_launch(pw, blocks, (int64_t)N * C, dw1, st);
    SEGF_CHECK_LAUNCH();
    colreduce_finalize_launch(pb, blocks, N, db1, st);
    SEGF_CHECK_LAUNCH();
    colreduce_finalize_launch(pg, blocks, 2 * (int64_t)C, dgamma, st);
    SEGF_CHECK_LAUNCH();
    return 0;
}
extern "C" int segf_layernorm_linear_bwd(int dt, int64_t rows, int C, int N, const void* dh, const void* w1, const void* x, const void* y,
                                         const void* dres, const float* gamma, const float* mean, const float* rstd, void* dx,
                                         const float* rscale, int64_t rows_per_group, void* dxs, void* dy_out, float* dw1, float* db1,
                                         float* dgamma, float* dbeta, float* ws, void* stream) {
    if (dt != SEGF_BF16) return SEGF_ERR_DTYPE;
    if (N != 4 * C || !y) return SEGF_ERR_SHAPE;
    return segf_layernorm_linear_bwd_ex(dt, rows, C, N, dh, w1, x, y, nullptr, nullptr, -1, 0, dres, gamma, mean, rstd, dx, rscale, rows_per_group, dxs,
                                        dy_out, dw1, db1, dgamma, dbeta, ws, stream);
}

// ---- LayerNorm as the operand prologue of the streaming thin product -------------------------------------------------------------
// `norm2 -> mlp.fc1` and `norm1 -> attn.q` of a MiT block (mit.py:45,98,136-146) at C = 32 / 64 as two launches write the C-wide LayerNorm
// output and read it back only to feed a product with K = C.  Here gemm_skinny_kernel's structure (gemm.hip, layout 0:
// weight fragments resident, a wave walks 16-token groups, the token rows ARE the MFMA B operand as they lie, the next group's rows in flight)
// takes the rows of x instead: lane (mi, g) holds features 32 s + 8 g .. + 7 of token mi, normalises them in registers and the bf16-rounded
// result is the B operand.  A token's chunks sit 16 lanes apart; the row sums pair them as ln_fwd_kernel's wave_sum(., lpr) does
// (xor 1, xor 2 on the chunk index = lanes 16 and 32 apart; at C = 64 then xor 4 = the lane's own second chunk).  The arithmetic is
// ln_fwd_kernel's as its gfx950 code performs it -- chunk sums from 0 in element order, mean = sum * (1 / C), squares of the differences as
// rounded products summed in element order, rstd = rsqrt(fma(sum, 1 / C, eps)), y = fma(gamma, (x - mean) * rstd, beta) -- with contraction
// off and the fused operations spelled out, so that mean, rstd and the rounded y carry that kernel's bits whatever the optimiser would choose
// here.  The product is gemm_skinny_kernel's chain (zero accumulator, K steps ascending, + bias, one rounding).  N = 16 NT NCH: NCH > 1
// (C = 64 -> 256: 32 fragments) keeps the fragments in LDS and loops the column chunks over the rows already normalised.
// Optional outputs: y in token order (HASY) and in patch-major row order (HASY2: segf_layernorm_fwd_patch's y2).
__device__ __forceinline__ float lnf_sum8(const float (&v)[8]) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s = s + v[j];
    return s;
}
__device__ __forceinline__ float lnf_sq8(const float (&v)[8], float mu) {
#pragma clang fp contract(off)
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float d = v[j] - mu; const float dd = d * d; q = q + dd; }
    return q;
}
__device__ __forceinline__ float lnf_mean(float s, float invC) {
#pragma clang fp contract(off)
    return s * invC;
}
__device__ __forceinline__ float lnf_rstd(float q, float invC, float eps) {
#pragma clang fp contract(off)
    return rsqrtf(__builtin_fmaf(q, invC, eps));
}
__device__ __forceinline__ void lnf_y8(const float (&v)[8], const float (&g)[8], const float (&b)[8], float mu, float rs, float (&o)[8]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float t = (v[j] - mu) * rs; o[j] = __builtin_fmaf(g[j], t, b[j]); }
}
template <int KS, int NT, int NCH, bool HASY, bool HASY2>
__global__ void __launch_bounds__(256) ln_linear_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const bf16_t* __restrict__ w /*[N][C]*/, const float* __restrict__ bias,
                                                             bf16_t* __restrict__ out /*[rows][N]*/, float* __restrict__ mean_out,
                                                             float* __restrict__ rstd_out, bf16_t* __restrict__ y, bf16_t* __restrict__ y2,
                                                             int64_t rows, float eps, int lw, int ls) {
    constexpr int C = 32 * KS, N = 16 * NT * NCH;
    constexpr bool WREG = NCH == 1;                                     // NT * KS <= 16 fragments: register-resident
    static_assert(!WREG || NT * KS <= 16, "fragment budget");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mi = lane & 15, g = lane >> 4;
    constexpr int SROW = 32 * NT + 16;                                  // staged output row bytes (+16: bank spread)
    __shared__ __attribute__((aligned(16))) unsigned char ostage[4][16 * SROW];
    __shared__ __attribute__((aligned(16))) unsigned char wl[WREG ? 16 : 1024 * NT * KS * NCH];
    __shared__ __attribute__((aligned(16))) float bl[WREG ? 4 : N];
    unsigned char* ost = ostage[wave];
    // weight fragments: MFMA row i of tile nt carries feature n0 + 32 (nt >> 1) + 8 (i >> 2) + 4 (nt & 1) + (i & 3) (gemm_skinny_kernel)
    lnl_bf16x8 Wf[WREG ? NT : 1][KS];
    float bv[WREG ? NT : 1][4];
    if (WREG) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = 32 * (nt >> 1) + 8 * (mi >> 2) + 4 * (nt & 1) + (mi & 3);
#pragma unroll
            for (int s = 0; s < KS; ++s) Wf[nt][s] = __builtin_bit_cast(lnl_bf16x8, *reinterpret_cast<const lnl_u32x4*>(w + n * C + 32 * s + 8 * g));
#pragma unroll
            for (int r = 0; r < 4; ++r) bv[nt][r] = bias[32 * (nt >> 1) + 8 * g + 4 * (nt & 1) + r];
        }
    } else {
        for (int f = wave; f < NT * KS * NCH; f += 4) {                 // fragment (ch, nt, s) at 1 KB * ((ch NT + nt) KS + s)
            const int s = f % KS, cn = f / KS, ch = cn / NT, nt = cn - ch * NT;
            const int n = 16 * NT * ch + 32 * (nt >> 1) + 8 * (mi >> 2) + 4 * (nt & 1) + (mi & 3);
            *reinterpret_cast<lnl_u32x4*>(wl + 1024 * f + 16 * lane) = *reinterpret_cast<const lnl_u32x4*>(w + n * C + 32 * s + 8 * g);
        }
        for (int i = threadIdx.x; i < N; i += 256) bl[i] = bias[i];
        __syncthreads();
    }
    float gm[KS][8], bt[KS][8];
#pragma unroll
    for (int s = 0; s < KS; ++s) { load8f(gamma + 32 * s + 8 * g, gm[s]); load8f(beta + 32 * s + 8 * g, bt[s]); }
    const float invC = 1.f / (float)C;
    const int64_t ngroups = (rows + 15) / 16, gstride = (int64_t)gridDim.x * 4;
    int64_t grp = (int64_t)blockIdx.x * 4 + wave;
    lnl_u32x4 xa[KS], xb[KS];
    auto rowptr = [&](int64_t gp) {
        int64_t m = gp * 16 + mi;
        m = m < rows ? m : rows - 1;
        return x + m * C + 8 * g;
    };
    {
        const bf16_t* p = rowptr(grp < ngroups ? grp : 0);
#pragma unroll
        for (int s = 0; s < KS; ++s) xa[s] = *reinterpret_cast<const lnl_u32x4*>(p + 32 * s);
    }
    // One group of 16 tokens; FULL = every row exists (all loads and stores of the main loop unconditional, as in gemm_skinny_kernel)
    auto one_group = [&](int64_t gp, auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        {
            const int64_t nxt = gp + gstride;
            const bf16_t* p = rowptr(nxt < ngroups ? nxt : gp);           // unconditional (the last one re-reads)
#pragma unroll
            for (int s = 0; s < KS; ++s) xb[s] = *reinterpret_cast<const lnl_u32x4*>(p + 32 * s);
            SEGF_LOADS_ISSUED();
        }
        const int64_t m = gp * 16 + mi;
        const bool mok = FULL || m < rows;
        // ---- LayerNorm of the lane's token
        float v[KS][8], ps[KS], pq[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            lnl_unpack8(xa[s], v[s]);
            ps[s] = lnf_sum8(v[s]);
            ps[s] += __shfl_xor(ps[s], 16, 64); ps[s] += __shfl_xor(ps[s], 32, 64);
        }
        float tot = ps[0];
        if (KS == 2) tot += ps[KS - 1];
        const float mu = lnf_mean(tot, invC);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            pq[s] = lnf_sq8(v[s], mu);
            pq[s] += __shfl_xor(pq[s], 16, 64); pq[s] += __shfl_xor(pq[s], 32, 64);
        }
        float qt = pq[0];
        if (KS == 2) qt += pq[KS - 1];
        const float rs = lnf_rstd(qt, invC, eps);
        lnl_u32x4 yb[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            float o[8];
            lnf_y8(v[s], gm[s], bt[s], mu, rs, o);
            yb[s] = lnl_pack8(o);
        }
        if (mok) {
            if (g == 0) { mean_out[m] = mu; rstd_out[m] = rs; }
            if (HASY) {
#pragma unroll
                for (int s = 0; s < KS; ++s) *reinterpret_cast<lnl_u32x4*>(y + m * C + 32 * s + 8 * g) = yb[s];
            }
            if (HASY2) {
                bf16_t* p2 = y2 + patch_row(m, lw, ls) * C + 8 * g;
#pragma unroll
                for (int s = 0; s < KS; ++s) *reinterpret_cast<lnl_u32x4*>(p2 + 32 * s) = yb[s];
            }
        }
        // ---- the product, a column chunk of 16 NT features at a time
#pragma unroll 1
        for (int ch = 0; ch < NCH; ++ch) {
            lnl_f32x4 acc[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                acc[nt] = lnl_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    lnl_bf16x8 wf;
                    if (WREG) wf = Wf[nt][s];
                    else wf = *reinterpret_cast<const lnl_bf16x8*>(wl + 1024 * ((ch * NT + nt) * KS + s) + 16 * lane);
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, __builtin_bit_cast(lnl_bf16x8, yb[s]), acc[nt], 0, 0, 0);
                }
            }
#pragma unroll
            for (int q = 0; q < NT / 2; ++q) {
                float b0[4], b1[4], o[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    b0[r] = WREG ? bv[2 * q][r] : bl[16 * NT * ch + 32 * q + 8 * g + r];
                    b1[r] = WREG ? bv[2 * q + 1][r] : bl[16 * NT * ch + 32 * q + 8 * g + 4 + r];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) { o[r] = acc[2 * q][r] + b0[r]; o[4 + r] = acc[2 * q + 1][r] + b1[r]; }
                *reinterpret_cast<lnl_u32x4*>(ost + mi * SROW + (32 * q + 8 * g) * 2) = lnl_pack8(o);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            {
                constexpr int CPR = 2 * NT;                              // 16-byte chunks per staged row
#pragma unroll
                for (int i = 0; i < (16 * CPR) / 64; ++i) {
                    const int idx = lane + 64 * i, row = idx / CPR, cc = idx - row * CPR;
                    const lnl_u32x4 o = *reinterpret_cast<const lnl_u32x4*>(ost + row * SROW + 16 * cc);
                    const int64_t mr = gp * 16 + row;
                    if (FULL || mr < rows) *reinterpret_cast<lnl_u32x4*>(out + mr * N + 16 * NT * ch + 8 * cc) = o;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            xa[s] = xb[s];
            asm volatile("" : "+v"(xa[s]));       // keep the copy (and its counted wait) here, behind this group's stores
        }
    };
    const int64_t nfull = rows / 16;                                      // groups whose 16 rows all exist
    // everything loaded so far is consumed here once (gemm_skinny_kernel: otherwise the loop header waits for the previous group's stores)
    if (WREG) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int s2 = 0; s2 < KS; ++s2) asm volatile("" : "+v"(Wf[nt][s2]));
#pragma unroll
            for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(bv[nt][r]));
        }
    }
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
        asm volatile("" : "+v"(xa[s2]));
#pragma unroll
        for (int j = 0; j < 8; ++j) { asm volatile("" : "+v"(gm[s2][j])); asm volatile("" : "+v"(bt[s2][j])); }
    }
    for (; grp < nfull; grp += gstride) one_group(grp, std::true_type{});
    if (grp < ngroups) one_group(grp, std::false_type{});                 // at most one ragged group, in one wave
}

static inline int lnf_blocks(int64_t rows) { return (int)imin64(cdiv64(cdiv64(rows, 16), 4 * 4), 2048); }     // >= 4 token groups per wave, as the product it replaces
// The shapes the fused forward exists for and the sizes the policy sends to it (SEGFAC_LN_LINEAR_FWD_FUSED: 0 never, 1 from 131072 token
// rows on -- the recorded batch-4 step keeps its two launches --, 2 wherever the shape has the kernel)
extern "C" int segf_layernorm_linear_fwd_supported(int dt, int64_t rows, int C, int N) {
    const int pol = POL(ln_linear_fwd_fused);
    if (pol <= 0 || dt != SEGF_BF16 || (C != 32 && C != 64) || (N != C && N != 4 * C)) return 0;
    if (rows <= 0 || rows > 0x7fffffffll) return 0;
    return (pol >= 2 || rows >= 131072) ? 1 : 0;
}
extern "C" int segf_layernorm_linear_fwd_blocks(int64_t rows) { return rows > 0 ? lnf_blocks(rows) : 0; }
extern "C" int segf_layernorm_linear_fwd(int dt, int64_t rows, int C, int N, const void* x, const float* gamma, const float* beta, float eps,
                                         const void* w, const float* bias, void* out, float* mean, float* rstd, void* y, void* y2, int log2_w,
                                         int log2_sr, void* stream) {
    if (dt != SEGF_BF16) return SEGF_ERR_DTYPE;
    if ((C != 32 && C != 64) || (N != C && N != 4 * C) || rows <= 0 || rows > 0x7fffffffll) return SEGF_ERR_SHAPE;
    if (!x || !gamma || !beta || !w || !bias || !out || !mean || !rstd) return SEGF_ERR_SHAPE;
    if (y2 && !patch_geom_ok(rows, log2_w, log2_sr)) return SEGF_ERR_SHAPE;
    if (((uintptr_t)x % 16) || ((uintptr_t)gamma % 16) || ((uintptr_t)beta % 16) || ((uintptr_t)w % 16) || ((uintptr_t)bias % 4) ||
        ((uintptr_t)out % 16) || ((uintptr_t)y % 16) || ((uintptr_t)y2 % 16)) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = lnf_blocks(rows);
#define LNF_GO(KS_, NT_, NCH_, Y_, Y2_) hipLaunchKernelGGL((ln_linear_fwd_kernel<KS_, NT_, NCH_, Y_, Y2_>), dim3(blocks), dim3(256), 0, st, (const bf16_t*)x, gamma, beta, \
                           (const bf16_t*)w, bias, (bf16_t*)out, mean, rstd, (bf16_t*)y, (bf16_t*)y2, rows, eps, log2_w, log2_sr)
#define LNF(KS_, NT_, NCH_) do { if (y) { if (y2) LNF_GO(KS_, NT_, NCH_, true, true); else LNF_GO(KS_, NT_, NCH_, true, false); } \
                                 else { if (y2) LNF_GO(KS_, NT_, NCH_, false, true); else LNF_GO(KS_, NT_, NCH_, false, false); } } while (0)
    // (K, N) -> the NT of the gemm_skinny_kernel<0, KS, NT> that segf_gemm takes for it (gemm.hip: gemm_skinny_nt)
    if (C == 32 && N == 32) LNF(1, 2, 1);
    else if (C == 32) LNF(1, 8, 1);
    else if (N == 64) LNF(2, 4, 1);
    else LNF(2, 8, 2);
#undef LNF
#undef LNF_GO
    SEGF_CHECK_LAUNCH();
    return 0;
}

// ---- BatchNorm on NHWC rows ---------------------------------------------------------------------------------
// Accuracy of the statistics: the variance is E[x^2] - mean^2 from fp32 sums of x and x^2 (combined in double), so it is as accurate as
// those sums allow and its relative error grows as (mean / sigma)^2 (tests/test_norm_float64.py pins this).
template <typename T> struct BnStatF {
    const T* x; int C; bool vec;
    struct Col {};
    __device__ void init(int, int, Col&) const {}
    __device__ void operator()(const Col&, int64_t r, int c0, int nv, float (&v)[2][8]) const {
        load8_guard<T>(x + r * C + c0, nv, vec, v[0]);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[1][j] = v[0][j] * v[0][j];
    }
};

// sums[2][C] -> mean, rstd, running stats (fp64 combine: E[x^2]-mean^2 is formed in double)
__global__ void bn_finalize_kernel(const float* __restrict__ sums, int C, double n, float eps, float momentum,
                                   float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ rmean,
                                   float* __restrict__ rvar) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double mu = (double)sums[c] / n;
    double var = (double)sums[C + c] / n - mu * mu;
    if (var < 0) var = 0;
    mean[c] = (float)mu;
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (rmean) {
        const double unb = n > 1 ? var * n / (n - 1) : var;
        rmean[c] = (1.f - momentum) * rmean[c] + momentum * (float)mu;
        rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unb;
    }
}

extern "C" int64_t segf_bn_ws(int64_t rows, int C) { return cr_ws_floats(rows, C, 2) + 2 * (int64_t)C; }

extern "C" int segf_bn_stats(int dt, int64_t rows, int C, const void* x, float* mean, float* rstd, float* running_mean,
                             float* running_var, float momentum, float eps, float* ws, void* stream) {
    if (rows <= 0 || C <= 0) return SEGF_ERR_SHAPE;
    if (!ws) return SEGF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* sums = ws + cr_ws_floats(rows, C, 2);
    SEGF_DISPATCH_DT(dt, T, {
        BnStatF<T> f{(const T*)x, C, vec_ok_host<T>(x, C)};
        const int rc = colreduce_launch<2>(f, rows, C, ws, sums, st);
        if (rc) return rc;
    })
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, st, sums, C, (double)rows, eps, momentum, mean,
                       rstd, running_mean, running_var);
    SEGF_CHECK_LAUNCH();
    return 0;
}

// mean / rstd / running statistics from per-channel sums [2][C] = (sum x, sum x^2) produced elsewhere (segf_upsample_add_stats)
extern "C" int segf_bn_stats_from_sums(const float* sums, int64_t rows, int C, float* mean, float* rstd, float* running_mean,
                                       float* running_var, float momentum, float eps, void* stream) {
    if (rows <= 0 || C <= 0 || !sums) return SEGF_ERR_SHAPE;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, sums, C, (double)rows, eps,
                       momentum, mean, rstd, running_mean, running_var);
    SEGF_CHECK_LAUNCH();
    return 0;
}

__device__ __forceinline__ float bn_act(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return fminf(fmaxf(v, 0.f), 6.f);
    return v;
}
__device__ __forceinline__ float bn_act_mask(float pre, int act) {
    if (act == 1) return pre > 0.f ? 1.f : 0.f;
    if (act == 2) return (pre > 0.f && pre < 6.f) ? 1.f : 0.f;
    return 1.f;
}

// y = act(a * x + b) * chan_scale, a = gamma * rstd, b = beta - mean * a: column-fixed threads, parameters in registers
template <typename T>
__global__ void __launch_bounds__(256) bn_apply_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int act, const float* __restrict__ cscale,
                                                        FastDivU32 rps, T* __restrict__ y, int64_t rows, int C, bool vec) {
    const int nchunk = (C + 7) / 8;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t T_ = (int64_t)gridDim.x * 256;
    const int ch = (int)(g % nchunk);
    const int64_t rstep = T_ / nchunk;
    const int c0 = ch * 8;
    const int nv = C - c0 < 8 ? C - c0 : 8;
    float a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + (j < nv ? j : 0);
        a[j] = gamma[c] * rstd[c];
        b[j] = beta[c] - mean[c] * a[j];
    }
    // the row loop is instantiated under `full 16-byte-aligned chunk` and under its negation, so that the guarded accesses of
    // the first copy fold to plain vector loads / stores (see colreduce_kernel)
    auto row_loop = [&](const int nvv, const bool vv) {
#pragma unroll 2
        for (int64_t r = g / nchunk; r < rows; r += rstep) {
            float v[8];
            load8_guard<T>(x + r * C + c0, nvv, vv, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = bn_act(fmaf(v[j], a[j], b[j]), act);
            if (cscale) {
                float cs[8];
                load8_guard<float>(cscale + (int64_t)fastdiv((uint32_t)r, rps) * C + c0, nvv, vv, cs);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] *= cs[j];
            }
            store8_guard<T>(y + r * C + c0, nvv, vv, v);
        }
    };
    if (nv >= 8 && vec) row_loop(8, true); else row_loop(nv, vec);
}

extern "C" int segf_bn_apply(int dt, int64_t rows, int C, const void* x, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, int act, const float* chan_scale,
                             int64_t rows_per_sample, void* y, void* stream) {
    if (rows <= 0 || C <= 0) return 0;
    if (chan_scale && rows_per_sample <= 0) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = colfixed_blocks(rows, (C + 7) / 8, 4, 8192);
    SEGF_DISPATCH_DT(dt, T, {
        const bool vec = vec_ok_host<T>(x, C) && vec_ok_host<T>(y, C) && (C % 8 == 0);
        hipLaunchKernelGGL((bn_apply_kernel<T>), dim3(blocks), dim3(256), 0, st, (const T*)x, mean, rstd, gamma, beta, act,
                           chan_scale, fastdiv_make((uint32_t)(rows_per_sample > 0 ? rows_per_sample : 1)), (T*)y, rows, C, vec);
    })
    SEGF_CHECK_LAUNCH();
    return 0;
}

// BatchNorm (+ Dropout2d channel scale) as per-(sample, channel) affine tables for segf_gemm_pro:
//   scale[g][c] = gamma rstd cs[g][c],  shift[g][c] = (beta - mean gamma rstd) cs[g][c]
// cs >= 0, so ReLU(a x + b) cs == ReLU(cs a x + cs b): the consumer applies the activation after the scaled affine.
__global__ void bn_affine_table_kernel(const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
                                       const float* __restrict__ beta, const float* __restrict__ cs, int G, int C,
                                       float* __restrict__ scale, float* __restrict__ shift) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G * C) return;
    const int c = i % C;
    const float a = gamma[c] * rstd[c], s = cs ? cs[i] : 1.f;
    scale[i] = a * s;
    shift[i] = (beta[c] - mean[c] * a) * s;
}
extern "C" int segf_bn_affine_table(const float* mean, const float* rstd, const float* gamma, const float* beta,
                                    const float* chan_scale, int groups, int C, float* scale, float* shift, void* stream) {
    if (groups <= 0 || C <= 0) return SEGF_ERR_SHAPE;
    hipLaunchKernelGGL(bn_affine_table_kernel, dim3((groups * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, mean, rstd, gamma,
                       beta, chan_scale, groups, C, scale, shift);
    SEGF_CHECK_LAUNCH();
    return 0;
}

// backward sums: [0] = sum dyr, [1] = sum dyr * xhat, where dyr = dy * chan_scale * act'(pre)
struct BnCol { float mean[8], rstd[8], a[8], b[8]; };
__device__ __forceinline__ void bn_col_init(const float* mean, const float* rstd, const float* gamma, const float* beta, int c0,
                                            int nv, BnCol& col) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + (j < nv ? j : 0);
        col.mean[j] = mean[c]; col.rstd[j] = rstd[c];
        col.a[j] = gamma[c]; col.b[j] = beta[c];
    }
}
template <typename T> struct BnBwdF {
    const T* x; const T* dy; const float* mean; const float* rstd; const float* gamma; const float* beta;
    const float* cscale; FastDivU32 rps; int C; int act; bool vec;
    typedef BnCol Col;
    __device__ void init(int c0, int nv, Col& col) const { bn_col_init(mean, rstd, gamma, beta, c0, nv, col); }
    __device__ void operator()(const Col& col, int64_t r, int c0, int nv, float (&v)[2][8]) const {
        float xv[8], dv[8], cs[8];
        load8_guard<T>(x + r * C + c0, nv, vec, xv);
        load8_guard<T>(dy + r * C + c0, nv, vec, dv);
        if (cscale) load8_guard<float>(cscale + (int64_t)fastdiv((uint32_t)r, rps) * C + c0, nv, vec, cs);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float xh = (xv[j] - col.mean[j]) * col.rstd[j];
            float d = dv[j] * bn_act_mask(fmaf(xh, col.a[j], col.b[j]), act);
            if (cscale) d *= cs[j];
            v[0][j] = j < nv ? d : 0.f;
            v[1][j] = j < nv ? d * xh : 0.f;
        }
    }
};

template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, int act,
                                                            const float* __restrict__ cscale, FastDivU32 rps,
                                                            const float* __restrict__ sums /*[2][C]: dbeta, dgamma*/,
                                                            int eval_mode, T* __restrict__ dx, int64_t rows, int C, bool vec) {
    const int nchunk = (C + 7) / 8;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t T_ = (int64_t)gridDim.x * 256;
    const int ch = (int)(g % nchunk);
    const int64_t rstep = T_ / nchunk;
    const int c0 = ch * 8;
    const int nv = C - c0 < 8 ? C - c0 : 8;
    const float invn = 1.f / (float)rows;
    BnCol col;
    bn_col_init(mean, rstd, gamma, beta, c0, nv, col);
    float k1[8], k2[8], gr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + (j < nv ? j : 0);
        k1[j] = eval_mode ? 0.f : sums[c] * invn;
        k2[j] = eval_mode ? 0.f : sums[C + c] * invn;
        gr[j] = col.a[j] * col.rstd[j];
    }
    auto row_loop = [&](const int nvv, const bool vv) {
#pragma unroll 2
        for (int64_t r = g / nchunk; r < rows; r += rstep) {
            float xv[8], dv[8], cs[8];
            load8_guard<T>(x + r * C + c0, nvv, vv, xv);
            load8_guard<T>(dy + r * C + c0, nvv, vv, dv);
            if (cscale) load8_guard<float>(cscale + (int64_t)fastdiv((uint32_t)r, rps) * C + c0, nvv, vv, cs);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float xh = (xv[j] - col.mean[j]) * col.rstd[j];
                float d = dv[j] * bn_act_mask(fmaf(xh, col.a[j], col.b[j]), act);
                if (cscale) d *= cs[j];
                xv[j] = gr[j] * (d - k1[j] - xh * k2[j]);
            }
            store8_guard<T>(dx + r * C + c0, nvv, vv, xv);
        }
    };
    if (nv >= 8 && vec) row_loop(8, true); else row_loop(nv, vec);
}

// dgamma = sums[1], dbeta = sums[0] are produced in-place: caller passes dbeta = ws-resident [C], dgamma [C]
__global__ void bn_copy_grads_kernel(const float* __restrict__ sums, int C, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    dbeta[c] = sums[c];
    dgamma[c] = sums[C + c];
}

extern "C" int segf_bn_bwd(int dt, int64_t rows, int C, const void* x, const void* dy, const float* mean, const float* rstd,
                           const float* gamma, const float* beta, int act, const float* chan_scale, int64_t rows_per_sample,
                           int eval_mode, void* dx, float* dgamma, float* dbeta, float* ws, void* stream) {
    if (rows <= 0 || C <= 0) return SEGF_ERR_SHAPE;
    if (!ws) return SEGF_ERR_WORKSPACE;
    if (chan_scale && rows_per_sample <= 0) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    float* sums = ws + cr_ws_floats(rows, C, 2);
    if (rows > 0xffffffffll) return SEGF_ERR_SHAPE;
    const FastDivU32 rps = fastdiv_make((uint32_t)(rows_per_sample > 0 ? rows_per_sample : 1));
    const int blocks = colfixed_blocks(rows, (C + 7) / 8, 4, 8192);
    SEGF_DISPATCH_DT(dt, T, {
        const bool vec = vec_ok_host<T>(x, C) && vec_ok_host<T>(dy, C) && vec_ok_host<T>(dx, C) && (C % 8 == 0);
        BnBwdF<T> f{(const T*)x, (const T*)dy, mean, rstd, gamma, beta, chan_scale, rps, C, act, vec};
        const int rc = colreduce_launch<2>(f, rows, C, ws, sums, st);
        if (rc) return rc;
        hipLaunchKernelGGL((bn_bwd_apply_kernel<T>), dim3(blocks), dim3(256), 0, st, (const T*)x, (const T*)dy, mean, rstd,
                           gamma, beta, act, chan_scale, rps, sums, eval_mode, (T*)dx, rows, C, vec);
    })
    SEGF_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_copy_grads_kernel, dim3((C + 255) / 256), dim3(256), 0, st, sums, C, dgamma, dbeta);
    SEGF_CHECK_LAUNCH();
    return 0;
}


// ---- Global Response Normalization (ConvNeXtV2, models/backbones/convnextv2.py:68-80) on NHWC rows -----------------------
//   Gx[b][c] = ||x[b,:,:,c]||_2 ;  Nx = Gx / (mean_c Gx + 1e-6) ;  y = gamma * (x * Nx) + beta + x = a[b][c] * x + beta[c]
// forward : batched column reduction (sum x^2) -> per-image coefficient kernel -> streaming apply
// backward: batched column reduction (sum dy*x, sum dy) -> coefficient kernel -> dx = a * dy + K * x, with
//           K[b][c] = dL/dGx / Gx,  dL/dGx[c] = A[c]/(m+eps) - (1/C) sum_c' A[c'] Gx[c'] / (m+eps)^2,  A = gamma * sum_p dy*x
#define GRN_EPS 1e-6f
// ACT: the GRN input is gelu(x) of what is stored (ConvNeXtV2: pwconv1 -> GELU -> GRN, convnextv2.py:92-94): the activation is
// applied on the way in, in fp32, and gelu(x) is never written -- the pre-activation is what the GELU backward needs anyway.
template <typename T, bool ACT = false> struct GrnSqF {
    const T* x; int C; bool vec;
    struct Col {};
    __device__ void init(int, int, Col&) const {}
    __device__ void operator()(const Col&, int64_t r, int c0, int nv, float (&v)[1][8]) const {
        load8_guard<T>(x + r * C + c0, nv, vec, v[0]);
        if (ACT) gelu_erf8_floats(v[0]);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[0][j] *= v[0][j];
    }
};
template <typename T, bool ACT = false> struct GrnBwdF {
    const T* x; const T* dy; int C; bool vec;
    struct Col {};
    __device__ void init(int, int, Col&) const {}
    __device__ void operator()(const Col&, int64_t r, int c0, int nv, float (&v)[2][8]) const {
        float xv[8];
        load8_guard<T>(x + r * C + c0, nv, vec, xv);
        load8_guard<T>(dy + r * C + c0, nv, vec, v[1]);
        if (ACT) gelu_erf8_floats(xv);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[0][j] = v[1][j] * xv[j];
    }
};
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum_all(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// one block per image.  fwd (S1 == nullptr): a[b][c] = 1 + gamma Nx, stash Gx.  bwd: also K[b][c] and per-image dgamma parts.
__global__ void __launch_bounds__(256) grn_coef_kernel(const float* __restrict__ sumsq, const float* __restrict__ gamma, int C,
                                                        float* __restrict__ a, float* __restrict__ G_out,
                                                        const float* __restrict__ S1, float* __restrict__ K, float* __restrict__ dg_part) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    const float* sq = sumsq + (int64_t)b * C;
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) s += sqrtf(sq[c]);
    const float m = block_sum_256(s, red) / (float)C;
    const float inv = 1.f / (m + GRN_EPS);
    float t = 0.f;
    if (S1)
        for (int c = threadIdx.x; c < C; c += 256) t += gamma[c] * S1[(int64_t)b * 2 * C + c] * sqrtf(sq[c]);
    const float AG = S1 ? block_sum_256(t, red) : 0.f;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float G = sqrtf(sq[c]);
        const float nx = G * inv;
        a[(int64_t)b * C + c] = 1.f + gamma[c] * nx;
        if (G_out) G_out[(int64_t)b * C + c] = sq[c];       // saved for the backward: per-image sum of squares
        if (S1) {
            const float s1 = S1[(int64_t)b * 2 * C + c];
            const float dG = gamma[c] * s1 * inv - AG * inv * inv / (float)C;
            K[(int64_t)b * C + c] = G > 0.f ? dG / G : 0.f;
            dg_part[(int64_t)b * C + c] = nx * s1;
        }
    }
}
// y = a[b][c] * x + (k ? k[b][c] * x2 : beta[c])     fwd: (x, a, beta);  bwd: dx = a * dy + K * x  (x := dy, x2 := x)
// ACT (see GrnSqF): fwd y = a * gelu(x) + beta;  bwd (x := dy, x2 := the stored pre-activation u): du = (a * dy + K * gelu(u)) * gelu'(u)
template <typename T, bool ACT = false>
__global__ void __launch_bounds__(256) grn_apply_kernel(const T* __restrict__ x, const T* __restrict__ x2, const float* __restrict__ a,
                                                         const float* __restrict__ k, const float* __restrict__ beta, T* __restrict__ y,
                                                         int64_t rows, FastDivU32 rps, int C) {
    const int nchunk = C / 8;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rstep = ((int64_t)gridDim.x * 256) / nchunk;
    const int c0 = (int)(g % nchunk) * 8;
    float bt[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bt[j] = beta ? beta[c0 + j] : 0.f;
    for (int64_t r = g / nchunk; r < rows; r += rstep) {
        const int64_t b = fastdiv((uint32_t)r, rps);
        float v[8], av[8];
        load8<T>(x + r * C + c0, v);
        load8f(a + b * C + c0, av);
        if (k) {
            float w[8], kv[8];
            load8<T>(x2 + r * C + c0, w);
            load8f(k + b * C + c0, kv);
            if (ACT) {
                f32x2_t u2[4] = {f32x2_t{w[0], w[1]}, f32x2_t{w[2], w[3]}, f32x2_t{w[4], w[5]}, f32x2_t{w[6], w[7]}}, g2[4];
                gelu_erf8_both(u2, g2);                       // g2 = gelu(u), u2 = gelu'(u)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[2 * i] = fmaf(av[2 * i], v[2 * i], kv[2 * i] * g2[i].x) * u2[i].x;
                    v[2 * i + 1] = fmaf(av[2 * i + 1], v[2 * i + 1], kv[2 * i + 1] * g2[i].y) * u2[i].y;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = fmaf(av[j], v[j], kv[j] * w[j]);
            }
        } else {
            if (ACT) gelu_erf8_floats(v);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = fmaf(av[j], v[j], bt[j]);
        }
        store8<T>(y + r * C + c0, v);
    }
}
// dgamma[c] = sum_b dg_part[b][c], dbeta[c] = sum_b S[b][1][c]
__global__ void grn_param_grads_kernel(const float* __restrict__ dg_part, const float* __restrict__ S, int B, int C,
                                       float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float g = 0.f, bsum = 0.f;
    for (int b = 0; b < B; ++b) { g += dg_part[(int64_t)b * C + c]; bsum += S[((int64_t)b * 2 + 1) * C + c]; }
    dgamma[c] = g; dbeta[c] = bsum;
}

// workspace (floats): forward B*cr_ws(rows,C,1) + B*C; backward B*cr_ws(rows,C,2) + 4*B*C
extern "C" int64_t segf_grn_ws(int B, int64_t rows_per_sample, int C, int bwd) {
    return (int64_t)B * cr_ws_floats(rows_per_sample, C, bwd ? 2 : 1) + (bwd ? 4 : 1) * (int64_t)B * C;
}
// y = gamma * (x * Nx) + beta + x;  a_out [B][C] (scratch) and g_out [B][C] (sum_p x^2, saved for the backward)
extern "C" int segf_grn_fwd(int dt, int B, int64_t rows_per_sample, int C, const void* x, const float* gamma, const float* beta,
                            void* y, float* a_out, float* g_out, float* ws, int pre_gelu, void* stream) {
    if (B <= 0 || rows_per_sample <= 0) return 0;
    if (C <= 0 || C % 8 || ((uintptr_t)x % 16) || ((uintptr_t)y % 16)) return SEGF_ERR_SHAPE;
    if (!ws) return SEGF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* sumsq = ws + (int64_t)B * cr_ws_floats(rows_per_sample, C, 1);
    const int64_t rows = (int64_t)B * rows_per_sample;
    SEGF_DISPATCH_DT(dt, T, {
        int rc;
        if (pre_gelu) { GrnSqF<T, true> f{(const T*)x, C, true}; rc = colreduce_launch_batched<1>(f, rows_per_sample, B, C, ws, sumsq, st); }
        else { GrnSqF<T, false> f{(const T*)x, C, true}; rc = colreduce_launch_batched<1>(f, rows_per_sample, B, C, ws, sumsq, st); }
        if (rc) return rc;
        hipLaunchKernelGGL(grn_coef_kernel, dim3(B), dim3(256), 0, st, sumsq, gamma, C, a_out, g_out, (const float*)nullptr,
                           (float*)nullptr, (float*)nullptr);
        const dim3 grid(colfixed_blocks(rows, C / 8, 4, 8192));
        if (pre_gelu) hipLaunchKernelGGL((grn_apply_kernel<T, true>), grid, dim3(256), 0, st, (const T*)x,
                           (const T*)nullptr, a_out, (const float*)nullptr, beta, (T*)y, rows, fastdiv_make((uint32_t)rows_per_sample), C);
        else hipLaunchKernelGGL((grn_apply_kernel<T, false>), grid, dim3(256), 0, st, (const T*)x,
                           (const T*)nullptr, a_out, (const float*)nullptr, beta, (T*)y, rows, fastdiv_make((uint32_t)rows_per_sample), C);
    })
    SEGF_CHECK_LAUNCH();
    return 0;
}
extern "C" int segf_grn_bwd(int dt, int B, int64_t rows_per_sample, int C, const void* x, const void* dy, const float* gamma,
                            const float* g_saved, void* dx, float* dgamma, float* dbeta, float* ws, int pre_gelu, void* stream) {
    if (B <= 0 || rows_per_sample <= 0) return 0;
    if (C <= 0 || C % 8 || ((uintptr_t)x % 16) || ((uintptr_t)dy % 16) || ((uintptr_t)dx % 16)) return SEGF_ERR_SHAPE;
    if (!ws) return SEGF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* S = ws + (int64_t)B * cr_ws_floats(rows_per_sample, C, 2);      // [B][2][C]: sum dy*x, sum dy
    float* a = S + 2 * (int64_t)B * C;
    float* K = a + (int64_t)B * C;
    const int64_t rows = (int64_t)B * rows_per_sample;
    SEGF_DISPATCH_DT(dt, T, {
        int rc;
        if (pre_gelu) { GrnBwdF<T, true> f{(const T*)x, (const T*)dy, C, true}; rc = colreduce_launch_batched<2>(f, rows_per_sample, B, C, ws, S, st); }
        else { GrnBwdF<T, false> f{(const T*)x, (const T*)dy, C, true}; rc = colreduce_launch_batched<2>(f, rows_per_sample, B, C, ws, S, st); }
        if (rc) return rc;
        // dg_part reuses the front of the (now consumed) partial workspace
        hipLaunchKernelGGL(grn_coef_kernel, dim3(B), dim3(256), 0, st, g_saved, gamma, C, a, (float*)nullptr, S, K, ws);
        const dim3 grid(colfixed_blocks(rows, C / 8, 4, 8192));
        if (pre_gelu) hipLaunchKernelGGL((grn_apply_kernel<T, true>), grid, dim3(256), 0, st, (const T*)dy,
                           (const T*)x, a, K, (const float*)nullptr, (T*)dx, rows, fastdiv_make((uint32_t)rows_per_sample), C);
        else hipLaunchKernelGGL((grn_apply_kernel<T, false>), grid, dim3(256), 0, st, (const T*)dy,
                           (const T*)x, a, K, (const float*)nullptr, (T*)dx, rows, fastdiv_make((uint32_t)rows_per_sample), C);
    })
    SEGF_CHECK_LAUNCH();
    hipLaunchKernelGGL(grn_param_grads_kernel, dim3((C + 255) / 256), dim3(256), 0, st, ws, S, B, C, dgamma, dbeta);
    SEGF_CHECK_LAUNCH();
    return 0;
}
