// 3 x 3 convolution with dilation (stride 1, padding = dilation = d, no bias) on NHWC tokens as an implicit GEMM: the three atrous
// branches of DeepLabV3's ASPP (heads/deeplabv3.py:65-75, rates 12 / 24 / 36 on the stride-32 map).  No im2col buffer.
//
//   mode 0  y[p][co]          = sum_{tap, ci} x[p + off(tap)][ci] w[co][tap * Cin + ci]          off(tap) = ((ty - 1) d, (tx - 1) d)
//   mode 1  dx[p][ci]         = sum_{tap, co} dy[p - off(tap)][co] wt[ci][tap * Cout + co]       (the same kernel, offsets negated)
//   mode 2  dw[co][tap][ci]   = sum_p dy[p][co] x[p + off(tap)][ci]                               fp32, split over pixels
//
// TAP CULLING.  A tap can only touch the image when |ty - 1| d < H and |tx - 1| d < W: on the 16 x 16 map of a 512 x 512 input the rates
// 24 and 36 keep the centre tap alone.  The host lists the live taps in the kernel arguments and the reduction runs over those only
// (K = n_live * C).  Inside a live tap a workgroup whose 64 pixels all fall outside the image for that tap skips it as well (rate 12 on
// 16 x 16: an off-centre tap is live for the pixels within 4 of one border), decided once per workgroup.  The weight gradient of a dead
// tap is written as zeros.  SEGFAC_DILCONV_NO_CULL walks all nine taps with zero loads for the dead ones (A/B runs, tests).
//
// TILE.  64 x 64 outputs per workgroup of 4 waves, 32 reduction elements per step, operands staged global -> registers -> LDS with the
// next step's loads in flight over the current step's MFMAs (two LDS buffers, one barrier per step).  Both LDS tiles are
// [index][reduction], so one fragment routine serves all modes: wave w owns 16 rows of the INNER tile (the index that is contiguous in
// the output: channels) and all 64 of the OUTER tile (pixels; output channels for the weight gradient), and the inner tile is the A
// operand -- the accumulator registers of a lane are then 4 consecutive output channels: one 8- / 16-byte store.
//   bf16: v_mfma_f32_16x16x32_bf16 (lane l: row l & 15, k = 8 (l >> 4) + j);  fp32: v_mfma_f32_16x16x4_f32 (k = l >> 4), an exact fp32
//   fma chain.  The maps are small (256 - 16 K pixels): the kernel is bound by launch and tail, not by the matrix rate.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 dc_bf16x8;
typedef __attribute__((ext_vector_type(4))) float dc_f32x4;

constexpr int DC_T = 64;          // tile edge, inner and outer
constexpr int DC_K = 32;          // reduction elements per step
// LDS row length in elements: 80-byte rows (bf16) / 144-byte rows (fp32) keep the 16-byte accesses aligned and spread the banks
template <typename T> struct DcLd;
template <> struct DcLd<bf16_t> { static constexpr int v = 40; };
template <> struct DcLd<float> { static constexpr int v = 36; };

struct DilArgs {
    const void* x;            // mode 0: x; mode 1: dy; mode 2: x
    const void* w;            // mode 0: w [Cout][9 Cin]; mode 1: wt [Cin][9 Cout]; mode 2: dy
    void* y;
    float* ws;
    int64_t ldx, ldw, ldy, P, ppc;
    int H, W, N, C;           // modes 0 / 1: N output channels, C reduction channels; mode 2: N = Cout, C = Cin
    int d, sign, cull, split;
    int n_live, live_mask;
    int live[9];
};

template <typename T> __device__ __forceinline__ Raw8<T> dc_zero();
template <> __device__ __forceinline__ Raw8<bf16_t> dc_zero<bf16_t>() { Raw8<bf16_t> r; r.u = make_uint4(0u, 0u, 0u, 0u); return r; }
template <> __device__ __forceinline__ Raw8<float> dc_zero<float>() {
    Raw8<float> r; r.a = make_float4(0.f, 0.f, 0.f, 0.f); r.b = r.a; return r;
}
// 8 elements along an LDS row
__device__ __forceinline__ void dc_st_row(bf16_t* s, const Raw8<bf16_t>& r) { *reinterpret_cast<uint4*>(s) = r.u; }
__device__ __forceinline__ void dc_st_row(float* s, const Raw8<float>& r) {
    *reinterpret_cast<float4*>(s) = r.a; *reinterpret_cast<float4*>(s + 4) = r.b;
}
// 8 elements down an LDS column (the weight gradient's operands are reduction-major in memory)
template <int LD> __device__ __forceinline__ void dc_st_col(bf16_t* s, const Raw8<bf16_t>& r) {
    s[0 * LD] = (bf16_t)(r.u.x & 0xffffu); s[1 * LD] = (bf16_t)(r.u.x >> 16);
    s[2 * LD] = (bf16_t)(r.u.y & 0xffffu); s[3 * LD] = (bf16_t)(r.u.y >> 16);
    s[4 * LD] = (bf16_t)(r.u.z & 0xffffu); s[5 * LD] = (bf16_t)(r.u.z >> 16);
    s[6 * LD] = (bf16_t)(r.u.w & 0xffffu); s[7 * LD] = (bf16_t)(r.u.w >> 16);
}
template <int LD> __device__ __forceinline__ void dc_st_col(float* s, const Raw8<float>& r) {
    s[0 * LD] = r.a.x; s[1 * LD] = r.a.y; s[2 * LD] = r.a.z; s[3 * LD] = r.a.w;
    s[4 * LD] = r.b.x; s[5 * LD] = r.b.y; s[6 * LD] = r.b.z; s[7 * LD] = r.b.w;
}

// acc[t][r] += sum_k sI[16 wave + 4 (lane >> 4) + r][k] * sO[16 t + (lane & 15)][k] over the DC_K elements of one step
template <typename T>
__device__ __forceinline__ void dc_mma(const T* __restrict__ sI, const T* __restrict__ sO, int wave, int lane, dc_f32x4 (&acc)[4]) {
    constexpr int LD = DcLd<T>::v;
    const int r = lane & 15, q = lane >> 4;
    if constexpr (sizeof(T) == 2) {
        const dc_bf16x8 fa = *reinterpret_cast<const dc_bf16x8*>(sI + (16 * wave + r) * LD + 8 * q);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const dc_bf16x8 fb = *reinterpret_cast<const dc_bf16x8*>(sO + (16 * t + r) * LD + 8 * q);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[t], 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int s = 0; s < DC_K / 4; ++s) {
            const float fa = sI[(16 * wave + r) * LD + 4 * s + q];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float fb = sO[(16 * t + r) * LD + 4 * s + q];
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa, fb, acc[t], 0, 0, 0);
            }
        }
    }
}

__device__ __forceinline__ void dc_store4(bf16_t* p, const dc_f32x4& c) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack2bf(c[0], c[1]), pack2bf(c[2], c[3]));
}
__device__ __forceinline__ void dc_store4(float* p, const dc_f32x4& c) { *reinterpret_cast<float4*>(p) = make_float4(c[0], c[1], c[2], c[3]); }

// ---- forward (sign +1) and data gradient (sign -1): grid (pixel tiles, channel tiles) --------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) conv3x3_dil_kernel(const DilArgs a) {
    constexpr int LD = DcLd<T>::v;
    __shared__ __attribute__((aligned(16))) T sI[2][DC_T * LD];          // weights [n][k]
    __shared__ __attribute__((aligned(16))) T sO[2][DC_T * LD];          // gathered pixels [pixel][k]
    __shared__ int s_mask;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * DC_T;
    const int n0 = blockIdx.y * DC_T;
    const T* __restrict__ X = (const T*)a.x;
    const T* __restrict__ Wt = (const T*)a.w;

    // this thread stages 8 reduction elements of one pixel row and of one weight row per step
    const int row = tid >> 2, kq = (tid & 3) * 8;
    const int64_t p = p0 + row;
    const bool pv = p < a.P;
    const int px = (int)(p % a.W), py = (int)((p / a.W) % a.H);
    const bool nv = n0 + row < a.N;
    const int step_y = a.sign * a.d, step_x = a.sign * a.d;

    // live taps of this workgroup: bit i = some pixel of the tile reads inside the image through tap live[i]
    if (tid == 0) s_mask = 0;
    __syncthreads();
    {
        int m = 0;
        for (int i = 0; i < a.n_live; ++i) {
            const int ty = a.live[i] / 3 - 1, tx = a.live[i] % 3 - 1;
            const int yy = py + ty * step_y, xx = px + tx * step_x;
            if (pv && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W) m |= 1 << i;
        }
        if (m && (tid & 3) == 0) atomicOr(&s_mask, m);
    }
    __syncthreads();
    const int mask = a.cull ? s_mask : (1 << a.n_live) - 1;
    const int KC = (a.C + DC_K - 1) / DC_K;
    const int nsteps = __popc(mask) * KC;

    Raw8<T> ra, rb;
    auto load = [&](int ti, int kc) {
        const int tap = a.live[ti];
        const int ty = tap / 3 - 1, tx = tap % 3 - 1;
        const int ch = kc * DC_K + kq;
        const bool cv = ch < a.C;
        const int yy = py + ty * step_y, xx = px + tx * step_x;
        ra = dc_zero<T>();
        rb = dc_zero<T>();
        if (pv && cv && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W)
            ra = load8_raw<T>(X + (p + (int64_t)ty * step_y * a.W + tx * step_x) * a.ldx + ch);
        if (nv && cv) rb = load8_raw<T>(Wt + (int64_t)(n0 + row) * a.ldw + (int64_t)tap * a.C + ch);
    };

    dc_f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = dc_f32x4{0.f, 0.f, 0.f, 0.f};

    int ti = mask ? __ffs(mask) - 1 : 0, kc = 0, buf = 0;
    if (nsteps) load(ti, kc);
    for (int s = 0; s < nsteps; ++s) {
        dc_st_row(&sO[buf][row * LD + kq], ra);
        dc_st_row(&sI[buf][row * LD + kq], rb);
        if (++kc == KC) {
            kc = 0;
            const int rest = mask >> (ti + 1);
            ti += rest ? __ffs(rest) : 0;
        }
        if (s + 1 < nsteps) load(ti, kc);          // in flight over this step's MFMAs
        __syncthreads();
        dc_mma<T>(sI[buf], sO[buf], wave, lane, acc);
        buf ^= 1;
    }

    T* __restrict__ Y = (T*)a.y;
    const int n = n0 + 16 * wave + 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t pix = p0 + 16 * t + (lane & 15);
        if (pix < a.P && n < a.N) dc_store4(Y + pix * a.ldy + n, acc[t]);
    }
}

// ---- weight gradient: grid (Cin tiles, Cout tiles, 9 * split); the reduction runs over pixels ---------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) conv3x3_dil_wgrad_kernel(const DilArgs a) {
    constexpr int LD = DcLd<T>::v;
    __shared__ __attribute__((aligned(16))) T sI[2][DC_T * LD];          // shifted x, transposed: [ci][pixel]
    __shared__ __attribute__((aligned(16))) T sO[2][DC_T * LD];          // dy, transposed: [co][pixel]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tap = blockIdx.z / a.split, slice = blockIdx.z % a.split;
    const int i0 = blockIdx.x * DC_T, o0 = blockIdx.y * DC_T;
    const int Cin = a.C, Cout = a.N;
    const bool live = (a.live_mask >> tap) & 1;
    if (!live && a.split > 1) return;          // the reduce pass writes a dead tap's zeros
    float* out = a.split > 1 ? a.ws + (int64_t)slice * Cout * 9 * Cin : (float*)a.y;
    const int64_t ldo = a.split > 1 ? (int64_t)9 * Cin : a.ldy;

    const int64_t pb = (int64_t)slice * a.ppc;
    int64_t pe = pb + a.ppc < a.P ? pb + a.ppc : a.P;
    if (!live || pe < pb) pe = pb;             // dead tap, one slice: no steps, the epilogue stores the zeros
    const int ntiles = (int)((pe - pb + DC_K - 1) / DC_K);
    const T* __restrict__ X = (const T*)a.x;
    const T* __restrict__ G = (const T*)a.w;
    const int ty = tap / 3 - 1, tx = tap % 3 - 1;
    const int64_t shift = (int64_t)ty * a.d * a.W + tx * a.d;
    const int pix = tid >> 3, c8 = (tid & 7) * 8;
    const bool iv = i0 + c8 < Cin, ov = o0 + c8 < Cout;

    Raw8<T> rx, rg;
    auto load = [&](int it) -> int {
        const int64_t p = pb + (int64_t)it * DC_K + pix;
        const int px = (int)(p % a.W), py = (int)((p / a.W) % a.H);
        const int yy = py + ty * a.d, xx = px + tx * a.d;
        const bool v = p < pe && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
        rx = dc_zero<T>();
        rg = dc_zero<T>();
        if (v && iv) rx = load8_raw<T>(X + (p + shift) * a.ldx + i0 + c8);
        if (v && ov) rg = load8_raw<T>(G + p * a.ldw + o0 + c8);          // (a pixel whose x is padding adds nothing: dy not read)
        return v ? 1 : 0;
    };

    dc_f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = dc_f32x4{0.f, 0.f, 0.f, 0.f};

    // a 32-pixel step none of whose pixels reads inside the image through this tap is skipped (uniform: decided at the barrier)
    int buf = 0;
    bool cur = false;
    if (ntiles) {
        const int v = load(0);
        cur = __syncthreads_or(v) != 0 || !a.cull;
    }
    for (int it = 0; it < ntiles; ++it) {
        if (cur) {
            dc_st_col<LD>(&sI[buf][c8 * LD + pix], rx);
            dc_st_col<LD>(&sO[buf][c8 * LD + pix], rg);
        }
        int vn = 0;
        if (it + 1 < ntiles) vn = load(it + 1);
        const bool next = (__syncthreads_or(vn) != 0 || !a.cull) && it + 1 < ntiles;
        if (cur) dc_mma<T>(sI[buf], sO[buf], wave, lane, acc);
        cur = next;
        buf ^= 1;
    }

    const int ci = i0 + 16 * wave + 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int co = o0 + 16 * t + (lane & 15);
        if (co < Cout && ci < Cin) dc_store4(out + (int64_t)co * ldo + (int64_t)tap * Cin + ci, acc[t]);
    }
}

// dw[co][col .. col + 3] = sum of the slices in fixed order; a dead tap's columns are zeros
__global__ void __launch_bounds__(256) conv3x3_dil_reduce_kernel(const float* __restrict__ ws, int split, int Cout, int Cin, int live_mask,
                                                                 float* __restrict__ y, int64_t ldy) {
    const int64_t row4 = (int64_t)9 * Cin / 4, total = (int64_t)Cout * row4;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t co = i / row4;
    const int col = (int)(i - co * row4) * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((live_mask >> (col / Cin)) & 1) {
        const int64_t slab = (int64_t)Cout * 9 * Cin;
        for (int z = 0; z < split; ++z) {
            const float4 v = *reinterpret_cast<const float4*>(ws + z * slab + co * 9 * Cin + col);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    *reinterpret_cast<float4*>(y + co * ldy + col) = s;
}

int dil_live_taps(int H, int W, int d, int* taps) {
    int n = 0;
    for (int ty = 0; ty < 3; ++ty)
        for (int tx = 0; tx < 3; ++tx)
            if ((int64_t)(ty == 1 ? 0 : 1) * d < H && (int64_t)(tx == 1 ? 0 : 1) * d < W) taps[n++] = ty * 3 + tx;
    return n;
}

bool dil_shape_ok(int dt, int mode, int B, int H, int W, int Cin, int Cout, int d) {
    if (dt != SEGF_F32 && dt != SEGF_BF16) return false;
    if (mode < 0 || mode > 2 || B < 1 || H < 1 || W < 1 || d < 1 || Cin < 8 || Cout < 8 || Cin % 8 || Cout % 8) return false;
    const int64_t P = (int64_t)B * H * W;
    if (P >= (1ll << 31) || (int64_t)d * ((int64_t)W + 1) >= (1ll << 31) || (int64_t)Cout * 9 * Cin >= (1ll << 31)) return false;
    if ((P + DC_T - 1) / DC_T >= (1ll << 31) || (Cin + DC_T - 1) / DC_T > 65535 || (Cout + DC_T - 1) / DC_T > 65535) return false;
    return true;
}

}   // namespace

// taps[9] <- the taps ty * 3 + tx that can touch an H x W map at this dilation; returns their number (the geometry alone:
// SEGFAC_DILCONV_NO_CULL does not change the answer)
extern "C" int segf_conv3x3_dil_live_taps(int H, int W, int dilation, int* taps) {
    if (H < 1 || W < 1 || dilation < 1 || !taps) return SEGF_ERR_SHAPE;
    return dil_live_taps(H, W, dilation, taps);
}

extern "C" int segf_conv3x3_dil_supported(int dt, int mode, int B, int H, int W, int Cin, int Cout, int dilation) {
    return dil_shape_ok(dt, mode, B, H, W, Cin, Cout, dilation) ? 1 : 0;
}

// slices of the pixel range for mode 2: enough workgroups for two rounds of the 256 compute units, at least two 32-pixel steps each
extern "C" int segf_conv3x3_dil_pick_splitk(int B, int H, int W, int Cin, int Cout, int dilation) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || dilation < 1) return 1;
    int taps[9];
    const int n_live = POL(dilconv_no_cull) ? 9 : dil_live_taps(H, W, dilation, taps);
    const int64_t tiles = cdiv64(Cin, DC_T) * cdiv64(Cout, DC_T) * n_live;
    const int64_t ksteps = cdiv64((int64_t)B * H * W, DC_K);
    int64_t split = cdiv64(512, tiles);
    if (split > ksteps / 2) split = ksteps / 2;
    if (split > 64) split = 64;
    return split < 1 ? 1 : (int)split;
}

extern "C" int segf_conv3x3_dil(int dt, int mode, int B, int H, int W, int Cin, int Cout, int dilation, const void* x, int64_t ldx,
                                const void* w, int64_t ldw, void* y, int64_t ldy, int split_k, float* ws, void* stream) {
    if (!dil_shape_ok(dt, mode, B, H, W, Cin, Cout, dilation) || !x || !w || !y) return SEGF_ERR_SHAPE;
    const int64_t es = dt == SEGF_BF16 ? 2 : 4, P = (int64_t)B * H * W;
    const int64_t reach = P + (int64_t)dilation * ((int64_t)W + 1);
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) % 16 || (ldx * es) % 16 || (ldw * es) % 16 || (ldy * (mode == 2 ? 4 : es)) % 16) return SEGF_ERR_SHAPE;
    const int64_t cx = mode == 1 ? Cout : Cin;                  // channels of the gathered operand
    if (ldx < cx || reach * ldx >= (1ll << 31)) return SEGF_ERR_SHAPE;          // 32-bit element offsets of the gather
    if (mode == 2) {
        if (ldw < Cout || ldy < (int64_t)9 * Cin || reach * ldw >= (1ll << 31) || (int64_t)Cout * ldy >= (1ll << 31)) return SEGF_ERR_SHAPE;
        if (split_k < 1 || split_k > 7281 || (split_k > 1 && (!ws || (uintptr_t)ws % 16))) return SEGF_ERR_SHAPE;
    } else {
        const int64_t N = mode == 0 ? Cout : Cin;
        if (ldw < 9 * cx || ldy < N || N * ldw >= (1ll << 31) || reach * ldy >= (1ll << 31)) return SEGF_ERR_SHAPE;
    }
    hipStream_t st = (hipStream_t)stream;
    DilArgs a;
    a.x = x; a.w = w; a.y = y; a.ws = ws;
    a.ldx = ldx; a.ldw = ldw; a.ldy = ldy; a.P = P;
    a.H = H; a.W = W; a.d = dilation;
    a.cull = POL(dilconv_no_cull) ? 0 : 1;
    a.n_live = dil_live_taps(H, W, dilation, a.live);
    if (!a.cull) { a.n_live = 9; for (int i = 0; i < 9; ++i) a.live[i] = i; }
    for (int i = a.n_live; i < 9; ++i) a.live[i] = 4;
    a.live_mask = 0;
    for (int i = 0; i < a.n_live; ++i) a.live_mask |= 1 << a.live[i];
    if (mode == 2) {
        a.N = Cout; a.C = Cin; a.sign = 1;
        a.split = split_k;
        a.ppc = cdiv64(cdiv64(P, split_k), DC_K) * DC_K;
        const dim3 grid((unsigned)cdiv64(Cin, DC_T), (unsigned)cdiv64(Cout, DC_T), (unsigned)(9 * split_k));
        SEGF_DISPATCH_DT(dt, T, { hipLaunchKernelGGL((conv3x3_dil_wgrad_kernel<T>), grid, dim3(256), 0, st, a); })
        SEGF_CHECK_LAUNCH();
        if (split_k > 1) {
            const int64_t total = (int64_t)Cout * 9 * Cin / 4;
            hipLaunchKernelGGL(conv3x3_dil_reduce_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, ws, split_k, Cout, Cin,
                               a.live_mask, (float*)y, ldy);
            SEGF_CHECK_LAUNCH();
        }
        return 0;
    }
    a.N = mode == 0 ? Cout : Cin;
    a.C = mode == 0 ? Cin : Cout;
    a.sign = mode == 0 ? 1 : -1;
    a.split = 1; a.ppc = 0;
    const dim3 grid((unsigned)cdiv64(P, DC_T), (unsigned)cdiv64(a.N, DC_T), 1);
    SEGF_DISPATCH_DT(dt, T, { hipLaunchKernelGGL((conv3x3_dil_kernel<T>), grid, dim3(256), 0, st, a); })
    SEGF_CHECK_LAUNCH();
    return 0;
}
