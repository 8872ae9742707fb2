// MetaFormer / ConvFormer (models/backbones/metaformer.py): the two parts of a block that are not a LayerNorm, a Linear or a depthwise 7 x 7:
//
//   StarReLU        y = s * relu(u)^2 + b          (metaformer.py:224-241; s, b one-element fp32 parameters, read from memory by the kernel)
//   residual scale  y = x * scale[c]               (metaformer.py:198-208, 489-513: res_scale(x) + branch in stages 3 and 4)
//
// four streaming passes over token tensors [rows][cols] in the storage dtype, fp32 arithmetic, operands with leading dimensions.
//
// Layout of every kernel ("column-fixed", common.h): a row is cols / 8 chunks of 8 elements (one 16-byte access in bf16, two in fp32); the
// launch has T = blocks * 256 threads with T % nchunk == 0, so global thread g keeps chunk g % nchunk for its whole walk over the rows
// g / nchunk, g / nchunk + T / nchunk, ...: a wave touches 64 consecutive chunks (1 KiB in bf16), per-channel operands are loaded once per
// thread and the loop carries no division.  Two rows are in flight per iteration.
//
// Sums.  StarReLU backward: ds = sum dy relu(u)^2 and db = sum dy over ALL elements (up to 5 x 10^8 at batch 64): eight products are added in
// a tree, the chunk sums along the thread's walk, the 64 lanes of a wave in a DPP butterfly, the four waves through LDS in wave order;
// the workgroup's pair goes to the caller's workspace and ONE workgroup adds the pairs in a fixed order.  Residual-scale backward:
// dscale[c] = sum_rows dy x stays in eight registers per thread, the threads of a workgroup that hold the same chunk are added through LDS in
// thread order, one [C] slab per workgroup goes to the workspace and colreduce_finalize adds the slabs.  No atomics: two runs give the
// same bits.
//
// Rooflines (elements of [rows][cols] moved): StarReLU forward 1 read + 1 written, backward 2 + 1; residual scale forward 1 + 1,
// backward 2 + 1.  At most three flops per element: memory-bound by two orders of magnitude.
#include "colreduce.h"

namespace {

constexpr int MF_THREADS = 256;
constexpr int MF_ROWS_PER_THREAD = 8;       // target number of rows a thread walks
constexpr int MF_MAX_BLOCKS = 4096;         // target upper bound of workgroups per launch (rounded up to the column-fixed unit)
constexpr int MF_STAR_MAX_COLS = 8192;
constexpr int MF_SCALE_MAX_COLS = 2048;     // <= 256 chunks: every workgroup holds every chunk, so its slab is complete

// validity + grid on the host; 0 = SEGF_ERR_SHAPE
static int mf_blocks(int64_t rows, int cols, int max_cols) {
    if (rows <= 0 || cols < 8 || cols > max_cols || cols % 8) return 0;
    if (rows >= (1ll << 31) || rows * cols >= (1ll << 31)) return 0;
    return colfixed_blocks(rows, cols / 8, MF_ROWS_PER_THREAD, MF_MAX_BLOCKS);
}
static bool mf_dt_ok(int dt) { return dt == SEGF_F32 || dt == SEGF_BF16; }
// rows of 16-byte chunks whose element offsets stay inside 32 bits
static bool mf_ld_ok(int dt, int64_t rows, int cols, int64_t ld) {
    return ld >= cols && ld % (dt == SEGF_BF16 ? 8 : 4) == 0 && rows > 0 && rows < (1ll << 31) && ld < (1ll << 31) && rows * ld < (1ll << 31);
}
static bool mf_op_ok(int dt, int64_t rows, int cols, const void* p, int64_t ld) {
    return p && ((uintptr_t)p & 15) == 0 && mf_ld_ok(dt, rows, cols, ld);
}

// this thread's place in the column-fixed walk
struct MfWalk {
    int c0;                 // first column of the thread's chunk
    int64_t r, rstep;       // first row, rows between two items
    __device__ __forceinline__ MfWalk(int nchunk) {
        const uint32_t g = blockIdx.x * MF_THREADS + threadIdx.x, q = g / (uint32_t)nchunk;
        c0 = (int)(g - q * (uint32_t)nchunk) * 8;
        r = q;
        rstep = (gridDim.x * MF_THREADS) / (uint32_t)nchunk;
    }
};

__device__ __forceinline__ float sum8(const float (&v)[8]) { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); }

// ---- StarReLU ----------------------------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void starrelu_fwd8(const Raw8<T>& raw, float s, float b, T* __restrict__ dst) {
    float v[8];
    unpack8(raw, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float p = fmaxf(v[j], 0.f); v[j] = fmaf(s, p * p, b); }
    store8<T>(dst, v);
}

template <typename T>
__global__ void __launch_bounds__(MF_THREADS) starrelu_fwd_kernel(const T* __restrict__ u, int64_t ldu, const float* __restrict__ s,
                                                                  const float* __restrict__ b, T* __restrict__ y, int64_t ldy, int64_t rows,
                                                                  int nchunk) {
    const MfWalk t(nchunk);
    const float sv = *s, bv = *b;
    int64_t r = t.r;
    for (; r + t.rstep < rows; r += 2 * t.rstep) {
        const Raw8<T> a0 = load8_raw<T>(u + r * ldu + t.c0);
        const Raw8<T> a1 = load8_raw<T>(u + (r + t.rstep) * ldu + t.c0);
        SEGF_LOADS_ISSUED();
        starrelu_fwd8<T>(a0, sv, bv, y + r * ldy + t.c0);
        starrelu_fwd8<T>(a1, sv, bv, y + (r + t.rstep) * ldy + t.c0);
    }
    if (r < rows) starrelu_fwd8<T>(load8_raw<T>(u + r * ldu + t.c0), sv, bv, y + r * ldy + t.c0);
}

// du = dy * 2 s relu(u); as += sum dy relu(u)^2, ab += sum dy
template <typename T>
__device__ __forceinline__ void starrelu_bwd8(const Raw8<T>& ur, const Raw8<T>& gr, float s2, T* __restrict__ dst, float& as, float& ab) {
    float v[8], g[8], q[8];
    unpack8(ur, v);
    unpack8(gr, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float p = fmaxf(v[j], 0.f);
        q[j] = g[j] * (p * p);
        v[j] = g[j] * (s2 * p);
    }
    store8<T>(dst, v);
    as += sum8(q);
    ab += sum8(g);
}

// partial: [gridDim.x][2] = (ds, db) of each workgroup
template <typename T>
__global__ void __launch_bounds__(MF_THREADS) starrelu_bwd_kernel(const T* __restrict__ u, int64_t ldu, const T* __restrict__ dy, int64_t lddy,
                                                                  const float* __restrict__ s, T* __restrict__ du, int64_t lddu,
                                                                  float* __restrict__ partial, int64_t rows, int nchunk) {
    __shared__ float red[2][MF_THREADS / 64];
    const MfWalk t(nchunk);
    const float s2 = 2.f * *s;
    float as = 0.f, ab = 0.f;
    int64_t r = t.r;
    for (; r + t.rstep < rows; r += 2 * t.rstep) {
        const int64_t r1 = r + t.rstep;
        const Raw8<T> u0 = load8_raw<T>(u + r * ldu + t.c0), g0 = load8_raw<T>(dy + r * lddy + t.c0);
        const Raw8<T> u1 = load8_raw<T>(u + r1 * ldu + t.c0), g1 = load8_raw<T>(dy + r1 * lddy + t.c0);
        SEGF_LOADS_ISSUED();
        starrelu_bwd8<T>(u0, g0, s2, du + r * lddu + t.c0, as, ab);
        starrelu_bwd8<T>(u1, g1, s2, du + r1 * lddu + t.c0, as, ab);
    }
    if (r < rows) {
        const Raw8<T> u0 = load8_raw<T>(u + r * ldu + t.c0), g0 = load8_raw<T>(dy + r * lddy + t.c0);
        starrelu_bwd8<T>(u0, g0, s2, du + r * lddu + t.c0, as, ab);
    }
    as = wave_sum_all(as);
    ab = wave_sum_all(ab);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = as; red[1][wave] = ab; }
    __syncthreads();
    if (threadIdx.x < 2) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < MF_THREADS / 64; ++w) v += red[threadIdx.x][w];
        partial[(int64_t)blockIdx.x * 2 + threadIdx.x] = v;
    }
}

// one workgroup: thread t adds the pairs t, t + 256, ... in that order, then lanes, then waves
__global__ void __launch_bounds__(MF_THREADS) starrelu_finalize_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ ds,
                                                                       float* __restrict__ db) {
    __shared__ float red[2][MF_THREADS / 64];
    float as = 0.f, ab = 0.f;
    for (int i = threadIdx.x; i < nblk; i += MF_THREADS) { as += partial[2 * i]; ab += partial[2 * i + 1]; }
    as = wave_sum_all(as);
    ab = wave_sum_all(ab);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = as; red[1][wave] = ab; }
    __syncthreads();
    if (threadIdx.x < 2) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < MF_THREADS / 64; ++w) v += red[threadIdx.x][w];
        *(threadIdx.x == 0 ? ds : db) = v;
    }
}

// ---- residual scale -------------------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void colscale8(const Raw8<T>& raw, const float (&sc)[8], T* __restrict__ dst) {
    float v[8];
    unpack8(raw, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] *= sc[j];
    store8<T>(dst, v);
}

template <typename T>
__global__ void __launch_bounds__(MF_THREADS) colscale_fwd_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ scale,
                                                                  T* __restrict__ y, int64_t ldy, int64_t rows, int nchunk) {
    const MfWalk t(nchunk);
    float sc[8];
    load8f(scale + t.c0, sc);
    int64_t r = t.r;
    for (; r + t.rstep < rows; r += 2 * t.rstep) {
        const Raw8<T> a0 = load8_raw<T>(x + r * ldx + t.c0);
        const Raw8<T> a1 = load8_raw<T>(x + (r + t.rstep) * ldx + t.c0);
        SEGF_LOADS_ISSUED();
        colscale8<T>(a0, sc, y + r * ldy + t.c0);
        colscale8<T>(a1, sc, y + (r + t.rstep) * ldy + t.c0);
    }
    if (r < rows) colscale8<T>(load8_raw<T>(x + r * ldx + t.c0), sc, y + r * ldy + t.c0);
}

template <typename T>
__device__ __forceinline__ void colscale_bwd8(const Raw8<T>& gr, const Raw8<T>& xr, const float (&sc)[8], T* __restrict__ dst, float (&acc)[8]) {
    float g[8], v[8];
    unpack8(gr, g);
    unpack8(xr, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) { acc[j] = fmaf(g[j], v[j], acc[j]); g[j] *= sc[j]; }
    store8<T>(dst, g);
}

// partial: [gridDim.x][C]
template <typename T>
__global__ void __launch_bounds__(MF_THREADS) colscale_bwd_kernel(const T* __restrict__ dy, int64_t lddy, const T* __restrict__ x, int64_t ldx,
                                                                  const float* __restrict__ scale, T* __restrict__ dx, int64_t lddx,
                                                                  float* __restrict__ partial, int64_t rows, int nchunk) {
    __shared__ float red[MF_THREADS * 8];
    const MfWalk t(nchunk);
    float sc[8], acc[8];
    load8f(scale + t.c0, sc);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    int64_t r = t.r;
    for (; r + t.rstep < rows; r += 2 * t.rstep) {
        const int64_t r1 = r + t.rstep;
        const Raw8<T> g0 = load8_raw<T>(dy + r * lddy + t.c0), x0 = load8_raw<T>(x + r * ldx + t.c0);
        const Raw8<T> g1 = load8_raw<T>(dy + r1 * lddy + t.c0), x1 = load8_raw<T>(x + r1 * ldx + t.c0);
        SEGF_LOADS_ISSUED();
        colscale_bwd8<T>(g0, x0, sc, dx + r * lddx + t.c0, acc);
        colscale_bwd8<T>(g1, x1, sc, dx + r1 * lddx + t.c0, acc);
    }
    if (r < rows) {
        const Raw8<T> g0 = load8_raw<T>(dy + r * lddy + t.c0), x0 = load8_raw<T>(x + r * ldx + t.c0);
        colscale_bwd8<T>(g0, x0, sc, dx + r * lddx + t.c0, acc);
    }
    // threads tid, tid + nchunk, tid + 2 nchunk, ... of a workgroup hold the same chunk (256 consecutive global ids, nchunk <= 256)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x * 8 + j] = acc[j];
    __syncthreads();
    if ((int)threadIdx.x < nchunk) {
        float sm[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) sm[j] = 0.f;
        for (int k = threadIdx.x; k < MF_THREADS; k += nchunk)
#pragma unroll
            for (int j = 0; j < 8; ++j) sm[j] += red[k * 8 + j];
        store8<float>(partial + (int64_t)blockIdx.x * nchunk * 8 + t.c0, sm);
    }
}

}  // namespace

extern "C" int segf_starrelu_supported(int dt, int64_t rows, int cols, int64_t ld) {
    return mf_dt_ok(dt) && mf_blocks(rows, cols, MF_STAR_MAX_COLS) > 0 && mf_ld_ok(dt, rows, cols, ld);
}

extern "C" int segf_starrelu_blocks(int64_t rows, int cols) { return mf_blocks(rows, cols, MF_STAR_MAX_COLS); }

extern "C" int64_t segf_starrelu_bwd_ws(int64_t rows, int cols) { return 2 * (int64_t)mf_blocks(rows, cols, MF_STAR_MAX_COLS); }

extern "C" int segf_starrelu_fwd(int dt, int64_t rows, int cols, const void* u, int64_t ldu, const float* s, const float* b, void* y,
                                 int64_t ldy, void* stream) {
    if (!mf_dt_ok(dt)) return SEGF_ERR_DTYPE;
    const int nblk = mf_blocks(rows, cols, MF_STAR_MAX_COLS);
    if (!nblk) return SEGF_ERR_SHAPE;                                    // before any launch
    if (!mf_op_ok(dt, rows, cols, u, ldu) || !mf_op_ok(dt, rows, cols, y, ldy) || !s || !b) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    SEGF_DISPATCH_DT(dt, T, {
        hipLaunchKernelGGL((starrelu_fwd_kernel<T>), dim3((unsigned)nblk), dim3(MF_THREADS), 0, st, (const T*)u, ldu, s, b, (T*)y, ldy, rows,
                           cols / 8);
    })
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int segf_starrelu_bwd(int dt, int64_t rows, int cols, const void* u, int64_t ldu, const void* dy, int64_t lddy, const float* s,
                                 void* du, int64_t lddu, float* ds, float* db, float* ws, void* stream) {
    if (!mf_dt_ok(dt)) return SEGF_ERR_DTYPE;
    const int nblk = mf_blocks(rows, cols, MF_STAR_MAX_COLS);
    if (!nblk) return SEGF_ERR_SHAPE;
    if (!mf_op_ok(dt, rows, cols, u, ldu) || !mf_op_ok(dt, rows, cols, dy, lddy) || !mf_op_ok(dt, rows, cols, du, lddu) || !s || !ds || !db)
        return SEGF_ERR_SHAPE;
    if (!ws) return SEGF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    SEGF_DISPATCH_DT(dt, T, {
        hipLaunchKernelGGL((starrelu_bwd_kernel<T>), dim3((unsigned)nblk), dim3(MF_THREADS), 0, st, (const T*)u, ldu, (const T*)dy, lddy, s,
                           (T*)du, lddu, ws, rows, cols / 8);
    })
    SEGF_CHECK_LAUNCH();
    hipLaunchKernelGGL(starrelu_finalize_kernel, dim3(1), dim3(MF_THREADS), 0, st, ws, nblk, ds, db);
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int segf_colscale_supported(int dt, int64_t rows, int C, int64_t ld) {
    return mf_dt_ok(dt) && mf_blocks(rows, C, MF_SCALE_MAX_COLS) > 0 && mf_ld_ok(dt, rows, C, ld);
}

extern "C" int segf_colscale_blocks(int64_t rows, int C) { return mf_blocks(rows, C, MF_SCALE_MAX_COLS); }

extern "C" int64_t segf_colscale_bwd_ws(int64_t rows, int C) { return (int64_t)mf_blocks(rows, C, MF_SCALE_MAX_COLS) * C; }

extern "C" int segf_colscale_fwd(int dt, int64_t rows, int C, const void* x, int64_t ldx, const float* scale, void* y, int64_t ldy,
                                 void* stream) {
    if (!mf_dt_ok(dt)) return SEGF_ERR_DTYPE;
    const int nblk = mf_blocks(rows, C, MF_SCALE_MAX_COLS);
    if (!nblk) return SEGF_ERR_SHAPE;
    if (!mf_op_ok(dt, rows, C, x, ldx) || !mf_op_ok(dt, rows, C, y, ldy) || !scale || ((uintptr_t)scale & 15)) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    SEGF_DISPATCH_DT(dt, T, {
        hipLaunchKernelGGL((colscale_fwd_kernel<T>), dim3((unsigned)nblk), dim3(MF_THREADS), 0, st, (const T*)x, ldx, scale, (T*)y, ldy, rows,
                           C / 8);
    })
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int segf_colscale_bwd(int dt, int64_t rows, int C, const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* scale,
                                 void* dx, int64_t lddx, float* dscale, float* ws, void* stream) {
    if (!mf_dt_ok(dt)) return SEGF_ERR_DTYPE;
    const int nblk = mf_blocks(rows, C, MF_SCALE_MAX_COLS);
    if (!nblk) return SEGF_ERR_SHAPE;
    if (!mf_op_ok(dt, rows, C, dy, lddy) || !mf_op_ok(dt, rows, C, x, ldx) || !mf_op_ok(dt, rows, C, dx, lddx) || !scale ||
        ((uintptr_t)scale & 15) || !dscale)
        return SEGF_ERR_SHAPE;
    if (!ws || ((uintptr_t)ws & 15)) return SEGF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    SEGF_DISPATCH_DT(dt, T, {
        hipLaunchKernelGGL((colscale_bwd_kernel<T>), dim3((unsigned)nblk), dim3(MF_THREADS), 0, st, (const T*)dy, lddy, (const T*)x, ldx, scale,
                           (T*)dx, lddx, ws, rows, C / 8);
    })
    SEGF_CHECK_LAUNCH();
    colreduce_finalize_launch(ws, nblk, C, dscale, st);
    SEGF_CHECK_LAUNCH();
    return 0;
}
