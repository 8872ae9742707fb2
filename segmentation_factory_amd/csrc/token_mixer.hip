// CAS-ViT additive token mixer (models/backbones/casvit.py:68-92, 112-138): the parts of
//
//     q' = ChannelOp(SpatialOp(q)),  k' = ChannelOp(SpatialOp(k)),  out = proj(dwc(q' + k') * v)
//
// that are not a 1 x 1 convolution, a depthwise 3 x 3 or a BatchNorm: three streaming kernel pairs on token tensors [M = B HW][C].
//
//   spatial gate       s[m] = sigmoid(sum_c r[m][c] w[c]),  y = x * s,  pool[b][c] = sum_pixels x * s          (r = ReLU(BN(dw3x3(x) + b)))
//   channel gate mix   u = q1 * gq[b] + k1 * gk[b]                                                              (g = sigmoid(Wc pool / HW))
//   gated product      z = a * v
//
// Layout of every kernel: a row is C / 8 chunks of 8 elements (16 bytes in bf16, two 16-byte accesses in fp32); L = the power of two
// >= C / 8, at most 64, lanes share a row and each takes chunk lx (and chunk lx + 64 when C > 512), so a row's reduction is a wave64
// butterfly of width L (DPP up to 16 lanes).  A workgroup of 256 threads holds 256 / L rows at a time and walks a contiguous range of
// rows of ONE sample (grid.y = sample), so the per-sample operands (gq, gk, dpool) are loaded once per thread and per-sample sums never
// mix samples.  Sums over rows stay in registers along the walk, are added over the workgroup's row lanes through LDS in a fixed order
// and go to the caller's workspace as one [C] slab per workgroup; colreduce_finalize adds the slabs in a fixed order.  No atomics.
//
// Rooflines (elements of [M][C] moved, fp32 side tensors of M or B C elements left out): spatial gate forward 2 read + 1 written,
// backward 3 read + 2 written; channel gate mix forward 2 + 1, backward 3 + 2; gated product forward 2 + 1, backward 3 + 2.  At about one
// flop per byte all six are memory-bound by two orders of magnitude.
#include "colreduce.h"

namespace {

constexpr int TM_THREADS = 256;
constexpr int TM_ROWS_PER_LANE = 16;       // target number of rows a row lane walks
constexpr int TM_MAX_BLOCKS = 4096;        // target upper bound of workgroups per launch

struct TmGeom {
    int B, HW, C;
    int L, lsh;            // lanes per row and its log2
    int RL;                // rows a workgroup holds at a time
    int NI;                // chunks per lane: 1, or 2 when C > 512
    int nblk;              // workgroups per sample (grid.x)
    int rpb;               // rows per workgroup
};

// validity + geometry on the host; false = SEGF_ERR_SHAPE
static bool tm_geom(int B, int HW, int C, TmGeom& g) {
    if (B <= 0 || B > 65535 || HW <= 0 || C < 8 || C > 1024 || C % 8) return false;          // (B is grid.y)
    if ((int64_t)B * HW >= (1ll << 31) / 4) return false;
    const int nchunk = C / 8;
    int L = 1, lsh = 0;
    while (L < nchunk && L < 64) { L <<= 1; ++lsh; }
    g.B = B; g.HW = HW; g.C = C; g.L = L; g.lsh = lsh; g.RL = TM_THREADS / L; g.NI = (nchunk + L - 1) / L;
    const int cap = TM_MAX_BLOCKS / B > 0 ? TM_MAX_BLOCKS / B : 1;
    const int64_t want = cdiv64(HW, (int64_t)g.RL * TM_ROWS_PER_LANE);
    const int nblk = (int)(want > cap ? cap : want);
    g.rpb = (int)cdiv64(HW, nblk);
    g.nblk = (int)cdiv64(HW, g.rpb);           // no empty workgroup
    return true;
}
static bool tm_dt_ok(int dt) { return dt == SEGF_F32 || dt == SEGF_BF16; }
// rows of 16-byte chunks: leading dimension and base pointer
static bool tm_ld_ok(int dt, int C, int64_t ld) { return ld >= C && ld % (dt == SEGF_BF16 ? 8 : 4) == 0; }
static bool tm_op_ok(int dt, int C, const void* p, int64_t ld) { return p && ((uintptr_t)p & 15) == 0 && tm_ld_ok(dt, C, ld); }
static bool tm_f32_ok(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

template <typename T> __device__ __forceinline__ Raw8<T> tm_zero();
template <> __device__ __forceinline__ Raw8<bf16_t> tm_zero<bf16_t>() { Raw8<bf16_t> r; r.u = make_uint4(0u, 0u, 0u, 0u); return r; }
template <> __device__ __forceinline__ Raw8<float> tm_zero<float>() {
    Raw8<float> r; r.a = make_float4(0.f, 0.f, 0.f, 0.f); r.b = r.a; return r;
}
template <typename T> __device__ __forceinline__ Raw8<T> tm_ld(const T* p, bool pred) { return pred ? load8_raw<T>(p) : tm_zero<T>(); }
__device__ __forceinline__ void tm_ldf(const float* p, bool pred, float (&v)[8]) {
    if (pred) { load8f(p, v); }
    else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.f;
    }
}

// this thread's place: lane lx of row lane ty; chunk i of the lane starts at column c0[i] (ok[i]: inside the row)
template <int NI> struct TmLane {
    int lx, ty, c0[NI];
    bool ok[NI];
    __device__ __forceinline__ TmLane(const TmGeom& g) {
        lx = threadIdx.x & (g.L - 1); ty = threadIdx.x >> g.lsh;
#pragma unroll
        for (int i = 0; i < NI; ++i) { c0[i] = (lx + i * g.L) * 8; ok[i] = c0[i] < g.C; }
    }
};

// Sum acc over the workgroup's row lanes (LDS, row-lane order) and write the [C] slab dst[c0 ..].  Every thread of the workgroup calls it.
template <int NI>
__device__ __forceinline__ void tm_block_tail(const float (&acc)[NI][8], const TmLane<NI>& t, const TmGeom& g, float* __restrict__ dst,
                                              float* red) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) red[threadIdx.x * 8 + j] = acc[i][j];
        __syncthreads();
        if (t.ty == 0 && t.ok[i]) {
            float s[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = 0.f;
            for (int y = 0; y < g.RL; ++y)
#pragma unroll
                for (int j = 0; j < 8; ++j) s[j] += red[((y << g.lsh) + t.lx) * 8 + j];
            store8<float>(dst + t.c0[i], s);
        }
    }
}

// ---- spatial gate ----------------------------------------------------------------------------------------------------------------------
// grid (nblk, B); partial: [B][nblk][C]
template <typename T, int NI>
__global__ void __launch_bounds__(TM_THREADS) spatial_gate_fwd_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ r,
                                                                      const float* __restrict__ w, float* __restrict__ s,
                                                                      T* __restrict__ y, int64_t ldy, float* __restrict__ partial,
                                                                      const TmGeom g) {
    __shared__ float red[TM_THREADS * 8];
    const TmLane<NI> t(g);
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * g.rpb, r1 = min(g.HW, r0 + g.rpb);
    float wv[NI][8], acc[NI][8];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        tm_ldf(w + t.c0[i], t.ok[i], wv[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    }
    for (int base = r0; base < r1; base += g.RL) {
        const int rr = base + t.ty;
        const bool act = rr < r1;
        const int64_t m = (int64_t)b * g.HW + rr;
        Raw8<T> rw[NI], xr[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            rw[i] = tm_ld<T>(r + m * g.C + t.c0[i], act && t.ok[i]);
            xr[i] = tm_ld<T>(x + m * ldx + t.c0[i], act && t.ok[i]);
        }
        SEGF_LOADS_ISSUED();
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            float v[8];
            unpack8(rw[i], v);
#pragma unroll
            for (int j = 0; j < 8; ++j) dot = fmaf(v[j], wv[i][j], dot);
        }
        dot = wave_sum(dot, g.L);
        const float sv = 1.f / (1.f + __expf(-dot));
        if (act && t.lx == 0) s[m] = sv;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (act && t.ok[i]) {
                float v[8];
                unpack8(xr[i], v);
#pragma unroll
                for (int j = 0; j < 8; ++j) { v[j] *= sv; acc[i][j] += v[j]; }
                store8<T>(y + m * ldy + t.c0[i], v);
            }
        }
    }
    tm_block_tail<NI>(acc, t, g, partial + ((int64_t)b * gridDim.x + blockIdx.x) * g.C, red);
}

// grid (nblk, B); partial: [B nblk][C] (the dw slabs of all samples: one reduction over all of them)
template <typename T, int NI>
__global__ void __launch_bounds__(TM_THREADS) spatial_gate_bwd_kernel(const T* __restrict__ dy, int64_t lddy, const float* __restrict__ dpool,
                                                                      const T* __restrict__ x, int64_t ldx, const T* __restrict__ r,
                                                                      const float* __restrict__ s, const float* __restrict__ w,
                                                                      T* __restrict__ dx, int64_t lddx, T* __restrict__ dr,
                                                                      float* __restrict__ partial, const TmGeom g) {
    __shared__ float red[TM_THREADS * 8];
    const TmLane<NI> t(g);
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * g.rpb, r1 = min(g.HW, r0 + g.rpb);
    float wv[NI][8], dp[NI][8], acc[NI][8];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        tm_ldf(w + t.c0[i], t.ok[i], wv[i]);
        tm_ldf(dpool + (int64_t)b * g.C + t.c0[i], t.ok[i] && dpool != nullptr, dp[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    }
    for (int base = r0; base < r1; base += g.RL) {
        const int rr = base + t.ty;
        const bool act = rr < r1;
        const int64_t m = (int64_t)b * g.HW + rr;
        Raw8<T> gr[NI], xr[NI], rw[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            gr[i] = tm_ld<T>(dy + m * lddy + t.c0[i], act && t.ok[i]);
            xr[i] = tm_ld<T>(x + m * ldx + t.c0[i], act && t.ok[i]);
            rw[i] = tm_ld<T>(r + m * g.C + t.c0[i], act && t.ok[i]);
        }
        const float sv = act ? s[m] : 0.f;
        SEGF_LOADS_ISSUED();
        float ds = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            float gv[8], xv[8];
            unpack8(gr[i], gv);
            unpack8(xr[i], xv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                gv[j] += dp[i][j];
                ds = fmaf(gv[j], xv[j], ds);
                gv[j] *= sv;
            }
            if (act && t.ok[i]) store8<T>(dx + m * lddx + t.c0[i], gv);
        }
        ds = wave_sum(ds, g.L);
        const float dl = ds * sv * (1.f - sv);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (act && t.ok[i]) {
                float rv[8], o[8];
                unpack8(rw[i], rv);
#pragma unroll
                for (int j = 0; j < 8; ++j) { o[j] = dl * wv[i][j]; acc[i][j] = fmaf(dl, rv[j], acc[i][j]); }
                store8<T>(dr + m * g.C + t.c0[i], o);
            }
        }
    }
    tm_block_tail<NI>(acc, t, g, partial + ((int64_t)b * gridDim.x + blockIdx.x) * g.C, red);
}

// ---- channel gate mix ------------------------------------------------------------------------------------------------------------------
template <typename T, int NI>
__global__ void __launch_bounds__(TM_THREADS) channel_gate_mix_fwd_kernel(const T* __restrict__ q1, int64_t ldq, const T* __restrict__ k1,
                                                                          int64_t ldk, const float* __restrict__ gq,
                                                                          const float* __restrict__ gk, T* __restrict__ u, int64_t ldu,
                                                                          const TmGeom g) {
    const TmLane<NI> t(g);
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * g.rpb, r1 = min(g.HW, r0 + g.rpb);
    float a[NI][8], c[NI][8];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        tm_ldf(gq + (int64_t)b * g.C + t.c0[i], t.ok[i], a[i]);
        tm_ldf(gk + (int64_t)b * g.C + t.c0[i], t.ok[i], c[i]);
    }
    for (int rr = r0 + t.ty; rr < r1; rr += g.RL) {
        const int64_t m = (int64_t)b * g.HW + rr;
        Raw8<T> qr[NI], kr[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            qr[i] = tm_ld<T>(q1 + m * ldq + t.c0[i], t.ok[i]);
            kr[i] = tm_ld<T>(k1 + m * ldk + t.c0[i], t.ok[i]);
        }
        SEGF_LOADS_ISSUED();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (t.ok[i]) {
                float qv[8], kv[8];
                unpack8(qr[i], qv);
                unpack8(kr[i], kv);
#pragma unroll
                for (int j = 0; j < 8; ++j) qv[j] = fmaf(qv[j], a[i][j], kv[j] * c[i][j]);
                store8<T>(u + m * ldu + t.c0[i], qv);
            }
        }
    }
}

// grid (nblk, B); pq / pk: [B][nblk][C] each
template <typename T, int NI>
__global__ void __launch_bounds__(TM_THREADS) channel_gate_mix_bwd_kernel(const T* __restrict__ du, int64_t lddu, const T* __restrict__ q1,
                                                                          int64_t ldq, const T* __restrict__ k1, int64_t ldk,
                                                                          const float* __restrict__ gq, const float* __restrict__ gk,
                                                                          T* __restrict__ dq1, int64_t lddq, T* __restrict__ dk1,
                                                                          int64_t lddk, float* __restrict__ pq, float* __restrict__ pk,
                                                                          const TmGeom g) {
    __shared__ float red[TM_THREADS * 8];
    const TmLane<NI> t(g);
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * g.rpb, r1 = min(g.HW, r0 + g.rpb);
    float a[NI][8], c[NI][8], aq[NI][8], ak[NI][8];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        tm_ldf(gq + (int64_t)b * g.C + t.c0[i], t.ok[i], a[i]);
        tm_ldf(gk + (int64_t)b * g.C + t.c0[i], t.ok[i], c[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) { aq[i][j] = 0.f; ak[i][j] = 0.f; }
    }
    for (int rr = r0 + t.ty; rr < r1; rr += g.RL) {
        const int64_t m = (int64_t)b * g.HW + rr;
        Raw8<T> dr[NI], qr[NI], kr[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            dr[i] = tm_ld<T>(du + m * lddu + t.c0[i], t.ok[i]);
            qr[i] = tm_ld<T>(q1 + m * ldq + t.c0[i], t.ok[i]);
            kr[i] = tm_ld<T>(k1 + m * ldk + t.c0[i], t.ok[i]);
        }
        SEGF_LOADS_ISSUED();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (t.ok[i]) {
                float dv[8], qv[8], kv[8], oq[8], ok_[8];
                unpack8(dr[i], dv);
                unpack8(qr[i], qv);
                unpack8(kr[i], kv);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    oq[j] = dv[j] * a[i][j];
                    ok_[j] = dv[j] * c[i][j];
                    aq[i][j] = fmaf(dv[j], qv[j], aq[i][j]);
                    ak[i][j] = fmaf(dv[j], kv[j], ak[i][j]);
                }
                store8<T>(dq1 + m * lddq + t.c0[i], oq);
                store8<T>(dk1 + m * lddk + t.c0[i], ok_);
            }
        }
    }
    const int64_t slab = ((int64_t)b * gridDim.x + blockIdx.x) * g.C;
    tm_block_tail<NI>(aq, t, g, pq + slab, red);
    tm_block_tail<NI>(ak, t, g, pk + slab, red);
}

// ---- gated product (B = 1, HW = M in the geometry) ------------------------------------------------------------------------------------------
template <typename T, int NI>
__global__ void __launch_bounds__(TM_THREADS) gated_mul_fwd_kernel(const T* __restrict__ a, int64_t lda, const T* __restrict__ v, int64_t ldv,
                                                                   T* __restrict__ z, int64_t ldz, const TmGeom g) {
    const TmLane<NI> t(g);
    const int r0 = blockIdx.x * g.rpb, r1 = min(g.HW, r0 + g.rpb);
    for (int rr = r0 + t.ty; rr < r1; rr += g.RL) {
        const int64_t m = rr;
        Raw8<T> ar[NI], vr[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            ar[i] = tm_ld<T>(a + m * lda + t.c0[i], t.ok[i]);
            vr[i] = tm_ld<T>(v + m * ldv + t.c0[i], t.ok[i]);
        }
        SEGF_LOADS_ISSUED();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (t.ok[i]) {
                float av[8], vv[8];
                unpack8(ar[i], av);
                unpack8(vr[i], vv);
#pragma unroll
                for (int j = 0; j < 8; ++j) av[j] *= vv[j];
                store8<T>(z + m * ldz + t.c0[i], av);
            }
        }
    }
}

template <typename T, int NI>
__global__ void __launch_bounds__(TM_THREADS) gated_mul_bwd_kernel(const T* __restrict__ dz, int64_t lddz, const T* __restrict__ a, int64_t lda,
                                                                   const T* __restrict__ v, int64_t ldv, T* __restrict__ da, int64_t ldda,
                                                                   T* __restrict__ dv, int64_t lddv, const TmGeom g) {
    const TmLane<NI> t(g);
    const int r0 = blockIdx.x * g.rpb, r1 = min(g.HW, r0 + g.rpb);
    for (int rr = r0 + t.ty; rr < r1; rr += g.RL) {
        const int64_t m = rr;
        Raw8<T> dr[NI], ar[NI], vr[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            dr[i] = tm_ld<T>(dz + m * lddz + t.c0[i], t.ok[i]);
            ar[i] = tm_ld<T>(a + m * lda + t.c0[i], t.ok[i]);
            vr[i] = tm_ld<T>(v + m * ldv + t.c0[i], t.ok[i]);
        }
        SEGF_LOADS_ISSUED();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (t.ok[i]) {
                float d[8], av[8], vv[8];
                unpack8(dr[i], d);
                unpack8(ar[i], av);
                unpack8(vr[i], vv);
#pragma unroll
                for (int j = 0; j < 8; ++j) { vv[j] *= d[j]; av[j] *= d[j]; }
                store8<T>(da + m * ldda + t.c0[i], vv);
                store8<T>(dv + m * lddv + t.c0[i], av);
            }
        }
    }
}

}  // namespace

// launch with the chunk count per lane as a template argument
#define TM_LAUNCH(dt, g, kernel, grid, st, ...)                                                                              \
    SEGF_DISPATCH_DT(dt, T, {                                                                                                \
        if ((g).NI == 1) hipLaunchKernelGGL((kernel<T, 1>), grid, dim3(TM_THREADS), 0, st, __VA_ARGS__);                     \
        else hipLaunchKernelGGL((kernel<T, 2>), grid, dim3(TM_THREADS), 0, st, __VA_ARGS__);                                 \
    })

extern "C" int segf_spatial_gate_supported(int dt, int B, int HW, int C, int64_t ld) {
    TmGeom g;
    return tm_dt_ok(dt) && tm_geom(B, HW, C, g) && tm_ld_ok(dt, C, ld);
}

extern "C" int64_t segf_spatial_gate_fwd_ws(int B, int HW, int C) {
    TmGeom g;
    if (!tm_geom(B, HW, C, g)) return 0;
    return (int64_t)B * g.nblk * C;
}

extern "C" int segf_spatial_gate_fwd(int dt, int B, int HW, int C, const void* x, int64_t ldx, const void* r, const float* w, float* s,
                                     void* y, int64_t ldy, float* pool, float* ws, void* stream) {
    TmGeom g;
    if (!tm_dt_ok(dt)) return SEGF_ERR_DTYPE;
    if (!tm_geom(B, HW, C, g)) return SEGF_ERR_SHAPE;                    // before any launch
    if (!tm_op_ok(dt, C, x, ldx) || !tm_op_ok(dt, C, r, C) || !tm_op_ok(dt, C, y, ldy) || !tm_f32_ok(w) || !s || !tm_f32_ok(pool))
        return SEGF_ERR_SHAPE;
    if (!tm_f32_ok(ws)) return SEGF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.nblk, (unsigned)B);
    TM_LAUNCH(dt, g, spatial_gate_fwd_kernel, grid, st, (const T*)x, ldx, (const T*)r, w, s, (T*)y, ldy, ws, g)
    SEGF_CHECK_LAUNCH();
    colreduce_finalize_launch(ws, g.nblk, C, pool, st, B);
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t segf_spatial_gate_bwd_ws(int B, int HW, int C) { return segf_spatial_gate_fwd_ws(B, HW, C); }

extern "C" int segf_spatial_gate_bwd(int dt, int B, int HW, int C, const void* dy, int64_t lddy, const float* dpool, const void* x,
                                     int64_t ldx, const void* r, const float* s, const float* w, void* dx, int64_t lddx, void* dr,
                                     float* dw, float* ws, void* stream) {
    TmGeom g;
    if (!tm_dt_ok(dt)) return SEGF_ERR_DTYPE;
    if (!tm_geom(B, HW, C, g)) return SEGF_ERR_SHAPE;
    if (!tm_op_ok(dt, C, dy, lddy) || !tm_op_ok(dt, C, x, ldx) || !tm_op_ok(dt, C, r, C) || !tm_op_ok(dt, C, dx, lddx) ||
        !tm_op_ok(dt, C, dr, C) || !tm_f32_ok(w) || !s || !tm_f32_ok(dw) || (dpool && !tm_f32_ok(dpool)))
        return SEGF_ERR_SHAPE;
    if (!tm_f32_ok(ws)) return SEGF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.nblk, (unsigned)B);
    TM_LAUNCH(dt, g, spatial_gate_bwd_kernel, grid, st, (const T*)dy, lddy, dpool, (const T*)x, ldx, (const T*)r, s, w, (T*)dx, lddx, (T*)dr,
              ws, g)
    SEGF_CHECK_LAUNCH();
    colreduce_finalize_launch(ws, B * g.nblk, C, dw, st);
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int segf_channel_gate_mix_supported(int dt, int B, int HW, int C, int64_t ld) {
    return segf_spatial_gate_supported(dt, B, HW, C, ld);
}

extern "C" int segf_channel_gate_mix_fwd(int dt, int B, int HW, int C, const void* q1, int64_t ldq, const void* k1, int64_t ldk,
                                         const float* gq, const float* gk, void* u, int64_t ldu, void* stream) {
    TmGeom g;
    if (!tm_dt_ok(dt)) return SEGF_ERR_DTYPE;
    if (!tm_geom(B, HW, C, g)) return SEGF_ERR_SHAPE;
    if (!tm_op_ok(dt, C, q1, ldq) || !tm_op_ok(dt, C, k1, ldk) || !tm_op_ok(dt, C, u, ldu) || !tm_f32_ok(gq) || !tm_f32_ok(gk))
        return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.nblk, (unsigned)B);
    TM_LAUNCH(dt, g, channel_gate_mix_fwd_kernel, grid, st, (const T*)q1, ldq, (const T*)k1, ldk, gq, gk, (T*)u, ldu, g)
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t segf_channel_gate_mix_bwd_ws(int B, int HW, int C) { return 2 * segf_spatial_gate_fwd_ws(B, HW, C); }

extern "C" int segf_channel_gate_mix_bwd(int dt, int B, int HW, int C, const void* du, int64_t lddu, const void* q1, int64_t ldq,
                                         const void* k1, int64_t ldk, const float* gq, const float* gk, void* dq1, int64_t lddq, void* dk1,
                                         int64_t lddk, float* dgq, float* dgk, float* ws, void* stream) {
    TmGeom g;
    if (!tm_dt_ok(dt)) return SEGF_ERR_DTYPE;
    if (!tm_geom(B, HW, C, g)) return SEGF_ERR_SHAPE;
    if (!tm_op_ok(dt, C, du, lddu) || !tm_op_ok(dt, C, q1, ldq) || !tm_op_ok(dt, C, k1, ldk) || !tm_op_ok(dt, C, dq1, lddq) ||
        !tm_op_ok(dt, C, dk1, lddk) || !tm_f32_ok(gq) || !tm_f32_ok(gk) || !tm_f32_ok(dgq) || !tm_f32_ok(dgk))
        return SEGF_ERR_SHAPE;
    if (!tm_f32_ok(ws)) return SEGF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.nblk, (unsigned)B);
    float* pq = ws;
    float* pk = ws + (int64_t)B * g.nblk * C;
    TM_LAUNCH(dt, g, channel_gate_mix_bwd_kernel, grid, st, (const T*)du, lddu, (const T*)q1, ldq, (const T*)k1, ldk, gq, gk, (T*)dq1, lddq,
              (T*)dk1, lddk, pq, pk, g)
    SEGF_CHECK_LAUNCH();
    colreduce_finalize_launch(pq, g.nblk, C, dgq, st, B);
    SEGF_CHECK_LAUNCH();
    colreduce_finalize_launch(pk, g.nblk, C, dgk, st, B);
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int segf_gated_mul_supported(int dt, int M, int C, int64_t ld) { return segf_spatial_gate_supported(dt, 1, M, C, ld); }

extern "C" int segf_gated_mul_fwd(int dt, int M, int C, const void* a, int64_t lda, const void* v, int64_t ldv, void* z, int64_t ldz,
                                  void* stream) {
    TmGeom g;
    if (!tm_dt_ok(dt)) return SEGF_ERR_DTYPE;
    if (!tm_geom(1, M, C, g)) return SEGF_ERR_SHAPE;
    if (!tm_op_ok(dt, C, a, lda) || !tm_op_ok(dt, C, v, ldv) || !tm_op_ok(dt, C, z, ldz)) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.nblk);
    TM_LAUNCH(dt, g, gated_mul_fwd_kernel, grid, st, (const T*)a, lda, (const T*)v, ldv, (T*)z, ldz, g)
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int segf_gated_mul_bwd(int dt, int M, int C, const void* dz, int64_t lddz, const void* a, int64_t lda, const void* v, int64_t ldv,
                                  void* da, int64_t ldda, void* dv, int64_t lddv, void* stream) {
    TmGeom g;
    if (!tm_dt_ok(dt)) return SEGF_ERR_DTYPE;
    if (!tm_geom(1, M, C, g)) return SEGF_ERR_SHAPE;
    if (!tm_op_ok(dt, C, dz, lddz) || !tm_op_ok(dt, C, a, lda) || !tm_op_ok(dt, C, v, ldv) || !tm_op_ok(dt, C, da, ldda) ||
        !tm_op_ok(dt, C, dv, lddv))
        return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.nblk);
    TM_LAUNCH(dt, g, gated_mul_bwd_kernel, grid, st, (const T*)dz, lddz, (const T*)a, lda, (const T*)v, ldv, (T*)da, ldda, (T*)dv, lddv, g)
    SEGF_CHECK_LAUNCH();
    return 0;
}
