// Per-pixel losses on the fused low-resolution loss path: online hard-example mining (OHEM) and focal loss.
//   reference: util/losses.py:9-26 (FocalLoss), :44-66 (OhemCrossEntropy), models/build_models.py:65 (the final resize).
// Forward: every full-resolution pixel's cross entropy ce = w[t] * (logsumexp(z) - z_t) is formed in fp32 from the stored low-res
// taps (whatever the storage type, so bf16 and fp32 runs select by the same function of the same numbers) and written to an fp32
// map [B][H][W] (4 bytes per pixel; the logits the reference materialises are C times that), clamped to >= +0.  Integer counts go
// through integer atomics, float sums through per-workgroup partials that one workgroup adds in float64 in a fixed order: there
// is no floating-point atomic in this file and every result is bitwise reproducible.
// Selection (OHEM): the reference decides on the host between {ce > theta} and loss.topk(n_min) (losses.py:58).  Here the finalize
// kernel leaves used_topk = (n_hard < n_min) on the device and the top-k kernels, which are launched on every step, return at
// once when it is 0: the launch sequence is static and replays in a hipGraph whichever branch the data takes.  The n_min-th
// largest value kappa is found by a radix select over the uint32 patterns of the map (monotone: every value is >= +0), four
// 8-bit digits, each an integer histogram (LDS, then one integer atomic per bin per workgroup) and a one-workgroup pick.
// Ties at kappa: torch.topk keeps arbitrary members; here every pixel with ce == kappa receives the share
// (n_min - n_gt) / (n_eq * n_min) -- the loss equals the reference's, the gradient is a deterministic member of its possible ones.
// Backward: coef(pixel) * w[t] * (softmax - onehot) scattered through the transposed resize onto the low-res taps with the tile /
// parity-colour structure of tile_cells_walk (loss_geom.h); the side of the decision value is read from the SAVED map, so
// forward and backward agree on every pixel.  Non-power-of-two ratios stage the full-resolution gradient and use segf_bilinear_bwd.
// The class-row helpers (tap loads, wave softmax, cell taps and bound) are those of loss_geom.h; the backward keeps its own copy of the walk.
#include "loss_geom.h"

namespace {

enum { PXS_NVALID = 0, PXS_NMIN, PXS_NHARD, PXS_NGT, PXS_NEQ, PXS_TOPK, PXS_KAPPA, PXS_BAD, PXS_NSEL, PXS_PREFIX, PXS_KREM,
       PXS_HEAD = 16, PXS_HIST = 4 * 256 };
#define PX_RBLK 256        // workgroups of the map passes (histograms, top-k sum)
#define PX_MODE_OHEM 0
#define PX_MODE_FOCAL 1

struct PixelParams { int mode; float p0, p1; int size_average; };     // OHEM: p0 = theta; focal: p0 = alpha, p1 = gamma

__device__ __forceinline__ int ld_state(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// upsampled logits of one pixel at ATen's source index and tap weights (any ratio); invalid class slots get -inf.  pixel_logits
// (loss_geom.h) without its same-size branch, which no caller here can reach and which costs pixel_loss_fwd_kernel<T, 3> a wave of
// occupancy (SGPRs)
template <typename T, int NS>
__device__ __forceinline__ void px_pixel_logits(const T* __restrict__ img, const LossGeom& g, int Y, int X, int lane, float (&z)[NS]) {
    int y0, y1, x0, x1; float ly, lx;
    bilinear_src(Y, g.h, g.H, 0, y0, y1, ly);
    bilinear_src(X, g.w, g.W, 0, x0, x1, lx);
    const T* p00 = img + ((int64_t)y0 * g.w + x0) * g.ldl;
    const T* p01 = img + ((int64_t)y0 * g.w + x1) * g.ldl;
    const T* p10 = img + ((int64_t)y1 * g.w + x0) * g.ldl;
    const T* p11 = img + ((int64_t)y1 * g.w + x1) * g.ldl;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = lane + 64 * s, ci = c < g.C ? c : g.C - 1;
        const float a = ldf<T>(p00 + ci), b = ldf<T>(p01 + ci), cc = ldf<T>(p10 + ci), d = ldf<T>(p11 + ci);
        z[s] = c < g.C ? (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * cc + lx * d) : -INFINITY;
    }
}

// focal: f = alpha (1 - pt)^gamma ce; its derivative with respect to ce, without alpha: (1 - pt)^gamma + gamma (1 - pt)^(gamma-1) pt ce
__device__ __forceinline__ float px_pow(float q, float gamma) {
    return gamma == 0.f ? 1.f : (gamma == 1.f ? q : (gamma == 2.f ? q * q : (q > 0.f ? __powf(q, gamma) : 0.f)));
}
__device__ __forceinline__ float focal_value(float ce, float gamma) {
    return px_pow(-expm1f(-ce), gamma) * ce;
}
__device__ __forceinline__ float focal_slope(float ce, float gamma) {
    const float q = -expm1f(-ce);
    float v = px_pow(q, gamma);
    if (gamma != 0.f && ce != 0.f) v += gamma * px_pow(q, gamma - 1.f) * (1.f - q) * ce;
    return v;
}

// what the forward kernels keep per lane, and how a workgroup hands it on: integer atomics for the counts, one float partial
struct PxAcc { int nvalid, nhard, bad; float sum; };
__device__ __forceinline__ void px_account(PxAcc& a, float ce, const PixelParams& pp) {
    if (pp.mode == PX_MODE_OHEM) { if (ce > pp.p0) { a.nhard += 1; a.sum += ce; } }
    else a.sum += focal_value(ce, pp.p1);
}
__device__ __forceinline__ void px_block_tail(const PxAcc& a, int* __restrict__ state, float* __restrict__ dst) {
    __shared__ float fred[LS_THREADS];
    __shared__ int ired[3];
    if (threadIdx.x < 3) ired[threadIdx.x] = 0;
    fred[threadIdx.x] = a.sum;
    __syncthreads();
    if (a.nvalid) atomicAdd(&ired[0], a.nvalid);
    if (a.nhard) atomicAdd(&ired[1], a.nhard);
    if (a.bad) atomicOr(&ired[2], 1);
    for (int o = LS_THREADS / 2; o > 0; o >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < o) fred[threadIdx.x] += fred[threadIdx.x + o];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        dst[0] = fred[0];
        if (ired[0]) atomicAdd(state + PXS_NVALID, ired[0]);
        if (ired[1]) atomicAdd(state + PXS_NHARD, ired[1]);
        if (ired[2]) atomicOr(state + PXS_BAD, 1);
    }
}

__global__ void __launch_bounds__(256) pixel_loss_zero_state_kernel(int* __restrict__ state) {
    for (int i = threadIdx.x; i < PXS_HEAD + PXS_HIST; i += 256) state[i] = 0;
}

// ---- forward over cells (power-of-two ratios; sc == 1: the cell is the pixel itself) -----------------------------------------
// A wave owns a cell: the sc x sc pixels that interpolate between the same four taps; the classes are spread over the lanes.
template <typename T, int NS>
__global__ void __launch_bounds__(LS_THREADS) pixel_loss_fwd_cells_kernel(const T* __restrict__ logits, LossGeom g, int sc,
                                                                           const int64_t* __restrict__ target, int64_t ignore_index,
                                                                           const float* __restrict__ cw, PixelParams pp,
                                                                           float* __restrict__ ce_map, int* __restrict__ state,
                                                                           float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int halo = sc > 1 ? 1 : 0, off = sc >> 1;
    const float inv_sc = 1.f / (float)sc, fhalo = (float)halo;
    const int ncx = g.w + halo, ncell = (g.h + halo) * ncx;
    const T* img = logits + (int64_t)b * g.h * g.w * g.ldl;
    const int64_t* tg = target + (int64_t)b * g.H * g.W;
    float* cm = ce_map + (int64_t)b * g.H * g.W;
    PxAcc acc{0, 0, 0, 0.f};
    for (int cell = blockIdx.x * 4 + wave; cell < ncell; cell += gridDim.x * 4) {
        // clamps and loads written out, not make_cell / load_cell_taps: with them the ratio-8 forward was 0.7 % slower, outside the
        // parent-to-parent spread (profiles/loss_rows.md)
        const int cj = cell / ncx - halo, ck = cell % ncx - halo;
        const int y0 = cj < 0 ? 0 : cj, y1 = cj + halo > g.h - 1 ? g.h - 1 : cj + halo;
        const int x0 = ck < 0 ? 0 : ck, x1 = ck + halo > g.w - 1 ? g.w - 1 : ck + halo;
        float t00[NS], t01[NS], t10[NS], t11[NS];
        load_tap<T, NS>(img + ((int64_t)y0 * g.w + x0) * g.ldl, lane, g.C, t00);
        load_tap<T, NS>(img + ((int64_t)y0 * g.w + x1) * g.ldl, lane, g.C, t01);
        load_tap<T, NS>(img + ((int64_t)y1 * g.w + x0) * g.ldl, lane, g.C, t10);
        load_tap<T, NS>(img + ((int64_t)y1 * g.w + x1) * g.ldl, lane, g.C, t11);
        // this lane's pixel of the cell (lane = a * sc + bb): code = class, -1 ignored, -2 out of range, -3 outside the image
        // (not cell_label_codes: an ignored pixel inside the image still gets its +0.0 written, so "outside" needs a code of its own)
        int code = -3, myY = 0, myX = 0;
        if (lane < sc * sc) {
            const int a = lane / sc;
            myY = sc * cj + off + a; myX = sc * ck + off + (lane - a * sc);
            if (myY >= 0 && myY < g.H && myX >= 0 && myX < g.W) {
                const int64_t t = tg[(int64_t)myY * g.W + myX];
                code = t == ignore_index ? -1 : ((t < 0 || t >= g.C) ? -2 : (int)t);
            }
        }
        float myce = 0.f;
        for (int a = 0; a < sc; ++a) {
            const int Y = sc * cj + off + a;
            if (Y < 0 || Y >= g.H) continue;
            const float ly = (a + 0.5f) * inv_sc * fhalo;
            float L[NS], R[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                L[s] = (1.f - ly) * t00[s] + ly * t10[s];
                R[s] = (1.f - ly) * t01[s] + ly * t11[s];
            }
            for (int bb = 0; bb < sc; ++bb) {
                const int t = __builtin_amdgcn_readlane(code, a * sc + bb);      // wave-uniform
                if (t < 0) continue;
                const float lx = (bb + 0.5f) * inv_sc * fhalo;
                float z[NS], pr[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) z[s] = (lane + 64 * s) < g.C ? (1.f - lx) * L[s] + lx * R[s] : -INFINITY;
                float mx;
                const float lsum = wave_softmax<NS>(z, pr, mx);
                const float ce = fmaxf((cw ? cw[t] : 1.f) * (lsum - (px_label_logit<NS>(z, t) - mx)), 0.f);
                if (lane == a * sc + bb) myce = ce;
            }
        }
        if (code != -3) {
            cm[(int64_t)myY * g.W + myX] = myce;            // ignored and out-of-range labels: +0.0
            if (code >= 0) acc.nvalid += 1;
            if (code == -2) acc.bad = 1;
            px_account(acc, myce, pp);
        }
    }
    px_block_tail(acc, state, partial + (int64_t)blockIdx.x * g.B + b);
}

// any ratio: one wave per full-resolution pixel at a time, ATen's source index and weights per pixel
template <typename T, int NS>
__global__ void __launch_bounds__(LS_THREADS) pixel_loss_fwd_kernel(const T* __restrict__ logits, LossGeom g,
                                                                     const int64_t* __restrict__ target, int64_t ignore_index,
                                                                     const float* __restrict__ cw, PixelParams pp,
                                                                     float* __restrict__ ce_map, int* __restrict__ state,
                                                                     float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    const int64_t npix = (int64_t)g.H * g.W;
    int64_t p0, p1;
    wave_pixel_range(npix, p0, p1);
    const T* img = logits + (int64_t)b * g.h * g.w * g.ldl;
    const int64_t* tg = target + (int64_t)b * npix;
    float* cm = ce_map + (int64_t)b * npix;
    PxAcc acc{0, 0, 0, 0.f};
    for (int64_t p = p0; p < p1; ++p) {
        const int64_t t = tg[p];
        float ce = 0.f;
        const bool ok = t != ignore_index && t >= 0 && t < g.C;
        if (ok) {
            const int Y = (int)(p / g.W), X = (int)(p - (int64_t)Y * g.W);
            float z[NS], pr[NS];
            px_pixel_logits<T, NS>(img, g, Y, X, lane, z);
            float mx;
            const float lsum = wave_softmax<NS>(z, pr, mx);
            ce = fmaxf((cw ? cw[t] : 1.f) * (lsum - (px_label_logit<NS>(z, (int)t) - mx)), 0.f);
        }
        if (lane == 0) {
            cm[p] = ce;
            if (ok) acc.nvalid += 1;
            else if (t != ignore_index) acc.bad = 1;
            px_account(acc, ce, pp);
        }
    }
    px_block_tail(acc, state, partial + (int64_t)blockIdx.x * g.B + b);
}

// one workgroup: add n float partials in float64 (thread-strided, then a fixed tree); every thread returns the total
__device__ __forceinline__ double px_sum_partials(const float* __restrict__ partial, int n) {
    __shared__ double dred[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)partial[i];
    dred[threadIdx.x] = s;
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < o) dred[threadIdx.x] += dred[threadIdx.x + o];
    }
    __syncthreads();
    return dred[0];
}

__global__ void __launch_bounds__(256) pixel_loss_finalize_kernel(int* __restrict__ state, const float* __restrict__ partial, int npart,
                                                                   PixelParams pp, int64_t npix, float* __restrict__ loss) {
    const double total = px_sum_partials(partial, npart);
    if (threadIdx.x != 0) return;
    const int nvalid = ld_state(state + PXS_NVALID), nhard = ld_state(state + PXS_NHARD);
    if (pp.mode == PX_MODE_FOCAL) {
        loss[0] = (float)((double)pp.p0 * total / (pp.size_average ? (double)npix : 1.0));
        state[PXS_NSEL] = pp.size_average ? (int)npix : 1;
        return;
    }
    const int nmin = nvalid / 16;
    const int topk = nhard < nmin ? 1 : 0;
    state[PXS_NMIN] = nmin; state[PXS_TOPK] = topk;
    state[PXS_PREFIX] = 0; state[PXS_KREM] = nmin;
    if (!topk) {
        state[PXS_NGT] = nhard; state[PXS_NEQ] = 0; state[PXS_NSEL] = nhard;
        reinterpret_cast<float*>(state)[PXS_KAPPA] = pp.p0;
        loss[0] = nhard ? (float)(total / (double)nhard) : __builtin_nanf("");      // torch.mean of an empty selection
    }
}

// ---- top-k branch: radix select of the n_min-th largest pattern, idle unless used_topk ------------------------------------
__global__ void __launch_bounds__(256) pixel_loss_select_hist_kernel(const uint32_t* __restrict__ bits, int64_t n, int pass,
                                                                      int* __restrict__ state) {
    if (ld_state(state + PXS_TOPK) == 0) return;
    __shared__ int hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t prefix = (uint32_t)ld_state(state + PXS_PREFIX);
    const uint32_t hmask = pass ? 0xffffffffu << (shift + 8) : 0u;      // digits already fixed by the earlier passes
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint32_t v = bits[i];
        if ((v & hmask) == (prefix & hmask)) atomicAdd(&hist[(v >> shift) & 255u], 1);
    }
    __syncthreads();
    const int c = hist[threadIdx.x];
    if (c) atomicAdd(state + PXS_HEAD + 256 * pass + threadIdx.x, c);
}
__global__ void __launch_bounds__(64) pixel_loss_select_pick_kernel(int pass, int* __restrict__ state) {
    if (ld_state(state + PXS_TOPK) == 0 || threadIdx.x != 0) return;
    const int* hist = state + PXS_HEAD + 256 * pass;
    int k = ld_state(state + PXS_KREM), bin = 255;
    for (; bin > 0; --bin) {                    // from the largest digit down: the bin that holds the k-th largest
        const int c = ld_state(hist + bin);
        if (c >= k) break;
        k -= c;
    }
    state[PXS_KREM] = k;
    state[PXS_PREFIX] = (int)((uint32_t)ld_state(state + PXS_PREFIX) | ((uint32_t)bin << (24 - 8 * pass)));
}
// sum of the values above kappa per workgroup (fixed grid, fixed order), integer counts of the values above / equal
__global__ void __launch_bounds__(256) pixel_loss_topk_sum_kernel(const float* __restrict__ ce_map, int64_t n, int* __restrict__ state,
                                                                   float* __restrict__ partial) {
    if (ld_state(state + PXS_TOPK) == 0) return;
    __shared__ float fred[256];
    __shared__ int ired[2];
    if (threadIdx.x < 2) ired[threadIdx.x] = 0;
    const float kappa = __int_as_float(ld_state(state + PXS_PREFIX));
    float s = 0.f; int ngt = 0, neq = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = ce_map[i];
        if (v > kappa) { s += v; ngt += 1; }
        else if (v == kappa) neq += 1;
    }
    fred[threadIdx.x] = s;
    __syncthreads();
    if (ngt) atomicAdd(&ired[0], ngt);
    if (neq) atomicAdd(&ired[1], neq);
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < o) fred[threadIdx.x] += fred[threadIdx.x + o];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = fred[0];
        if (ired[0]) atomicAdd(state + PXS_NGT, ired[0]);
        if (ired[1]) atomicAdd(state + PXS_NEQ, ired[1]);
    }
}
__global__ void __launch_bounds__(256) pixel_loss_topk_final_kernel(int* __restrict__ state, const float* __restrict__ partial, int npart,
                                                                     float* __restrict__ loss) {
    if (ld_state(state + PXS_TOPK) == 0) return;
    const double total = px_sum_partials(partial, npart);
    if (threadIdx.x != 0) return;
    const int nmin = ld_state(state + PXS_NMIN), ngt = ld_state(state + PXS_NGT);
    const float kappa = __int_as_float(ld_state(state + PXS_PREFIX));
    reinterpret_cast<float*>(state)[PXS_KAPPA] = kappa;
    state[PXS_NSEL] = nmin;
    loss[0] = (float)((total + (double)(nmin - ngt) * (double)kappa) / (double)nmin);
}

// ---- backward --------------------------------------------------------------------------------------------------
// coefficient of d ce(pixel): everything a pixel needs besides its own saved ce
struct PxCoef { int mode; float thr, c_gt, c_eq, gamma; };
__device__ __forceinline__ PxCoef px_coef_setup(const int* __restrict__ state, const PixelParams& pp, const float* __restrict__ grad_out) {
    const float go = grad_out ? grad_out[0] : 1.f;
    PxCoef c; c.mode = pp.mode; c.gamma = pp.p1; c.c_eq = 0.f;
    const int nsel = ld_state(state + PXS_NSEL);
    if (pp.mode == PX_MODE_FOCAL) { c.thr = 0.f; c.c_gt = go * pp.p0 / (float)nsel; return c; }
    c.thr = __int_as_float(ld_state(state + PXS_KAPPA));
    c.c_gt = nsel > 0 ? go / (float)nsel : 0.f;
    if (ld_state(state + PXS_TOPK)) {
        const int nmin = ld_state(state + PXS_NMIN), ngt = ld_state(state + PXS_NGT), neq = ld_state(state + PXS_NEQ);
        c.c_eq = neq > 0 ? go * (float)(nmin - ngt) / ((float)neq * (float)nmin) : 0.f;
    }
    return c;
}
__device__ __forceinline__ float px_coef(const PxCoef& c, float ce) {
    if (c.mode == PX_MODE_FOCAL) return c.c_gt * focal_slope(ce, c.gamma);
    return ce > c.thr ? c.c_gt : (ce == c.thr ? c.c_eq : 0.f);
}

// Workgroup = LS_TILE x LS_TILE low-res taps of one image; it evaluates the (LS_TILE+1)^2 cells that touch them (halo cells are
// recomputed by the neighbouring workgroup), four parity colours so that no two cells in flight share a tap, plain stores.
// Its own copy of the walk that tile_cells_walk (loss_geom.h) holds: on the shared walk the <float, 3> instantiation changed output
// bits, and with make_cell / load_cell_taps / cell_max_bound in place of the clamps, loads and bound written out below the kernel
// was 2.4 % slower (profiles/loss_rows.md).  A change to the scatter or the store below belongs in tile_cells_walk too.
template <typename T, int NS>
__global__ void __launch_bounds__(LS_THREADS) pixel_loss_bwd_cells_kernel(const T* __restrict__ logits, LossGeom g, int sc,
                                                                           const int64_t* __restrict__ target, int64_t ignore_index,
                                                                           const float* __restrict__ cw, PixelParams pp,
                                                                           const float* __restrict__ ce_map, const int* __restrict__ state,
                                                                           const float* __restrict__ grad_out, T* __restrict__ dlow,
                                                                           int64_t ldd) {
    __shared__ float accum[LS_TILE * LS_TILE][64 * NS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int tiles_x = (g.w + LS_TILE - 1) / LS_TILE;
    const int ty0 = (blockIdx.x / tiles_x) * LS_TILE, tx0 = (blockIdx.x % tiles_x) * LS_TILE;
    const int halo = sc > 1 ? 1 : 0, off = sc >> 1;
    const float inv_sc = 1.f / (float)sc, fhalo = (float)halo;
    for (int i = threadIdx.x; i < LS_TILE * LS_TILE * 64 * NS; i += LS_THREADS) (&accum[0][0])[i] = 0.f;
    const PxCoef pc = px_coef_setup(state, pp, grad_out);
    const T* img = logits + (int64_t)b * g.h * g.w * g.ldl;
    const int64_t* tg = target + (int64_t)b * g.H * g.W;
    const float* cm = ce_map + (int64_t)b * g.H * g.W;
    __syncthreads();
    const int ncl = LS_TILE + halo;
    const int ncol = halo ? 4 : 1;
    for (int col = 0; col < ncol; ++col) {
        const int pj = col >> 1, pk = col & 1;
        const int nj = halo ? (ncl - pj + 1) / 2 : ncl, nk = halo ? (ncl - pk + 1) / 2 : ncl;
        for (int idx = wave; idx < nj * nk; idx += 4) {
            const int lj = halo ? 2 * (idx / nk) + pj : idx / nk, lk = halo ? 2 * (idx % nk) + pk : idx % nk;
            const int cj = ty0 - halo + lj, ck = tx0 - halo + lk;
            if (cj > g.h - 1 || ck > g.w - 1) continue;
            // this lane's pixel: label code (< 0: no gradient) and coefficient from the saved map
            int code = -1; float coef = 0.f;
            if (lane < sc * sc) {
                const int a = lane / sc;
                const int Y = sc * cj + off + a, X = sc * ck + off + (lane - a * sc);
                if (Y >= 0 && Y < g.H && X >= 0 && X < g.W) {
                    const int64_t t = tg[(int64_t)Y * g.W + X];
                    if (t != ignore_index && t >= 0 && t < g.C) {
                        code = (int)t;
                        coef = px_coef(pc, cm[(int64_t)Y * g.W + X]) * (cw ? cw[t] : 1.f);
                    }
                }
            }
            if (__ballot(coef != 0.f) == 0) continue;          // nothing selected in this cell: no softmax
            const int y0 = cj < 0 ? 0 : cj, y1 = cj + halo > g.h - 1 ? g.h - 1 : cj + halo;
            const int x0 = ck < 0 ? 0 : ck, x1 = ck + halo > g.w - 1 ? g.w - 1 : ck + halo;
            float t00[NS], t01[NS], t10[NS], t11[NS], A00[NS], A01[NS], A10[NS], A11[NS];
            load_tap<T, NS>(img + ((int64_t)y0 * g.w + x0) * g.ldl, lane, g.C, t00);
            load_tap<T, NS>(img + ((int64_t)y0 * g.w + x1) * g.ldl, lane, g.C, t01);
            load_tap<T, NS>(img + ((int64_t)y1 * g.w + x0) * g.ldl, lane, g.C, t10);
            load_tap<T, NS>(img + ((int64_t)y1 * g.w + x1) * g.ldl, lane, g.C, t11);
            float mb = -INFINITY;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                A00[s] = 0.f; A01[s] = 0.f; A10[s] = 0.f; A11[s] = 0.f;
                if (lane + 64 * s < g.C) mb = fmaxf(mb, fmaxf(fmaxf(t00[s], t01[s]), fmaxf(t10[s], t11[s])));
            }
            mb = wave_max_all(mb);
            for (int a = 0; a < sc; ++a) {
                const float ly = (a + 0.5f) * inv_sc * fhalo;
                float L[NS], R[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    L[s] = (1.f - ly) * t00[s] + ly * t10[s];
                    R[s] = (1.f - ly) * t01[s] + ly * t11[s];
                }
                for (int bb = 0; bb < sc; ++bb) {
                    const int t = __builtin_amdgcn_readlane(code, a * sc + bb);        // wave-uniform
                    const float cf = readlane_f(coef, a * sc + bb);
                    if (t < 0 || cf == 0.f) continue;
                    const float lx = (bb + 0.5f) * inv_sc * fhalo;
                    float z[NS], pr[NS], shift;
#pragma unroll
                    for (int s = 0; s < NS; ++s) z[s] = (lane + 64 * s) < g.C ? (1.f - lx) * L[s] + lx * R[s] : -INFINITY;
                    wave_softmax_bounded<NS>(z, mb, pr, shift);
                    const float w00 = (1.f - ly) * (1.f - lx), w01 = (1.f - ly) * lx, w10 = ly * (1.f - lx), w11 = ly * lx;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const float dz = cf * (pr[s] - (lane + 64 * s == t ? 1.f : 0.f));
                        A00[s] = fmaf(w00, dz, A00[s]); A01[s] = fmaf(w01, dz, A01[s]);
                        A10[s] = fmaf(w10, dz, A10[s]); A11[s] = fmaf(w11, dz, A11[s]);
                    }
                }
            }
            const int ly0 = y0 - ty0, ly1 = y1 - ty0, lx0 = x0 - tx0, lx1 = x1 - tx0;
            const bool vy0 = ly0 >= 0 && ly0 < LS_TILE, vy1 = ly1 >= 0 && ly1 < LS_TILE;
            const bool vx0 = lx0 >= 0 && lx0 < LS_TILE, vx1 = lx1 >= 0 && lx1 < LS_TILE;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int cc = lane + 64 * s;
                if (vy0 && vx0) accum[ly0 * LS_TILE + lx0][cc] += A00[s];
                if (vy0 && vx1) accum[ly0 * LS_TILE + lx1][cc] += A01[s];
                if (vy1 && vx0) accum[ly1 * LS_TILE + lx0][cc] += A10[s];
                if (vy1 && vx1) accum[ly1 * LS_TILE + lx1][cc] += A11[s];
            }
        }
        __syncthreads();
    }
    for (int tap = wave; tap < LS_TILE * LS_TILE; tap += 4) {
        const int y = ty0 + tap / LS_TILE, x = tx0 + tap % LS_TILE;
        if (y >= g.h || x >= g.w) continue;
        T* drow = dlow + (((int64_t)b * g.h + y) * g.w + x) * ldd;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int cc = lane + 64 * s;
            if (cc < ldd) stf<T>(drow + cc, cc < g.C ? accum[tap][cc] : 0.f);
        }
    }
}

// any ratio: the full-resolution gradient [B][H][W][ldg], one wave per pixel at a time
template <typename T, int NS>
__global__ void __launch_bounds__(LS_THREADS) pixel_loss_bwd_kernel(const T* __restrict__ logits, LossGeom g,
                                                                     const int64_t* __restrict__ target, int64_t ignore_index,
                                                                     const float* __restrict__ cw, PixelParams pp,
                                                                     const float* __restrict__ ce_map, const int* __restrict__ state,
                                                                     const float* __restrict__ grad_out, T* __restrict__ dfull,
                                                                     int64_t ldg) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    const PxCoef pc = px_coef_setup(state, pp, grad_out);
    const int64_t npix = (int64_t)g.H * g.W;
    int64_t p0, p1;
    wave_pixel_range(npix, p0, p1);
    const T* img = logits + (int64_t)b * g.h * g.w * g.ldl;
    const int64_t* tg = target + (int64_t)b * npix;
    const float* cm = ce_map + (int64_t)b * npix;
    T* dimg = dfull + (int64_t)b * npix * ldg;
    for (int64_t p = p0; p < p1; ++p) {
        const int64_t t = tg[p];
        T* drow = dimg + p * ldg;
        float dz[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) dz[s] = 0.f;
        if (t != ignore_index && t >= 0 && t < g.C) {
            const float cf = px_coef(pc, cm[p]) * (cw ? cw[t] : 1.f);
            if (cf != 0.f) {
                const int Y = (int)(p / g.W), X = (int)(p - (int64_t)Y * g.W);
                float z[NS], pr[NS];
                px_pixel_logits<T, NS>(img, g, Y, X, lane, z);
                float mx;
                wave_softmax<NS>(z, pr, mx);
#pragma unroll
                for (int s = 0; s < NS; ++s) dz[s] = cf * (pr[s] - (lane + 64 * s == (int)t ? 1.f : 0.f));
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int c = lane + 64 * s;
            if (c < ldg) stf<T>(drow + c, c < g.C ? dz[s] : 0.f);
        }
    }
}

__global__ void pixel_loss_zero_words_kernel(uint32_t* __restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0u;
}

template <typename T>
void px_fwd_launch(int ns, int sc, dim3 grid, hipStream_t st, const T* logits, LossGeom g, const int64_t* target, int64_t ignore_index,
                   const float* cw, PixelParams pp, float* ce_map, int* state, float* partial) {
#define CALL(NS)                                                                                                                 \
    do {                                                                                                                         \
        if (sc) hipLaunchKernelGGL((pixel_loss_fwd_cells_kernel<T, NS>), grid, dim3(LS_THREADS), 0, st, logits, g, sc, target,   \
                                   ignore_index, cw, pp, ce_map, state, partial);                                                \
        else hipLaunchKernelGGL((pixel_loss_fwd_kernel<T, NS>), grid, dim3(LS_THREADS), 0, st, logits, g, target, ignore_index,  \
                                cw, pp, ce_map, state, partial);                                                                 \
    } while (0)
    LS_NS_DISPATCH(ns, CALL);
#undef CALL
}
template <typename T>
void px_bwd_launch(int ns, int sc, dim3 grid, hipStream_t st, const T* logits, LossGeom g, const int64_t* target, int64_t ignore_index,
                   const float* cw, PixelParams pp, const float* ce_map, const int* state, const float* grad_out, T* dst, int64_t ld) {
#define CALL(NS)                                                                                                                 \
    do {                                                                                                                         \
        if (sc) hipLaunchKernelGGL((pixel_loss_bwd_cells_kernel<T, NS>), grid, dim3(LS_THREADS), 0, st, logits, g, sc, target,   \
                                   ignore_index, cw, pp, ce_map, state, grad_out, dst, ld);                                      \
        else hipLaunchKernelGGL((pixel_loss_bwd_kernel<T, NS>), grid, dim3(LS_THREADS), 0, st, logits, g, target, ignore_index,  \
                                cw, pp, ce_map, state, grad_out, dst, ld);                                                       \
    } while (0)
    LS_NS_DISPATCH(ns, CALL);
#undef CALL
}

bool px_params(int mode, float p0, float p1, int size_average, PixelParams& pp) {
    pp = PixelParams{mode, p0, p1, size_average};
    if (mode == PX_MODE_OHEM) return p0 > 0.f && p0 < INFINITY;        // theta = -log(thresh), 0 < thresh < 1
    if (mode == PX_MODE_FOCAL) return p1 >= 0.f && p1 < INFINITY && p0 == p0;
    return false;
}

}  // namespace

extern "C" int segf_pixel_loss_supported(int dt, int mode, int B, int C, int h, int w, int H, int W) {
    if (dt != SEGF_F32 && dt != SEGF_BF16) return 0;
    if (mode != PX_MODE_OHEM && mode != PX_MODE_FOCAL) return 0;
    if (B <= 0 || B > 65535 || C <= 0 || C > 192 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
    if ((int64_t)B * H * W >= ((int64_t)1 << 31) || (int64_t)B * h * w >= ((int64_t)1 << 31)) return 0;
    return 1;
}

extern "C" int64_t segf_pixel_loss_state_words(int B) {
    if (B <= 0 || B > 65535) return 0;
    return PXS_HEAD + PXS_HIST + (int64_t)LS_NBLK * B + PX_RBLK;
}

extern "C" int64_t segf_pixel_loss_bwd_ws(int dt, int B, int C, int h, int w, int H, int W) {
    if (!segf_pixel_loss_supported(dt, PX_MODE_OHEM, B, C, h, w, H, W) || pow2_scale(h, w, H, W)) return 0;
    const int64_t ldg = (C + 7) / 8 * 8;
    const int64_t bytes = (int64_t)B * H * W * ldg * (dt == SEGF_BF16 ? 2 : 4);
    return (bytes + 3) / 4;
}

extern "C" int segf_pixel_loss_fwd(int dt, int mode, int B, int C, int h, int w, int H, int W, const void* logits, int64_t ldl,
                                   const int64_t* target, int64_t ignore_index, const float* class_weight, float p0, float p1,
                                   int size_average, float* ce_map, int32_t* state, float* loss, void* stream) {
    PixelParams pp;
    if (!segf_pixel_loss_supported(dt, mode, B, C, h, w, H, W) || ldl < C || !px_params(mode, p0, p1, size_average, pp))
        return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    LossGeom g{B, C, h, w, H, W, ldl};
    const int ns = (C + 63) / 64;
    const int sc = pow2_scale(h, w, H, W);
    const int64_t npix = (int64_t)B * H * W;
    float* partial = reinterpret_cast<float*>(state) + PXS_HEAD + PXS_HIST;
    float* rpartial = partial + (int64_t)LS_NBLK * B;
    // kernel nodes rather than hipMemsetAsync, as everywhere on the loss path (see segf_ce_dice_fwd)
    hipLaunchKernelGGL(pixel_loss_zero_state_kernel, dim3(1), dim3(256), 0, st, state);
    SEGF_CHECK_LAUNCH();
    SEGF_DISPATCH_DT(dt, T, { px_fwd_launch<T>(ns, sc, dim3(LS_NBLK, B), st, (const T*)logits, g, target, ignore_index, class_weight, pp, ce_map, state, partial); })
    SEGF_CHECK_LAUNCH();
    hipLaunchKernelGGL(pixel_loss_finalize_kernel, dim3(1), dim3(256), 0, st, state, partial, LS_NBLK * B, pp, npix, loss);
    SEGF_CHECK_LAUNCH();
    if (mode != PX_MODE_OHEM) return 0;
    const int mblk = (int)imin64(cdiv64(npix, 256 * 8), PX_RBLK);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(pixel_loss_select_hist_kernel, dim3(mblk), dim3(256), 0, st, (const uint32_t*)ce_map, npix, pass, state);
        hipLaunchKernelGGL(pixel_loss_select_pick_kernel, dim3(1), dim3(64), 0, st, pass, state);
        SEGF_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pixel_loss_topk_sum_kernel, dim3(mblk), dim3(256), 0, st, ce_map, npix, state, rpartial);
    hipLaunchKernelGGL(pixel_loss_topk_final_kernel, dim3(1), dim3(256), 0, st, state, rpartial, mblk, loss);
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int segf_bilinear_bwd(int dt, int B, int h, int w, int C, void* din, int64_t ldi, int H, int W, const void* dout,
                                 int64_t ldo, int align_corners, void* stream);

extern "C" int segf_pixel_loss_bwd(int dt, int mode, int B, int C, int h, int w, int H, int W, const void* logits, int64_t ldl,
                                   const int64_t* target, int64_t ignore_index, const float* class_weight, float p0, float p1,
                                   int size_average, const float* ce_map, const int32_t* state, const float* grad_out, void* dlogits,
                                   int64_t ldd, float* ws, void* stream) {
    PixelParams pp;
    if (!segf_pixel_loss_supported(dt, mode, B, C, h, w, H, W) || ldl < C || ldd < C || !px_params(mode, p0, p1, size_average, pp))
        return SEGF_ERR_SHAPE;
    if (ldd > 64 * ((C + 63) / 64)) return SEGF_ERR_SHAPE;        // pad columns are zero-filled by the class lanes
    hipStream_t st = (hipStream_t)stream;
    LossGeom g{B, C, h, w, H, W, ldl};
    const int ns = (C + 63) / 64;
    const int sc = pow2_scale(h, w, H, W);
    if (sc) {
        const dim3 grid(((h + LS_TILE - 1) / LS_TILE) * ((w + LS_TILE - 1) / LS_TILE), B);
        SEGF_DISPATCH_DT(dt, T, { px_bwd_launch<T>(ns, sc, grid, st, (const T*)logits, g, target, ignore_index, class_weight, pp, ce_map, state, grad_out, (T*)dlogits, ldd); })
        SEGF_CHECK_LAUNCH();
        return 0;
    }
    if (!ws) return SEGF_ERR_WORKSPACE;
    const int64_t ldg = (C + 7) / 8 * 8;
    SEGF_DISPATCH_DT(dt, T, { px_bwd_launch<T>(ns, 0, dim3(LS_NBLK, B), st, (const T*)logits, g, target, ignore_index, class_weight, pp, ce_map, state, grad_out, (T*)ws, ldg); })
    SEGF_CHECK_LAUNCH();
    if (ldd > C) {
        const int64_t nwords = ((int64_t)B * h * w * ldd * (dt == SEGF_BF16 ? 2 : 4) + 3) / 4;
        hipLaunchKernelGGL(pixel_loss_zero_words_kernel, dim3((unsigned)imin64(cdiv64(nwords, 256), 4096)), dim3(256), 0, st, (uint32_t*)dlogits, nwords);
        SEGF_CHECK_LAUNCH();
    }
    return segf_bilinear_bwd(dt, B, h, w, C, dlogits, ldd, H, W, ws, ldg, 0, stream);
}
