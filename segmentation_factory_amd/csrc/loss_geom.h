// Shared by loss.hip, loss_pixel.hip and loss_band.hip: geometry of the fused upsample + loss / arg max kernels, what a wave does
// with a class row (classes on the 64 lanes, NS <= 3 slots per lane: tap loads, per-pixel bilinear row, wave softmax, the cell's
// taps / bound / label codes, Dice coefficients) and the tile / parity-colour walk of the low-resolution gradient.  A new loss or
// evaluation mode starts from these.  Everything is inline: every .hip file compiles it under its own flags.  loss_band.hip takes
// only the geometry, the 16-lane helpers and dice_coef_one.  wave_pixel_range and eval_count come from eval_rows.h.
#pragma once
#include "eval_rows.h"

#define LS_NBLK 128         // workgroups per image in the forward / eval kernels
#define LS_THREADS 256
#define LS_EPS 1e-6f
#define LS_TILE 8           // backward (tile kernels): low-res taps per workgroup tile edge
#define LS_LOG2E 1.4426950408889634f
#define LS_LN2 0.6931471805599453f

#define LS_NS_DISPATCH(ns, CALL) do { if ((ns) == 1) { CALL(1); } else if ((ns) == 2) { CALL(2); } else { CALL(3); } } while (0)

struct LossGeom { int B, C, h, w, H, W; int64_t ldl; };

typedef float lossf4 __attribute__((ext_vector_type(4)));
typedef __bf16 lossbf8 __attribute__((ext_vector_type(8)));

static inline int pow2_scale(int h, int w, int H, int W) {
    // sc >= 1 when H == sc*h, W == sc*w and sc is a power of two (exact source-index arithmetic); else 0
    if (h <= 0 || w <= 0 || H % h || W % w) return 0;
    const int sc = H / h;
    if (W / w != sc || (sc & (sc - 1)) || sc > 8) return 0;   // sc*sc labels live one per lane
    return sc;
}

__device__ __forceinline__ float tap_weight(int k, float ly, float lx) {      // k = 2 * (row tap) + (column tap)
    return ((k >> 1) ? ly : 1.f - ly) * ((k & 1) ? lx : 1.f - lx);
}
__device__ __forceinline__ float row_sum16(float v) {
    v += dpp_mov<DPP_XOR1>(v); v += dpp_mov<DPP_XOR2>(v); v += dpp_mov<DPP_HALF_MIRROR>(v); v += dpp_mov<DPP_MIRROR>(v);
    return v;
}
__device__ __forceinline__ float sel4(const float (&v)[4], int r) {
    return r == 0 ? v[0] : (r == 1 ? v[1] : (r == 2 ? v[2] : v[3]));
}

// ---- per-lane class rows -------------------------------------------------------------------------------------
template <typename T, int NS>
__device__ __forceinline__ void load_tap(const T* __restrict__ p, int lane, int C, float (&t)[NS]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {     // unconditional loads from a clamped index: all taps of a cell stay in flight together
        const int c = lane + 64 * s;
        const float v = ldf<T>(p + (c < C ? c : C - 1));
        t[s] = c < C ? v : 0.f;
    }
}

// z[s] = upsampled logit of class lane + 64*s at full-res pixel (Y, X); invalid class slots get -inf  (generic path)
template <typename T, int NS, bool ATEN = false>
__device__ __forceinline__ void pixel_logits(const T* __restrict__ img, const LossGeom& g, int Y, int X, int lane, float (&z)[NS]) {
    if (g.h == g.H && g.w == g.W) {
        const T* p = img + ((int64_t)Y * g.w + X) * g.ldl;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int c = lane + 64 * s;
            const float v = ldf<T>(p + (c < g.C ? c : g.C - 1));
            z[s] = c < g.C ? v : -INFINITY;
        }
        return;
    }
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
        // ATEN (evaluation kernels): the operation order of the reference's CPU F.interpolate, so that arg max ties resolve alike
        const float v = ATEN ? bilinear_aten(a, b, cc, d, ly, lx) : (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * cc + lx * d);
        z[s] = c < g.C ? v : -INFINITY;
    }
}

// softmax over the wave with the exact maximum: p[s] and mx; returns log(sum exp(z - mx)) (all wave-uniform).  The log-sum-exp is
// mx + the result.  The per-pixel losses form ce = log(sum) - (z_t - mx) instead: at a confident pixel (z_t == mx, sum = 1 + eps)
// nothing of the size of the logits enters, so a ce of 1e-5 keeps an absolute error of the roundings of the sum (~1e-7) instead of
// that of mx + log(sum) (half an ulp of the logit)
template <int NS>
__device__ __forceinline__ float wave_softmax(const float (&z)[NS], float (&p)[NS], float& mx_out) {
    float mx = z[0];
#pragma unroll
    for (int s = 1; s < NS; ++s) mx = fmaxf(mx, z[s]);
    mx = wave_max_all(mx);
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) { p[s] = __expf(z[s] - mx); sum += p[s]; }
    sum = wave_sum_all(sum);
    const float inv = 1.f / sum;
#pragma unroll
    for (int s = 0; s < NS; ++s) p[s] *= inv;
    mx_out = mx;
    return __logf(sum);
}
// z_t for a wave-uniform label t: class c lives in lane c % 64, slot c / 64
template <int NS>
__device__ __forceinline__ float px_label_logit(const float (&z)[NS], int t) {
    float v = z[0];
#pragma unroll
    for (int s = 1; s < NS; ++s) v = (t >> 6) == s ? z[s] : v;
    return readlane_f(v, t & 63);
}

// softmax with a wave-uniform upper bound `mb` of max(z) in place of the exact maximum (every pixel of a cell is a convex
// combination of the cell's four taps, so the taps' maximum bounds all of them: one wave reduction per CELL instead of
// one per pixel).  Mathematically identical (softmax is shift invariant); if the bound is so loose that the sum
// underflows, the exact-maximum path is taken instead (wave-uniform branch, practically never).  Returns log(sum) of the
// shift it used, `shift` (mb, or the exact maximum): the log-sum-exp is shift + the result.
template <int NS>
__device__ __forceinline__ float wave_softmax_bounded(const float (&z)[NS], float mb, float (&p)[NS], float& shift) {
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) { p[s] = __expf(z[s] - mb); sum += p[s]; }
    sum = wave_sum_all(sum);
    if (!(sum > 1e-30f)) return wave_softmax<NS>(z, p, shift);
    const float inv = 1.f / sum;
#pragma unroll
    for (int s = 0; s < NS; ++s) p[s] *= inv;
    shift = mb;
    return __logf(sum);
}
template <int NS>
__device__ __forceinline__ float cell_max_bound(const float (&t00)[NS], const float (&t01)[NS], const float (&t10)[NS],
                                                const float (&t11)[NS], int lane, int C) {
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < NS; ++s)
        if (lane + 64 * s < C) mx = fmaxf(mx, fmaxf(fmaxf(t00[s], t01[s]), fmaxf(t10[s], t11[s])));
    return wave_max_all(mx);
}

// A cell = the sc x sc full-res pixels between low-res taps (cj, ck) .. (cj+1, ck+1); cj in [-1, h-1] (taps clamp).
struct Cell { int cj, ck, y0, y1, x0, x1; };
__device__ __forceinline__ Cell make_cell(int cj, int ck, int h, int w, int halo) {
    // halo == 0 (sc == 1, no resize): the cell is the pixel itself, all four taps coincide
    Cell c; c.cj = cj; c.ck = ck;
    c.y0 = cj < 0 ? 0 : cj; c.y1 = cj + halo > h - 1 ? h - 1 : cj + halo;
    c.x0 = ck < 0 ? 0 : ck; c.x1 = ck + halo > w - 1 ? w - 1 : ck + halo;
    return c;
}
template <typename T, int NS>
__device__ __forceinline__ void load_cell_taps(const T* __restrict__ img, const LossGeom& g, const Cell& c, int lane,
                                               float (&t00)[NS], float (&t01)[NS], float (&t10)[NS], float (&t11)[NS]) {
    load_tap<T, NS>(img + ((int64_t)c.y0 * g.w + c.x0) * g.ldl, lane, g.C, t00);
    load_tap<T, NS>(img + ((int64_t)c.y0 * g.w + c.x1) * g.ldl, lane, g.C, t01);
    load_tap<T, NS>(img + ((int64_t)c.y1 * g.w + c.x0) * g.ldl, lane, g.C, t10);
    load_tap<T, NS>(img + ((int64_t)c.y1 * g.w + c.x1) * g.ldl, lane, g.C, t11);
}
// fractional weight of pixel coordinate d inside its cell (exact for power-of-two sc; matches bilinear_src)
__device__ __forceinline__ float cell_frac(int d, int in, int out) {
    int i0, i1; float l;
    bilinear_src(d, in, out, 0, i0, i1, l);
    return l;
}

// Labels of the cell's sc x sc pixels, one per lane (lane = a * sc + bb), fetched with a single vector load:
// code = class index, or -1 (skip: outside the image or equal to `skip_label`), or -2 (out-of-range label).
__device__ __forceinline__ int cell_label_codes(const int64_t* __restrict__ tg, const LossGeom& g, int sc, int off, int cj, int ck,
                                                int lane, int64_t skip_label, int64_t* raw = nullptr) {
    int code = -1;
    if (lane < sc * sc) {
        const int a = lane / sc, bb = lane - a * sc;
        const int Y = sc * cj + off + a, X = sc * ck + off + bb;
        if (Y >= 0 && Y < g.H && X >= 0 && X < g.W) {
            const int64_t t = tg[(int64_t)Y * g.W + X];
            if (raw) *raw = t;
            code = t == skip_label ? -1 : ((t < 0 || t >= g.C) ? -2 : (int)t);
        }
    }
    return code;
}

// ---- Dice gradient ---------------------------------------------------------------------------------------------
// d loss / d I and d loss / d P of the Dice term for one class
__device__ __forceinline__ void dice_coef_one(const float* __restrict__ stats, int b, int B, int C, int dice, int cls, float& gI, float& gP) {
    gI = 0.f; gP = 0.f;
    if (cls < C && dice) {
        const float* st = stats + (int64_t)b * (3 * C + 4);
        const float I = st[cls], P = st[C + cls], Tt = st[2 * C + cls];
        const float sets = P + Tt;
        if (sets != 0.f) {   // sets == 0: d = (2I+eps)/(2I+eps) == 1 -> zero gradient
            const float nbc = 1.f / (float)(B * C);
            gI = -nbc * 2.f / (sets + LS_EPS);
            gP = nbc * (2.f * I + LS_EPS) / ((sets + LS_EPS) * (sets + LS_EPS));
        }
    }
}
// ... for this lane's classes.  The same expressions as dice_coef_one, in a loop of its own: written as calls of dice_coef_one, the
// compiler packs pixel_grad's three class slots differently in ce_dice_bwd_kernel<T, 2 / 3> (another fused multiply-add) and the
// gradient bits of the generic path change (profiles/loss_rows.md)
template <int NS>
__device__ __forceinline__ void dice_coefs(const float* __restrict__ stats, int b, int B, int C, int dice, int lane,
                                           float (&gI)[NS], float (&gP)[NS]) {
    const float* st = stats + (int64_t)b * (3 * C + 4);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = lane + 64 * s;
        float a = 0.f, bb = 0.f;
        if (c < C && dice) {
            const float I = st[c], P = st[C + c], Tt = st[2 * C + c];
            const float sets = P + Tt;
            if (sets != 0.f) {
                const float nbc = 1.f / (float)(B * C);
                a = -nbc * 2.f / (sets + LS_EPS);
                bb = nbc * (2.f * I + LS_EPS) / ((sets + LS_EPS) * (sets + LS_EPS));
            }
        }
        gI[s] = a; gP[s] = bb;
    }
}

// ---- backward: the tile / parity-colour walk ---------------------------------------------------------------------
// Workgroup = LS_TILE x LS_TILE low-res taps of one image (blockIdx.x = tile, blockIdx.y = image, LS_THREADS threads); it evaluates
// the (LS_TILE+1)^2 cells that touch them (halo cells are recomputed by the neighbouring workgroup) in four parity colours, so that
// no two cells in flight share a tap: plain LDS adds, no atomics, bitwise reproducible.  Ratios 2 / 4 / 8 (a halo of one cell).
//   cell(cj, ck, c, A00, A01, A10, A11) -> bool     one wave per call, every lane active; A** arrive zeroed and receive this lane's
//                                                   classes of d loss / d tap (y0,x0), (y0,x1), (y1,x0), (y1,x1) of the cell c;
//                                                   false: the cell contributes nothing.
// The walk owns the LDS tile, the cell order, the in-tile scatter, the barriers and the store of dlow[b][y][x][0 .. ldd) with
// zeroed pad columns; a kernel does its per-image set-up and passes what differs as `cell`.  Today ce_dice_bwd_cells8_kernel is its
// only user: ce_dice_bwd_cells_kernel (loss.hip) and pixel_loss_bwd_cells_kernel (loss_pixel.hip) keep copies of this walk, because on
// it their <float, 3> instantiations changed output bits (profiles/loss_rows.md) -- a fix here has to be repeated there.
template <typename T, int NS, typename F>
__device__ __forceinline__ void tile_cells_walk(const LossGeom& g, T* __restrict__ dlow, int64_t ldd, F&& cell) {
    __shared__ float accum[LS_TILE * LS_TILE][64 * NS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int tiles_x = (g.w + LS_TILE - 1) / LS_TILE;
    const int ty0 = (blockIdx.x / tiles_x) * LS_TILE, tx0 = (blockIdx.x % tiles_x) * LS_TILE;
    for (int i = threadIdx.x; i < LS_TILE * LS_TILE * 64 * NS; i += LS_THREADS) (&accum[0][0])[i] = 0.f;
    __syncthreads();
    constexpr int ncl = LS_TILE + 1;           // local cells per edge: lj in [0, ncl), cj = ty0 - 1 + lj
    for (int col = 0; col < 4; ++col) {        // parity colours (no two cells of one colour share a tap)
        const int pj = col >> 1, pk = col & 1;
        const int nj = (ncl - pj + 1) / 2, nk = (ncl - pk + 1) / 2;
        for (int idx = wave; idx < nj * nk; idx += 4) {
            const int lj = 2 * (idx / nk) + pj, lk = 2 * (idx % nk) + pk;
            const int cj = ty0 - 1 + lj, ck = tx0 - 1 + lk;
            if (cj > g.h - 1 || ck > g.w - 1) continue;
            const Cell c = make_cell(cj, ck, g.h, g.w, 1);
            float A00[NS], A01[NS], A10[NS], A11[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) { A00[s] = 0.f; A01[s] = 0.f; A10[s] = 0.f; A11[s] = 0.f; }
            if (!cell(cj, ck, c, A00, A01, A10, A11)) continue;
            // taps of this cell that belong to the tile (the others are recomputed by the neighbouring workgroups)
            const int ly0 = c.y0 - ty0, ly1 = c.y1 - ty0, lx0 = c.x0 - tx0, lx1 = c.x1 - tx0;
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

// loss_band.hip: band-sweep backward for ratio 4 / bf16; returns false when the configuration is not covered
// lse (nullable): per (image, cell, pixel) -log2(sum exp), written by the forward and consumed by the backward (LSE variant)
bool loss_band_fwd_covers(const bf16_t* logits, LossGeom g);
bool loss_band_bwd_launch(const bf16_t* logits, LossGeom g, const int64_t* target, int64_t ignore_index, const float* cw, int dice,
                          const float* stats, const float* grad_out, bf16_t* dlow, int64_t ldd, int* retry, const float* lse,
                          hipStream_t st);
bool loss_band_fwd_launch(const bf16_t* logits, LossGeom g, const int64_t* target, int64_t ignore_index, const float* cw,
                          float* partial, int* retry, float* lse, hipStream_t st);
