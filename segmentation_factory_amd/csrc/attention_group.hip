// CrossFormer group attention (models/backbones/crossformer.py:112-167, 258-339): softmax attention inside groups of G x G tokens,
//
//     O_g = softmax(scale * Q_g K_g^T + bias[head] + keymask_g) V_g,
//
// reading q / k / v straight out of the [B H W, 3 C] output of the qkv Linear (head h of q at columns 32 h, of k at C + 32 h, of v at
// 2 C + 32 h) and writing O straight into a [B H W, C] token tensor.  Head dim 32, N = G G <= 64 tokens per group.
//
// The group-to-token map is arithmetic on (H, W, G, I): slot (gi, gj) of group (rh, rw, ih, iw) is the token at padded coordinates
//     r = (rh G + gi) I + ih,   c = (rw G + gj) I + iw            (I = 1 in SDA mode: adjacent tokens; I = the interval in LDA mode),
// which is the reference's pad / reshape / permute sequence (:286-313) read backwards.  No permuted, padded or gathered copy of the map
// exists.  A token with r >= H or c >= W is padding: as a key it is skipped (the reference adds -1000000 to its score, whose exp is exactly
// 0 in fp32), as a query it is not computed (the reference crops it away, :337-338).  The reference pads AFTER norm1, so its padded tokens
// carry q = k = v = the qkv bias; being masked keys and cropped queries, that value reaches no real output and no gradient, and nothing
// is lost by never forming it.  Groups with no real token are not launched: along each axis the non-empty (region, phase) pairs are the
// first nh (nw) of them.
//
// One workgroup of four waves per (group, head): q, k, v of the group go to LDS once (zeros in the padding slots); wave w owns query rows
// 16 w .. 16 w + 15 through scores, softmax (fp32, in the accumulator registers) and P V.  Both products run on the matrix pipe:
// v_mfma_f32_16x16x32_bf16 for bf16 storage, the f32-input v_mfma_f32_16x16x4_f32 (an exact fp32 fma chain) for fp32 storage.
// Backward: one workgroup walks a contiguous range of groups of one head, recomputes P from the saved log-sum-exp, forms dV = P^T dO,
// dS = P (dP - rowsum(P dP)), dQ = scale dS K, dK = scale dS^T Q and stores them through the same map (every real token is in exactly one
// group: plain stores), and keeps the running sum of dS -- the bias gradient -- in registers.  The per-workgroup sums go to the caller's
// workspace and a second kernel adds them in a fixed order: no floating-point atomics, two runs give the same bits.
//
// Roofline: per (group, head) 3 N 32 elements in and N 32 out (+ N lse) against 2 * 2 N N 32 flops forward: 49 tokens in bf16 are 12.5 KB
// and 0.61 Mflop, i.e. 49 flop / byte against the chip's ~300 flop / byte (2.5 Pflop/s over 8 TB/s): memory-bound by 6 x, and the bound is
// the qkv read + o write, (3 + 1) B H W C elements (backward: (3 + 1) read, 3 written).
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 ga_bf16x8;
typedef __attribute__((ext_vector_type(4))) float ga_f32x4;

constexpr int GA_HD = 32;          // head dim
constexpr int GA_NMAX = 64;        // slots per group the tile holds
constexpr int GA_THREADS = 256;
constexpr int GA_BWD_BLOCKS = 2048;   // backward: target number of workgroups (each one writes an N x N slab of bias-gradient partial sums)

// LDS row lengths in elements for 32- and 64-element rows: 16-byte accesses stay aligned, rows spread over the banks
template <typename T> struct GaLd;
template <> struct GaLd<bf16_t> { static constexpr int d = 40, n = 72; };
template <> struct GaLd<float> { static constexpr int d = 36, n = 68; };

struct GaGeom {
    int B, H, W, heads, G, I, N;
    int nh, nw;                    // non-empty (region, phase) pairs along rows / columns
    int items;                     // B nh nw groups that hold a real token
    int rows;                      // B H W
};

// validity + geometry on the host; false = SEGF_ERR_SHAPE
static bool ga_geom(int B, int H, int W, int heads, int hd, int G, int interval, int lda, GaGeom& g) {
    if (B <= 0 || H <= 0 || W <= 0 || heads <= 0 || G <= 0 || hd != GA_HD) return false;
    if ((int64_t)G * G > GA_NMAX) return false;
    const int I = lda ? interval : 1;
    if (I <= 0) return false;
    const int64_t rows = (int64_t)B * H * W;
    if (rows >= (1ll << 31) / 4) return false;
    const int64_t div = (int64_t)G * I;
    const int Rh = (int)((H + div - 1) / div), Rw = (int)((W + div - 1) / div);
    // region rh < Rh - 1 is whole: all I phases hold real rows; the last one has the phases ih with (Rh - 1) G I + ih < H
    const int64_t nh = (int64_t)(Rh - 1) * I + imin64(I, H - (int64_t)(Rh - 1) * div);
    const int64_t nw = (int64_t)(Rw - 1) * I + imin64(I, W - (int64_t)(Rw - 1) * div);
    const int64_t items = (int64_t)B * nh * nw;
    if (items * heads >= (1ll << 31)) return false;
    g.B = B; g.H = H; g.W = W; g.heads = heads; g.G = G; g.I = I; g.N = G * G;
    g.nh = (int)nh; g.nw = (int)nw; g.items = (int)items; g.rows = (int)rows;
    return true;
}

// groups per backward workgroup
static int ga_items_per_block(const GaGeom& g) {
    const int chunks = GA_BWD_BLOCKS / g.heads > 0 ? GA_BWD_BLOCKS / g.heads : 1;
    return (g.items + chunks - 1) / chunks;
}
static int ga_chunks(const GaGeom& g) {
    const int ipb = ga_items_per_block(g);
    return (g.items + ipb - 1) / ipb;
}

// row index of slot n of group `it` in the [B H W] token tensors, or -1 for padding
__device__ __forceinline__ int ga_token(const GaGeom& g, int it, int n) {
    if (n >= g.N) return -1;
    const int v = it % g.nw, u = (it / g.nw) % g.nh, b = it / (g.nw * g.nh);
    const int gi = n / g.G, gj = n - gi * g.G;
    const int r = ((u / g.I) * g.G + gi) * g.I + u % g.I;
    const int c = ((v / g.I) * g.G + gj) * g.I + v % g.I;
    if (r >= g.H || c >= g.W) return -1;
    return (b * g.H + r) * g.W + c;
}

template <typename T> __device__ __forceinline__ Raw8<T> ga_zero();
template <> __device__ __forceinline__ Raw8<bf16_t> ga_zero<bf16_t>() { Raw8<bf16_t> r; r.u = make_uint4(0u, 0u, 0u, 0u); return r; }
template <> __device__ __forceinline__ Raw8<float> ga_zero<float>() {
    Raw8<float> r; r.a = make_float4(0.f, 0.f, 0.f, 0.f); r.b = r.a; return r;
}
__device__ __forceinline__ void ga_st_row(bf16_t* s, const Raw8<bf16_t>& r) { *reinterpret_cast<uint4*>(s) = r.u; }
__device__ __forceinline__ void ga_st_row(float* s, const Raw8<float>& r) {
    *reinterpret_cast<float4*>(s) = r.a; *reinterpret_cast<float4*>(s + 4) = r.b;
}
template <int LD> __device__ __forceinline__ void ga_st_col(bf16_t* s, const Raw8<bf16_t>& r) {
    s[0 * LD] = (bf16_t)(r.u.x & 0xffffu); s[1 * LD] = (bf16_t)(r.u.x >> 16);
    s[2 * LD] = (bf16_t)(r.u.y & 0xffffu); s[3 * LD] = (bf16_t)(r.u.y >> 16);
    s[4 * LD] = (bf16_t)(r.u.z & 0xffffu); s[5 * LD] = (bf16_t)(r.u.z >> 16);
    s[6 * LD] = (bf16_t)(r.u.w & 0xffffu); s[7 * LD] = (bf16_t)(r.u.w >> 16);
}
template <int LD> __device__ __forceinline__ void ga_st_col(float* s, const Raw8<float>& r) {
    s[0 * LD] = r.a.x; s[1 * LD] = r.a.y; s[2 * LD] = r.a.z; s[3 * LD] = r.a.w;
    s[4 * LD] = r.b.x; s[5 * LD] = r.b.y; s[6 * LD] = r.b.z; s[7 * LD] = r.b.w;
}

// One [64 slots][32] operand of the group from global memory into LDS: thread t brings 8 elements of slot t / 4 (zeros for padding slots);
// row-major [slot][d] (ROW) and / or transposed [d][slot] (TR).  src points at column 0 of the head.
template <typename T, bool ROW, bool TR>
__device__ __forceinline__ void ga_stage(const T* __restrict__ src, int64_t ld, const int* s_tok, T* rowm, T* trm, int tid) {
    constexpr int LDD = GaLd<T>::d, LDN = GaLd<T>::n;
    const int n = tid >> 2, c8 = (tid & 3) * 8;
    const int tok = s_tok[n];
    const Raw8<T> r = tok >= 0 ? load8_raw<T>(src + (int64_t)tok * ld + c8) : ga_zero<T>();
    if (ROW) ga_st_row(rowm + n * LDD + c8, r);
    if (TR) ga_st_col<LDN>(trm + c8 * LDN + n, r);
}

// The way back: a [64 slots][32] result tile in LDS (row-major) to the token rows of global memory, 16 bytes per thread and store
// (the accumulator layout itself would give 2-byte stores, 16 lanes to a 32-byte run); padding slots store nothing.
template <typename T>
__device__ __forceinline__ void ga_unstage(const T* rowm, const int* s_tok, T* __restrict__ dst, int64_t ld, int tid) {
    constexpr int LDD = GaLd<T>::d;
    const int n = tid >> 2, c8 = (tid & 3) * 8;
    const int tok = s_tok[n];
    if (tok < 0) return;
    const T* src = rowm + n * LDD + c8;
    T* out = dst + (int64_t)tok * ld + c8;
    if constexpr (sizeof(T) == 2) {
        *reinterpret_cast<uint4*>(out) = *reinterpret_cast<const uint4*>(src);
    } else {
        *reinterpret_cast<float4*>(out) = *reinterpret_cast<const float4*>(src);
        *reinterpret_cast<float4*>(out + 4) = *reinterpret_cast<const float4*>(src + 4);
    }
}

// acc[16 x 16] += A[16 x K] Bt[16 x K]^T: a, b point at row 0 of two 16-row tiles whose rows run along the reduction index.
// Result element e of a lane: row 4 (lane >> 4) + e of A's tile, row (lane & 15) of Bt's tile.
template <typename T, int K>
__device__ __forceinline__ ga_f32x4 ga_mma(const T* a, int lda, const T* b, int ldb, ga_f32x4 acc, int lane) {
    const int r = lane & 15, q = lane >> 4;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int s = 0; s < K / 32; ++s) {
            const ga_bf16x8 fa = *reinterpret_cast<const ga_bf16x8*>(a + r * lda + 32 * s + 8 * q);
            const ga_bf16x8 fb = *reinterpret_cast<const ga_bf16x8*>(b + r * ldb + 32 * s + 8 * q);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc, 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int s = 0; s < K / 4; ++s) {
            const float fa = a[r * lda + 4 * s + q];
            const float fb = b[r * ldb + 4 * s + q];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa, fb, acc, 0, 0, 0);
        }
    }
    return acc;
}

// ---- forward: grid (items * heads), head fastest ---------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(GA_THREADS) group_attn_fwd_kernel(const T* __restrict__ qkv, int64_t ldq, const float* __restrict__ bias,
                                                                    T* __restrict__ o, int64_t ldo, float* __restrict__ lse,
                                                                    const GaGeom g, float scale) {
    constexpr int LDD = GaLd<T>::d, LDN = GaLd<T>::n;
    __shared__ __attribute__((aligned(16))) T sQ[GA_NMAX * LDD];
    __shared__ __attribute__((aligned(16))) T sK[GA_NMAX * LDD];
    __shared__ __attribute__((aligned(16))) T sVt[GA_HD * LDN];
    __shared__ __attribute__((aligned(16))) T sP[GA_NMAX * LDN];
    __shared__ int s_tok[GA_NMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x % g.heads, it = blockIdx.x / g.heads;
    const int C = g.heads * GA_HD, N = g.N;
    const int r = lane & 15, q4 = lane >> 4;
    const int i0 = 16 * wave + 4 * q4;          // first of this lane's four query rows
    // this lane's 16 bias values (rows i0 .. i0 + 3, columns 16 t + r), requested before the tiles so that the two latencies overlap
    float bv[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[t][e] = (i0 + e < N && 16 * t + r < N) ? bias[((int64_t)h * N + i0 + e) * N + 16 * t + r] : 0.f;
    }
    if (tid < GA_NMAX) s_tok[tid] = ga_token(g, it, tid);
    __syncthreads();
    ga_stage<T, true, false>(qkv + h * GA_HD, ldq, s_tok, sQ, nullptr, tid);
    ga_stage<T, true, false>(qkv + C + h * GA_HD, ldq, s_tok, sK, nullptr, tid);
    ga_stage<T, false, true>(qkv + 2 * C + h * GA_HD, ldq, s_tok, nullptr, sVt, tid);
    __syncthreads();
    const bool act = 16 * wave < N;             // (wave-uniform) this wave's rows hold slots of the group
    float lg[4];
    if (act) {
        ga_f32x4 s[4];
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = ga_mma<T, GA_HD>(sQ + 16 * wave * LDD, LDD, sK + 16 * t * LDD, LDD, ga_f32x4{0.f, 0.f, 0.f, 0.f}, lane);
            const bool key = s_tok[16 * t + r] >= 0;         // padding slots and slots >= N: skipped keys
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s[t][e] = key ? fmaf(s[t][e], scale, bv[t][e]) : -INFINITY;
                m[e] = fmaxf(m[e], s[t][e]);
            }
        }
        // a row's 64 scores lie on the 16 lanes that share lane >> 4, four per lane; every launched group has a real key, so m is finite
        float sum[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m[e] = wave_max(m[e], 16);
            float a = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) { s[t][e] = __expf(s[t][e] - m[e]); a += s[t][e]; }
            sum[e] = wave_sum(a, 16);
            lg[e] = m[e] + __logf(sum[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float inv = 1.f / sum[e];
#pragma unroll
            for (int t = 0; t < 4; ++t) stf<T>(sP + (i0 + e) * LDN + 16 * t + r, s[t][e] * inv);
        }
    }
    __syncthreads();
    if (act) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const ga_f32x4 acc = ga_mma<T, GA_NMAX>(sP + 16 * wave * LDN, LDN, sVt + 16 * t * LDN, LDN, ga_f32x4{0.f, 0.f, 0.f, 0.f}, lane);
            // the O tile goes back through sQ (nobody reads Q after the barrier above): rows of this wave only
#pragma unroll
            for (int e = 0; e < 4; ++e) stf<T>(sQ + (i0 + e) * LDD + 16 * t + r, acc[e]);
        }
        if (r == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int tok = s_tok[i0 + e];
                if (tok >= 0) lse[(int64_t)h * g.rows + tok] = lg[e];
            }
        }
    }
    __syncthreads();
    ga_unstage<T>(sQ, s_tok, o + h * GA_HD, ldo, tid);
}

// ---- backward: grid (chunks * heads); the workgroup walks groups [chunk ipb, (chunk + 1) ipb) of head h -----------------------------------
template <typename T>
__global__ void __launch_bounds__(GA_THREADS) group_attn_bwd_kernel(const T* __restrict__ qkv, int64_t ldq, const float* __restrict__ bias,
                                                                    const T* __restrict__ d_o, int64_t lddo, const float* __restrict__ lse,
                                                                    T* __restrict__ dqkv, int64_t lddq, float* __restrict__ ws,
                                                                    const GaGeom g, float scale, int ipb) {
    constexpr int LDD = GaLd<T>::d, LDN = GaLd<T>::n;
    __shared__ __attribute__((aligned(16))) T sQ[GA_NMAX * LDD];
    __shared__ __attribute__((aligned(16))) T sK[GA_NMAX * LDD];
    __shared__ __attribute__((aligned(16))) T sV[GA_NMAX * LDD];
    __shared__ __attribute__((aligned(16))) T sdO[GA_NMAX * LDD];
    __shared__ __attribute__((aligned(16))) T sQt[GA_HD * LDN];
    __shared__ __attribute__((aligned(16))) T sKt[GA_HD * LDN];
    __shared__ __attribute__((aligned(16))) T sdOt[GA_HD * LDN];
    __shared__ __attribute__((aligned(16))) T sA[GA_NMAX * LDN];       // P [i][j], then dS [i][j]
    __shared__ __attribute__((aligned(16))) T sAt[GA_NMAX * LDN];      // P^T [j][i], then dS^T [j][i]
    __shared__ int s_tok[GA_NMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x % g.heads, chunk = blockIdx.x / g.heads;
    const int C = g.heads * GA_HD, N = g.N;
    const int r = lane & 15, q4 = lane >> 4;
    const int i0 = 16 * wave + 4 * q4;
    const bool act = 16 * wave < N;
    const ga_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // this lane's 16 bias values (rows i0 .. i0 + 3, columns 16 t + r): the same for every group of the head
    float bv[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[t][e] = (i0 + e < N && 16 * t + r < N) ? bias[((int64_t)h * N + i0 + e) * N + 16 * t + r] : 0.f;
    }
    ga_f32x4 db[4] = {zero, zero, zero, zero};        // running sum of dS over this workgroup's groups: rows i0 .. i0 + 3, columns 16 t + r
    const int it1 = min(g.items, (chunk + 1) * ipb);
    for (int it = chunk * ipb; it < it1; ++it) {
        __syncthreads();                              // the previous group's readers are done with the tiles
        if (tid < GA_NMAX) s_tok[tid] = ga_token(g, it, tid);
        __syncthreads();
        ga_stage<T, true, true>(qkv + h * GA_HD, ldq, s_tok, sQ, sQt, tid);
        ga_stage<T, true, true>(qkv + C + h * GA_HD, ldq, s_tok, sK, sKt, tid);
        ga_stage<T, true, false>(qkv + 2 * C + h * GA_HD, ldq, s_tok, sV, nullptr, tid);
        ga_stage<T, true, true>(d_o + h * GA_HD, lddo, s_tok, sdO, sdOt, tid);
        __syncthreads();
        ga_f32x4 ds[4];
        if (act) {
            ga_f32x4 p[4];
            float l[4], delta[4] = {0.f, 0.f, 0.f, 0.f};
            bool qok[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int tok = s_tok[i0 + e];
                qok[e] = tok >= 0;
                l[e] = qok[e] ? lse[(int64_t)h * g.rows + tok] : 0.f;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                p[t] = ga_mma<T, GA_HD>(sQ + 16 * wave * LDD, LDD, sK + 16 * t * LDD, LDD, zero, lane);
                ds[t] = ga_mma<T, GA_HD>(sdO + 16 * wave * LDD, LDD, sV + 16 * t * LDD, LDD, zero, lane);      // dP = dO V^T
                const bool key = s_tok[16 * t + r] >= 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool ok = key && qok[e];
                    p[t][e] = ok ? __expf(fmaf(p[t][e], scale, bv[t][e]) - l[e]) : 0.f;
                    delta[e] = fmaf(p[t][e], ds[t][e], delta[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) delta[e] = wave_sum(delta[e], 16);       // = sum_d dO[i][d] O[i][d]
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ds[t][e] = p[t][e] * (ds[t][e] - delta[e]);
                    db[t][e] += ds[t][e];
                    stf<T>(sA + (i0 + e) * LDN + 16 * t + r, p[t][e]);
                    stf<T>(sAt + (16 * t + r) * LDN + i0 + e, p[t][e]);
                }
            }
        } else {
            // rows of P / columns of P^T past the group's slots: zeros, so that the products over 64 slots read nothing stale
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                ds[t] = zero;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    stf<T>(sA + (i0 + e) * LDN + 16 * t + r, 0.f);
                    stf<T>(sAt + (16 * t + r) * LDN + i0 + e, 0.f);
                }
            }
        }
        __syncthreads();
        if (act) {          // dV rows (keys) 16 wave .. + 15:  dV = P^T dO
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const ga_f32x4 acc = ga_mma<T, GA_NMAX>(sAt + 16 * wave * LDN, LDN, sdOt + 16 * t * LDN, LDN, zero, lane);
                // (V was last read for dP, before the barrier above: its tile takes dV, this wave's rows)
#pragma unroll
                for (int e = 0; e < 4; ++e) stf<T>(sV + (i0 + e) * LDD + 16 * t + r, acc[e]);
            }
        }
        __syncthreads();
        if (act) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    stf<T>(sA + (i0 + e) * LDN + 16 * t + r, ds[t][e]);
                    stf<T>(sAt + (16 * t + r) * LDN + i0 + e, ds[t][e]);
                }
            }
        }
        __syncthreads();
        if (act) {          // dQ = scale dS K (query rows), dK = scale dS^T Q (key rows)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const ga_f32x4 aq = ga_mma<T, GA_NMAX>(sA + 16 * wave * LDN, LDN, sKt + 16 * t * LDN, LDN, zero, lane);
                const ga_f32x4 ak = ga_mma<T, GA_NMAX>(sAt + 16 * wave * LDN, LDN, sQt + 16 * t * LDN, LDN, zero, lane);
                // (the row-major Q and K tiles were last read for the scores: they take dQ and dK; the products read the transposed copies)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    stf<T>(sQ + (i0 + e) * LDD + 16 * t + r, aq[e] * scale);
                    stf<T>(sK + (i0 + e) * LDD + 16 * t + r, ak[e] * scale);
                }
            }
        }
        __syncthreads();
        ga_unstage<T>(sQ, s_tok, dqkv + h * GA_HD, lddq, tid);
        ga_unstage<T>(sK, s_tok, dqkv + C + h * GA_HD, lddq, tid);
        ga_unstage<T>(sV, s_tok, dqkv + 2 * C + h * GA_HD, lddq, tid);
    }
    // ws: [chunk][head][N][N], the layout of dbias per chunk
    float* slab = ws + ((int64_t)chunk * g.heads + h) * (N * N);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < N && 16 * t + r < N) slab[(i0 + e) * N + 16 * t + r] = db[t][e];
    }
}

// dbias[h][i][j] = sum over the chunks' slabs, in chunk order
__global__ void __launch_bounds__(256) group_attn_dbias_kernel(const float* __restrict__ ws, float* __restrict__ dbias, int heads, int N,
                                                               int chunks) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= heads * N * N) return;
    float a = 0.f;
    for (int c = 0; c < chunks; ++c) a += ws[(int64_t)c * heads * N * N + idx];
    dbias[idx] = a;
}

// 16-byte row chunks: base and row stride
static bool ga_vec_ok(int dt, const void* p, int64_t ld) {
    const int per = dt == SEGF_BF16 ? 8 : 4;
    return ((uintptr_t)p & 15) == 0 && ld % per == 0;
}

}  // namespace

extern "C" int segf_group_attention_supported(int dt, int B, int H, int W, int heads, int hd, int G, int interval, int lda) {
    GaGeom g;
    return (dt == SEGF_F32 || dt == SEGF_BF16) && ga_geom(B, H, W, heads, hd, G, interval, lda, g);
}

extern "C" int segf_group_attention_fwd(int dt, int B, int H, int W, int heads, int hd, int G, int interval, int lda, const void* qkv,
                                        int64_t ldqkv, const float* bias, float scale, void* o, int64_t ldo, float* lse, void* stream) {
    GaGeom g;
    if (!ga_geom(B, H, W, heads, hd, G, interval, lda, g)) return SEGF_ERR_SHAPE;          // before any launch
    if (ldqkv < 3 * heads * hd || ldo < heads * hd || !ga_vec_ok(dt, qkv, ldqkv) || !ga_vec_ok(dt, o, ldo)) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(g.items * heads));
    SEGF_DISPATCH_DT(dt, T, {
        hipLaunchKernelGGL((group_attn_fwd_kernel<T>), grid, dim3(GA_THREADS), 0, st, (const T*)qkv, ldqkv, bias, (T*)o, ldo, lse, g, scale);
    })
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t segf_group_attention_bwd_ws(int B, int H, int W, int heads, int hd, int G, int interval, int lda) {
    GaGeom g;
    if (!ga_geom(B, H, W, heads, hd, G, interval, lda, g)) return 0;
    return (int64_t)ga_chunks(g) * heads * g.N * g.N;
}

extern "C" int segf_group_attention_bwd(int dt, int B, int H, int W, int heads, int hd, int G, int interval, int lda, const void* qkv,
                                        int64_t ldqkv, const float* bias, float scale, const void* d_o, int64_t lddo, const float* lse,
                                        void* dqkv, int64_t lddqkv, float* dbias, float* ws, void* stream) {
    GaGeom g;
    if (!ga_geom(B, H, W, heads, hd, G, interval, lda, g)) return SEGF_ERR_SHAPE;
    if (ldqkv < 3 * heads * hd || lddqkv < 3 * heads * hd || lddo < heads * hd || !ga_vec_ok(dt, qkv, ldqkv) || !ga_vec_ok(dt, d_o, lddo) ||
        !ga_vec_ok(dt, dqkv, lddqkv))
        return SEGF_ERR_SHAPE;
    if (!ws) return SEGF_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int ipb = ga_items_per_block(g), chunks = ga_chunks(g);
    const dim3 grid((unsigned)(chunks * heads));
    SEGF_DISPATCH_DT(dt, T, {
        hipLaunchKernelGGL((group_attn_bwd_kernel<T>), grid, dim3(GA_THREADS), 0, st, (const T*)qkv, ldqkv, bias, (const T*)d_o, lddo, lse,
                           (T*)dqkv, lddqkv, ws, g, scale, ipb);
    })
    SEGF_CHECK_LAUNCH();
    hipLaunchKernelGGL(group_attn_dbias_kernel, dim3((unsigned)((heads * g.N * g.N + 255) / 256)), dim3(256), 0, st, ws, dbias, heads, g.N,
                       chunks);
    SEGF_CHECK_LAUNCH();
    return 0;
}
