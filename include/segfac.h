/*
 * segfac.h -- C ABI of libsegfac_hip.so: the MI355X (gfx950) kernels underneath the
 * Segmentation_Factory plugin API (SegmentationModel / backbones / heads / engine.criterion /
 * util.metrics).  The reference has no native boundary on this path (it is eager PyTorch,
 * SURVEY.md section 2.2); each entry point below names the reference code it stands in for.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch caching allocator);
 *     kernels never allocate, free or keep pointers; workspaces are caller-provided.
 *   - activations are token-major / NHWC: element (row, c) at base[row * ld + c]; `ld` in elements.
 *   - dt: SEGF_F32 (0) or SEGF_BF16 (1) = storage type of activations; all arithmetic,
 *     statistics and accumulation are fp32.  Parameters and parameter gradients are fp32.
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue, never synchronise.
 *   - return 0 = enqueued; <0 = argument error (-1 shape/alignment, -2 dtype, -3 workspace);
 *     >0 = hipError_t from the launch.  Nothing is printed.
 */
#ifndef SEGFAC_H
#define SEGFAC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEGF_F32 0
#define SEGF_BF16 1
#define SEGF_ERR_SHAPE (-1)
#define SEGF_ERR_DTYPE (-2)
#define SEGF_ERR_WORKSPACE (-3)

/* library / build info: returns a static string "segfac-hip <version> gfx950" */
const char* segf_version(void);

/* ---- elementwise plumbing ------------------------------------------------------------------- */
/* dst[i] = (dst_dt) src[i] */
int segf_cast(const void* src, int src_dt, void* dst, int dst_dt, int64_t n, void* stream);
/* dst[r][c] = (dst_dt) src[r][c], r < rows, c < cols, with leading dimensions (elements): weight packing / column slices */
int segf_cast2d(const void* src, int src_dt, int64_t ld_src, void* dst, int dst_dt, int64_t ld_dst, int64_t rows, int64_t cols,
                void* stream);
/* out[a][c][b] = in[a][b][c]  (+ zero padding of the last output dim up to ldb_out):
 * OIHW -> O(HW)I weight re-layout for NHWC im2col GEMMs (models/backbones/mit.py:105 conv weights),
 * NCHW <-> NHWC at the plugin boundary (mit.py:198 permute).  */
int segf_permute021(const void* in, int in_dt, void* out, int out_dt, int64_t A, int64_t Bd, int64_t Cd,
                    int64_t ld_out, void* stream);
/* Several of the three jobs above in ONE launch (the small-batch step is bound by its launch count, train_gpu.py:71 default batch 4):
 *   op 0  dst[r][c] = (dst_dt) src[r][c]                       rows x cols, leading dimensions ld_src / ld_dst (segf_cast2d)
 *   op 1  dst[a][c][b] = (dst_dt) src[a][b][c], a < rows, b < pb, c < pc; output row length ld_dst >= pb, the rest zero (segf_permute021);
 *         cols > 0: element distance between consecutive dst[a] blocks (default pc * ld_dst)
 *   op 2  dst[r][c] = 0                                        rows x cols at ld_dst
 * Jobs of one call must not overlap in what they write / read from each other: they run concurrently. */
typedef struct SegfPrepItem {
    const void* src; void* dst;
    int64_t rows, cols, ld_src, ld_dst, pb, pc;
    int32_t op, src_dt, dst_dt, reserved;
} SegfPrepItem;
int segf_prep_grouped(int n, const SegfPrepItem* items, void* stream);
/* y[r][c] = x[r][c] * scale[r / rows_per_group]   (DropPath backward, models/layers/drop_path.py:18-25) */
int segf_scale_rows(int dt, const void* x, int64_t ldx, void* y, int64_t ldy, const float* scale,
                    int64_t rows, int64_t cols, int64_t rows_per_group, void* stream);
/* y[r][c] = x[r][c] * scale[r * cols + c], scale fp32 and dense: nn.Dropout per element (heads/deeplabv3.py:56,115) with the
 * keep-scales of segf_bernoulli_scale; the backward is the same call on the gradient.  cols % 8 == 0. */
int segf_mul_scale(int dt, const void* x, int64_t ldx, const float* scale, void* y, int64_t ldy, int64_t rows, int64_t cols,
                   void* stream);
/* y = a + b  (residual / gradient fan-in), 2-D with leading dims */
int segf_add(int dt, const void* a, int64_t lda, const void* b, int64_t ldb, void* y, int64_t ldy,
             int64_t rows, int64_t cols, void* stream);
/* out[c] = sum_r x[r][c] as fp32 (bias gradients of nn.Linear / 1x1 conv).  ws >= segf_colsum_ws(rows, cols) floats */
int64_t segf_colsum_ws(int64_t rows, int64_t cols);
int segf_colsum(int dt, const void* x, int64_t ldx, int64_t rows, int64_t cols, float* out, float* ws, void* stream);

/* zero-fill / counter increment / stochastic-layer scales as library kernels (no framework kernels inside the captured step).
 * segf_bernoulli_scale: out[i] = U_i < keep_prob[i / row_len] ? 1 / keep_prob[i / row_len] : 0 -- DropPath
 * (models/layers/drop_path.py:18-25) with rows = draws and row_len = batch, Dropout2d (heads/segformer.py:40) with one row of
 * B * C entries; state = {seed, launch counter} (uint64[2], advanced by the kernel: graph replays draw fresh numbers). */
int segf_zero(void* p, int64_t nbytes, void* stream);
int segf_add_i64(int64_t* p, int64_t v, void* stream);
/* Metrics.update's `self.hist += bincount(...)` (util/metrics.py:24-27): hist fp32 [n] += (float)counts int64 [n] (torch's promotion of
 * float32 += int64: each count rounded to fp32, then added); clear != 0 also zeroes the counts for the next batch. */
int segf_hist_accum(float* hist, int64_t* counts, int64_t n, int clear, void* stream);
/* test hook: a single wave that occupies `stream` for `us` microseconds (<= 200000), e.g. to delay a gradient in the data-parallel
 * ordering test (the event-ordered exchange of train_gpu.py:233-236's DDP replacement). */
int segf_debug_spin(int64_t us, void* stream);
/* Tuning switch of the eight-phase GEMM (gemm8.hip; the UPerHead / PPM 3x3 ConvModules of heads/upernet.py:26-31, modules/ppm.py:19 and
 * the ConvNeXt block MLPs on fp8 operands): what = 0 selects whether the fp8 kernels run their two wave groups one barrier apart
 * (value 1, default) or in lockstep (value 0); any other value only reads.  Returns the previous setting (or SEGF_ERR_SHAPE).  The host
 * layer times both on the device at hand once per process: devices differ in the clock they hold under the denser schedule. */
int segf_gemm8_option(int what, int value);
int segf_bernoulli_scale(uint64_t* state, const float* keep_prob, int64_t n, int64_t row_len, float* out, void* stream);

/* ---- FP8 (OCP e4m3fn) forward GEMM: BASELINE cfg5 "ConvNeXtV2-L + UPerNet, fp8 MFMA weights" (the pointwise linears of
 * convnextv2.py:90-95; no fp8 exists in the reference -- an option of this build, tolerance stated in the tests) ------------
 * segf_quant_rows_fp8: q[r][k] = e4m3(x[r][k] / scale[r]), scale[r] = amax_k |x[r][k]| / 448 (token rows of the activations,
 * output-channel rows of the weights); x of dtype dt, K % 8 == 0.
 * segf_gemm_fp8: C[M][N] (bf16) = (A[M][K] . B[N][K]^T) * scale_a[m] * scale_b[n] + bias[n], optionally
 * residual[m][n] + rscale[m / rows_per_group] * (...); A, B e4m3 bytes; v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulate;
 * K % 128 == 0 (segf_gemm_fp8_supported). */
int segf_quant_rows_fp8(int dt, int64_t rows, int K, const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, void* stream);
int segf_gemm_fp8_supported(int64_t M, int64_t N, int64_t K);
int segf_gemm_fp8(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const float* scale_a, const void* B, int64_t ldb,
                  const float* scale_b, const float* bias, const void* residual, int64_t ldr, const float* rscale,
                  int64_t rows_per_group, void* C, int64_t ldc, void* stream);

/* fp8 3x3 convolutions (the UPerHead / PPM ConvModules, heads/upernet.py:26-31, modules/ppm.py:19: ~700 of cfg5's 2,050 GFLOP per
 * image).  segf_quant_tensor_fp8: ONE scale for a whole [rows][cols] tensor (the implicit-GEMM K axis gathers nine pixels, so
 * per-token scales do not factor out): q = cvt(x / scale), scale = amax |x| / FMAX; fmt 0 = e4m3fn (activations, FMAX 448),
 * 1 = e5m2 (gradients, FMAX 57344); amax_ws = 4 bytes of scratch; all on the stream, no host read (graph-safe).
 * segf_conv3x3_fp8: mode 0  y[pix][co] = sx * sw[co] * sum_{tap,ci} xq[pix+off(tap)][ci] wq[co][tap*Cin+ci]   (xq e4m3, wq e4m3 rows)
 *                   mode 1  dx[pix][ci] = sx * sw[ci] * sum_{tap,co} gq[pix-off(tap)][co] wq[ci][tap*Cout+co]  (gq e5m2, wq e4m3 rows)
 * bf16 output; Cin, Cout multiples of 16; ldx / ldw in bytes = elements, multiples of 16. */
int segf_quant_tensor_fp8(int dt, int fmt, int64_t rows, int cols, const void* x, int64_t ldx, void* q, int64_t ldq, float* scale,
                          void* amax_ws, void* stream);
int segf_conv3x3_fp8_supported(int mode, int B, int H, int W, int Cin, int Cout);
int segf_conv3x3_fp8(int mode, int B, int H, int W, int Cin, int Cout, const void* xq, int64_t ldx, const float* sx,
                     const void* wq, int64_t ldw, const float* sw, void* y, int64_t ldy, void* stream);
/* ... and the weight gradient on the SAME quantised tensors: dW[co][tap*Cin+ci] = sg * sx * sum_pix gq[pix][co] xq[pix+off(tap)][ci]
 * (gq: the e5m2 gradient of the data-gradient call, xq: the e4m3 input of the forward call; strides in bytes), fp32 [Cout][9*Cin];
 * split_k > 1 needs ws >= split_k * Cout * 9 * Cin floats.  Cin % 128 == 0, Cout % 256 == 0, B*H*W >= 65536. */
int segf_conv3x3_fp8_wgrad_supported(int B, int H, int W, int Cin, int Cout);
int segf_conv3x3_fp8_wgrad(int B, int H, int W, int Cin, int Cout, const void* xq, int64_t ldx, const float* sx, const void* gq,
                           int64_t ldg, const float* sg, float* dw, int64_t lddw, int split_k, float* ws, void* stream);

/* nn.Linear products on fp8 operands with one scale per activation / gradient TENSOR and one per weight row (the ConvNeXt block MLPs,
 * convnextv2.py:83-113), on the 256 x 256 tile kernel:
 *   mode 0  y[m][n] = sa * sb[n] * sum_k Aq[m][k] Bq[n][k] (+ bias[n]); with residual: y = residual + rscale[m / rows_per_group] * (..)
 *           Aq e4m3 [M][K] (segf_quant_tensor_fp8, fmt 0), Bq e4m3 [N][K] (segf_quant_rows_fp8 of the weight), bf16 out
 *   mode 1  the same with Aq in e5m2: the data gradient dx = dy W (Aq = the quantised gradient [M][N_out], Bq = W^T quantised per row)
 *   segf_linear_fp8_wgrad: dW[n][k] = sg * sx * sum_t gq[t][n] xq[t][k], gq e5m2 [T][N], xq e4m3 [T][K] -- the tensors mode 1 / mode 0
 *           were called with -- fp32 out; split_k > 1 needs ws >= split_k * N * K floats.
 * M (T), N multiples of 256, K of 128; strides in bytes = elements, multiples of 16.  segf_linear_fp8_supported(mode, M, N, K) with
 * mode 2 = the weight gradient (M = T tokens, N x K the weight). */
int segf_linear_fp8_supported(int mode, int64_t M, int64_t N, int64_t K);
int segf_linear_fp8(int mode, int64_t M, int64_t N, int64_t K, const void* Aq, int64_t lda, const float* sa, const void* Bq,
                    int64_t ldb, const float* sb, void* C, int64_t ldc, const float* bias, const void* residual, int64_t ldr,
                    const float* rscale, int64_t rows_per_group, void* stream);
int segf_linear_fp8_wgrad_splitk(int64_t N, int64_t K, int64_t T);      /* slices over the tokens (sizes ws) */
int segf_linear_fp8_wgrad(int64_t N, int64_t K, int64_t T, const void* gq, int64_t ldg, const float* sg, const void* xq,
                          int64_t ldx, const float* sx, float* dw, int64_t lddw, int split_k, float* ws, void* stream);

/* ---- stream ordering for the data-parallel exchange (train_gpu.py:233-236: DistributedDataParallel overlaps the gradient
 * all-reduce with backward through per-bucket hooks).  segf_event_record(.., external=1) during a stream capture adds an
 * EVENT-RECORD NODE to the hipGraph (hipEventRecordExternal); at each replay a stream outside the graph can
 * segf_stream_wait_event() on it: "this bucket of gradients is final".  `event` / `stream` are hipEvent_t / hipStream_t. */
int segf_event_create(void** event);
int segf_event_destroy(void* event);
int segf_event_record(void* event, void* stream, int external);
int segf_stream_wait_event(void* stream, void* event);

/* ---- GEMM: nn.Linear / 1x1 conv / im2col'd conv, forward and both backward products -------------
 * C[M,N] = epilogue( sum_k A(m,k) * B(k,n) ), fp32 accumulate.
 *   layout 0: A stored [M][K] (lda), B stored [N][K] (ldb)   y  = x W^T      (F.linear forward)
 *   layout 1: A stored [M][K],       B stored [K][N]         dx = dy W
 *   layout 2: A stored [K][M],       B stored [K][N]         dW = dy^T x     (K = token count)
 * epilogue: v = acc (+ bias[n]); if residual: v = residual[m][n] + (rscale ? rscale[m / rows_per_group] : 1) * v
 * c_dt may be SEGF_F32 while dt is SEGF_BF16 (parameter gradients).
 * split_k > 1 (layout 2 only) needs ws >= split_k * M * N floats; result is reduced deterministically.
 * bf16 uses v_mfma_f32_16x16x32_bf16; f32 uses an fp32 FMA kernel (exact-fp32 parity mode).       */
int segf_gemm(int dt, int layout, int64_t M, int64_t N, int64_t K,
              const void* A, int64_t lda, const void* B, int64_t ldb,
              void* C, int c_dt, int64_t ldc,
              const float* bias, const void* residual, int64_t ldr,
              const float* rscale, int64_t rows_per_group,
              int split_k, float* ws, void* stream);
int segf_gemm_pick_splitk(int64_t M, int64_t N, int64_t K);
/* Product whose ACTIVATION operand is normalised on the way into LDS: ConvModule's BatchNorm2d + ReLU and the Dropout2d
 * channel scale in front of SegFormerHead.linear_pred (heads/segformer.py:21-29,40,57-58), folded into per-(sample, channel)
 * tables by segf_bn_affine_table, so that the normalised [B*H*W, C] tensor is never written or re-read:
 *   layout 0:  C[M,N] = act(A s + t) B^T + bias      (A [M tokens][K], B [N][K]; bf16 out)
 *   layout 2:  C[M,N] = A^T act(B s + t)             (A = dy [K tokens][M], B = x [K tokens][N]; fp32 out, split-K)
 * s, t: fp32 [tokens / rows_per_group][features] (features = K in layout 0, N in layout 2); act 0 none / 1 ReLU / 2 ReLU6
 * (ReLU6 only with unit channel scale).  Implemented by the 256x256-tile kernel only: segf_gemm_pro_supported() tells
 * whether a shape qualifies (the caller otherwise materialises the normalised tensor with segf_bn_apply). */
int segf_gemm_pro_supported(int dt, int layout, int64_t M, int64_t N, int64_t K, int64_t rows_per_group);
int segf_gemm_pro(int dt, int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb,
                  void* C, int c_dt, int64_t ldc, const float* bias, int split_k, float* ws, const float* pro_scale,
                  const float* pro_shift, int64_t rows_per_group, int act, void* stream);
int segf_bn_affine_table(const float* mean, const float* rstd, const float* gamma, const float* beta, const float* chan_scale,
                         int groups, int C, float* scale, float* shift, void* stream);
/* Weight gradient and bias gradient of nn.Linear / 1x1 conv in ONE pass over dy (mit.py:45,52,58,98-99 backward):
 *   C[M,N] = sum_k A(k,m) B(k,n)  (layout 2: A = dy [K tokens][M], B = x [K tokens][N]),  dbias[m] = sum_k A(k,m)  (fp32).
 * The column sums ride on the matrix pipe (an all-ones operand) inside the GEMM; shapes that take the 256x256-tile or fp32
 * kernels run a separate column reduction behind the product.  ws >= segf_gemm_dw_db_ws(M, N, K, split_k) floats. */
int64_t segf_gemm_dw_db_ws(int64_t M, int64_t N, int64_t K, int split_k);
int segf_gemm_dw_db(int dt, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb,
                    void* C, int c_dt, int64_t ldc, int split_k, float* ws, float* dbias, void* stream);
/* The same for SEVERAL layers in one call (the backward of a MiT / ConvNeXt block: q, kv, proj, fc1, fc2 of mit.py:43-59,98-99 -- their
 * weight gradients do not depend on each other).  Items that take the 128-tile split-K kernel are gathered into grouped launches (one
 * product launch + one reduce launch per up to 12 layers); the rest run exactly as segf_gemm_dw_db.  Every item's dw [M][lddw] fp32 and
 * db [M] are (with shared_split == 0) bitwise what segf_gemm_dw_db(dt, M, N, K, dy, lddy, x, ldx, dw, F32, lddw, split_k, ws, db) produces; ws per item >=
 * segf_gemm_dw_db_ws(M, N, K, split_k) floats, 16-byte aligned. */
typedef struct SegfDwItem {
    int64_t M, N, K;            /* dw = dy^T x: dy [K][M], x [K][N] (K = tokens) */
    const void* dy; int64_t lddy;
    const void* x; int64_t ldx;
    float* dw; int64_t lddw;
    float* db;
    float* ws;
    int split_k;
    int shared_split;           /* != 0: split_k is an UPPER BOUND -- inside a group the flagged members may run with fewer slices (one common
                                 * K range per slice, chosen so that the group as a whole fills the chip); 0: exactly split_k, bitwise
                                 * segf_gemm_dw_db */
} SegfDwItem;
int segf_gemm_dw_db_grouped(int dt, int n, const SegfDwItem* items, void* stream);

/* ---- LayerNorm over the last dim (nn.LayerNorm eps 1e-5 in mit.py:107,136-140,178-190; ConvNeXt's
 * channels-first LayerNorm, convnext.py:8-23, is the same kernel on NHWC rows) ---------------------- */
int segf_layernorm_fwd(int dt, int64_t rows, int C, const void* x, const float* gamma, const float* beta,
                       float eps, void* y, float* mean, float* rstd, void* stream);
int64_t segf_layernorm_bwd_ws(int64_t rows, int C);
int segf_layernorm_bwd(int dt, int64_t rows, int C, const void* x, const void* dy, const float* gamma,
                       const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta,
                       float* ws, void* stream);
/* the same with two optional fan-in operands, so that a pre-norm residual block needs no separate gradient additions
 * (mit.py:143-146 `x + drop_path(f(norm(x)))`: dx = dres + LN_bwd(dy)) and a normalised map with two consumers (the stage
 * output feeding the head and the next patch embedding, mit.py:196-216) sums their gradients on load:
 *   dx = LN_bwd(dy + dy2) + dres;   dy2, dres nullable, [rows][C] of dtype dt. */
int segf_layernorm_bwd_fused(int dt, int64_t rows, int C, const void* x, const void* dy, const void* dy2, const void* dres,
                             const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta,
                             float* ws, void* stream);
/* ... with a second output dxs[r][c] = (dt) dx[r][c] * rscale[r / rows_per_group] (NULL, NULL: none): when dx's consumer is the backward of
 * a residual branch x + DropPath(f(.)) (mit.py:143-146, drop_path.py:18-25), the first thing it does is this row scaling of dx --
 * segf_scale_rows on the stored dx, bitwise.  rows < 2^22. */
int segf_layernorm_bwd_scaled(int dt, int64_t rows, int C, const void* x, const void* dy, const void* dy2, const void* dres,
                              const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta,
                              float* ws, const float* rscale, int64_t rows_per_group, void* dxs, void* stream);
/* The spatial-reduction convolution of MiT's attention (mit.py:20-22,47-48: Conv2d(dim, dim, sr, sr) on the LayerNorm output) without
 * im2col / col2im passes: segf_layernorm_fwd_patch also writes its output in the PATCH-MAJOR row order of that convolution's im2col matrix
 * (token (b, y, x) -> row ((b Ho + y / sr) Wo + x / sr), chunk (y % sr, x % sr)), so y2 viewed as [rows / sr^2][sr^2 C] is the matrix itself;
 * segf_layernorm_bwd_patch reads its fan-in operand dy2 in the same order -- the data gradient of the convolution as its product leaves it.
 * Map width W = 2^log2_w, sr = 2^log2_sr, rows % (W sr) == 0; log2_w < 0 in the backward: dy2 in token order (segf_layernorm_bwd_scaled). */
int segf_layernorm_fwd_patch(int dt, int64_t rows, int C, const void* x, const float* gamma, const float* beta, float eps, void* y,
                             float* mean, float* rstd, void* y2, int log2_w, int log2_sr, void* stream);
int segf_layernorm_bwd_patch(int dt, int64_t rows, int C, const void* x, const void* dy, const void* dy2, const void* dres,
                             const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta,
                             float* ws, const float* rscale, int64_t rows_per_group, void* dxs, int log2_w, int log2_sr, void* stream);
/* Deferred finalize: with dgamma == NULL segf_layernorm_bwd_fused leaves its per-block partial sums [blocks][2 C] in ws
 * (blocks = segf_layernorm_bwd_blocks(rows, C)) and the caller finalizes SEVERAL such reductions in one launch later:
 * out[i] = sum_b partial[b][i], i < len, summed in the order of the single finalize (bitwise the same dgamma / dbeta). */
typedef struct SegfFinalizeItem { const float* partial; float* out; int64_t len; int nblk; int scatter_c; } SegfFinalizeItem;
/* scatter_c = C > 0 (len must be 10 C): the sums are the [10][C] partials of segf_dwconv3x3_gelu_bwd called with dw == NULL
 * (segf_dwconv3x3_bwd_blocks(dt, B, H, W, C) blocks in its ws) and land as out = dw[C][9] followed by db[C] (mit.py:62-71 backward). */
int segf_layernorm_bwd_blocks(int64_t rows, int C);
int segf_colreduce_finalize_grouped(int n, const SegfFinalizeItem* items, void* stream);
/* The backward of `LayerNorm -> Linear` where the Linear is C -> N = 4 C wide, C = 32 or 64 (norm2 -> mlp.fc1 of a MiT block, mit.py:98,136-146)
 * in ONE pass over the hidden-width gradient dh [rows][N] (csrc/norm.hip: ln_linear_bwd_kernel): per tile of 64 token rows
 *   dy  = bf16(dh W1)                         the Linear's data gradient, bits of segf_gemm (layout 1) on these operands; never stored
 *                                             unless dy_out (nullable, [rows][C]) asks for it
 *   dx  = LN_bwd(dy) + dres                   bits of segf_layernorm_bwd_fused (dy2 == NULL) on that dy; dres nullable
 *   dxs = (dt) dx * rscale[r / rows_per_group] (NULL, NULL: none) bits of segf_scale_rows on the stored dx; any rows < 2^31 (the group
 *                                             index is an integer division here, so the 2^22 bound of segf_layernorm_bwd_scaled does not apply)
 *   dw1 [N][C] = dh^T y, db1 [N] = colsum(dh), dgamma | dbeta [2][C]   fp32, from per-workgroup partials in fixed order (no atomics:
 *                                             bitwise reproducible; NOT the summation order of segf_gemm_dw_db / segf_layernorm_bwd)
 * dh, x (the LayerNorm's input), y (its saved output), dres, dx, dxs, dy_out: bf16, 16-byte aligned, dense rows; w1 bf16 [N][C] dense.
 * dbeta == dgamma + C.  ws >= segf_layernorm_linear_bwd_ws(rows, C, N) floats.
 * Deferred finalize: with dw1 == NULL (then db1, dgamma, dbeta NULL too) the partials stay in ws as three blocks
 *   [nblk][N C] at ws, [nblk][N] at ws + nblk N C, [nblk][2 C] at ws + nblk (N C + N),   nblk = segf_layernorm_linear_bwd_blocks(rows),
 * for three SegfFinalizeItem members of a later segf_colreduce_finalize_grouped call (the same sums as the immediate form).
 * _supported: host arithmetic only; bf16, C in {32, 64}, N == 4 C, rows < 2^31 and SEGFAC_LN_LINEAR_BWD_FUSED (0 never, 1 from 131072
 * rows on, 2 wherever the shape has the kernel).  The entry point itself checks the shape only: fp32 returns SEGF_ERR_DTYPE. */
int segf_layernorm_linear_bwd_supported(int dt, int64_t rows, int C, int N);
int segf_layernorm_linear_bwd_blocks(int64_t rows);
int64_t segf_layernorm_linear_bwd_ws(int64_t rows, int C, int N);
int segf_layernorm_linear_bwd(int dt, int64_t rows, int C, int N, const void* dh, const void* w1, const void* x, const void* y,
                              const void* dres, const float* gamma, const float* mean, const float* rstd, void* dx,
                              const float* rscale, int64_t rows_per_group, void* dxs, void* dy_out, float* dw1, float* db1,
                              float* dgamma, float* dbeta, float* ws, void* stream);
/* The general form (csrc/norm.hip: ln_linear_bwd_kernel<KS, true, HM, FAN>), N = 4 C or N = C (the attention's q Linear behind norm1):
 *   y == NULL   the LayerNorm output is REBUILT from x, mean, rstd, gamma and beta (bits of segf_layernorm_fwd: dw1 does not change), so the
 *               forward keeps no y; y != NULL: N == 4 C only, segf_layernorm_linear_bwd itself
 *   dy2         (nullable, N == C only) a second consumer's gradient of the LayerNorm output, added to the bf16-rounded dy on load as
 *               segf_layernorm_bwd_patch adds it: patch-major row order with log2_w >= 0 (segf_layernorm_fwd_patch's y2), token order with < 0
 * Everything else as segf_layernorm_linear_bwd (same workspace layout with this N, same deferred finalize).
 * _ex_supported: bf16, C in {32, 64}, N in {C, 4 C}, rows < 2^31 and SEGFAC_LN_LINEAR_BWD_FUSED. */
int segf_layernorm_linear_bwd_ex_supported(int dt, int64_t rows, int C, int N);
int segf_layernorm_linear_bwd_ex(int dt, int64_t rows, int C, int N, const void* dh, const void* w1, const void* x, const void* y,
                                 const float* beta, const void* dy2, int log2_w, int log2_sr, const void* dres, const float* gamma,
                                 const float* mean, const float* rstd, void* dx, const float* rscale, int64_t rows_per_group, void* dxs,
                                 void* dy_out, float* dw1, float* db1, float* dgamma, float* dbeta, float* ws, void* stream);
/* `LayerNorm -> Linear` forward in ONE pass at C = 32 / 64, N = C or 4 C, bias present (norm1 -> attn.q, norm2 -> mlp.fc1 of a MiT block,
 * mit.py:45,98,136-146; csrc/norm.hip: ln_linear_fwd_kernel): the rows of x are normalised in registers and the bf16-rounded result is the
 * operand of the streaming product, so the C-wide LayerNorm output is neither written nor read back.
 *   out [rows][N] = bf16(y w^T + bias)   bits of segf_gemm (layout 0) on the y of segf_layernorm_fwd
 *   mean, rstd [rows]                    bits of segf_layernorm_fwd
 *   y  (nullable, [rows][C])             the LayerNorm output in token order, bits of segf_layernorm_fwd (only where a consumer still reads it)
 *   y2 (nullable)                        ... in patch-major row order: the arguments y2, log2_w, log2_sr of segf_layernorm_fwd_patch
 * x, out, y, y2: bf16, 16-byte aligned, dense rows; w bf16 [N][C] dense, 16-byte aligned; gamma, beta fp32 [C] 16-byte aligned; bias fp32 [N].
 * _supported: host arithmetic only; bf16, C in {32, 64}, N in {C, 4 C}, rows < 2^31 and SEGFAC_LN_LINEAR_FWD_FUSED (0 never, 1 from 131072
 * rows on, 2 wherever the shape has the kernel).  The entry point itself checks the shape only: fp32 returns SEGF_ERR_DTYPE.
 * _blocks: the workgroups the launch takes, min(ceil(ceil(rows / 16) / 16), 2048). */
int segf_layernorm_linear_fwd_supported(int dt, int64_t rows, int C, int N);
int segf_layernorm_linear_fwd_blocks(int64_t rows);
int segf_layernorm_linear_fwd(int dt, int64_t rows, int C, int N, const void* x, const float* gamma, const float* beta, float eps,
                              const void* w, const float* bias, void* out, float* mean, float* rstd, void* y, void* y2, int log2_w,
                              int log2_sr, void* stream);

/* ---- BatchNorm2d (train: batch statistics) + ReLU/ReLU6 + Dropout2d, NHWC rows -------------------
 * ConvModule of heads/segformer.py:21-29, layers/conv_module.py:4-9, mobilenetv2.py:5-11.
 * stats: mean/var(biased) over rows; running stats updated with momentum and unbiased var.
 * Accuracy: the variance is E[x^2] - mean^2 from fp32 sums of x and x^2 (combined in double), so it is as accurate as those sums allow
 * and its relative error grows as (mean / sigma)^2 (tests/test_norm_float64.py pins this).                    */
int64_t segf_bn_ws(int64_t rows, int C);
int segf_bn_stats(int dt, int64_t rows, int C, const void* x, float* mean, float* rstd,
                  float* running_mean, float* running_var, float momentum, float eps, float* ws, void* stream);
/* y = act(gamma * (x-mean)*rstd + beta) * (chan_scale ? chan_scale[row / rows_per_sample][c] : 1); act 0 none, 1 relu, 2 relu6 */
int segf_bn_apply(int dt, int64_t rows, int C, const void* x, const float* mean, const float* rstd,
                  const float* gamma, const float* beta, int act, const float* chan_scale,
                  int64_t rows_per_sample, void* y, void* stream);
/* training backward (batch statistics): dx, dgamma, dbeta.  eval_mode=1: statistics are constants. */
int segf_bn_bwd(int dt, int64_t rows, int C, const void* x, const void* dy, const float* mean, const float* rstd,
                const float* gamma, const float* beta, int act, const float* chan_scale, int64_t rows_per_sample,
                int eval_mode, void* dx, float* dgamma, float* dbeta, float* ws, void* stream);

/* BatchNorm backward of SegFormerHead's fuse ConvModule WITH the classifier's data gradient folded in (heads/segformer.py:21-29,
 * 40,57-58: linear_fuse.bn / activate -> Dropout2d -> linear_pred): instead of materialising da = dy W ([tokens, C]) and
 * streaming it twice through segf_bn_bwd, both BatchNorm passes recompute their da tile on the matrix pipe from the class
 * gradients dy [M][ldy >= K] (K = padded class count, a multiple of 32, pad columns zero) and w [K][ldw >= C] (classifier weight,
 * rows = classes, pad rows zero).  Same results as segf_gemm(layout 1) + segf_bn_bwd with da kept in fp32.
 * bf16 only; C % 128 == 0; rows_per_sample % 16 == 0: ask segf_bn_cls_bwd_supported.  ws >= segf_bn_cls_bwd_ws floats. */
int segf_bn_cls_bwd_supported(int dt, int64_t M, int C, int K, int64_t rows_per_sample);
int64_t segf_bn_cls_bwd_ws(int64_t M, int C, int64_t rows_per_sample);
int segf_bn_cls_bwd(int dt, int64_t M, int C, int K, const void* dy, int64_t ldy, const void* w, int64_t ldw, const void* x,
                    const float* mean, const float* rstd, const float* gamma, const float* beta, int act,
                    const float* chan_scale, int64_t rows_per_sample, int eval_mode, void* dx, float* dgamma, float* dbeta,
                    float* ws, void* stream);
/* The same with the NEXT backward step's weight-gradient product riding on pass 2: dx is the gradient of the folded SegFormerHead's
 * stride-4 map y = sum_i resize_i(x_i G_i^T) (heads/segformer.py:42-56); its stage-1 term needs dG_1 = dx^T x1 and colsum(dx), a
 * [C x C1] product over all M tokens.  dG: fp32 [C][C1 + 8] = [dx^T x1 | colsum(dx) | 0 x 7], accumulated from the bf16 dx tile each
 * workgroup has on chip (bit-identical operands to a separate product over the stored dx; saves one 2 M C byte pass).  C1 == 32,
 * K <= 160: ask segf_bn_cls_bwd_dw_supported.  ws >= segf_bn_cls_bwd_dw_ws floats. */
int segf_bn_cls_bwd_dw_supported(int dt, int64_t M, int C, int K, int64_t rows_per_sample, int C1);
int64_t segf_bn_cls_bwd_dw_ws(int64_t M, int C, int64_t rows_per_sample);
int segf_bn_cls_bwd_dw(int dt, int64_t M, int C, int K, const void* dy, int64_t ldy, const void* w, int64_t ldw, const void* x,
                       const float* mean, const float* rstd, const float* gamma, const float* beta, int act,
                       const float* chan_scale, int64_t rows_per_sample, int eval_mode, void* dx, float* dgamma,
                       float* dbeta, float* ws, const void* x1, int64_t ldx1, int C1, float* dG, void* stream);
/* The same with everything that can ride along, each part optional: (x1, dG) as in segf_bn_cls_bwd_dw (pass 2), and dwcls = the
 * CLASSIFIER's weight gradient fp32 [K][C] = dy^T act(bn(x)) * drop (heads/segformer.py:57-58 backward; act = 0 / 1 only),
 * formed in pass 1 from the x and dy tiles it already holds -- replaces the layout-2 segf_gemm_pro pass over x.
 * ws >= segf_bn_cls_bwd_full_ws(M, C, K, rows_per_sample) floats. */
int64_t segf_bn_cls_bwd_full_ws(int64_t M, int C, int K, int64_t rows_per_sample);
int segf_bn_cls_bwd_full(int dt, int64_t M, int C, int K, const void* dy, int64_t ldy, const void* w, int64_t ldw, const void* x,
                         const float* mean, const float* rstd, const float* gamma, const float* beta, int act,
                         const float* chan_scale, int64_t rows_per_sample, int eval_mode, void* dx, float* dgamma, float* dbeta,
                         float* ws, const void* x1, int64_t ldx1, int C1, float* dG, float* dwcls, void* stream);
/* segf_bn_cls_bwd_full with the classifier's BIAS gradient riding on pass 1 too: dbcls fp32 [K] = column sums of dy, added up from
 * the dy tiles the workgroups of the first feature slice stage anyway (fixed order: deterministic; a different order than
 * segf_colsum's, so dbcls differs from it in round-off).  dwcls and dbcls are both required; every other output has the bits of
 * segf_bn_cls_bwd_full.  _supported: segf_bn_cls_bwd_supported and the policy SEGFAC_HEAD_DB_RIDE (1 = from 131072 rows on).
 * ws >= segf_bn_cls_bwd_full_db_ws(M, C, K, rows_per_sample) floats. */
int segf_bn_cls_bwd_full_db_supported(int dt, int64_t M, int C, int K, int64_t rows_per_sample);
int64_t segf_bn_cls_bwd_full_db_ws(int64_t M, int C, int K, int64_t rows_per_sample);
int segf_bn_cls_bwd_full_db(int dt, int64_t M, int C, int K, const void* dy, int64_t ldy, const void* w, int64_t ldw, const void* x,
                            const float* mean, const float* rstd, const float* gamma, const float* beta, int act,
                            const float* chan_scale, int64_t rows_per_sample, int eval_mode, void* dx, float* dgamma, float* dbeta,
                            float* ws, const void* x1, int64_t ldx1, int C1, float* dG, float* dwcls, float* dbcls, void* stream);

/* ---- Global Response Normalization (ConvNeXtV2 GRN, convnextv2.py:68-80) on NHWC rows, B images of rows_per_sample rows:
 * y = gamma * (x * Nx) + beta + x, Nx = ||x||_2(H,W) / (mean_c ||x||_2 + 1e-6).  sumsq_out [B][C] is saved for the backward.
 * pre_gelu != 0: the input of the normalisation is gelu(x) of the stored tensor (nn.GELU between pwconv1 and grn, convnextv2.py:92-94):
 * the activation is applied on the way in and the backward returns the gradient of the PRE-activation, dx = dGRN * gelu'(x) -- gelu(x)
 * is never written or read. */
int64_t segf_grn_ws(int B, int64_t rows_per_sample, int C, int bwd);
int segf_grn_fwd(int dt, int B, int64_t rows_per_sample, int C, const void* x, const float* gamma, const float* beta, void* y,
                 float* a_scratch, float* sumsq_out, float* ws, int pre_gelu, void* stream);
int segf_grn_bwd(int dt, int B, int64_t rows_per_sample, int C, const void* x, const void* dy, const float* gamma,
                 const float* sumsq_saved, void* dx, float* dgamma, float* dbeta, float* ws, int pre_gelu, void* stream);

/* ---- MiT spatial-reduction attention core (mit.py:52-57): O = softmax(Q K^T * scale) V -----------
 * q: [B*N][ldq] with head h at columns h*hd; k, v likewise over B*Nkv rows; o: [B*N][ldo]; lse: [B][heads][N] */
int segf_attention_fwd(int dt, int B, int heads, int N, int Nkv, int hd, const void* q, int64_t ldq,
                       const void* k, int64_t ldk, const void* v, int64_t ldv, float scale,
                       void* o, int64_t ldo, float* lse, void* stream);
int64_t segf_attention_bwd_ws(int B, int heads, int N, int Nkv, int hd);
int segf_attention_bwd(int dt, int B, int heads, int N, int Nkv, int hd, const void* q, int64_t ldq,
                       const void* k, int64_t ldk, const void* v, int64_t ldv, float scale,
                       const void* o, int64_t ldo, const void* d_o, int64_t lddo, const float* lse,
                       void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
                       float* ws, void* stream);

/* ---- CrossFormer group attention core (crossformer.py:112-167, 258-339; csrc/attention_group.hip) ---------------
 * O_g = softmax(scale Q_g K_g^T + bias[head] + keymask_g) V_g inside groups of G x G tokens of a [B, H, W] map.  Slot (gi, gj) of group
 * (rh, rw, ih, iw) is the token at padded coordinates r = (rh G + gi) I + ih, c = (rw G + gj) I + iw, with I = interval when lda != 0 (LDA:
 * tokens sampled at the interval) and I = 1 otherwise (SDA: adjacent tokens; interval is ignored).  Tokens with r >= H or c >= W are the
 * reference's padding: skipped as keys, not computed as queries; groups without a real token are not launched.  G is the side the block
 * actually uses (the caller applies the reference's small-map rule).
 * qkv: [B H W][ldqkv], head h of q at columns h hd, of k at heads hd + h hd, of v at 2 heads hd + h hd (16-byte aligned rows);
 * bias: [heads][G G][G G] fp32; o: [B H W][ldo] (16-byte aligned rows, as dqkv); lse: [heads][B H W] fp32 (log-sum-exp of every real query row, kept for the backward).
 * hd = 32 and G G <= 64 only: anything else returns SEGF_ERR_SHAPE before any launch (segf_group_attention_supported answers 0).
 * Backward: dqkv [B H W][lddqkv] receives dq | dk | dv of every real token (plain stores: each token is in exactly one group);
 * dbias [heads][G G][G G] fp32 = dS summed over batch and groups, reduced in a fixed order through ws (segf_group_attention_bwd_ws floats):
 * no floating-point atomics, two runs give the same bits. */
int segf_group_attention_supported(int dt, int B, int H, int W, int heads, int hd, int G, int interval, int lda);
int segf_group_attention_fwd(int dt, int B, int H, int W, int heads, int hd, int G, int interval, int lda, const void* qkv,
                             int64_t ldqkv, const float* bias, float scale, void* o, int64_t ldo, float* lse, void* stream);
int64_t segf_group_attention_bwd_ws(int B, int H, int W, int heads, int hd, int G, int interval, int lda);
int segf_group_attention_bwd(int dt, int B, int H, int W, int heads, int hd, int G, int interval, int lda, const void* qkv,
                             int64_t ldqkv, const float* bias, float scale, const void* d_o, int64_t lddo, const float* lse,
                             void* dqkv, int64_t lddqkv, float* dbias, float* ws, void* stream);

/* ---- CAS-ViT additive token mixer (casvit.py:68-92, 112-138; csrc/token_mixer.hip): three streaming kernel pairs on token tensors
 * [M = B HW][C] of B samples with HW pixels each, in the storage dtype; gates, reductions and their results are fp32.
 * Rules common to all of them (anything else returns SEGF_ERR_SHAPE before any launch, and the *_supported queries answer 0):
 * 0 < B <= 65535, HW > 0; C % 8 == 0 and 8 <= C <= 1024; B HW < 2^31 / 4; every leading dimension (elements between rows) >= C with 16-byte aligned
 * rows (ld % 8 == 0 for bf16, ld % 4 == 0 for fp32, base pointers 16-byte aligned), so an operand may be a column slice of a wider
 * buffer such as the [M][3 C] qkv product; columns outside the slice are neither read nor written.  The *_supported queries take the
 * SMALLEST alignment-relevant leading dimension the caller will pass.  Sums over pixels / rows are per-workgroup partial sums in the
 * caller's workspace (the *_ws queries give its size in floats) added in a fixed order: no floating-point atomics, two runs give the
 * same bits.  Nothing is allocated.
 *
 * spatial gate (SpatialOperation's tail + the pooled sum of ChannelOperation): r [M][C] (contiguous) is the BatchNorm + ReLU output,
 * w [C] fp32 the 1 x 1 convolution to one channel:  s[m] = sigmoid(sum_c r[m][c] w[c]) (fp32 [M]),  y = x * s (ldy),
 * pool[b][c] = sum over the pixels of sample b of the UNROUNDED fp32 product x * s (fp32 [B][C]; the caller divides by HW).
 * Backward: g = dy + dpool[b] (dpool fp32 [B][C], may be null);  dx = g * s (lddx);  ds = sum_c g * x;  dl = ds s (1 - s);
 * dr = dl * w ([M][C] contiguous);  dw[c] = sum_m dl[m] r[m][c] (fp32). */
int segf_spatial_gate_supported(int dt, int B, int HW, int C, int64_t ld);
int64_t segf_spatial_gate_fwd_ws(int B, int HW, int C);
int segf_spatial_gate_fwd(int dt, int B, int HW, int C, const void* x, int64_t ldx, const void* r, const float* w, float* s, void* y,
                          int64_t ldy, float* pool, float* ws, void* stream);
int64_t segf_spatial_gate_bwd_ws(int B, int HW, int C);
int segf_spatial_gate_bwd(int dt, int B, int HW, int C, const void* dy, int64_t lddy, const float* dpool, const void* x, int64_t ldx,
                          const void* r, const float* s, const float* w, void* dx, int64_t lddx, void* dr, float* dw, float* ws,
                          void* stream);
/* channel gate mix (ChannelOperation of q and of k, and their sum):  u = q1 * gq[b] + k1 * gk[b], gq / gk fp32 [B][C].
 * Backward: dq1 = du * gq[b], dk1 = du * gk[b], dgq[b][c] = sum over the pixels of sample b of du * q1, dgk likewise with k1 (fp32 [B][C]). */
int segf_channel_gate_mix_supported(int dt, int B, int HW, int C, int64_t ld);
int segf_channel_gate_mix_fwd(int dt, int B, int HW, int C, const void* q1, int64_t ldq, const void* k1, int64_t ldk, const float* gq,
                              const float* gk, void* u, int64_t ldu, void* stream);
int64_t segf_channel_gate_mix_bwd_ws(int B, int HW, int C);
int segf_channel_gate_mix_bwd(int dt, int B, int HW, int C, const void* du, int64_t lddu, const void* q1, int64_t ldq, const void* k1,
                              int64_t ldk, const float* gq, const float* gk, void* dq1, int64_t lddq, void* dk1, int64_t lddk, float* dgq,
                              float* dgk, float* ws, void* stream);
/* gated product:  z = a * v;  backward da = dz * v, dv = dz * a.  M rows (M < 2^31 / 4). */
int segf_gated_mul_supported(int dt, int M, int C, int64_t ld);
int segf_gated_mul_fwd(int dt, int M, int C, const void* a, int64_t lda, const void* v, int64_t ldv, void* z, int64_t ldz, void* stream);
int segf_gated_mul_bwd(int dt, int M, int C, const void* dz, int64_t lddz, const void* a, int64_t lda, const void* v, int64_t ldv,
                       void* da, int64_t ldda, void* dv, int64_t lddv, void* stream);

/* ---- MetaFormer / ConvFormer (metaformer.py:198-241, 489-513; csrc/metaformer.hip): StarReLU and the residual scale, four streaming
 * passes over token tensors [rows][cols] in the storage dtype with fp32 arithmetic, each result rounded once.
 * Rules common to all of them (anything else returns SEGF_ERR_SHAPE before any launch, and the *_supported queries answer 0): rows > 0;
 * cols % 8 == 0, 8 <= cols <= 8192 (StarReLU) or 2048 (residual scale); every leading dimension (elements between rows) >= cols with 16-byte
 * aligned rows (ld % 8 == 0 for bf16, ld % 4 == 0 for fp32, base pointers 16-byte aligned) and rows * ld < 2^31, so an operand may be a
 * column slice of a wider buffer; columns outside the slice are neither read nor written.  The *_supported queries answer for ONE leading dimension
 * (ask once per operand).  *_blocks: workgroups of the launch = partial sums the backward adds.  Sums are
 * per-workgroup partial sums in the caller's workspace (the *_ws queries: floats) added in a fixed order: no floating-point atomics, two
 * runs give the same bits.  Nothing is allocated.
 *
 * StarReLU:  y = s * max(u, 0)^2 + b.  s and b are DEVICE pointers to one fp32 element each, read by the kernel (no host read, so the call
 * can be captured in a graph).  Backward: du = dy * 2 s max(u, 0);  *ds = sum dy max(u, 0)^2 and *db = sum dy over all rows * cols
 * elements in fp32 (lane -> wave -> workgroup partial -> one workgroup adds the partials); ds and db are independent pointers and may be
 * adjacent floats. */
int segf_starrelu_supported(int dt, int64_t rows, int cols, int64_t ld);
int segf_starrelu_blocks(int64_t rows, int cols);
int segf_starrelu_fwd(int dt, int64_t rows, int cols, const void* u, int64_t ldu, const float* s, const float* b, void* y, int64_t ldy,
                      void* stream);
int64_t segf_starrelu_bwd_ws(int64_t rows, int cols);
int segf_starrelu_bwd(int dt, int64_t rows, int cols, const void* u, int64_t ldu, const void* dy, int64_t lddy, const float* s, void* du,
                      int64_t lddu, float* ds, float* db, float* ws, void* stream);
/* residual scale (Scale on the skip path, stages 3 and 4):  y = x * scale[c], scale fp32 [C], 16-byte aligned.
 * Backward: dx = dy * scale[c];  dscale[c] = sum_rows dy * x (fp32 [C]; ws 16-byte aligned). */
int segf_colscale_supported(int dt, int64_t rows, int C, int64_t ld);
int segf_colscale_blocks(int64_t rows, int C);
int segf_colscale_fwd(int dt, int64_t rows, int C, const void* x, int64_t ldx, const float* scale, void* y, int64_t ldy, void* stream);
int64_t segf_colscale_bwd_ws(int64_t rows, int C);
int segf_colscale_bwd(int dt, int64_t rows, int C, const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* scale, void* dx,
                      int64_t lddx, float* dscale, float* ws, void* stream);

/* ---- depthwise 3x3 conv + bias + GELU(erf) on NHWC (mit.py:62-71,98-99 DWConv -> F.gelu) ----------- */
int segf_dwconv3x3_gelu_fwd(int dt, int B, int H, int W, int C, const void* x, const float* w /*[C][9]*/,
                            const float* bias, int apply_gelu, void* y, void* stream);
int64_t segf_dwconv3x3_bwd_ws(int B, int H, int W, int C);
/* du = dy * gelu'(conv(x)+b): `du` (same shape as x) is SCRATCH -- written by the three-pass forms, left untouched by the one-launch form of
 * small maps (H W <= 1024 in bf16 / 512 in fp32: the whole backward in LDS); dx = conv^T(du); dw[C][9], db[C] fp32 */
int segf_dwconv3x3_bwd_blocks(int dt, int B, int H, int W, int C);
int segf_dwconv3x3_gelu_bwd(int dt, int B, int H, int W, int C, const void* x, const float* w, const float* bias,
                            int apply_gelu, const void* dy, void* du, void* dx, float* dw, float* db,
                            float* ws, void* stream);
/* Mix-FFN backward (mit.py:98-99: fc2(gelu(dwconv(f)))) without the hidden-width gradient map: dg = dys W2 is formed inside pass A,
 * du = dg * gelu'(conv(f)+b), then dx / dw / db as above (same ws, same deferred finalize with dw == NULL).  Only for maps whose
 * segf_dwconv3x3_gelu_bwd runs the three walk passes (not the one-launch form of small maps, not SEGFAC_DW_NO_WALK): others are refused.
 * bf16 only; C_in = 32 or 64, C_hidden % 64 == 0; dys [B H W][C_in] with row stride ld_dys (elements, % 8 == 0); w2 bf16
 * [C_in][C_hidden] as layout-1 segf_gemm takes it.  Results carry the bits of segf_gemm(layout 1) + segf_dwconv3x3_gelu_bwd.
 * _supported: host arithmetic only; the shape rule, the walk form in use, and SEGFAC_FFN_BWD_FUSED (0 never, 1 by size, 2 always). */
int segf_dwconv3x3_gelu_bwd_fc2_supported(int dt, int B, int H, int W, int C_hidden, int C_in);
int segf_dwconv3x3_gelu_bwd_fc2(int dt, int B, int H, int W, int C_hidden, int C_in, const void* f, const float* w9,
                                const float* bias, const void* dys, int64_t ld_dys, const void* w2, void* du, void* dx,
                                float* dw, float* db, float* ws, void* stream);
/* The same call also takes C_in = 160 and 256 (MiT stages 3 and 4), where the W2 fragments no longer fit in registers: the four waves
 * of a workgroup share one 64-channel slab and read the fragments from an LDS copy (dwconv3x3_walk_fc2_kernel<5>, <8>); same arithmetic
 * per element, same bits.  Whether a step should take it is answered here and not by segf_dwconv3x3_gelu_bwd_fc2_supported, whose
 * answers stay what they were (tests/test_ffn_bwd_fused_cpu.py holds it to 0 at C_in = 160 under every policy value): the same three conditions, with the row bound of policy value 1 chosen per C_in
 * (profiles/ffn_bwd_stage34_ab.jsonl). */
int segf_dwconv3x3_gelu_bwd_fc2_lds_supported(int dt, int B, int H, int W, int C_hidden, int C_in);

/* ---- depthwise 7x7 conv + bias on NHWC (ConvNeXt Block.dwconv, convnext.py:29,39; convnextv2.py:88,101) --------------
 * wt: fp32 [49][C] (the [C][1][7][7] parameter transposed with segf_permute021); C % 8 == 0.                    */
int segf_dwconv7x7_fwd(int dt, int B, int H, int W, int C, const void* x, const float* wt, const float* bias, void* y,
                       void* stream);
int64_t segf_dwconv7x7_bwd_ws(int B, int H, int W, int C);
/* dx = conv^T(dy) (skipped when dx == NULL); dw fp32 [C][49]; db fp32 [C] (nullable) */
int segf_dwconv7x7_bwd(int dt, int B, int H, int W, int C, const void* x, const float* wt, const void* dy, void* dx,
                       float* dw, float* db, float* ws, void* stream);

/* ---- 3x3 conv, stride 1, pad 1, NHWC, as an implicit MFMA GEMM (no im2col buffer): ConvModule(.., 3, 1, 1) of
 * heads/upernet.py:26,28, modules/ppm.py:19, heads/fpn.py:19.  bf16 only; P = B*H*W pixels.
 *   mode 0: y[P][ldy]  = conv(x[P][ldx], w[Cout][9*Cin])            (+ bias[Cout], nullable)
 *   mode 1: y = dx[P][ldy] = conv^T: x := dy[P][ldx], w := wt[Cin][9*Cout] (weights transposed to [ci][tap][co])
 *   mode 2: y = dw fp32 [Cout][9*Cin] (ldy): x[P][ldx], w := dy[P][ldw]; split_k slices P, ws >= split_k*Cout*9*Cin floats */
/* Modes 0 / 1 with FEW output tiles over a long reduction (PPM bottleneck 3840 -> 768 on 16 x 16, ppm.py:19; the 40 x 40 / 20 x 20 levels):
 * segf_conv3x3_fwd_splitk > 1 = run with that split_k and ws of split_k * P * N floats (bf16 output, no bias): K slices of the eight-phase
 * tile, fp32 partials, one reduce pass.  Any other split_k for modes 0 / 1 is ignored. */
int segf_conv3x3_fwd_splitk(int mode, int B, int H, int W, int Cin, int Cout);
/* split-K count for mode 2 of segf_conv3x3 (size ws with it): segf_gemm_pick_splitk for the shapes that take the generic rule, a few slices
 * of the eight-phase tile for large outputs over short reductions (the FPN levels of UPerHead, upernet.py:26-28) */
int segf_conv3x3_pick_splitk(int Cin, int Cout, int64_t P);
int segf_conv3x3(int mode, int B, int H, int W, int Cin, int Cout, const void* x, int64_t ldx, const void* w, int64_t ldw,
                 void* y, int y_dt, int64_t ldy, const float* bias, int split_k, float* ws, void* stream);

/* ---- 3x3 conv with DILATION, stride 1, padding = dilation, no bias, NHWC, as an implicit MFMA GEMM without an im2col buffer
 * (csrc/conv_dilated.hip): _ASPPConv of DeepLabV3's ASPP, heads/deeplabv3.py:65-75 (rates 12 / 24 / 36, :51,105-108).  dt = SEGF_BF16
 * (v_mfma_f32_16x16x32_bf16) or SEGF_F32 (the f32-input matrix instruction: an exact fp32 fma chain); Cin, Cout multiples of 8;
 * P = B*H*W pixels; x and y may be column slices of wider buffers (ldx, ldy).  off(tap) = ((ty - 1) * dilation, (tx - 1) * dilation).
 *   mode 0: y[P][ldy] (dt)  = sum_{tap, ci} x[p + off(tap)][ci] * w[co][tap * Cin + ci]                     w [Cout][9*Cin] (ldw)
 *   mode 1: y = dx[P][ldy] (dt): x := dy[P][ldx], w := wt[Cin][9*Cout] ([ci][tap][co]), the tap offsets negated
 *   mode 2: y = dw fp32 [Cout][9*Cin] (ldy): x[P][ldx], w := dy[P][ldw]; the pixels are split into split_k slices
 *           (segf_conv3x3_dil_pick_splitk) with ws >= split_k * Cout * 9 * Cin floats when split_k > 1, summed by a reduce pass
 * Only the taps that can touch the map are walked (|ty - 1| * dilation < H and |tx - 1| * dilation < W: segf_conv3x3_dil_live_taps; at
 * 16 x 16 the rates 24 and 36 are the centre tap alone), and a workgroup skips a live tap none of its pixels reaches.  The weight
 * gradient of a dead tap is written as zeros.  SEGFAC_DILCONV_NO_CULL walks all nine taps.  Shapes whose element offsets do not fit
 * 32 bits return SEGF_ERR_SHAPE. */
int segf_conv3x3_dil_live_taps(int H, int W, int dilation, int* taps /*[9]: ty * 3 + tx*/);
int segf_conv3x3_dil_supported(int dt, int mode, int B, int H, int W, int Cin, int Cout, int dilation);
int segf_conv3x3_dil_pick_splitk(int B, int H, int W, int Cin, int Cout, int dilation);
int segf_conv3x3_dil(int dt, int mode, int B, int H, int W, int Cin, int Cout, int dilation, const void* x, int64_t ldx,
                     const void* w, int64_t ldw, void* y, int64_t ldy, int split_k, float* ws, void* stream);

/* y = gelu_erf(u) (mode 0) or dy * gelu_erf'(u) (mode 1), flat, n % 8 == 0 (nn.GELU, convnext.py:32,43) */
int segf_gelu(int dt, int mode, const void* u, const void* dy, void* y, int64_t n, void* stream);
/* out[r] = sum_c a[r][c] b[r][c] (+ extra_a[r] extra_b[r]), fp32: d gamma of a layer scale folded into the weights */
int segf_rowdot(const float* a, int64_t lda, const float* b, int64_t ldb, const float* extra_a, const float* extra_b,
                float* out, int64_t rows, int64_t cols, void* stream);
/* nn.AdaptiveAvgPool2d(S) on NHWC (modules/ppm.py:13): bwd=0 in[B][H][W][C] -> out[B][S][S][C]; bwd=1 the transpose */
int segf_adaptive_avgpool(int dt, int bwd, int B, int H, int W, int C, int S, const void* in, void* out, void* stream);

/* ---- im2col / col2im for strided convs (PatchEmbed mit.py:105,127; sr conv mit.py:21,48) ---------
 * col[(b,oy,ox)][(ky,kx,ci)] with leading dim ldcol (>= kh*kw*Cin, pad columns are zeroed).
 * in_nchw_f32=1: input is the fp32 NCHW image (train_gpu.py tensor contract); else NHWC of dtype dt. */
int segf_im2col(int dt, int in_nchw_f32, int B, int H, int W, int Cin, int kh, int kw, int stride, int pad,
                int Ho, int Wo, const void* x, void* col, int64_t ldcol, void* stream);
int segf_col2im(int dt, int B, int H, int W, int Cin, int kh, int kw, int stride, int pad,
                int Ho, int Wo, const void* dcol, int64_t ldcol, void* dx, void* stream);

/* ---- bilinear resize on NHWC (F.interpolate mode='bilinear'; heads/segformer.py:48, ppm.py:24,
 * upernet.py:41,46, build_models.py:65); out may be a channel slice of a wider buffer (ldo) ---------- */
int segf_bilinear_fwd(int dt, int B, int h, int w, int C, const void* in, int64_t ldi,
                      int H, int W, void* out, int64_t ldo, int align_corners, void* stream);
int segf_bilinear_bwd(int dt, int B, int h, int w, int C, void* din, int64_t ldi,
                      int H, int W, const void* dout, int64_t ldo, int align_corners, void* stream);
/* The transposes of the x2 / x4 / x8 bilinear upsamplings (align_corners = 0) of ONE gradient map in one pass over it: the
 * backward of the folded SegFormerHead's accumulation step (segf_upsample_add with sources at 1/2, 1/4, 1/8 of the grid,
 * heads/segformer.py:44-56).  dout [B][H][W][ldo >= C] -> d2 [B][H/2][W/2][C], d4 [B][H/4][W/4][C], d8 [B][H/8][W/8][C];
 * H % 8 == 0, W % 8 == 0, C % 8 == 0.  Same values as three segf_bilinear_bwd calls. */
int segf_bilinear_bwd_248(int dt, int B, int H, int W, int C, const void* dout, int64_t ldo, void* d2, void* d4, void* d8,
                          void* stream);
/* out = base + sum_{k<nsrc} bilinear_up(src_k), all NHWC of dtype dt, C % 8 == 0: the accumulation step of the folded
 * SegFormerHead (heads/segformer.py:44-56: Linear -> resize -> concat -> 1x1 conv is affine, and bilinear resizing
 * commutes with affine maps, so the per-scale products are formed at native resolution and added here).  nsrc <= 3.  */
int segf_upsample_add(int dt, int B, int H, int W, int C, const void* base, int64_t ldb, int nsrc,
                      const void* src0, int h0, int w0, int64_t ld0, const void* src1, int h1, int w1, int64_t ld1,
                      const void* src2, int h2, int w2, int64_t ld2, void* out, int64_t ldo, int align_corners, void* stream);
/* The same, also returning sums[2][C] = per-channel (sum, sum of squares) of the stored result over all B*H*W rows: the
 * BatchNorm batch statistics of the ConvModule that consumes it (heads/segformer.py:21-29), so no separate pass over the
 * [B*H*W, C] tensor is needed; segf_bn_stats_from_sums turns them into mean / rstd / running statistics.  Fused only for the
 * folded SegFormerHead geometry (three sources at 1/2, 1/4, 1/8 of the grid, align_corners = 0): SEGF_ERR_SHAPE otherwise
 * (use segf_upsample_add + segf_bn_stats).  ws >= segf_upsample_add_stats_ws(B, H, W, C) floats. */
int64_t segf_upsample_add_stats_ws(int B, int H, int W, int C);
int segf_upsample_add_stats(int dt, int B, int H, int W, int C, const void* base, int64_t ldb, int nsrc,
                            const void* src0, int h0, int w0, int64_t ld0, const void* src1, int h1, int w1, int64_t ld1,
                            const void* src2, int h2, int w2, int64_t ld2, void* out, int64_t ldo, int align_corners,
                            float* sums, float* ws, void* stream);
/* The folded SegFormerHead's stride-4 map in one pass on the matrix pipe (heads/segformer.py:42-56 after the fold):
 *   out[b,Y,X,:] = x1[b,Y,X,:] G1^T + bilinear(t2) + bilinear(t3) + bilinear(t4): the stage-1 product (K = C1 = 32 or 64) and the
 *   three align_corners=False resizes of the 1/2, 1/4, 1/8 maps t2, t3, t4 ([B*(H/r)*(W/r)][C] bf16, every bias already added:
 *   bilinear weights sum to one) as ONE accumulated MFMA product per 8 x 8 pixel block -- replaces segf_gemm (x1 G1^T written to
 *   memory) + segf_upsample_add_stats (read back, interpolated on the VALU).  bf16 only; H, W multiples of 8; C a multiple of 128.
 *   sums (nullable): fp32 [2][C] per-channel sum / sum of squares of the fp32 results (BatchNorm statistics of the consumer,
 *   heads/segformer.py:21-29); ws >= segf_fuse_map_248_ws floats when sums is given.  g1: [C][C1] bf16, row stride ldg. */
int segf_fuse_map_248_supported(int dt, int B, int H, int W, int C, int C1);
int64_t segf_fuse_map_248_ws(int B, int H, int W, int C);
int segf_fuse_map_248(int B, int H, int W, int C, int C1, const void* x1, int64_t ldx1, const void* g1, int64_t ldg,
                      const void* t2, int64_t ld2, const void* t3, int64_t ld3, const void* t4, int64_t ld4,
                      void* out, int64_t ldo, float* sums, float* ws, void* stream);
/* (the accuracy of segf_bn_stats: the variance is as accurate as the fp32 sums of x and x^2 it is given allow, so its relative error
 * grows as (mean / sigma)^2) */
int segf_bn_stats_from_sums(const float* sums, int64_t rows, int C, float* mean, float* rstd, float* running_mean,
                            float* running_var, float momentum, float eps, void* stream);
/* Nearest-neighbour resize on dense NHWC (F.interpolate mode='nearest': the top-down step of FPNHead, heads/fpn.py:31,35).
 * bwd=0: out[B][H][W][C] = in[B][src(Y)][src(X)][C] (+ base[B][H][W][C], nullable: the `out + lateral` of fpn.py:34 fused);
 * bwd=1: out[B][h][w][C] = sums of in[B][H][W][C] over the destinations of each source.  Integer ratios: src(Y) = Y / (H / h); any
 * other (h, H) -- inputs that are not multiples of 32 give 3 x 3 -> 5 x 6 and 10 x 12 -> 9 x 12 steps, fpn.py:30-31 -- follows ATen:
 * src(Y) = min((int)floorf(Y * ((float)h / H)), h - 1).  C % 8 == 0. */
int segf_nearest_up(int dt, int bwd, int B, int h, int w, int C, int H, int W, const void* in, const void* base, void* out,
                    void* stream);
/* out (fp32 NCHW [B][C][H][W]) = bilinear(in NHWC [B][h][w][ldi]) -- materialised logits for API parity */
int segf_bilinear_to_nchw_f32(int dt, int B, int h, int w, int C, const void* in, int64_t ldi,
                              int H, int W, float* out, void* stream);

/* ---- fused final-upsample + CrossEntropy + Dice (build_models.py:65 + engine.py:10-15 +
 * util/losses.py:126-177) ------------------------------------------------------------------------
 * logits: NHWC [B][h][w][ldl] (low-res head output; h==H,w==W means "already full-res");
 * target: int64 [B][H][W]; stats (opaque to the caller, segf_ce_dice_stats_floats(B, C) floats): per image
 * {I[C], P[C], T[C], ce_sum, w_sum, n_valid, bad_label_flag}, then the batch totals [4], then block partials;
 * loss: fp32 [3] {total, ce, dice_loss}.  class_weight nullable ([C]).  dice=0 -> CE only.  C <= 192.
 * When H/h == W/w is a power of two the upsample is fused in both directions (no full-resolution tensor).
 * pix_lse (nullable; segf_ce_dice_lse_floats(...) floats, 0 = this configuration has none): scratch that carries the
 * per-pixel log-sum-exp from the forward to the backward of the SAME logits, so the backward does not recompute the softmax
 * normalisation (bf16, ratio-4 fused path only).  Pass the same buffer to both calls, or NULL to both.     */
int64_t segf_ce_dice_stats_floats(int B, int C);
int64_t segf_ce_dice_lse_floats(int dt, int B, int C, int h, int w, int H, int W, const void* logits, int64_t ldl);
int segf_ce_dice_fwd(int dt, int B, int C, int h, int w, int H, int W, const void* logits, int64_t ldl,
                     const int64_t* target, int64_t ignore_index, const float* class_weight, int dice,
                     float* stats, float* loss, float* pix_lse, void* stream);
/* dlogits: NHWC [B][h][w][ldd] of dtype dt = grad_out[0] * d loss / d logits (the LOW-resolution head output; the
 * transposed bilinear resize is applied inside; columns [C, ldd) are zeroed).  ws: segf_ce_dice_bwd_ws floats
 * (0 on the fused power-of-two path; the generic path stages the full-resolution gradient there).
 * Accuracy contract (tests/test_loss_float64.py holds every path to it, against float64):
 *   - a pixel with the ignore index has no term at all: a batch without a valid pixel gives loss = {NaN, NaN, 0} (0 / 0 as
 *     F.cross_entropy; every Dice term is 1) and a gradient of exact zeros on every path, as autograd does;
 *   - bf16, ratio 4: exponentials and the per-pixel coefficients go * (wce - <G, p>) * tap weight are bf16 operands of the scatter,
 *     so a gradient element is accurate to 2^-9 of the sum of the absolute values of its parts, not of its own size.  At the label
 *     class of a confident pixel go * wce * p_t passes through bf16 and meets -go * wce in fp32: the error there is relative to
 *     go * wce, not to p_t - 1;
 *   - bf16, ratios that are no power of two: the staged full-resolution gradient is bf16, each pixel's d loss / d z is rounded
 *     (2^-8 relative) before the transposed resize adds them;
 *   - ratio-4 matrix-pipe kernels, both types: log2(e) rides in the interpolation operand, so a logit in the exp2 domain is rounded
 *     relative to its own size: the CE sum carries 2 * 2^-24 * (|log-sum-exp| + |z_t|) per pixel (logits near +-200: 1e-5 of a
 *     pixel's term), the probabilities and the gradient do not (the stabiliser is subtracted in the accumulator);
 *   - exponentials below 2^-126 of the largest logit of a cell's four taps are zero (the retry flag is raised only when a
 *     pixel's whole sum falls below 1e-30).                                                                  */
int64_t segf_ce_dice_bwd_ws(int dt, int B, int C, int h, int w, int H, int W);
int segf_ce_dice_bwd(int dt, int B, int C, int h, int w, int H, int W, const void* logits, int64_t ldl,
                     const int64_t* target, int64_t ignore_index, const float* class_weight, int dice,
                     const float* stats, const float* grad_out, void* dlogits, int64_t ldd, float* ws,
                     const float* pix_lse, void* stream);

/* ---- per-pixel losses on the fused low-resolution path: OhemCrossEntropy and FocalLoss (util/losses.py:9-66) applied to
 * F.interpolate(logits, (H, W), bilinear, align_corners=False) (build_models.py:65) without forming full-resolution logits or
 * gradients.  Arguments as segf_ce_dice_fwd; C <= 192, B*H*W < 2^31, bf16 and fp32 storage; anything else returns
 * SEGF_ERR_SHAPE before any launch (segf_pixel_loss_supported answers 0).
 * Per pixel ce = w[t] * (logsumexp(z) - z_t) for t != ignore_index, +0.0 for t == ignore_index (w = 1 when class_weight is
 * NULL).  Interpolation, log-sum-exp and ce are fp32 computed from the stored values WHATEVER the storage type, so a bf16 and an
 * fp32 run of the same stored numbers select the same pixels.  ce_map: fp32 [B][H][W], every value >= +0 with the sign bit clear.
 * A label that is neither ignore_index nor in [0, C) is treated as segf_ce_dice_fwd treats it: skipped (ce = 0, not counted as
 * valid, no gradient) and flagged in the state.
 * mode 0, OHEM (p0 = theta = float32(-log(thresh)), 0 < thresh < 1; p1, size_average unused):
 *   n_valid = #(t != ignore), n_min = n_valid / 16, n_hard = #(ce > theta) over all B*H*W pixels, compared in fp32.
 *   n_hard >= n_min: selection {ce > theta}, n_sel = n_hard, loss = mean of the selection.
 *   otherwise (used_topk): the n_min largest of ALL pixels; kappa = the n_min-th largest value, n_gt = #(ce > kappa),
 *   n_eq = #(ce == kappa), n_sel = n_min, loss = (sum_{ce > kappa} ce + (n_min - n_gt) kappa) / n_min.
 *   n_sel == 0 (all labels ignored, or fewer than 16 valid pixels and none hard): loss = NaN, gradient exact zeros, as the reference.
 *   Gradient coefficient of a pixel: grad_out / n_sel above the decision value (theta or kappa), 0 below.  Ties at kappa: torch.topk
 *   keeps arbitrary members; here EVERY pixel with ce == kappa gets grad_out (n_min - n_gt) / (n_eq n_min).  The loss is the
 *   reference's; the gradient is a deterministic member of the reference's possible ones.  An ignored pixel never has a gradient.
 *   The branch is decided on the device (no host synchronisation); the launch sequence is the same on every call, so a captured
 *   graph replays whichever branch the data takes.
 * mode 1, focal (p0 = alpha, p1 = gamma >= 0; no class weights in the reference class, class_weight is honoured if given):
 *   pt = exp(-ce), f = alpha (1 - pt)^gamma ce, loss = sum f / (B H W) (ignored pixels count in the divisor, as .mean() does) or
 *   sum f when size_average == 0.  Coefficient: grad_out alpha [(1 - pt)^gamma + gamma (1 - pt)^(gamma-1) pt ce] / N; the second
 *   term is 0 when gamma == 0 or ce == 0.
 * state: segf_pixel_loss_state_words(B) 32-bit words; the first eight are readable by the caller:
 *   int32 {n_valid, n_min, n_hard, n_gt, n_eq, used_topk}, fp32 kappa (the decision value: theta in the threshold branch), int32
 *   bad_label_flag; the rest is scratch (histograms, partial sums).  In mode 1 only n_valid and the flag are meaningful.
 * loss: fp32 [1].  No floating-point atomics: float sums are per-workgroup partials added in float64 in a fixed order, counts are
 * integer atomics; two runs on the same inputs give the same bits in loss, ce_map, state and dlogits.
 * Backward: takes the forward's ce_map and state (the side of the decision value is read from the saved map, not recomputed);
 * dlogits NHWC [B][h][w][ldd] of dtype dt = sum over pixels of coef w[t] (softmax(z) - onehot_t) through the transposed resize,
 * columns [C, ldd) zeroed (ldd <= 64 ceil(C / 64)).  ws: segf_pixel_loss_bwd_ws floats (0 when H/h == W/w is a power of two
 * <= 8; other ratios stage the full-resolution gradient there and use segf_bilinear_bwd).                              */
int segf_pixel_loss_supported(int dt, int mode, int B, int C, int h, int w, int H, int W);
int64_t segf_pixel_loss_state_words(int B);
int64_t segf_pixel_loss_bwd_ws(int dt, int B, int C, int h, int w, int H, int W);
int segf_pixel_loss_fwd(int dt, int mode, int B, int C, int h, int w, int H, int W, const void* logits, int64_t ldl,
                        const int64_t* target, int64_t ignore_index, const float* class_weight, float p0, float p1,
                        int size_average, float* ce_map, int32_t* state, float* loss, void* stream);
int segf_pixel_loss_bwd(int dt, int mode, int B, int C, int h, int w, int H, int W, const void* logits, int64_t ldl,
                        const int64_t* target, int64_t ignore_index, const float* class_weight, float p0, float p1,
                        int size_average, const float* ce_map, const int32_t* state, const float* grad_out, void* dlogits,
                        int64_t ldd, float* ws, void* stream);

/* test hook: out[16] = column sums of in[64][16] through the loss kernels' transposing wave reduction */
int segf_debug_wave_reduce16(const float* in, float* out, void* stream);

/* ---- fused upsample + argmax + confusion matrix (engine.py:89-91; util/utils.py:99-109;
 * util/metrics.py:24-27).  mat: int64 [n][n] += counts where 0<=t<n; hist: int64 [n][n] += counts
 * where t != ignore_label (t>=n and != ignore is skipped and flagged in flag[0]).                  */
int segf_argmax_confmat(int dt, int B, int C, int h, int w, int H, int W, const void* logits, int64_t ldl,
                        const int64_t* target, int64_t ignore_label, int64_t* mat, int64_t* hist,
                        int32_t* flag, int64_t* pred_out /*nullable [B][H][W]*/, void* stream);

/* ---- multi-scale + flip (MSF) evaluation: resample + softmax + sum over n low-resolution maps, arg max of the sum and both
 * confusion matrices in one kernel (csrc/eval_msf.hip).  The published mIoU protocol: the model runs on the image at several
 * scales, each also horizontally mirrored; every output is resized to the label size (H, W), softmaxed over the classes, the
 * probability maps are summed and the arg max of the sum is scored.  No full-resolution map exists here.
 * Map k: NHWC [B][h_k][w_k][ldl_k >= C] of dtype dt (all maps one dtype), device pointer logits[k]; hw[2k], hw[2k+1] = h_k, w_k;
 * flip[k] != 0: the map is the model's output for the MIRRORED image.  logits / hw / ldl / flip are HOST arrays of n entries, n <=
 * SEGF_MSF_MAX_MAPS: the library copies them into a by-value kernel argument of SEGF_MSF_MAX_MAPS entries -- no device table, no
 * upload, no host synchronisation (the call can be captured into a hipGraph; the host arrays may be freed on return).
 * For every output pixel (b, Y, X):
 *   resample   z_k[c] = bilinear sample of map k at (Y, X): source rows / columns / lambdas of F.interpolate(mode='bilinear',
 *              align_corners=False) at ANY ratio (h_k > H too: downsampling without antialiasing, as F.interpolate does), four taps
 *              combined in ATen's operation order -- the arithmetic of segf_argmax_confmat's generic path.  h_k == H and w_k == W: the
 *              row is read directly.  Flip rule: for flip[k] != 0 the tap columns x0, x1 are read at w_k-1-x0, w_k-1-x1 with the same
 *              weights (exactly the sample of the un-mirrored map; no mirrored copy is made).
 *   softmax    p_k = softmax_c(z_k), fp32, max-subtracted.
 *   sum        S[c] = p_0[c] + p_1[c] + ... + p_(n-1)[c], added in map order (summation order = the order of the arrays): two runs
 *              give the same bits; a permutation of the maps may change the last bits.
 *   arg max    pred = the lowest class index attaining max_c S[c] (0 on an all-NaN row).
 *   count      as segf_argmax_confmat: mat += 1 at [t][pred] where 0 <= t < C; hist the same except t == ignore_label; a label outside
 *              [0, C) that is not ignore_label sets flag[0] bit 0 and is counted nowhere.  target == NULL: no counting (inference).
 * pred_out (nullable): int64 [B][H][W].  prob_out (nullable): fp32 [B*H*W][ldp >= C], the sums S (NOT divided by n).
 * SEGF_ERR_SHAPE before any launch: n < 1 or n > SEGF_MSF_MAX_MAPS, C < 1 or C > 192, B < 1 or B > 65535, any h_k, w_k, H, W < 1,
 * ldl_k < C, prob_out given with ldp < C.  segf_msf_supported: 1 when the shape part of that (and dt) is acceptable, else 0.
 * Cost: reads every tap row it needs (4 per map and pixel, served from cache: a low-resolution row feeds many pixels), the labels
 * once, and writes the counts; measured figures in profiles/msf_eval.md.  No floating-point atomics.                      */
#define SEGF_MSF_MAX_MAPS 16
int segf_msf_supported(int dt, int B, int C, int n, const int* hw /*HOST [n][2]*/, int H, int W);
int segf_msf_argmax_confmat(int dt, int B, int C, int n,
                            void** logits       /*HOST array of n device pointers*/,
                            const int* hw       /*HOST [n][2] = h_k, w_k*/,
                            const int64_t* ldl  /*HOST [n]*/,
                            const int* flip     /*HOST [n]*/,
                            int H, int W, const int64_t* target, int64_t ignore_label,
                            int64_t* mat, int64_t* hist, int32_t* flag,
                            int64_t* pred_out /*nullable*/, float* prob_out /*nullable*/, int64_t ldp, void* stream);

/* ---- sliding-window evaluation: resample + mean over the low-resolution maps of overlapping crops, arg max of the mean and both
 * confusion matrices in one kernel (csrc/eval_slide.hip).  The other published protocol (mmseg's slide_inference): the model runs on
 * overlapping ch x cw crops of the image, every crop's logits are resized to the crop, the logits of overlapping crops are averaged
 * and the arg max of the mean is scored.  No full-resolution map, accumulator or count map exists here.
 * Grid: ny = max(H - ch + sh - 1, 0) / sh + 1 windows down and nx = max(W - cw + sw - 1, 0) / sw + 1 across (integer division);
 * window (i, j) has origin y_i = min(i sh, H - ch), x_j = min(j sw, W - cw): the last window of an axis is shifted back so that it
 * ends at the border, two windows never coincide, and every window has size exactly ch x cw.  segf_slide_grid writes ny, nx.
 * logits: ONE device buffer [B][ny nx][h][w][ldl >= C] of dtype dt, window index i nx + j: the head outputs of the windows, (h, w)
 * being the head's output size for a ch x cw input.  64-bit indexing throughout.
 * For every output pixel (b, Y, X), over every window that covers it (y_i <= Y < y_i + ch, x_j <= X < x_j + cw), in ascending
 * (i, j) order (i outer, j inner):
 *   resample   z_ij[c] = bilinear sample of the window's map at the local pixel (Y - y_i, X - x_j): source rows / columns / lambdas
 *              of F.interpolate(size=(ch, cw), mode='bilinear', align_corners=False) at ANY ratio (h > ch too), four taps combined in
 *              ATen's operation order -- the arithmetic of segf_argmax_confmat's generic path.  h == ch and w == cw: the row is read
 *              directly.
 *   sum        A[c] = z_ij[c] + ..., fp32, added in window order: the same sequence of additions on every run (same bits).
 *   mean       M[c] = A[c] / n, n = the number of covering windows: a true IEEE fp32 division, not a reciprocal approximation -- a
 *              pixel covered once keeps its sample bit for bit.
 *   arg max    pred = the lowest class index attaining max_c M[c] (0 on an all-NaN row).
 *   count      as segf_argmax_confmat: mat += 1 at [t][pred] where 0 <= t < C; hist the same except t == ignore_label; a label outside
 *              [0, C) that is not ignore_label sets flag[0] bit 0 and is counted nowhere.  target == NULL: no counting (inference).
 * pred_out (nullable): int64 [B][H][W].  mean_out (nullable): fp32 [B*H*W][ldm >= C], the mean logits M.
 * SEGF_ERR_SHAPE before any launch: C < 1 or C > 192, B < 1 or B > 65535, any of H, W, h, w < 1, 1 <= sh <= ch <= H or
 * 1 <= sw <= cw <= W violated (a stride larger than the crop would leave pixels uncovered), ldl < C, mean_out given with ldm < C,
 * logits NULL; SEGF_ERR_DTYPE for an unknown dt.  segf_slide_supported: 1 when the shape part of that (without the row strides and
 * pointers) and dt are acceptable, else 0.  segf_slide_grid: 0, or SEGF_ERR_SHAPE for a grid refused above (or NULL ny / nx).
 * No device table, no upload, no host synchronisation (the call can be captured into a hipGraph); no floating-point atomics: two runs
 * give the same bits.  Measured figures in profiles/slide_eval.md.                                                       */
int segf_slide_grid(int H, int W, int ch, int cw, int sh, int sw, int* ny, int* nx);
int segf_slide_supported(int dt, int B, int C, int H, int W, int ch, int cw, int sh, int sw, int h, int w);
int segf_slide_argmax_confmat(int dt, int B, int C, int H, int W, int ch, int cw, int sh, int sw, int h, int w,
                              const void* logits, int64_t ldl, const int64_t* target, int64_t ignore_label,
                              int64_t* mat, int64_t* hist, int32_t* flag,
                              int64_t* pred_out /*nullable*/, float* mean_out /*nullable*/, int64_t ldm, void* stream);

/* ---- multi-scale + flip SLIDING-WINDOW evaluation: the two entries above composed in one kernel (csrc/eval_msf_slide.hip).
 * mmseg's aug_test with mode='slide', the protocol behind SegFormer's multi-scale Cityscapes figures: at every scale, straight and
 * horizontally mirrored, the model runs on overlapping crops of the SCALED image; the logits of overlapping crops are averaged, the
 * mean map is resized to the label size (H, W) and softmaxed, the probability maps of all (scale, flip) pairs are summed and the arg
 * max of the sum is scored.  No full-resolution map, at the label size or at a scaled size, exists here.
 * n <= SEGF_MSF_MAX_MAPS window sets of one dtype dt.  Set k belongs to one (scale, flip) pair: geom[8k .. 8k+7] = Hs_k, Ws_k (the
 * scaled image size), ch_k, cw_k (the effective crop), sh_k, sw_k (the effective stride; both already clamped, 1 <= stride <= crop <=
 * scaled size per axis), h_k, w_k (the size of ONE window's low-resolution map); flip[k] != 0: the set holds the model's outputs
 * for the windows of the MIRRORED scaled image.  The grid of set k is segf_slide_grid(Hs_k, Ws_k, ch_k, cw_k, sh_k, sw_k) -> ny_k,
 * nx_k; logits[k]: ONE device buffer [B][ny_k nx_k][h_k][w_k][ldl_k >= C], image-major, then window order -- exactly the layout
 * segf_slide_argmax_confmat reads.  logits / geom / ldl / flip are HOST arrays of n entries: the library copies them into a by-value
 * kernel argument of SEGF_MSF_MAX_MAPS entries -- no device table, no upload, no host synchronisation (the call can be captured into
 * a hipGraph; the host arrays may be freed on return).  64-bit indexing throughout.
 * For every output pixel (b, Y, X), for every set k in list order:
 *   outer taps (Hs_k, Ws_k) == (H, W): the single scaled pixel (Y, X).  Otherwise the source rows / columns / lambdas y0, y1, ly and
 *              x0, x1, lx of F.interpolate(size=(H, W), mode='bilinear', align_corners=False) from (Hs_k, Ws_k) at ANY ratio (Hs_k > H
 *              too: downsampling without antialiasing).  Flip rule: for flip[k] != 0 the tap columns are read at Ws_k-1-x0, Ws_k-1-x1
 *              (same size: at Ws_k-1-X) with the same weights -- exactly the sample of the un-mirrored mean map; no mirrored copy is
 *              made.
 *   window mean at each tap (ys, xs), the arithmetic of segf_slide_argmax_confmat on the scaled image: over every window of set k
 *              that covers (ys, xs), in ascending (i, j) order, the bilinear sample of that window's map at the local pixel (four taps
 *              in ATen's operation order; h_k == ch_k and w_k == cw_k: the row is read directly), summed in fp32 in window order and
 *              divided by the cover count with a true IEEE fp32 division.
 *   logit      z_k[c] = the four means M00, M01, M10, M11 combined with ly, lx in ATen's operation order, fma(M11, w11, fma(M10, w10,
 *              fma(M00, w00, M01 w01))); same size: the one mean itself.
 *   softmax    p_k = softmax_c(z_k), fp32, max-subtracted.
 *   sum        S[c] = p_0[c] + p_1[c] + ... + p_(n-1)[c], added in set order (summation order = the order of the arrays): two runs
 *              give the same bits; a permutation of the sets may change the last bits.
 * After the last set:
 *   arg max    pred = the lowest class index attaining max_c S[c] (0 on an all-NaN row).
 *   count      as segf_argmax_confmat: mat += 1 at [t][pred] where 0 <= t < C; hist the same except t == ignore_label; a label outside
 *              [0, C) that is not ignore_label sets flag[0] bit 0 and is counted nowhere.  target == NULL: no counting (inference).
 *              A pixel counted nowhere is skipped when neither output below is wanted.
 * pred_out (nullable): int64 [B][H][W].  prob_out (nullable): fp32 [B*H*W][ldp >= C], the sums S (NOT divided by n).
 * SEGF_ERR_SHAPE before any launch: n < 1 or n > SEGF_MSF_MAX_MAPS, C < 1 or C > 192, B < 1 or B > 65535, H or W < 1, any set with
 * 1 <= sh_k <= ch_k <= Hs_k or 1 <= sw_k <= cw_k <= Ws_k violated or h_k, w_k < 1, ldl_k < C, prob_out given with ldp < C, a NULL
 * array or a NULL logits[k]; SEGF_ERR_DTYPE for an unknown dt.  segf_msf_slide_supported: 1 when the shape part of that (without the
 * row strides and pointers) and dt are acceptable, else 0.
 * Cost: up to four window means per set and pixel, each up to four tap rows per covering window, served from cache; the labels once;
 * the counts.  No floating-point atomics.  Measured figures in profiles/msf_slide_eval.md.                                  */
int segf_msf_slide_supported(int dt, int B, int C, int n, const int* geom /*HOST [n][8]*/, int H, int W);
int segf_msf_slide_argmax_confmat(int dt, int B, int C, int n,
                                  void** logits       /*HOST array of n device pointers*/,
                                  const int* geom     /*HOST [n][8] = Hs, Ws, ch, cw, sh, sw, h, w*/,
                                  const int64_t* ldl  /*HOST [n]*/,
                                  const int* flip     /*HOST [n]*/,
                                  int H, int W, const int64_t* target, int64_t ignore_label,
                                  int64_t* mat, int64_t* hist, int32_t* flag,
                                  int64_t* pred_out /*nullable*/, float* prob_out /*nullable*/, int64_t ldp, void* stream);

/* out[r] = argmax_c x[r][c] (lowest index on ties): the prediction step of single-image inference
 * (estimate_model.py:104-106, softmax(dim=1).argmax(dim=1) -- softmax is monotonic).  x: [rows][ld >= C], C <= 192. */
int segf_argmax_rows(int dt, int64_t rows, int C, const void* x, int64_t ld, int64_t* out, void* stream);

/* ConfusionMatrix.update(a, b) on explicit int64 (ground truth, prediction) pairs (util/utils.py:99-109) and
 * the Metrics.update bincount (util/metrics.py:24-27); mat / hist nullable.  flag bit0: label >= n that is not
 * ignore_label, bit1: prediction out of range.                                                      */
int segf_confmat_pairs(const int64_t* gt, const int64_t* pred, int64_t n, int C, int64_t ignore_label,
                       int64_t* mat, int64_t* hist, int32_t* flag, void* stream);

/* ---- optimizer step (engine.py:52-53 -> timm NativeScaler -> AGC clip -> AdamW) over flat fp32
 * param/grad/state buffers.  A "unit" is one dim-0 row of a >=2-D weight or a whole 1-D tensor:
 * unit_offset[u], unit_len[u] (elements), unit_flags[u] bit0 = apply weight decay, bit1 = the parameter got no gradient
 * this step: the unit is skipped entirely, as torch.optim.AdamW skips `p.grad is None` (train_gpu.py:269).  unit_step
 * (nullable): per-unit step counts kept on the device and advanced by the kernel for every unit it updates -- torch's per-parameter
 * state['step'], which sets the bias corrections; when null the host scalar `step` is used for all units.  clip_factor <= 0
 * disables AGC.  See oracle/optim.py for the restated arithmetic (timm 0.9.2; "parity unpinned").   */
int segf_agc_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                   const int64_t* unit_offset, const int32_t* unit_len, const uint8_t* unit_flags, int32_t* unit_step,
                   int nunits, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   float clip_factor, float agc_eps, void* stream);

/* The other --opt values of the reference's CLI (train_gpu.py:93-104: --opt / --opt-eps / --opt-betas / --momentum;
 * train_gpu.py:269: timm.optim.create_optimizer) over the same flat buffers and unit tables as segf_agc_adamw: one launch, every
 * hyper-parameter a launch scalar (no host read, graph-replay safe), unit_flags bit 0 = weight decay applies, bit 1 = no gradient
 * this step (the unit is skipped entirely: no decay, no state update, no step count -- torch.optim's `p.grad is None`), per-unit
 * step counts on the device (nullable except for SEGF_OPT_ADAM, whose bias corrections use the unit's own count).  clip_factor > 0
 * runs the unit-wise AGC pass of segf_agc_adamw first, on the raw gradient; then g <- g + weight_decay * p (L2 coupled into the
 * gradient) where bit 0 is set; then the rule -- the fp32 arithmetic of the torch.optim class named, maximize=False:
 *   SEGF_OPT_SGD      torch.optim.SGD (dampening 0)      h0 = momentum, nesterov;   s0 = momentum_buffer (null when h0 == 0), s1 unused
 *   SEGF_OPT_ADAM     torch.optim.Adam (no amsgrad)      h0 = beta1, h1 = beta2, eps;   s0 = exp_avg, s1 = exp_avg_sq
 *   SEGF_OPT_RMSPROP  torch.optim.RMSprop (not centered) h0 = alpha, h1 = momentum, eps;  s0 = square_avg, s1 = momentum_buffer
 *                                                         (null when h1 == 0)
 * State buffers have the flat layout and start at zero (torch's SGD clones the first gradient into momentum_buffer, which
 * equals momentum * 0 + g).  A null buffer the rule needs, or an unknown rule, returns SEGF_ERR_SHAPE. */
#define SEGF_OPT_SGD 0
#define SEGF_OPT_ADAM 1
#define SEGF_OPT_RMSPROP 2
int segf_flat_optim_step(int rule, float* param, const float* grad, float* s0, float* s1,
                         const int64_t* unit_offset, const int32_t* unit_len, const uint8_t* unit_flags, int32_t* unit_step,
                         int nunits, float lr, float weight_decay, float h0, float h1, float eps, int nesterov,
                         float clip_factor, float agc_eps, void* stream);

/* Per-group learning rate and weight decay (torch.optim parameter groups with their own `lr` / `weight_decay`: a decode head at
 * 10 x the backbone's rate, layer-wise learning-rate decay, differential fine-tuning).  segf_agc_adamw_groups and
 * segf_flat_optim_step_groups are segf_agc_adamw and segf_flat_optim_step -- the same kernel source, the same per-unit step counts,
 * AGC on the raw gradient and per-rule arithmetic -- with the scalars `lr` / `weight_decay` replaced by
 *   unit_group[u]  DEVICE uint8 [nunits]: the parameter group of unit u, < ngroups (a unit whose index is not is left untouched);
 *   group_lr[g], group_wd[g]  HOST float [ngroups], 1 <= ngroups <= SEGF_OPT_MAX_GROUPS: read during the call and copied into a
 *   by-value kernel argument (about 1 KB of kernarg), so the step stays ONE launch with launch scalars only -- no device table is
 *   refreshed per step, no host-to-device copy that a host running ahead could race, and the arrays may be freed on return.
 * Weight decay applies to unit u where group_wd[unit_group[u]] != 0; unit_flags bit 0 is IGNORED in the group forms, bit 1 (no
 * gradient this step) keeps its meaning.  Status codes: SEGF_ERR_SHAPE, before any launch, for ngroups < 1, ngroups >
 * SEGF_OPT_MAX_GROUPS, a null unit_group / group_lr / group_wd, and for whatever the scalar form of the rule refuses (a null buffer
 * the rule needs, an unknown rule, Nesterov without momentum, step < 1 without unit_step); 0 on success (also for nunits <= 0); a
 * positive hipError_t when the launch failed.  Measured against the scalar forms in profiles/optim_groups.md. */
#define SEGF_OPT_MAX_GROUPS 128
int segf_agc_adamw_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                          const int64_t* unit_offset, const int32_t* unit_len, const uint8_t* unit_flags, int32_t* unit_step,
                          int nunits, const uint8_t* unit_group, int ngroups, const float* group_lr, const float* group_wd,
                          float beta1, float beta2, float eps, int step, float clip_factor, float agc_eps, void* stream);
int segf_flat_optim_step_groups(int rule, float* param, const float* grad, float* s0, float* s1,
                                const int64_t* unit_offset, const int32_t* unit_len, const uint8_t* unit_flags, int32_t* unit_step,
                                int nunits, const uint8_t* unit_group, int ngroups, const float* group_lr, const float* group_wd,
                                float h0, float h1, float eps, int nesterov, float clip_factor, float agc_eps, void* stream);

/* The other --clip-mode values of the reference (train_gpu.py:99-102 -> timm.utils.dispatch_clip_grad) on the flat gradient buffer:
 * mode 0 'norm' = torch.nn.utils.clip_grad_norm_(params, value, 2.0): g *= min(1, value / (||g||_2 + 1e-6));
 * mode 1 'value' = clip_grad_value_: g = clamp(g, -value, value).  ws: segf_clip_grad_ws() floats (mode 0).  No host read. */
int64_t segf_clip_grad_ws(void);
int segf_clip_grad(float* grad, int64_t n, int mode, float value, float* ws, void* stream);

/* ---- device-side input pipeline over decoded uint8 images resident in HBM ---------------------------
 * segf_input_train: ExtRandomCrop -> ExtColorJitter -> ExtRandomHorizontalFlip -> ExtToTensor -> ExtNormalize
 * (datasets/build_datasets.py:14-22; datasets/extra_transform.py:319-392, 426-509, 196-214, 259-281, 288-313) and the dataset
 * classes' label table + .long() (datasets/ade.py:122-124, cityscapes.py:159, coco_stuff.py:95-100) for a batch of B samples
 * cropped to H x W.  Pillow's uint8 arithmetic (ImagingBlend, rgb2l, ImageStat mean) bit for bit; the float tail
 * ((u8 / 255) / 255 - mean) / std keeps the reference's second / 255 (quirk Q11).  One segf_input_sample per image: packed RGB
 * rows (img_stride bytes apart) and uint8 label rows; the crop window starts at (top, left) and reads 0 outside the source
 * (Image.crop); `order` lists the jitter steps in application order, 2 bits each (1 brightness, 2 contrast, 3 saturation,
 * 0 end), factor[k] belongs to step k; the random values are drawn by the caller.  lsum_ws: B x uint64 (luma sums for the
 * contrast means); label_lut nullable (int64[256]; identity when null).  out_img fp32 [B][3][H][W], out_lbl int64 [B][H][W]. */
typedef struct {
    const uint8_t* img;
    const uint8_t* lbl;
    int64_t img_stride, lbl_stride;
    int32_t src_h, src_w, top, left;
    int32_t flip, order;
    float factor[3];
    int32_t reserved;
} segf_input_sample;                                                     /* 72 bytes */
int segf_input_train(const segf_input_sample* samples /*device [B]*/, int B, int H, int W, uint64_t* lsum_ws, const float* mean3,
                     const float* std3, const int64_t* label_lut, float* out_img, int64_t* out_lbl, void* stream);
/* segf_input_train_scaled: the training protocol with scale augmentation,
 *   ExtRandomScale((lo, hi)) -> ExtRandomCrop((H, W), pad_if_needed=True) -> ExtColorJitter -> ExtRandomHorizontalFlip -> ExtToTensor
 *   -> ExtNormalize                                                  (datasets/extra_transform.py:75-96, 319-392 and as above)
 * and the label table.  The caller draws the random values and does the size arithmetic (transforms.py `draw_scaled`): the source is
 * resized to res_h x res_w -- Image.resize((res_w, res_h), BILINEAR) = ImagingResample's horizontal then vertical pass in 22-bit
 * fixed point, each rounded and clipped to uint8; the label by Image.resize(..., NEAREST) = ImagingScaleAffine's index accumulated
 * in double from output index 0 -- and the H x W crop window starts at (top, left) IN RESIZED COORDINATES, either of which may be
 * negative (the border F.pad added).  Outside [0, res_h) x [0, res_w) the image reads 0 and the label `label_fill` (a raw uint8
 * value, mapped through label_lut like any other).  Only the window is computed: no resized image and no horizontal-pass image
 * exists; every crop pixel evaluates its vertical taps over horizontal-pass values formed on the fly (at most kmax x kmax source
 * pixels), then the uint8 crops are staged in ws and segf_input_train's own kernels run over them (jitter, contrast mean over the
 * crop with its padding, flip, float tail: the same bits).
 * samples: HOST array [B] -- its values are checked on the host before anything is launched, then copied into ws on `stream`, and the
 * stream is waited for before the kernels are queued, so the array may be reused on return (not capturable into a graph; the image /
 * label pointers inside are device pointers and must outlive the kernels).  kmax >= every sample's tap count 2 * ceil(max(1, src /
 * res)) + 1 on both axes.  ws: segf_input_train_scaled_ws(B, H, W, kmax) BYTES, 16-byte aligned; the size does not depend on any
 * source or resized size.  SEGF_ERR_SHAPE, before any launch, for: a null pointer; out_img / out_lbl / ws not 16-byte aligned;
 * res_h or res_w < 1 (or a source size < 1, a row stride shorter than a row); a sample that needs more than kmax taps; H * W > 2^30;
 * |top| or |left| or a resized size > 2^30. */
typedef struct {
    const uint8_t* img;
    const uint8_t* lbl;
    int64_t img_stride, lbl_stride;
    int32_t src_h, src_w, res_h, res_w;
    int32_t top, left;
    int32_t flip, order;
    float factor[3];
    int32_t label_fill;
} segf_input_scaled_sample;                                              /* 80 bytes */
int64_t segf_input_train_scaled_ws(int B, int H, int W, int kmax);
int segf_input_train_scaled(const segf_input_scaled_sample* samples /*host [B]*/, int B, int H, int W, int kmax, void* ws,
                            const float* mean3, const float* std3, const int64_t* label_lut, float* out_img, int64_t* out_lbl,
                            void* stream);
/* Class-balanced crop choice: mmsegmentation's RandomCrop(crop_size, cat_max_ratio) in front of either training stack.  In words,
 * mmseg's loop is: draw a crop window; if cat_max_ratio < 1, up to ten times: crop the label map to the window, count its values
 * with np.unique(..., return_counts=True), drop the ignore index, and stop if more than one class is left and
 * np.max(cnt) / np.sum(cnt) < cat_max_ratio; otherwise draw another window.  After ten failed tests the window drawn last -- the
 * eleventh -- is used as it comes, without a test.  The random draws stay with the caller (transforms.py); the kernels see K =
 * tries + 1 candidate windows (top_k, left_k), k = 0 .. K-1, per sample, each H x W, and apply THE RULE:
 *   - every window pixel gives its raw uint8 label v exactly as the crop kernels read it.  Unscaled stack: lbl[top + y][left + x],
 *     and raw 0 outside the source (Image.crop).  Scaled stack: Pillow's NEAREST-resized label at resized coordinates (top + y,
 *     left + x) -- the source index is ImagingScaleAffine's, accumulated in double from output index 0, as in segf_input_train_scaled
 *     -- and label_fill outside [0, res_h) x [0, res_w);
 *   - c = label_lut[v] is its class (identity when the table is null); pixels with c == ignore_class are not counted; two raw values
 *     that the table maps to one class are one class;
 *   - with n_c the remaining counts, window k PASSES iff at least two classes have n_c > 0 AND
 *     (double)max_c n_c / (double)sum_c n_c < max_ratio -- strict, in double, like numpy's in mmseg.  A window with no counted pixel
 *     fails, and no division happens;
 *   - chosen[b] = the first passing k among 0 .. K-2; if none passes, K-1, which is used UNTESTED (ten tests, then the eleventh
 *     draw is taken as it comes).  With K == 1 the result is 0 and no label is read.
 * The horizontal flip and the colour jitter come after the crop and play no part.  The choice is made on the device: one workgroup
 * per sample walks the windows in order and stops at the first pass; nothing is read back, nothing is synchronised.  The counts are
 * integers (integer LDS adds only), so two runs give the same bits.  chosen (nullable) is written for every sample.
 *
 * segf_input_crop_select: the unscaled stack.  Rewrites top / left of the DEVICE records in place with the chosen candidate's; an
 * unchanged segf_input_train on the same records follows on the same stream.  cand: DEVICE int32 [B][K][2] = (top, left); they are
 * not read on the host, and like the top / left of segf_input_train they must not be negative.
 * SEGF_ERR_SHAPE, before any launch and with the outputs untouched: K < 1 or K > 32; max_ratio not in (0, 1] or NaN; a null samples /
 * cand; samples not 16-byte aligned or cand not 4-byte aligned; H * W > 2^30.  A candidate with |top| or |left| > 2^30 cannot be
 * refused here, because the candidates are not read on the host: the caller bounds them (transforms.py `pack` does).
 *
 * segf_input_train_scaled_select: segf_input_train_scaled with the choice in front.  samples and cand are HOST arrays, uploaded
 * into ws as segf_input_train_scaled uploads its records (one wait for the stream, both arrays reusable on return); cand holds
 * RESIZED coordinates and may be negative.  The selection kernel runs BEFORE the coefficient-table kernel, because those tables
 * depend on the window; it patches top / left of the uploaded records (the records' own top / left are checked and then replaced),
 * then segf_input_train_scaled's own kernels run.  ws: segf_input_train_scaled_select_ws(B, H, W, kmax, K) BYTES, 16-byte aligned:
 * segf_input_train_scaled_ws plus the candidates; it grows with K and does not depend on any source or resized size.
 * SEGF_ERR_SHAPE as above, for a candidate with |top| or |left| > 2^30, and for whatever segf_input_train_scaled refuses. */
int segf_input_crop_select(segf_input_sample* samples, const int32_t* cand, int B, int K, int H, int W, double max_ratio,
                           const int64_t* label_lut, int64_t ignore_class, int32_t* chosen, void* stream);
int64_t segf_input_train_scaled_select_ws(int B, int H, int W, int kmax, int K);
int segf_input_train_scaled_select(const segf_input_scaled_sample* samples, const int32_t* cand, int K, double max_ratio,
                                   int64_t ignore_class, int32_t* chosen, int B, int H, int W, int kmax, void* ws,
                                   const float* mean3, const float* std3, const int64_t* label_lut, float* out_img,
                                   int64_t* out_lbl, void* stream);
/* segf_input_val: ExtResize -> ExtToTensor -> ExtNormalize (build_datasets.py:24-29; extra_transform.py:395-419) for ONE image:
 * Image.resize((out_w, out_h), BILINEAR) = ImagingResample's horizontal then vertical pass in 22-bit fixed point, each rounded to
 * uint8, and Image.resize(..., NEAREST) for the label (ImagingScaleAffine's accumulated source index); the caller computes
 * (out_h, out_w) (smaller edge -> size, other edge int(size * long / short)).  ws: segf_input_val_ws(...) BYTES, 16-byte aligned.
 * out_img fp32 [3][out_h][out_w], out_lbl int64 [out_h][out_w]. */
/* Single-image inference preprocessing (estimate_model.py:85-97 with torchvision 0.15.2, environment.yml:22): T.Resize((out_h, out_w)) of a
 * uint8 CHW TENSOR = bilinear, align_corners = False, no antialias, computed in float32 and rounded half-to-even back to uint8, then
 * x / 255 and Normalize(mean, std).  img: uint8 [3][src_h][src_w] on the device; out: fp32 [3][out_h][out_w]. */
int segf_infer_preprocess(const uint8_t* img, int src_h, int src_w, int out_h, int out_w, const float* mean3, const float* std3,
                          float* out, void* stream);
int64_t segf_input_val_ws(int src_h, int src_w, int out_h, int out_w);
int segf_input_val(const uint8_t* img, int64_t img_stride, const uint8_t* lbl, int64_t lbl_stride, int src_h, int src_w, int out_h,
                   int out_w, void* ws, const float* mean3, const float* std3, const int64_t* label_lut, float* out_img,
                   int64_t* out_lbl, void* stream);

/* ---- Dispatch policy and launch trace (csrc/policy.h, csrc/policy.hip) -------------------------------------------------------------
 * Every switch that can change WHICH kernel (or which form of a kernel) a call takes lives in one table, csrc/policy.h, and is read
 * from the environment ONCE, at first use, into one struct: nothing on the launch path calls getenv().  A set variable that is not a
 * number counts as 1; "0" equals unset for the on/off switches.  The table (the reference has no counterpart: it dispatches through
 * ATen; models/build_models.py:43-54 is where the BASELINE shapes these rules were measured on come from):
 *
 *   SEGFAC_GEMM_NO_BIG           never take the 256 x 256-tile kernel (gemm_bf16_big_kernel): everything on the 128-tile one
 *   SEGFAC_GEMM_NO_SKINNY        no streaming products for K, N <= 128 (gemm_skinny_kernel and its relatives)
 *   SEGFAC_GEMM_NO_SKINNY_ROWS   the [tokens x 32] -> 768 projection on gemm_skinny_kernel instead of the whole-row form
 *   SEGFAC_GEMM_NO_SKINNY_K      no K-split streaming product for 32- / 64-wide outputs (gemm_skinny_k_kernel)
 *   SEGFAC_GEMM_NO_DW_SKINNY     small-output weight gradients on the tiled split-K kernel instead of gemm_dw_skinny_kernel
 *   SEGFAC_GEMM_NO_NARROW        256-tile kernel: full 128 x 64 wave tiles also for outputs <= 160 wide (bit-identical results)
 *   SEGFAC_GEMM_NO_DEEP          256-tile forward: one K step of operand loads in flight instead of two
 *   SEGFAC_GEMM_NO_DEEP128       128-tile kernel: one K step in flight instead of two
 *   SEGFAC_GEMM_NO_FASTLOAD      guarded tile loads everywhere (no workgroup-uniform guard-free full-K-step loads)
 *   SEGFAC_GEMM_NO_TR            debugging: reduction-major fragments by scalar LDS reads instead of ds_read_b64_tr_b16; disables every kernel built on the transposed read
 *   SEGFAC_GEMM_NO_PRO           segf_gemm_pro_supported answers 0: BatchNorm + ReLU + Dropout2d are applied by their own pass
 *   SEGFAC_GEMM_NO_FUSED_DB      bias gradient as its own column-sum launch instead of riding on the weight-gradient product
 *   SEGFAC_NO_GROUPED_DW         segf_gemm_dw_db_grouped runs its members one by one
 *   SEGFAC_DW_NO_XCD_SLABS       split-K weight gradients (128-tile kernel) in hardware workgroup order instead of one K slab per XCD
 *   SEGFAC_DW_NO_SHARED_SPLIT    grouped weight gradients keep their per-layer slice counts (also read by the host layer)
 *   SEGFAC_NO_WIDE_REDUCE        split-K partials of large outputs summed by the 16 x 16 form instead of whole rows
 *   SEGFAC_NO_REDUCE4            split-K reduce: one output per thread instead of four (bitwise the same sums)
 *   SEGFAC_GEMM_F32_NO_MFMA      fp32 storage (exact-parity mode, evaluate): products on the vector FMA kernel instead of the f32 matrix instruction
 *   SEGFAC_GEMM8_LINEAR          0: plain nn.Linear products never take the eight-phase kernel (the 256 / 128 tile kernels as in r04)  (default 1)
 *   SEGFAC_GEMM8_LINEAR_MIN_TILES fewest 256 x 256 tiles for which a K >= 2048 nn.Linear product takes the eight-phase kernel (192 for shorter K)  (default 128)
 *   SEGFAC_GEMM8_LINEAR_MIN_FILL smallest share (percent) of the launched 256 x 256 tiles that must be output for an nn.Linear product with ragged last tiles to take the eight-phase kernel  (default 60)
 *   SEGFAC_GEMM8_LINEAR_MIN_K    shortest reduction for which an nn.Linear product takes the eight-phase kernel (its 12-load prologue and drain against K / 64 tiles)  (default 256)
 *   SEGFAC_GEMM8_DW              0: nn.Linear weight gradients never take the eight-phase kernel below 65536 tokens (the grouped 128-tile kernel as in r04)  (default 1)
 *   SEGFAC_GEMM8_DW_MIN_GFLOP    smallest nn.Linear weight gradient (GFLOP; both feature counts multiples of 256, >= 256 FLOP per operand byte) that takes the eight-phase kernel + a column-sum pass instead of the grouped 128-tile kernel  (default 100)
 *   SEGFAC_GEMM8_LINEAR_MIN_GFLOP smallest nn.Linear product (GFLOP, K >= 512; 100 for shorter K) that takes the eight-phase kernel  (default 36)
 *   SEGFAC_NO_GEMM8              no eight-phase kernel at all (gemm8_kernel): the two-phase 256-tile kernel everywhere
 *   SEGFAC_NO_GEMM8T             no eight-phase kernel for weight gradients (reduction-major operands)
 *   SEGFAC_CONV_NO_FWD_SPLIT     3 x 3 forward / data gradient with few output tiles: no split over the (channel block, tap) walk
 *   SEGFAC_G8_STAGGER            eight-phase kernel: 1 = wave groups one barrier apart, 0 = lockstep, -1 = staggered for bf16 and the per-device choice (segf_gemm8_option) for fp8  (default -1)
 *   SEGFAC_NO_FP8                segf_gemm_fp8_supported answers 0 (block-scaled 128-tile fp8 GEMM)
 *   SEGFAC_NO_FP8_CONV           segf_conv3x3_fp8*_supported answer 0
 *   SEGFAC_NO_FP8_WGRAD          fp8 3 x 3 convolutions keep a bf16 weight gradient
 *   SEGFAC_NO_FP8_LINEAR         segf_linear_fp8_supported answers 0
 *   SEGFAC_DILCONV_NO_CULL       dilated 3 x 3 convolution: all nine taps are walked, with zero loads where a tap leaves the image, instead of the live taps only
 *   SEGFAC_ATTN_NO_MFMA          attention on the VALU reference kernels (attention.hip) also in bf16
 *   SEGFAC_ATTN_F32_NO_MFMA      fp32 attention forward on the vector kernel (one query per lane) instead of the f32 matrix instruction
 *   SEGFAC_ATTN64_PRESCALE       head dim 64, >= 128 keys: scale log2(e) rides on the Q fragments (bf16(q c), one more rounding per q element) and -max / -lse are the score accumulators' initial values, instead of one multiply-add per score: forward + query-side backward, +8 % / +2 % per kernel, attention error x 1.2 - 2.3
 *   SEGFAC_ATTN64_DKV_ROWS       head dim 64, >= 128 keys, key-side backward: query rows per staged Q / dO tile and barrier (128, 64 or 32: the same arithmetic, bit for bit)  (default 128)
 *   SEGFAC_ATTN_NO_FUSED_BWD     head dim 32, <= 256 keys: query-side + key-side backward kernels instead of the one-kernel backward
 *   SEGFAC_ATTN32_CLASSIC        head dim 32 backward (one-kernel and key-side kernels): the round-2 score arithmetic (subtract, multiply, __expf; (dP - D) scale per score) instead of P = exp2(S c - lse log2(e)) with -D as the C operand of the dP products and the scale applied once to dK and dQ
 *   SEGFAC_DW_NO_WALK            depthwise 3 x 3: the round-1 strip kernels instead of the vertical-walk kernels
 *   SEGFAC_DW_WALK_ROWS          depthwise 3 x 3 walk: rows per segment (0 = chosen from the map size)
 *   SEGFAC_DW_NO_SMALL           depthwise 3 x 3 backward of small maps: three passes instead of the one-launch LDS form
 *   SEGFAC_DW_SMALL_ALWAYS       ... the one-launch form beyond one round of workgroups as well
 *   SEGFAC_FFN_BWD_FUSED         Mix-FFN backward, fc2's data gradient formed inside pass A of the depthwise backward (segf_dwconv3x3_gelu_bwd_fc2_supported): 0 = never, 1 = from 131072 token rows on, 2 = wherever the shape has the kernel  (default 1)
 *   SEGFAC_NO_FUSE_MAP           folded SegFormerHead map: streaming product + VALU upsample-add instead of fuse_map_kernel
 *   SEGFAC_NO_BWD248_MFMA        transposed 1/2-1/4-1/8 resizes on the VALU kernel instead of fuse_map_bwd_kernel
 *   SEGFAC_UPADD_GENERIC         upsample-add: the generic per-source kernels also for the 2-4-8 pyramid
 *   SEGFAC_NO_HEAD_FUSED         segf_bn_cls_bwd_supported answers 0: classifier data gradient and BatchNorm backward as separate passes
 *   SEGFAC_NO_HEAD_FUSED_DW      the folded head's stage-1 weight gradient does not ride on pass 2 of the fused BatchNorm backward
 *   SEGFAC_HEAD_DB_RIDE          the classifier's bias gradient rides on pass 1 of the fused BatchNorm backward instead of a column-sum launch of its own (segf_bn_cls_bwd_full_db_supported): 0 = never, 1 = from 131072 token rows on, 2 = wherever the shape has the kernel  (default 1)
 *   SEGFAC_LOSS_NO_BAND          CE / Dice forward and backward on the tile kernels instead of the band sweep
 *   SEGFAC_LOSS_NO_BAND_FWD      ... the forward only
 *   SEGFAC_LOSS_BAND_ROWS        band sweep: rows per segment (0 = 16)
 *   SEGFAC_LOSS_NO_MFMA          ratio-4 loss kernels on the VALU cells form (fp32 storage)
 *   SEGFAC_LOSS_NO_RETRY         no exact per-pixel retry pass behind the flagged cells
 *   SEGFAC_LOSS_NO_LSE           the backward recomputes the softmax normalisation instead of taking the forward's per-pixel log-sum
 *   SEGFAC_LN_LINEAR_BWD_FUSED   Mix-FFN backward, fc1's data / weight / bias gradients formed inside the LayerNorm backward of norm2 (segf_layernorm_linear_bwd_supported): 0 = never, 1 = from 131072 token rows on, 2 = wherever the shape has the kernel  (default 1)
 *   SEGFAC_LN_LINEAR_FWD_FUSED   MiT stages 1 / 2: LayerNorm as the operand prologue of its thin Linear (norm2 -> fc1, norm1 -> q; segf_layernorm_linear_fwd_supported), the LayerNorm output neither stored nor saved, and norm1 -> q's backward in one pass where SEGFAC_LN_LINEAR_BWD_FUSED allows it too: 0 = never, 1 = from 131072 token rows on, 2 = wherever the shape has the kernel  (default 1)
 *   SEGFAC_NO_WIDE_FINALIZE      column-reduction finalize: one output per thread instead of four (bitwise the same sums)
 *   SEGFAC_NO_LN_PATCH           [host] MiT blocks: im2col / col2im around the spatial-reduction conv instead of the patch-major LayerNorm output
 *   SEGFAC_NO_SCALED_LN_BWD      [host] DropPath backward as its own scale_rows launch instead of riding on the LayerNorm backward
 *   SEGFAC_NO_DEFERRED_DW        [host] weight gradients issued layer by layer inside the captured step (no grouped launches)
 *   SEGFAC_NO_DEFERRED_FINALIZE  [host] LayerNorm dgamma / dbeta finalizes issued one by one
 *   SEGFAC_NO_HEAD_FUSED_CW      [host] the classifier's weight gradient as its own product instead of riding on pass 1 of the fused BatchNorm backward
 *   SEGFAC_NO_BWD248             [host] folded head backward: three segf_bilinear_bwd launches instead of the one-pass segf_bilinear_bwd_248
 *   SEGFAC_NO_GELU_GRN           [host] ConvNeXtV2 blocks: GELU as its own pass in front of the GRN kernels
 *   SEGFAC_NO_WEIGHT_SHADOW      [host] captured step: weights cast to bf16 per use instead of one cast of the flat buffer
 *   SEGFAC_NO_DERIVED_WEIGHTS    [host] captured step: derived weight layouts built in front of each layer instead of one grouped launch
 *
 * segf_policy_count / segf_policy_describe enumerate the table (field name, environment name, current value, default, description);
 * segf_policy_get / segf_policy_set read / change one value in the running process by field or environment name (INT_MIN: no such
 * switch; set returns the previous value); segf_policy_reload re-reads the environment (tests, A/B scripts).
 *
 * Launch trace: between segf_trace_begin(dry_run) and segf_trace_end(buf, cap) every kernel launched by the library ON THE CALLING
 * THREAD is recorded by its instantiated name (template arguments included), one per line in buf; segf_trace_end returns the number of
 * launches and closes the trace.  With dry_run != 0 the launches themselves (and the launch-error checks) are skipped: an entry point
 * can then be called with any non-null, 16-byte-aligned pointer values on a machine WITHOUT a GPU to learn which kernels a shape takes
 * -- tests/test_host_cpu.py::test_dispatch_of_baseline_shapes pins the BASELINE shapes against tests/golden/dispatch_table.json, so a
 * dispatch edit shows up as a diff. */
int segf_policy_count(void);
int segf_policy_describe(int i, const char** field, const char** env, int* value, int* def, const char** doc);
int segf_policy_get(const char* name);
int segf_policy_set(const char* name, int value);
void segf_policy_reload(void);
void segf_trace_begin(int dry_run);
int segf_trace_end(char* buf, int cap);

#ifdef __cplusplus
}
#endif
#endif
