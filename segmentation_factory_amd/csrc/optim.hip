// Fused optimizer steps over a flat fp32 parameter buffer: adaptive gradient clipping (unit-wise, AGC) + AdamW, and further down
// the same structure for SGD / Adam / RMSprop (flat_optim_kernel).
// Stands in for what engine.py:52-53 triggers through timm 0.9.2's NativeScaler: dispatch_clip_grad(mode='agc',
// value=0.02) followed by optimizer.step() of the AdamW that create_optimizer builds (train_gpu.py:99-102,269-270).
// timm is not installed in the build image, so this arithmetic is restated from timm 0.9.2 / torch.optim.AdamW
// semantics and pinned only by hand-derived known-answer tests ("parity unpinned"):
//   unit = one output row of a >=2-D weight (dim 0), or the whole tensor for 1-D parameters
//   max_norm = max(||p_unit||, agc_eps) * clip_factor;  g <- g * max_norm / max(||g_unit||, 1e-6)  if ||g_unit|| >= max_norm
//   p <- p * (1 - lr * wd);  m <- b1 m + (1-b1) g;  v <- b2 v + (1-b2) g^2;
//   p <- p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// unit_flags: bit 0 = weight decay applies, bit 1 = the unit's parameter received no gradient this step (skipped entirely).
// One wave per unit: two streaming passes over the unit (norms, then update); 7 x 4 B per parameter of HBM traffic.
#include "common.h"

// One wave per unit, grid-stride over the units.  Formed in the __global__ function itself and handed to the shared body: the launch
// geometry folds to the uniform-workgroup form there, which it does not inside a device function (the scalar kernels compile to
// the instructions they had before the body was shared; profiles/optim_groups.md).
struct WaveWalk {
    int lane;
    int64_t wave_global, nwaves;
};
#define WAVE_WALK() \
    WaveWalk{(int)(threadIdx.x & 63), ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, ((int64_t)gridDim.x * blockDim.x) >> 6}

// Where a unit's learning rate and weight decay come from.  The step kernels are written once over a `Hyper` (one home for each rule's
// arithmetic) and instantiated twice: OptScalars = one lr / wd for the whole buffer, decay switched per unit by flag bit 0 (the
// kernels of segf_agc_adamw / segf_flat_optim_step); OptGroups = the unit's parameter group picks both from a table that is itself
// a by-value kernel argument (read from the kernarg segment: still one launch with launch scalars only, no device table to refresh,
// nothing for a host that runs ahead to race), decay applies where the group's value is non-zero and bit 0 is ignored.
struct OptScalars {
    float lr, wd;
    __device__ __forceinline__ bool get(int64_t, int uflags, float& l, float& w, int& decays) const {
        l = lr; w = wd; decays = uflags & 1;
        return true;
    }
};

struct OptGroups {
    float lr[SEGF_OPT_MAX_GROUPS], wd[SEGF_OPT_MAX_GROUPS];
    const uint8_t* unit_group;
    int ngroups;
    __device__ __forceinline__ bool get(int64_t u, int, float& l, float& w, int& decays) const {
        const int g = unit_group[u];
        if (g >= ngroups) return false;          // a group index outside the table: the unit is left alone, nothing is read past it
        l = lr[g]; w = wd[g]; decays = w != 0.f;
        return true;
    }
};

template <class Hyper>
__device__ __forceinline__ void agc_adamw_units(float* __restrict__ param, const float* __restrict__ grad,
                                                float* __restrict__ m, float* __restrict__ v,
                                                const int64_t* __restrict__ unit_off, const int32_t* __restrict__ unit_len,
                                                const uint8_t* __restrict__ unit_flags, int32_t* __restrict__ unit_step,
                                                int nunits, const Hyper& hyper, float b1, float b2, float eps, float bc1_,
                                                float bc2_sqrt_, float clip_factor, float agc_eps, const WaveWalk w) {
    const int lane = w.lane;
    const int64_t wave_global = w.wave_global, nwaves = w.nwaves;
    for (int64_t u = wave_global; u < nunits; u += nwaves) {
        const int64_t off = unit_off[u];
        const int len = unit_len[u];
        const int uflags = unit_flags[u];
        if (uflags & 2) continue;          // no gradient this step: torch.optim.AdamW skips `p.grad is None` (no decay, no moments)
        float lr, wd;
        int decays;
        if (!hyper.get(u, uflags, lr, wd, decays)) continue;
        float bc1 = bc1_, bc2_sqrt = bc2_sqrt_;
        if (unit_step) {                   // per-parameter step count, as torch keeps it (state['step']): a skipped step does not count
            const int t = unit_step[u] + 1;      // every lane reads before lane 0 writes (same wave, program order)
            bc1 = 1.f - powf(b1, (float)t);
            bc2_sqrt = sqrtf(1.f - powf(b2, (float)t));
            if (lane == 0) unit_step[u] = t;
        }
        float gscale = 1.f;
        if (clip_factor > 0.f) {
            float pn = 0.f, gn = 0.f;
            for (int i = lane; i < len; i += 64) {
                const float p = param[off + i], g = grad[off + i];
                pn = fmaf(p, p, pn); gn = fmaf(g, g, gn);
            }
            pn = sqrtf(wave_sum(pn)); gn = sqrtf(wave_sum(gn));
            const float max_norm = fmaxf(pn, agc_eps) * clip_factor;
            if (!(gn < max_norm)) gscale = max_norm / fmaxf(gn, 1e-6f);
        }
        const float decay = decays ? 1.f - lr * wd : 1.f;
        const float step = lr / bc1;
        for (int i = lane; i < len; i += 64) {
            const float g = grad[off + i] * gscale;
            float p = param[off + i] * decay;
            const float mm = b1 * m[off + i] + (1.f - b1) * g;
            const float vv = b2 * v[off + i] + (1.f - b2) * g * g;
            p -= step * mm / (sqrtf(vv) / bc2_sqrt + eps);
            param[off + i] = p; m[off + i] = mm; v[off + i] = vv;
        }
    }
}

__global__ void __launch_bounds__(256) agc_adamw_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                         float* __restrict__ m, float* __restrict__ v,
                                                         const int64_t* __restrict__ unit_off, const int32_t* __restrict__ unit_len,
                                                         const uint8_t* __restrict__ unit_flags, int32_t* __restrict__ unit_step,
                                                         int nunits, float lr, float b1, float b2, float eps, float wd, float bc1_,
                                                         float bc2_sqrt_, float clip_factor, float agc_eps) {
    agc_adamw_units(param, grad, m, v, unit_off, unit_len, unit_flags, unit_step, nunits, OptScalars{lr, wd}, b1, b2, eps, bc1_,
                    bc2_sqrt_, clip_factor, agc_eps, WAVE_WALK());
}

__global__ void __launch_bounds__(256) agc_adamw_groups_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                                float* __restrict__ m, float* __restrict__ v,
                                                                const int64_t* __restrict__ unit_off, const int32_t* __restrict__ unit_len,
                                                                const uint8_t* __restrict__ unit_flags, int32_t* __restrict__ unit_step,
                                                                int nunits, OptGroups groups, float b1, float b2, float eps, float bc1_,
                                                                float bc2_sqrt_, float clip_factor, float agc_eps) {
    agc_adamw_units(param, grad, m, v, unit_off, unit_len, unit_flags, unit_step, nunits, groups, b1, b2, eps, bc1_, bc2_sqrt_,
                    clip_factor, agc_eps, WAVE_WALK());
}

// The host side of the group forms: the refusals documented in include/segfac.h, then the two host arrays copied into the by-value
// kernel argument.
static int opt_groups_fill(OptGroups& t, const uint8_t* unit_group, int ngroups, const float* group_lr, const float* group_wd) {
    if (ngroups < 1 || ngroups > SEGF_OPT_MAX_GROUPS || !unit_group || !group_lr || !group_wd) return SEGF_ERR_SHAPE;
    for (int g = 0; g < SEGF_OPT_MAX_GROUPS; ++g) {
        t.lr[g] = g < ngroups ? group_lr[g] : 0.f;
        t.wd[g] = g < ngroups ? group_wd[g] : 0.f;
    }
    t.unit_group = unit_group;
    t.ngroups = ngroups;
    return 0;
}

extern "C" int segf_agc_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const int64_t* unit_offset,
                              const int32_t* unit_len, const uint8_t* unit_flags, int32_t* unit_step, int nunits, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int step, float clip_factor, float agc_eps,
                              void* stream) {
    if (nunits <= 0) return 0;
    if (step < 1 && !unit_step) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2_sqrt = sqrtf(1.f - powf(beta2, (float)step));
    const int blocks = imin((nunits + 3) / 4, 4096);
    hipLaunchKernelGGL(agc_adamw_kernel, dim3(blocks), dim3(256), 0, st, param, grad, exp_avg, exp_avg_sq, unit_offset, unit_len,
                       unit_flags, unit_step, nunits, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, clip_factor, agc_eps);
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int segf_agc_adamw_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const int64_t* unit_offset,
                                     const int32_t* unit_len, const uint8_t* unit_flags, int32_t* unit_step, int nunits,
                                     const uint8_t* unit_group, int ngroups, const float* group_lr, const float* group_wd, float beta1,
                                     float beta2, float eps, int step, float clip_factor, float agc_eps, void* stream) {
    OptGroups groups;
    if (int rc = opt_groups_fill(groups, unit_group, ngroups, group_lr, group_wd)) return rc;
    if (nunits <= 0) return 0;
    if (step < 1 && !unit_step) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2_sqrt = sqrtf(1.f - powf(beta2, (float)step));
    const int blocks = imin((nunits + 3) / 4, 4096);
    hipLaunchKernelGGL(agc_adamw_groups_kernel, dim3(blocks), dim3(256), 0, st, param, grad, exp_avg, exp_avg_sq, unit_offset, unit_len,
                       unit_flags, unit_step, nunits, groups, beta1, beta2, eps, bc1, bc2_sqrt, clip_factor, agc_eps);
    SEGF_CHECK_LAUNCH();
    return 0;
}

// ---- the other --opt values of the reference's CLI (train_gpu.py:93-104 -> timm.optim.create_optimizer, train_gpu.py:269): SGD
// (momentum / nesterov), Adam and RMSprop over the same flat buffers, unit tables, skip bit and per-unit step counts as
// agc_adamw_kernel, so the step stays one launch with launch scalars only (graph-replay safe).  Each rule is the fp32 arithmetic of
// the torch.optim class of that name (maximize=False, dampening 0, not centered, no amsgrad) and is pinned to it step for step:
//   all rules:  g <- g * agc_scale (clip_factor > 0; on the RAW gradient, as dispatch_clip_grad precedes optimizer.step());
//               g <- g + wd * p  where flag bit 0 is set (L2 coupled into the gradient)
//   SGD:        buf <- mu buf + g;  d = g + mu buf (nesterov) | buf;  p <- p - lr d;      mu == 0: p <- p - lr g, no state
//   ADAM:       m <- b1 m + (1-b1) g;  v <- b2 v + (1-b2) g^2;  p <- p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
//   RMSPROP:    sq <- a sq + (1-a) g^2;  d = g / (sqrt(sq) + eps);  mu > 0: buf <- mu buf + d, p <- p - lr buf;  else p <- p - lr d
// torch's SGD starts momentum_buffer as a clone of the first gradient = mu * 0 + g: zero-initialised state reproduces it.
// HBM traffic per parameter: 12 B without state, 20 B with one state buffer, 28 B with two (+ 8 B for the AGC norm pass, which
// mostly hits L2 for units that fit).
template <int RULE, bool MOM, class Hyper>
__device__ __forceinline__ void flat_optim_units(float* __restrict__ param, const float* __restrict__ grad,
                                                 float* __restrict__ s0, float* __restrict__ s1,
                                                 const int64_t* __restrict__ unit_off, const int32_t* __restrict__ unit_len,
                                                 const uint8_t* __restrict__ unit_flags, int32_t* __restrict__ unit_step,
                                                 int nunits, const Hyper& hyper, float h0, float h1, float eps, int nesterov,
                                                 float clip_factor, float agc_eps, const WaveWalk w) {
    const int lane = w.lane;
    const int64_t wave_global = w.wave_global, nwaves = w.nwaves;
    for (int64_t u = wave_global; u < nunits; u += nwaves) {
        const int64_t off = unit_off[u];
        const int len = unit_len[u];
        const int uflags = unit_flags[u];
        if (uflags & 2) continue;          // no gradient this step: torch.optim skips `p.grad is None` (no decay, no state, no count)
        float lr, wd;
        int decays;
        if (!hyper.get(u, uflags, lr, wd, decays)) continue;
        int t = 1;
        if (unit_step) {                   // per-parameter step count, as torch keeps it (state['step']): a skipped step does not count
            t = unit_step[u] + 1;          // every lane reads before lane 0 writes (same wave, program order)
            if (lane == 0) unit_step[u] = t;
        }
        float gscale = 1.f;
        if (clip_factor > 0.f) {           // unit-wise AGC: the arithmetic of agc_adamw_kernel
            float pn = 0.f, gn = 0.f;
            for (int i = lane; i < len; i += 64) {
                const float p = param[off + i], g = grad[off + i];
                pn = fmaf(p, p, pn); gn = fmaf(g, g, gn);
            }
            pn = sqrtf(wave_sum(pn)); gn = sqrtf(wave_sum(gn));
            const float max_norm = fmaxf(pn, agc_eps) * clip_factor;
            if (!(gn < max_norm)) gscale = max_norm / fmaxf(gn, 1e-6f);
        }
        const float l2 = decays ? wd : 0.f;
        if (RULE == SEGF_OPT_SGD) {
            const float mu = h0;
            for (int i = lane; i < len; i += 64) {
                float p = param[off + i];
                const float g = fmaf(l2, p, grad[off + i] * gscale);
                float d = g;
                if (MOM) {
                    const float buf = fmaf(mu, s0[off + i], g);
                    s0[off + i] = buf;
                    d = nesterov ? fmaf(mu, buf, g) : buf;
                }
                param[off + i] = fmaf(-lr, d, p);
            }
        } else if (RULE == SEGF_OPT_ADAM) {
            const float b1 = h0, b2 = h1;
            const float step = lr / (1.f - powf(b1, (float)t));
            const float bc2_sqrt = sqrtf(1.f - powf(b2, (float)t));
            for (int i = lane; i < len; i += 64) {
                float p = param[off + i];
                const float g = fmaf(l2, p, grad[off + i] * gscale);
                const float mm = b1 * s0[off + i] + (1.f - b1) * g;
                const float vv = b2 * s1[off + i] + (1.f - b2) * g * g;
                p -= step * mm / (sqrtf(vv) / bc2_sqrt + eps);
                param[off + i] = p; s0[off + i] = mm; s1[off + i] = vv;
            }
        } else {
            const float alpha = h0, mu = h1;
            for (int i = lane; i < len; i += 64) {
                float p = param[off + i];
                const float g = fmaf(l2, p, grad[off + i] * gscale);
                const float sq = alpha * s0[off + i] + (1.f - alpha) * g * g;
                s0[off + i] = sq;
                float d = g / (sqrtf(sq) + eps);
                if (MOM) {
                    d = fmaf(mu, s1[off + i], d);
                    s1[off + i] = d;
                }
                param[off + i] = fmaf(-lr, d, p);
            }
        }
    }
}

template <int RULE, bool MOM>
__global__ void __launch_bounds__(256) flat_optim_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                          float* __restrict__ s0, float* __restrict__ s1,
                                                          const int64_t* __restrict__ unit_off, const int32_t* __restrict__ unit_len,
                                                          const uint8_t* __restrict__ unit_flags, int32_t* __restrict__ unit_step,
                                                          int nunits, float lr, float wd, float h0, float h1, float eps, int nesterov,
                                                          float clip_factor, float agc_eps) {
    flat_optim_units<RULE, MOM>(param, grad, s0, s1, unit_off, unit_len, unit_flags, unit_step, nunits, OptScalars{lr, wd}, h0, h1, eps,
                                nesterov, clip_factor, agc_eps, WAVE_WALK());
}

template <int RULE, bool MOM>
__global__ void __launch_bounds__(256) flat_optim_groups_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                                 float* __restrict__ s0, float* __restrict__ s1,
                                                                 const int64_t* __restrict__ unit_off, const int32_t* __restrict__ unit_len,
                                                                 const uint8_t* __restrict__ unit_flags, int32_t* __restrict__ unit_step,
                                                                 int nunits, OptGroups groups, float h0, float h1, float eps, int nesterov,
                                                                 float clip_factor, float agc_eps) {
    flat_optim_units<RULE, MOM>(param, grad, s0, s1, unit_off, unit_len, unit_flags, unit_step, nunits, groups, h0, h1, eps, nesterov,
                                clip_factor, agc_eps, WAVE_WALK());
}

// The rule / momentum choice and each rule's null-buffer refusals, once for both entry points: LAUNCH(rule, has momentum) starts the
// instantiation.  Nesterov without a momentum is torch's "Nesterov momentum requires a momentum and zero dampening"; Adam's bias
// corrections come from the unit's own count.
#define SEGF_FLAT_OPTIM_RULES(LAUNCH)                                                  \
    if (rule == SEGF_OPT_SGD) {                                                        \
        if (h0 != 0.f) {                                                               \
            if (!s0) return SEGF_ERR_SHAPE;                                            \
            LAUNCH(SEGF_OPT_SGD, true);                                                \
        } else {                                                                       \
            if (nesterov) return SEGF_ERR_SHAPE;                                       \
            LAUNCH(SEGF_OPT_SGD, false);                                               \
        }                                                                              \
    } else if (rule == SEGF_OPT_ADAM) {                                                \
        if (!s0 || !s1 || !unit_step) return SEGF_ERR_SHAPE;                           \
        LAUNCH(SEGF_OPT_ADAM, true);                                                   \
    } else if (rule == SEGF_OPT_RMSPROP) {                                             \
        if (!s0) return SEGF_ERR_SHAPE;                                                \
        if (h1 > 0.f) {                                                                \
            if (!s1) return SEGF_ERR_SHAPE;                                            \
            LAUNCH(SEGF_OPT_RMSPROP, true);                                            \
        } else {                                                                       \
            LAUNCH(SEGF_OPT_RMSPROP, false);                                           \
        }                                                                              \
    } else {                                                                           \
        return SEGF_ERR_SHAPE;                                                         \
    }

extern "C" int segf_flat_optim_step(int rule, float* param, const float* grad, float* s0, float* s1, const int64_t* unit_offset,
                                    const int32_t* unit_len, const uint8_t* unit_flags, int32_t* unit_step, int nunits, float lr,
                                    float weight_decay, float h0, float h1, float eps, int nesterov, float clip_factor, float agc_eps,
                                    void* stream) {
    if (nunits <= 0) return 0;
    if (!param || !grad || !unit_offset || !unit_len || !unit_flags) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = imin((nunits + 3) / 4, 4096);
#define SEGF_FLAT_OPTIM(R, M)                                                                                                      \
    hipLaunchKernelGGL((flat_optim_kernel<R, M>), dim3(blocks), dim3(256), 0, st, param, grad, s0, s1, unit_offset, unit_len,      \
                       unit_flags, unit_step, nunits, lr, weight_decay, h0, h1, eps, nesterov, clip_factor, agc_eps)
    SEGF_FLAT_OPTIM_RULES(SEGF_FLAT_OPTIM)
#undef SEGF_FLAT_OPTIM
    SEGF_CHECK_LAUNCH();
    return 0;
}

extern "C" int segf_flat_optim_step_groups(int rule, float* param, const float* grad, float* s0, float* s1, const int64_t* unit_offset,
                                           const int32_t* unit_len, const uint8_t* unit_flags, int32_t* unit_step, int nunits,
                                           const uint8_t* unit_group, int ngroups, const float* group_lr, const float* group_wd,
                                           float h0, float h1, float eps, int nesterov, float clip_factor, float agc_eps,
                                           void* stream) {
    OptGroups groups;
    if (int rc = opt_groups_fill(groups, unit_group, ngroups, group_lr, group_wd)) return rc;
    if (nunits <= 0) return 0;
    if (!param || !grad || !unit_offset || !unit_len || !unit_flags) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = imin((nunits + 3) / 4, 4096);
#define SEGF_FLAT_OPTIM_GROUPS(R, M)                                                                                               \
    hipLaunchKernelGGL((flat_optim_groups_kernel<R, M>), dim3(blocks), dim3(256), 0, st, param, grad, s0, s1, unit_offset, unit_len, \
                       unit_flags, unit_step, nunits, groups, h0, h1, eps, nesterov, clip_factor, agc_eps)
    SEGF_FLAT_OPTIM_RULES(SEGF_FLAT_OPTIM_GROUPS)
#undef SEGF_FLAT_OPTIM_GROUPS
    SEGF_CHECK_LAUNCH();
    return 0;
}

// ---- the other two --clip-mode values of the reference (train_gpu.py:99-102 -> timm.utils.dispatch_clip_grad) over the flat
// gradient buffer, device-only (no host read of the norm, graph-capturable):
//   'norm'  = torch.nn.utils.clip_grad_norm_(parameters, value, norm_type=2.0): g *= min(1, value / (||g||_2 + 1e-6))
//   'value' = torch.nn.utils.clip_grad_value_(parameters, value):               g = clamp(g, -value, value)
// The norm is a fixed-order reduction (per-workgroup partials over fixed slices, then every workgroup re-reduces the partials in
// the same order in double): bitwise reproducible, and independent of how the buffer is cut into parameters.
constexpr int CLIP_BLOCKS = 1024;

__global__ void __launch_bounds__(256) grad_sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partial) {
    __shared__ float red[4];
    const int64_t per = (n + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < n ? lo + per : n;
    float acc = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) { const float v = g[i]; acc = fmaf(v, v, acc); }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(256) grad_scale_by_norm_kernel(float* __restrict__ g, int64_t n, const float* __restrict__ partial,
                                                                  int nparts, float max_norm) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) acc += (double)partial[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const float total = (float)sqrt(red[0]);
    const float coef = fminf(max_norm / (total + 1e-6f), 1.f);
    if (coef >= 1.f) return;
    const int64_t per = (n + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < n ? lo + per : n;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) g[i] *= coef;
}

__global__ void __launch_bounds__(256) grad_clamp_kernel(float* __restrict__ g, int64_t n, float v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) g[i] = fminf(fmaxf(g[i], -v), v);
}

extern "C" int64_t segf_clip_grad_ws(void) { return CLIP_BLOCKS; }

extern "C" int segf_clip_grad(float* grad, int64_t n, int mode, float value, float* ws, void* stream) {
    if (n <= 0) return 0;
    if (!grad || (mode != 0 && mode != 1) || !(value >= 0.f)) return SEGF_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = (int)imin64(cdiv64(n, 4096), CLIP_BLOCKS);
    if (mode == 0) {
        if (!ws) return SEGF_ERR_WORKSPACE;
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, st, grad, n, ws);
        hipLaunchKernelGGL(grad_scale_by_norm_kernel, dim3(blocks), dim3(256), 0, st, grad, n, ws, blocks, value);
    } else {
        hipLaunchKernelGGL(grad_clamp_kernel, dim3(blocks), dim3(256), 0, st, grad, n, value);
    }
    SEGF_CHECK_LAUNCH();
    return 0;
}
