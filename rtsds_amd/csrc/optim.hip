// Fused optimizer steps over the flat parameter arena (gfx950): Adam, SGD.
#include "ew_common.h"

// ------------------------------------------------------------------ Adam (flat, fused)
// torch.optim.Adam (main.py:116-117; L2 weight decay folded into the gradient, as torch does
// for weight_decay != 0 without decoupling).  One launch over the flat parameter arena;
// optionally refreshes the bf16 shadow weights in the same pass.
template <typename GT>
__global__ void adam_kernel(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            bf16* __restrict__ shadow, long n, float lr, float b1, float b2, float eps, float wd, float bc1,
                            float bc2_sqrt, float gscale) {
  const float step = lr / bc1;
  GRID_STRIDE(i, n) {
    float gi = to_f(g[i]) * gscale;
    float pi = p[i];
    if (wd != 0.f) gi = fmaf(wd, pi, gi);
    float mi = m[i], vi = v[i];
    mi = fmaf(1.f - b1, gi - mi, mi);
    vi = fmaf(b2, vi, (1.f - b2) * gi * gi);
    const float den = sqrtf(vi) / bc2_sqrt + eps;
    pi -= step * (mi / den);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
    if (shadow) shadow[i] = (bf16)pi;
  }
}
// Same update with (lr, bias_correction1, sqrt(bias_correction2)) read from device memory, so
// a captured hipGraph replays correct steps as the host advances lr / step counts between
// replays (runtime.GraphedStep).
template <typename GT>
__global__ void adam_dev_kernel(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                bf16* __restrict__ shadow, long n, const float* __restrict__ hyper, float b1, float b2, float eps,
                                float wd, float gscale) {
  const float lr = hyper[0], bc1 = hyper[1], bc2_sqrt = hyper[2];
  const float step = lr / bc1;
  GRID_STRIDE(i, n) {
    float gi = to_f(g[i]) * gscale;
    float pi = p[i];
    if (wd != 0.f) gi = fmaf(wd, pi, gi);
    float mi = m[i], vi = v[i];
    mi = fmaf(1.f - b1, gi - mi, mi);
    vi = fmaf(b2, vi, (1.f - b2) * gi * gi);
    const float den = sqrtf(vi) / bc2_sqrt + eps;
    pi -= step * (mi / den);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
    if (shadow) shadow[i] = (bf16)pi;
  }
}
// the gradient in fp32 (the arena), or the all-reduced fp16 / bf16 wire copy read directly
#define DISPATCH_GRAD(gd, ...)                                               \
  do {                                                                       \
    if ((gd) == RTSDS_F32) { typedef float GT; __VA_ARGS__; }                \
    else if ((gd) == RTSDS_BF16) { typedef bf16 GT; __VA_ARGS__; }           \
    else if ((gd) == RTSDS_F16) { typedef f16 GT; __VA_ARGS__; }             \
    else return RTSDS_ERR_UNSUPPORTED;                                       \
  } while (0)
extern "C" int rtsds_adam_step_dev(float* param, const void* grad, float* exp_avg, float* exp_avg_sq, void* bf16_shadow,
                                   long n, const float* hyper, float beta1, float beta2, float eps, float weight_decay,
                                   float grad_scale, int grad_dtype, void* stream) {
  if (n <= 0 || !hyper) return RTSDS_ERR_SHAPE;
  DISPATCH_GRAD(grad_dtype, hipLaunchKernelGGL(adam_dev_kernel<GT>, dim3(ew_blocks(n, 256, 4096)), dim3(256), 0,
                                               (hipStream_t)stream, param, (const GT*)grad, exp_avg, exp_avg_sq,
                                               (bf16*)bf16_shadow, n, hyper, beta1, beta2, eps, weight_decay, grad_scale));
  RET_LAUNCH();
}

extern "C" int rtsds_adam_step(float* param, const void* grad, float* exp_avg, float* exp_avg_sq, void* bf16_shadow, long n, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, int grad_dtype,
                               void* stream) {
  if (n <= 0 || step <= 0) return RTSDS_ERR_SHAPE;
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  DISPATCH_GRAD(grad_dtype, hipLaunchKernelGGL(adam_kernel<GT>, dim3(ew_blocks(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream,
                                               param, (const GT*)grad, exp_avg, exp_avg_sq, (bf16*)bf16_shadow, n, lr, beta1, beta2,
                                               eps, weight_decay, (float)bc1, (float)sqrt(bc2), grad_scale));
  RET_LAUNCH();
}

// ------------------------------------------------------------------ SGD (flat, fused)
// torch.optim.SGD (main.py:118-120): d = g (+ wd p); with momentum, buf = d on a parameter's
// first step, else buf = momentum buf + (1 - dampening) d; d = nesterov ? d + momentum buf :
// buf; p -= lr d.  hyper (device, may be NULL) = {lr, first-step flag}: the hipGraph-replay
// variant (runtime.GraphedStep) reads them per replay.
template <typename GT>
__global__ void sgd_kernel(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ buf,
                           bf16* __restrict__ shadow, long n, const float* __restrict__ hyper, float lr, float momentum,
                           float dampening, float wd, int nesterov, int first, float gscale) {
  if (hyper) {
    lr = hyper[0];
    first = hyper[1] != 0.f;
  }
  GRID_STRIDE(i, n) {
    float pi = p[i];
    float d = to_f(g[i]) * gscale;
    if (wd != 0.f) d = d + wd * pi;
    if (momentum != 0.f) {
      const float b = first ? d : buf[i] * momentum + (1.f - dampening) * d;
      buf[i] = b;
      d = nesterov ? d + momentum * b : b;
    }
    pi = pi + (-lr) * d;
    p[i] = pi;
    if (shadow) shadow[i] = (bf16)pi;
  }
}

extern "C" int rtsds_sgd_step(float* param, const void* grad, float* momentum_buf, void* bf16_shadow, long n,
                              const float* hyper, float lr, float momentum, float dampening, float weight_decay,
                              int nesterov, int first, float grad_scale, int grad_dtype, void* stream) {
  if (n <= 0 || (momentum != 0.f && !momentum_buf)) return RTSDS_ERR_SHAPE;
  DISPATCH_GRAD(grad_dtype, hipLaunchKernelGGL(sgd_kernel<GT>, dim3(ew_blocks(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream,
                                               param, (const GT*)grad, momentum_buf, (bf16*)bf16_shadow, n, hyper, lr, momentum,
                                               dampening, weight_decay, nesterov, first, grad_scale));
  RET_LAUNCH();
}

// ------------------------------------------------------------------ EMA teacher (flat, fused)
// Mean-teacher update t += w (s - t) over a flat arena (ema.EMATeacher; no reference
// counterpart), the bf16 shadow written in the same pass as adam_kernel does.  Three separately
// rounded fp32 operations, never an FMA, so the update can be restated exactly on the host or
// with three torch ops; w = float32(1 - decay) comes from the host.
// (__fadd_rn(t, __fmul_rn(w, __fsub_rn(s, t))): the header intrinsics are plain operators the
// compiler may still contract into an FMA, so the three operations are written out with
// contraction switched off for this function.)
RT_DEV float ema_update(float t, float s, float w) {
#pragma clang fp contract(off)
  const float d = s - t;
  const float m = w * d;
  return t + m;
}
// VEC: 8 elements per thread and trip as two 16-B loads of t and of s, two 16-B stores of t and
// one 16-B store of the shadow (the host checked the three pointers); the tail, and everything
// when a pointer is not 16-B aligned, goes element by element.
template <bool VEC>
__global__ void __launch_bounds__(256) ema_kernel(float* __restrict__ t, const float* __restrict__ s, bf16* __restrict__ shadow,
                                                  long n, float w) {
  const long nv = VEC ? n >> 3 : 0;
  GRID_STRIDE(i, nv) {
    f32x4 ta = ((const f32x4*)t)[2 * i], tb = ((const f32x4*)t)[2 * i + 1];
    const f32x4 sa = ((const f32x4*)s)[2 * i], sb = ((const f32x4*)s)[2 * i + 1];
    bf16x8 h;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ta[j] = ema_update(ta[j], sa[j], w);
      tb[j] = ema_update(tb[j], sb[j], w);
      h[j] = (bf16)ta[j];
      h[4 + j] = (bf16)tb[j];
    }
    ((f32x4*)t)[2 * i] = ta;
    ((f32x4*)t)[2 * i + 1] = tb;
    if (shadow) ((bf16x8*)shadow)[i] = h;
  }
  const long done = nv << 3;
  GRID_STRIDE(r, n - done) {
    const long i = done + r;
    const float ti = ema_update(t[i], s[i], w);
    t[i] = ti;
    if (shadow) shadow[i] = (bf16)ti;
  }
}
extern "C" int rtsds_ema_step(float* teacher, const float* student, void* teacher_bf16_shadow, long n, float w, void* stream) {
  if (n <= 0) return RTSDS_ERR_SHAPE;
  if (teacher == nullptr || student == nullptr || ((uintptr_t)teacher & 3) || ((uintptr_t)student & 3) ||
      ((uintptr_t)teacher_bf16_shadow & 1))
    return RTSDS_ERR_UNSUPPORTED;
  const bool vec = (((uintptr_t)teacher | (uintptr_t)student | (uintptr_t)teacher_bf16_shadow) & 15) == 0 && n >= 8;
  with_bool(vec, [&](auto v) {
    constexpr bool VEC = decltype(v)::value;
    hipLaunchKernelGGL(ema_kernel<VEC>, dim3(ew_blocks(VEC ? (n + 7) / 8 : n, 256, 4096)), dim3(256), 0, (hipStream_t)stream,
                       teacher, student, (bf16*)teacher_bf16_shadow, n, w);
  });
  RET_LAUNCH();
}

// The same update for state outside an arena (the BatchNorm running statistics): count segments,
// one workgroup row (blockIdx.y) each, described by three device tables; no shadow.
static const int kEmaManyBlocks = 4;  // workgroups per segment: a BatchNorm statistic is <= 2048 floats
__global__ void __launch_bounds__(256) ema_many_kernel(float* const* __restrict__ teacher, const float* const* __restrict__ student,
                                                       const long* __restrict__ numel, float w) {
  const int seg = blockIdx.y;
  float* t = teacher[seg];
  const float* s = student[seg];
  const long n = numel[seg];
  GRID_STRIDE(i, n) t[i] = ema_update(t[i], s[i], w);
}
extern "C" int rtsds_ema_many(int count, float* const* teacher, const float* const* student, const long* numel, float w,
                              void* stream) {
  if (count <= 0) return RTSDS_ERR_SHAPE;
  if (teacher == nullptr || student == nullptr || numel == nullptr || (((uintptr_t)teacher | (uintptr_t)student | (uintptr_t)numel) & 7) ||
      count > 65535)
    return RTSDS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(ema_many_kernel, dim3(kEmaManyBlocks, count), dim3(256), 0, (hipStream_t)stream, teacher, student, numel, w);
  RET_LAUNCH();
}
