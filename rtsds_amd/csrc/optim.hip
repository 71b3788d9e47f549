// Fused optimizer steps over the flat parameter arena (gfx950): Adam, SGD.
#include "ew_common.h"
#include "split_reduce_dev.h"

// ------------------------------------------------------------------ Adam (flat, fused)
// torch.optim.Adam (main.py:116-117; L2 weight decay folded into the gradient, as torch does
// for weight_decay != 0 without decoupling).  One launch over the flat parameter arena;
// optionally refreshes the bf16 shadow weights in the same pass.
// One element's update, the single statement of it: adam_kernel, adam_dev_kernel and
// adam_slabs_kernel all inline this, so their bits cannot drift apart.  gi: the gradient already
// scaled; step = lr / bias_correction1.
RT_DEV void adam_elem(float& pi, float gi, float& mi, float& vi, float step, float b1, float b2, float eps, float wd,
                      float bc2_sqrt) {
  if (wd != 0.f) gi = fmaf(wd, pi, gi);
  mi = fmaf(1.f - b1, gi - mi, mi);
  vi = fmaf(b2, vi, (1.f - b2) * gi * gi);
  const float den = sqrtf(vi) / bc2_sqrt + eps;
  pi -= step * (mi / den);
}
template <typename GT>
__global__ void adam_kernel(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            bf16* __restrict__ shadow, long n, float lr, float b1, float b2, float eps, float wd, float bc1,
                            float bc2_sqrt, float gscale) {
  const float step = lr / bc1;
  GRID_STRIDE(i, n) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_elem(pi, to_f(g[i]) * gscale, mi, vi, step, b1, b2, eps, wd, bc2_sqrt);
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
    float pi = p[i], mi = m[i], vi = v[i];
    adam_elem(pi, to_f(g[i]) * gscale, mi, vi, step, b1, b2, eps, wd, bc2_sqrt);
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

// ------------------------------------------------------------------ Adam fused with the split-K reduce
// rtsds_adam_step_slabs: one launch over an arena run whose weight gradients still lie in split-K
// slabs.  Slab blocks (64 float4 outputs of one descriptor each) sum the slabs exactly as
// split_reduce_many_kernel does (split_reduce_block) and their sg == 0 wave applies adam_elem to the
// 4 elements per lane straight away: the gradient never reaches memory (RTSDS_SLAB_KEEP_GRAD: it
// is stored as well).  Plain blocks run the ordinary update, gradient from the arena, over the
// gaps between the descriptors' ranges [dw, dw + 4 nv), kAdamPlainChunk floats per block.  The
// host sorts nothing: it checks that the ranges are ascending, disjoint, 16-B aligned and inside
// the run, so every element is updated exactly once.
static const int kAdamSlabMax = 56;       // descriptors per launch (the tables are kernel arguments)
static const int kAdamPlainChunk = 4096;  // floats per plain block
struct AdamSlabArgs {
  rtsds_split_reduce_desc d[kAdamSlabMax];  // ascending dw
  int blk0[kAdamSlabMax];                   // first slab block of descriptor i
  int gap_lo[kAdamSlabMax + 1], gap_hi[kAdamSlabMax + 1];  // non-empty gaps [lo, hi), floats from the run's base
  int gblk0[kAdamSlabMax + 1];              // first plain block of gap i, counted from slab_blocks
  int n, ngaps, slab_blocks;
};
static_assert(sizeof(AdamSlabArgs) <= 3840, "AdamSlabArgs must fit the kernel argument segment with the pointers");
__global__ void __launch_bounds__(256) adam_slabs_kernel(const AdamSlabArgs a, float* __restrict__ p, float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, bf16* __restrict__ shadow,
                                                         const float* __restrict__ hyper, float b1, float b2, float eps, float wd,
                                                         float gscale) {
  __shared__ float red[4][64][4];
  const float lr = hyper[0], bc1 = hyper[1], bc2_sqrt = hyper[2];
  const float step = lr / bc1;
  const int b = blockIdx.x;
  if (b < a.slab_blocks) {
    int si = 0;
    for (int i = 1; i < a.n; ++i)
      if (a.blk0[i] <= b) si = i;
    const rtsds_split_reduce_desc& q = a.d[si];
    const int lane = threadIdx.x & 63, sg = threadIdx.x >> 6;
    const int i = (b - a.blk0[si]) * 64 + lane;
    float t[4];
    split_reduce_block(q, i, red, t);
    if (sg != 0 || i >= q.nv) return;
    const long off = (q.dw - g) + (long)i * 4;
    if (q.accumulate & 1) {  // the arena holds an earlier contribution: added first, as the reduce does
      const f32x4 o = *(const f32x4*)(g + off);
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = o[e] + t[e];
    }
    if (q.accumulate & RTSDS_SLAB_KEEP_GRAD) *(f32x4*)(g + off) = f32x4{t[0], t[1], t[2], t[3]};
    f32x4 pv = *(const f32x4*)(p + off), mv = *(const f32x4*)(m + off), vv = *(const f32x4*)(v + off);
    bf16x4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pi = pv[e], mi = mv[e], vi = vv[e];
      adam_elem(pi, t[e] * gscale, mi, vi, step, b1, b2, eps, wd, bc2_sqrt);
      pv[e] = pi; mv[e] = mi; vv[e] = vi;
      h[e] = (bf16)pi;
    }
    *(f32x4*)(m + off) = mv;
    *(f32x4*)(v + off) = vv;
    *(f32x4*)(p + off) = pv;
    if (shadow) *(bf16x4*)(shadow + off) = h;
    return;
  }
  const int pb = b - a.slab_blocks;
  int gi = 0;
  for (int i = 1; i < a.ngaps; ++i)
    if (a.gblk0[i] <= pb) gi = i;
  const long lo = a.gap_lo[gi] + (long)(pb - a.gblk0[gi]) * kAdamPlainChunk;  // (gap_lo: a multiple of 4)
  const long hi = min((long)a.gap_hi[gi], lo + kAdamPlainChunk);
  for (long e0 = lo + 4 * (long)threadIdx.x; e0 < hi; e0 += 4 * 256) {
    if (e0 + 4 <= hi) {
      const f32x4 gv = *(const f32x4*)(g + e0);
      f32x4 pv = *(const f32x4*)(p + e0), mv = *(const f32x4*)(m + e0), vv = *(const f32x4*)(v + e0);
      bf16x4 h;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pi = pv[e], mi = mv[e], vi = vv[e];
        adam_elem(pi, gv[e] * gscale, mi, vi, step, b1, b2, eps, wd, bc2_sqrt);
        pv[e] = pi; mv[e] = mi; vv[e] = vi;
        h[e] = (bf16)pi;
      }
      *(f32x4*)(m + e0) = mv;
      *(f32x4*)(v + e0) = vv;
      *(f32x4*)(p + e0) = pv;
      if (shadow) *(bf16x4*)(shadow + e0) = h;
    } else {
      for (long i = e0; i < hi; ++i) {  // the run's last 1..3 elements
        float pi = p[i], mi = m[i], vi = v[i];
        adam_elem(pi, g[i] * gscale, mi, vi, step, b1, b2, eps, wd, bc2_sqrt);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
        if (shadow) shadow[i] = (bf16)pi;
      }
    }
  }
}
extern "C" int rtsds_adam_step_slabs(float* param, float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_shadow, long n,
                                     const float* hyper, float beta1, float beta2, float eps, float weight_decay,
                                     float grad_scale, int grad_dtype, int n_descs, const rtsds_split_reduce_desc* descs,
                                     int max_descs, void* stream) {
  if (n <= 0 || !hyper || !param || !grad || !exp_avg || !exp_avg_sq || n_descs < 0 || (n_descs && !descs) || max_descs < 0)
    return RTSDS_ERR_SHAPE;
  const int cap = max_descs ? std::min(max_descs, kAdamSlabMax) : kAdamSlabMax;
  if (grad_dtype != RTSDS_F32 || n_descs > cap || n >= INT_MAX - kAdamPlainChunk) return RTSDS_ERR_UNSUPPORTED;
  if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) || ((uintptr_t)bf16_shadow & 7))
    return RTSDS_ERR_UNSUPPORTED;
  AdamSlabArgs a;
  a.n = n_descs;
  a.ngaps = 0;
  long sblocks = 0, pblocks = 0, at = 0;  // at: end of the last hole
  auto gap = [&](long lo, long hi) {
    if (hi <= lo) return;
    a.gap_lo[a.ngaps] = (int)lo;
    a.gap_hi[a.ngaps] = (int)hi;
    a.gblk0[a.ngaps] = (int)pblocks;
    pblocks += (hi - lo + kAdamPlainChunk - 1) / kAdamPlainChunk;
    ++a.ngaps;
  };
  for (int i = 0; i < n_descs; ++i) {
    const rtsds_split_reduce_desc& q = descs[i];
    if (q.nv <= 0 || q.cv <= 0 || q.splits <= 0 || !q.slab || !q.dw) return RTSDS_ERR_SHAPE;
    if (((uintptr_t)q.dw & 15) || ((uintptr_t)q.slab & 15) || (q.slab_stride & 3) || (q.cp & 3)) return RTSDS_ERR_UNSUPPORTED;
    const long lo = q.dw - grad, hi = lo + 4L * q.nv;
    if (q.dw < grad || lo < at || hi > n) return RTSDS_ERR_SHAPE;  // outside the run, unsorted or overlapping
    a.d[i] = q;
    a.blk0[i] = (int)sblocks;
    sblocks += (q.nv + 63) / 64;
    gap(at, lo);
    at = hi;
  }
  gap(at, n);
  if (sblocks + pblocks > INT_MAX) return RTSDS_ERR_UNSUPPORTED;
  a.slab_blocks = (int)sblocks;
  hipLaunchKernelGGL(adam_slabs_kernel, dim3((unsigned)(sblocks + pblocks)), dim3(256), 0, (hipStream_t)stream, a, param, grad,
                     exp_avg, exp_avg_sq, (bf16*)bf16_shadow, hyper, beta1, beta2, eps, weight_decay, grad_scale);
  RET_LAUNCH();
}

// Zero fill of count ranges [lo[i], hi[i]) (floats) of one buffer in one launch per 128 ranges: the
// optimizer's zero_grad over the gradient ranges written since the last one.
static const int kZeroRanges = 128, kZeroChunk = 4096;
struct ZeroRangeArgs {
  long lo[kZeroRanges];
  int len[kZeroRanges], blk0[kZeroRanges];
  int n;
};
__global__ void __launch_bounds__(256) zero_ranges_kernel(const ZeroRangeArgs a, float* __restrict__ buf) {
  int ri = 0;
  for (int i = 1; i < a.n; ++i)
    if (a.blk0[i] <= (int)blockIdx.x) ri = i;
  const int r0 = ((int)blockIdx.x - a.blk0[ri]) * kZeroChunk, r1 = min(a.len[ri], r0 + kZeroChunk);
  float* o = buf + a.lo[ri] + r0;  // (r0: a multiple of 4)
  const int n = r1 - r0, nv = ((uintptr_t)o & 15) == 0 ? n >> 2 : 0;
  for (int i = threadIdx.x; i < nv; i += 256) ((f32x4*)o)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = 4 * nv + threadIdx.x; i < n; i += 256) o[i] = 0.f;
}
extern "C" int rtsds_zero_ranges(float* buf, int count, const long* lo, const long* hi, void* stream) {
  if (count < 0 || (count && (!buf || !lo || !hi))) return RTSDS_ERR_SHAPE;
  for (int i = 0; i < count; ++i)
    if (lo[i] < 0 || hi[i] < lo[i] || hi[i] - lo[i] > INT_MAX - kZeroChunk) return RTSDS_ERR_SHAPE;
  for (int i0 = 0; i0 < count; i0 += kZeroRanges) {
    ZeroRangeArgs a;
    a.n = 0;
    long blocks = 0;
    for (int i = i0; i < count && i < i0 + kZeroRanges; ++i) {
      if (hi[i] == lo[i]) continue;
      a.lo[a.n] = lo[i];
      a.len[a.n] = (int)(hi[i] - lo[i]);
      a.blk0[a.n] = (int)blocks;
      blocks += (hi[i] - lo[i] + kZeroChunk - 1) / kZeroChunk;
      ++a.n;
    }
    if (blocks > INT_MAX) return RTSDS_ERR_UNSUPPORTED;
    if (a.n) hipLaunchKernelGGL(zero_ranges_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, buf);
  }
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
