// Input pipeline on the device (reference main.py:60-108, datasets/cityscapes.py:56-68,
// datasets/gta5.py:69-118): the per-sample torchvision transforms the reference runs on CPU
// DataLoader workers, here on a decoded uint8 image already in HBM.
//
//   resize   torchvision Resize(size) on a tensor = F.interpolate(bilinear, align_corners=False,
//            antialias=True) on the float image (integer tensors -- labels -- are interpolated
//            in float, rounded half-to-even and cast back).  ATen's separable antialias
//            resampler: triangle filter of support scale (scale = in/out when downscaling, 1
//            otherwise), horizontal pass first into an fp32 [H][Wo][C] intermediate, then the
//            vertical pass; weights normalised per output index.  Fused into the passes:
//            horizontal flip (RandomHorizontalFlip: the source is read mirrored), Normalize
//            ((v - mean) / std, on the reference's 0-255 scale), IntRangeTransformer clamp
//            (utils.py:67-75), and the NHWC compute-dtype store the network reads.
//   crop     RandomResizedCrop's window, drawn on the host: the resize reads the window of the
//            source image in place (same bits as the resize of a contiguous copy); the label
//            takes the same window through a nearest resample, so no class id is invented.
//   blur     GaussianBlur(kernel_size, sigma): the separable Gaussian of torchvision applied as
//            its 2-D outer-product kernel with reflect padding.
//   jitter   ColorJitter(brightness, contrast, saturation, hue) in the permutation drawn per
//            call, all adjustments in one pass over registers; contrast's grey mean comes
//            from a reduction launch in front of it.
//   decode   GTA5 RGB label -> train id (gta5.py:111-118: every pixel whose colour equals the
//            colour of train id i gets i, others 0).
//
// Images arrive as decoded HWC uint8 (PIL's layout); every kernel is HBM-bound elementwise /
// small-stencil work (one thread per output element, coalesced over the channel-inner layout).
#include "common.h"
#include <algorithm>
#include <cmath>

static const int kAaMaxTaps = 64;  // support up to a 31x downscale

// Antialias weights of one axis (ATen _compute_weights_aa, bilinear filter): xmin / xsize of
// output index o and its normalised weights.
__global__ void aa_weights_kernel(int in, int out, int ktaps, int* __restrict__ xmin, int* __restrict__ xsize,
                                  float* __restrict__ wt) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= out) return;
  // the float / double mix of ATen's expressions, kept exactly (weights identical to the CPU's)
  const float scale = (float)in / (float)out;
  const float support = scale >= 1.f ? (float)(1.0 * (double)scale) : 1.f;
  const float invscale = scale >= 1.f ? (float)(1.0 / (double)scale) : 1.f;
  const float center = (float)((double)scale * ((double)o + 0.5));
  const int lo = std::max((int)((double)center - (double)support + 0.5), 0);
  const int sz = std::min((int)((double)center + (double)support + 0.5), in) - lo;
  float w[kAaMaxTaps];
  float total = 0.f;
  for (int j = 0; j < ktaps; ++j) {
    float v = 0.f;
    if (j < sz) {
      float x = (float)(((double)(j + lo) - (double)center + 0.5) * (double)invscale);
      x = fabsf(x);
      v = x < 1.f ? 1.f - x : 0.f;
    }
    w[j] = v;
    total += v;
  }
  for (int j = 0; j < ktaps; ++j) wt[(long)o * ktaps + j] = total != 0.f && j < sz ? w[j] / total : 0.f;
  xmin[o] = lo;
  xsize[o] = sz;
}

// horizontal pass: tmp[y][xo][c] = sum_j w[xo][j] src[y][x(xmin + j)][c], x mirrored when flip.
// src points at the first pixel of an h x w window whose rows lie `pitch` elements apart (w * c
// for a whole image, the source image's row for a crop read in place).
template <typename S>
__global__ void aa_h_kernel(const S* __restrict__ src, long pitch, float* __restrict__ tmp, int h, int w, int c, int wo,
                            int ktaps, const int* __restrict__ xmin, const int* __restrict__ xsize,
                            const float* __restrict__ wt, int flip) {
  const long total = (long)h * wo * c;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(e % c);
    const long r = e / c;
    const int xo = (int)(r % wo), y = (int)(r / wo);
    const int lo = xmin[xo], sz = xsize[xo];
    const float* ww = wt + (long)xo * ktaps;
    const S* row = src + (long)y * pitch + ch;
    float acc = 0.f;
    for (int j = 0; j < sz; ++j) {
      const int x = flip ? w - 1 - (lo + j) : lo + j;
      acc = j == 0 ? (float)row[(long)x * c] * ww[0] : fmaf((float)row[(long)x * c], ww[j], acc);
    }
    tmp[e] = acc;
  }
}

// vertical pass + epilogue.  kind 0: f32 NHWC, 1: bf16 NHWC (normalised when mean/std given);
// 2: int64 label (round half-to-even, clamp to [lo, hi] when lo <= hi)
__global__ void aa_v_kernel(const float* __restrict__ tmp, void* __restrict__ dst, int h, int wo, int c, int ho, int ktaps,
                            const int* __restrict__ ymin, const int* __restrict__ ysize, const float* __restrict__ wt,
                            int kind, const float* __restrict__ mean, const float* __restrict__ stdv, int clamp_lo,
                            int clamp_hi) {
  const long total = (long)ho * wo * c;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(e % c);
    const long r = e / c;
    const int xo = (int)(r % wo), yo = (int)(r / wo);
    const int lo = ymin[yo], sz = ysize[yo];
    const float* ww = wt + (long)yo * ktaps;
    const float* col = tmp + (long)xo * c + ch;
    float acc = 0.f;
    for (int i = 0; i < sz; ++i) {
      const float t = col[(long)(lo + i) * wo * c];
      acc = i == 0 ? t * ww[0] : fmaf(t, ww[i], acc);
    }
    if (kind == 2) {
      long v = (long)rintf(acc);
      if (clamp_lo <= clamp_hi) v = std::min<long>(std::max<long>(v, clamp_lo), clamp_hi);
      ((int64_t*)dst)[e] = v;
    } else {
      if (mean) acc = (acc - mean[ch]) / stdv[ch];
      if (kind == 1) ((bf16*)dst)[e] = (bf16)acc;
      else ((float*)dst)[e] = acc;
    }
  }
}

static int aa_taps(int in, int out) {
  const float scale = (float)in / (float)out;
  const float support = scale >= 1.f ? (float)(1.0 * (double)scale) : 1.f;
  return (int)std::ceil(support) * 2 + 1;
}

static size_t al256(size_t b) { return (b + 255) / 256 * 256; }

extern "C" size_t rtsds_resize_aa_workspace(int c, int h, int w, int ho, int wo) {
  if (c <= 0 || h <= 0 || w <= 0 || ho <= 0 || wo <= 0) return 0;
  const int kx = aa_taps(w, wo), ky = aa_taps(h, ho);
  return al256((size_t)h * wo * c * 4) + al256((size_t)(wo + ho) * 8) + al256((size_t)(wo * kx + ho * ky) * 4);
}

// The resize of the h x w window at `src` (row pitch in elements); both entries below validate
// and hand over here, so a crop takes the launches, grids and arithmetic of a whole image.
static int aa_resize_window(const void* src, int src_u8, long pitch, int c, int h, int w, void* dst, int kind, int ho, int wo,
                            int flip, const float* mean, const float* stdv, int clamp_lo, int clamp_hi, void* ws,
                            size_t ws_bytes, void* stream) {
  if ((mean == nullptr) != (stdv == nullptr)) return RTSDS_ERR_SHAPE;
  const int kx = aa_taps(w, wo), ky = aa_taps(h, ho);
  if (kx > kAaMaxTaps || ky > kAaMaxTaps) return RTSDS_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < rtsds_resize_aa_workspace(c, h, w, ho, wo)) return RTSDS_ERR_WORKSPACE;
  char* p = (char*)ws;
  float* tmp = (float*)p;
  p += al256((size_t)h * wo * c * 4);
  int* xmin = (int*)p;
  int* xsz = xmin + wo;
  int* ymin = xsz + wo;
  int* ysz = ymin + ho;
  p += al256((size_t)(wo + ho) * 8);
  float* wx = (float*)p;
  float* wy = wx + (size_t)wo * kx;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(aa_weights_kernel, dim3(rt_cdiv(wo, 256)), dim3(256), 0, st, w, wo, kx, xmin, xsz, wx);
  hipLaunchKernelGGL(aa_weights_kernel, dim3(rt_cdiv(ho, 256)), dim3(256), 0, st, h, ho, ky, ymin, ysz, wy);
  const long nh = (long)h * wo * c, nv = (long)ho * wo * c;
  const int bh = (int)std::min<long>(8192, (nh + 255) / 256), bv = (int)std::min<long>(8192, (nv + 255) / 256);
  if (src_u8)
    hipLaunchKernelGGL(aa_h_kernel<uint8_t>, dim3(bh), dim3(256), 0, st, (const uint8_t*)src, pitch, tmp, h, w, c, wo, kx,
                       xmin, xsz, wx, flip);
  else
    hipLaunchKernelGGL(aa_h_kernel<float>, dim3(bh), dim3(256), 0, st, (const float*)src, pitch, tmp, h, w, c, wo, kx, xmin,
                       xsz, wx, flip);
  hipLaunchKernelGGL(aa_v_kernel, dim3(bv), dim3(256), 0, st, tmp, dst, h, wo, c, ho, ky, ymin, ysz, wy, kind, mean, stdv,
                     clamp_lo, clamp_hi);
  RET_LAUNCH();
}

extern "C" int rtsds_resize_aa(const void* src, int src_u8, int c, int h, int w, void* dst, int kind, int ho, int wo,
                               int flip, const float* mean, const float* stdv, int clamp_lo, int clamp_hi, void* ws,
                               size_t ws_bytes, void* stream) {
  if (c <= 0 || h <= 0 || w <= 0 || ho <= 0 || wo <= 0 || kind < 0 || kind > 2 || !src || !dst) return RTSDS_ERR_SHAPE;
  return aa_resize_window(src, src_u8, (long)w * c, c, h, w, dst, kind, ho, wo, flip, mean, stdv, clamp_lo, clamp_hi, ws,
                          ws_bytes, stream);
}

// a window [y0, y0 + hc) x [x0, x0 + wc) inside [0, h) x [0, w), without overflow in the sums
static bool window_inside(int h, int w, int y0, int x0, int hc, int wc) {
  return h > 0 && w > 0 && hc > 0 && wc > 0 && y0 >= 0 && x0 >= 0 && hc <= h && wc <= w && y0 <= h - hc && x0 <= w - wc;
}

// ---- crop + resize: the resize of src[y0 : y0 + hc, x0 : x0 + wc, :] read in place ----
// (RandomResizedCrop ahead of Resize: the same bits as rtsds_resize_aa on a contiguous copy of
// the window -- the weights come from (hc, wc), the kernels only see another origin and pitch)
extern "C" int rtsds_crop_resize_aa(const void* src, int src_u8, int c, int h, int w, int y0, int x0, int hc, int wc, void* dst,
                                    int kind, int ho, int wo, int flip, const float* mean, const float* stdv, int clamp_lo,
                                    int clamp_hi, void* ws, size_t ws_bytes, void* stream) {
  if (c <= 0 || ho <= 0 || wo <= 0 || kind < 0 || kind > 2 || !src || !dst) return RTSDS_ERR_SHAPE;
  if (!window_inside(h, w, y0, x0, hc, wc)) return RTSDS_ERR_SHAPE;
  const size_t origin = ((size_t)y0 * w + x0) * c;
  const void* win = src_u8 ? (const void*)((const uint8_t*)src + origin) : (const void*)((const float*)src + origin);
  return aa_resize_window(win, src_u8, (long)w * c, c, hc, wc, dst, kind, ho, wo, flip, mean, stdv, clamp_lo, clamp_hi, ws,
                          ws_bytes, stream);
}

// nearest resample of a label window (ATen upsample_nearest2d's index rule: floor(o * in / out)
// in fp32, capped at in - 1); flip writes the mirror of the unflipped result (output column xo
// takes the source column of wo - 1 - xo: the floor rule is not symmetric, so mirroring the
// window first would pick other pixels); clamped when lo <= hi
template <typename S>
__global__ void crop_nearest_kernel(const S* __restrict__ src, int w, int y0, int x0, int hc, int wc,
                                    int64_t* __restrict__ dst, int ho, int wo, int flip, int clamp_lo, int clamp_hi) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= (long)ho * wo) return;
  const int xo = (int)(e % wo), yo = (int)(e / wo);
  const float sh = (float)hc / (float)ho, sw = (float)wc / (float)wo;
  const int sy = std::min((int)floorf((float)yo * sh), hc - 1);
  const int sx = std::min((int)floorf((float)(flip ? wo - 1 - xo : xo) * sw), wc - 1);
  long v = (long)src[(long)(y0 + sy) * w + (x0 + sx)];
  if (clamp_lo <= clamp_hi) v = std::min<long>(std::max<long>(v, clamp_lo), clamp_hi);
  dst[e] = v;
}

extern "C" int rtsds_crop_resize_nearest(const void* src, int src_i64, int h, int w, int y0, int x0, int hc, int wc,
                                         int64_t* dst, int ho, int wo, int flip, int clamp_lo, int clamp_hi, void* stream) {
  if (ho <= 0 || wo <= 0 || !src || !dst) return RTSDS_ERR_SHAPE;
  if (!window_inside(h, w, y0, x0, hc, wc)) return RTSDS_ERR_SHAPE;
  const long n = (long)ho * wo;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (src_i64)
    hipLaunchKernelGGL(crop_nearest_kernel<int64_t>, grid, dim3(256), 0, (hipStream_t)stream, (const int64_t*)src, w, y0, x0,
                       hc, wc, dst, ho, wo, flip, clamp_lo, clamp_hi);
  else
    hipLaunchKernelGGL(crop_nearest_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, w, y0, x0,
                       hc, wc, dst, ho, wo, flip, clamp_lo, clamp_hi);
  RET_LAUNCH();
}

// ---- GaussianBlur: dst = conv2d(reflect_pad(src), outer(ky, kx)) per channel, HWC fp32 ----
// (torchvision gaussian_blur: 1-D kernels pdf(x) = exp(-0.5 (x / sigma)^2) over
// x = -(k-1)/2 .. (k-1)/2, normalised; 2-D kernel = ky^T kx; reflect padding k // 2)
__global__ void gblur_kernel(const void* __restrict__ src, int src_u8, float* __restrict__ dst, int h, int w, int c, int kx,
                             int ky, float sx, float sy) {
  __shared__ float kxw[32], kyw[32];
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < kx; ++i) {
      const float x = -(float)(kx - 1) * 0.5f + (float)i;
      kxw[i] = expf(-0.5f * (x / sx) * (x / sx));
      t += kxw[i];
    }
    for (int i = 0; i < kx; ++i) kxw[i] /= t;
    t = 0.f;
    for (int i = 0; i < ky; ++i) {
      const float y = -(float)(ky - 1) * 0.5f + (float)i;
      kyw[i] = expf(-0.5f * (y / sy) * (y / sy));
      t += kyw[i];
    }
    for (int i = 0; i < ky; ++i) kyw[i] /= t;
  }
  __syncthreads();
  const int px = kx / 2, py = ky / 2;
  const long total = (long)h * w * c;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(e % c);
    const long r = e / c;
    const int x = (int)(r % w), y = (int)(r / w);
    float acc = 0.f;
    for (int i = 0; i < ky; ++i) {
      int yy = y - py + i;
      yy = yy < 0 ? -yy : (yy >= h ? 2 * h - 2 - yy : yy);
      for (int j = 0; j < kx; ++j) {
        int xx = x - px + j;
        xx = xx < 0 ? -xx : (xx >= w ? 2 * w - 2 - xx : xx);
        const long o = ((long)yy * w + xx) * c + ch;
        const float v = src_u8 ? (float)((const uint8_t*)src)[o] : ((const float*)src)[o];
        acc = fmaf(v, kyw[i] * kxw[j], acc);
      }
    }
    dst[e] = acc;
  }
}

extern "C" int rtsds_gaussian_blur(const void* src, int src_u8, float* dst, int c, int h, int w, int kx, int ky, float sigma_x,
                                   float sigma_y, void* stream) {
  if (c <= 0 || h <= 0 || w <= 0 || kx <= 0 || ky <= 0 || kx % 2 == 0 || ky % 2 == 0 || kx > 31 || ky > 31) return RTSDS_ERR_SHAPE;
  if (kx / 2 >= w || ky / 2 >= h || !(sigma_x > 0.f) || !(sigma_y > 0.f)) return RTSDS_ERR_SHAPE;
  const long n = (long)h * w * c;
  hipLaunchKernelGGL(gblur_kernel, dim3((int)std::min<long>(8192, (n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src,
                     src_u8, dst, h, w, c, kx, ky, sigma_x, sigma_y);
  RET_LAUNCH();
}

// ---- ColorJitter(brightness, contrast, saturation, hue): HWC c = 3, uint8 or fp32 -> fp32 HWC ----
// (torchvision adjust_brightness / _contrast / _saturation / _hue on a float image in
// [0, bound], applied in the permutation drawn per call; the host passes the enabled ops already
// in application order.  Contrast blends with the mean grey of the image as it stands when
// contrast is applied, so with contrast on a first launch reduces gray(prefix(p)) into one
// partial per block, and every block of the apply launch adds those partials in a fixed order.)
static const int kCjMaxParts = 1024;  // grid cap of the reduction = partials in the workspace
static const int kCjPix = 4;          // consecutive pixels per thread: 12 B uint8 / 3 x 16 B fp32

struct CjOps {
  int n;     // enabled ops, in application order
  int cpos;  // index of contrast among them, -1 when off
  int id[4];
  float f[4];
  float bound, inv_bound;
};

RT_DEV float cj_gray(float r, float g, float b) { return fmaf(0.114f, b, fmaf(0.587f, g, 0.2989f * r)); }
RT_DEV float cj_clamp(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }
// blend(a, b, f) = clamp(f a + (1 - f) b); fb = (1 - f) b is the same for the three channels
RT_DEV float cj_blend(float a, float fb, float f, float bound) { return cj_clamp(fmaf(f, a, fb), bound); }

RT_DEV void cj_hue(float& r, float& g, float& b, float fh, float bound, float inv_bound) {
  r *= inv_bound;
  g *= inv_bound;
  b *= inv_bound;
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eq = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eq ? 1.f : maxc);
  const float crd = eq ? 1.f : cr;
  // h = bc - gc | 2 + rc - bc | 4 + gc - rc with xc = (maxc - x) / crd: only two quotients are used
  const bool mr = maxc == r, mg = maxc == g;
  const float x = mr ? b : (mg ? r : g), y = mr ? g : (mg ? b : r);
  const float off = mr ? 0.f : (mg ? 2.f : 4.f);
  float h = (off + (maxc - x) / crd) - (maxc - y) / crd;
  h = h / 6.f + 1.f;
  h -= floorf(h);  // fmod(h, 1), h > 0
  h += fh;
  h -= floorf(h);  // floor-mod
  const float h6 = h * 6.f, fi = floorf(h6), f = h6 - fi;
  int i = (int)fi;
  i = i >= 6 ? i - 6 : i;
  const float v = maxc;
  const float p_ = cj_clamp(v * (1.f - s), 1.f), q_ = cj_clamp(v * (1.f - f * s), 1.f),
              t_ = cj_clamp(v * (1.f - (1.f - f) * s), 1.f);
  r = (i == 0 || i == 5 ? v : (i == 1 ? q_ : (i == 4 ? t_ : p_))) * bound;
  g = (i == 1 || i == 2 ? v : (i == 0 ? t_ : (i == 3 ? q_ : p_))) * bound;
  b = (i == 3 || i == 4 ? v : (i == 2 ? t_ : (i == 5 ? q_ : p_))) * bound;
}

// The first `count` ops of the order on N pixels in registers (a = r g b r g b ...); m = mean
// grey for contrast.  The reduction calls it with count = cpos, the apply kernel with count = n:
// the same instructions on the same values per pixel (explicit fma, branches uniform over the
// launch), so the mean is the mean of what the apply kernel recomputes.  The ops are the outer
// loop: one read of the op and one branch serve the N independent pixels.
template <int N>
RT_DEV void cj_prefix(float* a, const CjOps& o, int count, float m) {
  for (int k = 0; k < count; ++k) {
    const int id = o.id[k];
    const float f = o.f[k];
    if (id == 3) {
#pragma unroll
      for (int j = 0; j < N; ++j) cj_hue(a[3 * j], a[3 * j + 1], a[3 * j + 2], f, o.bound, o.inv_bound);
      continue;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float other = 0.f;  // brightness: blend with black
      if (id == 1) other = m;
      if (id == 2) other = cj_gray(a[3 * j], a[3 * j + 1], a[3 * j + 2]);
      const float fb = (1.f - f) * other;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) a[3 * j + ch] = cj_blend(a[3 * j + ch], fb, f, o.bound);
    }
  }
}

// kCjPix consecutive pixels (12 values) of group gi.  VEC: three dwords of uint8 / three 16-B
// vectors of fp32 (the host checks the base alignment); else scalar loads.
template <typename S, bool VEC>
RT_DEV void cj_load(const S* src, long gi, float a[12]) {
  if constexpr (VEC && sizeof(S) == 1) {
    const uint32_t* p = (const uint32_t*)src + gi * 3;
    const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = (float)((w0 >> (8 * j)) & 255u);
      a[4 + j] = (float)((w1 >> (8 * j)) & 255u);
      a[8 + j] = (float)((w2 >> (8 * j)) & 255u);
    }
  } else if constexpr (VEC) {
    const f32x4* p = (const f32x4*)src + gi * 3;
    const f32x4 v0 = p[0], v1 = p[1], v2 = p[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = v0[j];
      a[4 + j] = v1[j];
      a[8 + j] = v2[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j) a[j] = (float)src[gi * 12 + j];
  }
}

// launch 1 (contrast on): part[block] = sum over the block's pixels of gray(prefix(p))
template <typename S, bool VEC>
__global__ void __launch_bounds__(256) cj_mean_kernel(const S* src, float* __restrict__ part, long npix, CjOps o) {
  __shared__ float wsum[4];
  const long ngroups = npix / kCjPix;
  float acc = 0.f;
  for (long gi = blockIdx.x * (long)blockDim.x + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * blockDim.x) {
    float a[12];
    cj_load<S, VEC>(src, gi, a);
    cj_prefix<kCjPix>(a, o, o.cpos, 0.f);
#pragma unroll
    for (int j = 0; j < kCjPix; ++j) acc += cj_gray(a[3 * j], a[3 * j + 1], a[3 * j + 2]);
  }
  const long tail = ngroups * kCjPix + threadIdx.x;  // the last npix % kCjPix pixels: block 0
  if (blockIdx.x == 0 && tail < npix) {
    float p[3] = {(float)src[tail * 3], (float)src[tail * 3 + 1], (float)src[tail * 3 + 2]};
    cj_prefix<1>(p, o, o.cpos, 0.f);
    acc += cj_gray(p[0], p[1], p[2]);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// launch 2: m = (sum of the partials in fp64, a fixed order) / npix in every block, then all
// ops on the block's pixels.  src may be dst (fp32): a thread reads its pixels before it stores.
template <typename S, bool VEC>
__global__ void __launch_bounds__(256) cj_apply_kernel(const S* src, float* dst, long npix, const float* __restrict__ part,
                                                       int nparts, CjOps o) {
  __shared__ double chunk[64];
  __shared__ float mean;
  float m = 0.f;
  if (o.cpos >= 0) {
    // lane l of wave 0 adds partials [16 l, 16 l + 16) in index order, thread 0 the 64 sums in
    // index order: the same association in every block and every run
    if (threadIdx.x < 64) {
      double t = 0.0;
      for (int i = threadIdx.x * (kCjMaxParts / 64); i < (threadIdx.x + 1) * (kCjMaxParts / 64); ++i)
        if (i < nparts) t += (double)part[i];
      chunk[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int i = 0; i < 64; ++i) t += chunk[i];
      mean = (float)(t / (double)npix);
    }
    __syncthreads();
    m = mean;
  }
  const long ngroups = npix / kCjPix;
  for (long gi = blockIdx.x * (long)blockDim.x + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * blockDim.x) {
    float a[12];
    cj_load<S, VEC>(src, gi, a);
    cj_prefix<kCjPix>(a, o, o.n, m);
    if constexpr (VEC) {
      f32x4* q = (f32x4*)dst + gi * 3;
      q[0] = f32x4{a[0], a[1], a[2], a[3]};
      q[1] = f32x4{a[4], a[5], a[6], a[7]};
      q[2] = f32x4{a[8], a[9], a[10], a[11]};
    } else {
#pragma unroll
      for (int j = 0; j < 12; ++j) dst[gi * 12 + j] = a[j];
    }
  }
  const long tail = ngroups * kCjPix + threadIdx.x;
  if (blockIdx.x == 0 && tail < npix) {
    float p[3] = {(float)src[tail * 3], (float)src[tail * 3 + 1], (float)src[tail * 3 + 2]};
    cj_prefix<1>(p, o, o.n, m);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) dst[tail * 3 + ch] = p[ch];
  }
}

static int cj_parts(long npix) {
  return (int)std::max<long>(1, std::min<long>(kCjMaxParts, (npix / kCjPix + 255) / 256));
}

template <typename S, bool VEC>
static void cj_launch(const void* src, float* dst, long npix, float* part, const CjOps& o, hipStream_t st) {
  const int nparts = cj_parts(npix);
  if (o.cpos >= 0)
    hipLaunchKernelGGL((cj_mean_kernel<S, VEC>), dim3(nparts), dim3(256), 0, st, (const S*)src, part, npix, o);
  const int blocks = (int)std::max<long>(1, std::min<long>(2048, (npix / kCjPix + 255) / 256));
  hipLaunchKernelGGL((cj_apply_kernel<S, VEC>), dim3(blocks), dim3(256), 0, st, (const S*)src, dst, npix, part, nparts, o);
}

extern "C" size_t rtsds_color_jitter_workspace(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  return al256((size_t)cj_parts((long)h * w) * sizeof(float));
}

extern "C" int rtsds_color_jitter(const void* src, int src_u8, float* dst, int c, int h, int w, const int* order, int mask,
                                  float fb, float fc, float fs, float fh, float bound, void* ws, size_t ws_bytes,
                                  void* stream) {
  if (c <= 0 || h <= 0 || w <= 0 || !src || !dst || !order || mask < 0 || mask > 15) return RTSDS_ERR_SHAPE;
  int seen = 0;
  for (int k = 0; k < 4; ++k) {
    if (order[k] < 0 || order[k] > 3 || (seen >> order[k] & 1)) return RTSDS_ERR_SHAPE;
    seen |= 1 << order[k];
  }
  if (!(fb >= 0.f) || !(fc >= 0.f) || !(fs >= 0.f) || !(fh >= -0.5f && fh <= 0.5f) || !(bound > 0.f)) return RTSDS_ERR_SHAPE;
  if (c != 3) return RTSDS_ERR_UNSUPPORTED;
  const float factor[4] = {fb, fc, fs, fh};
  CjOps o = {0, -1, {0, 0, 0, 0}, {1.f, 1.f, 1.f, 1.f}, bound, 1.f / bound};
  for (int k = 0; k < 4; ++k) {  // the enabled ops in application order (none: dst = float(src))
    if (!(mask >> order[k] & 1)) continue;
    if (order[k] == 1) o.cpos = o.n;
    o.id[o.n] = order[k];
    o.f[o.n++] = factor[order[k]];
  }
  if (o.cpos >= 0 && (!ws || ws_bytes < rtsds_color_jitter_workspace(h, w))) return RTSDS_ERR_WORKSPACE;
  const long npix = (long)h * w;
  const bool vec = (uintptr_t)dst % 16 == 0 && (uintptr_t)src % (src_u8 ? 4 : 16) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (src_u8) {
    if (vec) cj_launch<uint8_t, true>(src, dst, npix, (float*)ws, o, st);
    else cj_launch<uint8_t, false>(src, dst, npix, (float*)ws, o, st);
  } else {
    if (vec) cj_launch<float, true>(src, dst, npix, (float*)ws, o, st);
    else cj_launch<float, false>(src, dst, npix, (float*)ws, o, st);
  }
  RET_LAUNCH();
}

// ---- GTA5 RGB label -> train id (gta5.py:111-118), HWC uint8 -> int64 ----
__constant__ unsigned char kTrainColors[19][3] = {
    {128, 64, 128}, {244, 35, 232}, {70, 70, 70},   {102, 102, 156}, {190, 153, 153}, {153, 153, 153}, {250, 170, 30},
    {220, 220, 0},  {107, 142, 35}, {152, 251, 152}, {70, 130, 180},  {220, 20, 60},   {255, 0, 0},     {0, 0, 142},
    {0, 0, 70},     {0, 60, 100},   {0, 80, 100},   {0, 0, 230},     {119, 11, 32}};
__global__ void gta5_decode_kernel(const uint8_t* __restrict__ rgb, int64_t* __restrict__ out, long npix) {
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
    const uint8_t r = rgb[p * 3], g = rgb[p * 3 + 1], b = rgb[p * 3 + 2];
    int64_t v = 0;
    for (int i = 0; i < 19; ++i)
      if (r == kTrainColors[i][0] && g == kTrainColors[i][1] && b == kTrainColors[i][2]) v = i;
    out[p] = v;
  }
}
extern "C" int rtsds_gta5_decode(const uint8_t* rgb, int64_t* out, int h, int w, void* stream) {
  if (h <= 0 || w <= 0 || !rgb || !out) return RTSDS_ERR_SHAPE;
  const long n = (long)h * w;
  hipLaunchKernelGGL(gta5_decode_kernel, dim3((int)std::min<long>(8192, (n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     rgb, out, n);
  RET_LAUNCH();
}
