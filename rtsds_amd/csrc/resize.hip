// Bilinear resize (align_corners=False), forward and backward, and the kernels fused onto it
// (gfx950): resize + softmax for the discriminator input, multi-scale / flip evaluation.
#include "ew_common.h"

// ------------------------------------------------------------------ bilinear (align_corners=False)
// bil_src (ATen source index, align_corners=False): common.h
// Forward: one thread per (output pixel, channel chunk of CH); the 4 taps and weights are
// computed once per chunk.  CH = 16-B vector when the channel layout allows it, else the whole
// pixel (c <= 64, e.g. the 19-class heads) or single channels.
template <typename T, int MODE>  // MODE 0: 16-B vectors, 1: whole pixel loop, 2: per channel
__global__ void bilinear_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int n, int hi, int wi, int c, int ho, int wo,
                                    float sh, float sw, int yld, int yoff) {
  constexpr int V = VecT<T>::N;
  const int cpp = MODE == 0 ? c / V : (MODE == 1 ? 1 : c);  // chunks per pixel
  const long total = (long)n * ho * wo * cpp;
  GRID_STRIDE(i, total) {
    const int chunk = (int)(i % cpp);
    long q = i / cpp;
    const int ow = (int)(q % wo); q /= wo;
    const int oh = (int)(q % ho);
    const int img = (int)(q / ho);
    int h0, h1, w0, w1;
    float lh0, lh1, lw0, lw1;
    bil_src(oh, sh, hi, h0, h1, lh0, lh1);
    bil_src(ow, sw, wi, w0, w1, lw0, lw1);
    const T* b = x + (long)img * hi * wi * c;
    const T* p00 = b + ((long)h0 * wi + w0) * c;
    const T* p01 = b + ((long)h0 * wi + w1) * c;
    const T* p10 = b + ((long)h1 * wi + w0) * c;
    const T* p11 = b + ((long)h1 * wi + w1) * c;
    T* o = y + ((((long)img * ho + oh) * wo) + ow) * yld + yoff;
    if (MODE == 0) {
      typedef typename VecT<T>::v16 V16;
      const int c0 = chunk * V;
      const V16 a = *(const V16*)(p00 + c0), bb = *(const V16*)(p01 + c0);
      const V16 cc = *(const V16*)(p10 + c0), dd = *(const V16*)(p11 + c0);
      V16 r;
#pragma unroll
      for (int j = 0; j < V; ++j)
        r[j] = from_f<T>(bil_mix(to_f(a[j]), to_f(bb[j]), to_f(cc[j]), to_f(dd[j]), lh0, lh1, lw0, lw1));
      *(V16*)(o + c0) = r;
    } else {
      const int cs = MODE == 1 ? 0 : chunk, ce = MODE == 1 ? c : chunk + 1;
      for (int ch = cs; ch < ce; ++ch)
        o[ch] = from_f<T>(bil_mix(to_f(p00[ch]), to_f(p01[ch]), to_f(p10[ch]), to_f(p11[ch]), lh0, lh1, lw0, lw1));
    }
  }
}

// Upsampling with 16-B channel vectors (the context-path resizes into the FFM concat): one thread
// per (image, source row h0, output column, channel vector) loads the 4 taps once, forms bil_mix's
// two horizontal blends and writes every output row whose top tap is h0 (bit-identical to MODE 0;
// the taps are gathered once per source row instead of once per output row).  s1 / s2 (optional,
// [n][c]): channel scales applied to each tap first, rounded to T after each as the stored
// rtsds_chscale_fwd outputs would be (BiSeNet's attention refinement, build_bisenet.py:42-53,
// 157-159, folded into the eval forward's resize: bit-identical to scale, scale, resize).
template <typename T, int U>
__global__ void __launch_bounds__(256) bilinear_fwd_group_vec_kernel(const T* __restrict__ x, T* __restrict__ y, int n, int hi,
                                                                     int wi, int c, int ho, int wo, float sh, float sw, int yld,
                                                                     int yoff, const T* __restrict__ s1, const T* __restrict__ s2) {
  constexpr int V = VecT<T>::N;
  typedef typename VecT<T>::v16 V16;
  // grid (column-vector blocks, n * hi): the source row and its output rows are block-uniform.
  // A thread takes U column vectors gridDim.x * 256 apart and issues all their tap loads before
  // any arithmetic (U x 4 loads in flight instead of 4 per thread-lifetime).
  const int cpp = c / V, nv = wo * cpp;
  const int img = blockIdx.y / hi, h0 = blockIdx.y - img * hi;
  const int oa = bil_first_ge(h0, sh, hi, ho), ob = bil_first_ge(h0 + 1, sh, hi, ho);
  const int h1 = h0 + (h0 < hi - 1 ? 1 : 0);
  if (oa >= ob) return;
  const int i0 = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  const T* xb = x + (long)img * hi * wi * c;
  V16 a[U], bb[U], cc[U], dd[U], k1[U], k2[U];
  float lw0[U], lw1[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = min(i0 + u * step, nv - 1);  // clamped: unconditional loads
    const int ow = i / cpp, chunk = i - ow * cpp;
    int w0, w1;
    bil_src(ow, sw, wi, w0, w1, lw0[u], lw1[u]);
    const T* b = xb + chunk * V;
    a[u] = *(const V16*)(b + ((long)h0 * wi + w0) * c);
    bb[u] = *(const V16*)(b + ((long)h0 * wi + w1) * c);
    cc[u] = *(const V16*)(b + ((long)h1 * wi + w0) * c);
    dd[u] = *(const V16*)(b + ((long)h1 * wi + w1) * c);
    if (s1) k1[u] = *(const V16*)(s1 + (long)img * c + chunk * V);
    if (s2) k2[u] = *(const V16*)(s2 + (long)img * c + chunk * V);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = i0 + u * step;
    if (i >= nv) break;
    const int ow = i / cpp, chunk = i - ow * cpp;
    auto tap = [&](T v, int j) {
      float f = to_f(v);
      if (s1) f = to_f(from_f<T>(f * to_f(k1[u][j])));
      if (s2) f = to_f(from_f<T>(f * to_f(k2[u][j])));
      return f;
    };
    float t0[V], t1[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      t0[j] = fmaf(lw1[u], tap(bb[u][j], j), lw0[u] * tap(a[u][j], j));
      t1[j] = fmaf(lw1[u], tap(dd[u][j], j), lw0[u] * tap(cc[u][j], j));
    }
    for (int oh = oa; oh < ob; ++oh) {
      int i0_, i1_;
      float lh0, lh1;
      bil_src(oh, sh, hi, i0_, i1_, lh0, lh1);
      V16 r;
#pragma unroll
      for (int j = 0; j < V; ++j) r[j] = from_f<T>(fmaf(lh1, t1[j], lh0 * t0[j]));
      *(V16*)(y + (((long)img * ho + oh) * wo + ow) * yld + yoff + chunk * V) = r;
    }
  }
}

// Narrow channel counts that are not a 16-B multiple (the 19-class logits of the eval forward's
// final x8 resize, build_bisenet.py:165-166): one workgroup per output row.  The row's two source
// rows are staged in LDS as fp32 (coalesced), then every thread writes whole 16-B vectors of the
// dense output row (a wave writes 1 KB contiguously; the whole-pixel loop wrote 38-B runs at a
// 38-B lane stride, 1.8 TB/s) from 4 LDS taps per element.  Same taps, weights and bil_mix
// expression as the other modes.
template <typename T>
__global__ void __launch_bounds__(256) bilinear_fwd_rows_kernel(const T* __restrict__ x, T* __restrict__ y, int hi, int wi, int c,
                                                                 int ho, int wo, float sh, float sw, FastDiv f_c) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  extern __shared__ float rows[];  // [2][wi * c]
  const int row = blockIdx.x, img = row / ho, oh = row - img * ho;
  int h0, h1;
  float lh0, lh1;
  bil_src(oh, sh, hi, h0, h1, lh0, lh1);
  const int rl = wi * c;
  const T* r0 = x + ((long)img * hi + h0) * rl;
  const T* r1 = x + ((long)img * hi + h1) * rl;
  for (int e = threadIdx.x; e < rl; e += 256) {
    rows[e] = to_f(r0[e]);
    rows[rl + e] = to_f(r1[e]);
  }
  __syncthreads();
  const int nv = wo * c / V;  // (wo * c) % V == 0 (host)
  T* yo = y + (long)row * wo * c;
  for (int v = threadIdx.x; v < nv; v += 256) {
    const int e = v * V;
    int ow = (int)fdiv((uint32_t)e, f_c), ch = e - ow * c;
    int w0, w1;
    float lw0, lw1;
    bil_src(ow, sw, wi, w0, w1, lw0, lw1);
    V16 r;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (ch == c) {
        ch = 0;
        ++ow;
        bil_src(ow, sw, wi, w0, w1, lw0, lw1);
      }
      const float* a = rows + w0 * c + ch;
      const float* b = rows + w1 * c + ch;
      r[k] = from_f<T>(bil_mix(a[0], b[0], a[rl], b[rl], lh0, lh1, lw0, lw1));
      ++ch;
    }
    *(V16*)(yo + e) = r;
  }
}

// The same resize for upsampling, one workgroup per (image, source row h0, column chunk): every
// output row whose top tap is h0 blends the same two horizontal blends t0 / t1 (bil_mix's inner
// terms), so each thread computes them once for its J output vectors of the chunk, keeps them in
// registers and writes all of the group's rows (~ the scale factor of them) as
// fmaf(lh1, t1, lh0 * t0) -- bil_mix bit for bit, at 2 VALU ops per element instead of ~12 and
// 4 LDS reads per element per group instead of per row.
template <typename T, int J>
__global__ void __launch_bounds__(256) bilinear_fwd_rowgroup_kernel(const T* __restrict__ x, T* __restrict__ y, int hi, int wi, int c,
                                                                     int ho, int wo, float sh, float sw, int nchunk, FastDiv f_c) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  extern __shared__ float rows[];  // [2][wi * c]
  const int grp = blockIdx.x / nchunk, chunk = blockIdx.x - grp * nchunk;
  const int img = grp / hi, h0 = grp - img * hi;
  const int oa = bil_first_ge(h0, sh, hi, ho), ob = bil_first_ge(h0 + 1, sh, hi, ho);
  if (oa >= ob) return;  // no output row starts at h0 (downsampling): whole workgroup
  const int h1 = h0 + (h0 < hi - 1 ? 1 : 0);
  const int rl = wi * c;
  const T* r0 = x + ((long)img * hi + h0) * rl;
  const T* r1 = x + ((long)img * hi + h1) * rl;
  for (int e = threadIdx.x; e < rl; e += 256) {
    rows[e] = to_f(r0[e]);
    rows[rl + e] = to_f(r1[e]);
  }
  __syncthreads();
  const int nv = wo * c / V;  // (wo * c) % V == 0 (host)
  const int v0 = (int)((long)nv * chunk / nchunk), v1 = (int)((long)nv * (chunk + 1) / nchunk);
  float t0[J][V], t1[J][V];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int v = v0 + threadIdx.x + 256 * j;
    if (v >= v1) break;
    const int e = v * V;
    int ow = (int)fdiv((uint32_t)e, f_c), ch = e - ow * c;
    int w0, w1;
    float lw0, lw1;
    bil_src(ow, sw, wi, w0, w1, lw0, lw1);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (ch == c) {
        ch = 0;
        ++ow;
        bil_src(ow, sw, wi, w0, w1, lw0, lw1);
      }
      const float* a = rows + w0 * c + ch;
      const float* b = rows + w1 * c + ch;
      t0[j][k] = fmaf(lw1, b[0], lw0 * a[0]);
      t1[j][k] = fmaf(lw1, b[rl], lw0 * a[rl]);
      ++ch;
    }
  }
  for (int oh = oa; oh < ob; ++oh) {
    int i0, i1;
    float lh0, lh1;
    bil_src(oh, sh, hi, i0, i1, lh0, lh1);
    T* yo = y + ((long)img * ho + oh) * wo * c;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int v = v0 + threadIdx.x + 256 * j;
      if (v >= v1) break;
      V16 r;
#pragma unroll
      for (int k = 0; k < V; ++k) r[k] = from_f<T>(fmaf(lh1, t1[j][k], lh0 * t0[j][k]));
      *(V16*)(yo + (long)v * V) = r;
    }
  }
}

static const bool kBilRowGroup = true;
static constexpr auto kBilGroupU = 4;  // column vectors per thread of bilinear_fwd_group_vec_kernel (1 / 2 / 4: 48 / 43 / 41 us, profiles/r6f)
static constexpr auto kBilJ = 2;  // output vectors per thread and column chunk (2, 3, 4, 6 measured: 2 best)

// Backward, separable gather (deterministic, no atomics): input index i along one axis
// receives from outputs o with i0(o) == i (weight l0) or i1(o) == i (weight l1); those o lie
// in [(i-0.5)/s - 0.5, (i+1.5)/s - 0.5], widened by one and tested exactly with bil_src.
RT_DEV float bil_wsum_range(int i, float s, int in, int out, int& lo, int& hi) {
  lo = max(0, (int)floorf(((float)i - 0.5f) / s - 0.5f) - 1);
  hi = min(out - 1, (int)ceilf(((float)i + 1.5f) / s - 0.5f) + 1);
  return 0.f;
}
RT_DEV float bil_weight(int o, int i, float s, int in) {
  int a0, a1;
  float l0, l1;
  bil_src(o, s, in, a0, a1, l0, l1);
  return (a0 == i ? l0 : 0.f) + (a1 == i ? l1 : 0.f);
}
// pass 1 (W): tmp[img][oh][iw][c] = sum_ow w(ow->iw) dy[img][oh][ow][c]   (fp32)
template <typename T>
__global__ void bilinear_bwd_w_kernel(const T* __restrict__ dy, float* __restrict__ tmp, int n, int wi, int c, int ho, int wo, float sw,
                                      int dyld, int dyoff) {
  const long total = (long)n * ho * wi * c;
  GRID_STRIDE(i, total) {
    const int ch = (int)(i % c);
    long q = i / c;
    const int iw = (int)(q % wi);
    const long row = q / wi;  // img * ho + oh
    int lo, hi;
    bil_wsum_range(iw, sw, wi, wo, lo, hi);
    const T* src = dy + row * wo * dyld + dyoff + ch;
    float acc = 0.f;
    for (int ow = lo; ow <= hi; ++ow) {
      const float wt = bil_weight(ow, iw, sw, wi);
      if (wt != 0.f) acc = fmaf(wt, to_f(src[(long)ow * dyld]), acc);
    }
    tmp[i] = acc;
  }
}
// pass 2 (H): dx[img][ih][iw][c] = sum_oh w(oh->ih) tmp[img][oh][iw][c]
template <typename T>
__global__ void bilinear_bwd_h_kernel(const float* __restrict__ tmp, T* __restrict__ dx, int n, int hi, int wi, int c, int ho, float sh) {
  const long total = (long)n * hi * wi * c;
  const long plane = (long)wi * c;
  GRID_STRIDE(i, total) {
    const long inner = i % plane;  // iw * c + ch
    long q = i / plane;
    const int ih = (int)(q % hi);
    const int img = (int)(q / hi);
    int lo, hh;
    bil_wsum_range(ih, sh, hi, ho, lo, hh);
    const float* src = tmp + (long)img * ho * plane + inner;
    float acc = 0.f;
    for (int oh = lo; oh <= hh; ++oh) {
      const float wt = bil_weight(oh, ih, sh, hi);
      if (wt != 0.f) acc = fmaf(wt, src[(long)oh * plane], acc);
    }
    dx[i] = from_f<T>(acc);
  }
}
// Table-driven variants of the two passes: the weights of one axis (per input index i: lo(i)
// and w(lo + j -> i), zero past hi(i)) are tabulated once per block in LDS instead of being
// re-derived (two bil_src evaluations) for every element and tap; same taps, same order, same
// zero skipping, so the sums are bit-identical to the kernels above.
static const int kBilTabLds = 48 * 1024;
RT_DEV void bil_table_build(float* tab, int* tlo, int in, int out, float s, int maxw) {
  for (int e = threadIdx.x; e < in * maxw; e += blockDim.x) {
    const int i = e / maxw, j = e - i * maxw;
    int lo, hi;
    bil_wsum_range(i, s, in, out, lo, hi);
    tab[e] = lo + j <= hi ? bil_weight(lo + j, i, s, in) : 0.f;
    if (j == 0) tlo[i] = lo;
  }
  __syncthreads();
}
template <typename T>
__global__ void bilinear_bwd_w_tab_kernel(const T* __restrict__ dy, float* __restrict__ tmp, int n, int wi, int c, int ho, int wo,
                                          float sw, int dyld, int dyoff, int maxw, FastDiv f_c, FastDiv f_wi) {
  extern __shared__ float tab[];
  int* tlo = (int*)(tab + wi * maxw);
  bil_table_build(tab, tlo, wi, wo, sw, maxw);
  const long total = (long)n * ho * wi * c;  // < 2^31 (host)
  GRID_STRIDE(i, total) {
    const uint32_t q = fdiv((uint32_t)i, f_c), row = fdiv(q, f_wi);
    const int ch = (int)((uint32_t)i - q * c), iw = (int)(q - row * wi);
    const float* w = tab + iw * maxw;
    const T* src = dy + ((long)row * wo + tlo[iw]) * dyld + dyoff + ch;
    float acc = 0.f;
    for (int j = 0; j < maxw; ++j) {
      const float wt = w[j];
      if (wt != 0.f) acc = fmaf(wt, to_f(src[(long)j * dyld]), acc);
    }
    tmp[i] = acc;
  }
}
template <typename T>
__global__ void bilinear_bwd_h_tab_kernel(const float* __restrict__ tmp, T* __restrict__ dx, int n, int hi, int wi, int c, int ho,
                                          float sh, int maxh, FastDiv f_plane, FastDiv f_hi) {
  extern __shared__ float tab[];
  int* tlo = (int*)(tab + hi * maxh);
  bil_table_build(tab, tlo, hi, ho, sh, maxh);
  const uint32_t plane = (uint32_t)wi * c;
  const long total = (long)n * hi * plane;  // < 2^31 (host)
  GRID_STRIDE(i, total) {
    const uint32_t q = fdiv((uint32_t)i, f_plane), img = fdiv(q, f_hi);
    const uint32_t inner = (uint32_t)i - q * plane;
    const int ih = (int)(q - img * hi);
    const float* w = tab + ih * maxh;
    const float* src = tmp + ((long)img * ho + tlo[ih]) * plane + inner;
    float acc = 0.f;
    for (int j = 0; j < maxh; ++j) {
      const float wt = w[j];
      if (wt != 0.f) acc = fmaf(wt, src[(long)j * plane], acc);
    }
    dx[i] = from_f<T>(acc);
  }
}
// [first, last] nonzero entry of each table row, packed first | (last + 1) << 16 (the tables
// carry a one-entry margin either side, so a plain loop over maxw wastes taps)
RT_DEV void bil_table_span(const float* tab, int* span, int in, int maxw) {
  for (int i = threadIdx.x; i < in; i += blockDim.x) {
    int f = maxw, l = -1;
    for (int j = 0; j < maxw; ++j)
      if (tab[i * maxw + j] != 0.f) {
        f = min(f, j);
        l = j;
      }
    span[i] = f | (l + 1) << 16;
  }
  __syncthreads();
}
// Both passes in one kernel for 16-B channel vectors: a thread owns V channels of one input
// pixel and forms each output row's W-pass sum t (the W kernel's taps, order and zero skipping,
// fp32) right before the H-pass FMA that consumes it -- the same two fp32 FMA chains, so dx is
// bit-identical to the two-pass kernels, without the fp32 [ho][wi] intermediate's write and
// re-read.  Neighbouring input pixels re-read dY rows through L2 (XCD-aware block order).
// Only each row's nonzero span is visited, and its column taps go four at a time: the four
// loads issued (clamped into the span) before their FMAs, a zero weight leaving t unchanged
// exactly as the skipped tap of the two-pass kernel.
template <typename T, int G>
__global__ void __launch_bounds__(256) bilinear_bwd_fused_vec_kernel(const T* __restrict__ dy, T* __restrict__ dx, int hi, int wi,
                                                                     int c, int ho, int wo, float sh, float sw, int dyld, int dyoff,
                                                                     int maxh, int maxw, long total, FastDiv f_cv, FastDiv f_wi,
                                                                     FastDiv f_hi) {
  extern __shared__ float tab[];
  float* wtab = tab;
  int* wlo = (int*)(wtab + wi * maxw);
  float* htab = (float*)(wlo + wi);
  int* hlo = (int*)(htab + hi * maxh);
  int* wspan = hlo + hi;
  int* hspan = wspan + wi;
  bil_table_build(wtab, wlo, wi, wo, sw, maxw);
  bil_table_build(htab, hlo, hi, ho, sh, maxh);
  bil_table_span(wtab, wspan, wi, maxw);
  bil_table_span(htab, hspan, hi, maxh);
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  const int cv = c / V;
  GRID_STRIDE_XCD(i, total) {  // total < 2^31 (host)
    const uint32_t q = fdiv((uint32_t)i, f_cv), r = fdiv(q, f_wi);
    const int ch = ((int)((uint32_t)i - q * cv)) * V, iw = (int)(q - r * wi);
    const uint32_t img = fdiv(r, f_hi);
    const int ih = (int)(r - img * hi);
    const float* wx = wtab + iw * maxw;
    const float* wy = htab + ih * maxh;
    const T* base = dy + ((long)img * ho + hlo[ih]) * wo * dyld + (long)wlo[iw] * dyld + dyoff + ch;
    const int jx0 = wspan[iw] & 0xffff, jx1 = wspan[iw] >> 16;
    const int ky0 = hspan[ih] & 0xffff, ky1 = hspan[ih] >> 16;
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    for (int k = ky0; k < ky1; ++k) {
      const float yk = wy[k];
      if (yk == 0.f) continue;
      const T* row = base + (long)k * wo * dyld;
      float t[V];
#pragma unroll
      for (int e = 0; e < V; ++e) t[e] = 0.f;
      for (int j0 = jx0; j0 < jx1; j0 += G) {
        V16 v[G];
        float xw[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          const int j = j0 + u;
          xw[u] = j < jx1 ? wx[j] : 0.f;
          v[u] = *(const V16*)(row + (long)min(j, jx1 - 1) * dyld);
        }
#pragma unroll
        for (int u = 0; u < G; ++u)
#pragma unroll
          for (int e = 0; e < V; ++e) t[e] = xw[u] != 0.f ? fmaf(xw[u], to_f(v[u][e]), t[e]) : t[e];
      }
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = fmaf(yk, t[e], acc[e]);
    }
    V16 o;
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = from_f<T>(acc[e]);
    *(V16*)(dx + (((long)img * hi + ih) * wi + iw) * c + ch) = o;
  }
}
// The same one-pass form for channel counts off the vector width (the supervision heads'
// 19-class logits): a thread per (input pixel, channel), dY dense (pitch c).  Adjacent lanes
// read adjacent channels, so each tap's loads stay contiguous across the wave.
template <typename T, int G>
__global__ void __launch_bounds__(256) bilinear_bwd_fused_kernel(const T* __restrict__ dy, T* __restrict__ dx, int hi, int wi, int c,
                                                                 int ho, int wo, float sh, float sw, int maxh, int maxw, long total,
                                                                 FastDiv f_c, FastDiv f_wi, FastDiv f_hi) {
  extern __shared__ float tab[];
  float* wtab = tab;
  int* wlo = (int*)(wtab + wi * maxw);
  float* htab = (float*)(wlo + wi);
  int* hlo = (int*)(htab + hi * maxh);
  int* wspan = hlo + hi;
  int* hspan = wspan + wi;
  bil_table_build(wtab, wlo, wi, wo, sw, maxw);
  bil_table_build(htab, hlo, hi, ho, sh, maxh);
  bil_table_span(wtab, wspan, wi, maxw);
  bil_table_span(htab, hspan, hi, maxh);
  GRID_STRIDE_XCD(i, total) {  // total < 2^31 (host)
    const uint32_t q = fdiv((uint32_t)i, f_c), r = fdiv(q, f_wi);
    const int ch = (int)((uint32_t)i - q * c), iw = (int)(q - r * wi);
    const uint32_t img = fdiv(r, f_hi);
    const int ih = (int)(r - img * hi);
    const float* wx = wtab + iw * maxw;
    const float* wy = htab + ih * maxh;
    const T* base = dy + (((long)img * ho + hlo[ih]) * wo + wlo[iw]) * c + ch;
    const int jx0 = wspan[iw] & 0xffff, jx1 = wspan[iw] >> 16;
    const int ky0 = hspan[ih] & 0xffff, ky1 = hspan[ih] >> 16;
    float acc = 0.f;
    for (int k = ky0; k < ky1; ++k) {
      const float yk = wy[k];
      if (yk == 0.f) continue;
      const T* row = base + (long)k * wo * c;
      float t = 0.f;
      for (int j0 = jx0; j0 < jx1; j0 += G) {
        T v[G];
        float xw[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          const int j = j0 + u;
          xw[u] = j < jx1 ? wx[j] : 0.f;
          v[u] = row[(long)min(j, jx1 - 1) * c];
        }
#pragma unroll
        for (int u = 0; u < G; ++u) t = xw[u] != 0.f ? fmaf(xw[u], to_f(v[u]), t) : t;
      }
      acc = fmaf(yk, t, acc);
    }
    dx[i] = from_f<T>(acc);
  }
}
// most outputs any input index of an axis receives from (bil_wsum_range, host float math)
static int bil_maxw(int in, int out, float s) {
  int m = 0;
  for (int i = 0; i < in; ++i) {
    int lo = (int)std::floor(((float)i - 0.5f) / s - 0.5f) - 1;
    int hi = (int)std::ceil(((float)i + 1.5f) / s - 0.5f) + 1;
    lo = std::max(lo, 0);
    hi = std::min(hi, out - 1);
    m = std::max(m, hi - lo + 1);
  }
  return m + 1;  // margin for the device's own rounding of the same range (zero entries)
}
static size_t bil_tab_bytes(int in, int maxw) { return ((size_t)in * maxw + in) * 4; }
// launch both passes table-driven when the tables fit and the index math fits 32 bits, else the
// per-element kernels; w pass reads dy with row pitch dyld at channel offset dyoff
template <typename T>
static void bilinear_bwd_launch(const T* dy, float* tmp, T* dx, int n, int hi, int wi, int c, int ho, int wo, float sh, float sw,
                                int dyld, int dyoff, hipStream_t st) {
  const long tw = (long)n * ho * wi * c, th = (long)n * hi * wi * c;
  const int mw = bil_maxw(wi, wo, sw), mh = bil_maxw(hi, ho, sh);
  const size_t bw = bil_tab_bytes(wi, mw), bh = bil_tab_bytes(hi, mh);
  constexpr int V = VecT<T>::N;
  if (c % V == 0 && dyld % V == 0 && dyoff % V == 0 && th < (1L << 31) && bw + bh + (wi + hi) * 4 <= (size_t)kBilTabLds &&
      (long)n * ho * wo * dyld < (1L << 40)) {
    const long tv = th / V;
    // taps per load batch: 8 when an input column reaches ~8 output columns (x4), else 4 (x2)
    auto kern = mw >= 10 ? bilinear_bwd_fused_vec_kernel<T, 8> : bilinear_bwd_fused_vec_kernel<T, 4>;
    hipLaunchKernelGGL(kern, dim3(ew_blocks(tv)), dim3(256), bw + bh + (wi + hi) * 4, st, dy, dx, hi, wi, c, ho, wo, sh, sw, dyld,
                       dyoff, mh, mw, tv, fastdiv_make(c / V), fastdiv_make(wi), fastdiv_make(hi));
    return;
  }
  if (c % V != 0 && dyld == c && dyoff == 0 && th < (1L << 31) && bw + bh + (wi + hi) * 4 <= (size_t)kBilTabLds &&
      (long)n * ho * wo * c < (1L << 40)) {
    auto kern = mw >= 10 ? bilinear_bwd_fused_kernel<T, 8> : bilinear_bwd_fused_kernel<T, 4>;
    hipLaunchKernelGGL(kern, dim3(ew_blocks(th)), dim3(256), bw + bh + (wi + hi) * 4, st, dy, dx, hi, wi, c, ho, wo, sh, sw, mh, mw,
                       th, fastdiv_make(c), fastdiv_make(wi), fastdiv_make(hi));
    return;
  }
  if (tw < (1L << 31) && bw <= (size_t)kBilTabLds)
    hipLaunchKernelGGL(bilinear_bwd_w_tab_kernel<T>, dim3(ew_blocks(tw)), dim3(256), bw, st, dy, tmp, n, wi, c, ho, wo, sw, dyld,
                       dyoff, mw, fastdiv_make(c), fastdiv_make(wi));
  else
    hipLaunchKernelGGL(bilinear_bwd_w_kernel<T>, dim3(ew_blocks(tw)), dim3(256), 0, st, dy, tmp, n, wi, c, ho, wo, sw, dyld, dyoff);
  if (th < (1L << 31) && bh <= (size_t)kBilTabLds)
    hipLaunchKernelGGL(bilinear_bwd_h_tab_kernel<T>, dim3(ew_blocks(th)), dim3(256), bh, st, (const float*)tmp, dx, n, hi, wi, c, ho,
                       sh, mh, fastdiv_make((uint32_t)wi * c), fastdiv_make(hi));
  else
    hipLaunchKernelGGL(bilinear_bwd_h_kernel<T>, dim3(ew_blocks(th)), dim3(256), 0, st, (const float*)tmp, dx, n, hi, wi, c, ho, sh);
}
extern "C" int rtsds_bilinear_fwd(const void* x, void* y, int n, int hi, int wi, int c, int ho, int wo, float scale_h, float scale_w,
                                  int y_ld, int y_off, int dtype, void* stream) {
  const long total = (long)n * ho * wo * c;
  if (total <= 0 || hi <= 0 || wi <= 0) return RTSDS_ERR_SHAPE;
  if (y_ld <= 0) y_ld = c;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    constexpr int V = VecT<T>::N;
    const long pix = (long)n * ho * wo;
    // grouped taps pay off from ~3 output rows per source row (x2: 24 vs 17 us at 256 ch, x4:
    // 26 vs 28 us, tools/ab_bilinear.sh)
    if (c % V == 0 && y_ld % V == 0 && y_off % V == 0 && ho >= 3 * hi && kBilRowGroup)
      hipLaunchKernelGGL((bilinear_fwd_group_vec_kernel<T, kBilGroupU>), dim3(rt_cdiv(wo * (c / V), 256 * kBilGroupU), n * hi),
                         dim3(256), 0, st, (const T*)x, (T*)y, n, hi, wi, c, ho, wo, scale_h, scale_w, y_ld, y_off, nullptr, nullptr);
    else if (c % V == 0 && y_ld % V == 0 && y_off % V == 0)
      hipLaunchKernelGGL((bilinear_fwd_kernel<T, 0>), dim3(ew_blocks(pix * (c / V))), dim3(256), 0, st, (const T*)x, (T*)y, n, hi, wi, c, ho, wo, scale_h, scale_w, y_ld, y_off);
    else if (c >= V && y_ld == c && y_off == 0 && (wo * c) % V == 0 && 2L * wi * c * 4 <= 64 * 1024 && ho >= hi && kBilRowGroup) {
      // column chunks: <= 256 * kJ vectors each, and enough workgroups to fill the chip
      constexpr int kJ = kBilJ;
      const int nv = wo * c / V;
      int nchunk = std::max((nv + 256 * kJ - 1) / (256 * kJ), (1024 + n * hi - 1) / (n * hi));
      nchunk = std::min(nchunk, std::max(1, nv / 64));
      nchunk = std::max(nchunk, (nv + 256 * kJ - 1) / (256 * kJ));
      hipLaunchKernelGGL((bilinear_fwd_rowgroup_kernel<T, kJ>), dim3(n * hi * nchunk), dim3(256), 2 * wi * c * 4, st, (const T*)x,
                         (T*)y, hi, wi, c, ho, wo, scale_h, scale_w, nchunk, fastdiv_make(c));
    } else if (c >= V && y_ld == c && y_off == 0 && (wo * c) % V == 0 && 2L * wi * c * 4 <= 64 * 1024)
      hipLaunchKernelGGL((bilinear_fwd_rows_kernel<T>), dim3(n * ho), dim3(256), 2 * wi * c * 4, st, (const T*)x, (T*)y, hi, wi, c, ho,
                         wo, scale_h, scale_w, fastdiv_make(c));
    else if (c <= 64)
      hipLaunchKernelGGL((bilinear_fwd_kernel<T, 1>), dim3(ew_blocks(pix)), dim3(256), 0, st, (const T*)x, (T*)y, n, hi, wi, c, ho, wo, scale_h, scale_w, y_ld, y_off);
    else
      hipLaunchKernelGGL((bilinear_fwd_kernel<T, 2>), dim3(ew_blocks(pix * c)), dim3(256), 0, st, (const T*)x, (T*)y, n, hi, wi, c, ho, wo, scale_h, scale_w, y_ld, y_off);
  });
  RET_LAUNCH();
}
extern "C" int rtsds_bilinear_fwd_scaled(const void* x, const void* s1, const void* s2, void* y, int n, int hi, int wi, int c, int ho,
                                         int wo, float scale_h, float scale_w, int y_ld, int y_off, int dtype, void* stream) {
  const long total = (long)n * ho * wo * c;
  if (total <= 0 || hi <= 0 || wi <= 0) return RTSDS_ERR_SHAPE;
  if (y_ld <= 0) y_ld = c;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    constexpr int V = VecT<T>::N;
    if (!(c % V == 0 && y_ld % V == 0 && y_off % V == 0 && ho >= hi)) return RTSDS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((bilinear_fwd_group_vec_kernel<T, kBilGroupU>), dim3(rt_cdiv(wo * (c / V), 256 * kBilGroupU), n * hi),
                       dim3(256), 0, st, (const T*)x, (T*)y, n, hi, wi, c, ho, wo, scale_h, scale_w, y_ld, y_off, (const T*)s1,
                       (const T*)s2);
  });
  RET_LAUNCH();
}
extern "C" size_t rtsds_bilinear_bwd_workspace(int n, int hi, int wi, int c, int ho, int wo) {
  (void)hi; (void)wo;
  return (size_t)n * ho * wi * c * sizeof(float) + 256;
}
extern "C" int rtsds_bilinear_bwd(const void* dy, void* dx, int n, int hi, int wi, int c, int ho, int wo, float scale_h, float scale_w,
                                  int dy_ld, int dy_off, int dtype, void* ws, size_t ws_bytes, void* stream) {
  const long total = (long)n * hi * wi * c;
  if (total <= 0 || ho <= 0 || wo <= 0) return RTSDS_ERR_SHAPE;
  if (ws_bytes < rtsds_bilinear_bwd_workspace(n, hi, wi, c, ho, wo)) return RTSDS_ERR_WORKSPACE;
  if (dy_ld <= 0) dy_ld = c;
  hipStream_t st = (hipStream_t)stream;
  float* tmp = (float*)ws;
  DISPATCH_T(dtype, bilinear_bwd_launch<T>((const T*)dy, tmp, (T*)dx, n, hi, wi, c, ho, wo, scale_h, scale_w, dy_ld, dy_off, st));
  RET_LAUNCH();
}

// ------------------------------------------------------------------ fused resize + softmax
// The discriminator input of the DA iteration (train.py:225,245,256): softmax over classes of
// the bilinearly resized head, zero-padded to y_ld channels so the discriminator's first conv
// reads it without a separate pad pass.  The logits are the bilinear_fwd values rounded to T
// and the softmax is softmax_fwd_staged's arithmetic (two expf passes, sequential sum), so the
// probabilities are bit-identical to the unfused resize -> softmax -> pad chain; the resized
// logits and the unpadded probabilities never exist in memory.
//   forward:  one block per 256 output pixels of a row.  The two low-res source rows the tile
//             reads (a few dozen pixels for x8) are staged once in LDS as fp32 (coalesced), each
//             thread blends its pixel's 4 taps from LDS, and the tile's padded rows leave through
//             LDS as lane-consecutive 16-B chunks (HBM-bound on the padded output).
//   backward: one block per (row, tile of up to 64 input columns): the dy segment the tile's
//             width adjoint reads is staged in LDS (coalesced), then thread per output pixel
//             forms the softmax backward T(p_k (dp_k - sum_j p_j dp_j)) in place (its p row by
//             16-B loads); the tile's bilinear
//             weights are tabulated once in LDS; thread per (input column, class) accumulates
//             the width adjoint in bilinear_bwd_w_kernel's order (ascending output column,
//             zero weights skipped).  The vertical pass is bilinear_bwd_h_kernel.
static const int kUpsmMaxC = 32;
static const int kUpsmPix = 256;
static const int kUpsmLds = 48 * 1024;
// one tile of the fused resize + softmax kernels (blockIdx.x = row * tiles + tile): up to 256
// output pixels [ow0, ow0 + np) of output row `row`, the two source rows r0 / r1 with their
// weights and, STAGED, their columns [wlo, wlo + n1 / c) copied to src as fp32 [2][n1] (the
// caller places the barrier)
template <typename T>
struct UpsmTile {
  long row;  // img * ho + oh
  int ow0, np, wlo, n1;
  float lh0, lh1;
  const T *r0, *r1;
};
template <typename T, bool STAGED>
RT_DEV UpsmTile<T> upsm_tile(const T* __restrict__ x, float* src, int hi, int wi, int c, int ho, int wo, float sh, float sw,
                             int tiles) {
  UpsmTile<T> t;
  const int tile = blockIdx.x % tiles;
  t.row = blockIdx.x / tiles;
  const int oh = (int)(t.row % ho), img = (int)(t.row / ho);
  t.ow0 = tile * kUpsmPix;
  t.np = min(kUpsmPix, wo - t.ow0);
  int h0, h1;
  bil_src(oh, sh, hi, h0, h1, t.lh0, t.lh1);
  t.r0 = x + ((long)img * hi + h0) * wi * c;
  t.r1 = x + ((long)img * hi + h1) * wi * c;
  t.wlo = 0;
  t.n1 = 0;
  if (STAGED) {  // taps are monotone in ow: columns [w0(ow0), w1(last)] cover the tile
    int a0, a1, b0, b1;
    float t0, t1;
    bil_src(t.ow0, sw, wi, a0, a1, t0, t1);
    bil_src(t.ow0 + t.np - 1, sw, wi, b0, b1, t0, t1);
    t.wlo = a0;
    t.n1 = (b1 - a0 + 1) * c;
    for (int e = threadIdx.x; e < t.n1; e += 256) {
      src[e] = to_f(t.r0[(long)t.wlo * c + e]);
      src[t.n1 + e] = to_f(t.r1[(long)t.wlo * c + e]);
    }
  }
  return t;
}
// one output pixel's blend + softmax, shared by upsoftmax_fwd_kernel and upsoftmax_acc_kernel:
// on return the probability of class k is the fp32 product z[k] * iz
template <typename T, bool STAGED, int CC>
RT_DEV void upsm_probs(const T* __restrict__ r0, const T* __restrict__ r1, const float* src, int wlo, int n1, int c_, int ow,
                       float sw, int wi, float lh0, float lh1, float (&z)[kUpsmMaxC], float& iz) {
  const int c = CC > 0 ? CC : c_;
  int w0, w1;
  float lw0, lw1;
  bil_src(ow, sw, wi, w0, w1, lw0, lw1);
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < kUpsmMaxC; ++k) {
    if (k < c) {
      float p00, p01, p10, p11;
      if (STAGED) {
        p00 = src[(w0 - wlo) * c + k];
        p01 = src[(w1 - wlo) * c + k];
        p10 = src[n1 + (w0 - wlo) * c + k];
        p11 = src[n1 + (w1 - wlo) * c + k];
      } else {
        p00 = to_f(r0[(long)w0 * c + k]);
        p01 = to_f(r0[(long)w1 * c + k]);
        p10 = to_f(r1[(long)w0 * c + k]);
        p11 = to_f(r1[(long)w1 * c + k]);
      }
      z[k] = to_f(from_f<T>(bil_mix(p00, p01, p10, p11, lh0, lh1, lw0, lw1)));
      m = fmaxf(m, z[k]);
    }
  }
  float sum = 0.f;  // exp(z - m) evaluated once per class (softmax_fwd_staged evaluates the same
                    // expf twice: identical values)
#pragma unroll
  for (int k = 0; k < kUpsmMaxC; ++k)
    if (k < c) {
      z[k] = expf(z[k] - m);
      sum += z[k];
    }
  iz = 1.f / sum;
}
// one output pixel of upsoftmax_fwd_kernel: blend, softmax, padded row into the LDS tile
template <typename T, bool STAGED, int CC>
RT_DEV void upsm_pixel(const T* __restrict__ r0, const T* __restrict__ r1, const float* src, T* o, int wlo, int n1, int c_, int ow,
                       float sw, int wi, float lh0, float lh1, int yld) {
  const int c = CC > 0 ? CC : c_;
  float z[kUpsmMaxC];
  float iz;
  upsm_probs<T, STAGED, CC>(r0, r1, src, wlo, n1, c_, ow, sw, wi, lh0, lh1, z, iz);
  // the padded row goes through LDS so the tile leaves as lane-consecutive 16-B chunks (the
  // tile's rows are contiguous in y): full-line writes instead of 64-B-strided partial ones
  if (sizeof(T) == 2 && yld == 32) {  // 4 x 16-B LDS writes, chunk q at slot q ^ (pixel & 3)
    typedef typename VecT<T>::v16 V16;
    const int sw4 = ow & 3;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      V16 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = from_f<T>(q * 8 + j < c ? z[q * 8 + j] * iz : 0.f);
      *(V16*)(o + (q ^ sw4) * 8) = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kUpsmMaxC; ++k)
      if (k < yld) o[k] = from_f<T>(k < c ? z[k] * iz : 0.f);
  }
}
template <typename T, bool STAGED, int CC>  // CC > 0: compile-time class count (19), 0: runtime c
__global__ void __launch_bounds__(256) upsoftmax_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int hi, int wi, int c_,
                                                            int ho, int wo, float sh, float sw, int yld, int tiles) {
  const int c = CC > 0 ? CC : c_;
  extern __shared__ __attribute__((aligned(16))) float src[];  // STAGED: [2][ncols][c]
  const int tid = threadIdx.x;
  const UpsmTile<T> tl = upsm_tile<T, STAGED>(x, src, hi, wi, c, ho, wo, sh, sw, tiles);
  const int ow0 = tl.ow0, np = tl.np;
  if (STAGED) __syncthreads();
  T* outbuf = (T*)(src + ((2 * tl.n1 + 3) & ~3));  // [256][yld], 16-B aligned
  if (tid < np)
    upsm_pixel<T, STAGED, CC>(tl.r0, tl.r1, src, outbuf + tid * yld, tl.wlo, tl.n1, c, ow0 + tid, sw, wi, tl.lh0, tl.lh1, yld);
  __syncthreads();  // every lane reaches the same barrier (no early exit)
  T* dst = y + (tl.row * wo + ow0) * yld;
  if (sizeof(T) == 2 && yld == 32) {  // un-swizzle: LDS read linear, global chunk q = slot ^ (pixel & 3)
    typedef typename VecT<T>::v16 V16;
    for (int i = tid; i < np * 4; i += 256) {
      const int t = i >> 2, q = (i & 3) ^ ((ow0 + t) & 3);
      *(V16*)(dst + t * 32 + q * 8) = *(const V16*)(outbuf + i * 8);
    }
  } else {
    stage_out(dst, outbuf, np * yld);
  }
}
// ------------------------------------------------------------------ multi-scale / flip evaluation
// One pass of the summed-probability protocol (validation.predict_multiscale): the
// upsoftmax_fwd_kernel tile (same staging, same upsm_probs arithmetic), but the probabilities stay
// fp32 and are stored into / added onto the fp32 sum acc [n][ho][wo][c]; with flip the tile lands
// on the mirrored column range, which is still contiguous, so the pixel order is reversed inside
// LDS and the tile leaves (and, when accumulating, the old sums arrive) as lane-consecutive 16-B
// chunks.  The LDS tile sits at the destination's offset inside its 16-B chunk (a 19-class row
// is 76 B, so tiles start at any 4-B phase): head / tail floats move singly, the rest as float4.
// The add is one fp32 add of the rounded product (never an FMA), so acc equals the unfused
// softmax -> flip -> add chain bit for bit.  pred = first-max argmax of the updated row.
template <bool IN>  // IN: global -> LDS, else LDS -> global; s and g share the phase `(4 - head) & 3`
RT_DEV void upsm_tile_copy(float* __restrict__ g, float* s, int nel, int head) {
  const int tid = threadIdx.x;
  const int nv = (nel - head) >> 2, rest = nel - head - (nv << 2);
  float4* gv = (float4*)(g + head);
  float4* sv = (float4*)(s + head);
  for (int i = tid; i < nv; i += 256) {
    if (IN) sv[i] = gv[i];
    else gv[i] = sv[i];
  }
  int e = -1;  // head (< 4 floats) on lanes 0.., tail (< 4 floats) on the second wave
  if (tid < head) e = tid;
  else if (tid >= 64 && tid - 64 < rest) e = head + (nv << 2) + tid - 64;
  if (e >= 0) {
    if (IN) s[e] = g[e];
    else g[e] = s[e];
  }
}
template <typename T, bool STAGED, int CC>  // CC > 0: compile-time class count (19), 0: runtime c
__global__ void __launch_bounds__(256) upsoftmax_acc_kernel(const T* __restrict__ x, float* __restrict__ acc,
                                                            int64_t* __restrict__ pred, int hi, int wi, int c_, int ho, int wo,
                                                            float sh, float sw, int flip, int accumulate, int tiles) {
  const int c = CC > 0 ? CC : c_;
  extern __shared__ __attribute__((aligned(16))) float src[];  // STAGED: [2][ncols][c]
  const int tid = threadIdx.x;
  const UpsmTile<T> tl = upsm_tile<T, STAGED>(x, src, hi, wi, c, ho, wo, sh, sw, tiles);
  const int ow0 = tl.ow0, np = tl.np;
  // destination: output columns [ow0, ow0 + np), mirrored to [wo - ow0 - np, wo - ow0) with flip
  const int d0 = flip ? wo - ow0 - np : ow0;
  float* dst = acc + (tl.row * wo + d0) * c;
  const int nel = np * c;
  const int mis = (int)(((uintptr_t)dst >> 2) & 3), head = min(nel, (4 - mis) & 3);
  float* tbuf = src + ((2 * tl.n1 + 3) & ~3) + mis;  // [np][c] at dst's phase inside a 16-B chunk
  if (accumulate) upsm_tile_copy<true>(dst, tbuf, nel, head);
  __syncthreads();
  if (tid < np) {
    float z[kUpsmMaxC];
    float iz;
    upsm_probs<T, STAGED, CC>(tl.r0, tl.r1, src, tl.wlo, tl.n1, c, ow0 + tid, sw, wi, tl.lh0, tl.lh1, z, iz);
    const int lp = flip ? np - 1 - tid : tid;
    float* o = tbuf + lp * c;
    float best = 0.f;
    int bi = 0;
#pragma unroll
    for (int k = 0; k < kUpsmMaxC; ++k)
      if (k < c) {
        float v = __fmul_rn(z[k], iz);
        if (accumulate) v = __fadd_rn(o[k], v);
        o[k] = v;
        if (k == 0 || v > best) {
          best = v;
          bi = k;
        }
      }
    if (pred != nullptr) pred[tl.row * wo + d0 + lp] = bi;
  }
  __syncthreads();  // every lane reaches the same barrier (no early exit)
  upsm_tile_copy<false>(dst, tbuf, nel, head);
}
// exact output-pixel span [lo, hi] read by input columns [iw0, iw1] (bil_wsum_range bounds)
__host__ __device__ inline void upsm_span(int iw0, int iw1, float sw, int wi, int wo, int& lo, int& hi) {
  lo = (int)floorf(((float)iw0 - 0.5f) / sw - 0.5f) - 1;
  hi = (int)ceilf(((float)iw1 + 1.5f) / sw - 0.5f) + 1;
  lo = lo < 0 ? 0 : lo;
  hi = hi > wo - 1 ? wo - 1 : hi;
}
template <typename T, int CC>  // CC > 0: compile-time class count (19), 0: runtime c
__global__ void __launch_bounds__(256) upsoftmax_bwd_w_kernel(const T* __restrict__ dy, int dyld, const T* __restrict__ y,
                                                              int yld, float* __restrict__ tmp, int wi, int c_, int wo, float sw,
                                                              int tw, int tiles, int cap, int maxw) {
  const int c = CC > 0 ? CC : c_;
  extern __shared__ __attribute__((aligned(16))) float smf[];
  float* wt = smf;                       // [tw][maxw]: weights of output columns lo(iw) + j
  int* wlo = (int*)(wt + tw * maxw);     // [tw]
  T* sgt = (T*)(wlo + tw);               // [cap][c]: dy, then the softmax backward in place
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % tiles;
  const long row = blockIdx.x / tiles;  // img * ho + oh
  const int iw0 = tile * tw, iw1 = min(wi, iw0 + tw) - 1, nw = iw1 - iw0 + 1;
  int olo, ohi;
  upsm_span(iw0, iw1, sw, wi, wo, olo, ohi);
  const int cnt = ohi - olo + 1;  // <= cap (host: exact maximum over the tiles)
  // dy segment -> LDS as T, coalesced (rows of pitch c; contiguous in memory when dyld == c)
  const T* gseg = dy + (row * wo + olo) * dyld;
  if (dyld == c) {
    for (int e = tid; e < cnt * c; e += 256) sgt[e] = gseg[e];
  } else {
    for (int e = tid; e < cnt * c; e += 256) {
      const int q = e / c;
      sgt[e] = gseg[(long)q * dyld + (e - q * c)];
    }
  }
  __syncthreads();
  // thread per output pixel: p row (16-B vectors when the pitch allows), softmax backward in place
  for (int q = tid; q < cnt; q += 256) {
    const T* pr = y + (row * wo + olo + q) * yld;
    float pv[kUpsmMaxC];
    if (sizeof(T) == 2 && (yld & 7) == 0) {
      typedef typename VecT<T>::v16 V16;
#pragma unroll
      for (int v = 0; v < kUpsmMaxC / 8; ++v)
        if (v * 8 < c) {
          const V16 t = *(const V16*)(pr + v * 8);
#pragma unroll
          for (int j = 0; j < 8; ++j) pv[v * 8 + j] = to_f(t[j]);
        }
    } else {
#pragma unroll
      for (int k = 0; k < kUpsmMaxC; ++k)
        if (k < c) pv[k] = to_f(pr[k]);
    }
    T* g = sgt + q * c;
    float gv[kUpsmMaxC];
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < kUpsmMaxC; ++k)
      if (k < c) {
        gv[k] = to_f(g[k]);
        dot = fmaf(gv[k], pv[k], dot);
      }
#pragma unroll
    for (int k = 0; k < kUpsmMaxC; ++k)
      if (k < c) g[k] = from_f<T>(pv[k] * (gv[k] - dot));
  }
  for (int e = tid; e < nw * maxw; e += 256) {
    const int il = e / maxw, j = e - il * maxw, iw = iw0 + il;
    int lo, hi;
    bil_wsum_range(iw, sw, wi, wo, lo, hi);
    wt[e] = lo + j <= hi ? bil_weight(lo + j, iw, sw, wi) : 0.f;
    if (j == 0) wlo[il] = lo - olo;
  }
  __syncthreads();
  for (int e = tid; e < nw * c; e += 256) {  // (input column, class) items, classes inner
    const int il = e / c, k = e - il * c;
    const float* w = wt + il * maxw;
    const T* s = sgt + wlo[il] * c + k;
    float acc = 0.f;
    for (int j = 0; j < maxw; ++j) {
      const float wv = w[j];
      if (wv != 0.f) acc = fmaf(wv, to_f(s[j * c]), acc);
    }
    tmp[(row * wi + iw0) * c + e] = acc;
  }
}
// columns of the low-res rows one forward tile stages (taps monotone in ow)
static int upsm_fwd_cols(int wi, int wo, float sw) {
  int cols = 0;
  for (int ow0 = 0; ow0 < wo; ow0 += kUpsmPix) {
    const int ow1 = std::min(wo, ow0 + kUpsmPix) - 1;
    float src0 = sw * ((float)ow0 + 0.5f) - 0.5f, src1 = sw * ((float)ow1 + 0.5f) - 0.5f;
    int a = src0 < 0.f ? 0 : (int)src0, b = src1 < 0.f ? 0 : (int)src1;
    a = std::min(a, wi - 1);
    b = std::min(b, wi - 1);
    b = b + (b < wi - 1 ? 1 : 0);
    cols = std::max(cols, b - a + 1);
  }
  return cols + 2;  // margin: the device computes the tap columns with its own float rounding
}
extern "C" int rtsds_upsoftmax_fwd(const void* x, void* y, int n, int hi, int wi, int c, int ho, int wo, float scale_h,
                                   float scale_w, int y_ld, int dtype, void* stream) {
  if (n <= 0 || ho <= 0 || wo <= 0 || hi <= 0 || wi <= 0 || c <= 0 || c > kUpsmMaxC || y_ld < c || y_ld > kUpsmMaxC)
    return RTSDS_ERR_SHAPE;
  const int tiles = rt_cdiv(wo, kUpsmPix);
  const long blocks = (long)n * ho * tiles;
  if (blocks > INT_MAX) return RTSDS_ERR_UNSUPPORTED;
  const size_t taps = (size_t)2 * upsm_fwd_cols(wi, wo, scale_w) * c * sizeof(float);
  const bool staged = taps <= (size_t)kUpsmLds;
  const size_t outb = (size_t)kUpsmPix * y_ld * (dtype == RTSDS_BF16 ? 2 : 4);
  const size_t lds = (staged ? taps + 16 : 0) + outb;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    if (staged && c == 19)
      hipLaunchKernelGGL((upsoftmax_fwd_kernel<T, true, 19>), dim3((unsigned)blocks), dim3(256), lds, st, (const T*)x, (T*)y, hi,
                         wi, c, ho, wo, scale_h, scale_w, y_ld, tiles);
    else if (staged)
      hipLaunchKernelGGL((upsoftmax_fwd_kernel<T, true, 0>), dim3((unsigned)blocks), dim3(256), lds, st, (const T*)x, (T*)y, hi,
                         wi, c, ho, wo, scale_h, scale_w, y_ld, tiles);
    else
      hipLaunchKernelGGL((upsoftmax_fwd_kernel<T, false, 0>), dim3((unsigned)blocks), dim3(256), lds, st, (const T*)x, (T*)y, hi,
                         wi, c, ho, wo, scale_h, scale_w, y_ld, tiles);
  });
  RET_LAUNCH();
}
extern "C" int rtsds_upsoftmax_acc(const void* x, float* acc, int64_t* pred, int n, int hi, int wi, int c, int ho, int wo,
                                   float scale_h, float scale_w, int flip, int accumulate, int dtype, void* stream) {
  if (n <= 0 || ho <= 0 || wo <= 0 || hi <= 0 || wi <= 0 || c <= 0 || c > kUpsmMaxC) return RTSDS_ERR_SHAPE;
  if (dtype != RTSDS_F32 && dtype != RTSDS_BF16) return RTSDS_ERR_UNSUPPORTED;
  if (x == nullptr || acc == nullptr || ((uintptr_t)acc & 3)) return RTSDS_ERR_UNSUPPORTED;
  const int tiles = rt_cdiv(wo, kUpsmPix);
  const long blocks = (long)n * ho * tiles;
  if (blocks > INT_MAX) return RTSDS_ERR_UNSUPPORTED;
  const size_t taps = (size_t)2 * upsm_fwd_cols(wi, wo, scale_w) * c * sizeof(float);
  // the fp32 tile + up to 3 floats of phase behind the (16-B rounded) staged rows
  const size_t tileb = 16 + (size_t)kUpsmPix * c * sizeof(float);
  const bool staged = taps + 16 + tileb <= (size_t)64 * 1024;
  const size_t lds = (staged ? taps + 16 : 0) + tileb;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    if (staged && c == 19)
      hipLaunchKernelGGL((upsoftmax_acc_kernel<T, true, 19>), dim3((unsigned)blocks), dim3(256), lds, st, (const T*)x, acc, pred,
                         hi, wi, c, ho, wo, scale_h, scale_w, flip, accumulate, tiles);
    else if (staged)
      hipLaunchKernelGGL((upsoftmax_acc_kernel<T, true, 0>), dim3((unsigned)blocks), dim3(256), lds, st, (const T*)x, acc, pred,
                         hi, wi, c, ho, wo, scale_h, scale_w, flip, accumulate, tiles);
    else
      hipLaunchKernelGGL((upsoftmax_acc_kernel<T, false, 0>), dim3((unsigned)blocks), dim3(256), lds, st, (const T*)x, acc, pred,
                         hi, wi, c, ho, wo, scale_h, scale_w, flip, accumulate, tiles);
  });
  RET_LAUNCH();
}
extern "C" size_t rtsds_upsoftmax_bwd_workspace(int n, int hi, int wi, int c, int ho, int wo) {
  return rtsds_bilinear_bwd_workspace(n, hi, wi, c, ho, wo);
}
// widest tile (<= 64 input columns) whose staged segment + weight table fit kUpsmLds; cap =
// its exact largest segment, maxw = the most output columns any input column reads
static bool upsm_tiling(int wi, int wo, int c, float sw, size_t esz, int& tw, int& cap, int& maxw) {
  maxw = 0;
  for (int iw = 0; iw < wi; ++iw) {
    int lo, hi;
    upsm_span(iw, iw, sw, wi, wo, lo, hi);
    maxw = std::max(maxw, hi - lo + 1);
  }
  for (tw = 64; tw >= 1; tw /= 2) {
    cap = 0;
    for (int iw0 = 0; iw0 < wi; iw0 += tw) {
      int lo, hi;
      upsm_span(iw0, std::min(wi, iw0 + tw) - 1, sw, wi, wo, lo, hi);
      cap = std::max(cap, hi - lo + 1);
    }
    if ((size_t)cap * c * esz + (size_t)tw * (maxw + 1) * 4 <= (size_t)kUpsmLds) return true;
  }
  return false;
}
extern "C" int rtsds_upsoftmax_bwd(const void* dy, int dy_ld, const void* y, int y_ld, void* dx, int n, int hi, int wi, int c,
                                   int ho, int wo, float scale_h, float scale_w, int dtype, void* ws, size_t ws_bytes,
                                   void* stream) {
  const long total = (long)n * hi * wi * c;
  if (total <= 0 || ho <= 0 || wo <= 0 || c > kUpsmMaxC || dy_ld < c || y_ld < c) return RTSDS_ERR_SHAPE;
  if (ws_bytes < rtsds_upsoftmax_bwd_workspace(n, hi, wi, c, ho, wo)) return RTSDS_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* tmp = (float*)ws;
  DISPATCH_T(dtype, {
    int tw, cap, maxw;
    if (!upsm_tiling(wi, wo, c, scale_w, sizeof(T), tw, cap, maxw)) return RTSDS_ERR_UNSUPPORTED;
    const int tiles = rt_cdiv(wi, tw);
    const long blocks = (long)n * ho * tiles;
    if (blocks > INT_MAX) return RTSDS_ERR_UNSUPPORTED;
    const size_t lds = (size_t)tw * (maxw + 1) * 4 + (size_t)cap * c * sizeof(T);
    if (c == 19)
      hipLaunchKernelGGL((upsoftmax_bwd_w_kernel<T, 19>), dim3((unsigned)blocks), dim3(256), lds, st, (const T*)dy, dy_ld,
                         (const T*)y, y_ld, tmp, wi, c, wo, scale_w, tw, tiles, cap, maxw);
    else
      hipLaunchKernelGGL((upsoftmax_bwd_w_kernel<T, 0>), dim3((unsigned)blocks), dim3(256), lds, st, (const T*)dy, dy_ld,
                         (const T*)y, y_ld, tmp, wi, c, wo, scale_w, tw, tiles, cap, maxw);
    const int mh = bil_maxw(hi, ho, scale_h);
    const size_t bh = bil_tab_bytes(hi, mh);
    if (total < (1L << 31) && bh <= (size_t)kBilTabLds)
      hipLaunchKernelGGL(bilinear_bwd_h_tab_kernel<T>, dim3(ew_blocks(total)), dim3(256), bh, st, (const float*)tmp, (T*)dx, n,
                         hi, wi, c, ho, scale_h, mh, fastdiv_make((uint32_t)wi * c), fastdiv_make(hi));
    else
      hipLaunchKernelGGL(bilinear_bwd_h_kernel<T>, dim3(ew_blocks(total)), dim3(256), 0, st, (const float*)tmp, (T*)dx, n, hi,
                         wi, c, ho, scale_h);
  });
  RET_LAUNCH();
}
