// Spatial pooling (gfx950): max pool, adaptive average pool.
#include "ew_common.h"

// ------------------------------------------------------------------ max pool
// torchvision / deeplab max pool (build_contextpath.py:21, deeplabv2.py:79): padded taps are
// skipped, first maximum wins (ATen CPU scan order), NaN propagates.  idx = tap index.
template <typename T>
__global__ void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ idx, int n, int h, int w,
                                   int c, int ho, int wo, int k, int s, int p) {
  const long total = (long)n * ho * wo * c;
  GRID_STRIDE(i, total) {
    const int ch = (int)(i % c);
    long q = i / c;
    const int ow = (int)(q % wo); q /= wo;
    const int oh = (int)(q % ho);
    const int img = (int)(q / ho);
    const int h0 = oh * s - p, w0 = ow * s - p;
    float best = -INFINITY;
    int bi = -1;
    for (int a = 0; a < k; ++a) {
      const int hh = h0 + a;
      if (hh < 0 || hh >= h) continue;
      for (int b = 0; b < k; ++b) {
        const int ww = w0 + b;
        if (ww < 0 || ww >= w) continue;
        const float v = to_f(x[(((long)img * h + hh) * w + ww) * c + ch]);
        if (bi < 0 || v > best || v != v) { best = v; bi = a * k + b; if (v != v) goto done; }
      }
    }
  done:
    y[i] = from_f<T>(best);
    idx[i] = (uint8_t)(bi < 0 ? 0 : bi);
  }
}
// Gather backward (deterministic): each input element sums the windows that chose it.
template <typename T>
__global__ void maxpool_bwd_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ idx, T* __restrict__ dx, int n, int h,
                                   int w, int c, int ho, int wo, int k, int s, int p) {
  const long total = (long)n * h * w * c;
  GRID_STRIDE(i, total) {
    const int ch = (int)(i % c);
    long q = i / c;
    const int iw = (int)(q % w); q /= w;
    const int ih = (int)(q % h);
    const int img = (int)(q / h);
    const int oh_lo = max(0, (ih + p - k + s) / s), oh_hi = min(ho - 1, (ih + p) / s);
    const int ow_lo = max(0, (iw + p - k + s) / s), ow_hi = min(wo - 1, (iw + p) / s);
    float acc = 0.f;
    for (int oh = oh_lo; oh <= oh_hi; ++oh) {
      const int a = ih - (oh * s - p);
      if (a < 0 || a >= k) continue;
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        const int b = iw - (ow * s - p);
        if (b < 0 || b >= k) continue;
        const long o = (((long)img * ho + oh) * wo + ow) * c + ch;
        if (idx[o] == a * k + b) acc += to_f(dy[o]);
      }
    }
    dx[i] = from_f<T>(acc);
  }
}

// Vector variants (c % V == 0): one thread per (pixel, 16-B channel vector).
template <typename T>
__global__ void maxpool_fwd_vec(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ idx, int n, int h, int w,
                                int c, int ho, int wo, int k, int s, int p) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  const int cv = c / V;
  const long total = (long)n * ho * wo * cv;
  GRID_STRIDE(i, total) {
    const int ch = (int)(i % cv) * V;
    long q = i / cv;
    const int ow = (int)(q % wo); q /= wo;
    const int oh = (int)(q % ho);
    const int img = (int)(q / ho);
    const int h0 = oh * s - p, w0 = ow * s - p;
    float best[V];
    int bi[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { best[j] = -INFINITY; bi[j] = -1; }
    for (int a = 0; a < k; ++a) {
      const int hh = h0 + a;
      if (hh < 0 || hh >= h) continue;
      for (int b = 0; b < k; ++b) {
        const int ww = w0 + b;
        if (ww < 0 || ww >= w) continue;
        const V16 v = *(const V16*)(x + (((long)img * h + hh) * w + ww) * c + ch);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float f = to_f(v[j]);
          if (bi[j] < 0 || f > best[j] || (f != f && best[j] == best[j])) { best[j] = f; bi[j] = a * k + b; }
        }
      }
    }
    V16 o;
    const long oi = (((long)img * ho + oh) * wo + ow) * c + ch;
#pragma unroll
    for (int j = 0; j < V; ++j) { o[j] = from_f<T>(best[j]); idx[oi + j] = (uint8_t)(bi[j] < 0 ? 0 : bi[j]); }
    *(V16*)(y + oi) = o;
  }
}
template <typename T>
__global__ void maxpool_bwd_vec(const T* __restrict__ dy, const uint8_t* __restrict__ idx, T* __restrict__ dx, int n, int h, int w,
                                int c, int ho, int wo, int k, int s, int p) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  const int cv = c / V;
  const long total = (long)n * h * w * cv;
  GRID_STRIDE(i, total) {
    const int ch = (int)(i % cv) * V;
    long q = i / cv;
    const int iw = (int)(q % w); q /= w;
    const int ih = (int)(q % h);
    const int img = (int)(q / h);
    const int oh_lo = max(0, (ih + p - k + s) / s), oh_hi = min(ho - 1, (ih + p) / s);
    const int ow_lo = max(0, (iw + p - k + s) / s), ow_hi = min(wo - 1, (iw + p) / s);
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    for (int oh = oh_lo; oh <= oh_hi; ++oh) {
      const int a = ih - (oh * s - p);
      if (a < 0 || a >= k) continue;
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        const int b = iw - (ow * s - p);
        if (b < 0 || b >= k) continue;
        const long o = (((long)img * ho + oh) * wo + ow) * c + ch;
        const V16 g = *(const V16*)(dy + o);
        const int want = a * k + b;
#pragma unroll
        for (int j = 0; j < V; ++j)
          if (idx[o + j] == want) acc[j] += to_f(g[j]);
      }
    }
    V16 r;
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = from_f<T>(acc[j]);
    *(V16*)(dx + (((long)img * h + ih) * w + iw) * c + ch) = r;
  }
}

// 3x3 windows (the ResNet stem pool, build_contextpath.py via torchvision resnet.py:
// MaxPool2d(3, 2, 1)): all nine 16-B window loads issued unconditionally from clamped
// coordinates before any compare (the generic loop's bounds branches serialised them), the
// out-of-image taps masked afterwards in the same a-major order; the argmax bytes of a
// channel vector leave as one 8-B store.
template <typename T>
__global__ void __launch_bounds__(256) maxpool_fwd_k3(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ idx, int n,
                                                     int h, int w, int c, int ho, int wo, int s, int p, FastDiv f_cv, FastDiv f_wo,
                                                     FastDiv f_ho) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  const int cv = c / V;
  const long total = (long)n * ho * wo * cv;  // < 2^31 (host-checked): 32-bit index math
  GRID_STRIDE_XCD(i, total) {
    const uint32_t ii = (uint32_t)i, q0 = fdiv(ii, f_cv), q1 = fdiv(q0, f_wo), img = fdiv(q1, f_ho);
    const int ch = (int)(ii - q0 * cv) * V;
    const int ow = (int)(q0 - q1 * wo), oh = (int)(q1 - img * ho);
    const int h0 = oh * s - p, w0 = ow * s - p;
    V16 v[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hh = min(max(h0 + t / 3, 0), h - 1), ww = min(max(w0 + t % 3, 0), w - 1);
      v[t] = *(const V16*)(x + (((long)img * h + hh) * w + ww) * c + ch);
    }
    float best[V];
    int bi[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { best[j] = -INFINITY; bi[j] = -1; }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hh = h0 + t / 3, ww = w0 + t % 3;
      if ((unsigned)hh >= (unsigned)h || (unsigned)ww >= (unsigned)w) continue;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float f = to_f(v[t][j]);
        if (bi[j] < 0 || f > best[j] || (f != f && best[j] == best[j])) { best[j] = f; bi[j] = t; }
      }
    }
    V16 o;
    const long oi = (((long)img * ho + oh) * wo + ow) * c + ch;
    unsigned long long ib = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      o[j] = from_f<T>(best[j]);
      ib |= (unsigned long long)(bi[j] < 0 ? 0 : bi[j]) << (8 * j);
    }
    *(V16*)(y + oi) = o;
    if (idx == nullptr) continue;  // inference: no backward reads the argmax bytes
    if constexpr (V == 8) {
      *(unsigned long long*)(idx + oi) = ib;
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) idx[oi + j] = (uint8_t)(ib >> (8 * j));
    }
  }
}
// Backward of the 3x3 stride-2 pool: an input pixel is covered by at most 2 x 2 windows; their
// dY vectors and argmax bytes are loaded unconditionally (clamped), then matched.
template <typename T>
__global__ void __launch_bounds__(256) maxpool_bwd_k3s2(const T* __restrict__ dy, const uint8_t* __restrict__ idx, T* __restrict__ dx,
                                                       int n, int h, int w, int c, int ho, int wo, int p, FastDiv f_cv, FastDiv f_w,
                                                       FastDiv f_h) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  const int cv = c / V;
  const long total = (long)n * h * w * cv;  // < 2^31 (host-checked)
  GRID_STRIDE_XCD(i, total) {
    const uint32_t ii = (uint32_t)i, q0 = fdiv(ii, f_cv), q1 = fdiv(q0, f_w), img = fdiv(q1, f_h);
    const int ch = (int)(ii - q0 * cv) * V;
    const int iw = (int)(q0 - q1 * w), ih = (int)(q1 - img * h);
    const int oh_lo = max(0, (ih + p - 1) / 2), ow_lo = max(0, (iw + p - 1) / 2);  // (ih + p - k + s) / s
    V16 g[4];
    unsigned long long ib[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int oh = min(oh_lo + (t >> 1), ho - 1), ow = min(ow_lo + (t & 1), wo - 1);
      const long o = (((long)img * ho + oh) * wo + ow) * c + ch;
      g[t] = *(const V16*)(dy + o);
      if constexpr (V == 8) {
        ib[t] = *(const unsigned long long*)(idx + o);
      } else {
        ib[t] = 0;
#pragma unroll
        for (int j = 0; j < V; ++j) ib[t] |= (unsigned long long)idx[o + j] << (8 * j);
      }
    }
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int oh = oh_lo + (t >> 1), ow = ow_lo + (t & 1);
      const int a = ih - (oh * 2 - p), b = iw - (ow * 2 - p);
      if (oh >= ho || ow >= wo || a < 0 || a >= 3 || b < 0 || b >= 3) continue;
      const unsigned want = (unsigned)(a * 3 + b);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (((ib[t] >> (8 * j)) & 0xff) == want) acc[j] += to_f(g[t][j]);
    }
    V16 r;
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = from_f<T>(acc[j]);
    *(V16*)(dx + (((long)img * h + ih) * w + iw) * c + ch) = r;
  }
}

// The same gather for 2 x 2 input pixels per thread (padding 0 or 1): the four pixels of the quad
// (2m + {0, 1}, 2k + {0, 1}) are covered only by the windows (m - 1 + p + {0, 1}, k - 1 + p + {0, 1}),
// so one set of four dY vectors + argmax loads serves four outputs (the per-pixel kernel loaded
// 16 for them).  Each pixel adds its matching windows in the same (oh, ow) order: bit-identical.
template <typename T>
__global__ void __launch_bounds__(256) maxpool_bwd_k3s2_quad(const T* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                            T* __restrict__ dx, int n, int h, int w, int c, int ho, int wo, int p,
                                                            FastDiv f_cv, FastDiv f_w2, FastDiv f_h2) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  const int cv = c / V, w2 = (w + 1) >> 1, h2 = (h + 1) >> 1;
  const long total = (long)n * h2 * w2 * cv;  // < 2^31 (host-checked)
  GRID_STRIDE_XCD(i, total) {
    const uint32_t ii = (uint32_t)i, q0 = fdiv(ii, f_cv), q1 = fdiv(q0, f_w2), img = fdiv(q1, f_h2);
    const int ch = (int)(ii - q0 * cv) * V;
    const int kq = (int)(q0 - q1 * w2), mq = (int)(q1 - img * h2);
    const int oh0 = mq - 1 + p, ow0 = kq - 1 + p;
    V16 g[4];
    unsigned long long ib[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int oh = min(max(oh0 + (t >> 1), 0), ho - 1), ow = min(max(ow0 + (t & 1), 0), wo - 1);
      const long o = (((long)img * ho + oh) * wo + ow) * c + ch;
      g[t] = *(const V16*)(dy + o);
      if constexpr (V == 8) {
        ib[t] = *(const unsigned long long*)(idx + o);
      } else {
        ib[t] = 0;
#pragma unroll
        for (int j = 0; j < V; ++j) ib[t] |= (unsigned long long)idx[o + j] << (8 * j);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ih = 2 * mq + (e >> 1), iw = 2 * kq + (e & 1);
      if (ih >= h || iw >= w) continue;
      float acc[V];
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int oh = oh0 + (t >> 1), ow = ow0 + (t & 1);
        const int a = ih - (oh * 2 - p), b = iw - (ow * 2 - p);
        if (oh < 0 || ow < 0 || oh >= ho || ow >= wo || a < 0 || a >= 3 || b < 0 || b >= 3) continue;
        const unsigned want = (unsigned)(a * 3 + b);
#pragma unroll
        for (int j = 0; j < V; ++j)
          if (((ib[t] >> (8 * j)) & 0xff) == want) acc[j] += to_f(g[t][j]);
      }
      V16 r;
#pragma unroll
      for (int j = 0; j < V; ++j) r[j] = from_f<T>(acc[j]);
      *(V16*)(dx + (((long)img * h + ih) * w + iw) * c + ch) = r;
    }
  }
}

extern "C" int rtsds_maxpool_fwd(const void* x, void* y, uint8_t* idx, int n, int h, int w, int c, int ho, int wo, int k, int s,
                                 int p, int dtype, void* stream) {
  if (k * k > 255 || n <= 0 || ho <= 0 || wo <= 0) return RTSDS_ERR_SHAPE;
  const long total = (long)n * ho * wo * c;
  DISPATCH_T(dtype, {
    if (c % VecT<T>::N == 0 && k == 3 && total < (1L << 31))
      hipLaunchKernelGGL(maxpool_fwd_k3<T>, dim3(ew_blocks(total / VecT<T>::N, 256, 1 << 20)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, idx,
                         n, h, w, c, ho, wo, s, p, fastdiv_make(c / VecT<T>::N), fastdiv_make(wo), fastdiv_make(ho));
    else if (idx == nullptr)
      return RTSDS_ERR_UNSUPPORTED;
    else if (c % VecT<T>::N == 0)
      hipLaunchKernelGGL(maxpool_fwd_vec<T>, dim3(ew_blocks(total / VecT<T>::N)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, idx, n, h, w, c, ho, wo, k, s, p);
    else
      hipLaunchKernelGGL(maxpool_fwd_kernel<T>, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, idx, n, h, w, c, ho, wo, k, s, p);
  });
  RET_LAUNCH();
}
extern "C" int rtsds_maxpool_bwd(const void* dy, const uint8_t* idx, void* dx, int n, int h, int w, int c, int ho, int wo, int k,
                                 int s, int p, int dtype, void* stream) {
  const long total = (long)n * h * w * c;
  if (total <= 0) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, {
    if (c % VecT<T>::N == 0 && k == 3 && s == 2 && (p == 0 || p == 1) && total < (1L << 31)) {
      const long quads = (long)n * ((h + 1) / 2) * ((w + 1) / 2) * (c / VecT<T>::N);
      hipLaunchKernelGGL(maxpool_bwd_k3s2_quad<T>, dim3(ew_blocks(quads, 256, 1 << 20)), dim3(256), 0, (hipStream_t)stream, (const T*)dy,
                         idx, (T*)dx, n, h, w, c, ho, wo, p, fastdiv_make(c / VecT<T>::N), fastdiv_make((w + 1) / 2),
                         fastdiv_make((h + 1) / 2));
    } else if (c % VecT<T>::N == 0 && k == 3 && s == 2 && total < (1L << 31))
      hipLaunchKernelGGL(maxpool_bwd_k3s2<T>, dim3(ew_blocks(total / VecT<T>::N, 256, 1 << 20)), dim3(256), 0, (hipStream_t)stream, (const T*)dy, idx, (T*)dx,
                         n, h, w, c, ho, wo, p, fastdiv_make(c / VecT<T>::N), fastdiv_make(w), fastdiv_make(h));
    else if (c % VecT<T>::N == 0)
      hipLaunchKernelGGL(maxpool_bwd_vec<T>, dim3(ew_blocks(total / VecT<T>::N)), dim3(256), 0, (hipStream_t)stream, (const T*)dy, idx, (T*)dx, n, h, w, c, ho, wo, k, s, p);
    else
      hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const T*)dy, idx, (T*)dx, n, h, w, c, ho, wo, k, s, p);
  });
  RET_LAUNCH();
}

// ------------------------------------------------------------------ adaptive average pool
// ATen start/end indices: [floor(o*in/out), ceil((o+1)*in/out)).
RT_DEV int ap_start(int o, int out, int in) { return (int)(((long)o * in) / out); }
RT_DEV int ap_end(int o, int out, int in) { return (int)(((long)(o + 1) * in + out - 1) / out); }

// One thread per (output pixel, channel); channels fastest -> coalesced NHWC access.
template <typename T>
__global__ void adaptive_avgpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int n, int hi, int wi, int c,
                                            int ho, int wo) {
  const long total = (long)n * ho * wo * c;
  GRID_STRIDE(i, total) {
    const int ch = (int)(i % c);
    long q = i / c;
    const int ow = (int)(q % wo);
    q /= wo;
    const int oh = (int)(q % ho);
    const int img = (int)(q / ho);
    const int h0 = ap_start(oh, ho, hi), h1 = ap_end(oh, ho, hi);
    const int w0 = ap_start(ow, wo, wi), w1 = ap_end(ow, wo, wi);
    const T* b = x + (long)img * hi * wi * c + ch;
    float s = 0.f;
    for (int h = h0; h < h1; ++h)
      for (int w = w0; w < w1; ++w) s += to_f(b[((long)h * wi + w) * c]);
    y[i] = from_f<T>(s / (float)((h1 - h0) * (w1 - w0)));
  }
}
// dx[i] = sum over windows o containing i of dy[o] / area(o).  Window o covers input index i
// iff start(o) <= i < end(o); every such o lies in [floor(i*out/in) - 1, ceil((i+1)*out/in)],
// and each candidate is tested exactly.
template <typename T>
__global__ void adaptive_avgpool_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int n, int hi, int wi, int c,
                                            int ho, int wo) {
  const long total = (long)n * hi * wi * c;
  GRID_STRIDE(i, total) {
    const int ch = (int)(i % c);
    long q = i / c;
    const int iw = (int)(q % wi);
    q /= wi;
    const int ih = (int)(q % hi);
    const int img = (int)(q / hi);
    // candidate output rows: o with start(o) <= ih < end(o)
    const int oh_lo = max(0, (int)(((long)ih * ho) / hi) - 1), oh_hi = min(ho - 1, (int)(((long)(ih + 1) * ho + hi - 1) / hi));
    const int ow_lo = max(0, (int)(((long)iw * wo) / wi) - 1), ow_hi = min(wo - 1, (int)(((long)(iw + 1) * wo + wi - 1) / wi));
    const T* b = dy + (long)img * ho * wo * c + ch;
    float s = 0.f;
    for (int oh = oh_lo; oh <= oh_hi; ++oh) {
      const int h0 = ap_start(oh, ho, hi), h1 = ap_end(oh, ho, hi);
      if (ih < h0 || ih >= h1) continue;
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        const int w0 = ap_start(ow, wo, wi), w1 = ap_end(ow, wo, wi);
        if (iw < w0 || iw >= w1) continue;
        s += to_f(b[((long)oh * wo + ow) * c]) / (float)((h1 - h0) * (w1 - w0));
      }
    }
    dx[i] = from_f<T>(s);
  }
}
extern "C" int rtsds_adaptive_avgpool_fwd(const void* x, void* y, int n, int hi, int wi, int c, int ho, int wo, int dtype,
                                          void* stream) {
  if (n <= 0 || hi <= 0 || wi <= 0 || c <= 0 || ho <= 0 || wo <= 0) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, hipLaunchKernelGGL(adaptive_avgpool_fwd_kernel<T>, dim3(ew_blocks((long)n * ho * wo * c)), dim3(256), 0,
                                       (hipStream_t)stream, (const T*)x, (T*)y, n, hi, wi, c, ho, wo));
  RET_LAUNCH();
}
extern "C" int rtsds_adaptive_avgpool_bwd(const void* dy, void* dx, int n, int hi, int wi, int c, int ho, int wo, int dtype,
                                          void* stream) {
  if (n <= 0 || hi <= 0 || wi <= 0 || c <= 0 || ho <= 0 || wo <= 0) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, hipLaunchKernelGGL(adaptive_avgpool_bwd_kernel<T>, dim3(ew_blocks((long)n * hi * wi * c)), dim3(256), 0,
                                       (hipStream_t)stream, (const T*)dy, (T*)dx, n, hi, wi, c, ho, wo));
  RET_LAUNCH();
}
