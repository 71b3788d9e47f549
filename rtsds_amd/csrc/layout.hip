// Layout / dtype conversion and pointwise activations (gfx950).
#include "ew_common.h"

// ------------------------------------------------------------------ layout / dtype
// NCHW fp32 (the reference's input tensors) -> NHWC T.
template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x, T* __restrict__ y, int n, int c, long hw) {
  const long total = (long)n * c * hw;
  GRID_STRIDE(i, total) {
    const int ch = (int)(i % c);
    const long p = i / c;
    const long img = p / hw, s = p - img * hw;
    y[i] = from_f<T>(x[(img * c + ch) * hw + s]);
  }
}
extern "C" int rtsds_nchw_to_nhwc(const float* x, void* y, int n, int c, int h, int w, int dtype, void* stream) {
  const long total = (long)n * c * h * w;
  if (total <= 0) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, x, (T*)y, n, c, (long)h * w));
  RET_LAUNCH();
}

// NCHW fp32 -> NHWC T with channel pitch cp >= c, channels c..cp-1 zero: the image batch in
// the layout its convs gather (3 -> 4 channels: the superpixel view of the stem / spatial-path
// convs, conv_host.h sp_path), so they skip their own pad pass.  One thread per pixel.
template <typename T, int CP>
__global__ void nchw_to_nhwc_pad_kernel(const float* __restrict__ x, T* __restrict__ y, int c, long hw, long pixels) {
  GRID_STRIDE(p, pixels) {
    const long img = p / hw, s = p - img * hw;
    T v[CP];
#pragma unroll
    for (int ch = 0; ch < CP; ++ch) v[ch] = from_f<T>(ch < c ? x[(img * c + ch) * hw + s] : 0.f);
    if constexpr (CP * sizeof(T) == 8) {
      typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
      *(u32x2*)(y + p * CP) = __builtin_bit_cast(u32x2, v);
    } else {
#pragma unroll
      for (int ch = 0; ch < CP; ++ch) y[p * CP + ch] = v[ch];
    }
  }
}
// Same for planes of a multiple of 4 pixels: 4 pixels per thread, one 16-B load per channel
// plane and 16-B stores, the image index from the grid (no 64-bit divisions).
template <typename T>
__global__ void nchw_to_nhwc_pad4_x4_kernel(const float* __restrict__ x, T* __restrict__ y, int c, int hw4) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  typedef __attribute__((ext_vector_type(4))) float f32x4;
  const int img = blockIdx.y;
  const float* xi = x + (long)img * c * hw4 * 4;
  T* yi = y + (long)img * hw4 * 16;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < hw4; q += gridDim.x * 256) {
    f32x4 v[4];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) v[ch] = ch < c ? ((const f32x4*)(xi + (long)ch * hw4 * 4))[q] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 16 / V; ++k) {
      V16 r;
#pragma unroll
      for (int j = 0; j < V; ++j) r[j] = from_f<T>(v[(k * V + j) & 3][(k * V + j) >> 2]);
      ((V16*)(yi + (long)q * 16))[k] = r;
    }
  }
}
extern "C" int rtsds_nchw_to_nhwc_pad(const float* x, void* y, int n, int c, int h, int w, int pitch, int dtype, void* stream) {
  const long px = (long)n * h * w;
  if (px <= 0 || c <= 0 || pitch != 4 || c > pitch) return RTSDS_ERR_UNSUPPORTED;
  const long hw = (long)h * w;
  // 16-B vector loads / stores: only for 16-B aligned bases (a view with a storage offset
  // that is not a multiple of 4 floats takes the per-pixel kernel)
  if (hw % 4 == 0 && hw / 4 < INT_MAX && n <= 65535 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
    const int hw4 = (int)(hw / 4);
    DISPATCH_T(dtype, hipLaunchKernelGGL((nchw_to_nhwc_pad4_x4_kernel<T>), dim3(std::min(rt_cdiv(hw4, 256), 4096), n), dim3(256), 0,
                                         (hipStream_t)stream, x, (T*)y, c, hw4));
  } else {
    DISPATCH_T(dtype, hipLaunchKernelGGL((nchw_to_nhwc_pad_kernel<T, 4>), dim3(ew_blocks(px)), dim3(256), 0, (hipStream_t)stream, x,
                                         (T*)y, c, hw, px));
  }
  RET_LAUNCH();
}

// dst (dtype_dst) = src (dtype_src), elementwise.
template <typename S, typename D>
__global__ void cast_kernel(const S* __restrict__ s, D* __restrict__ d, long n) {
  GRID_STRIDE(i, n) d[i] = from_f<D>(to_f(s[i]));
}
extern "C" int rtsds_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, void* stream) {
  if (n <= 0) return n == 0 ? RTSDS_OK : RTSDS_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int b = ew_blocks(n);
  if (src_dtype == RTSDS_F32 && dst_dtype == RTSDS_BF16) hipLaunchKernelGGL((cast_kernel<float, bf16>), dim3(b), dim3(256), 0, st, (const float*)src, (bf16*)dst, n);
  else if (src_dtype == RTSDS_BF16 && dst_dtype == RTSDS_F32) hipLaunchKernelGGL((cast_kernel<bf16, float>), dim3(b), dim3(256), 0, st, (const bf16*)src, (float*)dst, n);
  else if (src_dtype == RTSDS_F32 && dst_dtype == RTSDS_F32) hipLaunchKernelGGL((cast_kernel<float, float>), dim3(b), dim3(256), 0, st, (const float*)src, (float*)dst, n);
  else if (src_dtype == RTSDS_BF16 && dst_dtype == RTSDS_BF16) hipLaunchKernelGGL((cast_kernel<bf16, bf16>), dim3(b), dim3(256), 0, st, (const bf16*)src, (bf16*)dst, n);
  else if (src_dtype == RTSDS_F32 && dst_dtype == RTSDS_F16) hipLaunchKernelGGL((cast_kernel<float, f16>), dim3(b), dim3(256), 0, st, (const float*)src, (f16*)dst, n);
  else if (src_dtype == RTSDS_F16 && dst_dtype == RTSDS_F32) hipLaunchKernelGGL((cast_kernel<f16, float>), dim3(b), dim3(256), 0, st, (const f16*)src, (float*)dst, n);
  else return RTSDS_ERR_UNSUPPORTED;
  RET_LAUNCH();
}

// Channel-slice copy: dst[r][doff + j] = src[r][soff + j], j < cnt  (torch.cat / its backward
// split along channels, build_bisenet.py:72,153).
template <typename T>
__global__ void copy_channels_kernel(const T* __restrict__ s, int sld, int soff, T* __restrict__ d, int dld, int doff, long rows, int cnt,
                                     int acc) {
  const long total = rows * cnt;
  GRID_STRIDE(i, total) {
    const long r = i / cnt;
    const int j = (int)(i - r * cnt);
    T* o = d + r * dld + doff + j;
    const T v = s[r * sld + soff + j];
    *o = acc ? from_f<T>(to_f(*o) + to_f(v)) : v;
  }
}
template <typename T>
__global__ void copy_channels_vec_kernel(const T* __restrict__ s, int sld, int soff, T* __restrict__ d, int dld, int doff, long rows, int cnt,
                                         int acc) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  const int cv = cnt / V;
  const long total = rows * cv;
  GRID_STRIDE(i, total) {
    const long r = i / cv;
    const int j = (int)(i - r * cv) * V;
    V16* o = (V16*)(d + r * dld + doff + j);
    V16 v = *(const V16*)(s + r * sld + soff + j);
    if (acc) {
      const V16 a = *o;
#pragma unroll
      for (int q = 0; q < V; ++q) v[q] = from_f<T>(to_f(a[q]) + to_f(v[q]));
    }
    *o = v;
  }
}
extern "C" int rtsds_copy_channels(const void* src, int src_ld, int src_off, void* dst, int dst_ld, int dst_off, long rows,
                                   int cnt, int accumulate, int dtype, void* stream) {
  if (rows <= 0 || cnt <= 0) return RTSDS_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    constexpr int V = VecT<T>::N;
    if (cnt % V == 0 && src_ld % V == 0 && dst_ld % V == 0 && src_off % V == 0 && dst_off % V == 0)
      hipLaunchKernelGGL(copy_channels_vec_kernel<T>, dim3(ew_blocks(rows * cnt / V)), dim3(256), 0, st, (const T*)src, src_ld, src_off, (T*)dst, dst_ld, dst_off, rows, cnt,
                         accumulate ? 1 : 0);
    else
      hipLaunchKernelGGL(copy_channels_kernel<T>, dim3(ew_blocks(rows * cnt)), dim3(256), 0, st, (const T*)src, src_ld, src_off, (T*)dst, dst_ld, dst_off, rows, cnt,
                         accumulate ? 1 : 0);
  });
  RET_LAUNCH();
}

// ------------------------------------------------------------------ activations (pointwise)
// act: 1 relu, 2 leaky(0.2), 3 sigmoid.  Backward uses the forward OUTPUT y.
template <typename T>
__global__ void act_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, long n, int act) {
  GRID_STRIDE(i, n) {
    float v = to_f(x[i]);
    if (act == 1) v = fmaxf(v, 0.f);
    else if (act == 2) v = v > 0.f ? v : 0.2f * v;
    else if (act == 3) v = 1.f / (1.f + expf(-v));
    y[i] = from_f<T>(v);
  }
}
template <typename T>
__global__ void act_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y, T* __restrict__ dx, long n, int act, float alpha) {
  GRID_STRIDE(i, n) {
    const float g = to_f(dy[i]);
    float r;
    if (act == 1) r = to_f(y[i]) > 0.f ? g : 0.f;
    else if (act == 2) r = to_f(y[i]) > 0.f ? g : 0.2f * g;
    else if (act == 3) { const float s = to_f(y[i]); r = g * s * (1.f - s); }
    else r = alpha * g;  // act 0: scale (gradient reversal, model.py:9-17)
    dx[i] = from_f<T>(r);
  }
}
extern "C" int rtsds_act_fwd(const void* x, void* y, long n, int act, int dtype, void* stream) {
  if (n <= 0) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, hipLaunchKernelGGL(act_fwd_kernel<T>, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, n, act));
  RET_LAUNCH();
}
extern "C" int rtsds_act_bwd(const void* dy, const void* y, void* dx, long n, int act, float alpha, int dtype, void* stream) {
  if (n <= 0) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, hipLaunchKernelGGL(act_bwd_kernel<T>, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, (const T*)dy, (const T*)y, (T*)dx, n, act, alpha));
  RET_LAUNCH();
}
