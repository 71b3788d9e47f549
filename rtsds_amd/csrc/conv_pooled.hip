// GEMV-sized 1x1 convs on pooled [N, C, 1, 1] vectors (conv_host.h pooled_1x1: the ARM / FFM
// attention convs), one launch per pass, and the FFM attention MLP's forward / backward in one
// launch each (rtsds_pooled_mlp_fwd / _bwd).
#include "conv_host.h"
#include "chan_dev.h"

template <typename T> RT_DEV typename VecT<T>::v16 vzero() {
  typename VecT<T>::v16 z;
#pragma unroll
  for (int j = 0; j < VecT<T>::N; ++j) z[j] = (T)0.0f;
  return z;
}

// y[m][k] = act(sum_c x[m][c] w[k][c] + bias[k]); one wave per output channel k.
// scale (optional, [k]): the eval-mode BatchNorm fold, y = act(acc * scale + bias) (as the GEMM
// epilogue of rtsds_conv2d_fwd_bn; fmaf(acc, 1, b) == acc + b without it)
template <typename T, int MR>
__global__ void __launch_bounds__(256) pooled_fwd_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                        const float* __restrict__ bias, T* __restrict__ y, int m_n, int c,
                                                        int k_n, int act, int accum, float* __restrict__ stats,
                                                        const float* __restrict__ scale) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= k_n) return;
  float acc[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m] = 0.f;
  for (int ci = lane; ci < c; ci += 64) {
    const float wv = to_f(w[(long)k * c + ci]);
#pragma unroll
    for (int m = 0; m < MR; ++m)
      if (m < m_n) acc[m] = fmaf(to_f(x[(long)m * c + ci]), wv, acc[m]);
  }
#pragma unroll
  for (int m = 0; m < MR; ++m)
    if (m < m_n) acc[m] = wave_sum(acc[m]);
  if (lane != 0) return;
  const float bv = bias ? bias[k] : 0.f, sv = scale ? scale[k] : 1.f;
  float mean = 0.f;
#pragma unroll
  for (int m = 0; m < MR; ++m)
    if (m < m_n) {
      float v = fmaf(acc[m], sv, bv);
      acc[m] = v;
      mean += v;
      if (accum) v += to_f(y[(long)m * k_n + k]);
      if (act == RTSDS_ACT_RELU) v = fmaxf(v, 0.f);
      else if (act == RTSDS_ACT_LEAKY) v = v > 0.f ? v : 0.2f * v;
      else if (act == RTSDS_ACT_SIGMOID) v = 1.f / (1.f + expf(-v));
      y[(long)m * k_n + k] = from_f<T>(v);
    }
  if (stats) {
    mean /= (float)m_n;
    float m2 = 0.f;
#pragma unroll
    for (int m = 0; m < MR; ++m)
      if (m < m_n) m2 += (acc[m] - mean) * (acc[m] - mean);
    *(f32x4*)(stats + k * 4) = f32x4{(float)m_n, mean, m2, 0.f};
  }
}

// dx[m][c] (+)= sum_k dy[m][k] w[k][c]; one wave per input channel c, lanes over k.
template <typename T, int MR>
__global__ void __launch_bounds__(256) pooled_dgrad_kernel(const T* __restrict__ dy, const T* __restrict__ w, T* __restrict__ dx,
                                                          int m_n, int c, int k_n, int accum) {
  const int ci = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (ci >= c) return;
  float acc[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m] = 0.f;
  for (int k = lane; k < k_n; k += 64) {
    const float wv = to_f(w[(long)k * c + ci]);
#pragma unroll
    for (int m = 0; m < MR; ++m)
      if (m < m_n) acc[m] = fmaf(to_f(dy[(long)m * k_n + k]), wv, acc[m]);
  }
#pragma unroll
  for (int m = 0; m < MR; ++m)
    if (m < m_n) acc[m] = wave_sum(acc[m]);
  if (lane != 0) return;
#pragma unroll
  for (int m = 0; m < MR; ++m)
    if (m < m_n) {
      const long o = (long)m * c + ci;
      dx[o] = from_f<T>(accum ? to_f(from_f<T>(acc[m])) + to_f(dx[o]) : acc[m]);
    }
}

// dw[k][c] (+)= sum_m dy[m][k] x[m][c] (fp32), dbias[k] (+)= sum_m dy[m][k]; one thread per (k, c).
template <typename T>
__global__ void __launch_bounds__(256) pooled_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ dw,
                                                          float* __restrict__ dbias, int m_n, int c, int k_n, int accum) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= k_n * c) return;
  const int k = i / c, ci = i - k * c;
  float acc = 0.f, bsum = 0.f;
  for (int m0 = 0; m0 < m_n; m0 += 8) {  // 8 rows' loads in flight (clamped), then the FMAs in order
    float g[8], xv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int m = min(m0 + u, m_n - 1);
      g[u] = to_f(dy[(long)m * k_n + k]);
      xv[u] = to_f(x[(long)m * c + ci]);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (m0 + u < m_n) {
        acc = fmaf(g[u], xv[u], acc);
        bsum += g[u];
      }
  }
  dw[i] = accum ? dw[i] + acc : acc;
  if (dbias && ci == 0) dbias[k] = accum ? dbias[k] + bsum : bsum;
}

// Vector forms (C % V == 0): every lane loads whole 16-B chunks, all loads of a lane issued
// before its FMAs -- one memory round trip per wave instead of one per 64 channels (the scalar
// kernels above walked C in 2-B steps: ~14 us for a 512 x 512 GEMV).
template <typename T, int MR>
__global__ void __launch_bounds__(256) pooled_fwd_vec_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                            const float* __restrict__ bias, T* __restrict__ y, int m_n, int c,
                                                            int k_n, int act, int accum, float* __restrict__ stats,
                                                            const float* __restrict__ scale) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= k_n) return;
  float acc[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m] = 0.f;
  for (int cc = lane * V; cc < c; cc += 64 * V) {
    const V16 wv = *(const V16*)(w + (long)k * c + cc);
    V16 xv[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) xv[m] = m < m_n ? *(const V16*)(x + (long)m * c + cc) : vzero<T>();
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int j = 0; j < V; ++j) acc[m] = fmaf(to_f(xv[m][j]), to_f(wv[j]), acc[m]);
  }
#pragma unroll
  for (int m = 0; m < MR; ++m)
    if (m < m_n) acc[m] = wave_sum(acc[m]);
  if (lane != 0) return;
  const float bv = bias ? bias[k] : 0.f, sv = scale ? scale[k] : 1.f;
  float mean = 0.f;
#pragma unroll
  for (int m = 0; m < MR; ++m)
    if (m < m_n) {
      float v = fmaf(acc[m], sv, bv);
      acc[m] = v;
      mean += v;
      if (accum) v += to_f(y[(long)m * k_n + k]);
      if (act == RTSDS_ACT_RELU) v = fmaxf(v, 0.f);
      else if (act == RTSDS_ACT_LEAKY) v = v > 0.f ? v : 0.2f * v;
      else if (act == RTSDS_ACT_SIGMOID) v = 1.f / (1.f + expf(-v));
      y[(long)m * k_n + k] = from_f<T>(v);
    }
  if (stats) {
    mean /= (float)m_n;
    float m2 = 0.f;
#pragma unroll
    for (int m = 0; m < MR; ++m)
      if (m < m_n) m2 += (acc[m] - mean) * (acc[m] - mean);
    *(f32x4*)(stats + k * 4) = f32x4{(float)m_n, mean, m2, 0.f};
  }
}

// bf16, m_n <= 8, C % 8 == 0: one wave per 8-channel chunk of dx, lanes over k (16-B weight
// chunks); the 8 x 8 per-lane partials are summed by a reduce-scatter butterfly (63 shuffles
// instead of 64 full wave sums), after which lane l holds dx[l / 8][ci0 + l % 8].
__global__ void __launch_bounds__(256) pooled_dgrad_vec_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ w,
                                                              bf16* __restrict__ dx, int m_n, int c, int k_n, int accum) {
  const int ci0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 8, lane = threadIdx.x & 63;
  if (ci0 >= c) return;
  float v[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) v[i] = 0.f;
  // KI k-rows per lane with every load issued before the FMAs (clamped, unconditional): one
  // memory round trip per 64 KI rows -- the 512-row loop serialised eight of them (18.6 us)
  constexpr int KI = 4;
  for (int k0 = lane; k0 < k_n; k0 += 64 * KI) {
    bf16x8 wv[KI];
    float g[KI][8];
#pragma unroll
    for (int u = 0; u < KI; ++u) {
      const int k = min(k0 + 64 * u, k_n - 1);
      wv[u] = *(const bf16x8*)(w + (long)k * c + ci0);
#pragma unroll
      for (int m = 0; m < 8; ++m) g[u][m] = (float)dy[(long)min(m, m_n - 1) * k_n + k];
    }
#pragma unroll
    for (int u = 0; u < KI; ++u) {
      if (k0 + 64 * u >= k_n) break;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const float gm = m < m_n ? g[u][m] : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[m * 8 + j] = fmaf(gm, (float)wv[u][j], v[m * 8 + j]);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // keep the half of v[0, 2o) this lane's bit o selects
    const bool hi = (lane & o) != 0;
#pragma unroll
    for (int i = 0; i < o; ++i) {
      const float send = hi ? v[i] : v[i + o];
      const float keep = hi ? v[i + o] : v[i];
      v[i] = keep + __shfl_xor(send, o, 64);
    }
  }
  const int m = lane >> 3;
  if (m < m_n) {
    const long off = (long)m * c + ci0 + (lane & 7);
    // accumulate: rounded first, then added (= storing it and adding the two bf16 gradients)
    dx[off] = (bf16)(accum ? (float)(bf16)v[0] + (float)dx[off] : v[0]);
  }
}

template <typename T>
static void pooled_fwd_launch(const rtsds_conv_desc* d, const void* x, const void* w, const float* bias, void* y, int act,
                              int accum, float* stats, const float* scale, hipStream_t st) {
  if (d->c % VecT<T>::N == 0) {
    if (d->n <= 8)
      hipLaunchKernelGGL((pooled_fwd_vec_kernel<T, 8>), dim3(rt_cdiv(d->k, 4)), dim3(256), 0, st, (const T*)x, (const T*)w,
                         bias, (T*)y, d->n, d->c, d->k, act, accum, stats, scale);
    else
      hipLaunchKernelGGL((pooled_fwd_vec_kernel<T, kPooledMaxRows>), dim3(rt_cdiv(d->k, 4)), dim3(256), 0, st, (const T*)x,
                         (const T*)w, bias, (T*)y, d->n, d->c, d->k, act, accum, stats, scale);
    return;
  }
  if (d->n <= 8)
    hipLaunchKernelGGL((pooled_fwd_kernel<T, 8>), dim3(rt_cdiv(d->k, 4)), dim3(256), 0, st, (const T*)x, (const T*)w, bias,
                       (T*)y, d->n, d->c, d->k, act, accum, stats, scale);
  else
    hipLaunchKernelGGL((pooled_fwd_kernel<T, kPooledMaxRows>), dim3(rt_cdiv(d->k, 4)), dim3(256), 0, st, (const T*)x,
                       (const T*)w, bias, (T*)y, d->n, d->c, d->k, act, accum, stats, scale);
}
template <typename T>
static void pooled_dgrad_launch(const rtsds_conv_desc* d, const void* dy, const void* w, void* dx, int accum, hipStream_t st) {
  if (sizeof(T) == 2 && d->n <= 8 && d->c % 8 == 0) {
    hipLaunchKernelGGL(pooled_dgrad_vec_kernel, dim3(rt_cdiv(d->c / 8, 4)), dim3(256), 0, st, (const bf16*)dy, (const bf16*)w,
                       (bf16*)dx, d->n, d->c, d->k, accum);
    return;
  }
  if (d->n <= 8)
    hipLaunchKernelGGL((pooled_dgrad_kernel<T, 8>), dim3(rt_cdiv(d->c, 4)), dim3(256), 0, st, (const T*)dy, (const T*)w,
                       (T*)dx, d->n, d->c, d->k, accum);
  else
    hipLaunchKernelGGL((pooled_dgrad_kernel<T, kPooledMaxRows>), dim3(rt_cdiv(d->c, 4)), dim3(256), 0, st, (const T*)dy,
                       (const T*)w, (T*)dx, d->n, d->c, d->k, accum);
}

// The three passes of a pooled_1x1() descriptor for the conv entry points (d->dtype picks the
// element type; scale: see pooled_fwd_kernel).
int pooled_fwd(const rtsds_conv_desc* d, const void* x, const void* w, const float* bias, void* y, int act, int accum,
               float* stats, const float* scale, hipStream_t st) {
  DISPATCH_T(d->dtype, pooled_fwd_launch<T>(d, x, w, bias, y, act, accum, stats, scale, st));
  RET_LAUNCH();
}
int pooled_dgrad(const rtsds_conv_desc* d, const void* dy, const void* w, void* dx, int accum, hipStream_t st) {
  DISPATCH_T(d->dtype, pooled_dgrad_launch<T>(d, dy, w, dx, accum, st));
  RET_LAUNCH();
}
int pooled_wgrad(const rtsds_conv_desc* d, const void* x, const void* dy, float* dw, float* dbias, int accum, hipStream_t st) {
  DISPATCH_T(d->dtype, hipLaunchKernelGGL(pooled_wgrad_kernel<T>, dim3(rt_cdiv((long)d->k * d->c, 256)), dim3(256), 0, st,
                                          (const T*)x, (const T*)dy, dw, dbias, d->n, d->c, d->k, accum));
  RET_LAUNCH();
}

// ---- the FFM attention's backward in one launch (build_bisenet.py:67-70: conv1 + ReLU, conv2 +
// sigmoid on the pooled [N, C] vectors).  The unfused chain was six launches of a few hundred
// values each (sigmoid backward, conv2 data / weight gradient, ReLU backward, conv1 data /
// weight gradient).  One workgroup runs the same arithmetic in the same order -- the activation
// gradients rounded to the storage type as act_bwd_kernel stores them, the data gradients as
// pooled_dgrad_kernel forms them (a wave per input channel, lanes over output channels, the
// wave's shuffle sum), the weight gradients as pooled_wgrad_kernel (sums over rows in order) --
// so every result is bit-identical to the chain.
static constexpr int kMlpMaxC = 64, kMlpMaxN = 8, kMlpThreads = 1024;  // 16 waves: a wave per input channel or two
// PART: da is not stored -- it is the channel scale's attention gradient sum_hw dr * f, summed here
// from chan_part_kernel<T, 1, true>'s slice partials (part [n][S][c2]) as chan_final_kernel sums
// and rounds them (rtsds_ffm_att_bwd).
template <typename T, bool PART>
__global__ void __launch_bounds__(kMlpThreads) pooled_mlp_bwd_kernel(const T* __restrict__ da, const float* __restrict__ part, int S,
                                                             const T* __restrict__ a, const T* __restrict__ h,
                                                             const T* __restrict__ p, const T* __restrict__ w1, const T* __restrict__ w2,
                                                             float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                                                             float* __restrict__ db2, T* __restrict__ dp, int n, int c0, int c1, int c2,
                                                             int accum) {
  __shared__ float sg2[kMlpMaxN][kMlpMaxC], sg1[kMlpMaxN][kMlpMaxC], sh[kMlpMaxN][kMlpMaxC], sp[kMlpMaxN][kMlpMaxC];
  __shared__ float sw1[kMlpMaxC * kMlpMaxC], sw2[kMlpMaxC * kMlpMaxC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // every operand staged in LDS up front, each thread's loads clamped and unconditional (one
  // memory round trip for the launch; a load per loop iteration serialised them)
  {
    constexpr int NW = kMlpMaxC * kMlpMaxC / kMlpThreads, NV = (kMlpMaxN * kMlpMaxC + kMlpThreads - 1) / kMlpThreads;
    const int n1 = c1 * c0, n2 = c2 * c1;
    float v1[NW], v2[NW], vd[NV], va[NV], vh[NV], vp[NV];
#pragma unroll
    for (int u = 0; u < NW; ++u) {
      const int e = tid + kMlpThreads * u;
      v1[u] = to_f(w1[min(e, n1 - 1)]);
      v2[u] = to_f(w2[min(e, n2 - 1)]);
    }
    // (m, ch) = (e / 64, e % 64) of the [kMlpMaxN][kMlpMaxC] arrays, zero outside [n][c]
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int e = tid + kMlpThreads * u, m = min(e >> 6, n - 1), ch = e & 63;
      if constexpr (PART) vd[u] = to_f(from_f<T>(slice_sum<32>(part + (long)m * S * c2 + min(ch, c2 - 1), S, c2) * 1.f));
      else vd[u] = to_f(da[m * c2 + min(ch, c2 - 1)]);
      va[u] = to_f(a[m * c2 + min(ch, c2 - 1)]);
      vh[u] = to_f(h[m * c1 + min(ch, c1 - 1)]);
      vp[u] = to_f(p[m * c0 + min(ch, c0 - 1)]);
    }
#pragma unroll
    for (int u = 0; u < NW; ++u) {
      const int e = tid + kMlpThreads * u;
      if (e < n1) sw1[e] = v1[u];
      if (e < n2) sw2[e] = v2[u];
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int e = tid + kMlpThreads * u, m = e >> 6, ch = e & 63;
      if (m >= kMlpMaxN) break;
      // sigmoid backward (act_bwd_kernel, act 3): g * s * (1 - s), stored rounded
      sg2[m][ch] = m < n && ch < c2 ? to_f(from_f<T>(vd[u] * va[u] * (1.f - va[u]))) : 0.f;
      sh[m][ch] = m < n && ch < c1 ? vh[u] : 0.f;
      sp[m][ch] = m < n && ch < c0 ? vp[u] : 0.f;
      sg1[m][ch] = 0.f;
    }
  }
  __syncthreads();
  // conv2 weight / bias gradient (pooled_wgrad_kernel): dw2[k][ci] over the rows in order
  for (int i = tid; i < c2 * c1; i += kMlpThreads) {
    const int k = i / c1, ci = i - k * c1;
    float acc = 0.f, bsum = 0.f;
    for (int m = 0; m < n; ++m) {
      acc = fmaf(sg2[m][k], sh[m][ci], acc);
      bsum += sg2[m][k];
    }
    dw2[i] = accum ? dw2[i] + acc : acc;
    if (db2 && ci == 0) db2[k] = accum ? db2[k] + bsum : bsum;
  }
  // conv2 data gradient (pooled_dgrad_kernel), then the ReLU backward (act_bwd_kernel, act 1)
  for (int ci = wave; ci < c1; ci += kMlpThreads / 64) {
    float acc[kMlpMaxN];
#pragma unroll
    for (int m = 0; m < kMlpMaxN; ++m) acc[m] = 0.f;
    for (int k = lane; k < c2; k += 64) {
      const float wv = sw2[k * c1 + ci];
#pragma unroll
      for (int m = 0; m < kMlpMaxN; ++m) acc[m] = fmaf(sg2[m][k], wv, acc[m]);  // (rows past n: zero)
    }
#pragma unroll
    for (int m = 0; m < kMlpMaxN; ++m) acc[m] = wave_sum(acc[m]);
    if (lane == 0)
#pragma unroll
      for (int m = 0; m < kMlpMaxN; ++m)
        if (m < n) sg1[m][ci] = sh[m][ci] > 0.f ? to_f(from_f<T>(acc[m])) : 0.f;
  }
  __syncthreads();
  // conv1 weight / bias gradient, data gradient into dp (stored, not accumulated)
  for (int i = tid; i < c1 * c0; i += kMlpThreads) {
    const int k = i / c0, ci = i - k * c0;
    float acc = 0.f, bsum = 0.f;
    for (int m = 0; m < n; ++m) {
      acc = fmaf(sg1[m][k], sp[m][ci], acc);
      bsum += sg1[m][k];
    }
    dw1[i] = accum ? dw1[i] + acc : acc;
    if (db1 && ci == 0) db1[k] = accum ? db1[k] + bsum : bsum;
  }
  for (int ci = wave; ci < c0; ci += kMlpThreads / 64) {
    float acc[kMlpMaxN];
#pragma unroll
    for (int m = 0; m < kMlpMaxN; ++m) acc[m] = 0.f;
    for (int k = lane; k < c1; k += 64) {
      const float wv = sw1[k * c0 + ci];
#pragma unroll
      for (int m = 0; m < kMlpMaxN; ++m) acc[m] = fmaf(sg1[m][k], wv, acc[m]);
    }
#pragma unroll
    for (int m = 0; m < kMlpMaxN; ++m) acc[m] = wave_sum(acc[m]);
    if (lane == 0)
#pragma unroll
      for (int m = 0; m < kMlpMaxN; ++m)
        if (m < n) dp[(long)m * c0 + ci] = from_f<T>(acc[m]);
  }
}
// Its forward in one launch: h = relu(conv1(p) + b1), a = sigmoid(conv2(h) + b2) with
// pooled_fwd_kernel's arithmetic per output channel (a wave per channel, lanes over the input
// channels in order, the wave's shuffle sum, then the bias and activation) -- bit-identical to
// its two launches; h is staged (rounded) in LDS between the two layers.
template <typename T>
__global__ void __launch_bounds__(kMlpThreads) pooled_mlp_fwd_kernel(const T* __restrict__ p, const T* __restrict__ w1,
                                                                     const float* __restrict__ b1, const T* __restrict__ w2,
                                                                     const float* __restrict__ b2, T* __restrict__ h, T* __restrict__ a,
                                                                     int n, int c0, int c1, int c2) {
  __shared__ float sx[kMlpMaxN][kMlpMaxC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < kMlpMaxN * kMlpMaxC; e += kMlpThreads) {
    const int m = e >> 6, ch = e & 63;
    sx[m][ch] = m < n && ch < c0 ? to_f(p[m * c0 + ch]) : 0.f;
  }
  __syncthreads();
  auto layer = [&](const T* __restrict__ w, const float* __restrict__ b, T* __restrict__ y, int c, int k_n, int act,
                   float (*keep)[kMlpMaxC]) {
    for (int k = wave; k < k_n; k += kMlpThreads / 64) {
      float acc[kMlpMaxN];
#pragma unroll
      for (int m = 0; m < kMlpMaxN; ++m) acc[m] = 0.f;
      for (int ci = lane; ci < c; ci += 64) {
        const float wv = to_f(w[(long)k * c + ci]);
#pragma unroll
        for (int m = 0; m < kMlpMaxN; ++m) acc[m] = fmaf(sx[m][ci], wv, acc[m]);  // (rows past n: zero)
      }
#pragma unroll
      for (int m = 0; m < kMlpMaxN; ++m) acc[m] = wave_sum(acc[m]);
      if (lane == 0) {
        const float bv = b ? b[k] : 0.f;
#pragma unroll
        for (int m = 0; m < kMlpMaxN; ++m)
          if (m < n) {
            float v = fmaf(acc[m], 1.f, bv);
            if (act == RTSDS_ACT_RELU) v = fmaxf(v, 0.f);
            else v = 1.f / (1.f + expf(-v));
            const T o = from_f<T>(v);
            y[(long)m * k_n + k] = o;
            if (keep) keep[m][k] = to_f(o);
          }
      }
    }
  };
  __shared__ float sh[kMlpMaxN][kMlpMaxC];
  for (int e = tid; e < kMlpMaxN * kMlpMaxC; e += kMlpThreads) sh[e >> 6][e & 63] = 0.f;
  __syncthreads();
  layer(w1, b1, h, c0, c1, RTSDS_ACT_RELU, sh);
  __syncthreads();
  for (int e = tid; e < kMlpMaxN * kMlpMaxC; e += kMlpThreads) sx[e >> 6][e & 63] = sh[e >> 6][e & 63];
  __syncthreads();
  layer(w2, b2, a, c1, c2, RTSDS_ACT_SIGMOID, nullptr);
}
static int mlp_check(int n, int c0, int c1, int c2) {
  if (n <= 0 || n > kMlpMaxN || c0 <= 0 || c1 <= 0 || c2 <= 0 || c0 > kMlpMaxC || c1 > kMlpMaxC || c2 > kMlpMaxC)
    return RTSDS_ERR_UNSUPPORTED;
  return RTSDS_OK;
}
extern "C" int rtsds_pooled_mlp_fwd(const void* p, const void* w1, const float* b1, const void* w2, const float* b2, void* h,
                                    void* a, int n, int c0, int c1, int c2, int dtype, void* stream) {
  if (int e = mlp_check(n, c0, c1, c2)) return e;
  if (!p || !w1 || !w2 || !h || !a) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, hipLaunchKernelGGL(pooled_mlp_fwd_kernel<T>, dim3(1), dim3(kMlpThreads), 0, (hipStream_t)stream, (const T*)p,
                                       (const T*)w1, b1, (const T*)w2, b2, (T*)h, (T*)a, n, c0, c1, c2));
  RET_LAUNCH();
}
extern "C" int rtsds_pooled_mlp_bwd(const void* da, const void* a, const void* h, const void* p, const void* w1, const void* w2,
                                    float* dw1, float* db1, float* dw2, float* db2, void* dp, int n, int c0, int c1, int c2,
                                    int accumulate, int dtype, void* stream) {
  if (int e = mlp_check(n, c0, c1, c2)) return e;
  if (!da || !a || !h || !p || !w1 || !w2 || !dw1 || !dw2 || !dp) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, hipLaunchKernelGGL((pooled_mlp_bwd_kernel<T, false>), dim3(1), dim3(kMlpThreads), 0, (hipStream_t)stream,
                                       (const T*)da, (const float*)nullptr, 0, (const T*)a, (const T*)h, (const T*)p, (const T*)w1,
                                       (const T*)w2, dw1, db1, dw2, db2, (T*)dp, n, c0, c1, c2, accumulate ? 1 : 0));
  RET_LAUNCH();
}
// The FeatureFusionModule attention's whole backward from the channel scale's output gradient dr
// and the feature f ([n][hw][c], r = f * a + f): the attention gradient's slice partials
// (chan_part_kernel<T, 1, true>, as rtsds_chscale_bwd's da), then one launch that sums them and
// runs rtsds_pooled_mlp_bwd's body.  Two launches for the chain's three; same bits.
// ws: rtsds_gap_workspace(n, hw, c) bytes.
extern "C" int rtsds_ffm_att_bwd(const void* dr, const void* f, const void* a, const void* h, const void* p, const void* w1,
                                 const void* w2, float* dw1, float* db1, float* dw2, float* db2, void* dp, int n, long hw, int c,
                                 int accumulate, int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (int e = mlp_check(n, c, c, c)) return e;
  if (hw <= 0 || !dr || !f || !a || !h || !p || !w1 || !w2 || !dw1 || !dw2 || !dp) return RTSDS_ERR_SHAPE;
  if (c % (dtype == RTSDS_BF16 ? 8 : 4) == 0) return RTSDS_ERR_UNSUPPORTED;  // the reductions' scalar route
  const int S = chan_slices(n, hw);
  if (ws_bytes < (size_t)n * S * c * 4) return RTSDS_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  DISPATCH_T(dtype, {
    hipLaunchKernelGGL((chan_part_kernel<T, 1, true>), dim3(S, n, 1), dim3(256), 0, st, (const T*)dr, (const T*)f, part, hw, c);
    hipLaunchKernelGGL((pooled_mlp_bwd_kernel<T, true>), dim3(1), dim3(kMlpThreads), 0, st, (const T*)nullptr, (const float*)part, S,
                       (const T*)a, (const T*)h, (const T*)p, (const T*)w1, (const T*)w2, dw1, db1, dw2, db2, (T*)dp, n, c, c, c,
                       accumulate ? 1 : 0);
  });
  RET_LAUNCH();
}
