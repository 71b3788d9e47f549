// Channel-vector kernels (gfx950): global average pool and the ARM / FFM channel attention
// (chan_* reductions, ffm_head_eval), then the per-pixel class-vector ops -- channel softmax,
// cross-entropy with ignore_index, BCE-with-logits, argmax / pixel accuracy, confusion.
#include "ew_common.h"
#include "class_row.h"
#include "chan_dev.h"

// ------------------------------------------------------------------ global average pool
// y[img][c] = mean_hw x[img][hw][c]   (AdaptiveAvgPool2d(1) / torch.mean over H,W:
// build_bisenet.py:46,75, build_contextpath.py:27-28, model.py:63,82).
//
// Shared per-image channel reduction: out[img][c] = scale * sum_hw a (* b if DOT), in two
// deterministic stages.  Stage 1: grid (S row slices, img, channel chunk) of 256-thread blocks
// laid out [row group][16-B channel vector] (VEC = 8 bf16 / 4 f32 when c allows, else 1) ->
// part[img][s][c] fp32.  Stage 2 sums the S slices in order.  (One block per image would
// leave all but n CUs idle: the ARM / FFM / tail pools have n = 8 images.)
// (the partition, the stage-1 loop and the slice sum: chan_dev.h)
template <typename T>
__global__ void __launch_bounds__(256) chan_final_kernel(const float* __restrict__ part, T* __restrict__ out, int S, int c, float scale) {
  const int img = blockIdx.y, ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  out[(long)img * c + ch] = from_f<T>(slice_sum(part + (long)img * S * c + ch, S, c) * scale);
}
extern "C" size_t rtsds_gap_workspace(int n, long hw, int c) {
  if (n <= 0 || hw <= 0 || c <= 0) return 256;
  return (size_t)n * chan_slices(n, hw) * c * 4 + 256;
}
template <typename T, bool DOT>
static void chan_reduce(const T* a, const T* b, T* out, int n, long hw, int c, float scale, float* part, hipStream_t st) {
  constexpr int V = VecT<T>::N;
  const int S = chan_slices(n, hw);
  if (c % V == 0)
    hipLaunchKernelGGL((chan_part_kernel<T, V, DOT>), dim3(S, n, rt_cdiv(c, 256 * V)), dim3(256), 0, st, a, b, part, hw, c);
  else
    hipLaunchKernelGGL((chan_part_kernel<T, 1, DOT>), dim3(S, n, rt_cdiv(c, 256)), dim3(256), 0, st, a, b, part, hw, c);
  hipLaunchKernelGGL(chan_final_kernel<T>, dim3(rt_cdiv(c, 256), n), dim3(256), 0, st, (const float*)part, out, S, c, scale);
}
// accum: dx += the (rounded) gradient -- the other reader's contribution already in dx
// (functional.GradJoin), the same two roundings as autograd's separate elementwise add
template <typename T>
__global__ void gap_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int n, long hw, int c, int accum) {
  const long total = (long)n * hw * c;
  const float inv = 1.f / (float)hw;
  GRID_STRIDE(i, total) {
    const int ch = (int)(i % c);
    const long img = i / c / hw;
    const T g = from_f<T>(to_f(dy[img * c + ch]) * inv);
    dx[i] = accum ? from_f<T>(to_f(dx[i]) + to_f(g)) : g;
  }
}
extern "C" int rtsds_gap_fwd(const void* x, void* y, int n, long hw, int c, int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (n <= 0 || hw <= 0 || c <= 0) return RTSDS_ERR_SHAPE;
  if (ws_bytes < rtsds_gap_workspace(n, hw, c)) return RTSDS_ERR_WORKSPACE;
  DISPATCH_T(dtype, (chan_reduce<T, false>((const T*)x, nullptr, (T*)y, n, hw, c, 1.f / (float)hw, (float*)ws, (hipStream_t)stream)));
  RET_LAUNCH();
}
// 16-B channel vectors (c % 8 == 0, bf16): one division per 8 elements instead of two per element
__global__ void gap_bwd_vec_kernel(const bf16* __restrict__ dy, bf16* __restrict__ dx, long pixels, long hw, int cv, int accum,
                                   float inv) {
  const long total = pixels * cv;
  GRID_STRIDE(i, total) {
    const long p = i / cv;
    const int q = (int)(i - p * cv);
    const long img = p / hw;
    const bf16x8 g = *(const bf16x8*)(dy + (img * cv + q) * 8);
    bf16x8 o;
    if (accum) o = *(const bf16x8*)(dx + i * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bf16 v = from_f<bf16>(to_f(g[j]) * inv);
      o[j] = accum ? from_f<bf16>(to_f(o[j]) + to_f(v)) : v;
    }
    *(bf16x8*)(dx + i * 8) = o;
  }
}
extern "C" int rtsds_gap_bwd(const void* dy, void* dx, int n, long hw, int c, int accumulate, int dtype, void* stream) {
  if (n <= 0 || hw <= 0 || c <= 0) return RTSDS_ERR_SHAPE;
  if (dtype == RTSDS_BF16 && c % 8 == 0) {
    const long pixels = (long)n * hw;
    hipLaunchKernelGGL(gap_bwd_vec_kernel, dim3(ew_blocks(pixels * (c / 8))), dim3(256), 0, (hipStream_t)stream, (const bf16*)dy,
                       (bf16*)dx, pixels, hw, c / 8, accumulate ? 1 : 0, 1.f / (float)hw);
    RET_LAUNCH();
  }
  DISPATCH_T(dtype, hipLaunchKernelGGL(gap_bwd_kernel<T>, dim3(ew_blocks((long)n * hw * c)), dim3(256), 0, (hipStream_t)stream, (const T*)dy, (T*)dx, n, hw, c, accumulate ? 1 : 0));
  RET_LAUNCH();
}

// ------------------------------------------------------------------ channel attention scale
// mode 0: y = x * a[img][c]           (ARM x*sigmoid, cx2*tail: build_bisenet.py:52,149)
// mode 1: y = x * a[img][c] + x       (FFM: build_bisenet.py:79-80)
template <typename T>
__global__ void chscale_fwd_kernel(const T* __restrict__ x, const T* __restrict__ a, T* __restrict__ y, int n, long hw, int c, int mode) {
  const long total = (long)n * hw * c;
  GRID_STRIDE(i, total) {
    const int ch = (int)(i % c);
    const long img = i / c / hw;
    const float xv = to_f(x[i]), av = to_f(a[img * c + ch]);
    y[i] = from_f<T>(mode ? fmaf(xv, av, xv) : xv * av);
  }
}
template <typename T>
__global__ void chscale_bwd_dx_kernel(const T* __restrict__ dy, const T* __restrict__ a, T* __restrict__ dx, int n, long hw, int c, int mode) {
  const long total = (long)n * hw * c;
  GRID_STRIDE(i, total) {
    const int ch = (int)(i % c);
    const long img = i / c / hw;
    const float av = to_f(a[img * c + ch]) + (mode ? 1.f : 0.f);
    dx[i] = from_f<T>(to_f(dy[i]) * av);
  }
}
// 16-B channel vectors (c % V == 0, 16-B aligned tensors): grid (chunks of an image's vectors, img),
// one 32-bit division per vector instead of two 64-bit ones per element; the per-element
// expressions are the scalar kernels' (BWD: chscale_bwd_dx_kernel's).  b: a second [n][c] scale
// (mode 0 only), y = round(round(x * a) * b) -- two chscale_fwd_kernel launches without the
// intermediate tensor (BiSeNet's cx2 = (f4 * att2) * tail, build_bisenet.py:52,149).
template <typename T, bool BWD>
__global__ void __launch_bounds__(256) chscale_vec_kernel(const T* __restrict__ x, const T* __restrict__ a, const T* __restrict__ b,
                                                          T* __restrict__ y, unsigned per_img, unsigned cv, int mode) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  const long img = blockIdx.y;
  const V16* xi = (const V16*)x + img * per_img;
  const V16* ai = (const V16*)a + img * cv;
  const V16* bi = b ? (const V16*)b + img * cv : nullptr;
  V16* yi = (V16*)y + img * per_img;
  for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < per_img; e += gridDim.x * 256u) {
    const unsigned q = e % cv;
    const V16 xv = xi[e], av = ai[q];
    V16 o;
    if (BWD) {
      const float one = mode ? 1.f : 0.f;
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = from_f<T>(to_f(xv[j]) * (to_f(av[j]) + one));
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float xf = to_f(xv[j]), af = to_f(av[j]);
        o[j] = from_f<T>(mode ? fmaf(xf, af, xf) : xf * af);
      }
      if (bi) {
        const V16 bv = bi[q];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = from_f<T>(to_f(o[j]) * to_f(bv[j]));
      }
    }
    yi[e] = o;
  }
}
// whether the vector kernels take the tensors: whole 16-B channel vectors, 16-B aligned, 32-bit
// vector indices within an image
template <typename T>
static bool chscale_vec_ok(int n, long hw, int c, std::initializer_list<const void*> ptrs) {
  constexpr int V = VecT<T>::N;
  if (c % V || n > 65535 || hw * (c / V) >= (1L << 31)) return false;
  for (const void* p : ptrs)
    if ((size_t)p & 15) return false;
  return true;
}
template <typename T, bool BWD>
static void chscale_vec(const T* x, const T* a, const T* b, T* y, int n, long hw, int c, int mode, hipStream_t st) {
  const long per_img = hw * (c / VecT<T>::N);
  hipLaunchKernelGGL((chscale_vec_kernel<T, BWD>), dim3(ew_blocks(per_img, 256, std::max(1, 8192 / n)), n), dim3(256), 0, st, x, a, b, y,
                     (unsigned)per_img, (unsigned)(c / VecT<T>::N), mode);
}
extern "C" int rtsds_chscale_fwd(const void* x, const void* a, void* y, int n, long hw, int c, int mode, int dtype, void* stream) {
  const long total = (long)n * hw * c;
  if (total <= 0) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, {
    if (chscale_vec_ok<T>(n, hw, c, {x, a, y}))
      chscale_vec<T, false>((const T*)x, (const T*)a, (const T*)nullptr, (T*)y, n, hw, c, mode, (hipStream_t)stream);
    else
      hipLaunchKernelGGL(chscale_fwd_kernel<T>, dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (const T*)a, (T*)y, n, hw, c, mode);
  });
  RET_LAUNCH();
}
extern "C" int rtsds_chscale2_fwd(const void* x, const void* a, const void* b, void* y, int n, long hw, int c, int dtype,
                                  void* stream) {
  if (n <= 0 || hw <= 0 || c <= 0 || !x || !a || !b || !y) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, {
    if (!chscale_vec_ok<T>(n, hw, c, {x, a, b, y})) return RTSDS_ERR_UNSUPPORTED;
    chscale_vec<T, false>((const T*)x, (const T*)a, (const T*)b, (T*)y, n, hw, c, 0, (hipStream_t)stream);
  });
  RET_LAUNCH();
}
// Inference tail of the FeatureFusionModule plus BiSeNet's final 1x1 conv (build_bisenet.py:75-80,
// 167): a = sigmoid(conv2(relu(conv1(GAP(f))))), r = f * a + f, out = conv(r) + bias, for a
// narrow class map f [N][hw][C] (C <= 32).  Unfused these are 8 launches (two-stage GAP, two
// pooled 1x1 convs, the channel scale, two channel pads and the padded GEMM: ~54 us at bs 8,
// all launch-bound).  Two launches here: (1) chan_part_kernel's GAP partials over FFM_CHUNK-pixel
// slices of each image; (2) grid (slices, N): every workgroup sums its image's partials in slice
// order, evaluates the two pooled convs in LDS, stages its slice of pixels in LDS (coalesced 16-B
// loads), maps each pixel in place (one pixel per thread, the C x C head weights in LDS) and writes
// the slice back with 16-B stores.  (One launch whose 64 workgroups each re-read their whole image
// for the GAP ran one wave per CU through the 19 x 19 per-pixel maps: 21.7 us.)  Each intermediate
// is rounded to T where the unfused chain stores it.
static constexpr int kFfmChunk = 256;  // pixels per slice / workgroup
template <typename T, int C>
__global__ void __launch_bounds__(256) ffm_head_apply_kernel(const float* __restrict__ part, const T* __restrict__ f,
                                                             const T* __restrict__ w1, const float* __restrict__ b1,
                                                             const T* __restrict__ w2, const float* __restrict__ b2,
                                                             const T* __restrict__ w3, const float* __restrict__ b3,
                                                             T* __restrict__ out, int hw) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  __shared__ float wl[3][C][C + 1];
  __shared__ float gap[C], hid[C], att[C], bias3[C];
  __shared__ __attribute__((aligned(16))) T stage[kFfmChunk * C];
  const int tid = threadIdx.x, img = blockIdx.y, S = gridDim.x;
  const T* fi = f + (long)img * hw * C;
  for (int e = tid; e < C * C; e += 256) {
    const int o = e / C, i = e - o * C;
    wl[0][o][i] = to_f(w1[e]);
    wl[1][o][i] = to_f(w2[e]);
    wl[2][o][i] = to_f(w3[e]);
  }
  // this slice's pixels, in flight while the attention vector is formed
  const int p0 = blockIdx.x * kFfmChunk, np = min(kFfmChunk, hw - p0);  // np % V == 0 (host: hw % V == 0)
  const int nvec = np * C / V;
  const V16* src = (const V16*)(fi + (long)p0 * C);
  for (int e = tid; e < nvec; e += 256) ((V16*)stage)[e] = src[e];
  if (tid < C) {  // GAP: chan_final_kernel's sum
    gap[tid] = to_f(from_f<T>(slice_sum(part + (long)img * S * C + tid, S, C) * (1.f / (float)hw)));
    bias3[tid] = b3 ? b3[tid] : 0.f;
  }
  __syncthreads();
  if (tid < C) {
    float v = b1 ? b1[tid] : 0.f;
    for (int i = 0; i < C; ++i) v = fmaf(wl[0][tid][i], gap[i], v);
    hid[tid] = to_f(from_f<T>(fmaxf(v, 0.f)));
  }
  __syncthreads();
  if (tid < C) {
    float v = b2 ? b2[tid] : 0.f;
    for (int i = 0; i < C; ++i) v = fmaf(wl[1][tid][i], hid[i], v);
    att[tid] = to_f(from_f<T>(1.f / (1.f + expf(-v))));
  }
  __syncthreads();
  for (int p = tid; p < np; p += 256) {
    T* q = stage + p * C;
    float r[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const float x = to_f(q[i]);
      r[i] = to_f(from_f<T>(fmaf(x, att[i], x)));
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
      float v = bias3[k];
#pragma unroll
      for (int i = 0; i < C; ++i) v = fmaf(wl[2][k][i], r[i], v);
      q[k] = from_f<T>(v);
    }
  }
  __syncthreads();
  V16* dst = (V16*)(out + ((long)img * hw + p0) * C);
  for (int e = tid; e < nvec; e += 256) dst[e] = ((const V16*)stage)[e];
}
extern "C" size_t rtsds_ffm_head_eval_workspace(int n, long hw, int c) {
  if (n <= 0 || hw <= 0 || c <= 0) return 256;
  return (size_t)n * ((hw + kFfmChunk - 1) / kFfmChunk) * c * 4 + 256;
}
extern "C" int rtsds_ffm_head_eval(const void* f, const void* w1, const float* b1, const void* w2, const float* b2,
                                   const void* w3, const float* b3, void* out, int n, long hw, int c, int dtype, void* ws,
                                   size_t ws_bytes, void* stream) {
  if (n <= 0 || n > 65535 || hw <= 0 || hw >= (1L << 31)) return RTSDS_ERR_SHAPE;
  if (c != 19) return RTSDS_ERR_UNSUPPORTED;  // instantiated for the 19-class maps
  const int V = dtype == RTSDS_BF16 ? 8 : 4;
  if (hw % V) return RTSDS_ERR_UNSUPPORTED;
  if (ws_bytes < rtsds_ffm_head_eval_workspace(n, hw, c)) return RTSDS_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int S = (int)((hw + kFfmChunk - 1) / kFfmChunk);
  float* part = (float*)ws;
  DISPATCH_T(dtype, {
    hipLaunchKernelGGL((chan_part_kernel<T, 1, false>), dim3(S, n, 1), dim3(256), 0, st, (const T*)f, (const T*)nullptr, part,
                       hw, c);
    hipLaunchKernelGGL((ffm_head_apply_kernel<T, 19>), dim3(S, n), dim3(256), 0, st, (const float*)part, (const T*)f, (const T*)w1,
                       b1, (const T*)w2, b2, (const T*)w3, b3, (T*)out, (int)hw);
  });
  RET_LAUNCH();
}
// Training form of the FeatureFusionModule's attention tail (build_bisenet.py:75-80) after the
// BatchNorm apply that also left the GAP partials (rtsds_bn_fwd_gap): unfused these are
// chan_final_kernel, pooled_mlp_fwd_kernel and chscale_fwd_kernel (mode 1).  Grid (pixel chunks,
// N): every workgroup sums its image's partials in slice order (slice_sum's order; staged in LDS
// when they fit, so the memory round trips do not queue), evaluates the two pooled convs for its
// image with pooled_mlp_fwd_kernel's arithmetic (a wave per output channel, lanes over the input
// channels, the wave's shuffle sum, then bias and activation) and maps its pixels
// r = round(fma(f, a, f)).  The first workgroup of an image stores pooled / hid / att for the
// backward.  Each intermediate is rounded to T where the unfused chain stores it.  r has pixel
// pitch ldr: C (dense), or the zero-padded pitch a reading conv gathers (RTSDS_INPUT_PADDED),
// written from an LDS copy of the chunk -- that conv's channel-pad launch is then not needed.
static constexpr int kFfmPartMax = 256;  // slices per image whose partials are staged in LDS
template <typename T, int C>
__global__ void __launch_bounds__(256) ffm_att_scale_kernel(const float* __restrict__ part, int S, const T* __restrict__ f,
                                                            const T* __restrict__ w1, const float* __restrict__ b1,
                                                            const T* __restrict__ w2, const float* __restrict__ b2,
                                                            T* __restrict__ pooled, T* __restrict__ hid_o, T* __restrict__ att_o,
                                                            T* __restrict__ r, int hw, float inv, int ldr) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  constexpr int KI = (C + 3) / 4;                          // output channels per wave
  constexpr int NV = (kFfmChunk * C / V + 255) / 256;      // pixel vectors per thread
  static_assert(C <= 64, "one input channel per lane");
  __shared__ float sp[kFfmPartMax * C];
  __shared__ float gap[C], hid[C], att[C];
  __shared__ __attribute__((aligned(16))) T stage[kFfmChunk * C];  // (ldr > C: the chunk's r before the padded stores)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, img = blockIdx.y;
  const bool first = blockIdx.x == 0;
  // weights, biases and this chunk's pixels in flight while the attention vector is formed
  float w1v[KI], w2v[KI], b1v[KI], b2v[KI];
#pragma unroll
  for (int u = 0; u < KI; ++u) {
    const int k = wave + 4 * u;
    const bool ok = k < C && lane < C;
    const int e = ok ? k * C + lane : 0;
    w1v[u] = ok ? to_f(w1[e]) : 0.f;
    w2v[u] = ok ? to_f(w2[e]) : 0.f;
    b1v[u] = b1 && k < C ? b1[k] : 0.f;
    b2v[u] = b2 && k < C ? b2[k] : 0.f;
  }
  const int p0 = blockIdx.x * kFfmChunk, np = min(kFfmChunk, hw - p0);  // np % V == 0 (host: hw % V == 0)
  const int nvec = np * C / V;
  const long off = ((long)img * hw + p0) * C;
  const V16* src = (const V16*)(f + off);
  V16 xv[NV];
#pragma unroll
  for (int u = 0; u < NV; ++u) xv[u] = src[min(tid + 256 * u, nvec - 1)];
  // GAP: chan_final_kernel's sum
  const float* pp = part + (long)img * S * C;
  const bool staged = S <= kFfmPartMax;
  if (staged)
    for (int e = tid; e < S * C; e += 256) sp[e] = pp[e];
  __syncthreads();
  if (tid < C) {
    float s = 0.f;
    if (staged)
      for (int q = 0; q < S; ++q) s += sp[q * C + tid];
    else
      s = slice_sum(pp + tid, S, C);
    const T o = from_f<T>(s * inv);
    gap[tid] = to_f(o);
    if (first) pooled[(long)img * C + tid] = o;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < KI; ++u) {
    const int k = wave + 4 * u;
    if (k >= C) break;
    float acc = 0.f;
    if (lane < C) acc = fmaf(gap[lane], w1v[u], acc);
    acc = wave_sum(acc);
    if (lane == 0) {
      const T o = from_f<T>(fmaxf(fmaf(acc, 1.f, b1v[u]), 0.f));
      hid[k] = to_f(o);
      if (first) hid_o[(long)img * C + k] = o;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < KI; ++u) {
    const int k = wave + 4 * u;
    if (k >= C) break;
    float acc = 0.f;
    if (lane < C) acc = fmaf(hid[lane], w2v[u], acc);
    acc = wave_sum(acc);
    if (lane == 0) {
      const float v = fmaf(acc, 1.f, b2v[u]);
      const T o = from_f<T>(1.f / (1.f + expf(-v)));
      att[k] = to_f(o);
      if (first) att_o[(long)img * C + k] = o;
    }
  }
  __syncthreads();
  const bool dense = ldr == C;
  V16* dst = dense ? (V16*)(r + off) : (V16*)stage;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int e = tid + 256 * u;
    if (e >= nvec) break;
    int ch = (e * V) % C;
    V16 o;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float x = to_f(xv[u][j]);
      o[j] = from_f<T>(fmaf(x, att[ch], x));
      ch = ch + 1 == C ? 0 : ch + 1;
    }
    dst[e] = o;
  }
  if (dense) return;
  // pixel pitch ldr (a multiple of V), zero beyond C: the padded form the final conv gathers
  __syncthreads();
  const int vpp = ldr / V;
  V16* out = (V16*)(r + ((long)img * hw + p0) * ldr);
  for (int e = tid; e < np * vpp; e += 256) {
    const int p = e / vpp, j0 = (e - p * vpp) * V;
    V16 o;
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = j0 + j < C ? stage[p * C + j0 + j] : from_f<T>(0.f);
    out[e] = o;
  }
}
extern "C" int rtsds_ffm_att_scale(const float* part, const void* f, const void* w1, const float* b1, const void* w2,
                                   const float* b2, void* pooled, void* hid, void* att, void* r, int ldr, int n, long hw, int c,
                                   int dtype, void* stream) {
  if (n <= 0 || n > 65535 || hw <= 0 || hw >= (1L << 31) / 64) return RTSDS_ERR_SHAPE;
  if (c != 19) return RTSDS_ERR_UNSUPPORTED;  // instantiated for the 19-class maps
  const int V = dtype == RTSDS_BF16 ? 8 : 4;
  if (hw % V) return RTSDS_ERR_UNSUPPORTED;
  if (ldr != c && (ldr < c || ldr % V || ldr > 64 || ((size_t)r & 15))) return RTSDS_ERR_UNSUPPORTED;
  if (!part || !f || !w1 || !w2 || !pooled || !hid || !att || !r) return RTSDS_ERR_SHAPE;
  const int S = chan_slices(n, hw);
  DISPATCH_T(dtype, hipLaunchKernelGGL((ffm_att_scale_kernel<T, 19>), dim3((int)((hw + kFfmChunk - 1) / kFfmChunk), n), dim3(256),
                                       0, (hipStream_t)stream, part, S, (const T*)f, (const T*)w1, b1, (const T*)w2, b2,
                                       (T*)pooled, (T*)hid, (T*)att, (T*)r, (int)hw, 1.f / (float)hw, ldr));
  RET_LAUNCH();
}
// The channel scale's backward in one pixel pass (c % V == 0): stage 1 of da = sum_hw dy * x reads
// dy through a functor that also stores dx = round(dy * (a + mode)), chscale_bwd_dx_kernel's
// expression -- every element is read by exactly one thread of chan_part_body's partition (as
// bn.hip's BnApplyLoad stores y).  The partials are chan_part_kernel<T, V, true>'s.
template <typename T, int VEC>
struct ScaleGradLoad {
  typedef typename VecT<T>::v16 V16;
  const T* dy;
  T* dx;
  float f[VEC];  // a + mode of the thread's channels
  RT_DEV float at(long o) const { return to_f(dy[o]); }  // (VEC > 1 only)
  RT_DEV V16 vec(long o) const {
    const V16 g = *(const V16*)(dy + o);
    V16 d;
#pragma unroll
    for (int j = 0; j < VEC; ++j) d[j] = from_f<T>(to_f(g[j]) * f[j]);
    *(V16*)(dx + o) = d;
    return g;
  }
};
template <typename T, int VEC>
__global__ void __launch_bounds__(256) chscale_bwd_part_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ a,
                                                               T* __restrict__ dx, float* __restrict__ part, long hw, int c, int mode) {
  typedef typename VecT<T>::v16 V16;
  __shared__ float red[256 * VEC];
  const V16 av = *(const V16*)(a + (long)blockIdx.y * c + chan_part_channel<VEC>(c));
  ScaleGradLoad<T, VEC> ld{dy, dx, {}};
  const float one = mode ? 1.f : 0.f;
#pragma unroll
  for (int j = 0; j < VEC; ++j) ld.f[j] = to_f(av[j]) + one;
  chan_part_body<T, VEC, true>(ld, x, part, hw, c, red);
}
// Backward of y = round(round(x * a) * b) (chscale_vec_kernel with b) in one pass over dy and x,
// for the chain's chscale_bwd_dx + chan_part<DOT> of the outer scale and then of the inner one:
// y1 = round(x * a) and dy1 = round(dy * b) are formed again per element, dx = round(dy1 * a),
// set 0 = sum dy1 * x (a's gradient), set 1 = sum dy * y1 (b's gradient).
template <typename T, int VEC>
struct Scale2GradRow {
  typedef typename VecT<T>::v16 V16;
  const T* dy;
  const T* x;
  T* dx;
  float a[VEC], b[VEC];  // the scales as chscale_bwd_dx_kernel takes them (+ 0.f: mode 0)
  RT_DEV void row(long o, float* acc_a, float* acc_b) const {
    const V16 g = *(const V16*)(dy + o), xv = *(const V16*)(x + o);
    V16 d;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float gf = to_f(g[j]), xf = to_f(xv[j]);
      const float y1 = to_f(from_f<T>(xf * a[j]));
      const float g1 = to_f(from_f<T>(gf * (b[j] + 0.f)));
      d[j] = from_f<T>(g1 * (a[j] + 0.f));
      acc_a[j] = fmaf(g1, xf, acc_a[j]);
      acc_b[j] = fmaf(gf, y1, acc_b[j]);
    }
    *(V16*)(dx + o) = d;
  }
};
template <typename T, int VEC>
__global__ void __launch_bounds__(256) chscale2_bwd_part_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ a,
                                                                const T* __restrict__ b, T* __restrict__ dx, float* __restrict__ part_a,
                                                                float* __restrict__ part_b, long hw, int c) {
  typedef typename VecT<T>::v16 V16;
  __shared__ float red[2 * 256 * VEC];
  const long so = (long)blockIdx.y * c + chan_part_channel<VEC>(c);
  const V16 av = *(const V16*)(a + so), bv = *(const V16*)(b + so);
  Scale2GradRow<T, VEC> f{dy, x, dx, {}, {}};
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    f.a[j] = to_f(av[j]);
    f.b[j] = to_f(bv[j]);
  }
  chan_part2_body<T, VEC>(f, part_a, part_b, hw, c, red);
}
// chan_final_kernel (scale 1) of two partial sets in one launch: blockIdx.z picks the set
template <typename T>
__global__ void __launch_bounds__(256) chan_final2_kernel(const float* __restrict__ part0, const float* __restrict__ part1,
                                                          T* __restrict__ out0, T* __restrict__ out1, int S, int c) {
  const int img = blockIdx.y, ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  const float* part = blockIdx.z ? part1 : part0;
  T* out = blockIdx.z ? out1 : out0;
  out[(long)img * c + ch] = from_f<T>(slice_sum(part + (long)img * S * c + ch, S, c) * 1.f);
}
extern "C" int rtsds_chscale_bwd(const void* dy, const void* x, const void* a, void* dx, void* da, int n, long hw, int c, int mode,
                                 int dtype, void* ws, size_t ws_bytes, void* stream) {
  const long total = (long)n * hw * c;
  if (total <= 0) return RTSDS_ERR_SHAPE;
  if (da && ws_bytes < rtsds_gap_workspace(n, hw, c)) return RTSDS_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    constexpr int V = VecT<T>::N;
    if (dx && da && chscale_vec_ok<T>(n, hw, c, {dy, x, a, dx})) {  // one pixel pass for both
      const int S = chan_slices(n, hw);
      hipLaunchKernelGGL((chscale_bwd_part_kernel<T, V>), dim3(S, n, rt_cdiv(c, 256 * V)), dim3(256), 0, st, (const T*)dy,
                         (const T*)x, (const T*)a, (T*)dx, (float*)ws, hw, c, mode);
      hipLaunchKernelGGL(chan_final_kernel<T>, dim3(rt_cdiv(c, 256), n), dim3(256), 0, st, (const float*)ws, (T*)da, S, c, 1.f);
    } else {
      if (dx && chscale_vec_ok<T>(n, hw, c, {dy, a, dx}))
        chscale_vec<T, true>((const T*)dy, (const T*)a, (const T*)nullptr, (T*)dx, n, hw, c, mode, st);
      else if (dx)
        hipLaunchKernelGGL(chscale_bwd_dx_kernel<T>, dim3(ew_blocks(total)), dim3(256), 0, st, (const T*)dy, (const T*)a, (T*)dx, n, hw, c, mode);
      if (da) chan_reduce<T, true>((const T*)dy, (const T*)x, (T*)da, n, hw, c, 1.f, (float*)ws, st);
    }
  });
  RET_LAUNCH();
}
// Backward of rtsds_chscale2_fwd, y = round(round(x * a) * b): the chain's two rtsds_chscale_bwd
// (four pixel passes, two finals) as one pixel pass and one final launch.
extern "C" int rtsds_chscale2_bwd(const void* dy, const void* x, const void* a, const void* b, void* dx, void* da, void* db, int n,
                                  long hw, int c, int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (n <= 0 || hw <= 0 || c <= 0 || !dy || !x || !a || !b || !dx || !da || !db) return RTSDS_ERR_SHAPE;
  const size_t set = (size_t)n * chan_slices(n, hw) * c;  // floats per partial set
  if (ws_bytes < 2 * set * 4 || ((size_t)ws & 15)) return RTSDS_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    constexpr int V = VecT<T>::N;
    if (!chscale_vec_ok<T>(n, hw, c, {dy, x, a, b, dx})) return RTSDS_ERR_UNSUPPORTED;
    const int S = chan_slices(n, hw);
    float* pa = (float*)ws;
    float* pb = pa + set;
    hipLaunchKernelGGL((chscale2_bwd_part_kernel<T, V>), dim3(S, n, rt_cdiv(c, 256 * V)), dim3(256), 0, st, (const T*)dy, (const T*)x,
                       (const T*)a, (const T*)b, (T*)dx, pa, pb, hw, c);
    hipLaunchKernelGGL(chan_final2_kernel<T>, dim3(rt_cdiv(c, 256), n, 2), dim3(256), 0, st, (const float*)pa, (const float*)pb, (T*)da,
                       (T*)db, S, c);
  });
  RET_LAUNCH();
}

// ------------------------------------------------------------------ per-pixel class-vector ops
// Each op is one per-pixel body over row views (class_row.h) and runs in two shells.  Logits are
// addressed by (sn, sc, shw) strides, so NHWC and NCHW tensors both work: a grid-stride loop, one
// thread per pixel straight from global memory at pixel_offset().  NHWC-contiguous logits with
// c <= kStageMaxC take the staged tile loop (STAGE_TILES / tile_in / tile_out, ew_common.h) and the
// body runs on dense LDS rows.
static const int kStageMaxC = 64;
static inline bool stage_ok(long sn, long sc, long shw, long hw, int c) {
  return sc == 1 && shw == c && sn == hw * c && c <= kStageMaxC;
}
// element offset of pixel p's logits
RT_DEV long pixel_offset(long p, long hw, long sn, long shw) {
  const long img = p / hw, s = p - img * hw;
  return img * sn + s * shw;
}

// ------------------------------------------------------------------ channel softmax (dim=1)
// train.py:225,245,256.  Output NHWC contiguous with row pitch yld (zero-padded channels
// c..yld-1 so a padded discriminator input can be produced directly).
template <typename RI, typename RO>
RT_DEV void px_softmax(RI x, RO y, int c) {
  const float m = row_max(x, c);
  const float iz = 1.f / row_sum_exp(x, c, m);
  for (int k = 0; k < c; ++k) y[k] = from_f<typename RO::elem>(expf(x(k) - m) * iz);
}
// dx = y * (dy - sum_k dy_k y_k); dy/y have row pitch ld (>= c), dx strided like the logits.
template <typename RG, typename RY, typename RO>
RT_DEV void px_softmax_bwd(RG g, RY y, RO dx, int c) {
  float dot = 0.f;
  for (int k = 0; k < c; ++k) dot = fmaf(g(k), y(k), dot);
  for (int k = 0; k < c; ++k) dx[k] = from_f<typename RO::elem>(y(k) * (g(k) - dot));
}
template <typename T>
__global__ void __launch_bounds__(256) softmax_fwd_staged(const T* __restrict__ x, T* __restrict__ y, long total, int c) {
  T* buf = stage_buf<T>();
  STAGE_TILES(p0, total) {
    const int np = tile_in(buf, p0, total, c, x);
    T* r = buf + threadIdx.x * c;
    if ((int)threadIdx.x < np) px_softmax(dense_row(r), dense_row(r), c);
    tile_out(y, buf, p0, np, c);
  }
}
template <typename T>
__global__ void softmax_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int n, long hw, int c, long sn, long sc, long shw, int yld) {
  const long total = (long)n * hw;
  GRID_STRIDE(p, total) {
    T* o = y + p * yld;
    px_softmax(strided_row(x + pixel_offset(p, hw, sn, shw), sc), dense_row(o), c);
    for (int k = c; k < yld; ++k) o[k] = from_f<T>(0.f);
  }
}
template <typename T>
__global__ void __launch_bounds__(256) softmax_bwd_staged(const T* __restrict__ dy, const T* __restrict__ y, T* __restrict__ dx, long total, int c) {
  T* buf = stage_buf<T>();  // [2][kStagePix][c]: dy (dx in place), y
  STAGE_TILES(p0, total) {
    const int np = tile_in(buf, p0, total, c, dy, y);
    T* g = buf + threadIdx.x * c;
    if ((int)threadIdx.x < np) px_softmax_bwd(dense_row(g), dense_row((const T*)g + kStagePix * c), dense_row(g), c);
    tile_out(dx, buf, p0, np, c);
  }
}
template <typename T>
__global__ void softmax_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y, T* __restrict__ dx, int n, long hw, int c, int ld,
                                   long sn, long sc, long shw) {
  const long total = (long)n * hw;
  GRID_STRIDE(p, total)
    px_softmax_bwd(dense_row(dy + p * ld), dense_row(y + p * ld), strided_row(dx + pixel_offset(p, hw, sn, shw), sc), c);
}
extern "C" int rtsds_softmax_fwd(const void* x, long sn, long sc, long shw, void* y, int y_ld, int n, long hw, int c, int dtype,
                                 void* stream) {
  if (n <= 0 || hw <= 0 || c <= 0 || y_ld < c) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, {
    if (y_ld == c && stage_ok(sn, sc, shw, hw, c))
      hipLaunchKernelGGL(softmax_fwd_staged<T>, dim3(ew_blocks((long)n * hw, kStagePix, 4096)), dim3(256), kStagePix * c * sizeof(T),
                         (hipStream_t)stream, (const T*)x, (T*)y, (long)n * hw, c);
    else
      hipLaunchKernelGGL(softmax_fwd_kernel<T>, dim3(ew_blocks((long)n * hw)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, n, hw, c, sn, sc, shw, y_ld);
  });
  RET_LAUNCH();
}
extern "C" int rtsds_softmax_bwd(const void* dy, const void* y, int ld, void* dx, long sn, long sc, long shw, int n, long hw, int c,
                                 int dtype, void* stream) {
  if (n <= 0 || hw <= 0 || c <= 0 || ld < c) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, {
    if (ld == c && stage_ok(sn, sc, shw, hw, c))
      hipLaunchKernelGGL(softmax_bwd_staged<T>, dim3(ew_blocks((long)n * hw, kStagePix, 4096)), dim3(256), 2 * kStagePix * c * sizeof(T),
                         (hipStream_t)stream, (const T*)dy, (const T*)y, (T*)dx, (long)n * hw, c);
    else
      hipLaunchKernelGGL(softmax_bwd_kernel<T>, dim3(ew_blocks((long)n * hw)), dim3(256), 0, (hipStream_t)stream, (const T*)dy, (const T*)y, (T*)dx, n, hw, c, ld, sn, sc, shw);
  });
  RET_LAUNCH();
}

// ------------------------------------------------------------------ cross entropy (ignore_index)
// nn.CrossEntropyLoss(ignore_index=19) (main.py:124-130, train.py:86-92,202-204): mean over
// non-ignored pixels of logsumexp(x) - x[t].  Two passes for the forward (per-block partial
// (sum, count) -> final), one fused pass for the backward.
// ws layout: [0, RB) partial sums, [RB, 2RB) partial counts, [2RB] total count, [2RB + 1] total sum.
// Class weights (nn.CrossEntropyLoss(weight=w), the WT = true instantiations behind
// rtsds_ce_weighted_*): a pixel's loss term, its "count" term (now w[t]: the count slots hold the
// weight sum) and its gradient factor g are each multiplied once by w[t].  A label outside [0, c)
// reads no weight (its loss is NaN already).
static const int kCeRB = 1024;
template <bool WT>
RT_DEV float ce_weight(const float* __restrict__ wgt, long t, int c) {
  if constexpr (WT) return (t >= 0 && t < c) ? wgt[t] : 1.f;
  else return 1.f;
}
// One non-ignored pixel's loss; a target outside [0, c) gives NaN.
template <typename R>
RT_DEV float px_ce_loss(R x, long t, int c) {
  const float m = row_max(x, c), z = row_sum_exp(x, c, m);
  const float xt = (t >= 0 && t < c) ? x(t) : NAN;
  return logf(z) + m - xt;
}
// dx = g * (softmax - onehot), zeros for an ignored pixel.  The two routes round differently and
// both are pinned: the strided one scales the probability (GZ = false), the staged one folds g
// into 1 / z first (GZ = true).
template <bool GZ, typename RI, typename RO>
RT_DEV void px_ce_grad(RI x, RO dx, long t, int c, int ignore, float g) {
  typedef typename RO::elem T;
  if (t == ignore) {
    for (int k = 0; k < c; ++k) dx[k] = from_f<T>(0.f);
    return;
  }
  const float m = row_max(x, c), z = row_sum_exp(x, c, m);
  if (GZ) {
    const float gz = g / z;
    for (int k = 0; k < c; ++k) dx[k] = from_f<T>(gz * expf(x(k) - m) - (k == t ? g : 0.f));
  } else {
    const float iz = 1.f / z;
    for (int k = 0; k < c; ++k) {
      const float pr = expf(x(k) - m) * iz;
      dx[k] = from_f<T>(g * (pr - (k == t ? 1.f : 0.f)));
    }
  }
}
// the block's (sum, count), both wave sums ahead of the exchanges
RT_DEV void ce_block_sums(float& s, float& cnt) {
  __shared__ float red[4];
  s = wave_sum(s);
  cnt = wave_sum(cnt);
  s = waves_sum4(s, red);
  cnt = waves_sum4(cnt, red);
}
RT_DEV void ce_part_store(float s, float cnt, float* __restrict__ part) {
  ce_block_sums(s, cnt);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s;
    part[kCeRB + blockIdx.x] = cnt;
  }
}
template <typename T, bool WT>
__global__ void ce_fwd_part_kernel(const T* __restrict__ x, const int64_t* __restrict__ tgt, float* __restrict__ part, int n, long hw, int c,
                                   long sn, long sc, long shw, int ignore, const float* __restrict__ wgt) {
  const long total = (long)n * hw;
  float ls = 0.f, lc = 0.f;
  GRID_STRIDE(p, total) {
    const long t = tgt[p];
    if (t == ignore) continue;
    const float l = px_ce_loss(strided_row(x + pixel_offset(p, hw, sn, shw), sc), t, c);
    if constexpr (WT) {
      const float w = ce_weight<WT>(wgt, t, c);
      ls += w * l;
      lc += w;
    } else {
      ls += l;
      lc += 1.f;
    }
  }
  ce_part_store(ls, lc, part);
}
template <typename T, bool WT>
__global__ void __launch_bounds__(256) ce_fwd_part_staged(const T* __restrict__ x, const int64_t* __restrict__ tgt, float* __restrict__ part,
                                                          long total, int c, int ignore, const float* __restrict__ wgt) {
  T* buf = stage_buf<T>();
  float ls = 0.f, lc = 0.f;
  STAGE_TILES(p0, total) {
    const int np = tile_in(buf, p0, total, c, x);
    if ((int)threadIdx.x < np) {
      const long t = tgt[p0 + threadIdx.x];
      if (t != ignore) {
        const float l = px_ce_loss(dense_row((const T*)buf + threadIdx.x * c), t, c);
        if constexpr (WT) {
          const float w = ce_weight<WT>(wgt, t, c);
          ls += w * l;
          lc += w;
        } else {
          ls += l;
          lc += 1.f;
        }
      }
    }
  }
  ce_part_store(ls, lc, part);
}
__global__ void ce_fwd_final_kernel(float* __restrict__ part, int nb, float* __restrict__ loss) {
  float S = 0.f, C = 0.f;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) { S += part[i]; C += part[kCeRB + i]; }
  ce_block_sums(S, C);
  if (threadIdx.x == 0) {
    part[2 * kCeRB] = C;
    part[2 * kCeRB + 1] = S;
    loss[0] = S / C;
  }
}
__global__ void ce_finish_kernel(const float* __restrict__ part, float* __restrict__ loss) {
  if (threadIdx.x == 0) loss[0] = part[2 * kCeRB + 1] / part[2 * kCeRB];
}
template <typename T, bool WT>
__global__ void ce_bwd_kernel(const T* __restrict__ x, const int64_t* __restrict__ tgt, const float* __restrict__ gout,
                              const float* __restrict__ count, T* __restrict__ dx, int n, long hw, int c, long sn, long sc, long shw,
                              int ignore, const float* __restrict__ wgt) {
  const float g = gout[0] / count[0];
  const long total = (long)n * hw;
  GRID_STRIDE(p, total) {
    const long off = pixel_offset(p, hw, sn, shw);
    const long t = tgt[p];
    px_ce_grad<false>(strided_row(x + off, sc), strided_row(dx + off, sc), t, c, ignore, WT ? g * ce_weight<WT>(wgt, t, c) : g);
  }
}
template <typename T, bool WT>
__global__ void __launch_bounds__(256) ce_bwd_staged(const T* __restrict__ x, const int64_t* __restrict__ tgt, const float* __restrict__ gout,
                                                     const float* __restrict__ count, T* __restrict__ dx, long total, int c, int ignore,
                                                     const float* __restrict__ wgt) {
  T* buf = stage_buf<T>();
  const float g = gout[0] / count[0];
  STAGE_TILES(p0, total) {
    const int np = tile_in(buf, p0, total, c, x);
    T* r = buf + threadIdx.x * c;
    if ((int)threadIdx.x < np) {
      const long t = tgt[p0 + threadIdx.x];
      px_ce_grad<true>(dense_row(r), dense_row(r), t, c, ignore, WT ? g * ce_weight<WT>(wgt, t, c) : g);
    }
    tile_out(dx, buf, p0, np, c);
  }
}

extern "C" size_t rtsds_ce_workspace(void) { return (2 * kCeRB + 64) * sizeof(float); }
// WT: the class-weighted kernels (wgt[c]); the routes and launch shapes are the same
template <bool WT>
static int ce_fwd_run(const void* x, long sn, long sc, long shw, const int64_t* tgt, const float* wgt, float* loss, int n, long hw, int c,
                      int ignore_index, int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (n <= 0 || hw <= 0 || c <= 0) return RTSDS_ERR_SHAPE;
  if (ws_bytes < rtsds_ce_workspace()) return RTSDS_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nb = std::min<int>(kCeRB, ew_blocks((long)n * hw, kStagePix, kCeRB));
  DISPATCH_T(dtype, {
    if (stage_ok(sn, sc, shw, hw, c))
      hipLaunchKernelGGL((ce_fwd_part_staged<T, WT>), dim3(nb), dim3(256), kStagePix * c * sizeof(T), st, (const T*)x, tgt, (float*)ws,
                         (long)n * hw, c, ignore_index, wgt);
    else
      hipLaunchKernelGGL((ce_fwd_part_kernel<T, WT>), dim3(nb), dim3(256), 0, st, (const T*)x, tgt, (float*)ws, n, hw, c, sn, sc, shw,
                         ignore_index, wgt);
  });
  hipLaunchKernelGGL(ce_fwd_final_kernel, dim3(1), dim3(256), 0, st, (float*)ws, nb, loss);
  RET_LAUNCH();
}
extern "C" int rtsds_ce_fwd(const void* x, long sn, long sc, long shw, const int64_t* tgt, float* loss, int n, long hw, int c,
                            int ignore_index, int dtype, void* ws, size_t ws_bytes, void* stream) {
  return ce_fwd_run<false>(x, sn, sc, shw, tgt, nullptr, loss, n, hw, c, ignore_index, dtype, ws, ws_bytes, stream);
}
extern "C" int rtsds_ce_weighted_fwd(const void* x, long sn, long sc, long shw, const int64_t* tgt, const float* weight, float* loss,
                                     int n, long hw, int c, int ignore_index, int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (!weight || !x || !tgt || c < 1 || c > 32) return RTSDS_ERR_SHAPE;
  if (!ws) return RTSDS_ERR_WORKSPACE;
  return ce_fwd_run<true>(x, sn, sc, shw, tgt, weight, loss, n, hw, c, ignore_index, dtype, ws, ws_bytes, stream);
}
// loss = S / C with C summed by the caller over data-parallel ranks (ws + 2*1024 floats: C, S).
extern "C" int rtsds_ce_finish(const void* ws, float* loss, void* stream) {
  hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)ws, loss);
  RET_LAUNCH();
}
// count = the valid-pixel count written by rtsds_ce_fwd into its workspace (ws + 2*1024 floats).
template <bool WT>
static int ce_bwd_run(const void* x, long sn, long sc, long shw, const int64_t* tgt, const float* wgt, const float* grad_loss,
                      const float* count, void* dx, int n, long hw, int c, int ignore_index, int dtype, void* stream) {
  if (n <= 0 || hw <= 0 || c <= 0) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, {
    if (stage_ok(sn, sc, shw, hw, c))
      hipLaunchKernelGGL((ce_bwd_staged<T, WT>), dim3(ew_blocks((long)n * hw, kStagePix, 4096)), dim3(256), kStagePix * c * sizeof(T),
                         (hipStream_t)stream, (const T*)x, tgt, grad_loss, count, (T*)dx, (long)n * hw, c, ignore_index, wgt);
    else
      hipLaunchKernelGGL((ce_bwd_kernel<T, WT>), dim3(ew_blocks((long)n * hw)), dim3(256), 0, (hipStream_t)stream, (const T*)x, tgt,
                         grad_loss, count, (T*)dx, n, hw, c, sn, sc, shw, ignore_index, wgt);
  });
  RET_LAUNCH();
}
extern "C" int rtsds_ce_bwd(const void* x, long sn, long sc, long shw, const int64_t* tgt, const float* grad_loss, const float* count,
                            void* dx, int n, long hw, int c, int ignore_index, int dtype, void* stream) {
  return ce_bwd_run<false>(x, sn, sc, shw, tgt, nullptr, grad_loss, count, dx, n, hw, c, ignore_index, dtype, stream);
}
// count = the weight sum the weighted forward left at ws + 2*1024 floats
extern "C" int rtsds_ce_weighted_bwd(const void* x, long sn, long sc, long shw, const int64_t* tgt, const float* weight,
                                     const float* grad_loss, const float* count, void* dx, int n, long hw, int c, int ignore_index,
                                     int dtype, void* stream) {
  if (!weight || !x || !tgt || !grad_loss || !count || !dx || c < 1 || c > 32) return RTSDS_ERR_SHAPE;
  return ce_bwd_run<true>(x, sn, sc, shw, tgt, weight, grad_loss, count, dx, n, hw, c, ignore_index, dtype, stream);
}

// ------------------------------------------------------------------ BCE with logits
// nn.BCEWithLogitsLoss() (main.py:131-132, train.py:229,247,258): mean of
// max(x,0) - x*t + log1p(exp(-|x|)).  Tiny (one logit per image): one block.
__global__ void bce_fwd_kernel(const float* __restrict__ x, const float* __restrict__ t, float* __restrict__ loss, int n) {
  __shared__ float r[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float v = x[i];
    s += fmaxf(v, 0.f) - v * t[i] + log1pf(expf(-fabsf(v)));
  }
  s = block_sum4(s, r);
  if (threadIdx.x == 0) loss[0] = s / (float)n;
}
__global__ void bce_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ gout, float* __restrict__ dx, int n) {
  const float g = gout[0] / (float)n;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float s = 1.f / (1.f + expf(-x[i]));
    dx[i] = g * (s - t[i]);
  }
}
extern "C" int rtsds_bce_fwd(const float* x, const float* target, float* loss, int n, void* stream) {
  if (n <= 0) return RTSDS_ERR_SHAPE;
  hipLaunchKernelGGL(bce_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, target, loss, n);
  RET_LAUNCH();
}
extern "C" int rtsds_bce_bwd(const float* x, const float* target, const float* grad_loss, float* dx, int n, void* stream) {
  if (n <= 0) return RTSDS_ERR_SHAPE;
  hipLaunchKernelGGL(bce_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, target, grad_loss, dx, n);
  RET_LAUNCH();
}

// ------------------------------------------------------------------ argmax / pixel accuracy
// argmax over channels, first maximum wins (torch.argmax / max(1), train.py:102-106,272-275,
// validation.py:51).  out_idx may be NULL; correct += #(argmax == target) (ignored pixels
// count as wrong, exactly like the reference).
template <typename R>
RT_DEV void px_argmax(R x, long p, int c, int64_t* __restrict__ out, const int64_t* __restrict__ tgt, unsigned long long& cnt) {
  float best;
  const int bi = first_max(x, c, best);
  if (out) out[p] = bi;
  if (tgt && tgt[p] == bi) ++cnt;
}
RT_DEV void argmax_count(unsigned long long* correct, unsigned long long cnt) {
  if (correct) {
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(correct, cnt);
  }
}
template <typename T>
__global__ void argmax_kernel(const T* __restrict__ x, int64_t* __restrict__ out, const int64_t* __restrict__ tgt,
                              unsigned long long* __restrict__ correct, int n, long hw, int c, long sn, long sc, long shw) {
  const long total = (long)n * hw;
  unsigned long long cnt = 0;
  GRID_STRIDE(p, total) px_argmax(strided_row(x + pixel_offset(p, hw, sn, shw), sc), p, c, out, tgt, cnt);
  argmax_count(correct, cnt);
}
template <typename T>
__global__ void __launch_bounds__(256) argmax_staged(const T* __restrict__ x, int64_t* __restrict__ out, const int64_t* __restrict__ tgt,
                                                     unsigned long long* __restrict__ correct, long total, int c) {
  T* buf = stage_buf<T>();
  unsigned long long cnt = 0;
  STAGE_TILES(p0, total) {
    const int np = tile_in(buf, p0, total, c, x);
    if ((int)threadIdx.x < np) px_argmax(dense_row((const T*)buf + threadIdx.x * c), p0 + threadIdx.x, c, out, tgt, cnt);
  }
  argmax_count(correct, cnt);
}

extern "C" int rtsds_argmax(const void* x, long sn, long sc, long shw, int64_t* out, const int64_t* target, unsigned long long* correct,
                            int n, long hw, int c, int dtype, void* stream) {
  if (n <= 0 || hw <= 0 || c <= 0) return RTSDS_ERR_SHAPE;
  DISPATCH_T(dtype, {
    if (stage_ok(sn, sc, shw, hw, c))
      hipLaunchKernelGGL(argmax_staged<T>, dim3(ew_blocks((long)n * hw, kStagePix, 4096)), dim3(256), kStagePix * c * sizeof(T),
                         (hipStream_t)stream, (const T*)x, out, target, correct, (long)n * hw, c);
    else
      hipLaunchKernelGGL(argmax_kernel<T>, dim3(ew_blocks((long)n * hw, 256, 4096)), dim3(256), 0, (hipStream_t)stream, (const T*)x, out, target, correct, n, hw, c, sn, sc, shw);
  });
  RET_LAUNCH();
}

// 19x19 confusion histogram (utils.fast_hist, utils.py:52-58): labels outside [0, nc) dropped.
__global__ void confusion_kernel(const int64_t* __restrict__ label, const int64_t* __restrict__ pred, unsigned long long* __restrict__ hist,
                                 long total, int nc) {
  extern __shared__ unsigned int lh[];
  for (int i = threadIdx.x; i < nc * nc; i += blockDim.x) lh[i] = 0;
  __syncthreads();
  GRID_STRIDE(p, total) {
    const long a = label[p];
    if (a >= 0 && a < nc) atomicAdd(&lh[a * nc + pred[p]], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nc * nc; i += blockDim.x)
    if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
}
extern "C" int rtsds_confusion(const int64_t* label, const int64_t* pred, unsigned long long* hist, long total, int nc, void* stream) {
  if (total <= 0 || nc <= 0 || nc > 64) return RTSDS_ERR_SHAPE;
  hipLaunchKernelGGL(confusion_kernel, dim3(ew_blocks(total, 256, 1024)), dim3(256), nc * nc * 4, (hipStream_t)stream, label, pred, hist, total, nc);
  RET_LAUNCH();
}
