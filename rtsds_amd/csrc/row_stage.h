// What the per-pixel loss units on low-resolution class maps share (distill.hip, entropy.hip): the
// 16-B staging of runs of class rows that start anywhere, the softened row, the fixed-order fp64
// sum of a launch's partials and the scaled store of a gradient.  Each exists once, here.
#pragma once
#include "ew_common.h"

// ------------------------------------------------------------------ 16-B staging of unaligned runs
// A run of class rows (19 classes: 38 or 76 bytes per pixel) starts anywhere.  Its LDS image keeps
// the run's offset inside a 16-B chunk (lead, in elements), so every whole chunk of the run moves
// as one lane-consecutive 16-B access and only the elements before the first and after the last
// whole chunk move singly.  s is 16-B aligned and holds lead + nel elements.
template <typename T>
RT_DEV int rs_lead(const T* g) {
  return (int)(((uintptr_t)g & 15) / sizeof(T));
}
template <typename T, bool IN>
RT_DEV void rs_move(T* __restrict__ g, T* s, int nel) {
  constexpr int N = 16 / (int)sizeof(T);
  const int lead = rs_lead(g);
  const int head = min(nel, (N - lead) & (N - 1));
  const int nv = (nel - head) / N, done = head + nv * N;
  uint4* gv = (uint4*)(g + head);
  uint4* sv = (uint4*)(s + lead + head);
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    if constexpr (IN) sv[i] = gv[i];
    else gv[i] = sv[i];
  }
  for (int i = threadIdx.x; i < head + nel - done; i += blockDim.x) {
    const int j = i < head ? i : done + (i - head);
    if constexpr (IN) s[lead + j] = g[j];
    else g[j] = s[lead + j];
  }
}
template <typename T>
RT_DEV void rs_in(const T* g, T* s, int nel) {
  rs_move<T, true>(const_cast<T*>(g), s, nel);
}
template <typename T>
RT_DEV void rs_out(T* g, T* s, int nel) {
  rs_move<T, false>(g, s, nel);
}
__host__ __device__ static inline size_t rs_lds_row(size_t nel, size_t elem) { return ((nel + 16 / elem) * elem + 15) & ~(size_t)15; }

// ------------------------------------------------------------------ the softened row
// v = logits * inv_temp in place, then d = v - max(v) in v, e = exp(d), z = sum e (class order),
// lz = log z: probability k is e[k] / z, its logarithm v[k] - lz.  Every row of either unit goes
// through this one function, and the products and differences are kept from fusing with their
// neighbours, so equal rows give equal bits.  inv_temp = 1 is the plain softmax.
template <int MAXC>
RT_DEV void rs_soften(float (&v)[MAXC], float (&e)[MAXC], int c, float inv_temp, float& z, float& lz) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < MAXC; ++k)
    if (k < c) {
      v[k] = __fmul_rn(v[k], inv_temp);
      m = fmaxf(m, v[k]);
    }
  z = 0.f;
#pragma unroll
  for (int k = 0; k < MAXC; ++k)
    if (k < c) {
      v[k] = __fsub_rn(v[k], m);
      e[k] = expf(v[k]);
      z = __fadd_rn(z, e[k]);
    }
  lz = logf(z);
}

// ------------------------------------------------------------------ partials -> scalars
// out[j] = coef * (sum over i of part[i * NOUT + j]), j < NOUT: each thread adds every 256th
// partial, the 256 sums meet in a fixed tree, all in fp64 -- the same bits on every run.
template <int NOUT>
struct RsOuts {
  float* p[NOUT];
};
template <int NOUT>
__global__ void __launch_bounds__(256) rs_finish_kernel(const float* __restrict__ part, int nparts, double coef, RsOuts<NOUT> out) {
  __shared__ double red[NOUT][256];
  double acc[NOUT];
#pragma unroll
  for (int j = 0; j < NOUT; ++j) acc[j] = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) {
#pragma unroll
    for (int j = 0; j < NOUT; ++j) acc[j] += (double)part[(long)i * NOUT + j];
  }
#pragma unroll
  for (int j = 0; j < NOUT; ++j) red[j][threadIdx.x] = acc[j];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int j = 0; j < NOUT; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < NOUT; ++j) *out.p[j] = (float)(coef * red[j][0]);
  }
}

// ------------------------------------------------------------------ the gradient's scaled store
// dx = cast(scale * term), scale = fp32(g * coef_g), term the fp32 per-element gradient the forward
// left.  A thread owns one 16-B chunk of dx (chunks counted from dx's own 16-B boundaries); a chunk
// cut by either end of the tensor is stored singly.
template <typename T>
__global__ void __launch_bounds__(256) rs_bwd_kernel(const float* __restrict__ term, const float* __restrict__ g, double coef_g,
                                                     T* __restrict__ dx, long total) {
  constexpr int N = VecT<T>::N;
  const int lead = rs_lead(dx);
  const float scale = (float)((double)*g * coef_g);
  const long chunks = (total + lead + N - 1) / N;
  GRID_STRIDE(j, chunks) {
    const long e0 = j * N - lead;
    if (e0 >= 0 && e0 + N <= total) {
      typename VecT<T>::v16 v;
#pragma unroll
      for (int i = 0; i < N; ++i) v[i] = from_f<T>(scale * term[e0 + i]);
      *(typename VecT<T>::v16*)(dx + e0) = v;
    } else {
      for (int i = 0; i < N; ++i)
        if (e0 + i >= 0 && e0 + i < total) dx[e0 + i] = from_f<T>(scale * term[e0 + i]);
    }
  }
}
