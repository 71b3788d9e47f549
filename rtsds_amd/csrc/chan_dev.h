// Per-image channel reduction shared by the channel-vector unit (chan.hip) and the kernels that
// form the same sums on the fly (bn.hip's BatchNorm apply + pool partials, conv_pooled.hip's
// attention backward): the slice partition, the stage-1 loop and the stage-2 slice sum.  One
// definition, so every user produces the same bits.
#pragma once
#include "common.h"
#include <algorithm>

// Row slices per image of the stage-1 pass
static inline int chan_slices(int n, long hw) {
  return (int)std::max<long>(1, std::min<long>(hw / 32, std::max(1, 1024 / std::max(1, n))));
}

// Where stage 1 reads its first operand: at(o) the element at offset o as a float (VEC == 1),
// vec(o) the 16-B vector starting there.
template <typename T>
struct ChanLoad {
  const T* a;
  RT_DEV float at(long o) const { return to_f(a[o]); }
  RT_DEV typename VecT<T>::v16 vec(long o) const { return *(const typename VecT<T>::v16*)(a + o); }
};

// Stage 1 of out[img][c] = scale * sum_hw a (* b if DOT): grid (S row slices, img, channel chunk)
// of 256-thread blocks laid out [row group][16-B channel vector] (VEC = 8 bf16 / 4 f32 when c
// allows, else 1) -> part[img][s][c] fp32.  red: 256 * VEC floats of LDS.
template <typename T, int VEC, bool DOT, class A>
RT_DEV void chan_part_body(const A& a, const T* __restrict__ b, float* __restrict__ part, long hw, int c, float* red) {
  const int s = blockIdx.x, S = gridDim.x, img = blockIdx.y;
  const int cbase = blockIdx.z * 256 * VEC;
  const int cl = min(c - cbase, 256 * VEC);
  const int tpr = (cl + VEC - 1) / VEC, rpi = 256 / tpr;
  const int tid = threadIdx.x, cv = tid % tpr, rg = tid / tpr;
  const int ch0 = cbase + cv * VEC;
  const long per = (hw + S - 1) / S, r0 = s * per, r1 = min(hw, r0 + per);
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  if (rg < rpi) {
    const long base = (long)img * hw * c + ch0;
    long r = r0 + rg;
    for (; r + rpi < r1; r += 2 * rpi) {  // two rows in flight
      const long o0 = base + r * c, o1 = o0 + (long)rpi * c;
      if constexpr (VEC > 1) {
        typedef typename VecT<T>::v16 V16;
        const V16 a0 = a.vec(o0), a1 = a.vec(o1);
        if (DOT) {
          const V16 b0 = *(const V16*)(b + o0), b1 = *(const V16*)(b + o1);
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc[j] = fmaf(to_f(a1[j]), to_f(b1[j]), fmaf(to_f(a0[j]), to_f(b0[j]), acc[j]));
        } else {
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc[j] += to_f(a0[j]) + to_f(a1[j]);
        }
      } else {
        const float a0 = a.at(o0), a1 = a.at(o1);
        acc[0] = DOT ? fmaf(a1, to_f(b[o1]), fmaf(a0, to_f(b[o0]), acc[0])) : acc[0] + (a0 + a1);
      }
    }
    for (; r < r1; r += rpi) {
      const long o = base + r * c;
      if constexpr (VEC > 1) {
        typedef typename VecT<T>::v16 V16;
        const V16 va = a.vec(o);
        if (DOT) {
          const V16 vb = *(const V16*)(b + o);
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc[j] = fmaf(to_f(va[j]), to_f(vb[j]), acc[j]);
        } else {
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc[j] += to_f(va[j]);
        }
      } else {
        const float a0 = a.at(o);
        acc[0] = DOT ? fmaf(a0, to_f(b[o]), acc[0]) : acc[0] + a0;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) red[tid * VEC + j] = acc[j];
  __syncthreads();
  if (rg == 0 && cv * VEC < cl) {
    for (int g = 1; g < rpi; ++g)
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[j] += red[(g * tpr + cv) * VEC + j];
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      if (ch0 + j < c) part[((long)img * S + s) * c + ch0 + j] = acc[j];
  }
}
template <typename T, int VEC, bool DOT>
__global__ void __launch_bounds__(256) chan_part_kernel(const T* __restrict__ a, const T* __restrict__ b, float* __restrict__ part,
                                                        long hw, int c) {
  __shared__ float red[256 * VEC];
  chan_part_body<T, VEC, DOT>(ChanLoad<T>{a}, b, part, hw, c, red);
}
// First channel of the calling thread's vector in chan_part_body's layout (c % VEC == 0: inside c
// for every thread), for operand functors that carry per-channel values.
template <int VEC>
RT_DEV int chan_part_channel(int c) {
  const int cbase = blockIdx.z * 256 * VEC;
  const int tpr = (min(c - cbase, 256 * VEC) + VEC - 1) / VEC;
  return cbase + (threadIdx.x % tpr) * VEC;
}
// Two DOT reductions in one pass over the pixels: part0 / part1 exactly as two
// chan_part_body<T, VEC, true> passes leave them -- the same partition, and per set the same fma
// chain (a thread's rows in order; the two-rows-in-flight form above is that chain too) and the
// same row-group sum.  f.row(o, acc0, acc1) adds the VEC products at element offset o to each
// set's accumulators with one fmaf per channel.  c % VEC == 0; red: 2 * 256 * VEC floats of LDS.
template <typename T, int VEC, class F>
RT_DEV void chan_part2_body(const F& f, float* __restrict__ part0, float* __restrict__ part1, long hw, int c, float* red) {
  const int s = blockIdx.x, S = gridDim.x, img = blockIdx.y;
  const int cbase = blockIdx.z * 256 * VEC;
  const int cl = min(c - cbase, 256 * VEC);
  const int tpr = (cl + VEC - 1) / VEC, rpi = 256 / tpr;
  const int tid = threadIdx.x, cv = tid % tpr, rg = tid / tpr;
  const int ch0 = cbase + cv * VEC;
  const long per = (hw + S - 1) / S, r0 = s * per, r1 = min(hw, r0 + per);
  float acc0[VEC], acc1[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc0[j] = acc1[j] = 0.f;
  if (rg < rpi) {
    const long base = (long)img * hw * c + ch0;
#pragma unroll 2
    for (long r = r0 + rg; r < r1; r += rpi) f.row(base + r * c, acc0, acc1);
  }
  float* red1 = red + 256 * VEC;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    red[tid * VEC + j] = acc0[j];
    red1[tid * VEC + j] = acc1[j];
  }
  __syncthreads();
  if (rg == 0 && cv * VEC < cl) {
    for (int g = 1; g < rpi; ++g)
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        acc0[j] += red[(g * tpr + cv) * VEC + j];
        acc1[j] += red1[(g * tpr + cv) * VEC + j];
      }
    const long o = ((long)img * S + s) * c + ch0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      part0[o + j] = acc0[j];
      part1[o + j] = acc1[j];
    }
  }
}
// p[0], p[c], .. p[(S - 1) c] summed in slice order, U loads in flight (the adds stay one chain
// in slice order, so U changes no bit)
template <int U = 8>
RT_DEV float slice_sum(const float* __restrict__ p, int S, int c) {
  float s = 0.f;
  int q = 0;
  for (; q + U <= S; q += U) {
    float t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) t[u] = p[(long)(q + u) * c];
#pragma unroll
    for (int u = 0; u < U; ++u) s += t[u];
  }
  for (; q < S; ++q) s += p[(long)q * c];
  return s;
}
