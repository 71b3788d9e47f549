// BatchNorm device expressions shared by the BatchNorm unit (bn.hip) and the kernels that apply a
// BatchNorm backward on the fly (imgconv.hip's fused weight gradient): 16-B row vectors, the
// activation mask and dx = a*g + b*(x - mu) + k.  One definition, so every user produces the
// same bits.
#pragma once
#include "common.h"

// VEC is either the 16-B vector width (dispatched only when c % VEC == 0, so an active thread's
// channel vector is always complete) or 1.
template <typename T, int VEC>
RT_DEV void load_vec(const T* p, float* v, int cvalid) {
  static_assert(VEC == 1 || VEC == VecT<T>::N, "VEC");
  if constexpr (VEC == VecT<T>::N) {
    typename VecT<T>::v16 t = *(const typename VecT<T>::v16*)p;
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = to_f(t[j]);
  } else {
    v[0] = cvalid > 0 ? to_f(p[0]) : 0.f;
  }
}
template <typename T, int VEC>
RT_DEV void store_vec(T* p, const float* v, int cvalid) {
  if constexpr (VEC == VecT<T>::N) {
    typename VecT<T>::v16 t;
#pragma unroll
    for (int j = 0; j < VEC; ++j) t[j] = from_f<T>(v[j]);
    *(typename VecT<T>::v16*)p = t;
  } else {
    if (cvalid > 0) p[0] = from_f<T>(v[0]);
  }
}

RT_DEV float act_grad(float y, int act) {
  if (act == RTSDS_ACT_RELU) return y > 0.f ? 1.f : 0.f;
  if (act == RTSDS_ACT_LEAKY) return y > 0.f ? 1.f : 0.2f;
  if (act == RTSDS_ACT_SIGMOID) return y * (1.f - y);
  return 1.f;
}

// g *= act'(.): the activation derivative from the saved output's values yv (HAS_Y), or -- when y
// is not kept (no residual, monotone activation with act'(v) determined by sign(v)) -- from the
// sign of the recomputed pre-activation x*scale+shift, which is bit-identical to the forward's.
// The one mask of the statistics loop and the apply passes.
template <int VEC, bool HAS_Y>
RT_DEV void bn_mask(float* g, const float* yv, const float* xv, const float* sc, const float* sh, int act) {
  if (!act) return;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    if constexpr (HAS_Y) g[j] *= act_grad(yv[j], act);
    else g[j] = fmaf(xv[j], sc[j], sh[j]) > 0.f ? g[j] : (act == RTSDS_ACT_LEAKY ? 0.2f * g[j] : 0.f);
  }
}

// The ReLU mask of a residual BatchNorm kept as bits: one byte per channel vector, bit j =
// y[ch0 + j] > 0 of the value as stored (rounded to T; +0, -0 and NaN give 0, as act_grad does
// from y).  bn_bits_y turns a byte back into stand-ins for y (1 or 0) that bn_mask<VEC, true> maps
// to the same factors 1 / 0 as the stored y.
template <typename T, int VEC>
RT_DEV unsigned bn_y_bits(const float* v) {
  static_assert(VEC <= 8, "one byte per channel vector");
  unsigned b = 0;
#pragma unroll
  for (int j = 0; j < VEC; ++j) b |= (to_f(from_f<T>(v[j])) > 0.f ? 1u : 0u) << j;
  return b;
}
template <int VEC>
RT_DEV void bn_bits_y(unsigned b, float* yv) {
#pragma unroll
  for (int j = 0; j < VEC; ++j) yv[j] = (b >> j) & 1u ? 1.f : 0.f;
}

// A thread's per-channel backward coefficients: dx = a*g + b*(x - mu) + k, and the forward's
// sc / sh for the mask recomputed from x.
template <int VEC> struct BnDx {
  float a[VEC], b[VEC], k[VEC], mu[VEC], sc[VEC], sh[VEC];
};

// The backward apply's row pieces: dx = a*g + b*(x - mu) + k, dres = g.
// The mask of one row; y: the row of the stored output (null: recomputed from x).
template <typename T, int VEC>
RT_DEV void bn_row_mask(float* g, const T* __restrict__ y, const float* xv, const BnDx<VEC>& k, int act, int cvalid) {
  if (!act) return;
  if (y) {
    float yv[VEC];
    load_vec<T, VEC>(y, yv, cvalid);
    bn_mask<VEC, true>(g, yv, xv, k.sc, k.sh, act);
  } else {
    bn_mask<VEC, false>(g, nullptr, xv, k.sc, k.sh, act);
  }
}
template <int VEC>
RT_DEV float bn_bwd_dx(const BnDx<VEC>& k, int j, float g, float x) { return fmaf(k.a[j], g, fmaf(k.b[j], x - k.mu[j], k.k[j])); }
