// The rules every kernel that reads a per-pixel class vector shares (chan.hip, pseudo.hip,
// resize.hip, classmix.hip): the row view, the NaN-aware first maximum, row maximum / sum of
// exponentials, the confidence bin and the thresholded pseudo-label.  Each exists once, here.
#pragma once
#include "common.h"

// A pixel's class vector: element k at p[k * s].  S = 1 is a dense row with the stride known at
// compile time (the LDS-staged kernels'), S = 0 takes the stride s of an NCHW / sliced tensor.
// Called with k, a row gives the value as fp32, so it stands wherever a callable k -> value does.
template <typename T, int S>
struct ClassRow {
  typedef T elem;
  T* p;
  long s;
  RT_DEV T& operator[](long k) const { return p[S ? k : k * s]; }
  RT_DEV float operator()(long k) const { return to_f((*this)[k]); }
};
template <typename T> RT_DEV ClassRow<T, 1> dense_row(T* p) { return {p, 1}; }
template <typename T> RT_DEV ClassRow<T, 0> strided_row(T* p, long s) { return {p, s}; }

// One step of the first-maximum scan, torch.argmax's rule: a later value takes over only if it is
// greater, or a NaN while the best so far is a number (a NaN beats every number, the first NaN wins).
RT_DEV void first_max_take(float v, int k, float& best, int& bi) {
  if (v > best || (v != v && best == best)) {
    best = v;
    bi = k;
  }
}
// First maximum of val(0 .. c - 1), c >= 1: returns the index, best = the value.  MAXC > 0: fully
// unrolled to MAXC steps guarded by k < c (val may index registers).
template <int MAXC = 0, typename F>
RT_DEV int first_max(F val, int c, float& best) {
  best = val(0);
  int bi = 0;
  if constexpr (MAXC > 0) {
#pragma unroll
    for (int k = 1; k < MAXC; ++k)
      if (k < c) first_max_take(val(k), k, best, bi);
  } else {
    for (int k = 1; k < c; ++k) first_max_take(val(k), k, best, bi);
  }
  return bi;
}

template <typename R>
RT_DEV float row_max(R x, int c) {
  float m = -INFINITY;
  for (int k = 0; k < c; ++k) m = fmaxf(m, x(k));
  return m;
}
template <typename R>
RT_DEV float row_sum_exp(R x, int c, float m) {
  float z = 0.f;
  for (int k = 0; k < c; ++k) z += expf(x(k) - m);
  return z;
}

// Confidence -> histogram bin: floor(conf * bins) clamped to bins - 1; a conf that is not > 0
// (NaN included) goes to bin 0.  bins is a power of two, so conf * bins is exact.
RT_DEV int conf_bin(float conf, int bins) {
  const float fb = (float)bins;
  int b = 0;
  if (conf > 0.f) {
    const float t = floorf(conf * fb);
    b = t >= fb ? bins - 1 : (int)t;
  }
  return b;
}

// Class-balanced pseudo-label: class k if its confidence bin b reaches the class threshold tb[k],
// else ignore; a class outside [0, c) is ignored too (GUARD = false where k < c by construction).
template <bool GUARD = true>
RT_DEV int pseudo_label(int k, int b, const int* tb, int c, int ignore) {
  return ((!GUARD || k < c) && b >= tb[k]) ? k : ignore;
}
