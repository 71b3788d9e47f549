// Bilinear resize (align_corners=False), forward and backward, and the kernels fused onto it
// (gfx950): resize + softmax for the discriminator input, multi-scale / flip evaluation, the
// online teacher's pseudo-labels, the painted frames of prediction.
// Every output bit of the unit is pinned (tests/test_resize_bits_gpu.py), and each piece that
// carries a bit-exactness promise exists once:
//   bil_src / bil_mix / bil_first_ge (common.h)   taps, weights, the blend's association
//   bil_stage_rows, BilWalk                       forward: source rows -> fp32 LDS; a dense output vector's elements
//   bil_row_group, bil_group_store                forward: the output rows sharing a top tap, written from t0 / t1
//   bil_adj_range, bil_weight, bil_gather         backward: which outputs an input reads, their weights, the sum's order
//   bil_table_build, bil_table_span, BilTables    backward: the weight tables in LDS
//   bil_bwd_h_launch                              the vertical pass (bilinear and resize + softmax backward)
//   upsm_tile, upsm_probs                         resize + softmax: one tile's staging, one pixel's probabilities
//   upsm_logit                                    one class of one pixel's resized logits, for on-the-fly reductions
#include "ew_common.h"
#include "class_row.h"

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

// Row groups (upsampling): every output row whose top tap is source row h0 blends the same two
// horizontal blends t0 / t1 (bil_mix's inner terms), so a thread forms them once and writes all
// of the group's rows (~ the scale factor of them) as bil_mix's outer fmaf -- bil_mix bit for bit.
// bil_row_group: the group's output rows [oa, ob) (empty when downsampling skips h0) and bottom tap h1
RT_DEV bool bil_row_group(int h0, float sh, int hi, int ho, int& oa, int& ob, int& h1) {
  oa = bil_first_ge(h0, sh, hi, ho);
  ob = bil_first_ge(h0 + 1, sh, hi, ho);
  h1 = h0 + (h0 < hi - 1 ? 1 : 0);
  return oa < ob;
}
// one 16-B vector of output row oh from its column's t0 / t1
template <typename T>
RT_DEV void bil_group_store(T* dst, const float (&t0)[VecT<T>::N], const float (&t1)[VecT<T>::N], int oh, float sh, int hi) {
  constexpr int V = VecT<T>::N;
  int i0, i1;
  float lh0, lh1;
  bil_src(oh, sh, hi, i0, i1, lh0, lh1);
  typename VecT<T>::v16 r;
#pragma unroll
  for (int k = 0; k < V; ++k) r[k] = from_f<T>(fmaf(lh1, t1[k], lh0 * t0[k]));
  *(typename VecT<T>::v16*)dst = r;
}

// Upsampling with 16-B channel vectors (the context-path resizes into the FFM concat): one thread
// per (image, source row h0, output column, channel vector) loads the 4 taps once, forms the
// two horizontal blends and writes the row group of h0 (bit-identical to MODE 0;
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
  int oa, ob, h1;
  if (!bil_row_group(h0, sh, hi, ho, oa, ob, h1)) return;
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
    for (int oh = oa; oh < ob; ++oh)
      bil_group_store(y + (((long)img * ho + oh) * wo + ow) * yld + yoff + chunk * V, t0, t1, oh, sh, hi);
  }
}

// Narrow channel counts that are not a 16-B multiple (the 19-class logits of the eval forward's
// final x8 resize, build_bisenet.py:165-166): one workgroup per output row.  The row's two source
// rows are staged in LDS as fp32 (coalesced), then every thread writes whole 16-B vectors of the
// dense output row (a wave writes 1 KB contiguously; the whole-pixel loop wrote 38-B runs at a
// 38-B lane stride, 1.8 TB/s) from 4 LDS taps per element.  Same taps, weights and bil_mix
// expression as the other modes.
// bil_stage_rows: two source rows (or a column window of them), n1 elements each -> fp32 LDS
// [2][n1], coalesced; the caller places the barrier
template <typename T>
RT_DEV void bil_stage_rows(const T* __restrict__ r0, const T* __restrict__ r1, float* rows, int n1) {
  for (int e = threadIdx.x; e < n1; e += 256) {
    rows[e] = to_f(r0[e]);
    rows[n1 + e] = to_f(r1[e]);
  }
}
// BilWalk: a dense [wo][c] output row walked element by element from flat element e, across pixel
// boundaries: taps() gives the element's w0 / w1 taps in the staged top row (bottom row: + wi * c),
// leaves their weights in lw0 / lw1 and steps to the next element.  (A stepper, not a helper that
// fills t0 / t1 or calls back per element: either form cost bilinear_fwd_rowgroup_kernel 22 - 48
// more register moves and 5 more waits, 62.97 -> 63.75 us at the fp32 x8 19-class shape.)
struct BilWalk {
  int ow, ch, w0, w1;
  float lw0, lw1;
  RT_DEV BilWalk(int e, int c, int wi, float sw, const FastDiv& f_c) {
    ow = (int)fdiv((uint32_t)e, f_c);
    ch = e - ow * c;
    bil_src(ow, sw, wi, w0, w1, lw0, lw1);
  }
  RT_DEV void taps(const float* rows, int c, int wi, float sw, const float*& a, const float*& b) {
    if (ch == c) {
      ch = 0;
      ++ow;
      bil_src(ow, sw, wi, w0, w1, lw0, lw1);
    }
    a = rows + w0 * c + ch;
    b = rows + w1 * c + ch;
    ++ch;
  }
};
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
  bil_stage_rows(x + ((long)img * hi + h0) * rl, x + ((long)img * hi + h1) * rl, rows, rl);
  __syncthreads();
  const int nv = wo * c / V;  // (wo * c) % V == 0 (host)
  T* yo = y + (long)row * wo * c;
  for (int v = threadIdx.x; v < nv; v += 256) {
    BilWalk w(v * V, c, wi, sw, f_c);
    V16 r;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float *a, *b;
      w.taps(rows, c, wi, sw, a, b);
      r[k] = from_f<T>(bil_mix(a[0], b[0], a[rl], b[rl], lh0, lh1, w.lw0, w.lw1));
    }
    *(V16*)(yo + v * V) = r;
  }
}

// The same resize for upsampling, one workgroup per (image, source row h0, column chunk): each
// thread computes t0 / t1 once for its J output vectors of the chunk, keeps them in registers and
// writes the row group of h0 -- 2 VALU ops per element instead of ~12 and 4 LDS reads per
// element per group instead of per row.
template <typename T, int J>
__global__ void __launch_bounds__(256) bilinear_fwd_rowgroup_kernel(const T* __restrict__ x, T* __restrict__ y, int hi, int wi, int c,
                                                                     int ho, int wo, float sh, float sw, int nchunk, FastDiv f_c) {
  constexpr int V = VecT<T>::N;
  extern __shared__ float rows[];  // [2][wi * c]
  const int grp = blockIdx.x / nchunk, chunk = blockIdx.x - grp * nchunk;
  const int img = grp / hi, h0 = grp - img * hi;
  int oa, ob, h1;
  if (!bil_row_group(h0, sh, hi, ho, oa, ob, h1)) return;  // whole workgroup
  const int rl = wi * c;
  bil_stage_rows(x + ((long)img * hi + h0) * rl, x + ((long)img * hi + h1) * rl, rows, rl);
  __syncthreads();
  const int nv = wo * c / V;  // (wo * c) % V == 0 (host)
  const int v0 = (int)((long)nv * chunk / nchunk), v1 = (int)((long)nv * (chunk + 1) / nchunk);
  float t0[J][V], t1[J][V];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int v = v0 + threadIdx.x + 256 * j;
    if (v >= v1) break;
    BilWalk w(v * V, c, wi, sw, f_c);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float *a, *b;
      w.taps(rows, c, wi, sw, a, b);
      t0[j][k] = fmaf(w.lw1, b[0], w.lw0 * a[0]);
      t1[j][k] = fmaf(w.lw1, b[rl], w.lw0 * a[rl]);
    }
  }
  for (int oh = oa; oh < ob; ++oh) {
    T* yo = y + ((long)img * ho + oh) * wo * c;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int v = v0 + threadIdx.x + 256 * j;
      if (v >= v1) break;
      bil_group_store(yo + (long)v * V, t0[j], t1[j], oh, sh, hi);
    }
  }
}

static constexpr auto kBilGroupU = 4;  // column vectors per thread of bilinear_fwd_group_vec_kernel (1 / 2 / 4: 48 / 43 / 41 us, profiles/r6f)
static constexpr auto kBilJ = 2;  // output vectors per thread and column chunk (2, 3, 4, 6 measured: 2 best)

// Backward, separable gather (deterministic, no atomics): input index i along one axis
// receives from outputs o with i0(o) == i (weight l0) or i1(o) == i (weight l1); those o lie
// in [(i-0.5)/s - 0.5, (i+1.5)/s - 0.5], widened by one and tested exactly with bil_src.
// bil_adj_range: the outputs [lo, hi] that inputs [i0, i1] may receive from; the host sizes tables
// and LDS segments with the same function, so it computes exactly what the device computes.
__host__ __device__ inline void bil_adj_range(int i0, int i1, float s, int out, int& lo, int& hi) {
  lo = (int)floorf(((float)i0 - 0.5f) / s - 0.5f) - 1;
  hi = (int)ceilf(((float)i1 + 1.5f) / s - 0.5f) + 1;
  lo = lo < 0 ? 0 : lo;
  hi = hi > out - 1 ? out - 1 : hi;
}
RT_DEV float bil_weight(int o, int i, float s, int in) {
  int a0, a1;
  float l0, l1;
  bil_src(o, s, in, a0, a1, l0, l1);
  return (a0 == i ? l0 : 0.f) + (a1 == i ? l1 : 0.f);
}
// bil_gather: the adjoint sum of one input element over its cnt candidate outputs, src[j * stride]
// with weight(j) -- ascending j, zero weights skipped, one fmaf per tap: the summation order of
// every width and height pass, tabulated or not
template <typename S, typename I, typename W>
RT_DEV float bil_gather(const S* src, I stride, int cnt, W weight) {
  float acc = 0.f;
  for (int j = 0; j < cnt; ++j) {
    const float wt = weight(j);
    if (wt != 0.f) acc = fmaf(wt, to_f(src[j * stride]), acc);
  }
  return acc;
}
// Weight tables: the weights of one axis (per input index i: lo(i) and w(lo + j -> i), zero past
// hi(i)) tabulated once per block in LDS instead of being re-derived (two bil_src evaluations)
// for every element and tap.  Rows for inputs [i0, i0 + cnt); tlo = lo(i) - origin.
static const int kBilTabLds = 48 * 1024;
static size_t bil_tab_bytes(int in, int maxw) { return ((size_t)in * maxw + in) * 4; }
RT_DEV void bil_table_build(float* tab, int* tlo, int i0, int cnt, int in, int out, float s, int maxw, int origin) {
  for (int e = threadIdx.x; e < cnt * maxw; e += blockDim.x) {
    const int il = e / maxw, j = e - il * maxw, i = i0 + il;
    int lo, hi;
    bil_adj_range(i, i, s, out, lo, hi);
    tab[e] = lo + j <= hi ? bil_weight(lo + j, i, s, in) : 0.f;
    if (j == 0) tlo[il] = lo - origin;
  }
  __syncthreads();
}
// The two passes, each with its weights from a table in LDS (TAB: the table fits and the index
// math fits 32 bits) or computed per tap; bil_gather either way, so the sums are bit-identical.
// pass 1 (W): tmp[img][oh][iw][c] = sum_ow w(ow->iw) dy[img][oh][ow][c]   (fp32)
template <typename T, bool TAB>
__global__ void bilinear_bwd_w_kernel(const T* __restrict__ dy, float* __restrict__ tmp, int n, int wi, int c, int ho, int wo, float sw,
                                      int dyld, int dyoff, int maxw, FastDiv f_c, FastDiv f_wi) {
  extern __shared__ float tab[];
  int* tlo = (int*)(tab + wi * maxw);
  if (TAB) bil_table_build(tab, tlo, 0, wi, wi, wo, sw, maxw, 0);
  const long total = (long)n * ho * wi * c;  // TAB: < 2^31 (host)
  GRID_STRIDE(i, total) {
    if (TAB) {
      const uint32_t q = fdiv((uint32_t)i, f_c), row = fdiv(q, f_wi);  // row = img * ho + oh
      const int ch = (int)((uint32_t)i - q * c), iw = (int)(q - row * wi);
      const float* w = tab + iw * maxw;
      tmp[i] = bil_gather(dy + ((long)row * wo + tlo[iw]) * dyld + dyoff + ch, (long)dyld, maxw, [&](int j) { return w[j]; });
    } else {
      const int ch = (int)(i % c);
      const long q = i / c, row = q / wi;
      const int iw = (int)(q % wi);
      int lo, hi;
      bil_adj_range(iw, iw, sw, wo, lo, hi);
      tmp[i] = bil_gather(dy + (row * wo + lo) * dyld + dyoff + ch, (long)dyld, hi - lo + 1,
                          [&](int j) { return bil_weight(lo + j, iw, sw, wi); });
    }
  }
}
// pass 2 (H): dx[img][ih][iw][c] = sum_oh w(oh->ih) tmp[img][oh][iw][c]
template <typename T, bool TAB>
__global__ void bilinear_bwd_h_kernel(const float* __restrict__ tmp, T* __restrict__ dx, int n, int hi, int wi, int c, int ho, float sh,
                                      int maxh, FastDiv f_plane, FastDiv f_hi) {
  extern __shared__ float tab[];
  int* tlo = (int*)(tab + hi * maxh);
  if (TAB) bil_table_build(tab, tlo, 0, hi, hi, ho, sh, maxh, 0);
  const long plane = (long)wi * c;
  const long total = (long)n * hi * plane;  // TAB: < 2^31 (host)
  GRID_STRIDE(i, total) {
    if (TAB) {
      const uint32_t q = fdiv((uint32_t)i, f_plane), img = fdiv(q, f_hi);
      const uint32_t inner = (uint32_t)i - q * (uint32_t)plane;  // iw * c + ch
      const int ih = (int)(q - img * hi);
      const float* w = tab + ih * maxh;
      dx[i] = from_f<T>(bil_gather(tmp + ((long)img * ho + tlo[ih]) * plane + inner, plane, maxh, [&](int j) { return w[j]; }));
    } else {
      const long inner = i % plane, q = i / plane;
      const int ih = (int)(q % hi), img = (int)(q / hi);
      int lo, hh;
      bil_adj_range(ih, ih, sh, ho, lo, hh);
      dx[i] = from_f<T>(bil_gather(tmp + ((long)img * ho + lo) * plane + inner, plane, hh - lo + 1,
                                   [&](int j) { return bil_weight(lo + j, ih, sh, hi); }));
    }
  }
}
// most outputs any input index of an axis receives from.  The + 1 dates from a host copy of the
// range formula that might have rounded differently; it is part of every table's row length and
// LDS byte count (and so of the routes taken), so it stays.
static int bil_maxw(int in, int out, float s) {
  int m = 0;
  for (int i = 0; i < in; ++i) {
    int lo, hi;
    bil_adj_range(i, i, s, out, lo, hi);
    m = std::max(m, hi - lo + 1);
  }
  return m + 1;
}
// the H pass of the bilinear backward and of the resize + softmax backward
template <typename T>
static void bil_bwd_h_launch(const float* tmp, T* dx, int n, int hi, int wi, int c, int ho, float sh, hipStream_t st) {
  const long th = (long)n * hi * wi * c;
  const int mh = bil_maxw(hi, ho, sh);
  const size_t bh = bil_tab_bytes(hi, mh);
  with_bool(th < (1L << 31) && bh <= (size_t)kBilTabLds, [&](auto tab) {
    constexpr bool TAB = decltype(tab)::value;
    hipLaunchKernelGGL((bilinear_bwd_h_kernel<T, TAB>), dim3(ew_blocks(th)), dim3(256), TAB ? bh : 0, st, tmp, dx, n, hi, wi, c, ho,
                       sh, mh, TAB ? fastdiv_make((uint32_t)wi * c) : FastDiv{}, fastdiv_make(hi));
  });
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
// The fused backward's LDS: the W and H weight tables with their first output and nonzero span per
// row.  bytes() is the dynamic LDS the host launches with.
struct BilTables {
  float *wtab, *htab;
  int *wlo, *hlo, *wspan, *hspan;
  static size_t bytes(int hi, int wi, int maxh, int maxw) { return bil_tab_bytes(wi, maxw) + bil_tab_bytes(hi, maxh) + (wi + hi) * 4; }
  RT_DEV BilTables(float* lds, int hi, int wi, int ho, int wo, float sh, float sw, int maxh, int maxw) {
    wtab = lds;
    wlo = (int*)(wtab + wi * maxw);
    htab = (float*)(wlo + wi);
    hlo = (int*)(htab + hi * maxh);
    wspan = hlo + hi;
    hspan = wspan + wi;
    bil_table_build(wtab, wlo, 0, wi, wi, wo, sw, maxw, 0);
    bil_table_build(htab, hlo, 0, hi, hi, ho, sh, maxh, 0);
    bil_table_span(wtab, wspan, wi, maxw);
    bil_table_span(htab, hspan, hi, maxh);
  }
};
// Both passes in one kernel: a thread owns W channels of one input pixel (W = the 16-B vector
// when c, the pitch and the offset of dY allow it; else 1 with dY dense, the supervision heads'
// 19-class logits: adjacent lanes read adjacent channels, so each tap's loads stay contiguous
// across the wave) and forms each output row's W-pass sum t (the W kernel's taps, order and
// zero skipping, fp32) right before the H-pass FMA that consumes it -- the same two fp32 FMA
// chains, so dx is bit-identical to the two-pass kernels, without the fp32 [ho][wi]
// intermediate's write and re-read.  Neighbouring input pixels re-read dY rows through L2
// (XCD-aware block order).  Only each row's nonzero span is visited, and its column taps go G
// at a time: the G loads issued (clamped into the span) before their FMAs, a zero weight
// leaving t unchanged exactly as the skipped tap of the two-pass kernel.
template <typename T, int W, int G>
__global__ void __launch_bounds__(256) bilinear_bwd_fused_kernel(const T* __restrict__ dy, T* __restrict__ dx, int hi, int wi, int c,
                                                                 int ho, int wo, float sh, float sw, int dyld, int dyoff, int maxh,
                                                                 int maxw, long total, FastDiv f_cw, FastDiv f_wi, FastDiv f_hi) {
  extern __shared__ float tab[];
  const BilTables tb(tab, hi, wi, ho, wo, sh, sw, maxh, maxw);
  typedef T VW __attribute__((ext_vector_type(W)));
  const int cw = c / W;
  GRID_STRIDE_XCD(i, total) {  // total < 2^31 (host)
    const uint32_t q = fdiv((uint32_t)i, f_cw), r = fdiv(q, f_wi);
    const int ch = ((int)((uint32_t)i - q * cw)) * W, iw = (int)(q - r * wi);
    const uint32_t img = fdiv(r, f_hi);
    const int ih = (int)(r - img * hi);
    const float* wx = tb.wtab + iw * maxw;
    const float* wy = tb.htab + ih * maxh;
    const T* base = dy + (((long)img * ho + tb.hlo[ih]) * wo + tb.wlo[iw]) * dyld + dyoff + ch;
    const int jx0 = tb.wspan[iw] & 0xffff, jx1 = tb.wspan[iw] >> 16;
    const int ky0 = tb.hspan[ih] & 0xffff, ky1 = tb.hspan[ih] >> 16;
    float acc[W];
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = 0.f;
    for (int k = ky0; k < ky1; ++k) {
      const float yk = wy[k];
      if (yk == 0.f) continue;
      const T* row = base + (long)k * wo * dyld;
      float t[W];
#pragma unroll
      for (int e = 0; e < W; ++e) t[e] = 0.f;
      for (int j0 = jx0; j0 < jx1; j0 += G) {
        VW v[G];
        float xw[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          const int j = j0 + u;
          xw[u] = j < jx1 ? wx[j] : 0.f;
          v[u] = *(const VW*)(row + (long)min(j, jx1 - 1) * dyld);
        }
#pragma unroll
        for (int u = 0; u < G; ++u)
#pragma unroll
          for (int e = 0; e < W; ++e) t[e] = xw[u] != 0.f ? fmaf(xw[u], to_f(v[u][e]), t[e]) : t[e];
      }
#pragma unroll
      for (int e = 0; e < W; ++e) acc[e] = fmaf(yk, t[e], acc[e]);
    }
    VW o;
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = from_f<T>(acc[e]);
    *(VW*)(dx + i * W) = o;  // i = ((img * hi + ih) * wi + iw) * cw + ch / W
  }
}
// one kernel for both passes when its tables fit and the index math fits 32 bits, else the two
// passes; dy is read with row pitch dyld at channel offset dyoff
template <typename T>
static void bilinear_bwd_launch(const T* dy, float* tmp, T* dx, int n, int hi, int wi, int c, int ho, int wo, float sh, float sw,
                                int dyld, int dyoff, hipStream_t st) {
  const long tw = (long)n * ho * wi * c, th = (long)n * hi * wi * c;
  const int mw = bil_maxw(wi, wo, sw), mh = bil_maxw(hi, ho, sh);
  const size_t bw = bil_tab_bytes(wi, mw), fused = BilTables::bytes(hi, wi, mh, mw);
  constexpr int V = VecT<T>::N;
  const bool vec = c % V == 0 && dyld % V == 0 && dyoff % V == 0, scalar = c % V != 0 && dyld == c && dyoff == 0;
  if ((vec || scalar) && th < (1L << 31) && fused <= (size_t)kBilTabLds && (long)n * ho * wo * dyld < (1L << 40)) {
    // taps per load batch: 8 when an input column reaches ~8 output columns (x4), else 4 (x2)
    with_bool(vec, [&](auto v) {
      with_bool(mw >= 10, [&](auto g8) {
        constexpr int W = decltype(v)::value ? V : 1, G = decltype(g8)::value ? 8 : 4;
        hipLaunchKernelGGL((bilinear_bwd_fused_kernel<T, W, G>), dim3(ew_blocks(th / W)), dim3(256), fused, st, dy, dx, hi, wi, c,
                           ho, wo, sh, sw, dyld, dyoff, mh, mw, th / W, fastdiv_make(c / W), fastdiv_make(wi), fastdiv_make(hi));
      });
    });
    return;
  }
  with_bool(tw < (1L << 31) && bw <= (size_t)kBilTabLds, [&](auto tab) {
    constexpr bool TAB = decltype(tab)::value;
    hipLaunchKernelGGL((bilinear_bwd_w_kernel<T, TAB>), dim3(ew_blocks(tw)), dim3(256), TAB ? bw : 0, st, dy, tmp, n, wi, c, ho, wo, sw,
                       dyld, dyoff, mw, fastdiv_make(c), fastdiv_make(wi));
  });
  bil_bwd_h_launch(tmp, dx, n, hi, wi, c, ho, sh, st);
}
template <typename T>
static void bil_group_vec_launch(const void* x, void* y, int n, int hi, int wi, int c, int ho, int wo, float sh, float sw, int y_ld,
                                 int y_off, const void* s1, const void* s2, hipStream_t st) {
  hipLaunchKernelGGL((bilinear_fwd_group_vec_kernel<T, kBilGroupU>), dim3(rt_cdiv(wo * (c / VecT<T>::N), 256 * kBilGroupU), n * hi),
                     dim3(256), 0, st, (const T*)x, (T*)y, n, hi, wi, c, ho, wo, sh, sw, y_ld, y_off, (const T*)s1, (const T*)s2);
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
    if (c % V == 0 && y_ld % V == 0 && y_off % V == 0 && ho >= 3 * hi)
      bil_group_vec_launch<T>(x, y, n, hi, wi, c, ho, wo, scale_h, scale_w, y_ld, y_off, nullptr, nullptr, st);
    else if (c % V == 0 && y_ld % V == 0 && y_off % V == 0)
      hipLaunchKernelGGL((bilinear_fwd_kernel<T, 0>), dim3(ew_blocks(pix * (c / V))), dim3(256), 0, st, (const T*)x, (T*)y, n, hi, wi, c, ho, wo, scale_h, scale_w, y_ld, y_off);
    else if (c >= V && y_ld == c && y_off == 0 && (wo * c) % V == 0 && 2L * wi * c * 4 <= 64 * 1024 && ho >= hi) {
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
    bil_group_vec_launch<T>(x, y, n, hi, wi, c, ho, wo, scale_h, scale_w, y_ld, y_off, s1, s2, st);
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
//             16-B loads); the tile's bilinear weights are tabulated once in LDS
//             (bil_table_build); thread per (input column, class) accumulates the width adjoint
//             with bil_gather, as bilinear_bwd_w_kernel does.  The vertical pass is
//             bil_bwd_h_launch.
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
// the same for any run of output pixels [ow0, ow0 + np) of output row `row` (the self-information
// backward's tiles are runs of the output columns that a tile of input columns receives from)
template <typename T, bool STAGED>
RT_DEV UpsmTile<T> upsm_span(const T* __restrict__ x, float* src, long row, int ow0, int np, int hi, int wi, int c, int ho, float sh,
                             float sw) {
  UpsmTile<T> t;
  t.row = row;
  const int oh = (int)(t.row % ho), img = (int)(t.row / ho);
  t.ow0 = ow0;
  t.np = np;
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
    bil_stage_rows(t.r0 + (long)t.wlo * c, t.r1 + (long)t.wlo * c, src, t.n1);
  }
  return t;
}
template <typename T, bool STAGED>
RT_DEV UpsmTile<T> upsm_tile(const T* __restrict__ x, float* src, int hi, int wi, int c, int ho, int wo, float sh, float sw,
                             int tiles) {
  const int ow0 = blockIdx.x % tiles * kUpsmPix;
  return upsm_span<T, STAGED>(x, src, blockIdx.x / tiles, ow0, min(kUpsmPix, wo - ow0), hi, wi, c, ho, sh, sw);
}
// class k of one output pixel's resized logits, upsm_probs' z[k] ahead of its exp: bil_mix of the
// four taps (column taps w0 / w1 of the staged rows, or of r0 / r1), rounded to T as
// rtsds_bilinear_fwd stores it and widened again.  For kernels that reduce the classes on the fly
// (upsample_paint_kernel).  upsm_probs keeps its own copy of the eight tap reads: calling this
// from it left every staged kernel's code as it was but gave the unstaged ones 64-bit address
// arithmetic per tap (v_lshl_add_u64 11 -> 135 in upsoftmax_acc_kernel<float, false, 0>).
template <typename T, bool STAGED>
RT_DEV float upsm_logit(const T* __restrict__ r0, const T* __restrict__ r1, const float* src, int wlo, int n1, int c, int k, int w0,
                        int w1, float lh0, float lh1, float lw0, float lw1) {
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
  return to_f(from_f<T>(bil_mix(p00, p01, p10, p11, lh0, lh1, lw0, lw1)));
}
// one output pixel's blend + softmax, shared by upsoftmax_fwd_kernel and upsoftmax_acc_kernel:
// on return the probability of class k is the fp32 product z[k] * iz.  With LOGITS it stops ahead of
// the exponentials: z[k] is the resized logit of class k, rounded to T as rtsds_bilinear_fwd stores
// it, and iz their maximum (upsm_logits).  One function with a switch, not a blend that this one
// calls: that split gave every staged runtime-c kernel 90 more instructions (the second row's LDS
// addresses formed per class), the same sensitivity as upsm_logit's above.
template <typename T, bool STAGED, int CC, bool LOGITS = false>
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
  if (LOGITS) {
    iz = m;
    return;
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
// one output pixel's resized logits z[k] (upsm_probs' values ahead of the exponentials); returns their maximum
template <typename T, bool STAGED, int CC>
RT_DEV float upsm_logits(const T* __restrict__ r0, const T* __restrict__ r1, const float* src, int wlo, int n1, int c_, int ow,
                         float sw, int wi, float lh0, float lh1, float (&z)[kUpsmMaxC]) {
  float m;
  upsm_probs<T, STAGED, CC, true>(r0, r1, src, wlo, n1, c_, ow, sw, wi, lh0, lh1, z, m);
  return m;
}
// one output pixel's self-information terms (rtsds_upselfinfo_fwd / _bwd, include/rtsds_hip.h): from
// the resized logits z and their maximum m (upsm_logits), e_k = expf(z_k - m), iz = 1 / S and
// ls = logf(S) with S = sum_k e_k in class order, so that p_k = e_k * iz and L_k = ls - (z_k - m) =
// -ln p_k >= 0: one logf per pixel, none per class.  e_k is held beside z_k: evaluating expf again
// where it is used (one 32-float array per lane instead of two, as softmax_fwd_staged does) measured
// the same in both kernels and both dtypes (profiles/advent/README.md).
struct UpsiRow {
  float z[kUpsmMaxC], e[kUpsmMaxC];
  float m, iz, ls;
  RT_DEV float d(int k) const { return z[k] - m; }
};
template <int CC>
RT_DEV void upsi_sums(UpsiRow& r, int c_) {
  const int c = CC > 0 ? CC : c_;
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < kUpsmMaxC; ++k)
    if (k < c) {
      r.e[k] = expf(r.z[k] - r.m);
      sum += r.e[k];
    }
  r.iz = 1.f / sum;
  r.ls = logf(sum);
}
// I_k = p_k L_k / ln c; a class with e_k == 0 (a logit at -inf, or one underflowed) gives 0, not 0 * inf
RT_DEV float upsi_info(const UpsiRow& r, int k, float inv_lnc) {
  const float e = r.e[k];
  return e == 0.f ? 0.f : e * r.iz * (r.ls - r.d(k)) * inv_lnc;
}
// the padded row of one output pixel, val(k) for k < c and zeros behind, into the LDS tile.  The row
// goes through LDS so the tile leaves as lane-consecutive 16-B chunks (the tile's rows are contiguous
// in y): full-line writes instead of 64-B-strided partial ones
template <typename T, typename V>
RT_DEV void upsm_row_out(T* o, int ow, int c, int yld, V val) {
  if (sizeof(T) == 2 && yld == 32) {  // 4 x 16-B LDS writes, chunk q at slot q ^ (pixel & 3)
    typedef typename VecT<T>::v16 V16;
    const int sw4 = ow & 3;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      V16 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = from_f<T>(q * 8 + j < c ? val(q * 8 + j) : 0.f);
      *(V16*)(o + (q ^ sw4) * 8) = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kUpsmMaxC; ++k)
      if (k < yld) o[k] = from_f<T>(k < c ? val(k) : 0.f);
  }
}
// one output pixel of the forward tile: blend, softmax (SI: self-information on top), padded row into the LDS tile
template <typename T, bool STAGED, int CC, bool SI>
RT_DEV void upsm_pixel(const T* __restrict__ r0, const T* __restrict__ r1, const float* src, T* o, int wlo, int n1, int c_, int ow,
                       float sw, int wi, float lh0, float lh1, int yld, float inv_lnc) {
  const int c = CC > 0 ? CC : c_;
  if (SI) {
    UpsiRow r;
    r.m = upsm_logits<T, STAGED, CC>(r0, r1, src, wlo, n1, c_, ow, sw, wi, lh0, lh1, r.z);
    upsi_sums<CC>(r, c_);
    upsm_row_out(o, ow, c, yld, [&](int k) { return upsi_info(r, k, inv_lnc); });
  } else {
    float z[kUpsmMaxC];
    float iz;
    upsm_probs<T, STAGED, CC>(r0, r1, src, wlo, n1, c_, ow, sw, wi, lh0, lh1, z, iz);
    upsm_row_out(o, ow, c, yld, [&](int k) { return z[k] * iz; });
  }
}
// the forward tile of rtsds_upsoftmax_fwd and rtsds_upselfinfo_fwd (SI)
template <typename T, bool STAGED, int CC, bool SI>
RT_DEV void upsm_fwd_tile(const T* __restrict__ x, T* __restrict__ y, int hi, int wi, int c_, int ho, int wo, float sh, float sw,
                          int yld, int tiles, float inv_lnc) {
  const int c = CC > 0 ? CC : c_;
  extern __shared__ __attribute__((aligned(16))) float src[];  // STAGED: [2][ncols][c]
  const int tid = threadIdx.x;
  const UpsmTile<T> tl = upsm_tile<T, STAGED>(x, src, hi, wi, c, ho, wo, sh, sw, tiles);
  const int ow0 = tl.ow0, np = tl.np;
  if (STAGED) __syncthreads();
  T* outbuf = (T*)(src + ((2 * tl.n1 + 3) & ~3));  // [256][yld], 16-B aligned
  if (tid < np)
    upsm_pixel<T, STAGED, CC, SI>(tl.r0, tl.r1, src, outbuf + tid * yld, tl.wlo, tl.n1, c, ow0 + tid, sw, wi, tl.lh0, tl.lh1, yld,
                                  inv_lnc);
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
template <typename T, bool STAGED, int CC>  // CC > 0: compile-time class count (19), 0: runtime c
__global__ void __launch_bounds__(256) upsoftmax_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int hi, int wi, int c_,
                                                            int ho, int wo, float sh, float sw, int yld, int tiles) {
  upsm_fwd_tile<T, STAGED, CC, false>(x, y, hi, wi, c_, ho, wo, sh, sw, yld, tiles, 0.f);
}
template <typename T, bool STAGED, int CC>
__global__ void __launch_bounds__(256) upselfinfo_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int hi, int wi, int c_,
                                                             int ho, int wo, float sh, float sw, int yld, int tiles, float inv_lnc) {
  upsm_fwd_tile<T, STAGED, CC, true>(x, y, hi, wi, c_, ho, wo, sh, sw, yld, tiles, inv_lnc);
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
        if (k == 0 || v > best) {  // not first_max(): no NaN clause (class-vector unit)
          best = v;
          bi = k;
        }
      }
    if (pred != nullptr) pred[tl.row * wo + d0 + lp] = bi;
  }
  __syncthreads();  // every lane reaches the same barrier (no early exit)
  upsm_tile_copy<false>(dst, tbuf, nel, head);
}
// ------------------------------------------------------------------ low-resolution head -> pseudo-labels
// The online teacher's labels (selftrain.TeacherLoader): upsoftmax_acc_kernel's tile and
// probabilities (accumulate = 0, flip = 0: v[k] = __fmul_rn(z[k], iz)), reduced in registers by
// conf_hist_tile's calls (class_row.h: first_max(), conf_bin() of conf = best * 1.0f) and
// thresholded by pseudo_select_kernel's pseudo_label(): pred / cbin / labels equal the
// chain rtsds_upsoftmax_acc -> rtsds_conf_hist (inv = 1) -> rtsds_pseudo_select bit for bit, and
// the fp32 probability tensor (c x 4 B written and read again per pixel) never exists.  LDS holds
// the staged source rows only; a tile's pixels are lane-consecutive, so each output leaves as
// contiguous 1 / 2 / 8-B stores of a wave.
template <typename T, bool STAGED, int CC>  // CC > 0: compile-time class count (19), 0: runtime c
__global__ void __launch_bounds__(256) upsample_pseudo_kernel(const T* __restrict__ x, uint8_t* __restrict__ pred,
                                                              uint16_t* __restrict__ cbin, const int* __restrict__ tbin,
                                                              int64_t* __restrict__ labels, int hi, int wi, int c_, int ho, int wo,
                                                              float sh, float sw, int bins, int ignore, int tiles) {
  const int c = CC > 0 ? CC : c_;
  extern __shared__ __attribute__((aligned(16))) float src[];  // STAGED: [2][ncols][c]
  const int tid = threadIdx.x;
  const UpsmTile<T> tl = upsm_tile<T, STAGED>(x, src, hi, wi, c, ho, wo, sh, sw, tiles);
  if (STAGED) __syncthreads();
  if (tid >= tl.np) return;  // no barrier below
  float z[kUpsmMaxC];
  float iz;
  upsm_probs<T, STAGED, CC>(tl.r0, tl.r1, src, tl.wlo, tl.n1, c, tl.ow0 + tid, sw, wi, tl.lh0, tl.lh1, z, iz);
  float best;
  const int bi = first_max<kUpsmMaxC>([&](int k) { return __fmul_rn(z[k], iz); }, c, best);
  const int b = conf_bin(best * 1.0f, bins);
  const long p = tl.row * wo + tl.ow0 + tid;
  if (pred) pred[p] = (uint8_t)bi;
  if (cbin) cbin[p] = (uint16_t)b;
  if (labels) labels[p] = pseudo_label<false>(bi, b, tbin, c, ignore);  // bi < c by construction
}
// ------------------------------------------------------------------ low-resolution head -> painted frame
// The output side of inference (predict.Predictor): the same tile, but no softmax -- k = arg-max
// of the resized logits (upsm_logit: what rtsds_bilinear_fwd would store) by first_max()
// (class_row.h, rtsds_argmax's scan) over a callable, a running maximum, so
// ids equal the chain rtsds_bilinear_fwd -> rtsds_argmax bit for bit and the full-resolution
// logits never exist.  ids[p] = lut[k] (k without a lut); rgb[p] = palette[k], blended over the
// frame in integers: (alpha * palette + (256 - alpha) * frame + 128) >> 8, alpha in [0, 256].
// Palette and lut (<= 96 + 32 B) sit in LDS behind the staged rows.  The 3-byte pixels of a tile
// are contiguous (768 B) at any byte phase: every lane reads its pixel's 3 frame bytes and writes
// its 3 output bytes itself, a wave covering 192 contiguous bytes per access.  (Routing both
// tiles through LDS as 16-B chunks with single head / tail bytes, upsm_tile_copy's way, measured
// 1.0 - 4.6 us slower per call at every shape, profiles/paint: a second barrier, 48 active lanes
// per copy, and the kernel is bound by the class loop, not by its stores.)
static const int kPaintTab = 4 * kUpsmMaxC;  // bytes: palette [c][3], then lut [c]
template <typename T, bool STAGED, int CC>  // CC > 0: compile-time class count (19), 0: runtime c
__global__ void __launch_bounds__(256) upsample_paint_kernel(const T* __restrict__ x, const uint8_t* __restrict__ frame,
                                                             const uint8_t* __restrict__ palette, const uint8_t* __restrict__ lut,
                                                             uint8_t* __restrict__ ids, uint8_t* __restrict__ rgb, int hi, int wi,
                                                             int c_, int ho, int wo, float sh, float sw, int alpha, int tiles) {
  const int c = CC > 0 ? CC : c_;
  extern __shared__ __attribute__((aligned(16))) float src[];  // STAGED: [2][ncols][c]
  const int tid = threadIdx.x;
  const UpsmTile<T> tl = upsm_tile<T, STAGED>(x, src, hi, wi, c, ho, wo, sh, sw, tiles);
  uint8_t* pal = (uint8_t*)(src + ((2 * tl.n1 + 3) & ~3));  // 16-B aligned
  uint8_t* idt = pal + 3 * kUpsmMaxC;
  if (rgb != nullptr && tid < 3 * c) pal[tid] = palette[tid];
  if (tid >= 128 && tid - 128 < c) idt[tid - 128] = lut != nullptr ? lut[tid - 128] : (uint8_t)(tid - 128);
  const bool blend = rgb != nullptr && alpha < 256;
  const long p = tl.row * wo + tl.ow0 + tid;  // this lane's pixel (tid < np)
  int f0 = 0, f1 = 0, f2 = 0;
  if (blend && tid < tl.np) {  // issued ahead of the barrier and the class loop
    const uint8_t* f = frame + 3 * p;
    f0 = f[0], f1 = f[1], f2 = f[2];
  }
  __syncthreads();
  if (tid >= tl.np) return;  // no barrier below
  int w0, w1;
  float lw0, lw1;
  bil_src(tl.ow0 + tid, sw, wi, w0, w1, lw0, lw1);
  float best;
  const int bi = first_max<kUpsmMaxC>(
      [&](int k) { return upsm_logit<T, STAGED>(tl.r0, tl.r1, src, tl.wlo, tl.n1, c, k, w0, w1, tl.lh0, tl.lh1, lw0, lw1); }, c, best);
  if (ids != nullptr) ids[p] = idt[bi];
  if (rgb != nullptr) {
    int q0 = pal[3 * bi], q1 = pal[3 * bi + 1], q2 = pal[3 * bi + 2];
    if (blend) {
      q0 = (alpha * q0 + (256 - alpha) * f0 + 128) >> 8;
      q1 = (alpha * q1 + (256 - alpha) * f1 + 128) >> 8;
      q2 = (alpha * q2 + (256 - alpha) * f2 + 128) >> 8;
    }
    uint8_t* o = rgb + 3 * p;
    o[0] = (uint8_t)q0, o[1] = (uint8_t)q1, o[2] = (uint8_t)q2;
  }
}
// ------------------------------------------------------------------ sliding windows -> painted frame
// Tiled inference at native resolution (validation.predict_sliding, predict.Predictor(stride=)):
// the model ran on nwin overlapping hw x ww crops of an H x W canvas; each crop's head gives
// upsoftmax_acc_kernel's probabilities (upsm_probs, then __fmul_rn) at the crop's own pixels, and a
// canvas pixel's result is their sum over the windows covering it, in ascending window index, one
// __fadd_rn each -- the chain rtsds_upsoftmax_acc per window -> slice add onto a zero canvas, bit
// for bit.  One owner per canvas pixel, so no atomics: a block takes 256 consecutive columns of
// one canvas row (slide tile set-up below: upsm_tile's, in canvas coordinates), filters the window
// table by its row and column range -- a test on blockIdx alone, so block-uniform, as is the
// barrier count -- and per kept window stages the two source rows of the window columns it covers
// (a mirrored window maps the tile's range to a contiguous, reversed range of window columns:
// the staging is the same) and lets the lanes inside the window add their probabilities onto
// their register row.  The sum is reduced in registers to the class (upsoftmax_acc_kernel's
// pred rule) and leaves as upsample_paint_kernel's bytes; the fp32 canvas acc is optional (in:
// accumulate, for window chunks; out: when given) and moves as upsm_tile_copy's 16-B chunks
// through an LDS tile.  Without it the kernel touches no fp32 canvas at all: 1 - 7 B per pixel.
// The window table travels by value in the kernel's arguments (<= 64 windows, 520 B): no device
// table to keep alive or to clamp.
static const int kSlideMaxWin = 64;
struct SlideWins {
  int y0[kSlideMaxWin], x0[kSlideMaxWin];
  unsigned long long flip;  // bit k: window k is mirrored
};
// one class of one window's probabilities, p = __fmul_rn(z, iz), added onto the running sum by one
// __fadd_rn (first: the sum starts as p).  The header intrinsics are plain operators the compiler
// may still contract into an FMA (optim.hip, ema_update), and here it did: the two operations
// are written out with contraction switched off for this function.
RT_DEV float slide_sum(float s, float z, float iz, bool any) {
#pragma clang fp contract(off)
  const float p = z * iz;
  return any ? s + p : p;
}
template <typename T, bool STAGED, int CC>  // CC > 0: compile-time class count (19), 0: runtime c
__global__ void __launch_bounds__(256) slide_paint_kernel(const T* __restrict__ x, const SlideWins wt, int nwin,
                                                          const uint8_t* __restrict__ frame, const uint8_t* __restrict__ palette,
                                                          const uint8_t* __restrict__ lut, float* __restrict__ acc,
                                                          uint8_t* __restrict__ ids, uint8_t* __restrict__ rgb, int nf, int hi, int wi,
                                                          int c_, int hw, int ww, int H, int W, float sh, float sw, int accumulate,
                                                          int alpha, int tiles, int srcf) {
  const int c = CC > 0 ? CC : c_;
  // STAGED: [2][ncols][c] of the current window (srcf floats hold any window's), then the
  // palette / lut table, then (acc) the fp32 tile [np][c] at its destination's 16-B phase
  extern __shared__ __attribute__((aligned(16))) float src[];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % tiles;
  const long row = blockIdx.x / tiles;  // f * H + Y
  const int Y = (int)(row % H), f = (int)(row / H);
  const int X0 = tile * kUpsmPix, np = min(kUpsmPix, W - X0), X = X0 + tid;
  uint8_t* pal = (uint8_t*)(src + srcf);  // 16-B aligned
  uint8_t* idt = pal + 3 * kUpsmMaxC;
  if (rgb != nullptr && tid < 3 * c) pal[tid] = palette[tid];
  if (tid >= 128 && tid - 128 < c) idt[tid - 128] = lut != nullptr ? lut[tid - 128] : (uint8_t)(tid - 128);
  const bool blend = rgb != nullptr && alpha < 256;
  const long p = row * W + X;  // this lane's pixel (tid < np)
  int f0 = 0, f1 = 0, f2 = 0;
  if (blend && tid < np) {  // issued ahead of the barriers and the window loop
    const uint8_t* fp = frame + 3 * p;
    f0 = fp[0], f1 = fp[1], f2 = fp[2];
  }
  const int nel = np * c;
  float* dst = nullptr;
  float* tbuf = src + srcf + kPaintTab / 4;
  int head = 0;
  if (acc != nullptr) {
    dst = acc + (row * W + X0) * c;
    const int mis = (int)(((uintptr_t)dst >> 2) & 3);
    head = min(nel, (4 - mis) & 3);
    tbuf += mis;
  }
  if (accumulate) upsm_tile_copy<true>(dst, tbuf, nel, head);  // host: acc != nullptr
  __syncthreads();
  float s[kUpsmMaxC];
  bool any = accumulate != 0;  // s holds a sum already
#pragma unroll
  for (int k = 0; k < kUpsmMaxC; ++k) s[k] = (accumulate && tid < np && k < c) ? tbuf[tid * c + k] : 0.f;
  for (int k = 0; k < nwin; ++k) {
    const int y0 = wt.y0[k], x0 = wt.x0[k];
    if (Y < y0 || Y >= y0 + hw || x0 >= X0 + np || x0 + ww <= X0) continue;  // block-uniform
    const bool flip = (wt.flip >> k) & 1;
    int h0, h1;
    float lh0, lh1;
    bil_src(Y - y0, sh, hi, h0, h1, lh0, lh1);
    const T* hb = x + (long)(k * nf + f) * hi * wi * c;  // window-major heads
    const T* r0 = hb + (long)h0 * wi * c;
    const T* r1 = hb + (long)h1 * wi * c;
    int wlo = 0, n1 = 0;
    if (STAGED) {  // the window columns of the tile's part of this window; taps are monotone in ow
      const int da = max(X0, x0) - x0, db = min(X0 + np, x0 + ww) - 1 - x0;
      const int oa = flip ? ww - 1 - db : da, ob = flip ? ww - 1 - da : db;
      int a0, a1, b0, b1;
      float t0, t1;
      bil_src(oa, sw, wi, a0, a1, t0, t1);
      bil_src(ob, sw, wi, b0, b1, t0, t1);
      wlo = a0;
      n1 = (b1 - a0 + 1) * c;  // 2 * n1 <= srcf (host: slide_cols)
      __syncthreads();  // the previous window's taps have been read
      bil_stage_rows(r0 + (long)wlo * c, r1 + (long)wlo * c, src, n1);
      __syncthreads();
    }
    const int d = X - x0;  // this lane's column of the window
    if (tid < np && d >= 0 && d < ww) {
      float z[kUpsmMaxC];
      float iz;
      upsm_probs<T, STAGED, CC>(r0, r1, src, wlo, n1, c, flip ? ww - 1 - d : d, sw, wi, lh0, lh1, z, iz);
#pragma unroll
      for (int j = 0; j < kUpsmMaxC; ++j)
        if (j < c) s[j] = slide_sum(s[j], z[j], iz, any);
      any = true;
    }
  }
  if (tid < np) {
    float best = 0.f;
    int bi = 0;
#pragma unroll
    for (int j = 0; j < kUpsmMaxC; ++j)
      if (j < c) {
        if (acc != nullptr) tbuf[tid * c + j] = s[j];
        if (j == 0 || s[j] > best) {  // upsoftmax_acc_kernel's pred: no NaN clause
          best = s[j];
          bi = j;
        }
      }
    if (ids != nullptr) ids[p] = idt[bi];
    if (rgb != nullptr) {
      int q0 = pal[3 * bi], q1 = pal[3 * bi + 1], q2 = pal[3 * bi + 2];
      if (blend) {
        q0 = (alpha * q0 + (256 - alpha) * f0 + 128) >> 8;
        q1 = (alpha * q1 + (256 - alpha) * f1 + 128) >> 8;
        q2 = (alpha * q2 + (256 - alpha) * f2 + 128) >> 8;
      }
      uint8_t* o = rgb + 3 * p;
      o[0] = (uint8_t)q0, o[1] = (uint8_t)q1, o[2] = (uint8_t)q2;
    }
  }
  if (acc != nullptr) {  // block-uniform; every lane reaches the barrier (no early exit above)
    __syncthreads();
    upsm_tile_copy<false>(dst, tbuf, nel, head);
  }
}
// one tile of the fused backward kernels' width pass (blockIdx.x = row * tiles + tile): input
// columns [iw0, iw0 + nw) of row `row` = img * ho + oh, and the output columns [olo, olo + cnt)
// their width adjoint reads (cnt <= cap, the host's exact maximum over the tiles)
struct UpsmBwdTile {
  long row;
  int iw0, nw, olo, cnt;
};
RT_DEV UpsmBwdTile upsm_bwd_tile(int wi, int wo, float sw, int tw, int tiles) {
  UpsmBwdTile t;
  const int tile = blockIdx.x % tiles;
  t.row = blockIdx.x / tiles;
  t.iw0 = tile * tw;
  const int iw1 = min(wi, t.iw0 + tw) - 1;
  t.nw = iw1 - t.iw0 + 1;
  int ohi;
  bil_adj_range(t.iw0, iw1, sw, wo, t.olo, ohi);
  t.cnt = ohi - t.olo + 1;
  return t;
}
// the tile's dy segment -> LDS [cnt][c] (as T, or widened to fp32), coalesced (rows of pitch c;
// contiguous in memory when dyld == c); the caller places the barrier
template <typename T, typename S>
RT_DEV void upsm_bwd_stage(const T* __restrict__ dy, int dyld, S* seg, const UpsmBwdTile& t, int wo, int c) {
  const int tid = threadIdx.x;
  const T* gseg = dy + (t.row * wo + t.olo) * dyld;
  if (dyld == c) {
    for (int e = tid; e < t.cnt * c; e += 256) seg[e] = (S)gseg[e];
  } else {
    for (int e = tid; e < t.cnt * c; e += 256) {
      const int q = e / c;
      seg[e] = (S)gseg[(long)q * dyld + (e - q * c)];
    }
  }
}
// the width adjoint of the tile's LDS segment into tmp: the tile's bilinear weights tabulated in wt /
// wlo (the barrier behind the segment's last writes is bil_table_build's), then thread per (input
// column, class), classes inner, with bil_gather
template <typename S>
RT_DEV void upsm_bwd_gather(const S* seg, float* wt, int* wlo, float* __restrict__ tmp, const UpsmBwdTile& t, int wi, int c, int wo,
                            float sw, int maxw) {
  bil_table_build(wt, wlo, t.iw0, t.nw, wi, wo, sw, maxw, t.olo);  // wlo: relative to the staged segment
  for (int e = threadIdx.x; e < t.nw * c; e += 256) {
    const int il = e / c, k = e - il * c;
    const float* w = wt + il * maxw;
    tmp[(t.row * wi + t.iw0) * c + e] = bil_gather(seg + wlo[il] * c + k, c, maxw, [&](int j) { return w[j]; });
  }
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
  const UpsmBwdTile t = upsm_bwd_tile(wi, wo, sw, tw, tiles);
  const long row = t.row;
  const int olo = t.olo, cnt = t.cnt;
  upsm_bwd_stage(dy, dyld, sgt, t, wo, c);
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
  upsm_bwd_gather(sgt, wt, wlo, tmp, t, wi, c, wo, sw, maxw);
}
// rtsds_upselfinfo_bwd's width pass, upsoftmax_bwd_w_kernel's tile: the dy segment is staged as
// fp32, and beside it the columns of the two low-resolution source rows that the segment's output
// pixels tap (upsm_span: the forward's staging).  Thread per output pixel: the forward's logits
// again (upsm_logits, upsi_sums: bit for bit the forward's z, p and L), then
// dz_j = p_j (u_j - sum_k p_k u_k), u_k = dy_k (L_k - 1) / ln c, in place as fp32; the width adjoint
// reads that.  Nothing of the forward's output is read.
template <typename T, int CC>  // CC > 0: compile-time class count (19), 0: runtime c
__global__ void __launch_bounds__(256) upselfinfo_bwd_w_kernel(const T* __restrict__ dy, int dyld, const T* __restrict__ x,
                                                               float* __restrict__ tmp, int hi, int wi, int c_, int ho, int wo,
                                                               float sh, float sw, int tw, int tiles, int cap, int maxw, int srcf,
                                                               float inv_lnc) {
  const int c = CC > 0 ? CC : c_;
  extern __shared__ __attribute__((aligned(16))) float smf[];
  float* src = smf;                      // [2][columns][c] (srcf floats: the host's bound)
  float* dz = src + srcf;                // [cap][c]: dy, then dz in place
  float* wt = dz + cap * c;              // [tw][maxw]
  int* wlo = (int*)(wt + tw * maxw);     // [tw]
  const UpsmBwdTile t = upsm_bwd_tile(wi, wo, sw, tw, tiles);
  const UpsmTile<T> tl = upsm_span<T, true>(x, src, t.row, t.olo, t.cnt, hi, wi, c, ho, sh, sw);
  upsm_bwd_stage(dy, dyld, dz, t, wo, c);
  __syncthreads();
  for (int q = threadIdx.x; q < t.cnt; q += 256) {
#pragma clang fp contract(off)  // u_k is the rounded product: contracted into u_j - dot, a row with p_j = 1 would not give dz_j = 0
    UpsiRow r;
    r.m = upsm_logits<T, true, CC>(tl.r0, tl.r1, src, tl.wlo, tl.n1, c, t.olo + q, sw, wi, tl.lh0, tl.lh1, r.z);
    upsi_sums<CC>(r, c);
    float* g = dz + q * c;
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < kUpsmMaxC; ++k)
      if (k < c) {  // z[k] <- p_k, e[k] <- u_k
        const float e = r.e[k], a = e == 0.f ? 0.f : (r.ls - r.d(k) - 1.f) * inv_lnc;
        r.z[k] = e * r.iz;
        r.e[k] = g[k] * a;
        dot = fmaf(r.e[k], r.z[k], dot);
      }
#pragma unroll
    for (int k = 0; k < kUpsmMaxC; ++k)
      if (k < c) g[k] = r.z[k] * (r.e[k] - dot);
  }
  upsm_bwd_gather(dz, wt, wlo, tmp, t, wi, c, wo, sw, maxw);
}
// columns of the low-res rows that output columns [ow0, ow1] tap (taps monotone in ow), as the host's
// float arithmetic gives them: the device's own rounding may move either end by one
static int upsm_tap_cols(int wi, float sw, int ow0, int ow1) {
  float src0 = sw * ((float)ow0 + 0.5f) - 0.5f, src1 = sw * ((float)ow1 + 0.5f) - 0.5f;
  int a = src0 < 0.f ? 0 : (int)src0, b = src1 < 0.f ? 0 : (int)src1;
  a = std::min(a, wi - 1);
  b = std::min(b, wi - 1);
  b = b + (b < wi - 1 ? 1 : 0);
  return b - a + 1;
}
// columns of the low-res rows one forward tile stages
static int upsm_fwd_cols(int wi, int wo, float sw) {
  int cols = 0;
  for (int ow0 = 0; ow0 < wo; ow0 += kUpsmPix) cols = std::max(cols, upsm_tap_cols(wi, sw, ow0, std::min(wo, ow0 + kUpsmPix) - 1));
  return cols + 2;  // margin: the device computes the tap columns with its own float rounding
}
// shape guard and sizing of the forward tiles (upsoftmax_fwd / upsoftmax_acc): tiles per row, grid,
// bytes of one tile's staged taps
struct UpsmPlan {
  int tiles;
  unsigned blocks;
  size_t taps;
};
static int upsm_plan(int n, int hi, int wi, int c, int ho, int wo, float sw, UpsmPlan& p) {
  if (n <= 0 || ho <= 0 || wo <= 0 || hi <= 0 || wi <= 0 || c <= 0 || c > kUpsmMaxC) return RTSDS_ERR_SHAPE;
  p.tiles = rt_cdiv(wo, kUpsmPix);
  const long blocks = (long)n * ho * p.tiles;
  if (blocks > INT_MAX) return RTSDS_ERR_UNSUPPORTED;
  p.blocks = (unsigned)blocks;
  p.taps = (size_t)2 * upsm_fwd_cols(wi, wo, sw) * c * sizeof(float);
  return RTSDS_OK;
}
// f(CC): the compile-time class count 19, else 0 (runtime c); f(STAGED, CC) for the forward tiles,
// whose unstaged form has the runtime count only
template <typename F>
static void upsm_with_cc(int c, F f) {
  if (c == 19) f(std::integral_constant<int, 19>());
  else f(std::integral_constant<int, 0>());
}
template <typename F>
static void upsm_dispatch(bool staged, int c, F f) {
  if (staged) upsm_with_cc(c, [&](auto cc) { f(std::true_type(), cc); });
  else f(std::false_type(), std::integral_constant<int, 0>());
}
// rtsds_upsoftmax_fwd and (SI) rtsds_upselfinfo_fwd: one guard, one choice of route, one LDS size
template <bool SI>
static int upsm_fwd_entry(const void* x, void* y, int n, int hi, int wi, int c, int ho, int wo, float scale_h, float scale_w,
                          int y_ld, int dtype, void* stream) {
  if (y_ld < c || y_ld > kUpsmMaxC || (SI && c < 2)) return RTSDS_ERR_SHAPE;  // SI: 1 / ln c
  UpsmPlan p;
  if (const int rc = upsm_plan(n, hi, wi, c, ho, wo, scale_w, p)) return rc;
  const bool staged = p.taps <= (size_t)kUpsmLds;
  const size_t outb = (size_t)kUpsmPix * y_ld * (dtype == RTSDS_BF16 ? 2 : 4);
  const size_t lds = (staged ? p.taps + 16 : 0) + outb;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, upsm_dispatch(staged, c, [&](auto s, auto cc) {
    if constexpr (SI)
      hipLaunchKernelGGL((upselfinfo_fwd_kernel<T, decltype(s)::value, decltype(cc)::value>), dim3(p.blocks), dim3(256), lds, st,
                         (const T*)x, (T*)y, hi, wi, c, ho, wo, scale_h, scale_w, y_ld, p.tiles,
                         (float)(1.0 / std::log((double)c)));
    else
      hipLaunchKernelGGL((upsoftmax_fwd_kernel<T, decltype(s)::value, decltype(cc)::value>), dim3(p.blocks), dim3(256), lds, st,
                         (const T*)x, (T*)y, hi, wi, c, ho, wo, scale_h, scale_w, y_ld, p.tiles);
  }));
  RET_LAUNCH();
}
extern "C" int rtsds_upsoftmax_fwd(const void* x, void* y, int n, int hi, int wi, int c, int ho, int wo, float scale_h,
                                   float scale_w, int y_ld, int dtype, void* stream) {
  return upsm_fwd_entry<false>(x, y, n, hi, wi, c, ho, wo, scale_h, scale_w, y_ld, dtype, stream);
}
extern "C" int rtsds_upselfinfo_fwd(const void* x, void* y, int n, int hi, int wi, int c, int ho, int wo, float scale_h,
                                    float scale_w, int y_ld, int dtype, void* stream) {
  return upsm_fwd_entry<true>(x, y, n, hi, wi, c, ho, wo, scale_h, scale_w, y_ld, dtype, stream);
}
extern "C" int rtsds_upsoftmax_acc(const void* x, float* acc, int64_t* pred, int n, int hi, int wi, int c, int ho, int wo,
                                   float scale_h, float scale_w, int flip, int accumulate, int dtype, void* stream) {
  UpsmPlan p;
  if (const int rc = upsm_plan(n, hi, wi, c, ho, wo, scale_w, p)) return rc;
  if (x == nullptr || acc == nullptr || ((uintptr_t)acc & 3)) return RTSDS_ERR_UNSUPPORTED;
  // the fp32 tile + up to 3 floats of phase behind the (16-B rounded) staged rows
  const size_t tileb = 16 + (size_t)kUpsmPix * c * sizeof(float);
  const bool staged = p.taps + 16 + tileb <= (size_t)64 * 1024;
  const size_t lds = (staged ? p.taps + 16 : 0) + tileb;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, upsm_dispatch(staged, c, [&](auto s, auto cc) {
    hipLaunchKernelGGL((upsoftmax_acc_kernel<T, decltype(s)::value, decltype(cc)::value>), dim3(p.blocks), dim3(256), lds, st,
                       (const T*)x, acc, pred, hi, wi, c, ho, wo, scale_h, scale_w, flip, accumulate, p.tiles);
  }));
  RET_LAUNCH();
}
extern "C" int rtsds_upsample_pseudo(const void* x, uint8_t* pred, uint16_t* cbin, const int* tbin, int64_t* labels, int n, int hi,
                                     int wi, int c, int ho, int wo, float scale_h, float scale_w, int bins, int ignore_index,
                                     int dtype, void* stream) {
  if (c < 2) return RTSDS_ERR_SHAPE;  // (c > 32: upsm_plan)
  if (bins < 16 || bins > 1024 || (bins & (bins - 1))) return RTSDS_ERR_SHAPE;
  UpsmPlan p;
  if (const int rc = upsm_plan(n, hi, wi, c, ho, wo, scale_w, p)) return rc;
  if (x == nullptr || (pred == nullptr && cbin == nullptr && labels == nullptr) || (labels != nullptr && tbin == nullptr) ||
      ((uintptr_t)cbin & 1) || ((uintptr_t)tbin & 3) || ((uintptr_t)labels & 7))
    return RTSDS_ERR_UNSUPPORTED;
  // LDS holds the staged source rows and nothing else (no output tile): staged whenever they fit
  // the 64 KiB a workgroup gets without opting in to more
  const bool staged = p.taps + 16 <= (size_t)64 * 1024;
  const size_t lds = staged ? p.taps + 16 : 0;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, upsm_dispatch(staged, c, [&](auto s, auto cc) {
    hipLaunchKernelGGL((upsample_pseudo_kernel<T, decltype(s)::value, decltype(cc)::value>), dim3(p.blocks), dim3(256), lds, st,
                       (const T*)x, pred, cbin, tbin, labels, hi, wi, c, ho, wo, scale_h, scale_w, bins, ignore_index, p.tiles);
  }));
  RET_LAUNCH();
}
extern "C" int rtsds_upsample_paint(const void* x, const uint8_t* frame, const uint8_t* palette, const uint8_t* lut, uint8_t* ids,
                                    uint8_t* rgb, int n, int hi, int wi, int c, int ho, int wo, float scale_h, float scale_w,
                                    int alpha_q8, int dtype, void* stream) {
  if (c < 2) return RTSDS_ERR_SHAPE;  // (c > 32: upsm_plan)
  if (alpha_q8 < 0 || alpha_q8 > 256) return RTSDS_ERR_SHAPE;
  UpsmPlan p;
  if (const int rc = upsm_plan(n, hi, wi, c, ho, wo, scale_w, p)) return rc;
  if (x == nullptr || (ids == nullptr && rgb == nullptr) || (rgb != nullptr && palette == nullptr) ||
      (rgb != nullptr && alpha_q8 < 256 && frame == nullptr))
    return RTSDS_ERR_UNSUPPORTED;
  // LDS: the staged source rows (whenever they fit the 64 KiB a workgroup gets without opting in to
  // more), then the palette / lut table
  const bool staged = p.taps + 16 + kPaintTab <= (size_t)64 * 1024;
  const size_t lds = (staged ? p.taps + 16 : 0) + kPaintTab;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, upsm_dispatch(staged, c, [&](auto s, auto cc) {
    hipLaunchKernelGGL((upsample_paint_kernel<T, decltype(s)::value, decltype(cc)::value>), dim3(p.blocks), dim3(256), lds, st,
                       (const T*)x, frame, palette, lut, ids, rgb, hi, wi, c, ho, wo, scale_h, scale_w, alpha_q8, p.tiles);
  }));
  RET_LAUNCH();
}
// columns of a head's rows that any run of <= 256 consecutive window columns [a, b] taps: at most
// floor(src(b)) + 1 - floor(src(a)) + 1 <= sw * (b - a) + 3, one more for the device's own float
// rounding; never more than the head has
static int slide_cols(int wi, int ww, float sw) {
  const int run = std::min(ww, kUpsmPix) - 1;
  return (int)std::min((double)wi, std::ceil((double)sw * run) + 4.0);
}
extern "C" int rtsds_slide_paint(const void* x, const int* win, int nwin, const uint8_t* frame, const uint8_t* palette,
                                 const uint8_t* lut, float* acc, uint8_t* ids, uint8_t* rgb, int nf, int hi, int wi, int c, int hw,
                                 int ww, int H, int W, float scale_h, float scale_w, int accumulate, int alpha_q8, int dtype,
                                 void* stream) {
  if (nf < 1 || hi < 1 || wi < 1 || hw < 1 || ww < 1 || H < 1 || W < 1 || nwin < 1 || hw > H || ww > W) return RTSDS_ERR_SHAPE;
  if (c < 2 || c > kUpsmMaxC || alpha_q8 < 0 || alpha_q8 > 256) return RTSDS_ERR_SHAPE;
  if (nwin > kSlideMaxWin || win == nullptr) return RTSDS_ERR_UNSUPPORTED;
  SlideWins wt = {};
  for (int k = 0; k < nwin; ++k) {
    const int y0 = win[3 * k], x0 = win[3 * k + 1];
    if (y0 < 0 || y0 > H - hw || x0 < 0 || x0 > W - ww) return RTSDS_ERR_SHAPE;
    wt.y0[k] = y0;
    wt.x0[k] = x0;
    if (win[3 * k + 2] != 0) wt.flip |= 1ull << k;
  }
  if (dtype != RTSDS_F32 && dtype != RTSDS_BF16) return RTSDS_ERR_UNSUPPORTED;
  if (x == nullptr || (acc == nullptr && ids == nullptr && rgb == nullptr) || (accumulate && acc == nullptr) ||
      (rgb != nullptr && palette == nullptr) || (rgb != nullptr && alpha_q8 < 256 && frame == nullptr) || ((uintptr_t)acc & 3))
    return RTSDS_ERR_UNSUPPORTED;
  const int tiles = rt_cdiv(W, kUpsmPix);
  const long blocks = (long)nf * H * tiles;
  if (blocks > INT_MAX) return RTSDS_ERR_UNSUPPORTED;
  // LDS: the staged rows of one window (while they stay within kUpsmLds and the whole within the
  // 64 KiB a workgroup gets without opting in to more), the palette / lut table, and with acc the
  // fp32 tile + up to 3 floats of phase
  const size_t taps = (size_t)2 * slide_cols(wi, ww, scale_w) * c * sizeof(float);
  const size_t tileb = acc != nullptr ? 16 + (size_t)kUpsmPix * c * sizeof(float) : 0;
  const bool staged = taps <= (size_t)kUpsmLds && taps + 16 + kPaintTab + tileb <= (size_t)64 * 1024;
  const int srcf = staged ? (int)((taps / 4 + 3) & ~(size_t)3) : 0;
  const size_t lds = (size_t)srcf * 4 + kPaintTab + tileb;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, upsm_dispatch(staged, c, [&](auto s, auto cc) {
    hipLaunchKernelGGL((slide_paint_kernel<T, decltype(s)::value, decltype(cc)::value>), dim3((unsigned)blocks), dim3(256), lds, st,
                       (const T*)x, wt, nwin, frame, palette, lut, acc, ids, rgb, nf, hi, wi, c, hw, ww, H, W, scale_h, scale_w,
                       accumulate, alpha_q8, tiles, srcf);
  }));
  RET_LAUNCH();
}
extern "C" size_t rtsds_upsoftmax_bwd_workspace(int n, int hi, int wi, int c, int ho, int wo) {
  return rtsds_bilinear_bwd_workspace(n, hi, wi, c, ho, wo);
}
// tiles of tw input columns: cap = the exact largest segment of output columns any of them reads, cols =
// the most low-res columns any tile's segment taps (upsm_tap_cols + its margin)
static void upsm_tile_span(int wi, int wo, float sw, int tw, int& cap, int& cols) {
  cap = cols = 0;
  for (int iw0 = 0; iw0 < wi; iw0 += tw) {
    int lo, hi;
    bil_adj_range(iw0, std::min(wi, iw0 + tw) - 1, sw, wo, lo, hi);
    cap = std::max(cap, hi - lo + 1);
    cols = std::max(cols, upsm_tap_cols(wi, sw, lo, hi) + 2);
  }
}
// widest tile (64 input columns, narrowed by halves) whose staged segment + weight table fit kUpsmLds;
// cap = its exact largest segment, maxw = the most output columns any input column reads
// extra(tw, cols): what else the kernel keeps in LDS beside a segment of esz-byte elements and the
// table, cols = the most low-res columns any tile's segment taps (upsm_tap_cols + its margin)
template <typename X>
static bool upsm_tiling(int wi, int wo, int c, float sw, size_t esz, int& tw, int& cap, int& maxw, int& cols, X extra) {
  maxw = 0;
  for (int iw = 0; iw < wi; ++iw) {
    int lo, hi;
    bil_adj_range(iw, iw, sw, wo, lo, hi);
    maxw = std::max(maxw, hi - lo + 1);
  }
  for (tw = 64; tw >= 1; tw /= 2) {
    upsm_tile_span(wi, wo, sw, tw, cap, cols);
    if ((size_t)cap * c * esz + (size_t)tw * (maxw + 1) * 4 + extra(tw, cols) <= (size_t)kUpsmLds) return true;
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
    int tw, cap, maxw, cols;
    if (!upsm_tiling(wi, wo, c, scale_w, sizeof(T), tw, cap, maxw, cols, [](int, int) { return (size_t)0; }))
      return RTSDS_ERR_UNSUPPORTED;
    const int tiles = rt_cdiv(wi, tw);
    const long blocks = (long)n * ho * tiles;
    if (blocks > INT_MAX) return RTSDS_ERR_UNSUPPORTED;
    const size_t lds = (size_t)tw * (maxw + 1) * 4 + (size_t)cap * c * sizeof(T);
    upsm_with_cc(c, [&](auto cc) {
      hipLaunchKernelGGL((upsoftmax_bwd_w_kernel<T, decltype(cc)::value>), dim3((unsigned)blocks), dim3(256), lds, st, (const T*)dy,
                         dy_ld, (const T*)y, y_ld, tmp, wi, c, wo, scale_w, tw, tiles, cap, maxw);
    });
    bil_bwd_h_launch(tmp, (T*)dx, n, hi, wi, c, ho, scale_h, st);
  });
  RET_LAUNCH();
}
extern "C" size_t rtsds_upselfinfo_bwd_workspace(int n, int hi, int wi, int c, int ho, int wo) {
  return rtsds_bilinear_bwd_workspace(n, hi, wi, c, ho, wo);
}
// The self-information backward's tile keeps, beside rtsds_upsoftmax_bwd's table, the segment as fp32
// (dy, then dz) and the two staged source rows [2][cols][c] as fp32.  The tile narrows from 64 input
// columns by halves until that fits kUpsmLds; a geometry whose single-column tile does not fit (one
// input column spreading over some 370 output columns at 32 classes) is unsupported.
// The per-pixel recomputation, the kernel's main cost, takes the segment 256 pixels at a pass, so a
// segment just over a multiple of 256 (x8: 8 tw + 12 pixels, 268 at tw = 32) spends a whole pass on a
// few lanes.  upsi_trim narrows the tile further to the widest width whose segment needs one pass
// less, where that lowers the passes per input column (32 -> 30 at x8 and 19 classes: 1 pass per 30
// columns instead of 2 per 32); narrower tiles need no more LDS.
static void upsi_trim(int wi, int wo, float sw, int& tw, int& cap, int& cols) {
  const int passes = rt_cdiv(cap, kUpsmPix);
  if (passes < 2) return;
  for (int t2 = tw - 1; (passes - 1) * tw < passes * t2; --t2) {  // (passes - 1) / t2 < passes / tw
    int cap2, cols2;
    upsm_tile_span(wi, wo, sw, t2, cap2, cols2);
    if (cap2 <= kUpsmPix * (passes - 1) && cols2 <= cols) {
      tw = t2, cap = cap2, cols = cols2;
      return;
    }
  }
}
extern "C" int rtsds_upselfinfo_bwd(const void* dy, int dy_ld, const void* x, void* dx, int n, int hi, int wi, int c, int ho,
                                    int wo, float scale_h, float scale_w, int dtype, void* ws, size_t ws_bytes, void* stream) {
  const long total = (long)n * hi * wi * c;
  if (total <= 0 || ho <= 0 || wo <= 0 || c < 2 || c > kUpsmMaxC || dy_ld < c) return RTSDS_ERR_SHAPE;
  if (ws_bytes < rtsds_upselfinfo_bwd_workspace(n, hi, wi, c, ho, wo)) return RTSDS_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* tmp = (float*)ws;
  const auto rows = [c](int, int cols) { return (size_t)2 * cols * c * sizeof(float); };
  int tw, cap, maxw, cols;
  if (!upsm_tiling(wi, wo, c, scale_w, sizeof(float), tw, cap, maxw, cols, rows)) return RTSDS_ERR_UNSUPPORTED;
  upsi_trim(wi, wo, scale_w, tw, cap, cols);
  const int tiles = rt_cdiv(wi, tw);
  const long blocks = (long)n * ho * tiles;
  if (blocks > INT_MAX) return RTSDS_ERR_UNSUPPORTED;
  const size_t lds = (size_t)tw * (maxw + 1) * 4 + (size_t)cap * c * sizeof(float) + rows(tw, cols);
  DISPATCH_T(dtype, {
    upsm_with_cc(c, [&](auto cc) {
      hipLaunchKernelGGL((upselfinfo_bwd_w_kernel<T, decltype(cc)::value>), dim3((unsigned)blocks), dim3(256), lds, st, (const T*)dy,
                         dy_ld, (const T*)x, tmp, hi, wi, c, ho, wo, scale_h, scale_w, tw, tiles, cap, maxw, 2 * cols * c,
                         (float)(1.0 / std::log((double)c)));
    });
    bil_bwd_h_launch(tmp, (T*)dx, n, hi, wi, c, ho, scale_h, st);
  });
  RET_LAUNCH();
}
