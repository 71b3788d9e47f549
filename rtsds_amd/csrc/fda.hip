// Fourier Domain Adaptation (Yang & Soatto, CVPR 2020) of a decoded uint8 HWC RGB image (gfx950):
// the low-frequency amplitude of the source's 2-D spectrum is replaced by a target image's, the
// phase is kept.  No reference counterpart (its pipeline trains on GTA5 frames as they are).
// Only the (2b+1)^2 coefficients of the band |u|, |v| <= b change, so no full-frame FFT is made:
//   out(y,x) = src(y,x) + 1/(hw) * sum_{(u,v) in band} D(u,v) e^{2 pi i (uy/h + vx/w)}
//   D = strength * (A_t - A_s) * F_s / A_s        A_s = |F_s|; D = strength * A_t where A_s == 0
// rtsds_fda_spectrum forms the band of F_s (a band-limited DFT, O(hw b)) and |F| / (hw);
// rtsds_fda_apply adds the correction.  Band layout everywhere: [ch][iu = u + b][v = 0..b] (re, im);
// the half v < 0 follows from F(-u,-v) = conj F(u,v).
//
// Twiddles: the phase is reduced in integers first (k = |u| y mod h <= 2^30 in 32 bits, likewise
// v x mod w), folded to (-n/2, n/2], and only then goes to sincospif(2k/n): the argument never
// grows with u y.  The twiddles over x, which every row needs again, come from a table of the w
// values e^{2 pi i k / w} that each block fills once in LDS (w <= kFdaTable; else each is formed
// where it is used, with the same bits).  All sums run in a fixed order (lane-strided, then a butterfly over the wave):
// no floating-point atomics, two runs give the same bits.  Every multiply-add is written as fmaf
// and the compiler forms none of its own (fp contract off), so the dword and the byte path, the
// table and the in-place twiddles, and the measurement variants all give the same bits.
#include "ew_common.h"

#pragma clang fp contract(off)

static const int kFdaMaxB = 64;
static const int kFdaPx = 4;                  // consecutive pixels (12 bytes) per lane and step
static const int kFdaRows = 4;                // rows of an apply tile
// FDA_TABLE: the widest image whose x twiddles are tabled in LDS (8 bytes each); 0 builds the
// variant without the table that DESIGN.md compares.
#ifndef FDA_TABLE
#define FDA_TABLE 4096
#endif
static const int kFdaTable = FDA_TABLE;
// Capped grids of 256-thread blocks (4 waves, one work item per wave and pass).
#ifndef FDA_SPEC_BLOCKS
#define FDA_SPEC_BLOCKS 1024
#endif
// FDA_G_KERNEL = 1 builds the variant DESIGN.md compares (tools/bench_fda.py): G by a kernel in
// front, through a static device buffer of FDA_G_ROWS rows, instead of in every block's prologue.
#ifndef FDA_G_KERNEL
#define FDA_G_KERNEL 0
#endif
#ifndef FDA_G_ROWS
#define FDA_G_ROWS 1024
#endif

// e^{2 pi i k / n} for 0 <= k < n <= 2^24: (cos, sin)
RT_DEV float2 fda_twiddle(int k, int n) {
  if (2 * k > n) k -= n;
  float s, c;
  sincospif((float)(2 * k) / (float)n, &s, &c);
  return make_float2(c, s);
}

// The 12 bytes of pixels x .. x + 3 of a row (x % 4 == 0) as three dwords, little endian.  VEC: the
// row and x * 3 are 4-B aligned and the four pixels exist; else byte loads of the nvalid pixels.
template <bool VEC>
RT_DEV void fda_load_px(const uint8_t* row, int x, int nvalid, unsigned int (&d)[3]) {
  if constexpr (VEC) {
    const unsigned int* p = (const unsigned int*)(row + 3 * (long)x);
    d[0] = p[0], d[1] = p[1], d[2] = p[2];
  } else {
    d[0] = d[1] = d[2] = 0;
    for (int j = 0; j < 3 * nvalid; ++j) d[j >> 2] |= (unsigned int)row[3 * (long)x + j] << (8 * (j & 3));
  }
}
// TAB: tab[k] = fda_twiddle(k, w) for k < w, by the block's 256 threads; ends with a barrier.
template <bool TAB>
RT_DEV void fda_fill_table(float2* tab, int w) {
  if constexpr (TAB) {
    for (int k = threadIdx.x; k < w; k += 256) tab[k] = fda_twiddle(k, w);
    __syncthreads();
  }
}
template <bool TAB>
RT_DEV float2 fda_twiddle_x(const float2* tab, int k, int w) {
  if constexpr (TAB) return tab[k];
  else return fda_twiddle(k, w);
}
RT_DEV float fda_byte(const unsigned int (&d)[3], int j) { return (float)((d[j >> 2] >> (8 * (j & 3))) & 255u); }

// ------------------------------------------------------------------ spectrum
// Stage 1: part[y][ch][v] = sum_x img[y][x][ch] e^{-2 pi i v x / w}.  One wave per (y, v): lane l
// takes the pixel groups l, l + 64, ...; the four waves of a block share a row.
template <bool VEC, bool TAB>
__global__ void __launch_bounds__(256) fda_rows_kernel(const uint8_t* __restrict__ img, int h, int w, int b, float2* __restrict__ part) {
  __shared__ float2 tab[TAB && kFdaTable > 0 ? kFdaTable : 1];
  fda_fill_table<TAB>(tab, w);
  const int lane = threadIdx.x & 63, nb1 = b + 1;
  const int ngroups = (w + kFdaPx - 1) / kFdaPx;
  const long items = (long)h * nb1, nwaves = (long)gridDim.x * 4;
  for (long it = (long)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += nwaves) {
    const int y = (int)(it / nb1), v = (int)(it - (long)y * nb1);
    const uint8_t* row = img + (long)y * w * 3;
    float re[3] = {0.f, 0.f, 0.f}, im[3] = {0.f, 0.f, 0.f};
    for (int g = lane; g < ngroups; g += 64) {
      const int x = kFdaPx * g, nvalid = min(kFdaPx, w - x);
      unsigned int d[3];
      fda_load_px<VEC>(row, x, nvalid, d);
      int k = (int)((unsigned int)(v * x) % (unsigned int)w);
#pragma unroll
      for (int i = 0; i < kFdaPx; ++i) {
        if (i < nvalid) {
          const float2 t = fda_twiddle_x<TAB>(tab, k, w);
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const float p = fda_byte(d, 3 * i + ch);
            re[ch] = fmaf(p, t.x, re[ch]);
            im[ch] = fmaf(-p, t.y, im[ch]);
          }
        }
        k += v;
        if (k >= w) k -= w;
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float sr = wave_sum(re[ch]), si = wave_sum(im[ch]);
      if (lane == 0) part[((long)y * 3 + ch) * nb1 + v] = make_float2(sr, si);
    }
  }
}

// Stage 2: F(u,v) = sum_y part[y][ch][v] e^{-2 pi i u y / h}, one wave per coefficient.
__global__ void __launch_bounds__(256) fda_cols_kernel(const float2* __restrict__ part, int h, int w, int b, float* __restrict__ spec,
                                                       float* __restrict__ amp_norm) {
  const int lane = threadIdx.x & 63, nb1 = b + 1, nu = 2 * b + 1;
  const int total = 3 * nu * nb1, nwaves = gridDim.x * 4;
  const float hw = (float)(h * w);
  for (int o = blockIdx.x * 4 + (threadIdx.x >> 6); o < total; o += nwaves) {
    const int v = o % nb1, iu = (o / nb1) % nu, ch = o / (nb1 * nu);
    const int au = abs(iu - b);
    float re = 0.f, im = 0.f;
    for (int y = lane; y < h; y += 64) {
      float2 t = fda_twiddle((int)((unsigned int)(au * y) % (unsigned int)h), h);
      if (iu >= b) t.y = -t.y;  // e^{-2 pi i u y / h}: the conjugate for u >= 0
      const float2 p = part[((long)y * 3 + ch) * nb1 + v];
      re = fmaf(p.x, t.x, re);
      re = fmaf(-p.y, t.y, re);
      im = fmaf(p.x, t.y, im);
      im = fmaf(p.y, t.x, im);
    }
    re = wave_sum(re);
    im = wave_sum(im);
    if (lane == 0) {
      if (spec) spec[2 * o] = re, spec[2 * o + 1] = im;
      if (amp_norm) amp_norm[o] = sqrtf(fmaf(re, re, im * im)) / hw;
    }
  }
}

static bool fda_bad_shape(int c, int h, int w, int b) {
  return c <= 0 || h <= 0 || w <= 0 || b < 1 || b > kFdaMaxB || 2 * b + 1 > std::min(h, w) ||
         (unsigned long long)h * (unsigned long long)w > (1ull << 24);
}
// the dword path: every row starts 4-B aligned and holds whole groups of four pixels
static bool fda_vec(const void* base, int w) { return ((uintptr_t)base & 15) == 0 && w % kFdaPx == 0; }

extern "C" size_t rtsds_fda_workspace(int h, int w, int b) {
  if (fda_bad_shape(3, h, w, b)) return 0;
  return (size_t)h * 3 * (b + 1) * sizeof(float2);
}

extern "C" int rtsds_fda_spectrum(const uint8_t* img, int c, int h, int w, int b, float* spec, float* amp_norm, void* ws, size_t ws_bytes,
                                  void* stream) {
  if (!img || (!spec && !amp_norm) || fda_bad_shape(c, h, w, b)) return RTSDS_ERR_SHAPE;
  if (c != 3 || ((uintptr_t)spec & 3) || ((uintptr_t)amp_norm & 3)) return RTSDS_ERR_UNSUPPORTED;
  if (!ws || ((uintptr_t)ws & 7) || ws_bytes < rtsds_fda_workspace(h, w, b)) return RTSDS_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float2* part = (float2*)ws;
  const int blocks = ew_blocks((long)h * (b + 1), 4, FDA_SPEC_BLOCKS);
  with_bool(fda_vec(img, w), [&](auto v) {
    with_bool(w <= kFdaTable, [&](auto t) {
      hipLaunchKernelGGL((fda_rows_kernel<decltype(v)::value, decltype(t)::value>), dim3(blocks), dim3(256), 0, st, img, h, w, b, part);
    });
  });
  RT_CHECK_LAUNCH();
  hipLaunchKernelGGL(fda_cols_kernel, dim3(ew_blocks(3L * (2 * b + 1) * (b + 1), 4, FDA_SPEC_BLOCKS)), dim3(256), 0, st, (const float2*)part, h,
                     w, b, spec, amp_norm);
  RET_LAUNCH();
}

// ------------------------------------------------------------------ apply
// A block takes a tile of kFdaRows rows x at most 1024 columns (the groups of four pixels of a
// row are spread evenly over the tiles of columns); thread t the four pixels x0 + 4 t .. + 3 of
// each row.  Prologue, per block, in LDS:
//   ty[r][iu]    = e^{2 pi i u y / h} for the tile's rows
//   g[v][r][ch]  = G(y,v) * (v == 0 ? 1 : 2) / (hw),  G(y,v) = sum_u D(u,v) e^{2 pi i u y / h};
//                  D is formed from the two spectra as it is used (at b = 64 it would not fit)
// then out = src + g[0].re + sum_{v >= 1} Re(g[v] e^{2 pi i v x / w}): one twiddle per (x, v) serves
// the tile's rows and channels; g is read as a broadcast.  A thread reads its own 12 source
// bytes of a row before it stores them, and no byte belongs to two threads: dst may be src.
struct FdaLds {
  float2 ty[kFdaRows * (2 * kFdaMaxB + 1)];
  __attribute__((aligned(16))) float2 g[(kFdaMaxB + 1) * kFdaRows * 3];
};
// ty and g of the tile rows y0 .. y0 + kFdaRows - 1 (rows past the image repeat the last one), by
// the 256 threads of a block; ends with a barrier.
RT_DEV void fda_form_g(int y0, int h, int w, int b, const float* __restrict__ spec, const float* __restrict__ amp_ref, float strength,
                       FdaLds& s) {
  float2* ty = s.ty;
  float2* g = s.g;
  const int tid = threadIdx.x, nb1 = b + 1, nu = 2 * b + 1;
  const float hw = (float)(h * w);
  for (int i = tid; i < kFdaRows * nu; i += 256) {
    const int r = i / nu, iu = i - r * nu, au = abs(iu - b);
    const int y = min(y0 + r, h - 1);
    float2 t = fda_twiddle((int)((unsigned int)(au * y) % (unsigned int)h), h);
    if (iu < b) t.y = -t.y;
    ty[i] = t;
  }
  __syncthreads();
  for (int i = tid; i < kFdaRows * 3 * nb1; i += 256) {
    const int v = i % nb1, ch = (i / nb1) % 3, r = i / (3 * nb1);
    const float2* tr = ty + r * nu;
    float gr = 0.f, gi = 0.f;
    for (int iu = 0; iu < nu; ++iu) {
      const int o = (ch * nu + iu) * nb1 + v;
      const float fr = spec[2 * o], fi = spec[2 * o + 1];
      const float at = amp_ref[o] * hw, as = sqrtf(fmaf(fr, fr, fi * fi));
      float dr = strength * at, di = 0.f;  // A_s == 0: the phase of 0 is 0
      if (as != 0.f) {
        const float q = strength * (at - as) / as;
        dr = q * fr, di = q * fi;
      }
      const float2 t = tr[iu];
      gr = fmaf(dr, t.x, gr);
      gr = fmaf(-di, t.y, gr);
      gi = fmaf(dr, t.y, gi);
      gi = fmaf(di, t.x, gi);
    }
    const float scale = (v == 0 ? 1.f : 2.f) / hw;
    g[(v * kFdaRows + r) * 3 + ch] = make_float2(gr * scale, gi * scale);
  }
  __syncthreads();
}

// G_IN (the measurement variant): g_in[tile_y][v][r][ch], written by fda_g_kernel, is copied to LDS.
template <bool VEC, bool U8, bool TAB, bool G_IN>
__global__ void __launch_bounds__(256) fda_apply_kernel(const uint8_t* src, void* dst, int h, int w, int b, const float* __restrict__ spec,
                                                        const float* __restrict__ amp_ref, float strength, int tiles_x, int tile_groups,
                                                        const float2* __restrict__ g_in) {
  __shared__ FdaLds s;
  __shared__ float2 tab[TAB && kFdaTable > 0 ? kFdaTable : 1];
  const float2* g = s.g;
  const int tid = threadIdx.x;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int y0 = tile_y * kFdaRows, x = kFdaPx * (tile_x * tile_groups + tid);
  if constexpr (TAB)  // no barrier of its own: the prologue below ends with one
    for (int k = tid; k < w; k += 256) tab[k] = fda_twiddle(k, w);
  if constexpr (G_IN) {
    const int n = (b + 1) * kFdaRows * 3;
    for (int i = tid; i < n; i += 256) s.g[i] = g_in[(long)tile_y * n + i];
    __syncthreads();
  } else {
    fda_form_g(y0, h, w, b, spec, amp_ref, strength, s);
  }
  if (tid >= tile_groups || x >= w) return;
  const int nvalid = min(kFdaPx, w - x);
  float acc[kFdaPx][kFdaRows][3];
#pragma unroll
  for (int r = 0; r < kFdaRows; ++r)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float g0 = g[r * 3 + ch].x;
#pragma unroll
      for (int i = 0; i < kFdaPx; ++i) acc[i][r][ch] = g0;
    }
  int k[kFdaPx];
#pragma unroll
  for (int i = 0; i < kFdaPx; ++i) k[i] = 0;
  for (int v = 1; v <= b; ++v) {
    float2 t[kFdaPx];
#pragma unroll
    for (int i = 0; i < kFdaPx; ++i) {
      k[i] += min(x + i, w - 1);  // (v x) mod w; columns past the edge repeat the last one, unused
      if (k[i] >= w) k[i] -= w;
      t[i] = fda_twiddle_x<TAB>(tab, k[i], w);
    }
    const float2* gv = g + v * kFdaRows * 3;
#pragma unroll
    for (int r = 0; r < kFdaRows; ++r)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float2 gg = gv[r * 3 + ch];
#pragma unroll
        for (int i = 0; i < kFdaPx; ++i) {
          acc[i][r][ch] = fmaf(gg.x, t[i].x, acc[i][r][ch]);
          acc[i][r][ch] = fmaf(-gg.y, t[i].y, acc[i][r][ch]);
        }
      }
  }
  unsigned int d[kFdaRows][3];  // the thread's source bytes of all its rows, read before any is stored
#pragma unroll
  for (int r = 0; r < kFdaRows; ++r) fda_load_px<VEC>(src + (long)min(y0 + r, h - 1) * w * 3, x, nvalid, d[r]);
#pragma unroll
  for (int r = 0; r < kFdaRows; ++r) {
    const int y = y0 + r;
    if (y >= h) break;
    const long px = (long)y * w + x;
    float o[3 * kFdaPx];
#pragma unroll
    for (int i = 0; i < kFdaPx; ++i)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float val = fda_byte(d[r], 3 * i + ch) + acc[i][r][ch];
        if constexpr (U8) val = rintf(val);
        o[3 * i + ch] = fminf(fmaxf(val, 0.f), 255.f);
      }
    if constexpr (U8) {
      uint8_t* out = (uint8_t*)dst + 3 * px;
      if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
          ((unsigned int*)out)[q] = (unsigned int)o[4 * q] | (unsigned int)o[4 * q + 1] << 8 | (unsigned int)o[4 * q + 2] << 16 |
                                    (unsigned int)o[4 * q + 3] << 24;
      } else {
#pragma unroll
        for (int j = 0; j < 3 * kFdaPx; ++j)
          if (j < 3 * nvalid) out[j] = (uint8_t)o[j];
      }
    } else {
      float* out = (float*)dst + 3 * px;
      if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < 3; ++q) ((f32x4*)out)[q] = f32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
      } else {
#pragma unroll
        for (int j = 0; j < 3 * kFdaPx; ++j)
          if (j < 3 * nvalid) out[j] = o[j];
      }
    }
  }
}

#if FDA_G_KERNEL
__device__ float2 fda_g_rows[(size_t)FDA_G_ROWS * 3 * (kFdaMaxB + 1)];
__global__ void __launch_bounds__(256) fda_g_kernel(int h, int w, int b, const float* __restrict__ spec, const float* __restrict__ amp_ref,
                                                    float strength, float2* __restrict__ g_out) {
  __shared__ FdaLds s;
  fda_form_g(blockIdx.x * kFdaRows, h, w, b, spec, amp_ref, strength, s);
  const int n = (b + 1) * kFdaRows * 3;
  for (int i = threadIdx.x; i < n; i += 256) g_out[(long)blockIdx.x * n + i] = s.g[i];
}
#endif

extern "C" int rtsds_fda_apply(const uint8_t* src, void* dst, int dst_u8, int c, int h, int w, int b, const float* spec_src,
                               const float* amp_ref_norm, float strength, void* stream) {
  if (!src || !dst || !spec_src || !amp_ref_norm || fda_bad_shape(c, h, w, b) || !(strength >= 0.f && strength <= 1.f))
    return RTSDS_ERR_SHAPE;
  if (c != 3 || ((uintptr_t)spec_src & 3) || ((uintptr_t)amp_ref_norm & 3) || (!dst_u8 && ((uintptr_t)dst & 3))) return RTSDS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int groups = rt_cdiv(w, kFdaPx), tiles_x = rt_cdiv(groups, 256), tile_groups = rt_cdiv(groups, tiles_x);
  const int blocks = tiles_x * rt_cdiv(h, kFdaRows);
  const bool vec = fda_vec(src, w) && ((uintptr_t)dst & 15) == 0;
  const float2* g_in = nullptr;
#if FDA_G_KERNEL
  if (rt_cdiv(h, kFdaRows) * kFdaRows > FDA_G_ROWS) return RTSDS_ERR_UNSUPPORTED;
  float2* g_rows = nullptr;
  if (hipGetSymbolAddress((void**)&g_rows, HIP_SYMBOL(fda_g_rows)) != hipSuccess) return RTSDS_ERR_LAUNCH;
  hipLaunchKernelGGL(fda_g_kernel, dim3(rt_cdiv(h, kFdaRows)), dim3(256), 0, st, h, w, b, spec_src, amp_ref_norm, strength, g_rows);
  g_in = g_rows;
#endif
  with_bool(vec, [&](auto v) {
    with_bool(dst_u8 != 0, [&](auto u) {
      with_bool(w <= kFdaTable, [&](auto t) {
        hipLaunchKernelGGL((fda_apply_kernel<decltype(v)::value, decltype(u)::value, decltype(t)::value, FDA_G_KERNEL != 0>), dim3(blocks),
                           dim3(256), 0, st, src, dst, h, w, b, spec_src, amp_ref_norm, strength, tiles_x, tile_groups, g_in);
      });
    });
  });
  RET_LAUNCH();
}
