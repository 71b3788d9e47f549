// ClassMix cross-domain mixing for target self-training (gfx950): which classes a window of a
// labelled source map holds (rtsds_class_presence), and the mixture of that window with a target
// batch -- image, label and the thresholded pseudo-label of the pixels that stay target -- in one
// pass (rtsds_classmix).  No reference counterpart (its train.py never trains on target pixels).
// Everything is an integer or a bit copy: results are exact and independent of the launch shape.
// Kept in a unit of its own (not in pseudo.hip), so the generated code of the pseudo-label
// kernels does not depend on this file.
#include "ew_common.h"
#include "class_row.h"

static const int kCmMinC = 2, kCmMaxC = 32;  // one bit per class in a 32-bit mask
// One wave owns one item: kCmChunk consecutive pixels of one window row (64 lanes x 8 pixels).
// A row is the unit at which the alignment of the source window changes (its start moves by ws
// pixels per row and by x0 per sample), so the choice between the vector and the scalar form is
// wave-uniform.  kCmBlocks workgroups of kCmWaves waves = 4 waves per SIMD of the chip; with 14
// 16-B loads per lane in flight that is far more than the bytes HBM needs outstanding.
static const int kCmWaves = 4, kCmChunk = 512, kCmBlocks = 1024;

struct CmGeo {
  int hs, ws, h, w, nchunk;  // source map, window (= target) size, chunks per window row
};
static inline int cm_blocks(const CmGeo& g, int n) {
  return ew_blocks((long)g.h * g.nchunk, kCmWaves, std::max(1, kCmBlocks / n));
}
static inline bool cm_geo_ok(int n, int hs, int ws, int h, int w) {
  return n > 0 && n <= 65535 && h > 0 && w > 0 && hs >= h && ws >= w;
}

// The window origin of sample n.  The origins live in device memory, so the host cannot refuse a
// bad one: it is clamped into the source map here (an in-range origin is unchanged), which keeps
// every access inside the buffers whatever the values are.
RT_DEV void cm_origin(const int* __restrict__ origins, int pitch, int n, const CmGeo& g, int& y0, int& x0) {
  y0 = min(max(origins[(long)n * pitch], 0), g.hs - g.h);
  x0 = min(max(origins[(long)n * pitch + 1], 0), g.ws - g.w);
}
// Wave-uniform split of item `it` into (row y, first column xc, pixels len).
RT_DEV void cm_item(long it, const CmGeo& g, int& y, int& xc, int& len) {
  y = (int)(it / g.nchunk);
  xc = (int)(it - (long)y * g.nchunk) * kCmChunk;
  len = min(kCmChunk, g.w - xc);
}
// A label is a class iff 0 <= s < c (-100, 255, c itself and anything above are not).
RT_DEV bool cm_is_class(long long s, int c) { return (unsigned long long)s < (unsigned long long)c; }
RT_DEV unsigned int cm_bit(long long s, int c) { return cm_is_class(s, c) ? 1u << (int)s : 0u; }

// ------------------------------------------------------------------ presence
// present[n] = OR over the window of 1u << label (classes only).  8 B/pixel read.  Rows whose
// first element is 16-B aligned move as 16-B pairs; an odd row start peels one element first.
// Per-lane OR, xor-shuffle OR over the wave, one LDS word per wave, at most one global atomicOr
// per workgroup (an OR does not depend on the order).  Only window elements are ever loaded.
__global__ void __launch_bounds__(kCmWaves * 64) class_presence_kernel(const int64_t* __restrict__ slab, const int* __restrict__ origins,
                                                                        int opitch, unsigned int* __restrict__ present, CmGeo g, int c,
                                                                        int vec) {
  __shared__ unsigned int part[kCmWaves];
  const int n = blockIdx.y, lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int y0, x0;
  cm_origin(origins, opitch, n, g, y0, x0);
  const long items = (long)g.h * g.nchunk;
  unsigned int bits = 0;
  for (long it = (long)blockIdx.x * kCmWaves + wv; it < items; it += (long)gridDim.x * kCmWaves) {
    int y, xc, len;
    cm_item(it, g, y, xc, len);
    const long e0 = ((long)n * g.hs + y0 + y) * g.ws + x0 + xc;
    const int64_t* row = slab + e0;
    if (vec) {
      const int a = (int)(e0 & 1), np = (len - a) >> 1;  // slab is 16-B aligned: an even index is too
      const longlong2* pr = (const longlong2*)(row + a);
      // four 16-B loads per lane issued before the first use: a whole chunk in one round
      for (int j = lane; j < np; j += 256) {
        longlong2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = j + 64 * u < np ? pr[j + 64 * u] : make_longlong2(-1, -1);
#pragma unroll
        for (int u = 0; u < 4; ++u) bits |= cm_bit(v[u].x, c) | cm_bit(v[u].y, c);
      }
      if (lane == 0 && a) bits |= cm_bit(row[0], c);
      if (lane == 1 && ((len - a) & 1)) bits |= cm_bit(row[len - 1], c);
    } else {
      for (int x = lane; x < len; x += 64) bits |= cm_bit(row[x], c);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits |= (unsigned int)__shfl_xor((int)bits, o, 64);
  if (lane == 0) part[wv] = bits;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int b = 0;
#pragma unroll
    for (int i = 0; i < kCmWaves; ++i) b |= part[i];
    // bits only ever get set, so a (possibly stale) read that already holds this workgroup's bits
    // makes its atomic redundant: after the first few workgroups most skip it
    if (b & ~__hip_atomic_load(&present[n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&present[n], b);
  }
}

extern "C" int rtsds_class_presence(const int64_t* slab, const int* origins, int origin_pitch, unsigned int* present, int n, int hs,
                                    int ws, int h, int w, int c, void* stream) {
  if (!cm_geo_ok(n, hs, ws, h, w) || c < kCmMinC || c > kCmMaxC || origin_pitch < 2) return RTSDS_ERR_SHAPE;
  if (slab == nullptr || origins == nullptr || present == nullptr || ((uintptr_t)slab & 7) || ((uintptr_t)origins & 3) ||
      ((uintptr_t)present & 3))
    return RTSDS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  // the kernel ORs into present: cleared here, on the stream (a memset node under capture)
  if (hipMemsetAsync(present, 0, (size_t)n * sizeof(unsigned int), st) != hipSuccess) return RTSDS_ERR_LAUNCH;
  const CmGeo g = {hs, ws, h, w, (w + kCmChunk - 1) / kCmChunk};
  const int vec = ((uintptr_t)slab & 15) == 0;
  hipLaunchKernelGGL(class_presence_kernel, dim3(cm_blocks(g, n), n), dim3(kCmWaves * 64), 0, st, slab, origins, origin_pitch, present, g,
                     c, vec);
  RET_LAUNCH();
}

// ------------------------------------------------------------------ mix
struct CmArgs {
  const char* src;
  const int64_t* slab;
  const char* tgt;
  const uint8_t* pred;
  const uint16_t* cbin;
  const int* tbin;
  const unsigned int* present;
  const int* perm;
  const int* origins;
  char* out_img;
  int64_t* out_lab;
  uint8_t* mask;
  unsigned int* chosen;
  CmGeo g;
  int ppitch, opitch, c, ignore, vec;
};

// 16 bytes with a stated alignment: <16> is a plain 16-B vector, <8> lets a group of 8-B records
// that starts on an odd record be loaded without claiming an alignment it does not have.
template <int A>
struct __attribute__((aligned(A))) CmV16 {
  unsigned int x, y, z, w;
};

// One pixel record of PIX bytes, copied in the widest unit every record of that size is aligned to.
template <int PIX>
RT_DEV void cm_copy_pixel(char* dst, const char* src) {
  if (PIX == 16) {
    *(uint4*)dst = *(const uint4*)src;
  } else if (PIX == 8) {
    *(uint2*)dst = *(const uint2*)src;
  } else if (PIX == 12) {
#pragma unroll
    for (int i = 0; i < 3; ++i) ((unsigned int*)dst)[i] = ((const unsigned int*)src)[i];
  } else {
#pragma unroll
    for (int i = 0; i < PIX / 2; ++i) ((unsigned short*)dst)[i] = ((const unsigned short*)src)[i];
  }
}

// One pixel: window-relative source element e, target pixel t.
template <int PIX>
RT_DEV void cm_pixel(const CmArgs& a, const int* tb, unsigned int chosen, long e, long t) {
  const long long s = a.slab[e];
  const bool m = cm_is_class(s, a.c) && ((chosen >> (int)(s & 31)) & 1u);
  long long lab = s;
  if (!m) {
    const int k = a.pred[t], b = a.cbin[t];
    lab = pseudo_label(k, b, tb, a.c, a.ignore);
  }
  cm_copy_pixel<PIX>(a.out_img + t * PIX, m ? a.src + e * PIX : a.tgt + t * PIX);
  a.out_lab[t] = lab;
  if (a.mask) a.mask[t] = m ? 1 : 0;
}

// Eight pixels whose target index t is a multiple of 8 (every target-side access is then a whole
// aligned vector: 8 B of pred, 16 B of cbin, PIX / 2 16-B vectors of pixels, 64 B of labels) and
// whose source element e is aligned to SA bytes on both the label and the pixel side.  All loads
// are issued before the first use.  The image is blended per 32-bit word with a mask built from
// the two pixels the word's halves belong to: records of 6 and 12 bytes straddle the vectors.
template <int PIX, int SA>
RT_DEV void cm_group(const CmArgs& a, const int* tb, unsigned int chosen, long e, long t) {
  constexpr int NV = PIX / 2, NW = 4 * NV;
  typedef CmV16<SA> SV;
  typedef CmV16<16> TV;
  const SV* lp = (const SV*)(a.slab + e);
  const SV* sp = (const SV*)(a.src + e * PIX);
  const TV* tp = (const TV*)(a.tgt + t * PIX);
  SV lv[4], sv[NV];
  TV tv[NV];
#pragma unroll
  for (int j = 0; j < 4; ++j) lv[j] = lp[j];
#pragma unroll
  for (int j = 0; j < NV; ++j) sv[j] = sp[j];
#pragma unroll
  for (int j = 0; j < NV; ++j) tv[j] = tp[j];
  const uint2 pv = *(const uint2*)(a.pred + t);
  const uint4 cv = *(const uint4*)(a.cbin + t);
  const unsigned int pw[2] = {pv.x, pv.y}, cw[4] = {cv.x, cv.y, cv.z, cv.w};
  unsigned int lw[16], sw[NW], tw[NW];
#pragma unroll
  for (int j = 0; j < 4; ++j) { lw[4 * j] = lv[j].x; lw[4 * j + 1] = lv[j].y; lw[4 * j + 2] = lv[j].z; lw[4 * j + 3] = lv[j].w; }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    sw[4 * j] = sv[j].x; sw[4 * j + 1] = sv[j].y; sw[4 * j + 2] = sv[j].z; sw[4 * j + 3] = sv[j].w;
    tw[4 * j] = tv[j].x; tw[4 * j + 1] = tv[j].y; tw[4 * j + 2] = tv[j].z; tw[4 * j + 3] = tv[j].w;
  }
  bool m[8];
  long long o[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const unsigned int lo = lw[2 * p], hi = lw[2 * p + 1];
    m[p] = hi == 0 && lo < (unsigned int)a.c && ((chosen >> (lo & 31)) & 1u);
    const int k = (int)((pw[p >> 2] >> (8 * (p & 3))) & 0xffu);
    const int b = (int)((cw[p >> 1] >> (16 * (p & 1))) & 0xffffu);
    const long long pl = pseudo_label(k, b, tb, a.c, a.ignore);
    o[p] = m[p] ? (long long)lo : pl;
  }
  longlong2* ol = (longlong2*)(a.out_lab + t);
#pragma unroll
  for (int j = 0; j < 4; ++j) ol[j] = make_longlong2(o[2 * j], o[2 * j + 1]);
  TV* op = (TV*)(a.out_img + t * PIX);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    unsigned int ow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int wd = 4 * j + i;
      const unsigned int sel = (m[(4 * wd) / PIX] ? 0x0000ffffu : 0u) | (m[(4 * wd + 2) / PIX] ? 0xffff0000u : 0u);
      ow[i] = (sw[wd] & sel) | (tw[wd] & ~sel);
    }
    TV v;
    v.x = ow[0]; v.y = ow[1]; v.z = ow[2]; v.w = ow[3];
    op[j] = v;
  }
  if (a.mask) {
    unsigned int mw[2] = {0, 0};
#pragma unroll
    for (int p = 0; p < 8; ++p) mw[p >> 2] |= (m[p] ? 1u : 0u) << (8 * (p & 3));
    *(uint2*)(a.mask + t) = make_uint2(mw[0], mw[1]);
  }
}

// Grid: (workgroups per sample, samples).  Prologue: perm[n, :], tbin and present[n] -> chosen[n]
// (class k of the present set P is chosen iff fewer than (|P| + 1) >> 1 members of P come before
// it in the order (perm, class index)): a 32 x 32 rank count by the first wave, collected with
// one ballot.  Body: one wave per item, see kCmChunk.  Per row the wave takes
//   - cm_group<PIX, 16> when the target row start is a multiple of 8 pixels and the source row
//     start is a multiple of kSrcPix pixels (8 for 6-B records, 4 for 12-B, 2 for 8- and 16-B),
//   - cm_group<PIX, 8> for 8- and 16-B records on any other source start (the target side stays
//     on whole vectors; a random x0 is odd half of the time),
//   - cm_pixel, one pixel per lane, otherwise and for the last w % 8 pixels of a row.
template <int PIX>
__global__ void __launch_bounds__(kCmWaves * 64) classmix_kernel(CmArgs a) {
  __shared__ int sperm[kCmMaxC], tb[kCmMaxC];
  __shared__ unsigned int sch;
  constexpr int kSrcPix = PIX == 6 ? 8 : PIX == 12 ? 4 : 2;
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const CmGeo g = a.g;
  const int c = a.c;
  if (tid < c) {
    sperm[tid] = a.perm[(long)n * a.ppitch + tid];
    tb[tid] = a.tbin[tid];
  }
  __syncthreads();
  if (tid < 64) {
    const unsigned int P = a.present[n] & (c == 32 ? 0xffffffffu : (1u << c) - 1u);
    bool sel = false;
    if (tid < c && ((P >> tid) & 1u)) {
      const int quota = (__popc(P) + 1) >> 1, pk = sperm[tid];
      int rank = 0;
      for (int j = 0; j < c; ++j) {
        const int pj = sperm[j];
        rank += (int)(((P >> j) & 1u) && (pj < pk || (pj == pk && j < tid)));
      }
      sel = rank < quota;
    }
    const unsigned long long b = __ballot(sel);
    if (tid == 0) {
      sch = (unsigned int)b;
      if (a.chosen && blockIdx.x == 0) a.chosen[n] = (unsigned int)b;
    }
  }
  __syncthreads();
  const unsigned int chosen = sch;
  int y0, x0;
  cm_origin(a.origins, a.opitch, n, g, y0, x0);
  const long items = (long)g.h * g.nchunk;
  for (long it = (long)blockIdx.x * kCmWaves + wv; it < items; it += (long)gridDim.x * kCmWaves) {
    int y, xc, len;
    cm_item(it, g, y, xc, len);
    const long e0 = ((long)n * g.hs + y0 + y) * g.ws + x0 + xc;  // source element of the item's first pixel
    const long t0 = ((long)n * g.h + y) * g.w + xc;              // its target pixel
    int done = 0;
    if (a.vec && (t0 & 7) == 0) {
      const int ng = len >> 3;
      if ((e0 & (kSrcPix - 1)) == 0) {
        for (int j = lane; j < ng; j += 64) cm_group<PIX, 16>(a, tb, chosen, e0 + 8 * j, t0 + 8 * j);
        done = ng << 3;
      } else if constexpr (PIX % 8 == 0) {
        for (int j = lane; j < ng; j += 64) cm_group<PIX, 8>(a, tb, chosen, e0 + 8 * j, t0 + 8 * j);
        done = ng << 3;
      }
    }
    for (int x = done + lane; x < len; x += 64) cm_pixel<PIX>(a, tb, chosen, e0 + x, t0 + x);
  }
}

static inline uintptr_t cm_pix_align(int pix) { return pix == 6 ? 1 : pix == 12 ? 3 : pix == 8 ? 7 : 15; }

extern "C" int rtsds_classmix(const void* src, const int64_t* slab, const void* tgt, const uint8_t* pred, const uint16_t* cbin,
                              const int* tbin, const unsigned int* present, const int* perm, int perm_pitch, const int* origins,
                              int origin_pitch, void* out_img, int64_t* out_lab, uint8_t* mask, unsigned int* chosen, int n, int hs,
                              int ws, int h, int w, int c, int pix_bytes, int ignore_index, void* stream) {
  if (!cm_geo_ok(n, hs, ws, h, w) || c < kCmMinC || c > kCmMaxC || perm_pitch < c || origin_pitch < 2) return RTSDS_ERR_SHAPE;
  if (pix_bytes != 6 && pix_bytes != 8 && pix_bytes != 12 && pix_bytes != 16) return RTSDS_ERR_UNSUPPORTED;
  if (src == nullptr || slab == nullptr || tgt == nullptr || pred == nullptr || cbin == nullptr || tbin == nullptr ||
      present == nullptr || perm == nullptr || origins == nullptr || out_img == nullptr || out_lab == nullptr)
    return RTSDS_ERR_UNSUPPORTED;
  const uintptr_t pa = cm_pix_align(pix_bytes);
  const uintptr_t img = (uintptr_t)src | (uintptr_t)tgt | (uintptr_t)out_img;
  const uintptr_t i32 = (uintptr_t)tbin | (uintptr_t)present | (uintptr_t)perm | (uintptr_t)origins | (uintptr_t)chosen;
  if ((img & pa) || (((uintptr_t)slab | (uintptr_t)out_lab) & 7) || ((uintptr_t)cbin & 1) || (i32 & 3)) return RTSDS_ERR_UNSUPPORTED;
  CmArgs a;
  a.src = (const char*)src; a.slab = slab; a.tgt = (const char*)tgt; a.pred = pred; a.cbin = cbin; a.tbin = tbin;
  a.present = present; a.perm = perm; a.origins = origins; a.out_img = (char*)out_img; a.out_lab = out_lab; a.mask = mask;
  a.chosen = chosen;
  a.g = CmGeo{hs, ws, h, w, (w + kCmChunk - 1) / kCmChunk};
  a.ppitch = perm_pitch; a.opitch = origin_pitch; a.c = c; a.ignore = ignore_index;
  a.vec = ((img | (uintptr_t)slab | (uintptr_t)out_lab | (uintptr_t)cbin) & 15) == 0 && (((uintptr_t)pred | (uintptr_t)mask) & 7) == 0;
  const dim3 grid(cm_blocks(a.g, n), n), block(kCmWaves * 64);
  hipStream_t st = (hipStream_t)stream;
  switch (pix_bytes) {
    case 6: hipLaunchKernelGGL(classmix_kernel<6>, grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL(classmix_kernel<8>, grid, block, 0, st, a); break;
    case 12: hipLaunchKernelGGL(classmix_kernel<12>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(classmix_kernel<16>, grid, block, 0, st, a); break;
  }
  RET_LAUNCH();
}
