// Class-balanced pseudo-labels for target self-training (gfx950): the per-class confidence
// histogram of a summed-probability map (rtsds_conf_hist) and the thresholded label map
// (rtsds_pseudo_select).  No reference counterpart (its train.py never trains on target pixels).
// The per-pixel rules (first maximum, confidence bin, thresholded label) are class_row.h's, shared
// with chan.hip, resize.hip and classmix.hip.
#include "ew_common.h"
#include "class_row.h"

static const int kPlMinC = 2, kPlMaxC = 32;         // uint8 pred, one LDS row of thresholds
static const int kPlMinBins = 16, kPlMaxBins = 1024;  // uint16 cbin; a power of two
// LDS budget of rtsds_conf_hist: one workgroup may use the CU's whole 160 KiB, and next to the
// c * bins privatised counters it must still stage a tile of at least kPlMinTile pixels (8 waves:
// fewer cannot keep enough 16-B loads in flight for a streaming read).  c * (bins + 512) * 4 <=
// 160 KiB: every bins at c <= 26, bins <= 512 up to c = 32.
static const size_t kPlLds = 160 * 1024;
static const int kPlMinTile = 512, kPlMaxTile = 1024;

static inline bool pl_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
static inline size_t pl_lds_bytes(int tile, int c, int bins) { return ((size_t)tile * c + (size_t)c * bins) * 4; }

// ------------------------------------------------------------------ confidence histogram
// acc: total pixels x c fp32 (the sum upsoftmax_acc_kernel leaves).  Per pixel k = first_max()
// class, conf = acc[k] * inv, b = conf_bin(conf, bins); hist[k * bins + b] += 1, pred[p] = k,
// cbin[p] = b.  bins is a power of two, so conf * bins is exact and the bin is the one the host
// computes from the same two fp32 multiplies.
//
// One workgroup = TILE threads: a tile of TILE pixel rows (TILE * c contiguous floats, not 16-B
// aligned per pixel) is staged through LDS with 16-B loads, one thread then owns one pixel.  The
// histogram is privatised per workgroup in LDS (32-bit counters, integer atomics) and flushed
// once at the end, one 64-bit global atomic per non-zero cell: integer counts, so the result
// does not depend on the order.
//
// Contention: predictions are spatially coherent and confident, so most lanes of a wave hit the
// same (class, top bin) cell and same-address LDS atomics serialise.  Each wave therefore peels
// its two most likely keys first -- the key of its first pending lane, twice: the lanes holding
// it are found with one ballot and ONE lane adds their count -- and only the lanes left over add
// 1 each.  A one-class wave issues a single LDS atomic; a wave of 64 different keys pays two
// ballots and then behaves like the plain per-lane add.  (Per-wave histogram copies were not an
// option: c * bins counters are 76 KiB at 19 x 1024, one copy is all the LDS holds.)
//
// conf_hist_tile: one tile out of LDS, thread tid owns pixel p0 + tid.
template <int TILE>
RT_DEV void conf_hist_tile(const float* buf, unsigned int* lh, uint8_t* __restrict__ pred, uint16_t* __restrict__ cbin, long p0, int np,
                           int c, int bins, float inv) {
  const int tid = threadIdx.x, lane = tid & 63;
  const bool valid = tid < np;
  int key = 0;
  if (valid) {
    float best;
    const int bi = first_max(dense_row(buf + tid * c), c, best);
    const int b = conf_bin(best * inv, bins);
    key = bi * bins + b;
    const long p = p0 + tid;
    if (pred) pred[p] = (uint8_t)bi;
    if (cbin) cbin[p] = (uint16_t)b;
  }
  // wave-uniform control flow from here: every lane takes part in the ballots
  bool pending = valid;
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const unsigned long long act = __ballot(pending);
    if (act == 0) break;
    const int lead = __ffsll((long long)act) - 1;
    const int lkey = __shfl(key, lead, 64);
    const bool same = pending && key == lkey;
    const unsigned long long m = __ballot(same);
    if (lane == lead) atomicAdd(&lh[lkey], (unsigned int)__popcll(m));
    pending = pending && !same;
  }
  if (pending) atomicAdd(&lh[key], 1u);
}
// Tiles start at multiples of TILE * c * 4 bytes, so all of them are 16-B aligned when acc is.
// Then the 16-B vectors of the NEXT tile are fetched into registers (c / 4 <= 8 per thread) before
// the current tile is reduced, and only written to LDS after it: the loads stay in flight across
// the per-pixel work.  With the 19 x 1024 histogram one workgroup fills a CU's LDS, so there is
// no second workgroup to hide the load latency behind (staged-only, load -> barrier -> reduce:
// 135 us at [8, 512, 1024, 19]; see DESIGN.md for this form).  An unaligned acc takes the plain
// stage_in loop.
template <int TILE>
__global__ void __launch_bounds__(TILE) conf_hist_kernel(const float* __restrict__ acc, unsigned long long* __restrict__ hist,
                                                         uint8_t* __restrict__ pred, uint16_t* __restrict__ cbin, long total, int c,
                                                         int bins, float inv) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* buf = (float*)smem_raw;                  // [TILE][c]
  unsigned int* lh = (unsigned int*)(buf + TILE * c);  // [c][bins]
  const int tid = threadIdx.x, cells = c * bins;
  const long stride = (long)gridDim.x * TILE;
  for (int i = tid; i < cells; i += TILE) lh[i] = 0;
  long p0 = (long)blockIdx.x * TILE;
  if (((uintptr_t)acc & 15) != 0) {
    for (; p0 < total; p0 += stride) {
      const int np = (int)min<long>(TILE, total - p0);
      __syncthreads();
      stage_in(acc + p0 * c, buf, np * c);
      __syncthreads();
      conf_hist_tile<TILE>(buf, lh, pred, cbin, p0, np, c, bins, inv);
    }
  } else {
    // kPlMaxC / 4 = 8 named 16-B registers per thread (an indexed array went to scratch)
#define PL_VECS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define PL_DECL(j) uint4 v##j = make_uint4(0, 0, 0, 0);
#define PL_FETCH(j) if (tid + j * TILE < nf) v##j = src[tid + j * TILE];
#define PL_PUT(j) if (tid + j * TILE < nv) ((uint4*)buf)[tid + j * TILE] = v##j;
    PL_VECS(PL_DECL)
    int np = (int)min<long>(TILE, total - p0), nv = (np * c) >> 2;  // np <= 0: no tile for this workgroup
    if (p0 < total) {
      const uint4* src = (const uint4*)(acc + p0 * c);
      const int nf = nv;
      PL_VECS(PL_FETCH)
    }
    while (p0 < total) {
      PL_VECS(PL_PUT)
      for (int i = (nv << 2) + tid; i < np * c; i += TILE) buf[i] = acc[p0 * c + i];  // ragged last tile
      __syncthreads();  // (also orders the zeroing of lh before the first tile's atomics)
      const long pn = p0 + stride;
      const int npn = (int)min<long>(TILE, total - pn), nvn = pn < total ? (npn * c) >> 2 : 0;
      if (pn < total) {
        const uint4* src = (const uint4*)(acc + pn * c);
        const int nf = nvn;
        PL_VECS(PL_FETCH)
      }
      conf_hist_tile<TILE>(buf, lh, pred, cbin, p0, np, c, bins, inv);
      __syncthreads();  // every row is read before the next tile overwrites buf
      p0 = pn;
      np = npn;
      nv = nvn;
    }
#undef PL_VECS
#undef PL_DECL
#undef PL_FETCH
#undef PL_PUT
  }
  __syncthreads();
  for (int i = tid; i < cells; i += TILE)
    if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
}

static int pl_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus < 1)
      cus = 256;
  }
  return cus;
}
template <int TILE>
static void conf_hist_launch(const float* acc, unsigned long long* hist, uint8_t* pred, uint16_t* cbin, long total, int c, int bins,
                             float inv, hipStream_t st) {
  static const bool lds_ok = hipFuncSetAttribute((const void*)conf_hist_kernel<TILE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)kPlLds) == hipSuccess;
  (void)lds_ok;
  const size_t lds = pl_lds_bytes(TILE, c, bins);
  // persistent: as many workgroups as the chip holds at once (LDS and the 32 waves of a CU), so
  // the zeroing and the flush of the private histogram are paid once per resident workgroup
  const long per_cu = std::max<long>(1, std::min<long>((long)(kPlLds / lds), 2048 / TILE));
  const int blocks = ew_blocks(total, TILE, (int)std::min<long>(per_cu * pl_cus(), 8192));
  hipLaunchKernelGGL(conf_hist_kernel<TILE>, dim3(blocks), dim3(TILE), lds, st, acc, hist, pred, cbin, total, c, bins, inv);
}
extern "C" int rtsds_conf_hist(const float* acc, unsigned long long* hist, uint8_t* pred, uint16_t* cbin, long total, int c, int bins,
                               float inv, void* stream) {
  if (total <= 0 || c < kPlMinC || c > kPlMaxC) return RTSDS_ERR_SHAPE;
  if (bins < kPlMinBins || bins > kPlMaxBins || !pl_pow2(bins)) return RTSDS_ERR_SHAPE;
  if (acc == nullptr || hist == nullptr || ((uintptr_t)acc & 3) || ((uintptr_t)hist & 7) || ((uintptr_t)cbin & 1))
    return RTSDS_ERR_UNSUPPORTED;
  if (pl_lds_bytes(kPlMinTile, c, bins) > kPlLds) return RTSDS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (pl_lds_bytes(kPlMaxTile, c, bins) <= kPlLds)
    conf_hist_launch<kPlMaxTile>(acc, hist, pred, cbin, total, c, bins, inv, st);
  else
    conf_hist_launch<kPlMinTile>(acc, hist, pred, cbin, total, c, bins, inv, st);
  RET_LAUNCH();
}

// ------------------------------------------------------------------ thresholded labels
// out[p] = pseudo_label(pred[p], cbin[p], tbin, c, ignore_index).  3 B in, 8 B out per pixel;
// groups of 8 pixels move as one 8-B + one 16-B load and four 16-B stores when the three pointers
// allow it.
__global__ void __launch_bounds__(256) pseudo_select_kernel(const uint8_t* __restrict__ pred, const uint16_t* __restrict__ cbin,
                                                            const int* __restrict__ tbin, int64_t* __restrict__ out, long total, int c,
                                                            int ignore, int vec) {
  __shared__ int tb[kPlMaxC];
  if ((int)threadIdx.x < c) tb[threadIdx.x] = tbin[threadIdx.x];
  __syncthreads();
  const long ng = vec ? total >> 3 : 0;
  GRID_STRIDE(g, ng) {
    const uint2 pv = ((const uint2*)pred)[g];
    const uint4 cv = ((const uint4*)cbin)[g];
    const unsigned int pw[2] = {pv.x, pv.y}, cw[4] = {cv.x, cv.y, cv.z, cv.w};
    long long o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = (int)((pw[j >> 2] >> (8 * (j & 3))) & 0xffu);
      const int b = (int)((cw[j >> 1] >> (16 * (j & 1))) & 0xffffu);
      o[j] = pseudo_label(k, b, tb, c, ignore);
    }
    longlong2* dst = (longlong2*)(out + (g << 3));
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[j] = make_longlong2(o[2 * j], o[2 * j + 1]);
  }
  const long done = ng << 3;
  GRID_STRIDE(i, total - done) {
    const long p = done + i;
    const int k = pred[p], b = cbin[p];
    out[p] = pseudo_label(k, b, tb, c, ignore);
  }
}
extern "C" int rtsds_pseudo_select(const uint8_t* pred, const uint16_t* cbin, const int* tbin, int64_t* out, long total, int c,
                                   int ignore_index, void* stream) {
  if (total <= 0 || c < kPlMinC || c > kPlMaxC) return RTSDS_ERR_SHAPE;
  if (pred == nullptr || cbin == nullptr || tbin == nullptr || out == nullptr || ((uintptr_t)cbin & 1) || ((uintptr_t)tbin & 3) ||
      ((uintptr_t)out & 7))
    return RTSDS_ERR_UNSUPPORTED;
  const int vec = (((uintptr_t)pred & 7) | ((uintptr_t)cbin & 15) | ((uintptr_t)out & 15)) == 0;
  hipLaunchKernelGGL(pseudo_select_kernel, dim3(ew_blocks(vec ? (total + 7) / 8 : total, 256, 4096)), dim3(256), 0,
                     (hipStream_t)stream, pred, cbin, tbin, out, total, c, ignore_index, vec);
  RET_LAUNCH();
}
