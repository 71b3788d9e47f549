// Histogram matching of a decoded uint8 HWC RGB image to a reference image's statistics (gfx950):
// the per-channel histogram (rtsds_hist_u8) and the matched image (rtsds_hist_match).  No
// reference counterpart (its pipeline trains on GTA5 colours as they are).  All integer: counts,
// prefix sums, the 64-bit cross-multiplied CDF comparison and the Q8 blend, so the results are
// reproducible bit for bit and independent of the order in which blocks arrive.
//
// For one channel, hs / hr the source / reference counts, Cs / Cr their inclusive prefix sums,
// Ns = Cs[255], Nr = Cr[255]:
//   m[v]   = min { t : Cr[t] * Ns >= Cs[v] * Nr }     (v when Ns == 0 or Nr == 0)
//   lut[v] = (v * (256 - A) + m[v] * A + 128) >> 8    A = strength_q8 in 0..256
//   out    = lut[channel][in]
#include "ew_common.h"

static const int kHmBins = 256, kHmCells = 3 * kHmBins;  // [channel][value]
// Capped grids of 256-thread blocks: every block of the histogram ends with up to 768 global
// atomics, every block of the match starts with the 6 KB LUT prologue, so neither grows with the
// image.  HM_HIST_BLOCKS / HM_MATCH_BLOCKS, HM_HIST_AGGREGATE and HM_LUT_KERNEL build the
// variants DESIGN.md compares (tools/bench_histmatch.py); the defaults are what was fastest on
// the MI355X at 1052 x 1914: one histogram block per CU (the flush, not the read, is what more
// blocks add to; fewer leave a one-colour image to too few LDS atomic units), two match blocks.
#ifndef HM_HIST_BLOCKS
#define HM_HIST_BLOCKS 256
#endif
#ifndef HM_MATCH_BLOCKS
#define HM_MATCH_BLOCKS 512
#endif
#ifndef HM_HIST_AGGREGATE
#define HM_HIST_AGGREGATE 0
#endif
#ifndef HM_LUT_KERNEL
#define HM_LUT_KERNEL 0
#endif

// ------------------------------------------------------------------ histogram
// One byte into the block's LDS counters.  Every lane of the wave calls it (valid says whether
// the lane holds a byte).  Real images put most of a wave on one cell (sky, road), and
// same-address LDS atomics serialise:
//   AGG = false: lh is the wave's own copy of the 768 counters, one add per lane;
//   AGG = true:  lh is shared by the block; the wave peels its two most likely keys first (the
//                key of its first pending lane: one ballot, ONE lane adds the count), the lanes
//                left over add 1 each -- the scheme of pseudo.hip's confidence histogram.
template <bool AGG>
RT_DEV void hm_count(unsigned int* lh, int key, bool valid) {
  if constexpr (AGG) {
    const int lane = threadIdx.x & 63;
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
  } else {
    if (valid) atomicAdd(&lh[key], 1u);
  }
}

// img: nbytes = h * w * 3 bytes, the channel of byte i is i % 3.  VEC (16-B aligned base): a
// thread takes 16 bytes per step, the channel of its first byte is (16 g) % 3 = g % 3; the last
// nbytes % 16 bytes go through the scalar loop of block 0.  Else the scalar loop takes them all.
// Both loops run a wave-uniform number of steps (the ballots of hm_count need every lane).
template <bool VEC, bool AGG>
__global__ void __launch_bounds__(256) hm_hist_kernel(const uint8_t* __restrict__ img, unsigned int* __restrict__ hist, long nbytes) {
  constexpr int kCopies = AGG ? 1 : 4;
  __shared__ unsigned int lh_all[kCopies * kHmCells];
  const int tid = threadIdx.x;
  for (int i = tid; i < kCopies * kHmCells; i += 256) lh_all[i] = 0;
  __syncthreads();
  unsigned int* lh = lh_all + (AGG ? 0 : (tid >> 6) * kHmCells);
  const long stride = (long)gridDim.x * 256;
  long done = 0;
  if constexpr (VEC) {
    const long nvec = nbytes >> 4;
    const uint4* src = (const uint4*)img;
    for (long g0 = (long)blockIdx.x * 256; g0 < nvec; g0 += stride) {
      const long g = g0 + tid;
      const bool valid = g < nvec;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (valid) v = src[g];
      const int phase = (int)(g % 3);
      const unsigned int wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        int ch = phase + (j % 3);
        if (ch >= 3) ch -= 3;
        hm_count<AGG>(lh, ch * kHmBins + (int)((wd[j >> 2] >> (8 * (j & 3))) & 255u), valid);
      }
    }
    done = nvec << 4;
  }
  if (!VEC || blockIdx.x == 0) {
    const long first = VEC ? 0 : (long)blockIdx.x * 256, step = VEC ? 256 : stride;
    for (long i0 = first; i0 < nbytes - done; i0 += step) {
      const long i = done + i0 + tid;
      const bool valid = i < nbytes;
      hm_count<AGG>(lh, valid ? (int)(i % 3) * kHmBins + (int)img[i] : 0, valid);
    }
  }
  __syncthreads();
  for (int i = tid; i < kHmCells; i += 256) {
    unsigned int s = lh_all[i];
    if constexpr (!AGG) s += lh_all[kHmCells + i] + lh_all[2 * kHmCells + i] + lh_all[3 * kHmCells + i];
    if (s) atomicAdd(&hist[i], s);
  }
}

extern "C" int rtsds_hist_u8(const uint8_t* img, int c, int h, int w, unsigned int* hist, void* stream) {
  if (!img || !hist || c <= 0 || h <= 0 || w <= 0 || (unsigned long long)h * (unsigned long long)w > 0xffffffffull)
    return RTSDS_ERR_SHAPE;
  if (c != 3 || ((uintptr_t)hist & 3)) return RTSDS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(hist, 0, kHmCells * sizeof(unsigned int), st) != hipSuccess) {
    (void)hipGetLastError();
    return RTSDS_ERR_LAUNCH;
  }
  const long nbytes = (long)h * w * 3;
  constexpr bool kAgg = HM_HIST_AGGREGATE != 0;
  if (((uintptr_t)img & 15) == 0)
    hipLaunchKernelGGL((hm_hist_kernel<true, kAgg>), dim3(ew_blocks(nbytes >> 4, 256, HM_HIST_BLOCKS)), dim3(256), 0, st, img, hist,
                       nbytes);
  else
    hipLaunchKernelGGL((hm_hist_kernel<false, kAgg>), dim3(ew_blocks(nbytes, 256, HM_HIST_BLOCKS)), dim3(256), 0, st, img, hist,
                       nbytes);
  RET_LAUNCH();
}

// ------------------------------------------------------------------ match
// The 768-byte LUT from the two histograms, by the 256 threads of one block; thread v owns value
// v of the three channels.  Six inclusive scans (source and reference, three channels): a shuffle
// scan per wave, the three preceding wave totals added through LDS.  uint32 sums: the totals of
// both histograms are pixel counts <= 2^32 - 1 (rtsds_hist_u8 refuses larger images), so the
// cross products stay below 2^64.  m[v] by an 8-step binary search over the non-decreasing Cr
// (the predicate holds at t = 255 whenever Ns and Nr are positive, so the count of t that fail
// is the smallest t that holds).
struct HmLds {
  unsigned int cr[kHmCells];  // the reference's prefix sums
  unsigned int wtot[6][4];    // per scan, the totals of the four waves
  uint8_t lut[kHmCells];
};
RT_DEV void hm_build_lut(const unsigned int* __restrict__ hist_src, const unsigned int* __restrict__ hist_ref, int a, HmLds& s) {
  const int v = threadIdx.x, lane = v & 63, wv = v >> 6;
  unsigned int x[6];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    x[ch] = hist_src[ch * kHmBins + v];
    x[3 + ch] = hist_ref[ch * kHmBins + v];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned int up = __shfl_up(x[k], o, 64);
      if (lane >= o) x[k] += up;
    }
    if (lane == 63) s.wtot[k][wv] = x[k];
  }
  __syncthreads();
  unsigned int total[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    unsigned int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned int t = s.wtot[k][i];
      if (i < wv) before += t;
      all += t;
    }
    x[k] += before;
    total[k] = all;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) s.cr[ch * kHmBins + v] = x[3 + ch];
  __syncthreads();
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const unsigned long long ns = total[ch], nr = total[3 + ch];
    int m = v;
    if (ns != 0 && nr != 0) {
      const unsigned long long target = (unsigned long long)x[ch] * nr;
      const unsigned int* cr = s.cr + ch * kHmBins;
      int lo = 0;
#pragma unroll
      for (int step = 128; step > 0; step >>= 1)
        if ((unsigned long long)cr[lo + step - 1] * ns < target) lo += step;
      m = lo;
    }
    s.lut[ch * kHmBins + v] = (uint8_t)((v * (256 - a) + m * a + 128) >> 8);
  }
  __syncthreads();
}

// dst[i] = lut[i % 3][src[i]].  LUT_IN (the one-launch form): every block builds the LUT in its
// prologue, block 0 also stores it to lut_out; else the 768 bytes are read from lut_in, which
// hm_lut_kernel wrote.  src may be dst: a thread reads its bytes before it stores them, and no
// byte is touched by two threads.  VEC: both bases 16-B aligned, 16 bytes per thread and step.
template <bool VEC, bool LUT_IN>
__global__ void __launch_bounds__(256) hm_match_kernel(const uint8_t* src, uint8_t* dst, long nbytes, const unsigned int* __restrict__ hist_src,
                                                       const unsigned int* __restrict__ hist_ref, int a, const uint8_t* lut_in,
                                                       uint8_t* lut_out) {
  __shared__ HmLds s;
  const int tid = threadIdx.x;
  if constexpr (LUT_IN) {
    for (int i = tid; i < kHmCells; i += 256) s.lut[i] = lut_in[i];
    __syncthreads();
  } else {
    hm_build_lut(hist_src, hist_ref, a, s);
    if (blockIdx.x == 0 && lut_out)
      for (int i = tid; i < kHmCells; i += 256) lut_out[i] = s.lut[i];
  }
  long done = 0;
  if constexpr (VEC) {
    const long nvec = nbytes >> 4;
    GRID_STRIDE(g, nvec) {
      const uint4 v = ((const uint4*)src)[g];
      const int phase = (int)(g % 3);
      unsigned int wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        unsigned int o = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          int ch = phase + ((4 * q + b) % 3);
          if (ch >= 3) ch -= 3;
          o |= (unsigned int)s.lut[ch * kHmBins + (int)((wd[q] >> (8 * b)) & 255u)] << (8 * b);
        }
        wd[q] = o;
      }
      ((uint4*)dst)[g] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    }
    done = nvec << 4;
    if (blockIdx.x != 0) return;
    for (long i = done + tid; i < nbytes; i += 256) dst[i] = s.lut[(int)(i % 3) * kHmBins + src[i]];
  } else {
    GRID_STRIDE(i, nbytes) dst[i] = s.lut[(int)(i % 3) * kHmBins + src[i]];
  }
}

__global__ void __launch_bounds__(256) hm_lut_kernel(const unsigned int* __restrict__ hist_src, const unsigned int* __restrict__ hist_ref, int a,
                                                     uint8_t* __restrict__ lut_out) {
  __shared__ HmLds s;
  hm_build_lut(hist_src, hist_ref, a, s);
  for (int i = threadIdx.x; i < kHmCells; i += 256) lut_out[i] = s.lut[i];
}

extern "C" int rtsds_hist_match(const uint8_t* src, uint8_t* dst, int c, int h, int w, const unsigned int* hist_src,
                                const unsigned int* hist_ref, int strength_q8, uint8_t* lut_out, void* stream) {
  if (!src || !dst || !hist_src || !hist_ref || c <= 0 || h <= 0 || w <= 0 || strength_q8 < 0 || strength_q8 > 256 ||
      (unsigned long long)h * (unsigned long long)w > 0xffffffffull)
    return RTSDS_ERR_SHAPE;
  if (c != 3 || ((uintptr_t)hist_src & 3) || ((uintptr_t)hist_ref & 3)) return RTSDS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const long nbytes = (long)h * w * 3;
  const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  const int blocks = ew_blocks(vec ? nbytes >> 4 : nbytes, 256, HM_MATCH_BLOCKS);
#if HM_LUT_KERNEL
  // measurement variant: the LUT by a one-block kernel in front, through lut_out (required here)
  if (!lut_out) return RTSDS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(hm_lut_kernel, dim3(1), dim3(256), 0, st, hist_src, hist_ref, strength_q8, lut_out);
  if (vec)
    hipLaunchKernelGGL((hm_match_kernel<true, true>), dim3(blocks), dim3(256), 0, st, src, dst, nbytes, hist_src, hist_ref, strength_q8,
                       (const uint8_t*)lut_out, (uint8_t*)nullptr);
  else
    hipLaunchKernelGGL((hm_match_kernel<false, true>), dim3(blocks), dim3(256), 0, st, src, dst, nbytes, hist_src, hist_ref, strength_q8,
                       (const uint8_t*)lut_out, (uint8_t*)nullptr);
#else
  if (vec)
    hipLaunchKernelGGL((hm_match_kernel<true, false>), dim3(blocks), dim3(256), 0, st, src, dst, nbytes, hist_src, hist_ref, strength_q8,
                       (const uint8_t*)nullptr, lut_out);
  else
    hipLaunchKernelGGL((hm_match_kernel<false, false>), dim3(blocks), dim3(256), 0, st, src, dst, nbytes, hist_src, hist_ref,
                       strength_q8, (const uint8_t*)nullptr, lut_out);
#endif
  RET_LAUNCH();
}
