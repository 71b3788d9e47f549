// Label statistics for class weighting (losses.class_statistics -> losses.class_weights).
//
// Over a batch of int64 label maps [n][h][w] with c <= 32 classes:
//   count[k]   += number of pixels labelled k
//   support[k] += number of valid pixels (label in [0, c)) of the images that contain class k
// (the second is median-frequency balancing's denominator: Eigen & Fergus, 2015).  A label equal
// to ignore_index or outside [0, c) is neither counted nor part of any support.
//
// Integers only, so the result is exact and independent of any order:
//   pass 1  one workgroup per (image, chunk of the image): a workgroup-private LDS histogram
//           (32 copies, one per LDS bank, so the lanes of a half wave never collide on the frequent
//           classes) filled with LDS integer atomics, reduced and written to ws[image][chunk][32];
//           nothing to clear beforehand.
//   pass 2  one workgroup per image: sums the image's chunk counts per class, forms the image's
//           valid-pixel total from the 32 class sums, and adds both into count[k] / support[k] with
//           64-bit integer atomics (at most 2 c per image).
#include "common.h"

static const int kLsClasses = 32;  // class_row.h's bound on a class vector
static const int kLsChunks = 64;   // workgroups per image

__global__ void __launch_bounds__(256) label_hist_kernel(const int64_t* __restrict__ label, long hw, int c, int ignore,
                                                         unsigned int* __restrict__ part) {
  __shared__ unsigned int hist[kLsClasses * 32];  // [class][copy]: copy = bank
  const int tid = threadIdx.x;
  for (int e = tid; e < kLsClasses * 32; e += 256) hist[e] = 0u;
  __syncthreads();
  const int img = blockIdx.y, chunk = blockIdx.x;
  const long per = (hw + kLsChunks - 1) / kLsChunks;
  const long p0 = chunk * per, p1 = min(p0 + per, hw);
  const int64_t* L = label + (long)img * hw;
  const int copy = tid & 31;
  // four labels in flight per thread (clamped in range, counted only when inside the chunk)
  for (long p = p0 + tid; p < p1; p += 4 * 256) {
    long t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) t[u] = L[min(p + u * 256, p1 - 1)];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (p + u * 256 < p1 && t[u] != ignore && t[u] >= 0 && t[u] < c) atomicAdd(&hist[(int)t[u] * 32 + copy], 1u);
  }
  __syncthreads();
  if (tid < kLsClasses) {
    unsigned int s = 0;
    for (int k = 0; k < 32; ++k) s += hist[tid * 32 + ((k + tid) & 31)];
    part[((long)img * kLsChunks + chunk) * kLsClasses + tid] = s;
  }
}

// one workgroup per image: thread (j, k) sums class k over the chunks j, j + 8, ... (all loads in
// flight at once), the eight partial sums meet in LDS
__global__ void __launch_bounds__(256) label_merge_kernel(const unsigned int* __restrict__ part, int c,
                                                          unsigned long long* __restrict__ count,
                                                          unsigned long long* __restrict__ support) {
  __shared__ unsigned long long red[8][kLsClasses];
  __shared__ unsigned long long cls[kLsClasses];
  const int tid = threadIdx.x, k = tid & 31, j = tid >> 5;
  const unsigned int* P = part + (long)blockIdx.x * kLsChunks * kLsClasses;
  unsigned int v[kLsChunks / 8];
#pragma unroll
  for (int u = 0; u < kLsChunks / 8; ++u) v[u] = P[(j + 8 * u) * kLsClasses + k];
  unsigned long long s = 0;
#pragma unroll
  for (int u = 0; u < kLsChunks / 8; ++u) s += v[u];
  red[j][k] = s;
  __syncthreads();
  if (tid < kLsClasses) {
    unsigned long long m = 0;
    for (int q = 0; q < 8; ++q) m += red[q][tid];
    cls[tid] = m;
  }
  __syncthreads();
  if (tid < c) {  // classes >= c hold 0 (pass 1 counts labels in [0, c) only)
    unsigned long long valid = 0;
    for (int q = 0; q < kLsClasses; ++q) valid += cls[q];
    const unsigned long long mine = cls[tid];
    if (mine > 0) {
      atomicAdd(&count[tid], mine);
      atomicAdd(&support[tid], valid);
    }
  }
}

extern "C" size_t rtsds_label_stats_workspace(int n, int c) {
  if (n < 1 || c < 1 || c > kLsClasses) return 0;
  return (size_t)n * kLsChunks * kLsClasses * sizeof(unsigned int);
}

extern "C" int rtsds_label_stats(const int64_t* label, int n, int h, int w, int c, int ignore_index, unsigned long long* count,
                                 unsigned long long* support, void* ws, size_t ws_bytes, void* stream) {
  if (!label || !count || !support || n < 1 || n > 65535 || h < 1 || w < 1 || c < 1 || c > kLsClasses) return RTSDS_ERR_SHAPE;
  if ((long)h * w > 0xffffffffL) return RTSDS_ERR_SHAPE;  // an image's counts are 32-bit
  if (!ws || ws_bytes < rtsds_label_stats_workspace(n, c)) return RTSDS_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(label_hist_kernel, dim3(kLsChunks, n), dim3(256), 0, st, label, (long)h * w, c, ignore_index, (unsigned int*)ws);
  hipLaunchKernelGGL(label_merge_kernel, dim3(n), dim3(256), 0, st, (const unsigned int*)ws, c, count, support);
  RET_LAUNCH();
}
