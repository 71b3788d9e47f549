// Probe: the entropy forward (csrc/entropy.hip em_fwd_kernel<T, 19, L>) with a thread per pixel (L = 1)
// against a pixel's classes split over L = 2 or 4 adjacent lanes (class k on lane k % L; maximum and
// sums joined by xor shuffles in a fixed order), at n = 8, c = 19, 64 x 128, bf16 and fp32, robust
// penalty.  The library launches kEmLanes; profiles/entropy/README.md holds the figures.  The
// candidates take turns: per round 5 warm-up launches, then 200 launches between one pair of events.
// Results are compared first (partials to 1e-5 relative, gradient term to 1e-6 absolute).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/probe/entropy_lanes.hip -o entropy_lanes
#include "../../rtsds_amd/csrc/entropy.hip"
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                               \
  do {                                                                      \
    hipError_t e_ = (x);                                                    \
    if (e_ != hipSuccess) {                                                 \
      printf("%s: %s\n", #x, hipGetErrorString(e_));                        \
      exit(1);                                                              \
    }                                                                       \
  } while (0)

template <typename T>
static void run(const char* name) {
  const int n = 8, h = 64, w = 128, c = 19;
  const long pixels = (long)n * h * w, total = pixels * c;
  std::vector<T> hx(total);
  unsigned s = 12345u;
  for (long i = 0; i < total; ++i) {  // sum of four uniforms, about N(0, 4^2)
    float acc = 0.f;
    for (int j = 0; j < 4; ++j) {
      s = s * 1664525u + 1013904223u;
      acc += (float)(s >> 8) / 16777216.f - 0.5f;
    }
    hx[i] = (T)(acc * 6.93f);
  }
  const EmPlan p = em_plan(n, h, w, c);
  T* dx;
  char* ws[3];
  CK(hipMalloc(&dx, total * sizeof(T)));
  CK(hipMemcpy(dx, hx.data(), total * sizeof(T), hipMemcpyHostToDevice));
  for (auto& q : ws) CK(hipMalloc(&q, p.part_bytes + p.term_bytes));
  EmArgs a[3];
  for (int i = 0; i < 3; ++i) {
    a[i].x = dx; a[i].pixels = pixels; a[i].c = c; a[i].penalty = RTSDS_ENTROPY_ROBUST; a[i].want_grad = 1;
    a[i].eta = 2.f; a[i].inv_lnc = (float)(1.0 / std::log((double)c));
    a[i].part = (float*)ws[i]; a[i].term = (float*)(ws[i] + p.part_bytes); a[i].hmap = nullptr;
  }
  const size_t lds = em_lds(c, sizeof(T));
  auto launch = [&](int v) {
    if (v == 0) hipLaunchKernelGGL((em_fwd_kernel<T, 19, 1>), dim3(p.blocks), dim3(kEmPix), lds, 0, a[0]);
    else if (v == 1) hipLaunchKernelGGL((em_fwd_kernel<T, 19, 2>), dim3(p.blocks), dim3(kEmPix * 2), lds, 0, a[1]);
    else hipLaunchKernelGGL((em_fwd_kernel<T, 19, 4>), dim3(p.blocks), dim3(kEmPix * 4), lds, 0, a[2]);
  };
  for (int v = 0; v < 3; ++v) launch(v);
  CK(hipDeviceSynchronize());
  std::vector<float> r[3];
  const size_t nf = (p.part_bytes + p.term_bytes) / 4;
  for (int v = 0; v < 3; ++v) {
    r[v].resize(nf);
    CK(hipMemcpy(r[v].data(), ws[v], nf * 4, hipMemcpyDeviceToHost));
  }
  for (int v = 1; v < 3; ++v) {
    double dpart = 0, dterm = 0;
    for (int i = 0; i < 2 * p.blocks; ++i) dpart = std::max(dpart, std::fabs((double)r[v][i] - r[0][i]) / std::fabs((double)r[0][i]));
    for (size_t i = p.part_bytes / 4; i < nf; ++i) dterm = std::max(dterm, std::fabs((double)r[v][i] - r[0][i]));
    printf("%s lanes %d against 1: partials differ by %.2e relative, gradient term by %.2e\n", name, 2 * v, dpart, dterm);
    if (dpart > 1e-5 || dterm > 1e-6) exit(2);
  }
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int reps = 200;
  for (int round = 0; round < 5; ++round)
    for (int v = 0; v < 3; ++v) {
      for (int i = 0; i < 5; ++i) launch(v);
      CK(hipDeviceSynchronize());
      CK(hipEventRecord(e0, 0));
      for (int i = 0; i < reps; ++i) launch(v);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      printf("%s round %d lanes %d: %.2f us per launch\n", name, round, v == 0 ? 1 : 2 * v, ms * 1e3 / reps);
    }
  CK(hipFree(dx));
  for (auto& q : ws) CK(hipFree(q));
}

int main() {
  run<bf16>("bf16");
  run<float>("fp32");
  return 0;
}
