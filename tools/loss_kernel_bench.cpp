// loss_kernel_bench.cpp — times the Sigmoid / SigmoidCrossEntropyLoss /
// EuclideanLoss kernels against the kernels of the same traffic class that
// the engine already had: ReLU forward / backward (same bytes per element)
// and the float4 BatchNorm statistics kernel (the existing block reduce);
// beside them the clip_gradients sum of squares.
// One process, the variants alternated round by round, one large element
// count (512 MiB per tensor, beyond the Infinity Cache).
//
//   make -C caffe-mpi.github.io_amd loss-kernel-bench
//   tools/loss_kernel_bench [rounds]     # table of profiles/sigmoid_loss_kernels.txt
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "math.hpp"

using namespace camd;

struct Variant {
  std::string name;
  double bytes;  // moved per launch
  std::function<void(hipStream_t)> run;
  std::vector<float> ms;
};

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 5;
  const long n = 1L << 27;  // floats per tensor: 512 MiB
  Engine& E = Engine::get();
  E.set_mode_gpu(0);
  hipStream_t s = E.stream;
  float *a, *b, *c, *loss;
  double* partials;
  HIP_CHECK(hipMalloc((void**)&a, n * sizeof(float)));
  HIP_CHECK(hipMalloc((void**)&b, n * sizeof(float)));
  HIP_CHECK(hipMalloc((void**)&c, n * sizeof(float)));
  HIP_CHECK(hipMalloc((void**)&loss, 16 * sizeof(float)));
  // BN statistics: the same n floats as [N][C][S], S % 4 == 0 -> the f4 body
  const int N = 64, C = 256;
  const long S = n / ((long)N * C);
  const int nb = gpu::bn_blocks_per_channel(N, C);
  const size_t pbytes = std::max<size_t>(
      sizeof(double) * gpu::loss_partials(n), 2 * sizeof(double) * C * nb);
  HIP_CHECK(hipMalloc((void**)&partials, pbytes));
  gpu::fill_uniform(s, n, 1, 0, -3.f, 3.f, a);  // logits / activations
  gpu::fill_uniform(s, n, 2, 0, 0.f, 1.f, b);   // targets / top data
  const double fb = (double)n * sizeof(float);
  std::vector<Variant> v = {
      {"k_relu_fwd", 2 * fb,
       [&](hipStream_t st) { gpu::relu_fwd(st, a, n, 0.f, c); }, {}},
      {"k_sigmoid_fwd", 2 * fb,
       [&](hipStream_t st) { gpu::sigmoid_fwd(st, a, n, c); }, {}},
      {"k_relu_bwd", 3 * fb,
       [&](hipStream_t st) { gpu::relu_bwd(st, a, b, n, 0.f, c); }, {}},
      {"k_sigmoid_bwd", 3 * fb,
       [&](hipStream_t st) { gpu::sigmoid_bwd(st, b, a, n, c); }, {}},
      {"k_bn_fwd_stats<f4>", fb,
       [&](hipStream_t st) { gpu::bn_fwd_stats(st, a, N, C, S, nb, partials); },
       {}},
      {"k_sigmoid_ce_fwd", 2 * fb,
       [&](hipStream_t st) {
         gpu::sigmoid_ce_fwd(st, a, b, n, N, partials, loss);
       },
       {}},
      {"k_euclid_fwd", 2 * fb,
       [&](hipStream_t st) { gpu::euclid_fwd(st, a, b, n, N, partials, loss); },
       {}},
      // clip_gradients: the sum of squares over one stream
      // (profiles/clip_gradients.txt); one partial per block, no final sum
      {"k_grad_sumsq", fb,
       [&](hipStream_t st) { gpu::grad_sumsq(st, a, 0, n, partials); }, {}},
      {"k_sigmoid_ce_bwd", 3 * fb,
       [&](hipStream_t st) { gpu::sigmoid_ce_bwd(st, a, b, n, 1.f / N, c); },
       {}},
      {"k_euclid_bwd", 3 * fb,
       [&](hipStream_t st) {
         gpu::euclid_bwd(st, a, b, n, 1.f / N, c, 0.f, nullptr);
       },
       {}},
  };
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  for (int r = -1; r < rounds; ++r)  // round -1 warms up, untimed
    for (auto& k : v) {
      HIP_CHECK(hipEventRecord(e0, s));
      k.run(s);
      HIP_CHECK(hipEventRecord(e1, s));
      HIP_CHECK(hipEventSynchronize(e1));
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 0) k.ms.push_back(ms);
    }
  float h_loss = 0;
  HIP_CHECK(hipMemcpy(&h_loss, loss, sizeof(float), hipMemcpyDeviceToHost));
  // the norm the clip path would report for tensor a, against its expectation
  float nf[2];
  const int np = gpu::grad_sumsq(s, a, 0, n, partials);
  gpu::clip_finalize(s, partials, np, 1, 1.f, loss);
  HIP_CHECK(hipStreamSynchronize(s));
  HIP_CHECK(hipMemcpy(nf, loss, sizeof(nf), hipMemcpyDeviceToHost));
  printf("# grad_sumsq norm %.9g, factor at clip 1 %.9g (uniform [-3, 3): "
         "sqrt(3 n) = %.9g)\n",
         nf[0], nf[1], std::sqrt(3.0 * n));
  printf("# n = %ld floats per tensor (%.0f MiB), %d alternated rounds, one "
         "process; last loss written %g\n",
         n, fb / 1048576.0, rounds, h_loss);
  printf("# the two loss forwards include their one-block final sum launch\n");
  printf("%-20s %10s %10s %10s %12s %10s\n", "kernel", "min ms", "median ms",
         "max ms", "median GB/s", "spread %");
  for (auto& k : v) {
    std::sort(k.ms.begin(), k.ms.end());
    const float med = k.ms[k.ms.size() / 2];
    printf("%-20s %10.4f %10.4f %10.4f %12.1f %10.2f\n", k.name.c_str(),
           k.ms.front(), med, k.ms.back(), k.bytes / med / 1e6,
           100.0 * (k.ms.back() - k.ms.front()) / med);
  }
  return 0;
}
