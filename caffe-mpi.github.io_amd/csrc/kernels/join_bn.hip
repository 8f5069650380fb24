// join_bn.hip — two kernels that each do the work of a pair of launches the
// residual-join / BatchNorm chain used to make: the backward of a residual
// join (Split + ReLU) in one pass, and the BN forward finalize that also
// advances the moving averages.  Both are bit-identical to the pairs they
// replace (same fp32 operations in the same order, nothing contracted).
// Built with the packed-fp32 instructions off (Makefile), like depthwise.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../math.hpp"

namespace camd {
namespace gpu {
namespace {

constexpr int kTPB = 256;
using f4 = __attribute__((ext_vector_type(4))) float;

// Backward of a two-top Split directly after a ReLU, with that ReLU's
// backward: dx = (a + b) * (ref > 0 ? 1 : slope) — the add of k_add3, then
// the multiply of k_relu_bwd, without the write and re-read of the sum
// between them.  dx may be a or b (a thread reads its pack before it writes
// it), so those three carry no __restrict__.
__global__ void k_add_relu_bwd(long n4, const f4* a, const f4* b,
                               const f4* __restrict__ ref, float slope,
                               f4* dx) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    const f4 v = ref[i];
    f4 d = a[i] + b[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] *= v[j] > 0.f ? 1.f : slope;
    dx[i] = d;
  }
}

// One block, C-wide, between the statistics and the norm kernel: the batch
// slices' partials summed in index order in double, then the moving
// averages from the mean / var just written (batch_norm_layer.cpp:200-207).
__global__ void k_bn_fwd_finalize(const double2* __restrict__ partials,
                                  int nb, int C, long NS, float eps,
                                  float maf, int copy_only,
                                  float* __restrict__ mean,
                                  float* __restrict__ var,
                                  float* __restrict__ inv_std,
                                  float* __restrict__ gmean,
                                  float* __restrict__ gvar) {
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    double s1 = 0, s2 = 0;
    for (int b = 0; b < nb; ++b) {
      s1 += partials[(long)c * nb + b].x;
      s2 += partials[(long)c * nb + b].y;
    }
    const double m = s1 / NS;
    const double v = s2 / NS - m * m;  // E[x^2]-m^2 in double ≈ E[(x-m)^2]
    const float mf = (float)m, vf = (float)v;
    mean[c] = mf;
    var[c] = vf;
    inv_std[c] = (float)(1.0 / sqrt(v + (double)eps));
    if (copy_only) {
      gmean[c] = mf;
      gvar[c] = vf;
    } else {
      // two products and one sum, each rounded: an FMA here would change
      // the running statistics in the last bit
#pragma clang fp contract(off)
      gmean[c] = (1.f - maf) * mf + maf * gmean[c];
      gvar[c] = (1.f - maf) * vf + maf * gvar[c];
    }
  }
}

}  // namespace

void add_relu_bwd(hipStream_t s, long n, const float* a, const float* b,
                  const float* ref, float slope, float* dx) {
  PerfScope perf(PERF_CLASS("eltwise"), s, 0, 16.0 * n);
  const long n4 = (n + 3) / 4;  // blobs are 64B-padded: the last pack is whole
  const long blocks = (n4 + (long)kTPB * 4 - 1) / ((long)kTPB * 4);
  hipLaunchKernelGGL(k_add_relu_bwd, dim3((int)std::min<long>(blocks, 2048)),
                     dim3(kTPB), 0, s, n4, (const f4*)a, (const f4*)b,
                     (const f4*)ref, slope, (f4*)dx);
}

void bn_fwd_finalize(hipStream_t s, const void* partials, int nb, int C,
                     long NS, float eps, float maf, int copy_only,
                     float* mean, float* var, float* inv_std, float* gmean,
                     float* gvar) {
  hipLaunchKernelGGL(k_bn_fwd_finalize, dim3(1), dim3(kTPB), 0, s,
                     (const double2*)partials, nb, C, NS, eps, maf,
                     copy_only, mean, var, inv_std, gmean, gvar);
}

}  // namespace gpu
}  // namespace camd
