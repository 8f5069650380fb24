// dense_softmax.hip — gfx950 kernels for the head of a segmentation net:
// SoftmaxWithLoss over a [N][C][H][W] score map with a loss_param
// (ignore_label, normalization), and the Crop layer in front of it.
//
// The class-per-row kernels of elementwise.hip give a wave to one pixel and
// stride the lanes over the channels, `inner` floats apart.  Here the work
// is split the other way: a thread owns P pixels adjacent along the
// flattened H*W axis and loops over the channels, so for every channel the
// lanes of a wave read one contiguous run of a channel plane, P floats per
// lane in one 4-, 8- or 16-byte access.  P is the widest of 4, 2, 1 that
// divides `inner` (every plane's run is then aligned, and a thread's pixels
// never straddle two images), capped so that the registers hold.
//
//   resident (C <= 32)  the thread's CR x P logits stay in registers, CR
//     the channel count padded to 4, 8, 16 or 32 and P * CR <= 64: x is read
//     once and prob written once.
//   stream (C > 32)  one pass keeps a running max and a rescaled sum per
//     pixel and picks up x[label]; a second pass re-reads x (L2 at FCN
//     sizes is not assumed) and writes prob once.
//
// Either form takes the loss term and the valid count of its pixels from
// the registers it holds: one double and one int per thread, a block tree
// in a fixed order, one partial pair per block, then k_dsm_final (one
// block, fixed order) applies the normalizer and leaves {valid count,
// 1 / normalizer} on the device for the backward.  No atomics; the grid is
// a function of the shape alone, so a rerun gives the same bits.
//
// The resident/stream switch, the (CR, P) table and the grid cap are policy
// constants read off the register budget, not measurements.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../math.hpp"

namespace camd {
namespace gpu {
namespace {

constexpr int kTPB = 256;
constexpr int kResidentMaxC = 32;
constexpr int kResidentRegs = 64;  // P * CR logits a thread may hold
constexpr int kStreamChunk = 8;    // channels loaded ahead per pixel run
constexpr float kFltMax = 3.402823466e38f;

// P adjacent floats as one access
template <int P>
struct Run {
  using T = __attribute__((ext_vector_type(P))) float;
};
template <>
struct Run<1> {
  using T = float;
};
template <int P>
__device__ __forceinline__ void load_run(const float* __restrict__ p,
                                         float (&v)[P]) {
  if constexpr (P == 1) {
    v[0] = *p;
  } else {
    const typename Run<P>::T t = *(const typename Run<P>::T*)p;
#pragma unroll
    for (int j = 0; j < P; ++j) v[j] = t[j];
  }
}
template <int P>
__device__ __forceinline__ void store_run(float* __restrict__ p,
                                          const float (&v)[P]) {
  if constexpr (P == 1) {
    *p = v[0];
  } else {
    typename Run<P>::T t;
#pragma unroll
    for (int j = 0; j < P; ++j) t[j] = v[j];
    *(typename Run<P>::T*)p = t;
  }
}

// the block's Σ a and Σ b, thread order fixed; valid in thread 0
__device__ __forceinline__ void block_sum2(double& a, double& b) {
  __shared__ double sh[2][kTPB];
  sh[0][threadIdx.x] = a;
  sh[1][threadIdx.x] = b;
  __syncthreads();
  for (int off = kTPB / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + off];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + off];
    }
    __syncthreads();
  }
  a = sh[0][0];
  b = sh[1][0];
}

// pixel group t of P pixels: image o, first pixel s0 within the image
struct Group {
  long x0;    // offset of (o, channel 0, s0) in x / prob / dx
  long lab0;  // offset of (o, s0) in label
};
template <int P>
__device__ __forceinline__ Group group_at(unsigned t, unsigned gpi, int C,
                                          int inner) {
  const unsigned o = t / gpi;
  const unsigned s0 = (t - o * gpi) * P;
  return Group{(long)o * C * inner + s0, (long)o * inner + s0};
}

// what one non-ignored pixel adds; pl is NaN for a label outside [0, C)
struct LossAcc {
  double sum = 0;
  int valid = 0;
  __device__ __forceinline__ void add(const DenseSoftmax& g, int lv,
                                      float pl) {
    if (g.has_ignore && lv == g.ignore) return;
    sum += (double)softmax_nll_term(pl);
    ++valid;
  }
  __device__ __forceinline__ void store(double* __restrict__ partials) {
    double a = sum, b = (double)valid;
    block_sum2(a, b);
    if (threadIdx.x == 0) {
      partials[2 * blockIdx.x] = a;
      partials[2 * blockIdx.x + 1] = b;
    }
  }
};

// ------------------------------------------------------- forward, resident
// NaN / +inf in a pixel's logits make its whole prob row NaN and -inf is
// benign, as in k_softmax_fwd: fmaxf drops NaN operands and __expf may
// launder NaN, so the contamination is detected explicitly.
template <int CR, int P>
__global__ __launch_bounds__(kTPB) void k_dsm_fwd(
    const float* __restrict__ x, const float* __restrict__ label,
    DenseSoftmax g, unsigned gpi, unsigned groups, float* __restrict__ prob,
    double* __restrict__ partials) {
  const int C = g.C;
  const long plane = g.inner;
  LossAcc acc;
  for (unsigned t = blockIdx.x * kTPB + threadIdx.x; t < groups;
       t += gridDim.x * kTPB) {
    const Group q = group_at<P>(t, gpi, C, g.inner);
    float v[CR][P];
    float lab[P];
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < C) load_run<P>(x + q.x0 + c * plane, v[c]);
    load_run<P>(label + q.lab0, lab);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      float mx = -kFltMax;
      int bad = 0;
#pragma unroll
      for (int c = 0; c < CR; ++c)
        if (c < C) {
          mx = fmaxf(mx, v[c][j]);
          bad |= (v[c][j] != v[c][j]) | (v[c][j] > kFltMax);
        }
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < CR; ++c)
        if (c < C) {
          v[c][j] = __expf(v[c][j] - mx);
          sum += v[c][j];
        }
      const float inv = 1.f / sum;
      const float fix = bad ? __builtin_nanf("") : 0.f;
      const int lv = (int)lab[j];
      float pl = __builtin_nanf("");
#pragma unroll
      for (int c = 0; c < CR; ++c)
        if (c < C) {
          v[c][j] = v[c][j] * inv + fix;
          if (c == lv) pl = v[c][j];  // a select: no register indexing
        }
      acc.add(g, lv, pl);
    }
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < C) store_run<P>(prob + q.x0 + c * plane, v[c]);
  }
  acc.store(partials);
}

// ------------------------------------------------------ forward, streaming
template <int P>
__global__ __launch_bounds__(kTPB) void k_dsm_fwd_stream(
    const float* __restrict__ x, const float* __restrict__ label,
    DenseSoftmax g, unsigned gpi, unsigned groups, float* __restrict__ prob,
    double* __restrict__ partials) {
  const int C = g.C;
  const long plane = g.inner;
  LossAcc acc;
  for (unsigned t = blockIdx.x * kTPB + threadIdx.x; t < groups;
       t += gridDim.x * kTPB) {
    const Group q = group_at<P>(t, gpi, C, g.inner);
    float lab[P], m[P], sm[P], xl[P];
    int lv[P], bad[P];
    load_run<P>(label + q.lab0, lab);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      lv[j] = (int)lab[j];
      m[j] = -kFltMax;
      sm[j] = 0.f;
      xl[j] = 0.f;
      bad[j] = 0;
    }
    // pass 1: running max m and Σ exp(x - m), rescaled when m moves; one
    // exp per element: with d = x - m, e = exp(-|d|) is the new term
    // (d <= 0) or the factor that rescales the old sum (d > 0)
    for (int c0 = 0; c0 < C; c0 += kStreamChunk) {
      float v[kStreamChunk][P];
#pragma unroll
      for (int k = 0; k < kStreamChunk; ++k)
        if (c0 + k < C) load_run<P>(x + q.x0 + (c0 + k) * plane, v[k]);
#pragma unroll
      for (int k = 0; k < kStreamChunk; ++k)
        if (c0 + k < C) {
#pragma unroll
          for (int j = 0; j < P; ++j) {
            const float val = v[k][j];
            bad[j] |= (val != val) | (val > kFltMax);
            if (c0 + k == lv[j]) xl[j] = val;
            const float d = val - m[j];
            const float e = __expf(-fabsf(d));
            sm[j] = d > 0.f ? sm[j] * e + 1.f : sm[j] + e;
            m[j] = d > 0.f ? val : m[j];
          }
        }
    }
    float inv[P], fix[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      inv[j] = 1.f / sm[j];
      fix[j] = bad[j] ? __builtin_nanf("") : 0.f;
      const bool in_range = lv[j] >= 0 && lv[j] < C;
      acc.add(g, lv[j],
              in_range ? __expf(xl[j] - m[j]) * inv[j] + fix[j]
                       : __builtin_nanf(""));
    }
    // pass 2: prob, written once
    for (int c0 = 0; c0 < C; c0 += kStreamChunk) {
      float v[kStreamChunk][P];
#pragma unroll
      for (int k = 0; k < kStreamChunk; ++k)
        if (c0 + k < C) load_run<P>(x + q.x0 + (c0 + k) * plane, v[k]);
#pragma unroll
      for (int k = 0; k < kStreamChunk; ++k)
        if (c0 + k < C) {
#pragma unroll
          for (int j = 0; j < P; ++j)
            v[k][j] = __expf(v[k][j] - m[j]) * inv[j] + fix[j];
          store_run<P>(prob + q.x0 + (c0 + k) * plane, v[k]);
        }
    }
  }
  acc.store(partials);
}

// one block: thread k adds partial pairs k, k + kTPB, ... then the tree
__global__ void k_dsm_final(const double* __restrict__ partials, int np,
                            int mode, long outer, long inner,
                            float* __restrict__ loss,
                            float* __restrict__ norm_slot) {
  double sum = 0, valid = 0;  // counts are exact in a double
  for (int i = threadIdx.x; i < np; i += kTPB) {
    sum += partials[2 * i];
    valid += partials[2 * i + 1];
  }
  block_sum2(sum, valid);
  if (threadIdx.x == 0) {
    const double n = softmax_loss_normalizer(mode, outer, inner, (long)valid);
    loss[0] = (float)(sum / n);
    norm_slot[0] = (float)valid;
    norm_slot[1] = (float)(1.0 / n);
  }
}

// ---------------------------------------------------------------- backward
template <int P>
__global__ __launch_bounds__(kTPB) void k_dsm_bwd(
    const float* __restrict__ prob, const float* __restrict__ label,
    DenseSoftmax g, unsigned gpi, unsigned groups,
    const float* __restrict__ norm_slot, float loss_weight,
    float* __restrict__ dx) {
  const int C = g.C;
  const long plane = g.inner;
  const float scale = loss_weight * norm_slot[1];
  for (unsigned t = blockIdx.x * kTPB + threadIdx.x; t < groups;
       t += gridDim.x * kTPB) {
    const Group q = group_at<P>(t, gpi, C, g.inner);
    float lab[P];
    int lv[P];
    bool keep[P];
    load_run<P>(label + q.lab0, lab);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      lv[j] = (int)lab[j];
      keep[j] = !(g.has_ignore && lv[j] == g.ignore);
    }
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
      float p[P];
      load_run<P>(prob + q.x0 + c * plane, p);
#pragma unroll
      for (int j = 0; j < P; ++j)  // a select: NaN prob * 0 would be NaN
        p[j] = keep[j] ? (p[j] - (c == lv[j] ? 1.f : 0.f)) * scale : 0.f;
      store_run<P>(dx + q.x0 + c * plane, p);
    }
  }
}

// ------------------------------------------------------------------- plan
struct DsmPlan {
  bool stream;
  int CR, P;
  unsigned gpi, groups;
  int blocks;
};
static DsmPlan dsm_plan(const DenseSoftmax& g, const void* a, const void* b,
                        const void* c) {
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c;
  int vec = 1;
  if (g.inner % 4 == 0 && bits % 16 == 0)
    vec = 4;
  else if (g.inner % 2 == 0 && bits % 8 == 0)
    vec = 2;
  DsmPlan p;
  p.stream = g.C > kResidentMaxC;
  p.CR = p.stream ? 0 : g.C <= 4 ? 4 : g.C <= 8 ? 8 : g.C <= 16 ? 16 : 32;
  p.P = p.stream ? vec : std::min(vec, kResidentRegs / p.CR);
  p.gpi = (unsigned)(g.inner / p.P);
  p.groups = (unsigned)g.outer * p.gpi;
  p.blocks = (int)std::max<long>(
      1, std::min<long>(((long)p.groups + kTPB - 1) / kTPB, kDsmMaxBlocks));
  return p;
}
static void dsm_check(const DenseSoftmax& g) {
  CHECK_(g.outer > 0 && g.C > 0 && g.inner > 0 &&
         (long)g.outer * g.inner < (1L << 31))
      << "dense softmax loss: " << g.outer << " x " << g.C << " x " << g.inner
      << " is empty or has 2^31 pixels or more";
}
static void dsm_trace(int which, const DenseSoftmax& g, const DsmPlan& p) {
  kernel_trace_dsm(which, p.stream,
                   {p.CR, p.P, p.P, (long)g.outer * g.inner, g.C, p.blocks});
}

template <int CR, int P>
static void launch_fwd(hipStream_t s, const DsmPlan& p, const DenseSoftmax& g,
                       const float* x, const float* label, float* prob,
                       double* partials) {
  if constexpr (CR == 0)
    hipLaunchKernelGGL(k_dsm_fwd_stream<P>, dim3(p.blocks), dim3(kTPB), 0, s,
                       x, label, g, p.gpi, p.groups, prob, partials);
  else
    hipLaunchKernelGGL((k_dsm_fwd<CR, P>), dim3(p.blocks), dim3(kTPB), 0, s,
                       x, label, g, p.gpi, p.groups, prob, partials);
}
template <int CR>
static void launch_fwd_p(hipStream_t s, const DsmPlan& p,
                         const DenseSoftmax& g, const float* x,
                         const float* label, float* prob, double* partials) {
  if (p.P == 1) launch_fwd<CR, 1>(s, p, g, x, label, prob, partials);
  if (p.P == 2) launch_fwd<CR, 2>(s, p, g, x, label, prob, partials);
  if constexpr (CR * 4 <= kResidentRegs)
    if (p.P == 4) launch_fwd<CR, 4>(s, p, g, x, label, prob, partials);
}

}  // namespace

void dense_softmaxloss_fwd(hipStream_t s, const DenseSoftmax& g,
                           const float* x, const float* label, float* prob,
                           double* partials, float* loss_out,
                           float* norm_slot) {
  dsm_check(g);
  const DsmPlan p = dsm_plan(g, x, label, prob);
  const double px = (double)g.outer * g.inner;
  PerfScope perf(PERF_CLASS("dense_softmax_fwd"), s, 0,
                 4.0 * px * ((p.stream ? 3 : 2) * g.C + 1));
  switch (p.CR) {
    case 0: launch_fwd_p<0>(s, p, g, x, label, prob, partials); break;
    case 4: launch_fwd_p<4>(s, p, g, x, label, prob, partials); break;
    case 8: launch_fwd_p<8>(s, p, g, x, label, prob, partials); break;
    case 16: launch_fwd_p<16>(s, p, g, x, label, prob, partials); break;
    default: launch_fwd_p<32>(s, p, g, x, label, prob, partials); break;
  }
  hipLaunchKernelGGL(k_dsm_final, dim3(1), dim3(kTPB), 0, s,
                     (const double*)partials, p.blocks, g.norm, (long)g.outer,
                     (long)g.inner, loss_out, norm_slot);
  dsm_trace(0, g, p);
}

void dense_softmaxloss_bwd(hipStream_t s, const DenseSoftmax& g,
                           const float* prob, const float* label,
                           const float* norm_slot, float loss_weight,
                           float* dx) {
  dsm_check(g);
  const DsmPlan p = dsm_plan(g, prob, label, dx);
  PerfScope perf(PERF_CLASS("dense_softmax_bwd"), s, 0,
                 4.0 * g.outer * g.inner * (2.0 * g.C + 1));
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(p.blocks), dim3(kTPB), 0, s, prob, label,
                       g, p.gpi, p.groups, norm_slot, loss_weight, dx);
  };
  if (p.P == 1) launch(k_dsm_bwd<1>);
  if (p.P == 2) launch(k_dsm_bwd<2>);
  if (p.P == 4) launch(k_dsm_bwd<4>);
  dsm_trace(1, g, p);
}

// -------------------------------------------------------------------- Crop
// Both directions run over packs of V floats along the innermost axis, lanes
// adjacent there; V = 4 needs that axis's offset and both widths to be
// multiples of 4 (a pack is then wholly inside the window or wholly
// outside), else V = 1.  The index arithmetic is 32-bit.
namespace {

template <int V>
__global__ void k_crop_fwd(const float* __restrict__ x, CropGeom g,
                           unsigned packs, float* __restrict__ y) {
  const unsigned T3 = g.T[3] / V, B3 = g.B[3] / V, o3 = g.off[3] / V;
  for (unsigned i = blockIdx.x * kTPB + threadIdx.x; i < packs;
       i += gridDim.x * kTPB) {
    unsigned r = i / T3;
    const unsigned c3 = i - r * T3;
    const unsigned c2 = r % g.T[2];
    r /= g.T[2];
    const unsigned c1 = r % g.T[1];
    const unsigned c0 = r / g.T[1];
    const unsigned src =
        (((c0 + g.off[0]) * g.B[1] + c1 + g.off[1]) * g.B[2] + c2 +
         g.off[2]) * B3 + c3 + o3;
    float v[V];
    load_run<V>(x + (long)src * V, v);
    store_run<V>(y + (long)i * V, v);
  }
}

// over the bottom's packs: the top diff inside the window, zero outside
template <int V>
__global__ void k_crop_bwd(const float* __restrict__ dy, CropGeom g,
                           unsigned packs, float* __restrict__ dx) {
  const unsigned T3 = g.T[3] / V, B3 = g.B[3] / V, o3 = g.off[3] / V;
  for (unsigned i = blockIdx.x * kTPB + threadIdx.x; i < packs;
       i += gridDim.x * kTPB) {
    unsigned r = i / B3;
    // unsigned: a coordinate before the window wraps past T
    const unsigned c3 = i - r * B3 - o3;
    const unsigned c2 = r % g.B[2] - g.off[2];
    r /= g.B[2];
    const unsigned c1 = r % g.B[1] - g.off[1];
    const unsigned c0 = r / g.B[1] - g.off[0];
    float v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = 0.f;
    if (c3 < T3 && c2 < g.T[2] && c1 < g.T[1] && c0 < g.T[0]) {
      const unsigned src = ((c0 * g.T[1] + c1) * g.T[2] + c2) * T3 + c3;
      load_run<V>(dy + (long)src * V, v);
    }
    store_run<V>(dx + (long)i * V, v);
  }
}

static int crop_vec(const CropGeom& g, const void* a, const void* b) {
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b;
  return (g.B[3] % 4 == 0 && g.T[3] % 4 == 0 && g.off[3] % 4 == 0 &&
          bits % 16 == 0) ? 4 : 1;
}
static long crop_count(const unsigned (&d)[4]) {
  return (long)d[0] * d[1] * d[2] * d[3];
}
static void crop_check(const CropGeom& g) {
  for (int i = 0; i < 4; ++i)
    CHECK_(g.T[i] > 0 && (long)g.off[i] + g.T[i] <= (long)g.B[i])
        << "crop: window " << g.off[i] << " + " << g.T[i]
        << " leaves collapsed axis " << i << " of size " << g.B[i];
  CHECK_(crop_count(g.B) < (1L << 31))
      << "crop: a bottom of 2^31 elements or more";
}
static int crop_blocks(long packs) {
  return (int)std::max<long>(1, std::min<long>((packs + kTPB - 1) / kTPB,
                                               2048));
}

}  // namespace

void crop_fwd(hipStream_t s, const CropGeom& g, const float* x, float* y) {
  crop_check(g);
  const long n = crop_count(g.T);
  PerfScope perf(PERF_CLASS("crop"), s, 0, 8.0 * n);
  const int V = crop_vec(g, x, y);
  const unsigned packs = (unsigned)(n / V);
  if (V == 4)
    hipLaunchKernelGGL(k_crop_fwd<4>, dim3(crop_blocks(packs)), dim3(kTPB), 0,
                       s, x, g, packs, y);
  else
    hipLaunchKernelGGL(k_crop_fwd<1>, dim3(crop_blocks(packs)), dim3(kTPB), 0,
                       s, x, g, packs, y);
}

void crop_bwd(hipStream_t s, const CropGeom& g, const float* dy, float* dx) {
  crop_check(g);
  const long n = crop_count(g.B);
  PerfScope perf(PERF_CLASS("crop"), s, 0, 4.0 * (n + crop_count(g.T)));
  const int V = crop_vec(g, dy, dx);
  const unsigned packs = (unsigned)(n / V);
  if (V == 4)
    hipLaunchKernelGGL(k_crop_bwd<4>, dim3(crop_blocks(packs)), dim3(kTPB), 0,
                       s, dy, g, packs, dx);
  else
    hipLaunchKernelGGL(k_crop_bwd<1>, dim3(crop_blocks(packs)), dim3(kTPB), 0,
                       s, dy, g, packs, dx);
}

}  // namespace gpu
}  // namespace camd
