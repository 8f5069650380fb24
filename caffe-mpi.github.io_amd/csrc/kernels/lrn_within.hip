// lrn_within.hip — gfx950 kernels for LRN with norm_region WITHIN_CHANNEL.
//
// For x[N][C][H][W], odd local_size k and pre = (k - 1) / 2:
//   s  = 1 + alpha / k^2 * Σ_{|dh|,|dw| <= pre} x[h+dh][w+dw]^2   (zero outside
//        the plane; the divisor is k^2 at the border too)
//   y  = x * s^-beta
//   dx = dy * s^-beta - 2 alpha beta / k^2 * x * Σ_window(dy * x * s^(-beta-1))
// The reference composes this from Split, Power, AVE Pooling, Power and
// Eltwise PROD (lrn_layer.cpp:17-65): five launches and four intermediates
// each way.  Here each direction is one stencil pass.  Forward reads x and
// writes y and s (12 B per element); backward reads x, dy and s, recomputes
// s^-beta instead of reading y, and writes dx (16 B per element).  No
// atomics, a fixed summation order: a rerun gives the same bits.
//
// A block of 256 threads owns P slots in LDS, each a TH x TW region of one
// (n, c) plane with a pre-wide halo on every side, zero where it leaves the
// plane.  Two work splits share the one kernel body:
//   planes  wherever a whole plane's backward slot fits the LDS budget: the
//           slot is the plane (TH, TW = H, W rounded up to kSeg) and a block
//           takes P planes, as many as give every thread a column walk (at
//           most kMaxPlanes).  Every slot has its own zero halo, so
//           neighbouring planes never meet.
//   tiles   larger planes: P = 1, the slot is one kTileH x kTileW tile of one
//           plane; edge tiles are partial on both axes.
// Whole planes won where both serve (55 x 55, k = 5: 64 against 71 us
// forward, 81 against 93 us backward at 32 x 96 planes), so the LDS budget
// is the only threshold.
// The window sum is separable and takes three steps with a barrier between:
//   stage       the slot's operand (x forward, t = dy*x*s^(-beta-1) backward)
//               with its halo, lanes adjacent along W; backward also keeps x
//               and u = dy*s^-beta of the slot's interior.
//   horizontal  a thread walks kSeg adjacent columns of one row (x squared on
//               the way in forward) and writes the k-wide row sums.  Lanes
//               are adjacent along the rows, and both row pitches are odd,
//               so neither side has a bank conflict.
//   vertical    a thread walks kSeg adjacent rows of one column of the row
//               sums, lanes adjacent along W, and writes its kSeg pixels.
// k = 3 holds the kSeg + 2 operands of a walk in registers and adds each
// window directly; any other k slides a running sum (add the entering term,
// subtract the leaving one): O(1) LDS reads per pixel for every k.  A k = 5
// body of the first kind was measured no faster than the sliding one and was
// cut; the k = 3 one gains 5 % on 8 x 8 planes (profiles/lrn_within.txt).
//
// The largest local_size is kLrnWithinMaxSize = 41 (math.hpp): the backward
// slot of one kTileH x kTileW tile with a 20-wide halo is the last that fits
// the 64 KB of LDS a block may take.  Index arithmetic inside a plane is
// 32-bit; only the plane's base offset is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "../math.hpp"

namespace camd {
namespace gpu {
namespace {

constexpr int kTPB = 256;
constexpr int kSeg = 4;           // pixels a thread walks, either pass
constexpr int kTileH = 32, kTileW = 64;
constexpr int kMaxPlanes = 32;    // slots per block, planes split
constexpr int kLdsFloats = 16384;  // 64 KB

constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
constexpr int round_up(int a, int b) { return ceil_div(a, b) * b; }
// row pitches: odd, so lanes a row apart fall into different banks
constexpr int pitch_x(int tw, int pre) { return (tw + 2 * pre) | 1; }
constexpr int pitch_h(int tw) { return tw | 1; }
// floats of one backward slot (forward needs 2 * th * tw fewer; one plan
// serves both directions, so both are sized by this)
constexpr long slot_floats(int th, int tw, int pre) {
  return (long)(th + 2 * pre) * (pitch_x(tw, pre) + pitch_h(tw)) +
         2L * th * tw;
}
static_assert(slot_floats(kTileH, kTileW, (kLrnWithinMaxSize - 1) / 2) <=
                      kLdsFloats &&
                  slot_floats(kTileH, kTileW, (kLrnWithinMaxSize + 1) / 2) >
                      kLdsFloats,
              "kLrnWithinMaxSize is the last local_size whose tile fits");
static_assert(kTileH % kSeg == 0 && kTileW % kSeg == 0, "whole walks");

// the block's slots: first plane and the tile's origin in the plane
struct Block {
  int pl0, r0, c0;
};
__device__ __forceinline__ Block block_at(const LrnWithinPlan& t) {
  const unsigned tiles = t.ty * t.tx;
  const unsigned pb = blockIdx.x / tiles;
  const unsigned tl = blockIdx.x - pb * tiles;
  const unsigned tyi = fastdiv(tl, t.fd_tx);
  return {(int)(pb * t.P), (int)(tyi * t.TH), (int)((tl - tyi * t.tx) * t.TW)};
}

// out[i] = Σ_{j < k} f(in[(i + j) * stride]) for i < kSeg; K = 0: runtime k
template <int K, bool SQUARE>
__device__ __forceinline__ void window_walk(const float* __restrict__ in,
                                            int stride, int k,
                                            float (&out)[kSeg]) {
  auto f = [](float v) { return SQUARE ? v * v : v; };
  if constexpr (K > 0) {
    float v[kSeg + K - 1];
#pragma unroll
    for (int j = 0; j < kSeg + K - 1; ++j) v[j] = f(in[j * stride]);
#pragma unroll
    for (int i = 0; i < kSeg; ++i) {
      float a = v[i];
#pragma unroll
      for (int j = 1; j < K; ++j) a += v[i + j];
      out[i] = a;
    }
  } else {
    float a = 0.f;
    for (int j = 0; j < k; ++j) a += f(in[j * stride]);
    out[0] = a;
#pragma unroll
    for (int i = 1; i < kSeg; ++i) {
      a += f(in[(i + k - 1) * stride]) - f(in[(i - 1) * stride]);
      out[i] = a;
    }
  }
}

// hs[p][r][c] = Σ_{j < k} f(xs[p][r][c + j]) over the slot's LH rows: items
// (p, column segment, row) with the row fastest across lanes
template <int K, bool SQUARE>
__device__ __forceinline__ void horizontal_pass(const LrnWithinPlan& t, int k,
                                                const float* __restrict__ xs,
                                                float* __restrict__ hs) {
  const int segs = t.TW / kSeg;
  const int items = t.P * segs * t.LH;
  const int PX = pitch_x(t.TW, (k - 1) / 2), PH = pitch_h(t.TW);
  for (int it = threadIdx.x; it < items; it += kTPB) {
    const int pq = (int)fastdiv(it, t.fd_lh);
    const int r = it - pq * t.LH;
    const int p = (int)fastdiv(pq, t.fd_segs_w);
    const int q = pq - p * segs;
    float out[kSeg];
    window_walk<K, SQUARE>(xs + (p * t.LH + r) * PX + q * kSeg, 1, k, out);
    float* o = hs + (p * t.LH + r) * PH + q * kSeg;
#pragma unroll
    for (int i = 0; i < kSeg; ++i) o[i] = out[i];
  }
}

// The vertical pass hands every pixel of the block to `emit` once with its
// window sum: items (p, row segment, column), the column fastest.
template <int K, typename Emit>
__device__ __forceinline__ void vertical_pass(const LrnWithin& g,
                                              const LrnWithinPlan& t,
                                              const Block& b,
                                              const float* __restrict__ hs,
                                              Emit emit) {
  const int segs = t.TH / kSeg;
  const int items = t.P * segs * t.TW;
  const int PH = pitch_h(t.TW);
  for (int it = threadIdx.x; it < items; it += kTPB) {
    const int pq = (int)fastdiv(it, t.fd_tw);
    const int c = it - pq * t.TW;
    const int p = (int)fastdiv(pq, t.fd_segs_h);
    const int q = pq - p * segs;
    const int pl = b.pl0 + p, h0 = b.r0 + q * kSeg, w = b.c0 + c;
    if (pl >= g.planes || h0 >= g.H || w >= g.W) continue;
    float sum[kSeg];
    window_walk<K, false>(hs + (p * t.LH + q * kSeg) * PH + c, PH, g.size,
                          sum);
#pragma unroll
    for (int i = 0; i < kSeg; ++i)
      if (h0 + i < g.H)
        emit(p, q * kSeg + i, c, (long)pl * g.H * g.W + (h0 + i) * g.W + w,
             sum[i]);
  }
}

// ---------------------------------------------------------------- forward
template <int K>
__global__ __launch_bounds__(kTPB) void k_lrn_within_fwd(
    LrnWithin g, LrnWithinPlan t, const float* __restrict__ x,
    float* __restrict__ scale, float* __restrict__ y) {
  extern __shared__ float lds[];
  const int pre = (g.size - 1) / 2;
  const int PX = pitch_x(t.TW, pre);
  const int per = t.LH * PX;
  float* xs = lds;              // [P][LH][PX], raw x
  float* hs = lds + t.P * per;  // [P][LH][PH]
  const Block b = block_at(t);
  for (int i = threadIdx.x; i < t.P * per; i += kTPB) {
    const int p = (int)fastdiv(i, t.fd_per);
    const int rem = i - p * per;
    const int r = (int)fastdiv(rem, t.fd_px);
    const int h = b.r0 - pre + r, w = b.c0 - pre + (rem - r * PX);
    const int pl = b.pl0 + p;
    float v = 0.f;
    if (pl < g.planes && (unsigned)h < (unsigned)g.H &&
        (unsigned)w < (unsigned)g.W)
      v = x[(long)pl * g.H * g.W + h * g.W + w];
    xs[i] = v;
  }
  __syncthreads();
  horizontal_pass<K, true>(t, g.size, xs, hs);
  __syncthreads();
  const float aos = g.alpha / (float)(g.size * g.size);
  vertical_pass<K>(g, t, b, hs, [&](int p, int r, int c, long o, float sum) {
    const float s = 1.f + aos * sum;
    scale[o] = s;
    y[o] = xs[p * per + (r + pre) * PX + c + pre] * __powf(s, -g.beta);
  });
}

// --------------------------------------------------------------- backward
template <int K>
__global__ __launch_bounds__(kTPB) void k_lrn_within_bwd(
    LrnWithin g, LrnWithinPlan t, const float* __restrict__ x,
    const float* __restrict__ dy, const float* __restrict__ scale,
    float* __restrict__ dx) {
  extern __shared__ float lds[];
  const int pre = (g.size - 1) / 2;
  const int PX = pitch_x(t.TW, pre);
  const int per = t.LH * PX;
  const int inner = t.TH * t.TW;
  float* ts = lds;                            // [P][LH][PX], t with halo
  float* hs = ts + t.P * per;                 // [P][LH][PH]
  float* xi = hs + t.P * t.LH * pitch_h(t.TW);  // [P][TH][TW], x
  float* ui = xi + t.P * inner;               // [P][TH][TW], dy * s^-beta
  const Block b = block_at(t);
  for (int i = threadIdx.x; i < t.P * per; i += kTPB) {
    const int p = (int)fastdiv(i, t.fd_per);
    const int rem = i - p * per;
    const int r = (int)fastdiv(rem, t.fd_px);
    const int c = rem - r * PX;
    const int h = b.r0 - pre + r, w = b.c0 - pre + c;
    const int pl = b.pl0 + p;
    float xv = 0.f, u = 0.f, tv = 0.f;
    if (pl < g.planes && (unsigned)h < (unsigned)g.H &&
        (unsigned)w < (unsigned)g.W) {
      const long o = (long)pl * g.H * g.W + h * g.W + w;
      const float s = scale[o];
      xv = x[o];
      u = dy[o] * __powf(s, -g.beta);
      tv = u * xv / s;
    }
    ts[i] = tv;
    const unsigned ri = r - pre, ci = c - pre;  // wraps in the halo
    if (ri < (unsigned)t.TH && ci < (unsigned)t.TW) {
      xi[p * inner + ri * t.TW + ci] = xv;
      ui[p * inner + ri * t.TW + ci] = u;
    }
  }
  __syncthreads();
  horizontal_pass<K, false>(t, g.size, ts, hs);
  __syncthreads();
  const float cr = 2.f * g.alpha * g.beta / (float)(g.size * g.size);
  vertical_pass<K>(g, t, b, hs, [&](int p, int r, int c, long o, float sum) {
    const int i = p * inner + r * t.TW + c;
    dx[o] = ui[i] - cr * xi[i] * sum;
  });
}

}  // namespace

LrnWithinPlan lrn_within_plan(const LrnWithin& g) {
  CHECK_(g.planes > 0 && g.H > 0 && g.W > 0 && (long)g.H * g.W < (1L << 30))
      << "within-channel LRN: " << g.planes << " planes of " << g.H << " x "
      << g.W << " are empty or have 2^30 pixels or more";
  CHECK_(g.size % 2 == 1 && g.size >= 1 && g.size <= kLrnWithinMaxSize)
      << "within-channel LRN: local_size " << g.size
      << " is even or above " << kLrnWithinMaxSize;
  const int pre = (g.size - 1) / 2;
  // For measurement (profiles/lrn_within.txt): CAFFE_LRN_WITHIN_TILES=1
  // tiles a plane that would go whole, CAFFE_LRN_WITHIN_GENERIC=1 gives
  // k = 3 the generic body
  const char* te = getenv("CAFFE_LRN_WITHIN_TILES");
  const char* ge = getenv("CAFFE_LRN_WITHIN_GENERIC");
  const int PH = round_up(g.H, kSeg), PW = round_up(g.W, kSeg);
  const bool planes =
      slot_floats(PH, PW, pre) <= kLdsFloats && !(te && atoi(te));
  LrnWithinPlan t{};
  t.var = g.size == 3 && !(ge && atoi(ge)) ? 0 : 1;
  t.tiled = !planes;
  t.TH = planes ? PH : kTileH;
  t.TW = planes ? PW : kTileW;
  t.ty = planes ? 1 : ceil_div(g.H, kTileH);
  t.tx = planes ? 1 : ceil_div(g.W, kTileW);
  t.LH = t.TH + 2 * pre;
  t.P = 1;
  if (planes) {
    const int walks = (t.TH / kSeg) * t.TW;  // vertical walks of one plane
    t.P = std::min(g.planes, std::max(1, std::min(kMaxPlanes, kTPB / walks)));
    while (t.P > 1 && t.P * slot_floats(t.TH, t.TW, pre) > kLdsFloats) --t.P;
  }
  const long blocks = (long)ceil_div(g.planes, t.P) * t.ty * t.tx;
  CHECK_(blocks < (1L << 31)) << "within-channel LRN: " << blocks
                              << " blocks do not fit a grid";
  t.blocks = (int)blocks;
  const int PX = pitch_x(t.TW, pre);
  t.fd_per = fastdiv_make((unsigned long)t.LH * PX);
  t.fd_px = fastdiv_make(PX);
  t.fd_lh = fastdiv_make(t.LH);
  t.fd_tw = fastdiv_make(t.TW);
  t.fd_segs_w = fastdiv_make(t.TW / kSeg);
  t.fd_segs_h = fastdiv_make(t.TH / kSeg);
  t.fd_tx = fastdiv_make(t.tx);
  return t;
}

void lrn_within_fwd(hipStream_t s, const LrnWithin& g, const LrnWithinPlan& t,
                    const float* x, float* scale, float* y) {
  PerfScope perf(PERF_CLASS("lrn"), s, 0, 12.0 * g.planes * g.H * g.W);
  const int pre = (g.size - 1) / 2;
  const size_t lds =
      sizeof(float) * t.P * (slot_floats(t.TH, t.TW, pre) - 2L * t.TH * t.TW);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(t.blocks), dim3(kTPB), lds, s, g, t, x,
                       scale, y);
  };
  if (t.var == 0) launch(k_lrn_within_fwd<3>);
  if (t.var == 1) launch(k_lrn_within_fwd<0>);
  kernel_trace_lrn_within(0, t.var, t.tiled, t.P, t.ty, t.tx, t.blocks);
}

void lrn_within_bwd(hipStream_t s, const LrnWithin& g, const LrnWithinPlan& t,
                    const float* x, const float* dy, const float* scale,
                    float* dx) {
  PerfScope perf(PERF_CLASS("lrn"), s, 0, 16.0 * g.planes * g.H * g.W);
  const int pre = (g.size - 1) / 2;
  const size_t lds = sizeof(float) * t.P * slot_floats(t.TH, t.TW, pre);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(t.blocks), dim3(kTPB), lds, s, g, t, x, dy,
                       scale, dx);
  };
  if (t.var == 0) launch(k_lrn_within_bwd<3>);
  if (t.var == 1) launch(k_lrn_within_bwd<0>);
  kernel_trace_lrn_within(1, t.var, t.tiled, t.P, t.ty, t.tx, t.blocks);
}

}  // namespace gpu
}  // namespace camd
