// prelu.hip — gfx950 kernels for the PReLU layer (prelu_layer.cpp).
//
// For x[N][C][S] and slopes a[C] (a[1] when channel_shared):
//   y     = x > 0 ? x : a[c] * x
//   dx    = dy * (x > 0 ? 1 : a[c])
//   da[c] = Σ_{n,s} dy * x * [x <= 0]
// The reference's backward is a masked-product kernel and a GEMV per image
// plus a dx kernel, and its in-place forward copies the tensor first
// (prelu_layer.cu:64-128): N + 2 launches, about five passes.  Here forward
// is one pass (8 B per element, 12 in-place: the saved x leaves with the
// same load) and backward one pass (12 B per element, 8 without dx) plus a
// finalize over the partials.  The parameter sum is two-stage, in double,
// in a fixed order, without atomics: a rerun gives the same bits.
//
// Three layouts, chosen once per Reshape by prelu_plan():
//   v4      S % 4 == 0.  A float4 never straddles a plane, so a block's
//           slope is one scalar load.  A plane is cut into `chunks` pieces
//           of `clen` float4 loads (one piece up to kChunk loads; the last
//           may be shorter), the N * chunks pieces of a channel are its
//           rows, and a block owns one channel and one slice of `rps` rows.
//           It walks them as one flat index, kUnroll loads of x and dy in
//           flight per thread; two exact fast divisions turn the index into
//           (image, piece, offset).  Cutting planes, not only the batch,
//           fills the device at N = 1 (a super-resolution net at test
//           time).
//   scalar  S > 1 and S % 4 != 0: planes start unaligned.  The same
//           ownership and walk with float loads (a load is then 4 B per
//           lane; the aligned-body form with masked head and tail packs
//           was not built).
//   cols    S == 1: x is [N][C], the channel is the fastest axis.  A lane
//           owns a column, or a float4 of columns when C % 4 == 0, and keeps
//           its slopes in registers; the four waves of a block walk
//           interleaved rows of the block's row slice, so a wave's load is
//           one contiguous run along C and no lane ever adds another lane's
//           column.  The waves meet once in LDS.
// Backward writes one double per (slice, channel) into the kPReluPart
// workspace slot, [slice][C]: v4 and scalar reduce the block with wave
// shuffles and one LDS exchange, cols adds its four waves per column.
// k_prelu_final adds a channel's slices, a wave per channel, and writes the
// float da[c]; channel_shared, one block adds every partial into da[0].
// Both in a fixed order.
//
// Element offsets are 64-bit; a block's flat index, the rows of a channel
// and the grid are checked below 2^31 by the plan.  x, dy and dx carry no
// __restrict__: in-place, y is x and dx may be dy.  Every thread loads its
// packs of a pass before it stores any.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../layers.hpp"
#include "../math.hpp"

namespace camd {
namespace gpu {
namespace {

using f4 = __attribute__((ext_vector_type(4))) float;
template <typename V>
constexpr int kLanes = sizeof(V) / sizeof(float);
__device__ __forceinline__ float lane(float v, int) { return v; }
__device__ __forceinline__ float lane(f4 v, int j) { return v[j]; }
__device__ __forceinline__ void put(float& v, int, float s) { v = s; }
__device__ __forceinline__ void put(f4& v, int j, float s) { v[j] = s; }

constexpr int kTPB = kPReluThreads;
constexpr int kWave = 64;
constexpr int kWaves = kTPB / kWave;
constexpr int kUnroll = 4;  // loads of each operand in flight per thread
static_assert(kPReluChunk == kTPB * kUnroll, "a piece is one unrolled pass");
static_assert(kPReluColsPerBlock == kWave, "a lane per column pack");

// ------------------------------------------------------------ v4, scalar
// What a block owns: channel c and the flat loads [0, span) of its rows
struct Rows {
  unsigned c, r0, span;
};
__device__ __forceinline__ Rows rows_of_block(const PRelu& g,
                                              const PReluPlan& t) {
  const unsigned c = blockIdx.x % (unsigned)g.C;
  const unsigned slice = blockIdx.x / (unsigned)g.C;
  const unsigned r0 = slice * t.rps;
  const unsigned r1 = min((unsigned)t.rows, r0 + t.rps);
  return {c, r0, (r1 - r0) * t.clen};
}
// the offset, in loads, of the block's i-th load; -1 past the block's rows
// or past the end of a plane's short last piece
__device__ __forceinline__ long load_at(const PRelu& g, const PReluPlan& t,
                                        const Rows& b, unsigned i) {
  if (i >= b.span) return -1;
  const unsigned lr = fastdiv(i, t.fd_clen);
  const unsigned row = b.r0 + lr;
  const unsigned n = fastdiv(row, t.fd_chunks);
  const unsigned p = (row - n * t.chunks) * t.clen + (i - lr * t.clen);
  if (p >= (unsigned)t.per) return -1;
  return ((long)n * g.C + b.c) * t.per + p;
}

// INPLACE: y is x; the loaded x also goes to `saved` for the backward
template <typename V, bool INPLACE>
__global__ __launch_bounds__(kTPB) void k_prelu_fwd(
    PRelu g, PReluPlan t, const V* x, const float* __restrict__ a, V* y,
    V* saved) {
  const Rows b = rows_of_block(g, t);
  const float ac = a[g.shared ? 0 : b.c];
  for (unsigned i0 = threadIdx.x; i0 < b.span; i0 += kUnroll * kTPB) {
    long o[kUnroll];
    V v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      o[u] = load_at(g, t, b, i0 + u * kTPB);
      if (o[u] >= 0) v[u] = x[o[u]];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (o[u] < 0) continue;
      if (INPLACE) saved[o[u]] = v[u];
#pragma unroll
      for (int j = 0; j < kLanes<V>; ++j)
        put(v[u], j, prelu_value(lane(v[u], j), ac));
      y[o[u]] = v[u];
    }
  }
}

// the block's sum into thread 0: shuffles inside a wave, then one exchange
template <int WAVES>
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double red[WAVES];
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
    v += __shfl_down(v, off, kWave);
  if (threadIdx.x % kWave == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  double sum = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) sum += red[w];
  return sum;
}

// DX: dx is wanted (and may be dy)
template <typename V, bool DX>
__global__ __launch_bounds__(kTPB) void k_prelu_bwd(
    PRelu g, PReluPlan t, const V* x, const V* dy,
    const float* __restrict__ a, V* dx, double* __restrict__ part) {
  const Rows b = rows_of_block(g, t);
  const float ac = a[g.shared ? 0 : b.c];
  double acc = 0;
  for (unsigned i0 = threadIdx.x; i0 < b.span; i0 += kUnroll * kTPB) {
    long o[kUnroll];
    V xv[kUnroll], dv[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      o[u] = load_at(g, t, b, i0 + u * kTPB);
      if (o[u] >= 0) {
        xv[u] = x[o[u]];
        dv[u] = dy[o[u]];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (o[u] < 0) continue;
#pragma unroll
      for (int j = 0; j < kLanes<V>; ++j) {
        const float xj = lane(xv[u], j), dj = lane(dv[u], j);
        acc += prelu_da_term(xj, dj);
        put(dv[u], j, prelu_dx(xj, dj, ac));
      }
      if (DX) dx[o[u]] = dv[u];
    }
  }
  const double sum = block_sum<kWaves>(acc);
  if (threadIdx.x == 0)
    part[(long)(blockIdx.x / (unsigned)g.C) * g.C + b.c] = sum;
}

// ------------------------------------------------------------------ cols
// What a thread owns: column pack `col` (dead past the last one) and the
// rows r0 + wave, r0 + wave + kWaves, .. below r1
struct Cols {
  unsigned col, slice;
  bool live;
  long r0, r1;
};
template <typename V>
__device__ __forceinline__ Cols cols_of_thread(const PRelu& g,
                                               const PReluPlan& t,
                                               float (&al)[kLanes<V>],
                                               const float* a) {
  const unsigned cb = blockIdx.x % (unsigned)t.cb;
  const unsigned slice = blockIdx.x / (unsigned)t.cb;
  const unsigned col = cb * kWave + threadIdx.x % kWave;
  const bool live = col < (unsigned)t.per;
#pragma unroll
  for (int j = 0; j < kLanes<V>; ++j)
    al[j] = live ? a[g.shared ? 0 : col * kLanes<V> + j] : 0.f;
  const long r0 = (long)slice * t.rps;
  const long r1 = r0 + t.rps < t.rows ? r0 + t.rps : t.rows;
  return {col, slice, live, r0 + threadIdx.x / kWave, r1};
}

template <typename V, bool INPLACE>
__global__ __launch_bounds__(kTPB) void k_prelu_cols_fwd(
    PRelu g, PReluPlan t, const V* x, const float* __restrict__ a, V* y,
    V* saved) {
  float al[kLanes<V>];
  const Cols b = cols_of_thread<V>(g, t, al, a);
  if (!b.live) return;
  for (long r = b.r0; r < b.r1; r += kUnroll * kWaves) {
    V v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (r + u * kWaves < b.r1) v[u] = x[(r + u * kWaves) * t.per + b.col];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (r + u * kWaves >= b.r1) continue;
      const long o = (r + u * kWaves) * t.per + b.col;
      if (INPLACE) saved[o] = v[u];
#pragma unroll
      for (int j = 0; j < kLanes<V>; ++j)
        put(v[u], j, prelu_value(lane(v[u], j), al[j]));
      y[o] = v[u];
    }
  }
}

template <typename V, bool DX>
__global__ __launch_bounds__(kTPB) void k_prelu_cols_bwd(
    PRelu g, PReluPlan t, const V* x, const V* dy,
    const float* __restrict__ a, V* dx, double* __restrict__ part) {
  constexpr int L = kLanes<V>;
  float al[L];
  const Cols b = cols_of_thread<V>(g, t, al, a);
  double acc[L] = {};
  for (long r = b.r0; b.live && r < b.r1; r += kUnroll * kWaves) {
    V xv[kUnroll], dv[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (r + u * kWaves < b.r1) {
        const long o = (r + u * kWaves) * t.per + b.col;
        xv[u] = x[o];
        dv[u] = dy[o];
      }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (r + u * kWaves >= b.r1) continue;
#pragma unroll
      for (int j = 0; j < L; ++j) {
        const float xj = lane(xv[u], j), dj = lane(dv[u], j);
        acc[j] += prelu_da_term(xj, dj);
        put(dv[u], j, prelu_dx(xj, dj, al[j]));
      }
      if (DX) dx[(r + u * kWaves) * t.per + b.col] = dv[u];
    }
  }
  // the block's waves hold the same columns: add them in wave order
  __shared__ double red[kWaves][L][kWave];
  const int w = threadIdx.x / kWave, ln = threadIdx.x % kWave;
#pragma unroll
  for (int j = 0; j < L; ++j) red[w][j][ln] = acc[j];
  __syncthreads();
  if (w != 0 || !b.live) return;
#pragma unroll
  for (int j = 0; j < L; ++j) {
    double sum = red[0][j][ln];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) sum += red[k][j][ln];
    part[(long)b.slice * g.C + b.col * L + j] = sum;
  }
}

// ------------------------------------------------------------- finalize
// da[c] = Σ_slice part[slice][c]: a wave per channel, lane l adds slices l,
// l + 64, .. in that order and the shuffle tree adds the lanes.  (A thread
// per channel walking its slices one dependent load after another cost
// 0.3 us a slice: 13 of the backward's 66 us at 128 x 64 x 56 x 56.)
__global__ __launch_bounds__(kTPB) void k_prelu_final(
    const double* __restrict__ part, int C, int slices,
    float* __restrict__ da) {
  const int ln = threadIdx.x % kWave;
  for (long c = blockIdx.x * (long)kWaves + threadIdx.x / kWave; c < C;
       c += (long)gridDim.x * kWaves) {
    double sum = 0;
    for (int sl = ln; sl < slices; sl += kWave) sum += part[(long)sl * C + c];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
      sum += __shfl_down(sum, off, kWave);
    if (ln == 0) da[c] = (float)sum;
  }
}
// channel_shared: every partial goes into the one da.  One block; thread k
// adds partials k, k + kFinalThreads, .. in that order, then block_sum.
constexpr int kFinalThreads = 1024;
__global__ __launch_bounds__(kFinalThreads) void k_prelu_final_shared(
    const double* __restrict__ part, long n, float* __restrict__ da) {
  double acc = 0;
  for (long i = threadIdx.x; i < n; i += kFinalThreads) acc += part[i];
  const double sum = block_sum<kFinalThreads / kWave>(acc);
  if (threadIdx.x == 0) da[0] = (float)sum;
}

constexpr long ceil_div(long a, long b) { return (a + b - 1) / b; }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename V, bool INPLACE>
void launch_fwd(hipStream_t s, const PRelu& g, const PReluPlan& t,
                const float* x, const float* a, float* y, float* saved) {
  auto kernel = t.var == kPReluCols ? k_prelu_cols_fwd<V, INPLACE>
                                    : k_prelu_fwd<V, INPLACE>;
  hipLaunchKernelGGL(kernel, dim3(t.blocks), dim3(kTPB), 0, s, g, t,
                     (const V*)x, a, (V*)y, (V*)saved);
}
template <typename V, bool DX>
void launch_bwd(hipStream_t s, const PRelu& g, const PReluPlan& t,
                const float* x, const float* dy, const float* a, float* dx,
                double* part) {
  auto kernel = t.var == kPReluCols ? k_prelu_cols_bwd<V, DX>
                                    : k_prelu_bwd<V, DX>;
  hipLaunchKernelGGL(kernel, dim3(t.blocks), dim3(kTPB), 0, s, g, t,
                     (const V*)x, (const V*)dy, a, (V*)dx, part);
}

}  // namespace

PReluPlan prelu_plan(const PRelu& g) {
  CHECK_(g.N > 0 && g.C > 0 && g.S > 0 && g.N < kFastDivLimit &&
         g.S < kFastDivLimit)
      << "PReLU: " << g.N << " x " << g.C << " x " << g.S
      << " is empty or has an axis of 2^31 or more";
  PReluPlan t{};
  long want;  // slices that would fill the device
  if (g.S == 1) {
    t.var = kPReluCols;
    t.vec = g.C % 4 == 0 ? 4 : 1;
    t.per = g.C / t.vec;
    t.chunks = t.clen = 1;
    t.cb = (int)ceil_div(t.per, kPReluColsPerBlock);
    t.rows = (int)g.N;
    // a slice of fewer rows would write more partials than it saves time
    want = std::min<long>(std::max(1, kPReluBlocks / t.cb),
                          ceil_div(g.N, kPReluColsMinRows));
  } else {
    t.var = g.S % 4 == 0 ? kPReluV4 : kPReluScalar;
    t.vec = t.var == kPReluV4 ? 4 : 1;
    t.per = (int)(g.S / t.vec);
    t.chunks = (int)ceil_div(t.per, kPReluChunk);
    t.clen = (int)ceil_div(t.per, t.chunks);
    t.cb = g.C;
    const long rows = g.N * t.chunks;
    CHECK_(rows < kFastDivLimit)
        << "PReLU: " << rows << " plane pieces per channel";
    t.rows = (int)rows;
    want = std::max(1, kPReluBlocks / g.C);
  }
  t.rps = (int)ceil_div(t.rows, std::min<long>(want, t.rows));
  t.slices = (int)ceil_div(t.rows, t.rps);
  const long blocks = (long)t.cb * t.slices;
  CHECK_(blocks < kFastDivLimit && (long)t.rps * t.clen < kFastDivLimit)
      << "PReLU: " << blocks << " blocks of " << (long)t.rps * t.clen
      << " loads do not fit 32-bit indices";
  t.blocks = (int)blocks;
  t.fd_clen = fastdiv_make(t.clen);
  t.fd_chunks = fastdiv_make(t.chunks);
  return t;
}

void prelu_fwd(hipStream_t s, const PRelu& g, const PReluPlan& t,
               const float* x, const float* a, float* y, float* saved) {
  const double n = (double)g.N * g.C * g.S;
  PerfScope perf(PERF_CLASS("prelu"), s, 0, (saved ? 12.0 : 8.0) * n);
  CHECK_(!saved || x == y) << "PReLU forward: a saved copy is for in-place";
  CHECK_(t.vec == 1 || (aligned16(x) && aligned16(y) && aligned16(saved)))
      << "PReLU forward: float4 layout on an unaligned tensor";
  if (t.vec == 4)
    saved ? launch_fwd<f4, true>(s, g, t, x, a, y, saved)
          : launch_fwd<f4, false>(s, g, t, x, a, y, saved);
  else
    saved ? launch_fwd<float, true>(s, g, t, x, a, y, saved)
          : launch_fwd<float, false>(s, g, t, x, a, y, saved);
  kernel_trace_prelu(0, t.var, t.vec, t.slices, t.blocks, saved != nullptr);
}

void prelu_bwd(hipStream_t s, const PRelu& g, const PReluPlan& t,
               const float* x, const float* dy, const float* a, float* dx,
               float* da) {
  const double n = (double)g.N * g.C * g.S;
  PerfScope perf(PERF_CLASS("prelu"), s, 0, (dx ? 12.0 : 8.0) * n);
  CHECK_(t.vec == 1 || (aligned16(x) && aligned16(dy) && aligned16(dx)))
      << "PReLU backward: float4 layout on an unaligned tensor";
  double* part = (double*)Workspace::get_global().get(
      Workspace::kPReluPart, sizeof(double) * (size_t)t.slices * g.C);
  if (t.vec == 4)
    dx ? launch_bwd<f4, true>(s, g, t, x, dy, a, dx, part)
       : launch_bwd<f4, false>(s, g, t, x, dy, a, dx, part);
  else
    dx ? launch_bwd<float, true>(s, g, t, x, dy, a, dx, part)
       : launch_bwd<float, false>(s, g, t, x, dy, a, dx, part);
  if (g.shared)
    hipLaunchKernelGGL(k_prelu_final_shared, dim3(1), dim3(kFinalThreads), 0,
                       s, (const double*)part, (long)t.slices * g.C, da);
  else
    hipLaunchKernelGGL(k_prelu_final,
                       dim3((int)std::min<long>(ceil_div(g.C, kWaves), 2048)),
                       dim3(kTPB), 0, s, (const double*)part, g.C, t.slices,
                       da);
  kernel_trace_prelu(1, t.var, t.vec, t.slices, t.blocks, dx != nullptr);
}

}  // namespace gpu
}  // namespace camd
