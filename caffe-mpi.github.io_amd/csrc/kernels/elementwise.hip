// elementwise.hip — gfx950 kernels for the HBM-bound hot-path ops:
// im2col/col2im (batched, [K][Nimg*Spad] col layout), pooling, fused
// BatchNorm (3 kernels/direction vs the reference's ~10-launch GEMV chain,
// batch_norm_layer.hpp:96-120), ReLU, LRN, dropout, softmax+NLL, fused SGD
// update (sgd_solver.cu:10-20 semantics), eltwise and synthetic-data fills.
//
// Design rules (cdna_hip_programming.md): grid-stride loops capped at
// 2048 blocks ×256 threads (G11), coalesced unit-stride innermost access,
// no atomics on the backward scatter paths (gather formulation instead —
// deterministic, matching the reference's no-atomics choice,
// conv_layer.cu:43-48).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "../math.hpp"

namespace camd {
namespace gpu {

constexpr int TPB = 256;
static inline int nblocks(long n, int per_thread = 1) {
  long b = (n + (long)TPB * per_thread - 1) / ((long)TPB * per_thread);
  return (int)std::min<long>(b, 2048);
}

// ---- variant trace: which specialisation a launch wrapper below picked,
// and the launch-shaping numbers a test cannot see from outside (BN slice
// split, LRN odd tail, softmax grid, SGD bucket range).  Host-side only;
// off by default (one relaxed load per wrapper call), capped like the GEMM
// route trace.  Every field is passed from the branch / expression that
// launches, so the log cannot disagree with what ran.
enum KOp {
  kPoolMaxFwd, kPoolMaxBwd, kPoolAveFwd, kPoolAveBwd, kBnFwdStats,
  kBnBwdStats, kLrnFwd, kLrnBwd, kSoftmaxFwd, kSgdSeg, kSolverSeg,
  kSigmoidFwd, kSigmoidBwd, kSigmoidCeFwd, kSigmoidCeBwd, kEuclidFwd,
  kEuclidBwd, kSharedDiffSum, kContrastiveFwd, kContrastiveBwd, kGradSumsq,
  kClipFinal
};
enum KVar { kVarNone, kVarK3, kVarK3S1, kVarK3S2, kVarGeneric, kVarV4,
            kVarScalar, kVarRing5, kVarRowThread, kVarRowWave };
struct KernelRec {
  long a, b, c, d;  // per-op fields, see kernel_trace_read
  unsigned char op, var;
};
constexpr size_t kKTraceCap = 4096;
static std::atomic<bool> g_ktrace_on{false};
static std::mutex g_ktrace_mu;
static std::vector<KernelRec> g_ktrace_log;

static void ktrace_push(int op, int var, long a, long b, long c,
                        long d = 0) {
  std::lock_guard<std::mutex> lk(g_ktrace_mu);
  if (g_ktrace_log.size() < kKTraceCap)
    g_ktrace_log.push_back(
        KernelRec{a, b, c, d, (unsigned char)op, (unsigned char)var});
}
static inline void ktrace(int op, int var = kVarNone, long a = 0, long b = 0,
                          long c = 0, long d = 0) {
  if (g_ktrace_on.load(std::memory_order_relaxed))
    ktrace_push(op, var, a, b, c, d);
}
void kernel_trace(bool enable) {
  std::lock_guard<std::mutex> lk(g_ktrace_mu);
  if (enable) {
    g_ktrace_log.clear();
    g_ktrace_log.reserve(kKTraceCap);
  }
  g_ktrace_on.store(enable, std::memory_order_relaxed);
}

long kernel_trace_read(char* buf, long cap) {
  static const char* const op[] = {
      "pool_max_fwd", "pool_max_bwd", "pool_ave_fwd", "pool_ave_bwd",
      "bn_fwd_stats", "bn_bwd_stats", "lrn_fwd",      "lrn_bwd",
      "softmax_fwd",  "sgd_seg",      "solver_seg",   "sigmoid_fwd",
      "sigmoid_bwd",  "sigmoid_ce_fwd", "sigmoid_ce_bwd", "euclid_fwd",
      "euclid_bwd",   "shared_diff_sum", "contrastive_fwd",
      "contrastive_bwd", "grad_sumsq",  "clip_final"};
  // solver_seg keeps rule * 2 + l1 in the var byte
  static const char* const rule[] = {"sgd",     "nesterov", "adagrad",
                                     "rmsprop", "adadelta", "adam"};
  static const char* const var[] = {"",        "k3",     "k3s1",
                                    "k3s2",    "generic", "v4",
                                    "scalar",  "ring5",  "row_thread",
                                    "row_wave"};
  std::lock_guard<std::mutex> lk(g_ktrace_mu);
  long len = 0;
  if (cap > 0) buf[0] = 0;
  for (const KernelRec& r : g_ktrace_log) {
    char line[160];
    int n = 0;
    switch (r.op) {
      case kPoolMaxFwd:
      case kPoolMaxBwd:
        n = snprintf(line, sizeof(line), "op=%s var=%s\n", op[r.op],
                     var[r.var]);
        break;
      case kPoolAveFwd:
      case kPoolAveBwd:
        n = snprintf(line, sizeof(line), "op=%s\n", op[r.op]);
        break;
      case kBnFwdStats:
      case kBnBwdStats:
        n = snprintf(line, sizeof(line), "op=%s var=%s nb=%ld span_max=%ld\n",
                     op[r.op], var[r.var], r.a, r.b);
        break;
      case kLrnFwd:
      case kLrnBwd:
        n = snprintf(line, sizeof(line), "op=%s var=%s odd=%ld\n", op[r.op],
                     var[r.var], r.a);
        break;
      case kSoftmaxFwd:
        n = snprintf(line, sizeof(line), "op=%s rows=%ld C=%ld blocks=%ld\n",
                     op[r.op], r.a, r.b, r.c);
        break;
      case kSolverSeg:
        // d: the launch read the clip factor; the unclipped text is unchanged
        n = snprintf(line, sizeof(line),
                     "op=%s rule=%s reg=%s lo=%ld hi=%ld nseg=%ld%s\n",
                     op[r.op], rule[r.var >> 1], (r.var & 1) ? "L1" : "L2",
                     r.a, r.b, r.c, r.d ? " clip=1" : "");
        break;
      case kGradSumsq:
        n = snprintf(line, sizeof(line),
                     "op=%s lo=%ld hi=%ld blocks=%ld passes=%ld\n", op[r.op],
                     r.a, r.b, r.c, r.d);
        break;
      case kClipFinal:
        n = snprintf(line, sizeof(line), "op=%s partials=%ld\n", op[r.op],
                     r.a);
        break;
      case kSigmoidFwd:
      case kSigmoidBwd:
      case kSigmoidCeBwd:
      case kEuclidBwd:
        n = snprintf(line, sizeof(line), "op=%s n=%ld blocks=%ld passes=%ld\n",
                     op[r.op], r.a, r.b, r.c);
        break;
      case kSigmoidCeFwd:
      case kEuclidFwd:
        n = snprintf(line, sizeof(line),
                     "op=%s n=%ld blocks=%ld partials=%ld passes=%ld\n",
                     op[r.op], r.a, r.b, r.c, r.d);
        break;
      case kSharedDiffSum:
        n = snprintf(line, sizeof(line),
                     "op=%s lo=%ld hi=%ld nseg=%ld nsrc=%ld\n", op[r.op], r.a,
                     r.b, r.c, r.d);
        break;
      case kContrastiveFwd:
      case kContrastiveBwd:
        n = snprintf(line, sizeof(line), "op=%s var=%s N=%ld C=%ld blocks=%ld\n",
                     op[r.op], var[r.var], r.a, r.b, r.c);
        break;
      default:  // sgd_seg; d as for solver_seg
        n = snprintf(line, sizeof(line), "op=%s lo=%ld hi=%ld nseg=%ld%s\n",
                     op[r.op], r.a, r.b, r.c, r.d ? " clip=1" : "");
        break;
    }
    if (len + n < cap) memcpy(buf + len, line, (size_t)n + 1);
    len += n;
  }
  return len;
}

#define GRID_STRIDE(i, n)                                        \
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); \
       i += (long)gridDim.x * blockDim.x)

// ------------------------------------------------------------ im2col
// 3D grid: z = image, y = col row (c,ki,kj), x-threads sweep the output
// pixels — all inner indexing 32-bit, writes fully coalesced along sp.
__global__ void k_im2col_b(const float* __restrict__ x, int C, int H, int W,
                           int kh, int kw, int ph, int pw, int sh, int sw,
                           int dh, int dw, int OH, int OW, long Spad,
                           long cols, float* __restrict__ col) {
  const int n = blockIdx.z;
  const int row = blockIdx.y;  // c*kh*kw + ki*kw + kj
  const int c = row / (kh * kw);
  const int ki = (row / kw) % kh;
  const int kj = row % kw;
  const int S = OH * OW;
  const float* xp = x + ((long)n * C + c) * H * W;
  float* cp = col + (long)row * cols + (long)n * Spad;
  // 4-wide packs: the scalar form was ISSUE-bound (SQ: 51% instruction
  // stall — one div + bounds + load + store per element); an interior
  // s1 pack is one unaligned float4 read + one aligned float4 write
  using f4u = __attribute__((ext_vector_type(4), aligned(4))) float;
  const int Spad4 = (int)(Spad / 4);  // Spad % 16 == 0
  for (int p4 = blockIdx.x * blockDim.x + threadIdx.x; p4 < Spad4;
       p4 += gridDim.x * blockDim.x) {
    const int sp = 4 * p4;
    const int oh = sp / OW, ow = sp - oh * OW;
    const int h = oh * sh - ph + ki * dh;
    const int w = ow * sw - pw + kj * dw;
    if (sw == 1 && dw == 1 && sp + 3 < S && ow + 3 < OW && h >= 0 &&
        h < H && w >= 0 && w + 3 < W) {
      *(f4u*)(cp + sp) = *(const f4u*)(xp + h * W + w);
      continue;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = 0.f;
      const int spj = sp + j;
      if (spj < S) {
        const int ohj = spj / OW, owj = spj - ohj * OW;
        const int hj = ohj * sh - ph + ki * dh;
        const int wj = owj * sw - pw + kj * dw;
        if (hj >= 0 && hj < H && wj >= 0 && wj < W) v = xp[hj * W + wj];
      }
      cp[spj] = v;
    }
  }
}

void im2col_batched(hipStream_t s, const float* x, int Nimg, int C, int H,
                    int W, int kh, int kw, int ph, int pw, int sh, int sw,
                    int dh, int dw, int OH, int OW, long Spad, float* col) {
  const long total = (long)C * kh * kw * Nimg * Spad;
  PerfScope perf(PERF_CLASS("im2col"), s, 0,
                 8.0 * total);  // ~1 read + 1 write per element
  const int bx = (int)std::min<long>((Spad / 4 + TPB - 1) / TPB, 16);
  dim3 grid(bx, C * kh * kw, Nimg);
  hipLaunchKernelGGL(k_im2col_b, grid, dim3(TPB), 0, s, x, C, H, W, kh, kw,
                     ph, pw, sh, sw, dh, dw, OH, OW, Spad,
                     (long)Nimg * Spad, col);
}

// gather col2im (reference im2col.cu:256-295 pattern — no atomics)
// 3D grid: z = image, y = channel, x-threads sweep H*W (32-bit indices)
__global__ void k_col2im_b(const float* __restrict__ col, int C, int H,
                           int W, int kh, int kw, int ph, int pw, int sh,
                           int sw, int dh, int dw, int OH, int OW,
                           long Spad, long cols, float* __restrict__ dx) {
  const int n = blockIdx.z;
  const int c = blockIdx.y;
  const float* cp = col + (long)n * Spad;
  float* dp = dx + ((long)n * C + c) * H * W;
  for (int hw = blockIdx.x * blockDim.x + threadIdx.x; hw < H * W;
       hw += gridDim.x * blockDim.x) {
    const int h = hw / W, w = hw - h * W;
    float acc = 0.f;
    for (int i = 0; i < kh; ++i) {
      int hk = h + ph - i * dh;
      if (hk < 0 || hk % sh) continue;
      hk /= sh;
      if (hk >= OH) continue;
      for (int j = 0; j < kw; ++j) {
        int wk = w + pw - j * dw;
        if (wk < 0 || wk % sw) continue;
        wk /= sw;
        if (wk >= OW) continue;
        const int row = (c * kh + i) * kw + j;
        acc += cp[(long)row * cols + hk * OW + wk];
      }
    }
    dp[hw] = acc;
  }
}

void col2im_batched(hipStream_t s, const float* dcol, int Nimg, int C, int H,
                    int W, int kh, int kw, int ph, int pw, int sh, int sw,
                    int dh, int dw, int OH, int OW, long Spad, float* dx) {
  const long total = (long)Nimg * C * H * W;
  PerfScope perf(PERF_CLASS("col2im"), s, 0, 8.0 * total * kh * kw / (sh * sw));
  const int bx = (int)std::min<long>(((long)H * W + TPB - 1) / TPB, 16);
  dim3 grid(bx, C, Nimg);
  hipLaunchKernelGGL(k_col2im_b, grid, dim3(TPB), 0, s, dcol, C, H, W, kh,
                     kw, ph, pw, sh, sw, dh, dw, OH, OW, Spad,
                     (long)Nimg * Spad, dx);
}

// ---- float4 elementwise helpers (tensors are 64B-padded, so the float4
// body covers n/4*4 and a scalar tail handles the rest)
using f4 = __attribute__((ext_vector_type(4))) float;
#define VEC_GRID(i, n4) \
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n4); \
       i += (long)gridDim.x * blockDim.x)
// ------------------------------------------------------------ relu
__global__ void k_relu_fwd(const f4* __restrict__ x, long n4, float slope,
                           f4* __restrict__ y) {
  VEC_GRID(i, n4) {
    f4 v = x[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.f ? v[j] : slope * v[j];
    y[i] = v;
  }
}
void relu_fwd(hipStream_t s, const float* x, long n, float slope, float* y) {
  PerfScope perf(PERF_CLASS("relu"), s, 0, 8.0 * n);
  const long n4 = (n + 3) / 4;  // blobs are 64B-padded
  hipLaunchKernelGGL(k_relu_fwd, dim3(nblocks(n4, 4)), dim3(TPB), 0, s,
                     (const f4*)x, n4, slope, (f4*)y);
}

__global__ void k_relu_bwd(const f4* __restrict__ x,
                           const f4* __restrict__ dy, long n4, float slope,
                           f4* __restrict__ dx) {
  VEC_GRID(i, n4) {
    const f4 v = x[i];
    f4 d = dy[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] *= v[j] > 0.f ? 1.f : slope;
    dx[i] = d;
  }
}
void relu_bwd(hipStream_t s, const float* x, const float* dy, long n,
              float slope, float* dx) {
  PerfScope perf(PERF_CLASS("relu"), s, 0, 12.0 * n);
  const long n4 = (n + 3) / 4;
  hipLaunchKernelGGL(k_relu_bwd, dim3(nblocks(n4, 4)), dim3(TPB), 0, s,
                     (const f4*)x, (const f4*)dy, n4, slope, (f4*)dx);
}

__global__ void k_axpy(const f4* __restrict__ x, long n4, float a,
                       f4* __restrict__ y) {
  VEC_GRID(i, n4) {
    f4 v = y[i];
    const f4 xv = x[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += a * xv[j];
    y[i] = v;
  }
}
// y += a*x over the (64B-padded) gradient arena — iter_size accumulation
void axpy(hipStream_t s, long n, float a, const float* x, float* y) {
  PerfScope perf(PERF_CLASS("eltwise"), s, 0, 12.0 * n);
  const long n4 = (n + 3) / 4;
  hipLaunchKernelGGL(k_axpy, dim3(nblocks(n4, 4)), dim3(TPB), 0, s,
                     (const f4*)x, n4, a, (f4*)y);
}

// ------------------------------------------------------------ pooling
// flat index over [nc][H][W] -> (w, h, nc): the output pixel of the forward
// kernels (called with OW, OH), the input pixel of the backward ones
struct PoolIdx {
  int w, h;
  long nc;
};
__device__ __forceinline__ PoolIdx pool_idx(long idx, int W, int H) {
  return {(int)(idx % W), (int)((idx / W) % H), idx / ((long)W * H)};
}
// [p0, p1): the output positions, of O along one axis, whose k-wide window
// at stride s covers padded input coordinate t = h + pad >= 0.  With the
// stride a template constant S > 0 the divisions are unsigned (t - k >= 0
// where it is divided) and fold away: nothing at S = 1, shifts at S = 2.
struct WinRange {
  int p0, p1;
};
template <int S = 0>
__device__ __forceinline__ WinRange pool_win_range(int t, int k, int s,
                                                   int O) {
  if constexpr (S > 0)
    return {t < k ? 0 : (int)((unsigned)(t - k) / S) + 1,
            min((int)((unsigned)t / S) + 1, O)};
  return {t < k ? 0 : (t - k) / s + 1, min(t / s + 1, O)};
}

__global__ void k_pool_max_fwd(const float* __restrict__ x, int N, int C,
                               int H, int W, int kh, int kw, int ph, int pw,
                               int sh, int sw, int OH, int OW,
                               float* __restrict__ y, int* __restrict__ mask) {
  const long total = (long)N * C * OH * OW;
  GRID_STRIDE(idx, total) {
    const PoolIdx o = pool_idx(idx, OW, OH);
    const float* xp = x + o.nc * H * W;
    int hs = o.h * sh - ph, ws = o.w * sw - pw;
    const int he = min(hs + kh, H), we = min(ws + kw, W);
    hs = max(hs, 0);
    ws = max(ws, 0);
    float best = -3.402823466e38f;
    int bi = -1;
    for (int h = hs; h < he; ++h)
      for (int w = ws; w < we; ++w) {
        const float v = xp[h * W + w];
        if (v > best) {  // strict >, first max wins (pooling_layer.cpp:166)
          best = v;
          bi = h * W + w;
        }
      }
    y[idx] = best;
    mask[idx] = bi;
  }
}
// 3x3 specialization: the generic kernel's runtime-bounded window loop
// keeps only ~2 loads in flight per wave (SQ: 76-78% parked on the
// GoogLeNet pools); a fully-unrolled predicated 3x3 issues all 9 loads
// before any wait.  Same first-max-wins order (fixed (h,w) ascending).
__global__ void k_pool_max_fwd3(const float* __restrict__ x, int N, int C,
                                int H, int W, int ph, int pw, int sh,
                                int sw, int OH, int OW,
                                float* __restrict__ y,
                                int* __restrict__ mask) {
  const long total = (long)N * C * OH * OW;
  GRID_STRIDE(idx, total) {
    const PoolIdx o = pool_idx(idx, OW, OH);
    const float* xp = x + o.nc * H * W;
    const int hs = o.h * sh - ph, ws = o.w * sw - pw;
    float v[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int h = hs + a, w = ws + b;
        const bool ok = h >= 0 && h < H && w >= 0 && w < W;
        v[a * 3 + b] = ok ? xp[h * W + w] : -3.402823466e38f;
      }
    float best = -3.402823466e38f;
    int bi = -1;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int h = hs + a, w = ws + b;
        const bool ok = h >= 0 && h < H && w >= 0 && w < W;
        if (ok && v[a * 3 + b] > best) {  // strict >: first max wins
          best = v[a * 3 + b];
          bi = h * W + w;
        }
      }
    y[idx] = best;
    mask[idx] = bi;
  }
}

void pool_max_fwd(hipStream_t s, const float* x, int N, int C, int H, int W,
                  int kh, int kw, int ph, int pw, int sh, int sw, int OH,
                  int OW, float* y, int* mask) {
  const long total = (long)N * C * OH * OW;
  PerfScope perf(PERF_CLASS("pool"), s, 0, 4.0 * total * (kh * kw + 2));
  if (kh == 3 && kw == 3) {
    hipLaunchKernelGGL(k_pool_max_fwd3, dim3(nblocks(total, 2)), dim3(TPB),
                       0, s, x, N, C, H, W, ph, pw, sh, sw, OH, OW, y,
                       mask);
    ktrace(kPoolMaxFwd, kVarK3);
    return;
  }
  hipLaunchKernelGGL(k_pool_max_fwd, dim3(nblocks(total, 2)), dim3(TPB), 0,
                     s, x, N, C, H, W, kh, kw, ph, pw, sh, sw, OH, OW, y,
                     mask);
  ktrace(kPoolMaxFwd, kVarGeneric);
}

// deterministic gather backward: each input element scans the <= ceil(k/s)^2
// windows that can contain it and sums where mask points at it
__global__ void k_pool_max_bwd(const float* __restrict__ dy,
                               const int* __restrict__ mask, int N, int C,
                               int H, int W, int kh, int kw, int ph, int pw,
                               int sh, int sw, int OH, int OW,
                               float* __restrict__ dx) {
  const long total = (long)N * C * H * W;
  GRID_STRIDE(idx, total) {
    const PoolIdx p = pool_idx(idx, W, H);
    const int me = p.h * W + p.w;
    const WinRange ra = pool_win_range(p.h + ph, kh, sh, OH);
    const WinRange rb = pool_win_range(p.w + pw, kw, sw, OW);
    float acc = 0.f;
    const float* dyp = dy + p.nc * OH * OW;
    const int* mp = mask + p.nc * OH * OW;
    for (int a = ra.p0; a < ra.p1; ++a)
      for (int b = rb.p0; b < rb.p1; ++b)
        if (mp[a * OW + b] == me) acc += dyp[a * OW + b];
    dx[idx] = acc;
  }
}
// 3x3 bwd specialization: for k=3 an input element sits in at most 3x3
// candidate windows — unroll them with predicates so all 18 mask/dy
// loads issue before any wait (the generic loop was latency-serialized,
// 78% parked).  Ascending (a, b) — fixed, deterministic order.
// S = 0 takes the strides at run time.  S = 1 (the 13 GoogLeNet inception
// pools) and S = 2 (the ResNet/GoogLeNet/AlexNet downsampling pools) are
// the stride at compile time: the window bounds lose their divisions (the
// run-time form pays four), and at stride 2 an input pixel overlaps at
// most 2x2 windows, so the gather is 4 dy + 4 mask loads instead of 9 + 9.
template <int S>
__global__ void k_pool_max_bwd3(const float* __restrict__ dy,
                                const int* __restrict__ mask, int N, int C,
                                int H, int W, int ph, int pw, int sh,
                                int sw, int OH, int OW,
                                float* __restrict__ dx) {
  constexpr int NW = S == 2 ? 2 : 3;  // candidate windows per axis
  const long total = (long)N * C * H * W;
  GRID_STRIDE(idx, total) {
    const PoolIdx p = pool_idx(idx, W, H);
    const int me = p.h * W + p.w;
    const WinRange ra = pool_win_range<S>(p.h + ph, 3, sh, OH);
    const WinRange rb = pool_win_range<S>(p.w + pw, 3, sw, OW);
    const float* dyp = dy + p.nc * OH * OW;
    const int* mp = mask + p.nc * OH * OW;
    bool hit[NW * NW];
    float d[NW * NW];
#pragma unroll
    for (int da = 0; da < NW; ++da)
#pragma unroll
      for (int db = 0; db < NW; ++db) {
        const int a = ra.p0 + da, b = rb.p0 + db;
        const bool ok = a < ra.p1 && b < rb.p1;
        const int off = ok ? a * OW + b : 0;
        hit[da * NW + db] = ok && mp[off] == me;
        d[da * NW + db] = dyp[off];
      }
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NW * NW; ++i)
      if (hit[i]) acc += d[i];  // select, not multiply: a stray NaN in a
                                // NON-matching window must not leak in
    dx[idx] = acc;
  }
}

void pool_max_bwd(hipStream_t s, const float* dy, const int* mask, int N,
                  int C, int H, int W, int kh, int kw, int ph, int pw,
                  int sh, int sw, int OH, int OW, float* dx) {
  const long total = (long)N * C * H * W;
  PerfScope perf(PERF_CLASS("pool"), s, 0, 12.0 * total);
  const dim3 grid(nblocks(total, 2)), block(TPB);
  if (kh == 3 && kw == 3 && sh == 1 && sw == 1) {
    hipLaunchKernelGGL(k_pool_max_bwd3<1>, grid, block, 0, s, dy, mask, N, C,
                       H, W, ph, pw, sh, sw, OH, OW, dx);
    ktrace(kPoolMaxBwd, kVarK3S1);
    return;
  }
  if (kh == 3 && kw == 3 && sh == 2 && sw == 2) {
    hipLaunchKernelGGL(k_pool_max_bwd3<2>, grid, block, 0, s, dy, mask, N, C,
                       H, W, ph, pw, sh, sw, OH, OW, dx);
    ktrace(kPoolMaxBwd, kVarK3S2);
    return;
  }
  if (kh == 3 && kw == 3) {
    hipLaunchKernelGGL(k_pool_max_bwd3<0>, grid, block, 0, s, dy, mask, N, C,
                       H, W, ph, pw, sh, sw, OH, OW, dx);
    ktrace(kPoolMaxBwd, kVarK3);
    return;
  }
  hipLaunchKernelGGL(k_pool_max_bwd, grid, block, 0, s, dy, mask, N, C, H, W,
                     kh, kw, ph, pw, sh, sw, OH, OW, dx);
  ktrace(kPoolMaxBwd, kVarGeneric);
}

__global__ void k_pool_ave_fwd(const float* __restrict__ x, int N, int C,
                               int H, int W, int kh, int kw, int ph, int pw,
                               int sh, int sw, int OH, int OW,
                               float* __restrict__ y) {
  const long total = (long)N * C * OH * OW;
  GRID_STRIDE(idx, total) {
    const PoolIdx o = pool_idx(idx, OW, OH);
    const float* xp = x + o.nc * H * W;
    int hs = o.h * sh - ph, ws = o.w * sw - pw;
    int he = min(hs + kh, H + ph), we = min(ws + kw, W + pw);
    const int ps = (he - hs) * (we - ws);  // padded size (:201)
    hs = max(hs, 0);
    ws = max(ws, 0);
    he = min(he, H);
    we = min(we, W);
    float acc = 0.f;
    for (int h = hs; h < he; ++h)
      for (int w = ws; w < we; ++w) acc += xp[h * W + w];
    y[idx] = acc / ps;
  }
}
void pool_ave_fwd(hipStream_t s, const float* x, int N, int C, int H, int W,
                  int kh, int kw, int ph, int pw, int sh, int sw, int OH,
                  int OW, float* y) {
  const long total = (long)N * C * OH * OW;
  PerfScope perf(PERF_CLASS("pool"), s, 0, 4.0 * total * (kh * kw + 1));
  hipLaunchKernelGGL(k_pool_ave_fwd, dim3(nblocks(total, 2)), dim3(TPB), 0,
                     s, x, N, C, H, W, kh, kw, ph, pw, sh, sw, OH, OW, y);
  ktrace(kPoolAveFwd);
}

__global__ void k_pool_ave_bwd(const float* __restrict__ dy, int N, int C,
                               int H, int W, int kh, int kw, int ph, int pw,
                               int sh, int sw, int OH, int OW,
                               float* __restrict__ dx) {
  const long total = (long)N * C * H * W;
  GRID_STRIDE(idx, total) {
    const PoolIdx p = pool_idx(idx, W, H);
    const WinRange ra = pool_win_range(p.h + ph, kh, sh, OH);
    const WinRange rb = pool_win_range(p.w + pw, kw, sw, OW);
    float acc = 0.f;
    const float* dyp = dy + p.nc * OH * OW;
    for (int a = ra.p0; a < ra.p1; ++a)
      for (int b = rb.p0; b < rb.p1; ++b) {
        int hs = a * sh - ph, ws = b * sw - pw;
        const int he = min(hs + kh, H + ph), we = min(ws + kw, W + pw);
        const int ps = (he - hs) * (we - ws);
        acc += dyp[a * OW + b] / ps;
      }
    dx[idx] = acc;
  }
}
void pool_ave_bwd(hipStream_t s, const float* dy, int N, int C, int H, int W,
                  int kh, int kw, int ph, int pw, int sh, int sw, int OH,
                  int OW, float* dx) {
  const long total = (long)N * C * H * W;
  PerfScope perf(PERF_CLASS("pool"), s, 0, 8.0 * total);
  hipLaunchKernelGGL(k_pool_ave_bwd, dim3(nblocks(total, 2)), dim3(TPB), 0,
                     s, dy, N, C, H, W, kh, kw, ph, pw, sh, sw, OH, OW, dx);
  ktrace(kPoolAveBwd);
}

// y = x * a[c] (+ b[c]) — Scale layer forward (b = bias or null) and its
// backward-data (a = scale, b = null), reference scale_layer.cpp
__global__ void k_chan_affine(const float* __restrict__ x,
                              const float* __restrict__ a,
                              const float* __restrict__ b, int C, long S,
                              long total, float* __restrict__ y) {
  GRID_STRIDE(i, total) {
    const int c = (int)((i / S) % C);
    y[i] = x[i] * a[c] + (b ? b[c] : 0.f);
  }
}
void chan_affine(hipStream_t s, const float* x, const float* a,
                 const float* b, int N, int C, long S, float* y) {
  const long total = (long)N * C * S;
  PerfScope perf(PERF_CLASS("eltwise"), s, 0, 8.0 * total);
  hipLaunchKernelGGL(k_chan_affine, dim3(nblocks(total, 8)), dim3(TPB), 0,
                     s, x, a, b, C, S, total, y);
}

// ------------------------------------------------------------ batchnorm
// partials layout: double2[C][nb] {sum, sumsq} (fwd) / {sum_dy, sum_dyxn}
// (bwd).  Deterministic: fixed block→slice mapping, in-block tree reduce.
int bn_blocks_per_channel(int N, int C) {
  // image-sliced reduction: nb batch slices per channel, ~2048 blocks total
  return std::max(1, std::min(N, 2048 / std::max(1, C)));
}

// Batch slice `slice` of nb covers the images [n0, n1).  The kernels and
// the trace both take the bounds from here.
struct BnSlice {
  int n0, n1;
};
__host__ __device__ inline BnSlice bn_slice(int N, int slice, int nb) {
  return {(int)((long)N * slice / nb), (int)((long)N * (slice + 1) / nb)};
}
// trace record of a statistics launch: the largest per-block span
// (n1 - n0) * per over the nb batch slices; computed only when tracing
static inline void ktrace_bn(int op, int var, int N, int nb, long per) {
  if (!g_ktrace_on.load(std::memory_order_relaxed)) return;
  long span_max = 0;
  for (int slice = 0; slice < nb; ++slice) {
    const BnSlice sl = bn_slice(N, slice, nb);
    span_max = std::max(span_max, (sl.n1 - sl.n0) * per);
  }
  ktrace_push(op, var, nb, span_max, 0);
}
// What one block of a statistics kernel reduces: channel c = blockIdx % C
// over batch slice blockIdx / C — `span` loads, `per` of them per image
// (S floats, or S / 4 float4 packs), the i-th at addr(i).
struct BnBlock {
  int c, slice, n0, span, per, C;
  __device__ __forceinline__ long addr(int i) const {
    const int n = n0 + i / per;
    return ((long)n * C + c) * per + (i - (n - n0) * per);
  }
};
__device__ __forceinline__ BnBlock bn_block(int N, int C, int per, int nb) {
  const int c = blockIdx.x % C, slice = blockIdx.x / C;
  const BnSlice sl = bn_slice(N, slice, nb);
  return {c, slice, sl.n0, (sl.n1 - sl.n0) * per, per, C};
}
// in-block tree reduce of the threads' (s1, s2) and the store of the
// block's partial: fixed order, so the partials are deterministic
__device__ __forceinline__ void bn_reduce_store(double s1, double s2,
                                                const BnBlock& b, int nb,
                                                double2* __restrict__ out) {
  __shared__ double sh1[TPB], sh2[TPB];
  sh1[threadIdx.x] = s1;
  sh2[threadIdx.x] = s2;
  __syncthreads();
  for (int off = TPB / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) {
      sh1[threadIdx.x] += sh1[threadIdx.x + off];
      sh2[threadIdx.x] += sh2[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[(long)b.c * nb + b.slice] = {sh1[0], sh2[0]};
}
// a load of the statistics kernels is V = float, or f4 when S % 4 == 0
template <typename V>
constexpr int kLanes = sizeof(V) / sizeof(float);
__device__ __forceinline__ float lane(float v, int) { return v; }
__device__ __forceinline__ float lane(f4 v, int j) { return v[j]; }

// V = f4 (S % 4 == 0: every ResNet spatial stage except 7x7=49) quarters
// the load count and the per-element index divisions.  4-way unrolled with
// independent partial sums: the rolled loop kept ONE load in flight per
// wave (the accumulate chained on it), measuring 2.85 TB/s with waves
// 59-81% parked — four independent loads per iteration is the
// memory-level-parallelism fix, not more occupancy.
template <typename V>
__global__ void k_bn_fwd_stats(const V* __restrict__ x, int N, int C, int per,
                               int nb, double2* __restrict__ out) {
  constexpr int L = kLanes<V>;
  const BnBlock b = bn_block(N, C, per, nb);
  const int B = blockDim.x;
  double s1 = 0, s2 = 0;
  double t1 = 0, t2 = 0;  // second accumulator pair halves the add chain
  int i = threadIdx.x;
  for (; i + 3 * B < b.span; i += 4 * B) {  // 4 loads in flight (MLP)
    const V v0 = x[b.addr(i)];
    const V v1 = x[b.addr(i + B)];
    const V v2 = x[b.addr(i + 2 * B)];
    const V v3 = x[b.addr(i + 3 * B)];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const float a0 = lane(v0, j), a1 = lane(v1, j);
      const float a2 = lane(v2, j), a3 = lane(v3, j);
      s1 += (double)a0 + a1;
      s2 += (double)a0 * a0 + (double)a1 * a1;
      t1 += (double)a2 + a3;
      t2 += (double)a2 * a2 + (double)a3 * a3;
    }
  }
  for (; i < b.span; i += B) {
    const V v = x[b.addr(i)];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const double a = lane(v, j);
      s1 += a;
      s2 += a * a;
    }
  }
  bn_reduce_store(s1 + t1, s2 + t2, b, nb, out);
}

void bn_fwd_stats(hipStream_t s, const float* x, int N, int C, long S,
                  int nb, void* partials) {
  PerfScope perf(PERF_CLASS("bn"), s, 0, 4.0 * N * C * S);
  if (S % 4 == 0) {
    hipLaunchKernelGGL(k_bn_fwd_stats<f4>, dim3(C * nb), dim3(TPB), 0, s,
                       (const f4*)x, N, C, (int)(S / 4), nb,
                       (double2*)partials);
    ktrace_bn(kBnFwdStats, kVarV4, N, nb, (int)(S / 4));
    return;
  }
  hipLaunchKernelGGL(k_bn_fwd_stats<float>, dim3(C * nb), dim3(TPB), 0, s, x,
                     N, C, (int)S, nb, (double2*)partials);
  ktrace_bn(kBnFwdStats, kVarScalar, N, nb, S);
}

__global__ void k_bn_fwd_finalize(const double2* __restrict__ partials,
                                  int nb, int C, long NS, float eps,
                                  float* __restrict__ mean,
                                  float* __restrict__ var,
                                  float* __restrict__ inv_std) {
  GRID_STRIDE(c, (long)C) {
    double s1 = 0, s2 = 0;
    for (int b = 0; b < nb; ++b) {
      s1 += partials[c * nb + b].x;
      s2 += partials[c * nb + b].y;
    }
    const double m = s1 / NS;
    const double v = s2 / NS - m * m;  // E[x^2]-m^2 in double ≈ E[(x-m)^2]
    mean[c] = (float)m;
    var[c] = (float)v;
    inv_std[c] = (float)(1.0 / sqrt(v + (double)eps));
  }
}
void bn_fwd_finalize(hipStream_t s, const void* partials, int nb, int C,
                     long NS, float eps, float* mean, float* var,
                     float* inv_std) {
  hipLaunchKernelGGL(k_bn_fwd_finalize, dim3(1), dim3(TPB), 0, s,
                     (const double2*)partials, nb, C, NS, eps, mean, var,
                     inv_std);
}

// The norm / apply kernels walk the tensor as flat float4 packs; per pack
// ONE division recovers the channel.  A pack that straddles a channel
// boundary (whole == false) takes the channel per element, from bn_chan.
// 32-bit index math: the 64-bit division per 16B pack is ~3x the
// instruction cost of the 32-bit one, and every count here fits uint32
// (largest tensor ~300M elements).
struct BnPack {
  unsigned e0;  // first element
  int c;        // its channel
  bool whole;   // all four elements lie in channel c
};
__device__ __forceinline__ BnPack bn_pack(long i, int C, int S) {
  const unsigned e0 = (unsigned)(i * 4);
  const int row = (int)(e0 / (unsigned)S);  // n*C + c
  const int rem = (int)(e0 - (unsigned)row * (unsigned)S);
  return {e0, row % C, rem + 4 <= S};
}
__device__ __forceinline__ int bn_chan(unsigned e, int C, int S) {
  return (int)((e / (unsigned)S) % (unsigned)C);
}

__global__ void k_bn_fwd_norm(const f4* __restrict__ x,
                              const float* __restrict__ mean,
                              const float* __restrict__ inv_std,
                              const float* __restrict__ scale,
                              const float* __restrict__ bias, int sb, int C,
                              int S, int frelu, long n4,
                              const f4* __restrict__ add,
                              f4* __restrict__ y) {
  struct Chan {
    float mu, inv, sc, bi;
  };
  auto chan = [&](int c) {
    return Chan{mean[c], inv_std[c], sb ? scale[c] : 1.f,
                sb ? bias[c] : 0.f};
  };
  auto norm = [](float v, const Chan& k) {
    return (v - k.mu) * k.inv * k.sc + k.bi;
  };
  VEC_GRID(i, n4) {
    const BnPack p = bn_pack(i, C, S);
    f4 v = x[i];
    if (p.whole) {
      const Chan k = chan(p.c);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = norm(v[j], k);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[j] = norm(v[j], chan(bn_chan(p.e0 + j, C, S)));
    }
    if (add) {  // fused residual: bn(x) + other (ResNet block pattern)
      const f4 a = add[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += a[j];
    }
    if (frelu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
    }
    y[i] = v;
  }
}
void bn_fwd_norm(hipStream_t s, const float* x, const float* mean,
                 const float* inv_std, const float* scale, const float* bias,
                 int sb, int N, int C, long S, float* y, int fuse_relu,
                 const float* add) {
  const long total = (long)N * C * S;
  PerfScope perf(PERF_CLASS("bn"), s, 0, (add ? 12.0 : 8.0) * total);
  // blobs are 16-float padded: the final partial pack reads/writes pad
  // space with wrapped (but in-bounds) channel indices — harmless
  const long n4 = (total + 3) / 4;
  hipLaunchKernelGGL(k_bn_fwd_norm, dim3(nblocks(n4, 4)), dim3(TPB), 0, s,
                     (const f4*)x, mean, inv_std, scale, bias, sb, C,
                     (int)S, fuse_relu, n4, (const f4*)add, (f4*)y);
}

__global__ void k_bn_moving_avg(const float* __restrict__ mean,
                                const float* __restrict__ var, int C,
                                float maf, int copy_only,
                                float* __restrict__ gmean,
                                float* __restrict__ gvar) {
  GRID_STRIDE(c, (long)C) {
    if (copy_only) {
      gmean[c] = mean[c];
      gvar[c] = var[c];
    } else {  // batch_norm_layer.cpp:200-207
      gmean[c] = (1.f - maf) * mean[c] + maf * gmean[c];
      gvar[c] = (1.f - maf) * var[c] + maf * gvar[c];
    }
  }
}
void bn_moving_avg(hipStream_t s, const float* mean, const float* var, int C,
                   float maf, int copy_only, float* gmean, float* gvar) {
  hipLaunchKernelGGL(k_bn_moving_avg, dim3(1), dim3(TPB), 0, s, mean, var,
                     C, maf, copy_only, gmean, gvar);
}

__global__ void k_bn_fwd_test(const float* __restrict__ x,
                              const float* __restrict__ gmean,
                              const float* __restrict__ gvar,
                              const float* __restrict__ scale,
                              const float* __restrict__ bias, int sb, int N,
                              int C, long S, float eps,
                              float* __restrict__ y) {
  const long total = (long)N * C * S;
  GRID_STRIDE(i, total) {
    const int c = (int)((i / S) % C);
    const float inv = rsqrtf(gvar[c] + eps);
    const float v = (x[i] - gmean[c]) * inv;
    y[i] = sb ? v * scale[c] + bias[c] : v;
  }
}
void bn_fwd_test(hipStream_t s, const float* x, const float* gmean,
                 const float* gvar, const float* scale, const float* bias,
                 int sb, int N, int C, long S, float eps, float* y) {
  const long total = (long)N * C * S;
  PerfScope perf(PERF_CLASS("bn"), s, 0, 8.0 * total);
  hipLaunchKernelGGL(k_bn_fwd_test, dim3(nblocks(total, 8)), dim3(TPB), 0,
                     s, x, gmean, gvar, scale, bias, sb, N, C, S, eps, y);
}

template <typename V>
__global__ void k_bn_bwd_stats(const V* __restrict__ x,
                               const V* __restrict__ dy,
                               const float* __restrict__ mean,
                               const float* __restrict__ inv_std, int N,
                               int C, int per, int nb,
                               const float* __restrict__ scale,
                               const float* __restrict__ bias, int frelu,
                               double2* __restrict__ out) {
  constexpr int L = kLanes<V>;
  const BnBlock b = bn_block(N, C, per, nb);
  const int B = blockDim.x;
  const float m = mean[b.c], inv = inv_std[b.c];
  // fused ReLU backward: recompute the forward activation's sign exactly
  // (same fp32 op sequence as k_bn_fwd_norm) — no extra memory stream
  const float sc = scale ? scale[b.c] : 1.f;
  const float bi = bias ? bias[b.c] : 0.f;
  // one element into the pair (s_dy, s_dyxn)
  auto add = [&](float xv, float dv, double& s_dy, double& s_dyxn) {
    const float xn = (xv - m) * inv;
    double d = dv;
    if (frelu && xn * sc + bi <= 0.f) d = 0.0;
    s_dy += d;
    s_dyxn += d * (double)xn;
  };
  double s_dy = 0, s_dyxn = 0, t_dy = 0, t_dyxn = 0;
  int i = threadIdx.x;
  for (; i + B < b.span; i += 2 * B) {  // 4 loads (2 pairs) in flight
    const long o0 = b.addr(i), o1 = b.addr(i + B);
    const V xv0 = x[o0], dv0 = dy[o0];
    const V xv1 = x[o1], dv1 = dy[o1];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      add(lane(xv0, j), lane(dv0, j), s_dy, s_dyxn);
      add(lane(xv1, j), lane(dv1, j), t_dy, t_dyxn);
    }
  }
  for (; i < b.span; i += B) {
    const long off = b.addr(i);
    const V xv = x[off], dv = dy[off];
#pragma unroll
    for (int j = 0; j < L; ++j) add(lane(xv, j), lane(dv, j), s_dy, s_dyxn);
  }
  bn_reduce_store(s_dy + t_dy, s_dyxn + t_dyxn, b, nb, out);
}

void bn_bwd_stats(hipStream_t s, const float* x, const float* dy,
                  const float* mean, const float* inv_std, int N, int C,
                  long S, int nb, const float* scale, const float* bias,
                  int frelu, void* partials) {
  PerfScope perf(PERF_CLASS("bn"), s, 0, 8.0 * N * C * S);
  if (S % 4 == 0) {
    hipLaunchKernelGGL(k_bn_bwd_stats<f4>, dim3(C * nb), dim3(TPB), 0, s,
                       (const f4*)x, (const f4*)dy, mean, inv_std, N, C,
                       (int)(S / 4), nb, scale, bias, frelu,
                       (double2*)partials);
    ktrace_bn(kBnBwdStats, kVarV4, N, nb, (int)(S / 4));
    return;
  }
  hipLaunchKernelGGL(k_bn_bwd_stats<float>, dim3(C * nb), dim3(TPB), 0, s, x,
                     dy, mean, inv_std, N, C, (int)S, nb, scale, bias, frelu,
                     (double2*)partials);
  ktrace_bn(kBnBwdStats, kVarScalar, N, nb, S);
}

__global__ void k_bn_bwd_finalize(const double2* __restrict__ partials,
                                  int nb, int C, long NS,
                                  const float* __restrict__ scale, int sb,
                                  float* __restrict__ dscale,
                                  float* __restrict__ dbias,
                                  float* __restrict__ m_dy,
                                  float* __restrict__ m_dyxn) {
  GRID_STRIDE(c, (long)C) {
    double s_dy = 0, s_dyxn = 0;
    for (int b = 0; b < nb; ++b) {
      s_dy += partials[c * nb + b].x;
      s_dyxn += partials[c * nb + b].y;
    }
    if (sb) {
      dscale[c] = (float)s_dyxn;  // Σ dy·x̂ (batch_norm_layer.cpp:322-330)
      dbias[c] = (float)s_dy;     // Σ dy
    }
    const double sc = sb ? (double)scale[c] : 1.0;
    m_dy[c] = (float)(sc * s_dy / NS);
    m_dyxn[c] = (float)(sc * s_dyxn / NS);
  }
}
void bn_bwd_finalize(hipStream_t s, const void* partials, int nb, int C,
                     long NS, const float* scale, int sb, float* dscale,
                     float* dbias, float* m_dy, float* m_dyxn) {
  hipLaunchKernelGGL(k_bn_bwd_finalize, dim3(1), dim3(TPB), 0, s,
                     (const double2*)partials, nb, C, NS, scale, sb, dscale,
                     dbias, m_dy, m_dyxn);
}

__global__ void k_bn_bwd_apply(const f4* __restrict__ x,
                               const f4* __restrict__ dy,
                               const float* __restrict__ mean,
                               const float* __restrict__ inv_std,
                               const float* __restrict__ scale, int sb,
                               const float* __restrict__ m_dy,
                               const float* __restrict__ m_dyxn,
                               const float* __restrict__ bias, int frelu,
                               int C, int S, long n4, f4* __restrict__ dx) {
  // dx of one element of channel c; the fused ReLU's sign test is
  // k_bn_fwd_norm's expression, op for op
  // The per-element formula stands twice on purpose.  The
  // compiler contracts dj * sc - mdy - mdyxn * xn into FMAs in the whole-pack
  // path (hoisted values, branch-free: four elements vectorise into packed
  // FMAs) and leaves it as multiplies and subtractions in the straddle path
  // (the bias load sits behind frelu, mid-element).  Written once, as a
  // function of hoisted values or of c, both paths round the same way, which
  // moves the last bits of dx wherever S % 4 != 0 (the 7x7 stage): results
  // are pinned bit for bit by bench.py --dump-outputs.
  VEC_GRID(i, n4) {
    const BnPack p = bn_pack(i, C, S);
    const f4 xv = x[i];
    f4 d = dy[i];
    if (p.whole) {
      const int c = p.c;
      const float mu = mean[c], inv = inv_std[c];
      const float sc = sb ? scale[c] : 1.f;
      const float bi = (frelu && bias) ? bias[c] : 0.f;
      const float mdy = m_dy[c], mdyxn = m_dyxn[c];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xn = (xv[j] - mu) * inv;
        float dj = d[j];
        if (frelu && xn * sc + bi <= 0.f) dj = 0.f;
        d[j] = (dj * sc - mdy - mdyxn * xn) * inv;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cc = bn_chan(p.e0 + j, C, S);
        const float xn = (xv[j] - mean[cc]) * inv_std[cc];
        const float scc = sb ? scale[cc] : 1.f;
        float dj = d[j];
        if (frelu && xn * scc + ((frelu && bias) ? bias[cc] : 0.f) <= 0.f)
          dj = 0.f;
        d[j] = (dj * scc - m_dy[cc] - m_dyxn[cc] * xn) * inv_std[cc];
      }
    }
    dx[i] = d;
  }
}
void bn_bwd_apply(hipStream_t s, const float* x, const float* dy,
                  const float* mean, const float* inv_std,
                  const float* scale, int sb, const float* m_dy,
                  const float* m_dyxn, int N, int C, long S,
                  const float* bias, int frelu, float* dx) {
  const long total = (long)N * C * S;
  PerfScope perf(PERF_CLASS("bn"), s, 0, 12.0 * total);
  const long n4 = (total + 3) / 4;
  hipLaunchKernelGGL(k_bn_bwd_apply, dim3(nblocks(n4, 4)), dim3(TPB), 0, s,
                     (const f4*)x, (const f4*)dy, mean, inv_std, scale, sb,
                     m_dy, m_dyxn, bias, frelu, C, (int)S, n4, (f4*)dx);
}

// ------------------------------------------------------------ LRN
// TWO (n, s) positions per thread, far apart so both streams stay
// coalesced: the single running cross-channel window was a serial
// load->accumulate chain (SQ: 66% parked) — interleaving two independent
// chains doubles the loads in flight (lrn_layer.cu:9-60 restated)
// the pair of thread i: positions i and i + half of the N*S (n, s)
// positions, as the offsets b0, b1 of their channel 0; the odd last thread
// has one (two == false) and reads b1 = b0 without storing it
struct LrnPair {
  long b0, b1;
  bool two;
};
__device__ __forceinline__ LrnPair lrn_pair(long i, long half, long total,
                                            int C, long S) {
  const long idx0 = i;
  const long idx1 = i + half;
  const bool two = idx1 < total;
  const int n0 = (int)(idx0 / S);
  const int n1 = two ? (int)(idx1 / S) : n0;
  const long b0 = (long)n0 * C * S + (idx0 - (long)n0 * S);
  const long b1 = two ? (long)n1 * C * S + (idx1 - (long)n1 * S) : b0;
  return {b0, b1, two};
}
__global__ void k_lrn_fwd(const float* __restrict__ x, int N, int C, long S,
                          int size, float aos, float beta, float k,
                          float* __restrict__ scale, float* __restrict__ y) {
  const long total = (long)N * S;
  const long half = (total + 1) / 2;
  const int pre = (size - 1) / 2;
  GRID_STRIDE(i, half) {
    const LrnPair pp = lrn_pair(i, half, total, C, S);
    const long b0 = pp.b0, b1 = pp.b1;
    const bool two = pp.two;
    float a0 = 0.f, a1 = 0.f;
    for (int c = 0; c < size - pre && c < C; ++c) {
      const float v0 = x[b0 + (long)c * S];
      const float v1 = x[b1 + (long)c * S];
      a0 += v0 * v0;
      a1 += v1 * v1;
    }
    for (int c = 0; c < C; ++c) {
      if (c > 0) {
        const int head = c + size - 1 - pre;
        if (head < C) {
          const float v0 = x[b0 + (long)head * S];
          const float v1 = x[b1 + (long)head * S];
          a0 += v0 * v0;
          a1 += v1 * v1;
        }
        const int tail = c - 1 - pre;
        if (tail >= 0) {
          const float v0 = x[b0 + (long)tail * S];
          const float v1 = x[b1 + (long)tail * S];
          a0 -= v0 * v0;
          a1 -= v1 * v1;
        }
      }
      const long o0 = b0 + (long)c * S;
      const long o1 = b1 + (long)c * S;
      const float s0 = k + aos * a0;
      const float s1 = k + aos * a1;
      scale[o0] = s0;
      y[o0] = x[o0] * __powf(s0, -beta);
      if (two) {
        scale[o1] = s1;
        y[o1] = x[o1] * __powf(s1, -beta);
      }
    }
  }
}
// size-SPECIALIZED forward (local_size is 5 in every model-zoo LRN): a
// compile-time register ring of the last SZ window terms makes the
// running-window update ONE global load per channel — the tail term and
// the center value both come out of the ring instead of being re-read
// from HBM (3 loads/channel -> 1).  Same two-position interleave.
template <int SZ>
__global__ void k_lrn_fwd_t(const float* __restrict__ x, int N, int C,
                            long S, float aos, float beta, float k,
                            float* __restrict__ scale,
                            float* __restrict__ y) {
  constexpr int pre = (SZ - 1) / 2;       // window [c-pre, c+SZ-1-pre]
  const long total = (long)N * S;
  const long half = (total + 1) / 2;
  GRID_STRIDE(i, half) {
    const LrnPair pp = lrn_pair(i, half, total, C, S);
    const long b0 = pp.b0, b1 = pp.b1;
    const bool two = pp.two;
    // ring[j] at top of iter c holds channel c-1-pre+j's raw value /
    // square = window(c-1); out-of-range channels are zero
    float q0[SZ], q1[SZ], v0[SZ], v1[SZ];
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int j = 0; j < SZ; ++j) q0[j] = q1[j] = v0[j] = v1[j] = 0.f;
#pragma unroll
    for (int j = 0; j + pre + 1 < SZ; ++j)  // channels 0..SZ-2-pre
      if (j < C) {
        const float u0 = x[b0 + (long)j * S];
        const float u1 = x[b1 + (long)j * S];
        v0[j + pre + 1] = u0;
        q0[j + pre + 1] = u0 * u0;
        a0 += u0 * u0;
        v1[j + pre + 1] = u1;
        q1[j + pre + 1] = u1 * u1;
        a1 += u1 * u1;
      }
    for (int c = 0; c < C; ++c) {
      const int head = c + SZ - 1 - pre;
      float h0 = 0.f, h1 = 0.f;
      if (head < C) {
        h0 = x[b0 + (long)head * S];
        h1 = x[b1 + (long)head * S];
      }
      a0 += h0 * h0 - q0[0];
      a1 += h1 * h1 - q1[0];
#pragma unroll
      for (int j = 0; j + 1 < SZ; ++j) {
        q0[j] = q0[j + 1]; q1[j] = q1[j + 1];
        v0[j] = v0[j + 1]; v1[j] = v1[j + 1];
      }
      q0[SZ - 1] = h0 * h0; q1[SZ - 1] = h1 * h1;
      v0[SZ - 1] = h0;      v1[SZ - 1] = h1;
      const long o0 = b0 + (long)c * S;
      const float s0 = k + aos * a0;
      scale[o0] = s0;
      y[o0] = v0[pre] * __powf(s0, -beta);  // ring slot pre == channel c
      if (two) {
        const long o1 = b1 + (long)c * S;
        const float s1 = k + aos * a1;
        scale[o1] = s1;
        y[o1] = v1[pre] * __powf(s1, -beta);
      }
    }
  }
}

void lrn_fwd(hipStream_t s, const float* x, int N, int C, int H, int W,
             int size, float alpha, float beta, float k, float* scale,
             float* y) {
  const long S = (long)H * W;
  PerfScope perf(PERF_CLASS("lrn"), s, 0, 12.0 * N * C * S);
  if (size == 5) {
    hipLaunchKernelGGL(k_lrn_fwd_t<5>, dim3(nblocks((N * S + 1) / 2)),
                       dim3(TPB), 0, s, x, N, C, S, alpha / size, beta, k,
                       scale, y);
    ktrace(kLrnFwd, kVarRing5, (N * S) & 1);
    return;
  }
  hipLaunchKernelGGL(k_lrn_fwd, dim3(nblocks((N * S + 1) / 2)), dim3(TPB),
                     0, s, x, N, C, S, size, alpha / size, beta, k, scale,
                     y);
  ktrace(kLrnFwd, kVarGeneric, (N * S) & 1);
}

__global__ void k_lrn_bwd(const float* __restrict__ x,
                          const float* __restrict__ y,
                          const float* __restrict__ dy,
                          const float* __restrict__ scale, int N, int C,
                          long S, int size, float cr, float beta,
                          float* __restrict__ dx) {
  const long total = (long)N * S;
  const int pre = (size - 1) / 2;
  GRID_STRIDE(idx, total) {
    const int n = (int)(idx / S);
    const long sp = idx - (long)n * S;
    const long base = (long)n * C * S + sp;
    // ratio(c) = dy*y/scale; window for dx[c]: cc in [c-(size-1-pre), c+pre]
    float acc = 0.f;
    const int lo0 = -(size - 1 - pre);
    for (int cc = lo0; cc <= pre - 1; ++cc)
      if (cc >= 0 && cc < C) {
        const long i = base + (long)cc * S;
        acc += dy[i] * y[i] / scale[i];
      }
    for (int c = 0; c < C; ++c) {
      const int head = c + pre;
      if (head >= 0 && head < C) {
        const long i = base + (long)head * S;
        acc += dy[i] * y[i] / scale[i];
      }
      const long i = base + (long)c * S;
      dx[i] = dy[i] * __powf(scale[i], -beta) - cr * x[i] * acc;
      const int tail = c + lo0;
      if (tail >= 0 && tail < C) {
        const long j = base + (long)tail * S;
        acc -= dy[j] * y[j] / scale[j];
      }
    }
  }
}
// size-SPECIALIZED backward: register rings of the last SZ-1 window
// ratios (dy*y/scale) AND of the diagonal term dy*scale^-beta — each
// channel's (dy, y, scale) triple is loaded ONCE, as the window head,
// instead of three times (head ratio, tail ratio, diagonal): 9 loads +
// 2 divisions per channel -> 4 loads + 1 division.  Two (n, s) positions
// per thread as in the forward (the single running chain serializes).
template <int SZ>
__global__ void k_lrn_bwd_t(const float* __restrict__ x,
                            const float* __restrict__ y,
                            const float* __restrict__ dy,
                            const float* __restrict__ scale, int N, int C,
                            long S, float cr, float beta,
                            float* __restrict__ dx) {
  constexpr int pre = (SZ - 1) / 2;
  constexpr int ctr = SZ - 1 - pre;  // center channel's ring slot (-lo0)
  const long total = (long)N * S;
  const long half = (total + 1) / 2;
  GRID_STRIDE(i, half) {
    const LrnPair pp = lrn_pair(i, half, total, C, S);
    const long b0 = pp.b0, b1 = pp.b1;
    const bool two = pp.two;
    // rings hold channels [c-ctr, c+pre-1] at top of iter c
    float rr0[SZ - 1], rr1[SZ - 1], tt0[SZ - 1], tt1[SZ - 1];
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int j = 0; j < SZ - 1; ++j) rr0[j] = rr1[j] = tt0[j] = tt1[j] = 0.f;
#pragma unroll
    for (int ch = 0; ch < pre; ++ch)    // prologue: channels 0..pre-1
      if (ch < C) {
        const long i0 = b0 + (long)ch * S, i1 = b1 + (long)ch * S;
        const float d0 = dy[i0], d1 = dy[i1];
        const float s0 = scale[i0], s1 = scale[i1];
        const float r0 = d0 * y[i0] / s0, r1 = d1 * y[i1] / s1;
        rr0[ch + ctr] = r0;
        tt0[ch + ctr] = d0 * __powf(s0, -beta);
        a0 += r0;
        rr1[ch + ctr] = r1;
        tt1[ch + ctr] = d1 * __powf(s1, -beta);
        a1 += r1;
      }
    for (int c = 0; c < C; ++c) {
      const int head = c + pre;
      float rh0 = 0.f, rh1 = 0.f, th0 = 0.f, th1 = 0.f;
      if (head < C) {
        const long i0 = b0 + (long)head * S, i1 = b1 + (long)head * S;
        const float d0 = dy[i0], d1 = dy[i1];
        const float s0 = scale[i0], s1 = scale[i1];
        rh0 = d0 * y[i0] / s0;
        th0 = d0 * __powf(s0, -beta);
        rh1 = d1 * y[i1] / s1;
        th1 = d1 * __powf(s1, -beta);
      }
      a0 += rh0;
      a1 += rh1;
      const long o0 = b0 + (long)c * S;
      dx[o0] = tt0[ctr] - cr * x[o0] * a0;
      if (two) {
        const long o1 = b1 + (long)c * S;
        dx[o1] = tt1[ctr] - cr * x[o1] * a1;
      }
      a0 -= rr0[0];
      a1 -= rr1[0];
#pragma unroll
      for (int j = 0; j + 1 < SZ - 1; ++j) {
        rr0[j] = rr0[j + 1]; rr1[j] = rr1[j + 1];
        tt0[j] = tt0[j + 1]; tt1[j] = tt1[j + 1];
      }
      rr0[SZ - 2] = rh0; rr1[SZ - 2] = rh1;
      tt0[SZ - 2] = th0; tt1[SZ - 2] = th1;
    }
  }
}

void lrn_bwd(hipStream_t s, const float* x, const float* y, const float* dy,
             const float* scale, int N, int C, int H, int W, int size,
             float alpha, float beta, float* dx) {
  const long S = (long)H * W;
  PerfScope perf(PERF_CLASS("lrn"), s, 0, 20.0 * N * C * S);
  if (size == 5) {
    hipLaunchKernelGGL(k_lrn_bwd_t<5>, dim3(nblocks((N * S + 1) / 2)),
                       dim3(TPB), 0, s, x, y, dy, scale, N, C, S,
                       2.f * alpha * beta / size, beta, dx);
    ktrace(kLrnBwd, kVarRing5, (N * S) & 1);
    return;
  }
  hipLaunchKernelGGL(k_lrn_bwd, dim3(nblocks(N * S)), dim3(TPB), 0, s, x, y,
                     dy, scale, N, C, S, size, 2.f * alpha * beta / size,
                     beta, dx);
  ktrace(kLrnBwd, kVarGeneric, (N * S) & 1);
}

// ------------------------------------------------------------ softmax
// one wave per sample row (C up to 1000): wave-parallel max/sum reductions.
// Non-finite inputs PROPAGATE as NaN exactly like the CPU path: a NaN or
// +inf logit makes the whole row NaN (CPU: exp(NaN-mx)=NaN contaminates the
// sum), while -inf logits are benign (exp(-inf-mx)=0).  fmaxf silently
// drops NaN operands and __expf may launder NaN, so the contamination is
// detected explicitly — a divergence here once masked an all-NaN logits
// tensor as a clean uniform distribution.
__global__ void k_softmax_fwd(const float* __restrict__ x, int outer, int C,
                              int inner, float* __restrict__ y) {
  const long rows = (long)outer * inner;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  for (long r = (long)blockIdx.x * wpb + wave; r < rows;
       r += (long)gridDim.x * wpb) {
    const int o = (int)(r / inner);
    const int sp = (int)(r - (long)o * inner);
    const float* xp = x + (long)o * C * inner + sp;
    float* yp = y + (long)o * C * inner + sp;
    float mx = -3.402823466e38f;
    int bad = 0;  // any NaN / +inf in the row
    for (int c = lane; c < C; c += 64) {
      const float v = xp[(long)c * inner];
      mx = fmaxf(mx, v);
      bad |= (v != v) | (v > 3.402823466e38f);
    }
    for (int off = 32; off > 0; off >>= 1) {
      mx = fmaxf(mx, __shfl_xor(mx, off, 64));
      bad |= __shfl_xor(bad, off, 64);
    }
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float e = __expf(xp[(long)c * inner] - mx);
      yp[(long)c * inner] = e;
      sum += e;
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    const float inv = 1.f / sum;
    const float fix = bad ? __builtin_nanf("") : 0.f;
    for (int c = lane; c < C; c += 64)
      yp[(long)c * inner] = yp[(long)c * inner] * inv + fix;
  }
}
void softmax_fwd(hipStream_t s, const float* x, int outer, int C, int inner,
                 float* prob) {
  const long rows = (long)outer * inner;
  PerfScope perf(PERF_CLASS("softmax"), s, 0, 12.0 * rows * C);
  const int blocks = (int)std::min<long>((rows + 3) / 4, 2048);
  hipLaunchKernelGGL(k_softmax_fwd, dim3(blocks), dim3(TPB), 0, s, x, outer,
                     C, inner, prob);
  ktrace(kSoftmaxFwd, kVarNone, rows, C, blocks);
}

// two-stage deterministic loss sum: block partials then final add
__global__ void k_sm_loss(const float* __restrict__ prob,
                          const float* __restrict__ label, int outer, int C,
                          int inner, float norm, float* __restrict__ loss) {
  const long rows = (long)outer * inner;
  double acc = 0;
  for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < rows;
       r += (long)gridDim.x * blockDim.x) {
    const int o = (int)(r / inner);
    const int sp = (int)(r - (long)o * inner);
    const int lv = (int)label[(long)o * inner + sp];
    const float p = prob[((long)o * C + lv) * inner + sp];
    // NaN prob must surface as NaN loss (CPU parity): fmaxf(NaN, FLT_MIN)
    // would clamp it to a clean finite number and hide the divergence
    if (p != p)
      acc += (double)p;
    else
      acc -= (double)__logf(fmaxf(p, 1.175494351e-38f));
  }
  __shared__ double sh[TPB];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = TPB / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    // single block launch: write final
    loss[blockIdx.x] = (float)(sh[0] / norm);
  }
}
void softmaxloss_fwd(hipStream_t s, const float* prob, const float* label,
                     int outer, int C, int inner, float* loss_out) {
  PerfScope perf(PERF_CLASS("softmax"), s, 0, 8.0 * outer * inner);
  hipLaunchKernelGGL(k_sm_loss, dim3(1), dim3(TPB), 0, s, prob, label,
                     outer, C, inner, (float)((long)outer * inner),
                     loss_out);
}

__global__ void k_sm_loss_bwd(const float* __restrict__ prob,
                              const float* __restrict__ label, int outer,
                              int C, int inner, float scale,
                              float* __restrict__ dx) {
  const long total = (long)outer * C * inner;
  GRID_STRIDE(i, total) {
    const long o = i / ((long)C * inner);
    const long rem = i - o * C * inner;
    const int c = (int)(rem / inner);
    const int sp = (int)(rem - (long)c * inner);
    const int lv = (int)label[o * inner + sp];
    dx[i] = (prob[i] - (c == lv ? 1.f : 0.f)) * scale;
  }
}
void softmaxloss_bwd(hipStream_t s, const float* prob, const float* label,
                     int outer, int C, int inner, float scale, float* dx) {
  const long total = (long)outer * C * inner;
  PerfScope perf(PERF_CLASS("softmax"), s, 0, 8.0 * total);
  hipLaunchKernelGGL(k_sm_loss_bwd, dim3(nblocks(total, 4)), dim3(TPB), 0,
                     s, prob, label, outer, C, inner, scale, dx);
}

// ------------------------------------------- sigmoid, its loss, euclidean
// Flat float4 streaming over n elements.  The pack at the edge is loaded
// whole (allocations are padded to 16 floats) and its lanes past n are kept
// out of every sum and every store: a blob reshaped smaller, or a top that
// shares memory with a larger blob, has live values there.
__device__ __forceinline__ void store_pack(float* __restrict__ y, long i,
                                           long n, f4 v) {
  if (4 * i + 4 <= n) {
    ((f4*)y)[i] = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * i + j < n) y[4 * i + j] = v[j];
  }
}
// grid of a flat pack kernel and, for the trace, how many grid-stride
// passes its busiest thread makes
struct PackGrid {
  long n4;
  int blocks;
  long passes;
};
static inline PackGrid pack_grid(long n) {
  PackGrid g;
  g.n4 = (n + 3) / 4;
  g.blocks = std::max(1, nblocks(g.n4, 4));
  const long threads = (long)g.blocks * TPB;
  g.passes = (g.n4 + threads - 1) / threads;
  return g;
}

// x and y may be the same buffer (in-place Sigmoid): no __restrict__
__global__ void k_sigmoid_fwd(const f4* x, long n, float* y) {
  VEC_GRID(i, (n + 3) / 4) {
    f4 v = x[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = sigmoid_value(v[j]);
    store_pack(y, i, n, v);
  }
}
void sigmoid_fwd(hipStream_t s, const float* x, long n, float* y) {
  PerfScope perf(PERF_CLASS("sigmoid"), s, 0, 8.0 * n);
  const PackGrid g = pack_grid(n);
  hipLaunchKernelGGL(k_sigmoid_fwd, dim3(g.blocks), dim3(TPB), 0, s,
                     (const f4*)x, n, y);
  ktrace(kSigmoidFwd, kVarNone, n, g.blocks, g.passes);
}

// dy and dx may be the same buffer (in-place Sigmoid)
__global__ void k_sigmoid_bwd(const f4* __restrict__ y, const f4* dy, long n,
                              float* dx) {
  VEC_GRID(i, (n + 3) / 4) {
    const f4 v = y[i];
    f4 d = dy[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] *= v[j] * (1.f - v[j]);
    store_pack(dx, i, n, d);
  }
}
void sigmoid_bwd(hipStream_t s, const float* y, const float* dy, long n,
                 float* dx) {
  PerfScope perf(PERF_CLASS("sigmoid"), s, 0, 12.0 * n);
  const PackGrid g = pack_grid(n);
  hipLaunchKernelGGL(k_sigmoid_bwd, dim3(g.blocks), dim3(TPB), 0, s,
                     (const f4*)y, (const f4*)dy, n, dx);
  ktrace(kSigmoidBwd, kVarNone, n, g.blocks, g.passes);
}

// Loss sums, two-stage and deterministic: every thread adds Term(a, b) of
// its packs into one double, the block tree-reduces them in a fixed order
// and stores partials[blockIdx.x]; k_loss_final then adds the partials, again
// in a fixed order, and writes the scaled float.  Same grid for the same n,
// so two forwards of one input agree bit for bit.
struct SigmoidCeTerm {
  __device__ __forceinline__ float operator()(float x, float t) const {
    return sigmoid_ce_term(x, t);
  }
};
struct EuclidTerm {
  __device__ __forceinline__ float operator()(float a, float b) const {
    const float d = a - b;
    return d * d;
  }
};
__device__ __forceinline__ double block_sum(double acc) {
  __shared__ double sh[TPB];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = TPB / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  return sh[0];
}
template <typename Term>
__device__ __forceinline__ void loss_partial(const f4* __restrict__ a,
                                             const f4* __restrict__ b, long n,
                                             double* __restrict__ partials) {
  const Term term;
  double acc = 0;
  VEC_GRID(i, (n + 3) / 4) {
    const f4 va = a[i];
    const f4 vb = b[i];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * i + j < n) acc += (double)term(va[j], vb[j]);
  }
  const double sum = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}
__global__ void k_sigmoid_ce_fwd(const f4* __restrict__ x,
                                 const f4* __restrict__ t, long n,
                                 double* __restrict__ partials) {
  loss_partial<SigmoidCeTerm>(x, t, n, partials);
}
__global__ void k_euclid_fwd(const f4* __restrict__ a,
                             const f4* __restrict__ b, long n,
                             double* __restrict__ partials) {
  loss_partial<EuclidTerm>(a, b, n, partials);
}
// one block: thread k adds partials k, k + TPB, ... then the tree
__global__ void k_loss_final(const double* __restrict__ partials, int np,
                             double scale, float* __restrict__ loss) {
  double acc = 0;
  for (int i = threadIdx.x; i < np; i += TPB) acc += partials[i];
  const double sum = block_sum(acc);
  if (threadIdx.x == 0) loss[0] = (float)(sum * scale);
}
int loss_partials(long n) { return pack_grid(n).blocks; }

template <typename K>
static void loss_fwd_launch(K kernel, int op, hipStream_t s, const float* a,
                            const float* b, long n, double scale,
                            double* partials, float* loss_out) {
  PerfScope perf(PERF_CLASS("loss"), s, 0, 8.0 * n);
  const PackGrid g = pack_grid(n);
  hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(TPB), 0, s, (const f4*)a,
                     (const f4*)b, n, partials);
  hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(TPB), 0, s,
                     (const double*)partials, g.blocks, scale, loss_out);
  ktrace(op, kVarNone, n, g.blocks, g.blocks, g.passes);
}
void sigmoid_ce_fwd(hipStream_t s, const float* x, const float* t, long n,
                    int num, double* partials, float* loss_out) {
  loss_fwd_launch(k_sigmoid_ce_fwd, kSigmoidCeFwd, s, x, t, n, 1.0 / num,
                  partials, loss_out);
}
void euclid_fwd(hipStream_t s, const float* a, const float* b, long n,
                int num, double* partials, float* loss_out) {
  loss_fwd_launch(k_euclid_fwd, kEuclidFwd, s, a, b, n, 0.5 / num, partials,
                  loss_out);
}

__global__ void k_sigmoid_ce_bwd(const f4* __restrict__ x,
                                 const f4* __restrict__ t, long n,
                                 float scale, float* __restrict__ dx) {
  VEC_GRID(i, (n + 3) / 4) {
    f4 v = x[i];
    const f4 tv = t[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (sigmoid_value(v[j]) - tv[j]) * scale;
    store_pack(dx, i, n, v);
  }
}
void sigmoid_ce_bwd(hipStream_t s, const float* x, const float* t, long n,
                    float scale, float* dx) {
  PerfScope perf(PERF_CLASS("loss"), s, 0, 12.0 * n);
  const PackGrid g = pack_grid(n);
  hipLaunchKernelGGL(k_sigmoid_ce_bwd, dim3(g.blocks), dim3(TPB), 0, s,
                     (const f4*)x, (const f4*)t, n, scale, dx);
  ktrace(kSigmoidCeBwd, kVarNone, n, g.blocks, g.passes);
}

// da / db null = that bottom takes no gradient; a zero scale still writes
// (zeros): the split above the bottom sums this diff
__global__ void k_euclid_bwd(const f4* __restrict__ a,
                             const f4* __restrict__ b, long n, float scale_a,
                             float* __restrict__ da, float scale_b,
                             float* __restrict__ db) {
  VEC_GRID(i, (n + 3) / 4) {
    const f4 d = a[i] - b[i];
    if (da) store_pack(da, i, n, d * scale_a);
    if (db) store_pack(db, i, n, d * scale_b);
  }
}
void euclid_bwd(hipStream_t s, const float* a, const float* b, long n,
                float scale_a, float* da, float scale_b, float* db) {
  PerfScope perf(PERF_CLASS("loss"), s, 0,
                 (8.0 + (da ? 4.0 : 0.0) + (db ? 4.0 : 0.0)) * n);
  const PackGrid g = pack_grid(n);
  hipLaunchKernelGGL(k_euclid_bwd, dim3(g.blocks), dim3(TPB), 0, s,
                     (const f4*)a, (const f4*)b, n, scale_a, da, scale_b, db);
  ktrace(kEuclidBwd, kVarNone, n, g.blocks, g.passes);
}

// ContrastiveLoss over a [N][C], b [N][C], sim [N].  Two row mappings: one
// thread per row while a row is narrower than a wave (the siamese net has
// C = 2; a wave per row would idle most lanes), one wave per row from
// kContrastiveWaveC on (a thread per row would walk C elements with its
// neighbours C floats apart, uncoalesced).  The switch point comes from
// reading the two loops, not from a measurement.  Both index rows by scalar
// element, so neither needs C % 4 == 0 or a 16-byte-aligned row start.
// The forward stores each row's d² (double sum in a fixed order, rounded to
// float once) for the backward and feeds the row's loss term into the
// two-stage sum above: one double per thread, block_sum, k_loss_final.
constexpr int kWave = 64;
constexpr int kContrastiveWaveC = kWave;
static inline bool contrastive_row_wave(int C) {
  return C >= kContrastiveWaveC;
}
static inline int contrastive_blocks(int N, int C) {
  const long rows_per_block = contrastive_row_wave(C) ? TPB / kWave : TPB;
  return (int)std::min<long>(2048, std::max<long>(
                                       1, (N + rows_per_block - 1) /
                                              rows_per_block));
}
int contrastive_partials(int N, int C) { return contrastive_blocks(N, C); }

// lane 0 of the wave returns the sum, added in a fixed tree
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;
}

template <bool kRowWave>
__global__ void k_contrastive_fwd(const float* __restrict__ a,
                                  const float* __restrict__ b,
                                  const float* __restrict__ sim, int N, int C,
                                  float margin, int legacy,
                                  float* __restrict__ dist_sq,
                                  double* __restrict__ partials) {
  double acc = 0;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long nthreads = (long)gridDim.x * blockDim.x;
  if (kRowWave) {
    const int lane = threadIdx.x % kWave;
    for (long r = tid / kWave; r < N; r += nthreads / kWave) {
      const float* ar = a + r * C;
      const float* br = b + r * C;
      double s = 0;
      for (int c = lane; c < C; c += kWave) {
        const float d = ar[c] - br[c];
        s += (double)d * (double)d;
      }
      s = wave_sum(s);
      if (lane == 0) {
        const float dsq = (float)s;
        dist_sq[r] = dsq;
        acc += (double)contrastive_row_loss(dsq, (int)sim[r] != 0, margin,
                                            legacy != 0);
      }
    }
  } else {
    for (long r = tid; r < N; r += nthreads) {
      const float* ar = a + r * C;
      const float* br = b + r * C;
      double s = 0;
      for (int c = 0; c < C; ++c) {
        const float d = ar[c] - br[c];
        s += (double)d * (double)d;
      }
      const float dsq = (float)s;
      dist_sq[r] = dsq;
      acc += (double)contrastive_row_loss(dsq, (int)sim[r] != 0, margin,
                                          legacy != 0);
    }
  }
  const double sum = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

void contrastive_fwd(hipStream_t s, const float* a, const float* b,
                     const float* sim, int N, int C, float margin,
                     bool legacy, float* dist_sq, double* partials,
                     float* loss_out) {
  PerfScope perf(PERF_CLASS("loss"), s, 0, 8.0 * N * C + 8.0 * N);
  const int blocks = contrastive_blocks(N, C);
  const bool wave = contrastive_row_wave(C);
  if (wave)
    hipLaunchKernelGGL(k_contrastive_fwd<true>, dim3(blocks), dim3(TPB), 0, s,
                       a, b, sim, N, C, margin, legacy ? 1 : 0, dist_sq,
                       partials);
  else
    hipLaunchKernelGGL(k_contrastive_fwd<false>, dim3(blocks), dim3(TPB), 0, s,
                       a, b, sim, N, C, margin, legacy ? 1 : 0, dist_sq,
                       partials);
  hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(TPB), 0, s,
                     (const double*)partials, blocks, 0.5 / N, loss_out);
  ktrace(kContrastiveFwd, wave ? kVarRowWave : kVarRowThread, N, C, blocks);
}

// a - b is recomputed; the row's coefficient comes from its stored d².
// da / db null = that bottom takes no gradient.  db's coefficient is da's
// negated (alpha only changes sign), and a zero coefficient writes exact
// zeros as the reference's caffe_set does.
template <bool kRowWave>
__global__ void k_contrastive_bwd(const float* __restrict__ a,
                                  const float* __restrict__ b,
                                  const float* __restrict__ sim,
                                  const float* __restrict__ dist_sq, int N,
                                  int C, float margin, int legacy, float alpha,
                                  float* __restrict__ da,
                                  float* __restrict__ db) {
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long nthreads = (long)gridDim.x * blockDim.x;
  const long r0 = kRowWave ? tid / kWave : tid;
  const long rstep = kRowWave ? nthreads / kWave : nthreads;
  const int c0 = kRowWave ? threadIdx.x % kWave : 0;
  const int cstep = kRowWave ? kWave : 1;
  for (long r = r0; r < N; r += rstep) {
    const float coef = contrastive_row_beta(dist_sq[r], (int)sim[r] != 0,
                                            margin, legacy != 0, alpha);
    for (int c = c0; c < C; c += cstep) {
      const long i = r * C + c;
      const float g = coef == 0.f ? 0.f : coef * (a[i] - b[i]);
      if (da) da[i] = g;
      if (db) db[i] = -g;
    }
  }
}

void contrastive_bwd(hipStream_t s, const float* a, const float* b,
                     const float* sim, const float* dist_sq, int N, int C,
                     float margin, bool legacy, float alpha, float* da,
                     float* db) {
  PerfScope perf(PERF_CLASS("loss"), s, 0,
                 (8.0 + (da ? 4.0 : 0.0) + (db ? 4.0 : 0.0)) * N * C);
  const int blocks = contrastive_blocks(N, C);
  const bool wave = contrastive_row_wave(C);
  if (wave)
    hipLaunchKernelGGL(k_contrastive_bwd<true>, dim3(blocks), dim3(TPB), 0, s,
                       a, b, sim, dist_sq, N, C, margin, legacy ? 1 : 0, alpha,
                       da, db);
  else
    hipLaunchKernelGGL(k_contrastive_bwd<false>, dim3(blocks), dim3(TPB), 0,
                       s, a, b, sim, dist_sq, N, C, margin, legacy ? 1 : 0,
                       alpha, da, db);
  ktrace(kContrastiveBwd, wave ? kVarRowWave : kVarRowThread, N, C, blocks);
}

// ------------------------------------------------------- row/col sums
__global__ void k_colsum(const float* __restrict__ A, long M, long N,
                         float* __restrict__ out) {
  GRID_STRIDE(n, N) {
    double acc = 0;
    for (long m = 0; m < M; ++m) acc += A[m * N + n];
    out[n] = (float)acc;
  }
}
void colsum(hipStream_t s, const float* A, long M, long N, float* out) {
  PerfScope perf(PERF_CLASS("reduce"), s, 0, 4.0 * M * N);
  hipLaunchKernelGGL(k_colsum, dim3(nblocks(N)), dim3(TPB), 0, s, A, M, N,
                     out);
}

// ------------------------------------------------------------ eltwise etc.
__global__ void k_axpby(long n, float a, const float* __restrict__ x,
                        float b, float* __restrict__ y) {
  GRID_STRIDE(i, n) y[i] = a * x[i] + b * y[i];
}
void axpby(hipStream_t s, long n, float a, const float* x, float b,
           float* y) {
  PerfScope perf(PERF_CLASS("eltwise"), s, 0, 12.0 * n);
  hipLaunchKernelGGL(k_axpby, dim3(nblocks(n, 8)), dim3(TPB), 0, s, n, a, x,
                     b, y);
}

__global__ void k_copy(long n4, const f4* __restrict__ x,
                       f4* __restrict__ y) {
  VEC_GRID(i, n4) y[i] = x[i];
}
void copy(hipStream_t s, long n, const float* x, float* y) {
  if (x == y) return;
  PerfScope perf(PERF_CLASS("eltwise"), s, 0, 8.0 * n);
  const long n4 = (n + 3) / 4;
  hipLaunchKernelGGL(k_copy, dim3(nblocks(n4, 4)), dim3(TPB), 0, s, n4,
                     (const f4*)x, (f4*)y);
}

__global__ void k_set(long n, float v, float* __restrict__ y) {
  GRID_STRIDE(i, n) y[i] = v;
}
void set_const(hipStream_t s, long n, float v, float* y) {
  hipLaunchKernelGGL(k_set, dim3(nblocks(n, 8)), dim3(TPB), 0, s, n, v, y);
}

__global__ void k_add3(long n4, const f4* __restrict__ a,
                       const f4* __restrict__ b, int frelu,
                       f4* __restrict__ y) {
  VEC_GRID(i, n4) {
    f4 v = a[i] + b[i];
    if (frelu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
    }
    y[i] = v;
  }
}
void add3(hipStream_t s, long n, const float* a, const float* b, float* y,
          int fuse_relu) {
  PerfScope perf(PERF_CLASS("eltwise"), s, 0, 12.0 * n);
  const long n4 = (n + 3) / 4;
  hipLaunchKernelGGL(k_add3, dim3(nblocks(n4, 4)), dim3(TPB), 0, s, n4,
                     (const f4*)a, (const f4*)b, fuse_relu, (f4*)y);
}

__global__ void k_acc(long n4, const f4* __restrict__ x,
                      f4* __restrict__ y) {
  VEC_GRID(i, n4) y[i] += x[i];
}
void acc(hipStream_t s, long n, const float* x, float* y) {
  PerfScope perf(PERF_CLASS("eltwise"), s, 0, 12.0 * n);
  const long n4 = (n + 3) / 4;
  hipLaunchKernelGGL(k_acc, dim3(nblocks(n4, 4)), dim3(TPB), 0, s, n4,
                     (const f4*)x, (f4*)y);
}

__global__ void k_concat_fwd(const float* __restrict__ x, int N, int Cs,
                             long S, int Cd, int c_off,
                             float* __restrict__ y) {
  const long total = (long)N * Cs * S;
  GRID_STRIDE(i, total) {
    const int n = (int)(i / ((long)Cs * S));
    const long rem = i - (long)n * Cs * S;
    y[((long)n * Cd + c_off) * S + rem] = x[i];
  }
}
void concat_fwd(hipStream_t s, const float* x, int N, int Cs, long S, int Cd,
                int c_off, float* y) {
  const long total = (long)N * Cs * S;
  PerfScope perf(PERF_CLASS("concat"), s, 0, 8.0 * total);
  hipLaunchKernelGGL(k_concat_fwd, dim3(nblocks(total, 4)), dim3(TPB), 0, s,
                     x, N, Cs, S, Cd, c_off, y);
}

__global__ void k_concat_bwd(const float* __restrict__ dy, int N, int Cs,
                             long S, int Cd, int c_off,
                             float* __restrict__ dx) {
  const long total = (long)N * Cs * S;
  GRID_STRIDE(i, total) {
    const int n = (int)(i / ((long)Cs * S));
    const long rem = i - (long)n * Cs * S;
    dx[i] = dy[((long)n * Cd + c_off) * S + rem];
  }
}
void concat_bwd(hipStream_t s, const float* dy, int N, int Cs, long S,
                int Cd, int c_off, float* dx) {
  const long total = (long)N * Cs * S;
  PerfScope perf(PERF_CLASS("concat"), s, 0, 8.0 * total);
  hipLaunchKernelGGL(k_concat_bwd, dim3(nblocks(total, 4)), dim3(TPB), 0, s,
                     dy, N, Cs, S, Cd, c_off, dx);
}

// ------------------------------------------------------------ dropout/rng
__device__ __forceinline__ uint64_t d_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ float d_u01(uint64_t h) {
  return (float)((h >> 11) * (1.0 / 9007199254740992.0));
}

__global__ void k_dropout_fwd(const float* __restrict__ x, long n,
                              uint64_t key, float threshold, float scale,
                              float* __restrict__ y,
                              uint8_t* __restrict__ mask) {
  GRID_STRIDE(i, n) {
    const uint8_t m = d_u01(d_splitmix64(key ^ (uint64_t)i)) >= threshold;
    mask[i] = m;
    y[i] = x[i] * m * scale;
  }
}
void dropout_fwd(hipStream_t s, const float* x, long n, uint64_t seed,
                 uint64_t counter, float threshold, float scale, float* y,
                 uint8_t* mask) {
  PerfScope perf(PERF_CLASS("dropout"), s, 0, 9.0 * n);
  (void)counter;  // caller passes the pre-mixed key via `seed`
  hipLaunchKernelGGL(k_dropout_fwd, dim3(nblocks(n, 4)), dim3(TPB), 0, s, x,
                     n, seed, threshold, scale, y, mask);
}

__global__ void k_dropout_bwd(const float* __restrict__ dy,
                              const uint8_t* __restrict__ mask, long n,
                              float scale, float* __restrict__ dx) {
  GRID_STRIDE(i, n) dx[i] = dy[i] * mask[i] * scale;
}
void dropout_bwd(hipStream_t s, const float* dy, const uint8_t* mask, long n,
                 float scale, float* dx) {
  PerfScope perf(PERF_CLASS("dropout"), s, 0, 9.0 * n);
  hipLaunchKernelGGL(k_dropout_bwd, dim3(nblocks(n, 4)), dim3(TPB), 0, s,
                     dy, mask, n, scale, dx);
}

// ------------------------------------------------------------ SGD
// the segment of arena offset i: the largest k with seg_off[k] <= i
__device__ __forceinline__ int seg_find(const long* __restrict__ seg_off,
                                        int nseg, long i) {
  int a = 0, b = nseg - 1;
  while (a < b) {
    const int m = (a + b + 1) >> 1;
    if (seg_off[m] <= i)
      a = m;
    else
      b = m - 1;
  }
  return a;
}

// segmented fused SGD: one launch covers a whole bucket's params.
// segs: sorted arena offsets; per-seg weight base pointer and lr/decay
// MULTIPLIERS (uploaded once — the per-iteration lr/decay ride in as
// kernel args, so no H2D traffic in the iteration loop).
// Elements in inter-param padding update harmlessly (their g is 0).
// The loop is a macro so that k_sgd_seg and its clip_gradients sibling
// compile from the same text: a shared __device__ function changed the
// unclipped kernel's registers, and that kernel is the benchmark's.
#define SGD_SEG_LOOP(GSCALE)                                              \
  for (long i = lo + blockIdx.x * (long)blockDim.x + threadIdx.x; i < hi; \
       i += (long)gridDim.x * blockDim.x) {                               \
    const int a = seg_find(seg_off, nseg, i);                             \
    float* w = w_ptrs[a] + (i - seg_off[a]);                              \
    float gi = g_arena[i] * GSCALE + (decay * decay_mults[a]) * *w;       \
    gi = h_arena[i] = mom * h_arena[i] + (lr * lr_mults[a]) * gi;         \
    *w -= gi;                                                             \
    g_arena[i] = 0.f;                                                     \
  }
__global__ void k_sgd_seg(long lo, long hi, float* __restrict__ g_arena,
                          float* __restrict__ h_arena,
                          const long* __restrict__ seg_off,
                          float* const* __restrict__ w_ptrs,
                          const float* __restrict__ lr_mults,
                          const float* __restrict__ decay_mults, int nseg,
                          float mom, float lr, float decay, float gscale) {
  SGD_SEG_LOOP(gscale)
}
// clip_gradients: the same update with the iteration's clip factor (written
// to device memory by k_clip_final) folded into gscale once per thread
__global__ void k_sgd_seg_clip(long lo, long hi, float* __restrict__ g_arena,
                               float* __restrict__ h_arena,
                               const long* __restrict__ seg_off,
                               float* const* __restrict__ w_ptrs,
                               const float* __restrict__ lr_mults,
                               const float* __restrict__ decay_mults, int nseg,
                               float mom, float lr, float decay, float gscale,
                               const float* __restrict__ factor) {
  const float clipped = gscale * factor[0];
  SGD_SEG_LOOP(clipped)
}
#undef SGD_SEG_LOOP
void sgd_update_segmented(hipStream_t s, long lo, long hi, float* g_arena,
                          float* h_arena, const long* seg_off,
                          float* const* w_ptrs, const float* lr_mults,
                          const float* decay_mults, int nseg, float mom,
                          float lr, float decay, float gscale,
                          const float* clip_factor) {
  PerfScope perf(PERF_CLASS("sgd"), s, 0, 20.0 * (hi - lo));
  if (clip_factor) {
    hipLaunchKernelGGL(k_sgd_seg_clip, dim3(nblocks(hi - lo, 4)), dim3(TPB), 0,
                       s, lo, hi, g_arena, h_arena, seg_off, w_ptrs, lr_mults,
                       decay_mults, nseg, mom, lr, decay, gscale, clip_factor);
    ktrace(kSgdSeg, kVarNone, lo, hi, nseg, 1);
    return;
  }
  hipLaunchKernelGGL(k_sgd_seg, dim3(nblocks(hi - lo, 4)), dim3(TPB), 0, s,
                     lo, hi, g_arena, h_arena, seg_off, w_ptrs, lr_mults,
                     decay_mults, nseg, mom, lr, decay, gscale);
  ktrace(kSgdSeg, kVarNone, lo, hi, nseg);
}

// segmented fused update for the other solver rules (and SGD with L1): the
// k_sgd_seg contract — one launch per bucket over the arena range, segment
// tables uploaded once, per-iteration coefficients as kernel arguments, no
// atomics (each element belongs to one thread: deterministic) — but
// float4-wide.  lo4/hi4 count 4-float packs; arena offsets and padded counts
// are multiples of 16 floats and blob memory is 64B-padded, so a pack never
// straddles a segment, the weight pack is 16B-aligned and in bounds, and
// the binary search runs once per pack.
// Pad lanes have g == 0 and w == 0 (blob memory is zero-filled past count),
// so gr == 0 there for L2 and L1 alike, and from a zeroed history every rule
// leaves them finite: the quotients are 0 / (0 + delta) with delta > 0
// (AdaGrad, RMSProp, Adam) or 0 * sqrt(delta / delta) (AdaDelta).
// The loop is a macro for the reason given at SGD_SEG_LOOP.
#define SOLVER_SEG_LOOP                                                      \
  constexpr bool kTwo = Rule == kRuleAdaDelta || Rule == kRuleAdam;          \
  for (long p = lo4 + blockIdx.x * (long)blockDim.x + threadIdx.x; p < hi4;  \
       p += (long)gridDim.x * blockDim.x) {                                  \
    const long i = 4 * p;                                                    \
    const int a = seg_find(seg_off, nseg, i);                                \
    f4* wp = (f4*)(w_ptrs[a] + (i - seg_off[a]));                            \
    const float lr = c.lr * lr_mults[a];                                     \
    const float decay = c.decay * decay_mults[a];                            \
    const f4 gv = g_arena[p];                                                \
    f4 wv = *wp, hv = h_arena[p];                                            \
    f4 h2v = {0.f, 0.f, 0.f, 0.f};                                           \
    if (kTwo) h2v = h2_arena[p];                                             \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                          \
      float hj = hv[j], h2j = h2v[j];                                        \
      wv[j] -= solver_rule_step<Rule, kL1>(gv[j], wv[j], hj, h2j, c, lr,     \
                                           decay);                           \
      hv[j] = hj;                                                            \
      h2v[j] = h2j;                                                          \
    }                                                                        \
    *wp = wv;                                                                \
    h_arena[p] = hv;                                                         \
    if (kTwo) h2_arena[p] = h2v;                                             \
    g_arena[p] = f4{0.f, 0.f, 0.f, 0.f};                                     \
  }
template <int Rule, bool kL1>
__global__ void k_solver_seg(long lo4, long hi4, f4* __restrict__ g_arena,
                             f4* __restrict__ h_arena,
                             f4* __restrict__ h2_arena,
                             const long* __restrict__ seg_off,
                             float* const* __restrict__ w_ptrs,
                             const float* __restrict__ lr_mults,
                             const float* __restrict__ decay_mults, int nseg,
                             SolverCoef c) {
  SOLVER_SEG_LOOP
}
// clip_gradients: the clip factor folded into c.gscale once per thread
template <int Rule, bool kL1>
__global__ void k_solver_seg_clip(long lo4, long hi4, f4* __restrict__ g_arena,
                                  f4* __restrict__ h_arena,
                                  f4* __restrict__ h2_arena,
                                  const long* __restrict__ seg_off,
                                  float* const* __restrict__ w_ptrs,
                                  const float* __restrict__ lr_mults,
                                  const float* __restrict__ decay_mults,
                                  int nseg, SolverCoef c,
                                  const float* __restrict__ factor) {
  c.gscale *= factor[0];
  SOLVER_SEG_LOOP
}
#undef SOLVER_SEG_LOOP
void solver_update_segmented(hipStream_t s, int rule, bool l1, long lo,
                             long hi, float* g_arena, float* h_arena,
                             float* h2_arena, const long* seg_off,
                             float* const* w_ptrs, const float* lr_mults,
                             const float* decay_mults, int nseg,
                             const SolverCoef& coef,
                             const float* clip_factor) {
  CHECK_(lo % 4 == 0 && hi % 4 == 0)
      << "solver_update_segmented: range [" << lo << ", " << hi
      << ") is not float4-aligned";
  CHECK_(rule >= 0 && rule < kNumSolverRules) << "bad solver rule " << rule;
  const int slots = solver_rule_slots(rule);
  CHECK_(slots == 1 || h2_arena) << "rule " << rule << " needs two slots";
  if (hi <= lo) return;
  PerfScope perf(PERF_CLASS("solver"), s, 0,
                 (16.0 + 8.0 * slots) * (hi - lo));
  const long lo4 = lo / 4, hi4 = hi / 4;
  const dim3 grid(nblocks(hi4 - lo4)), block(TPB);
#define SOLVER_SEG_LAUNCH(R)                                                \
  case R:                                                                   \
    if (clip_factor && l1)                                                  \
      hipLaunchKernelGGL((k_solver_seg_clip<R, true>), grid, block, 0, s,   \
                         lo4, hi4, (f4*)g_arena, (f4*)h_arena,              \
                         (f4*)h2_arena, seg_off, w_ptrs, lr_mults,          \
                         decay_mults, nseg, coef, clip_factor);             \
    else if (clip_factor)                                                   \
      hipLaunchKernelGGL((k_solver_seg_clip<R, false>), grid, block, 0, s,  \
                         lo4, hi4, (f4*)g_arena, (f4*)h_arena,              \
                         (f4*)h2_arena, seg_off, w_ptrs, lr_mults,          \
                         decay_mults, nseg, coef, clip_factor);             \
    else if (l1)                                                            \
      hipLaunchKernelGGL((k_solver_seg<R, true>), grid, block, 0, s, lo4,   \
                         hi4, (f4*)g_arena, (f4*)h_arena, (f4*)h2_arena,    \
                         seg_off, w_ptrs, lr_mults, decay_mults, nseg,      \
                         coef);                                             \
    else                                                                    \
      hipLaunchKernelGGL((k_solver_seg<R, false>), grid, block, 0, s, lo4,  \
                         hi4, (f4*)g_arena, (f4*)h_arena, (f4*)h2_arena,    \
                         seg_off, w_ptrs, lr_mults, decay_mults, nseg,      \
                         coef);                                             \
    break;
  switch (rule) {
    SOLVER_SEG_LAUNCH(kRuleSgd)
    SOLVER_SEG_LAUNCH(kRuleNesterov)
    SOLVER_SEG_LAUNCH(kRuleAdaGrad)
    SOLVER_SEG_LAUNCH(kRuleRmsProp)
    SOLVER_SEG_LAUNCH(kRuleAdaDelta)
    SOLVER_SEG_LAUNCH(kRuleAdam)
  }
#undef SOLVER_SEG_LAUNCH
  ktrace(kSolverSeg, rule * 2 + (l1 ? 1 : 0), lo, hi, nseg,
         clip_factor ? 1 : 0);
}

// ------------------------------------------------------ clip_gradients
// Sum of squares of the arena range [lo4, hi4) (float4 packs), the two-stage
// deterministic form of the loss sums: each square and every add in double,
// one double per block into partials[blockIdx.x], no atomics, same grid for
// the same range.  Arena padding holds zeros, so the padded range is summed
// whole.  One accumulator per thread: the form with four independent loads
// and accumulators (what paid off in k_bn_fwd_stats) measured 12% slower
// here, 5.51 against 6.17 TB/s at 512 MiB (profiles/clip_gradients.txt).
__global__ void k_grad_sumsq(const f4* __restrict__ g_arena, long lo4,
                             long hi4, double* __restrict__ partials) {
  double acc = 0;
  for (long p = lo4 + blockIdx.x * (long)blockDim.x + threadIdx.x; p < hi4;
       p += (long)gridDim.x * blockDim.x) {
    const f4 v = g_arena[p];
    acc += ((double)v[0] * v[0] + (double)v[1] * v[1]) +
           ((double)v[2] * v[2] + (double)v[3] * v[3]);
  }
  const double sum = block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}
int grad_sumsq_partials(long n) { return pack_grid(n).blocks; }
int grad_sumsq(hipStream_t s, const float* g_arena, long lo, long hi,
               double* partials) {
  CHECK_(lo % 4 == 0 && hi % 4 == 0 && lo < hi)
      << "grad_sumsq: range [" << lo << ", " << hi
      << ") is empty or not float4-aligned";
  PerfScope perf(PERF_CLASS("clip"), s, 0, 4.0 * (hi - lo));
  const PackGrid g = pack_grid(hi - lo);
  hipLaunchKernelGGL(k_grad_sumsq, dim3(g.blocks), dim3(TPB), 0, s,
                     (const f4*)g_arena, lo / 4, hi / 4, partials);
  ktrace(kGradSumsq, kVarNone, lo, hi, g.blocks, g.passes);
  return g.blocks;
}

// one block: the partials of every bucket of the iteration in a fixed order
// (thread k adds k, k + TPB, ... then the tree), then the clip formula:
// norm = (float)(sqrt(sumsq) / world), factor = norm > clip ? clip / norm : 1
// written as that comparison, so a NaN norm does not clip.  out = {norm,
// factor}; the clipped update kernels read out[1].
__global__ void k_clip_final(const double* __restrict__ partials, int np,
                             double world, float clip,
                             float* __restrict__ out) {
  double acc = 0;
  for (int i = threadIdx.x; i < np; i += TPB) acc += partials[i];
  const double sum = block_sum(acc);
  if (threadIdx.x == 0) {
    const float norm = (float)(sqrt(sum) / world);
    out[0] = norm;
    out[1] = clip_factor(norm, clip);
  }
}
void clip_finalize(hipStream_t s, const double* partials, int np, int world,
                   float clip, float* norm_factor) {
  PerfScope perf(PERF_CLASS("clip"), s, 0, 8.0 * np);
  hipLaunchKernelGGL(k_clip_final, dim3(1), dim3(TPB), 0, s, partials, np,
                     (double)world, clip, norm_factor);
  ktrace(kClipFinal, kVarNone, np);
}

// Shared params: one owner layer's arena range [lo, hi) gets the diffs of
// its blobs' sharers added.  seg_off holds the arena offset of each of the
// layer's learnable blobs, src_begin[a] .. src_begin[a + 1] bound segment
// a's sources in srcs (none for a blob nobody shares).  float4 packs in a
// grid-stride loop, seg_find once per pack, the sources added in table
// order by the one thread that owns the pack: deterministic, no atomics.
// A sharer has the owner's count and every blob allocation is padded to 16
// floats, so a whole pack is loadable from every source; lanes past count
// add padding to padding.
__global__ void k_shared_diff_sum(long lo4, long hi4, f4* __restrict__ g_arena,
                                  const long* __restrict__ seg_off, int nseg,
                                  const int* __restrict__ src_begin,
                                  const float* const* __restrict__ srcs) {
  for (long p = lo4 + blockIdx.x * (long)blockDim.x + threadIdx.x; p < hi4;
       p += (long)gridDim.x * blockDim.x) {
    const long i = 4 * p;
    const int a = seg_find(seg_off, nseg, i);
    const int s0 = src_begin[a], s1 = src_begin[a + 1];
    if (s0 == s1) continue;
    const long off = i - seg_off[a];
    f4 g = g_arena[p];
    for (int k = s0; k < s1; ++k) g += *(const f4*)(srcs[k] + off);
    g_arena[p] = g;
  }
}
void shared_diff_sum(hipStream_t s, long lo, long hi, float* g_arena,
                     const long* seg_off, int nseg, const int* src_begin,
                     const float* const* srcs, int nsrc) {
  CHECK_(lo % 4 == 0 && hi % 4 == 0)
      << "shared_diff_sum: range [" << lo << ", " << hi
      << ") is not float4-aligned";
  if (hi <= lo || nsrc == 0) return;
  PerfScope perf(PERF_CLASS("shared_diff_sum"), s, 0,
                 4.0 * (hi - lo) * (2 + nsrc));
  const long lo4 = lo / 4, hi4 = hi / 4;
  hipLaunchKernelGGL(k_shared_diff_sum, dim3(nblocks(hi4 - lo4)), dim3(TPB),
                     0, s, lo4, hi4, (f4*)g_arena, seg_off, nseg, src_begin,
                     srcs);
  ktrace(kSharedDiffSum, kVarNone, lo, hi, nseg, nsrc);
}

// ---------------------------------------------------- LMDB transform
// uint8 -> fp32 crop/mirror/mean/scale (reference data_transformer.cu:
// 14-100): one thread per output element; geo = per-image (ho, wo,
// mirror); mean subtracted in SOURCE coordinates (mean_file semantics).
__global__ void k_transform_u8(const uint8_t* __restrict__ in, int N,
                               int C, int inH, int inW, int outH, int outW,
                               const int* __restrict__ geo,
                               const float* __restrict__ mean,
                               int mean_mode, float scale,
                               float* __restrict__ out) {
  const long total = (long)N * C * outH * outW;
  GRID_STRIDE(i, total) {
    const int x = (int)(i % outW);
    const int y = (int)((i / outW) % outH);
    const int c = (int)((i / ((long)outW * outH)) % C);
    const int n = (int)(i / ((long)outW * outH * C));
    const int ho = geo[3 * n], wo = geo[3 * n + 1], mir = geo[3 * n + 2];
    const int sx = wo + (mir ? outW - 1 - x : x);
    const long src = (((long)n * C + c) * inH + ho + y) * inW + sx;
    float m = 0.f;
    if (mean_mode == 1)
      m = mean[c];
    else if (mean_mode == 2)
      m = mean[((long)c * inH + ho + y) * inW + sx];
    out[i] = ((float)in[src] - m) * scale;
  }
}
void transform_u8(hipStream_t s, const uint8_t* in, int N, int C, int inH,
                  int inW, int outH, int outW, const int* geo,
                  const float* mean, int mean_mode, float scale,
                  float* out) {
  const long total = (long)N * C * outH * outW;
  PerfScope perf(PERF_CLASS("data"), s, 0, 5.0 * total);
  hipLaunchKernelGGL(k_transform_u8, dim3(nblocks(total, 4)), dim3(TPB), 0,
                     s, in, N, C, inH, inW, outH, outW, geo, mean,
                     mean_mode, scale, out);
}

// ------------------------------------------------------------ synthetic
__global__ void k_fill_uniform(long n, uint64_t key, float lo, float hi,
                               float* __restrict__ y) {
  GRID_STRIDE(i, n)
  y[i] = lo + (hi - lo) * d_u01(d_splitmix64(key ^ (uint64_t)i));
}
void fill_uniform(hipStream_t s, long n, uint64_t seed, uint64_t counter,
                  float lo, float hi, float* y) {
  PerfScope perf(PERF_CLASS("data"), s, 0, 4.0 * n);
  (void)counter;
  hipLaunchKernelGGL(k_fill_uniform, dim3(nblocks(n, 4)), dim3(TPB), 0, s,
                     n, seed, lo, hi, y);
}

__global__ void k_fill_labels(long n, uint64_t key, int classes,
                              float* __restrict__ y) {
  GRID_STRIDE(i, n)
  y[i] = (float)(d_splitmix64(key ^ 0xABCDull ^ (uint64_t)i) %
                 (uint64_t)classes);
}
void fill_labels(hipStream_t s, long n, uint64_t seed, uint64_t counter,
                 int classes, float* y) {
  (void)counter;
  hipLaunchKernelGGL(k_fill_labels, dim3(nblocks(n)), dim3(TPB), 0, s, n,
                     seed, classes, y);
}

}  // namespace gpu
}  // namespace camd
