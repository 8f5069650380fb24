// depthwise.hip — direct gfx950 kernels for Convolution with group == C
// (one input channel per group, `mult` = Cout / C filters per channel): a
// bandwidth-bound stencil with no contraction worth a matrix instruction,
// so it stays out of the GEMM family.  Forward, dgrad and wgrad read x, dy
// and W as stored (NCHW); there is no col buffer and no flipped-weight
// scratch.  All three are deterministic: no atomics, fixed summation order.
//
// Forward and dgrad share one work split (DwTile).  A block of 256 threads
// owns P (n, c) planes times one TH x TW tile of the produced tensor (y for
// forward, dx for dgrad).  Small planes (one tile covers the plane) take
// several whole planes per block; large planes are cut into 2-D tiles with
// P = 1.  The tile of the tensor that is READ (x, or dy for all `mult`
// filters of the channel) goes into LDS once with its halo, zero-filled
// where it leaves the image, so the inner loops carry no bounds tests; the
// channel's mult*kh*kw weights go to LDS beside it.  Each thread then
// produces runs of kRun adjacent pixels along W: for 3x3 at stride 1 and
// stride 2 the nine weights and a row segment of the tile sit in registers
// and the window slides through them; every other geometry takes a generic
// loop.  Stores are float4 where the address allows and masked scalars
// otherwise (planes of 49 pixels are never 16-byte aligned).
//
// dgrad is the gather form: dx[h][w] sums dy[oh][ow] * w[ki][kj] over the
// taps with oh*sh + ki*dh - ph == h (likewise in w), so every dx element is
// written exactly once and no zero-fill pass is needed.  At stride 2 a 3x3
// reaches at most 2x2 outputs per pixel, picked by the parity of h + ph and
// w + pw.
//
// wgrad is two-stage, in the shape of bias_grad: grid = output channels x
// batch slices, each thread keeps kh*kw fp32 sums over its strip (3x3) or
// walks the taps one by one (generic), sums cross the wave by shuffles and
// the block through LDS, per-(channel, slice) partials are written in
// double and a second kernel adds the slices in fixed order.  The same pass
// accumulates the bias gradient: dy is being read anyway.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../layers.hpp"

namespace camd {
namespace gpu {
namespace {

constexpr int kTPB = 256;
constexpr int kRun = 4;             // adjacent pixels per thread along W
constexpr int kLdsFloats = 12288;   // 48 KB: read tile(s) + weights
constexpr int kMaxPlanes = 32;      // planes per block, small-plane split

enum DwKind { kK3S1, kK3S2, kGeneric };

// launch shape of forward / dgrad
struct DwTile {
  int P;        // (n, c) planes per block
  int TH, TW;   // tile of produced pixels; TW is a multiple of kRun
  int ty, tx;   // tiles per plane
  int LH, LW;   // LDS tile of the read tensor, per read plane
  int blocks;
  bool fits;    // the smallest tile fits kLdsFloats
  FastDiv fd_per, fd_lw, fd_rw, fd_th, fd_mult, fd_tx;
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return ceil_div(a, b) * b; }

// dgrad = true: tiles over dx (H x W), LDS holds dy for all mult filters
DwTile dw_tile(const DwConv& g, bool dgrad) {
  const int EH = dgrad ? g.H : g.OH, EW = dgrad ? g.W : g.OW;
  const int read_planes = dgrad ? g.mult : 1;  // LDS planes per (n, c)
  const int item_planes = dgrad ? 1 : g.mult;  // produced planes per (n, c)
  const int wfloats = g.mult * (g.kh * g.kw + 1);
  // rows / columns of the read tensor a tile of th x tw pixels touches.
  // dgrad: the first row is floor((h0 + ph - (kh-1)*dh) / sh) and the last
  // floor((h0 + th-1 + ph) / sh), at most this many apart (floor(a + b) <=
  // floor(a) + floor(b) + 1)
  auto lh = [&](int th) {
    return dgrad ? (th - 1 + (g.kh - 1) * g.dh) / g.sh + 2
                 : (th - 1) * g.sh + (g.kh - 1) * g.dh + 1;
  };
  auto lw = [&](int tw) {
    return dgrad ? (tw - 1 + (g.kw - 1) * g.dw) / g.sw + 2
                 : (tw - 1) * g.sw + (g.kw - 1) * g.dw + 1;
  };
  auto floats = [&](int th, int tw) {
    return (long)read_planes * lh(th) * lw(tw) + wfloats;
  };
  DwTile t{};
  // balanced column tiles of at most 64, then rows to fill the block
  t.tx = ceil_div(EW, 64);
  t.TW = round_up(ceil_div(EW, t.tx), kRun);
  t.TH = std::max(1, std::min(EH, kTPB / (t.TW / kRun)));
  while (floats(t.TH, t.TW) > kLdsFloats && t.TH > 1) t.TH = (t.TH + 1) / 2;
  while (floats(t.TH, t.TW) > kLdsFloats && t.TW > kRun)
    t.TW = std::max(kRun, round_up(t.TW / 2, kRun));
  t.fits = floats(t.TH, t.TW) <= kLdsFloats;
  t.ty = ceil_div(EH, t.TH);
  t.TH = ceil_div(EH, t.ty);
  t.tx = ceil_div(EW, t.TW);
  t.LH = lh(t.TH);
  t.LW = lw(t.TW);
  t.P = 1;
  const long planes = (long)g.N * g.C;
  if (t.ty * t.tx == 1) {  // small planes: several whole planes per block
    const int items = item_planes * t.TH * (t.TW / kRun);
    t.P = (int)std::min<long>(
        planes, std::max(1, std::min(kMaxPlanes, kTPB / items)));
    while (t.P > 1 && t.P * floats(t.TH, t.TW) > kLdsFloats) --t.P;
  }
  t.blocks = (int)((planes + t.P - 1) / t.P) * t.ty * t.tx;
  t.fd_per = fastdiv_make((unsigned long)t.LH * t.LW);
  t.fd_lw = fastdiv_make(t.LW);
  t.fd_rw = fastdiv_make(t.TW / kRun);
  t.fd_th = fastdiv_make(t.TH);
  t.fd_mult = fastdiv_make(g.mult);
  t.fd_tx = fastdiv_make(t.tx);
  return t;
}

DwKind dw_kind(const DwConv& g) {
  if (g.kh == 3 && g.kw == 3 && g.dh == 1 && g.dw == 1) {
    if (g.sh == 1 && g.sw == 1) return kK3S1;
    if (g.sh == 2 && g.sw == 2) return kK3S2;
  }
  return kGeneric;
}

// floor(a / b) for b > 0 and any a
__device__ inline int floor_div(int a, int b) {
  const int q = a / b;
  return q * b > a ? q - 1 : q;
}

// the block's tile: plane group and tile origin in the produced tensor
struct DwBlock {
  int pl0, r0, c0;
};
__device__ inline DwBlock dw_block(const DwTile& t) {
  const int tiles = t.ty * t.tx;
  const int pb = blockIdx.x / tiles;
  const int tl = blockIdx.x - pb * tiles;
  const int tyi = (int)fastdiv(tl, t.fd_tx);
  return {pb * t.P, tyi * t.TH, (tl - tyi * t.tx) * t.TW};
}

// weights of the block's planes into LDS: ws[p][j][taps + 1], the filter's
// bias (0 without one) in the last slot
__device__ inline void dw_stage_weights(const DwConv& g, const DwTile& t,
                                        int pl0, const float* __restrict__ w,
                                        const float* __restrict__ bias,
                                        float* ws) {
  const int taps = g.kh * g.kw;
  const int per = g.mult * (taps + 1);
  const int planes = g.N * g.C;
  for (int i = threadIdx.x; i < t.P * per; i += kTPB) {
    const int p = i / per;
    const int e = i - p * per;
    const int j = e / (taps + 1), tt = e - j * (taps + 1);
    const int co = ((pl0 + p) % g.C) * g.mult + j;
    float v = 0.f;
    if (pl0 + p < planes) {
      if (tt < taps)
        v = w[co * taps + tt];
      else if (bias)
        v = bias[co];
    }
    ws[i] = v;
  }
}

// a run of kRun pixels at element offset o of dst; n_ok of them inside the row
__device__ inline void dw_store_run(float* __restrict__ dst, int o,
                                    const float (&v)[kRun], int n_ok) {
  float* p = dst + o;
  if (n_ok >= kRun && ((uintptr_t)p & 15) == 0) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < kRun; ++i)
      if (i < n_ok) p[i] = v[i];
  }
}

// ---------------------------------------------------------------- forward
template <int KIND>
__global__ __launch_bounds__(kTPB) void k_dwconv_fwd(
    DwConv g, DwTile t, const float* __restrict__ x,
    const float* __restrict__ w, const float* __restrict__ bias, int relu,
    float* __restrict__ y) {
  extern __shared__ float lds[];
  const int per = t.LH * t.LW;
  const int taps = g.kh * g.kw;
  float* xs = lds;               // [P][LH][LW]
  float* ws = lds + t.P * per;   // [P][mult][taps + 1]
  const DwBlock b = dw_block(t);
  const int planes = g.N * g.C;
  const int h0 = b.r0 * g.sh - g.ph, w0 = b.c0 * g.sw - g.pw;
  for (int i = threadIdx.x; i < t.P * per; i += kTPB) {
    const int p = (int)fastdiv(i, t.fd_per);
    const int rem = i - p * per;
    const int r = (int)fastdiv(rem, t.fd_lw);
    const int h = h0 + r, wc = w0 + (rem - r * t.LW);
    const int pl = b.pl0 + p;
    float v = 0.f;
    if (pl < planes && (unsigned)h < (unsigned)g.H &&
        (unsigned)wc < (unsigned)g.W)
      v = x[(pl * g.H + h) * g.W + wc];
    xs[i] = v;
  }
  dw_stage_weights(g, t, b.pl0, w, bias, ws);
  __syncthreads();

  const int RW = t.TW / kRun;
  const int items = t.P * g.mult * t.TH * RW;
  for (int it = threadIdx.x; it < items; it += kTPB) {
    int rest = (int)fastdiv(it, t.fd_rw);
    const int q = it - rest * RW;
    int nx = (int)fastdiv(rest, t.fd_th);
    const int r = rest - nx * t.TH;
    const int p = (int)fastdiv(nx, t.fd_mult);
    const int j = nx - p * g.mult;
    const int pl = b.pl0 + p, oh = b.r0 + r, ow = b.c0 + q * kRun;
    if (pl >= planes || oh >= g.OH || ow >= g.OW) continue;
    const float* xp = xs + p * per + r * g.sh * t.LW + q * kRun * g.sw;
    const float* wp = ws + (p * g.mult + j) * (taps + 1);
    float acc[kRun] = {0.f, 0.f, 0.f, 0.f};
    if (KIND == kGeneric) {
      for (int ki = 0; ki < g.kh; ++ki)
        for (int kj = 0; kj < g.kw; ++kj) {
          const float wv = wp[ki * g.kw + kj];
          const float* row = xp + ki * g.dh * t.LW + kj * g.dw;
#pragma unroll
          for (int i = 0; i < kRun; ++i) acc[i] += row[i * g.sw] * wv;
        }
    } else {
      constexpr int S = KIND == kK3S1 ? 1 : 2;
      constexpr int NV = (kRun - 1) * S + 3;  // row segment under the run
      float k[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) k[i] = wp[i];
#pragma unroll
      for (int ki = 0; ki < 3; ++ki) {
        float v[NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) v[c] = xp[ki * t.LW + c];
#pragma unroll
        for (int i = 0; i < kRun; ++i)
#pragma unroll
          for (int kj = 0; kj < 3; ++kj) acc[i] += v[i * S + kj] * k[ki * 3 + kj];
      }
    }
    const int co = pl * g.mult + j;  // == n*Cout + c*mult + j
    const float bv = wp[taps];
#pragma unroll
    for (int i = 0; i < kRun; ++i) {
      acc[i] += bv;
      if (relu) acc[i] = acc[i] > 0.f ? acc[i] : 0.f;
    }
    dw_store_run(y, (co * g.OH + oh) * g.OW + ow, acc, g.OW - ow);
  }
}

// ------------------------------------------------------------------ dgrad
template <int KIND>
__global__ __launch_bounds__(kTPB) void k_dwconv_bwd_data(
    DwConv g, DwTile t, const float* __restrict__ dy,
    const float* __restrict__ w, float* __restrict__ dx) {
  extern __shared__ float lds[];
  const int per = t.LH * t.LW;
  const int taps = g.kh * g.kw;
  float* ds = lds;                        // [P][mult][LH][LW]
  float* ws = lds + t.P * g.mult * per;   // [P][mult][taps + 1]
  const DwBlock b = dw_block(t);
  const int planes = g.N * g.C;
  // first dy row / column any pixel of the tile can reach
  const int oh_lo = floor_div(b.r0 + g.ph - (g.kh - 1) * g.dh, g.sh);
  const int ow_lo = floor_div(b.c0 + g.pw - (g.kw - 1) * g.dw, g.sw);
  const int yplanes = planes * g.mult;
  for (int i = threadIdx.x; i < t.P * g.mult * per; i += kTPB) {
    const int pm = (int)fastdiv(i, t.fd_per);
    const int rem = i - pm * per;
    const int r = (int)fastdiv(rem, t.fd_lw);
    const int oh = oh_lo + r, ow = ow_lo + (rem - r * t.LW);
    const int yp = b.pl0 * g.mult + pm;
    float v = 0.f;
    if (yp < yplanes && (unsigned)oh < (unsigned)g.OH &&
        (unsigned)ow < (unsigned)g.OW)
      v = dy[(yp * g.OH + oh) * g.OW + ow];
    ds[i] = v;
  }
  dw_stage_weights(g, t, b.pl0, w, nullptr, ws);
  __syncthreads();

  const int RW = t.TW / kRun;
  const int items = t.P * t.TH * RW;
  for (int it = threadIdx.x; it < items; it += kTPB) {
    const int rest = (int)fastdiv(it, t.fd_rw);
    const int q = it - rest * RW;
    const int p = (int)fastdiv(rest, t.fd_th);
    const int r = rest - p * t.TH;
    const int pl = b.pl0 + p, h = b.r0 + r, wq = b.c0 + q * kRun;
    if (pl >= planes || h >= g.H || wq >= g.W) continue;
    float acc[kRun] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < g.mult; ++j) {
      const float* dp = ds + (p * g.mult + j) * per;
      const float* wp = ws + (p * g.mult + j) * (taps + 1);
      if (KIND == kK3S1) {
        // dy rows h+ph-ki, columns w+pw-kj: a 3 x (kRun+2) patch
        float k[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) k[i] = wp[i];
        const int lc = wq + g.pw - 2 - ow_lo;
#pragma unroll
        for (int ki = 0; ki < 3; ++ki) {
          const float* row = dp + (h + g.ph - ki - oh_lo) * t.LW + lc;
          float v[kRun + 2];
#pragma unroll
          for (int c = 0; c < kRun + 2; ++c) v[c] = row[c];
#pragma unroll
          for (int i = 0; i < kRun; ++i)
#pragma unroll
            for (int kj = 0; kj < 3; ++kj)
              acc[i] += v[i + 2 - kj] * k[ki * 3 + kj];
        }
      } else if (KIND == kK3S2) {
        // parity picks the taps: a = h + ph even -> ki 0 (row a/2) and ki 2
        // (row a/2 - 1); odd -> ki 1 (row a/2) alone.  Likewise in w.
        float k[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) k[i] = wp[i];
        const int a = h + g.ph;
        const bool odd_h = a & 1;
        const float* row0 = dp + ((a >> 1) - oh_lo) * t.LW - ow_lo;
        const float* row1 = row0 - t.LW;
        float kr0[3], kr1[3];
#pragma unroll
        for (int kj = 0; kj < 3; ++kj) {
          kr0[kj] = odd_h ? k[3 + kj] : k[kj];
          kr1[kj] = k[6 + kj];
        }
#pragma unroll
        for (int i = 0; i < kRun; ++i) {
          const int bb = wq + i + g.pw;
          const int c = bb >> 1;
          const bool odd_w = bb & 1;
          const float d00 = row0[c];
          const float d01 = odd_w ? 0.f : row0[c - 1];
          const float d10 = odd_h ? 0.f : row1[c];
          const float d11 = odd_h || odd_w ? 0.f : row1[c - 1];
          const float k00 = odd_w ? kr0[1] : kr0[0];
          const float k10 = odd_w ? kr1[1] : kr1[0];
          acc[i] += d00 * k00 + d01 * kr0[2] + d10 * k10 + d11 * kr1[2];
        }
      } else {
        for (int ki = 0; ki < g.kh; ++ki) {
          const int th = h + g.ph - ki * g.dh;
          const int oh = th / g.sh;
          if (oh * g.sh != th) continue;
          const float* row = dp + (oh - oh_lo) * t.LW - ow_lo;
          for (int kj = 0; kj < g.kw; ++kj) {
            const float wv = wp[ki * g.kw + kj];
#pragma unroll
            for (int i = 0; i < kRun; ++i) {
              const int tw = wq + i + g.pw - kj * g.dw;
              const int ow = tw / g.sw;
              if (ow * g.sw == tw) acc[i] += row[ow] * wv;
            }
          }
        }
      }
    }
    dw_store_run(dx, (pl * g.H + h) * g.W + wq, acc, g.W - wq);
  }
}

// ------------------------------------------------------------------ wgrad
// part[(co * nb + slice) * (taps + 1) + t]: tap sums, then Σ dy at t = taps
template <int NV>
__device__ inline void dw_block_sum(float (&v)[NV], float (*red)[NV]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off, 64);
    if (lane == 0) red[wave][i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i)
    v[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  __syncthreads();
}

template <bool K3>
__global__ __launch_bounds__(kTPB) void k_dwconv_wgrad_part(
    DwConv g, const float* __restrict__ x, const float* __restrict__ dy,
    int nb, int want_bias, FastDiv fd_S, FastDiv fd_OW,
    double* __restrict__ part) {
  const int Cout = g.C * g.mult;
  const int co = blockIdx.x % Cout, slice = blockIdx.x / Cout;
  const int c = co / g.mult;
  const int n0 = (int)((long)g.N * slice / nb);
  const int n1 = (int)((long)g.N * (slice + 1) / nb);
  const int S = g.OH * g.OW, HW = g.H * g.W;
  const int span = (n1 - n0) * S;
  const int taps = g.kh * g.kw;
  double* out = part + ((long)co * nb + slice) * (taps + 1);
  if (K3) {
    __shared__ float red[4][10];
    float acc[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) acc[i] = 0.f;
    for (int i = threadIdx.x; i < span; i += kTPB) {
      const int dn = (int)fastdiv(i, fd_S);
      const int s = i - dn * S;
      const int oh = (int)fastdiv(s, fd_OW), ow = s - oh * g.OW;
      const int n = n0 + dn;
      const float d = dy[(n * Cout + co) * S + s];
      const float* xp = x + (n * g.C + c) * HW;
      const int hb = oh * g.sh - g.ph, wb = ow * g.sw - g.pw;
#pragma unroll
      for (int ki = 0; ki < 3; ++ki) {
        const int h = hb + ki * g.dh;
        const bool hok = (unsigned)h < (unsigned)g.H;
#pragma unroll
        for (int kj = 0; kj < 3; ++kj) {
          const int wc = wb + kj * g.dw;
          const float xv =
              hok && (unsigned)wc < (unsigned)g.W ? xp[h * g.W + wc] : 0.f;
          acc[ki * 3 + kj] += d * xv;
        }
      }
      acc[9] += d;
    }
    dw_block_sum<10>(acc, red);
    if (threadIdx.x < 10 && (threadIdx.x < 9 || want_bias))
      out[threadIdx.x] = (double)acc[threadIdx.x];
  } else {
    // generic: one tap at a time (t == taps is the bias sum), dy re-read
    // from cache; a register array indexed by a runtime tap would spill
    __shared__ float red[4][1];
    for (int t = 0; t < taps + (want_bias ? 1 : 0); ++t) {
      const int ki = t / g.kw, kj = t - ki * g.kw;
      float acc[1] = {0.f};
      for (int i = threadIdx.x; i < span; i += kTPB) {
        const int dn = (int)fastdiv(i, fd_S);
        const int s = i - dn * S;
        const int n = n0 + dn;
        const float d = dy[(n * Cout + co) * S + s];
        if (t == taps) {
          acc[0] += d;
          continue;
        }
        const int oh = (int)fastdiv(s, fd_OW), ow = s - oh * g.OW;
        const int h = oh * g.sh - g.ph + ki * g.dh;
        const int wc = ow * g.sw - g.pw + kj * g.dw;
        if ((unsigned)h < (unsigned)g.H && (unsigned)wc < (unsigned)g.W)
          acc[0] += d * x[(n * g.C + c) * HW + h * g.W + wc];
      }
      dw_block_sum<1>(acc, red);
      if (threadIdx.x == 0) out[t] = (double)acc[0];
    }
  }
}

__global__ void k_dwconv_wgrad_fin(const double* __restrict__ part, int nb,
                                   int Cout, int taps, int want_bias,
                                   float* __restrict__ dw,
                                   float* __restrict__ db) {
  const int total = Cout * (taps + 1);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    const int co = i / (taps + 1), t = i - co * (taps + 1);
    if (t == taps && !want_bias) continue;
    double acc = 0;
    for (int s = 0; s < nb; ++s)
      acc += part[((long)co * nb + s) * (taps + 1) + t];
    if (t == taps)
      db[co] = (float)acc;
    else
      dw[co * taps + t] = (float)acc;
  }
}

// the kernels index in 32 bits
void dw_check_counts(const DwConv& g) {
  const long lim = 1L << 31;
  CHECK_((long)g.N * g.C * g.H * g.W < lim &&
         (long)g.N * g.C * g.mult * g.OH * g.OW < lim)
      << "depthwise conv: tensor of 2^31 elements or more";
}

int dw_var(DwKind k, const DwTile& t) {
  return (int)k * 2 + (t.ty * t.tx == 1 ? 0 : 1);
}

size_t dw_lds_bytes(const DwConv& g, const DwTile& t, int read_planes) {
  return sizeof(float) * (size_t)t.P *
         ((size_t)read_planes * t.LH * t.LW +
          (size_t)g.mult * (g.kh * g.kw + 1));
}

}  // namespace

bool dwconv_supported(const DwConv& g) {
  return dw_tile(g, false).fits && dw_tile(g, true).fits;
}

void dwconv_fwd(hipStream_t s, const DwConv& g, const float* x,
                const float* w, const float* bias, bool relu, float* y) {
  dw_check_counts(g);
  const double nx = (double)g.N * g.C * g.H * g.W;
  const double ny = (double)g.N * g.C * g.mult * g.OH * g.OW;
  const double nw = (double)g.C * g.mult * g.kh * g.kw;
  PerfScope perf(PERF_CLASS("dwconv"), s, 2.0 * g.kh * g.kw * ny,
                 4.0 * (nx + ny + nw));
  const DwTile t = dw_tile(g, false);
  CHECK_(t.fits) << "depthwise conv: window does not fit the LDS tile";
  const DwKind k = dw_kind(g);
  const size_t lds = dw_lds_bytes(g, t, 1);
  const dim3 grid(t.blocks), block(kTPB);
  if (k == kK3S1)
    hipLaunchKernelGGL(k_dwconv_fwd<kK3S1>, grid, block, lds, s, g, t, x, w,
                       bias, (int)relu, y);
  else if (k == kK3S2)
    hipLaunchKernelGGL(k_dwconv_fwd<kK3S2>, grid, block, lds, s, g, t, x, w,
                       bias, (int)relu, y);
  else
    hipLaunchKernelGGL(k_dwconv_fwd<kGeneric>, grid, block, lds, s, g, t, x,
                       w, bias, (int)relu, y);
  kernel_trace_dwconv(0, dw_var(k, t), t.P, t.ty, t.tx, t.blocks);
}

void dwconv_bwd_data(hipStream_t s, const DwConv& g, const float* dy,
                     const float* w, float* dx) {
  dw_check_counts(g);
  const double nx = (double)g.N * g.C * g.H * g.W;
  const double ny = (double)g.N * g.C * g.mult * g.OH * g.OW;
  const double nw = (double)g.C * g.mult * g.kh * g.kw;
  PerfScope perf(PERF_CLASS("dwconv"), s, 2.0 * g.kh * g.kw * ny,
                 4.0 * (nx + ny + nw));
  const DwTile t = dw_tile(g, true);
  CHECK_(t.fits) << "depthwise conv: window does not fit the LDS tile";
  const DwKind k = dw_kind(g);
  const size_t lds = dw_lds_bytes(g, t, g.mult);
  const dim3 grid(t.blocks), block(kTPB);
  if (k == kK3S1)
    hipLaunchKernelGGL(k_dwconv_bwd_data<kK3S1>, grid, block, lds, s, g, t,
                       dy, w, dx);
  else if (k == kK3S2)
    hipLaunchKernelGGL(k_dwconv_bwd_data<kK3S2>, grid, block, lds, s, g, t,
                       dy, w, dx);
  else
    hipLaunchKernelGGL(k_dwconv_bwd_data<kGeneric>, grid, block, lds, s, g,
                       t, dy, w, dx);
  kernel_trace_dwconv(1, dw_var(k, t), t.P, t.ty, t.tx, t.blocks);
}

void dwconv_bwd_weight(hipStream_t s, const DwConv& g, const float* x,
                       const float* dy, float* dw, float* db) {
  dw_check_counts(g);
  const double nx = (double)g.N * g.C * g.H * g.W;
  const double ny = (double)g.N * g.C * g.mult * g.OH * g.OW;
  PerfScope perf(PERF_CLASS("dwconv"), s, 2.0 * g.kh * g.kw * ny,
                 4.0 * (nx + ny));
  const int Cout = g.C * g.mult, taps = g.kh * g.kw;
  const long S = (long)g.OH * g.OW;
  // batch slices: enough blocks to fill the device, at least 512 pixels
  // (two per thread) per slice
  const int nb = (int)std::max<long>(
      1, std::min<long>({(long)g.N, 2048L / Cout, (g.N * S + 511) / 512}));
  double* part = (double*)Workspace::get_global().get(
      Workspace::kDwPart, sizeof(double) * (size_t)Cout * nb * (taps + 1));
  const bool k3 = g.kh == 3 && g.kw == 3;
  const FastDiv fd_S = fastdiv_make(S), fd_OW = fastdiv_make(g.OW);
  const int want_bias = db != nullptr;
  if (k3)
    hipLaunchKernelGGL(k_dwconv_wgrad_part<true>, dim3(Cout * nb),
                       dim3(kTPB), 0, s, g, x, dy, nb, want_bias, fd_S,
                       fd_OW, part);
  else
    hipLaunchKernelGGL(k_dwconv_wgrad_part<false>, dim3(Cout * nb),
                       dim3(kTPB), 0, s, g, x, dy, nb, want_bias, fd_S,
                       fd_OW, part);
  const int total = Cout * (taps + 1);
  hipLaunchKernelGGL(k_dwconv_wgrad_fin,
                     dim3(std::min((total + kTPB - 1) / kTPB, 2048)),
                     dim3(kTPB), 0, s, part, nb, Cout, taps, want_bias, dw,
                     db);
  kernel_trace_dwconv(2, k3 ? 0 : 1, nb, want_bias, 0, Cout * nb);
}

}  // namespace gpu
}  // namespace camd
