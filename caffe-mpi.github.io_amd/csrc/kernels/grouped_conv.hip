// grouped_conv.hip — direct gfx950 kernels for Convolution with a small
// number of channels per group (cig = C/group in 4..32, cog = Cout/group in
// 1..32, group >= 8: the ResNeXt / ShuffleNet class).  The per-group GEMM
// loop runs `group` GEMMs of M = cog per pass; at cog < 32 most rows of the
// smallest MFMA tile idle and every launch is latency.  On this part the
// fp32 vector and matrix peaks are the same figure, so these are VALU
// stencils on LDS tiles with register blocking, not per-group MFMA tiles.
// Forward, dgrad and wgrad read x, dy and W as stored (NCHW); there is no
// col buffer and no flipped-weight scratch.  All are deterministic: no
// atomics, fixed summation order.
//
// Forward and dgrad share one work split (GcTile).  A block of 256 threads
// owns one group, P images and one TH x TW tile of the produced tensor (y
// for forward, dx for dgrad); small planes take several images per block,
// large planes are cut into 2-D tiles with P = 1.  The tile of the tensor
// that is READ goes to LDS with its halo, zero-filled where it leaves the
// image, for a chunk of cc of the group's read channels (cig for forward,
// cog for dgrad); beside it go the group's weights for that chunk, re-laid
// so that the produced channels of one (read channel, tap) are contiguous
// ([ci][tap][co] forward, [co][tap][ci] dgrad, padded to the channel block)
// and are read as broadcast 128-bit loads.  A thread owns ONE item: kRun
// adjacent pixels along W times a block of MB (4 or 8) produced channels,
// MB * kRun accumulators that stay in registers while the block loops over
// the channel chunks.  One LDS tile value feeds MB FMAs, one weight kRun.
// 3x3 at stride 1 and 2 keep the row segment in registers; every other
// geometry takes a generic tap loop.
//
// dgrad is the gather form: every dx element is written exactly once, no
// zero fill.  At stride 2 a 3x3 reaches at most 2x2 outputs per pixel,
// picked by the parity of h + ph and w + pw; the generic form tests
// divisibility once per tap, outside the channel loop.
//
// wgrad is two-stage: grid = groups x batch slices (x unit passes, generic).
// A block stages a band of dy rows (all cog channels) and the x rows under
// it (all cig channels) in LDS, image by image.  3x3: a thread owns one
// input channel and NP (1, 2, 4) output channels with all nine taps of each
// as accumulators (at most 40 with the Σ dy of each), and walks the band in
// runs of kRun pixels with the x row segment in registers: 22 LDS reads for
// 36 * NP FMAs.  Generic: a thread owns one (input channel, tap) unit and
// all cog output channels of it; the bias gradient is one more unit whose x
// is 1.  Threads left over split the band's runs between them and are added
// in fixed order through LDS.  Per-(group, slice) partials are written in
// double and a second kernel adds the slices in order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../layers.hpp"

namespace camd {
namespace gpu {
namespace {

constexpr int kTPB = 256;
constexpr int kRun = 4;             // adjacent pixels per thread along W
constexpr int kLdsFloats = 16384;   // 64 KB per block: two blocks per CU
constexpr int kMaxImages = 16;      // images per block, small-plane split

enum GcKind { kK3S1, kK3S2, kGeneric };

// launch shape of forward / dgrad.  "read" channels are the contraction
// (cig forward, cog dgrad), "produced" channels the other side.
struct GcTile {
  int P;            // images per block
  int TH, TW;       // tile of produced pixels; TW is a multiple of kRun
  int ty, tx;       // tiles per plane
  int LH, LW;       // LDS tile of the read tensor, per read channel
  int cc, chunks;   // read channels per LDS chunk, chunks per block
  int mb, nmb, pcp; // produced-channel block, blocks, padded channel count
  int xs_floats;    // P * cc * LH * LW, rounded up to a float4
  int nb;           // image blocks: ceil(N / P)
  int blocks;
  bool fits;
  FastDiv fd_per, fd_lw, fd_cc, fd_ct, fd_taps, fd_pcp;
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return ceil_div(a, b) * b; }

GcTile gc_tile(const GConv& g, bool dgrad) {
  const int EH = dgrad ? g.H : g.OH, EW = dgrad ? g.W : g.OW;
  const int rc = dgrad ? g.cog : g.cig, pc = dgrad ? g.cig : g.cog;
  const int taps = g.kh * g.kw;
  GcTile t{};
  // 8 channels per thread where that pads no more than 4 would
  t.mb = round_up(pc, 8) == round_up(pc, 4) ? 8 : 4;
  t.pcp = round_up(pc, t.mb);
  t.nmb = t.pcp / t.mb;
  // rows / columns of the read tensor under th x tw produced pixels (dgrad:
  // floor((h0 + ph - (kh-1)*dh) / sh) .. floor((h0 + th-1 + ph) / sh))
  auto lh = [&](int th) {
    return dgrad ? (th - 1 + (g.kh - 1) * g.dh) / g.sh + 2
                 : (th - 1) * g.sh + (g.kh - 1) * g.dh + 1;
  };
  auto lw = [&](int tw) {
    return dgrad ? (tw - 1 + (g.kw - 1) * g.dw) / g.sw + 2
                 : (tw - 1) * g.sw + (g.kw - 1) * g.dw + 1;
  };
  auto floats = [&](int P, int th, int tw, int cc) {
    return (long)round_up(P * cc * lh(th) * lw(tw), 4) +
           (long)cc * taps * t.pcp;
  };
  // balanced column tiles, narrower when a pixel run has several channel
  // blocks, then rows until every thread has its one item
  const int max_tw = std::max(16, 64 / t.nmb);
  t.tx = ceil_div(EW, max_tw);
  t.TW = round_up(ceil_div(EW, t.tx), kRun);
  t.TH = std::max(1, std::min(EH, kTPB / (t.TW / kRun * t.nmb)));
  t.cc = rc;
  while (floats(1, t.TH, t.TW, t.cc) > kLdsFloats && t.cc > 4)
    t.cc = (t.cc + 1) / 2;
  while (floats(1, t.TH, t.TW, t.cc) > kLdsFloats && t.TH > 1)
    t.TH = (t.TH + 1) / 2;
  while (floats(1, t.TH, t.TW, t.cc) > kLdsFloats && t.TW > kRun)
    t.TW = std::max(kRun, round_up(t.TW / 2, kRun));
  while (floats(1, t.TH, t.TW, t.cc) > kLdsFloats && t.cc > 1)
    t.cc = (t.cc + 1) / 2;
  t.fits = floats(1, t.TH, t.TW, t.cc) <= kLdsFloats;
  t.ty = ceil_div(EH, t.TH);
  t.TH = ceil_div(EH, t.ty);
  t.tx = ceil_div(EW, t.TW);
  t.chunks = ceil_div(rc, t.cc);
  t.cc = ceil_div(rc, t.chunks);
  t.P = 1;
  if (t.ty * t.tx == 1) {  // small planes: several images per block
    const int items = t.nmb * t.TH * (t.TW / kRun);
    t.P = std::min(g.N, std::max(1, std::min(kMaxImages, kTPB / items)));
    while (t.P > 1 && floats(t.P, t.TH, t.TW, t.cc) > kLdsFloats) --t.P;
  }
  t.LH = lh(t.TH);
  t.LW = lw(t.TW);
  t.xs_floats = round_up(t.P * t.cc * t.LH * t.LW, 4);
  t.nb = ceil_div(g.N, t.P);
  t.blocks = g.G * t.nb * t.ty * t.tx;
  t.fd_per = fastdiv_make((unsigned long)t.LH * t.LW);
  t.fd_lw = fastdiv_make(t.LW);
  t.fd_cc = fastdiv_make(t.cc);
  t.fd_ct = fastdiv_make((unsigned long)t.cc * taps);
  t.fd_taps = fastdiv_make(taps);
  t.fd_pcp = fastdiv_make(t.pcp);
  return t;
}

GcKind gc_kind(const GConv& g) {
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

// the block's group, first image and tile origin in the produced tensor
struct GcBlock {
  int grp, n0, r0, c0;
};
__device__ inline GcBlock gc_block(const GcTile& t) {
  const int tiles = t.ty * t.tx;
  const int gb = blockIdx.x / tiles;
  const int tl = blockIdx.x - gb * tiles;
  const int grp = gb / t.nb;
  const int tyi = tl / t.tx;
  return {grp, (gb - grp * t.nb) * t.P, tyi * t.TH, (tl - tyi * t.tx) * t.TW};
}

// the thread's item: image p of the block, first produced channel mb0, row
// r and run q of the tile
struct GcItem {
  int p, mb0, r, q;
};
__device__ inline GcItem gc_item(const GcTile& t) {
  const int RW = t.TW / kRun;
  int rest = threadIdx.x / RW;
  const int q = threadIdx.x - rest * RW;
  const int r = rest % t.TH;
  rest /= t.TH;
  const int mbi = rest % t.nmb;
  return {rest / t.nmb, mbi * t.mb, r, q};
}

// tile of `ccn` channels from ch0 of src[N][chans][H][W], rows from h0 and
// columns from w0, for the block's P images: xs[p][c][LH][LW], zero outside
__device__ inline void gc_stage_tile(float* xs, const GcTile& t,
                                     const float* __restrict__ src, int chans,
                                     int ch0, int ccn, int n0, int N, int h0,
                                     int w0, int H, int W) {
  const int per = t.LH * t.LW;
  for (int i = threadIdx.x; i < t.P * t.cc * per; i += kTPB) {
    const int pc = (int)fastdiv(i, t.fd_per);
    const int rem = i - pc * per;
    const int r = (int)fastdiv(rem, t.fd_lw);
    const int p = (int)fastdiv(pc, t.fd_cc), c = pc - p * t.cc;
    const int n = n0 + p, h = h0 + r, wc = w0 + (rem - r * t.LW);
    float v = 0.f;
    if (c < ccn && n < N && (unsigned)h < (unsigned)H &&
        (unsigned)wc < (unsigned)W)
      v = src[((n * chans + ch0 + c) * H + h) * W + wc];
    xs[i] = v;
  }
}

// MB weights of one (channel, tap), 16-byte aligned in LDS
template <int MB>
__device__ inline void gc_ld(float (&v)[MB], const float* p) {
#pragma unroll
  for (int m = 0; m < MB; m += 4) {
    const float4 a = *reinterpret_cast<const float4*>(p + m);
    v[m] = a.x, v[m + 1] = a.y, v[m + 2] = a.z, v[m + 3] = a.w;
  }
}

// a run of kRun pixels at element offset o of dst; n_ok of them inside the row
__device__ inline void gc_store_run(float* __restrict__ dst, int o,
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
template <int KIND, int MB>
__global__ __launch_bounds__(kTPB) void k_gconv_fwd(
    GConv g, GcTile t, const float* __restrict__ x,
    const float* __restrict__ w, const float* __restrict__ bias, int relu,
    float* __restrict__ y) {
  extern __shared__ float lds[];
  const int per = t.LH * t.LW;
  const int taps = g.kh * g.kw;
  float* xs = lds;                 // [P][cc][LH][LW]
  float* ws = lds + t.xs_floats;   // [cc][taps][pcp]
  const GcBlock b = gc_block(t);
  const GcItem it = gc_item(t);
  const int n = b.n0 + it.p, oh = b.r0 + it.r, ow = b.c0 + it.q * kRun;
  const bool active = it.p < t.P && n < g.N && oh < g.OH && ow < g.OW;
  const int C = g.G * g.cig, Cout = g.G * g.cog;
  const int h0 = b.r0 * g.sh - g.ph, w0 = b.c0 * g.sw - g.pw;
  float acc[MB][kRun];
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int i = 0; i < kRun; ++i) acc[m][i] = 0.f;

  for (int c0 = 0; c0 < g.cig; c0 += t.cc) {
    const int ccn = min(t.cc, g.cig - c0);
    if (c0) __syncthreads();
    gc_stage_tile(xs, t, x, C, b.grp * g.cig + c0, ccn, b.n0, g.N, h0, w0,
                  g.H, g.W);
    // W[co][c0 + ci][tap] read in stored order -> ws[ci][tap][co]
    const int ct = t.cc * taps;
    for (int i = threadIdx.x; i < t.pcp * ct; i += kTPB) {
      const int co = (int)fastdiv(i, t.fd_ct);
      const int e = i - co * ct;
      float v = 0.f;
      if (co < g.cog && e < ccn * taps)
        v = w[((b.grp * g.cog + co) * g.cig + c0) * taps + e];
      ws[e * t.pcp + co] = v;
    }
    __syncthreads();
    if (!active) continue;
    const float* xp =
        xs + it.p * t.cc * per + it.r * g.sh * t.LW + it.q * kRun * g.sw;
    const float* wp = ws + it.mb0;
    for (int ci = 0; ci < ccn; ++ci, xp += per, wp += taps * t.pcp) {
      if (KIND == kGeneric) {
        for (int ki = 0; ki < g.kh; ++ki)
          for (int kj = 0; kj < g.kw; ++kj) {
            const float* row = xp + ki * g.dh * t.LW + kj * g.dw;
            float xv[kRun], wv[MB];
#pragma unroll
            for (int i = 0; i < kRun; ++i) xv[i] = row[i * g.sw];
            gc_ld<MB>(wv, wp + (ki * g.kw + kj) * t.pcp);
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
              for (int i = 0; i < kRun; ++i) acc[m][i] += xv[i] * wv[m];
          }
      } else {
        constexpr int S = KIND == kK3S1 ? 1 : 2;
        constexpr int NV = (kRun - 1) * S + 3;  // row segment under the run
#pragma unroll
        for (int ki = 0; ki < 3; ++ki) {
          float v[NV];
#pragma unroll
          for (int c = 0; c < NV; ++c) v[c] = xp[ki * t.LW + c];
#pragma unroll
          for (int kj = 0; kj < 3; ++kj) {
            float wv[MB];
            gc_ld<MB>(wv, wp + (ki * 3 + kj) * t.pcp);
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
              for (int i = 0; i < kRun; ++i) acc[m][i] += v[i * S + kj] * wv[m];
          }
        }
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const int co = it.mb0 + m;
    if (co >= g.cog) break;
    const int cg = b.grp * g.cog + co;
    const float bv = bias ? bias[cg] : 0.f;
    float v[kRun];
#pragma unroll
    for (int i = 0; i < kRun; ++i) {
      v[i] = acc[m][i] + bv;
      if (relu) v[i] = v[i] > 0.f ? v[i] : 0.f;
    }
    gc_store_run(y, ((n * Cout + cg) * g.OH + oh) * g.OW + ow, v, g.OW - ow);
  }
}

// ------------------------------------------------------------------ dgrad
template <int KIND, int MB>
__global__ __launch_bounds__(kTPB) void k_gconv_bwd_data(
    GConv g, GcTile t, const float* __restrict__ dy,
    const float* __restrict__ w, float* __restrict__ dx) {
  extern __shared__ float lds[];
  const int per = t.LH * t.LW;
  const int taps = g.kh * g.kw;
  float* ds = lds;                 // [P][cc][LH][LW]
  float* ws = lds + t.xs_floats;   // [cc][taps][pcp]
  const GcBlock b = gc_block(t);
  const GcItem it = gc_item(t);
  const int n = b.n0 + it.p, h = b.r0 + it.r, wq = b.c0 + it.q * kRun;
  const bool active = it.p < t.P && n < g.N && h < g.H && wq < g.W;
  const int C = g.G * g.cig, Cout = g.G * g.cog;
  // first dy row / column any pixel of the tile can reach
  const int oh_lo = floor_div(b.r0 + g.ph - (g.kh - 1) * g.dh, g.sh);
  const int ow_lo = floor_div(b.c0 + g.pw - (g.kw - 1) * g.dw, g.sw);
  float acc[MB][kRun];
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int i = 0; i < kRun; ++i) acc[m][i] = 0.f;

  for (int c0 = 0; c0 < g.cog; c0 += t.cc) {
    const int ccn = min(t.cc, g.cog - c0);
    if (c0) __syncthreads();
    gc_stage_tile(ds, t, dy, Cout, b.grp * g.cog + c0, ccn, b.n0, g.N, oh_lo,
                  ow_lo, g.OH, g.OW);
    // W[c0 + co][ci][tap] -> ws[co][tap][ci]
    for (int i = threadIdx.x; i < t.cc * t.pcp * taps; i += kTPB) {
      const int pair = (int)fastdiv(i, t.fd_taps);
      const int tap = i - pair * taps;
      const int co = (int)fastdiv(pair, t.fd_pcp), ci = pair - co * t.pcp;
      float v = 0.f;
      if (co < ccn && ci < g.cig)
        v = w[((b.grp * g.cog + c0 + co) * g.cig + ci) * taps + tap];
      ws[(co * taps + tap) * t.pcp + ci] = v;
    }
    __syncthreads();
    if (!active) continue;
    const float* dp = ds + it.p * t.cc * per;
    const float* wp = ws + it.mb0;
    if (KIND == kK3S1) {
      // dy rows h+ph-ki, columns w+pw-kj: a 3 x (kRun+2) patch
      const int lc = wq + g.pw - 2 - ow_lo;
      for (int co = 0; co < ccn; ++co, dp += per, wp += 9 * t.pcp) {
#pragma unroll
        for (int ki = 0; ki < 3; ++ki) {
          const float* row = dp + (h + g.ph - ki - oh_lo) * t.LW + lc;
          float v[kRun + 2];
#pragma unroll
          for (int c = 0; c < kRun + 2; ++c) v[c] = row[c];
#pragma unroll
          for (int kj = 0; kj < 3; ++kj) {
            float wv[MB];
            gc_ld<MB>(wv, wp + (ki * 3 + kj) * t.pcp);
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
              for (int i = 0; i < kRun; ++i)
                acc[m][i] += v[i + 2 - kj] * wv[m];
          }
        }
      }
    } else if (KIND == kK3S2) {
      // parity picks the taps: a = h + ph even -> ki 0 (row a/2) and ki 2
      // (row a/2 - 1); odd -> ki 1 (row a/2) alone.  Likewise in w, where
      // wq is a multiple of kRun, so the parity of a pixel is the block's.
      const int a = h + g.ph;
      const bool odd_h = a & 1;
      const float* row0 = dp + ((a >> 1) - oh_lo) * t.LW - ow_lo;
      for (int co = 0; co < ccn; ++co, row0 += per, wp += 9 * t.pcp) {
        for (int j = 0; j < (odd_h ? 1 : 2); ++j) {
          const int ki = j ? 2 : (odd_h ? 1 : 0);
          const float* row = row0 - j * t.LW;
          const float* wk = wp + ki * 3 * t.pcp;
#pragma unroll
          for (int i = 0; i < kRun; ++i) {
            const int bb = wq + i + g.pw;
            const int c = bb >> 1;
            float wv[MB];
            if (bb & 1) {
              gc_ld<MB>(wv, wk + t.pcp);
              const float d = row[c];
#pragma unroll
              for (int m = 0; m < MB; ++m) acc[m][i] += d * wv[m];
            } else {
              float wv2[MB];
              gc_ld<MB>(wv, wk);
              gc_ld<MB>(wv2, wk + 2 * t.pcp);
              const float d0 = row[c], d1 = row[c - 1];
#pragma unroll
              for (int m = 0; m < MB; ++m)
                acc[m][i] += d0 * wv[m] + d1 * wv2[m];
            }
          }
        }
      }
    } else {
      // the taps that reach a pixel are found once, outside the channel loop
      for (int ki = 0; ki < g.kh; ++ki) {
        const int th = h + g.ph - ki * g.dh;
        const int oh = th / g.sh;
        if (oh * g.sh != th) continue;
        const float* rowb = dp + (oh - oh_lo) * t.LW;
        for (int kj = 0; kj < g.kw; ++kj) {
          int col[kRun];
          bool ok[kRun], any = false;
#pragma unroll
          for (int i = 0; i < kRun; ++i) {
            const int tw = wq + i + g.pw - kj * g.dw;
            const int ow = tw / g.sw;
            ok[i] = ow * g.sw == tw;
            col[i] = ok[i] ? ow - ow_lo : 0;
            any |= ok[i];
          }
          if (!any) continue;
          const float* wk = wp + (ki * g.kw + kj) * t.pcp;
          for (int co = 0; co < ccn; ++co) {
            const float* row = rowb + co * per;
            float wv[MB];
            gc_ld<MB>(wv, wk + co * taps * t.pcp);
#pragma unroll
            for (int i = 0; i < kRun; ++i) {
              const float d = ok[i] ? row[col[i]] : 0.f;
#pragma unroll
              for (int m = 0; m < MB; ++m) acc[m][i] += d * wv[m];
            }
          }
        }
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const int ci = it.mb0 + m;
    if (ci >= g.cig) break;
    gc_store_run(dx, ((n * C + b.grp * g.cig + ci) * g.H + h) * g.W + wq,
                 acc[m], g.W - wq);
  }
}

// ------------------------------------------------------------------ wgrad
// part[((grp * nb + slice) * cog + co) * E + e], E = cig * taps + 1: the
// group's dW row of co in stored order, then Σ dy at e = cig * taps
struct GcWg {
  int TR, bands;     // dy rows per staged band, bands per image
  int OWt, ctiles;   // dy columns per band (multiple of kRun), column tiles
  int XR, XW;        // x rows / columns under a band
  int dper, xper;    // LDS floats per dy / x channel: TR * OWt and XR * XW
                     // padded to an odd count of float4s / floats, so the
                     // channels a wave reads together fall in different banks
  int dy_floats;     // cog * dper
  int NP, CB;        // 3x3: output channels per thread, cb + k * CB, k < NP
  int npl, splits;   // owners per block, threads sharing one owner's runs
  int upass;         // generic: blocks per (group, slice), npl units each
  int nb;            // batch slices
  int lds_floats;
  bool fits;
  FastDiv fd_dyper, fd_owt, fd_xper, fd_xw, fd_rw;
};

GcWg gc_wg(const GConv& g, bool k3, bool want_bias) {
  GcWg t{};
  const int taps = g.kh * g.kw;
  const int OWp = round_up(g.OW, kRun);
  t.ctiles = ceil_div(OWp, 64);
  t.OWt = round_up(ceil_div(OWp, t.ctiles), kRun);
  auto xr = [&](int tr) { return (tr - 1) * g.sh + (g.kh - 1) * g.dh + 1; };
  auto xw = [&](int owt) { return (owt - 1) * g.sw + (g.kw - 1) * g.dw + 1; };
  auto dper = [&](int tr, int owt) { return (tr * owt / 4 | 1) * 4; };
  auto xper = [&](int tr, int owt) { return xr(tr) * xw(owt) | 1; };
  auto floats = [&](int tr, int owt) {
    return (long)g.cog * dper(tr, owt) + (long)g.cig * xper(tr, owt);
  };
  t.TR = g.OH;
  while (floats(t.TR, t.OWt) > kLdsFloats && t.TR > 1) --t.TR;
  while (floats(t.TR, t.OWt) > kLdsFloats && t.OWt > kRun)
    t.OWt = std::max(kRun, round_up(t.OWt / 2, kRun));
  t.fits = floats(t.TR, t.OWt) <= kLdsFloats;
  t.ctiles = ceil_div(OWp, t.OWt);
  t.bands = ceil_div(g.OH, t.TR);
  t.TR = ceil_div(g.OH, t.bands);
  t.XR = xr(t.TR);
  t.XW = xw(t.OWt);
  t.dper = dper(t.TR, t.OWt);
  t.xper = xper(t.TR, t.OWt);
  t.dy_floats = g.cog * t.dper;
  int nacc;  // accumulators a thread hands to the split sum
  if (k3) {
    t.NP = 1;
    while (g.cig * ceil_div(g.cog, t.NP) > kTPB) t.NP *= 2;  // 32 * 8 fits
    t.CB = ceil_div(g.cog, t.NP);
    t.npl = g.cig * t.CB;
    t.upass = 1;
    nacc = t.NP * 10;
  } else {
    const int units = g.cig * taps + (want_bias ? 1 : 0);
    t.upass = ceil_div(units, kTPB);
    t.npl = ceil_div(units, t.upass);
    nacc = 32;
  }
  t.splits = kTPB / t.npl;
  // batch slices: enough blocks to fill the device, at least 256 pixels of
  // every channel per slice
  const long S = (long)g.OH * g.OW;
  t.nb = (int)std::max<long>(
      1, std::min<long>({(long)g.N, 2048L / g.G, (g.N * S + 255) / 256}));
  t.lds_floats = std::max(t.dy_floats + g.cig * t.xper, nacc * kTPB);
  t.fd_dyper = fastdiv_make((unsigned long)t.TR * t.OWt);
  t.fd_owt = fastdiv_make(t.OWt);
  t.fd_xper = fastdiv_make((unsigned long)t.XR * t.XW);
  t.fd_xw = fastdiv_make(t.XW);
  t.fd_rw = fastdiv_make(t.OWt / kRun);
  return t;
}

// image n, band from dy row oh0, columns from ow0: dys[co][dper] holding
// [TR][OWt] and xs[ci][xper] holding [XR][XW], zero outside the tensors
__device__ inline void gc_wg_stage(const GConv& g, const GcWg& t, int grp,
                                   int n, int oh0, int ow0,
                                   const float* __restrict__ x,
                                   const float* __restrict__ dy, float* dys,
                                   float* xs) {
  const int dper = t.TR * t.OWt, xper = t.XR * t.XW;
  for (int i = threadIdx.x; i < g.cog * dper; i += kTPB) {
    const int co = (int)fastdiv(i, t.fd_dyper);
    const int rem = i - co * dper;
    const int r = (int)fastdiv(rem, t.fd_owt);
    const int oh = oh0 + r, ow = ow0 + (rem - r * t.OWt);
    float v = 0.f;
    if (oh < g.OH && ow < g.OW)
      v = dy[((n * g.G * g.cog + grp * g.cog + co) * g.OH + oh) * g.OW + ow];
    dys[co * t.dper + rem] = v;
  }
  const int h0 = oh0 * g.sh - g.ph, w0 = ow0 * g.sw - g.pw;
  for (int i = threadIdx.x; i < g.cig * xper; i += kTPB) {
    const int ci = (int)fastdiv(i, t.fd_xper);
    const int rem = i - ci * xper;
    const int r = (int)fastdiv(rem, t.fd_xw);
    const int h = h0 + r, wc = w0 + (rem - r * t.XW);
    float v = 0.f;
    if ((unsigned)h < (unsigned)g.H && (unsigned)wc < (unsigned)g.W)
      v = x[((n * g.G * g.cig + grp * g.cig + ci) * g.H + h) * g.W + wc];
    xs[ci * t.xper + rem] = v;
  }
}

// the threads of one owner (pl, splits sp = 0..) hold partial sums of the
// same outputs: add them into sp 0 in fixed order through LDS
template <int NA>
__device__ inline void gc_split_sum(float (&v)[NA], float* red, int pl,
                                    int sp, const GcWg& t) {
  if (t.splits == 1) return;
  __syncthreads();  // the last tile has been consumed
#pragma unroll
  for (int a = 0; a < NA; ++a) red[a * kTPB + threadIdx.x] = v[a];
  __syncthreads();
  if (sp != 0) return;
  for (int s = 1; s < t.splits; ++s)
#pragma unroll
    for (int a = 0; a < NA; ++a) v[a] += red[a * kTPB + s * t.npl + pl];
}

// 3x3 at stride S, no dilation
template <int S, int NP>
__global__ __launch_bounds__(kTPB) void k_gconv_wgrad_part(
    GConv g, GcWg t, const float* __restrict__ x,
    const float* __restrict__ dy, double* __restrict__ part) {
  extern __shared__ float lds[];
  float* dys = lds;
  float* xs = lds + t.dy_floats;
  const int grp = blockIdx.x / t.nb, slice = blockIdx.x - grp * t.nb;
  const int n0 = (int)((long)g.N * slice / t.nb);
  const int n1 = (int)((long)g.N * (slice + 1) / t.nb);
  const int sp = threadIdx.x / t.npl, pl = threadIdx.x - sp * t.npl;
  const bool live = sp < t.splits;
  const int cb = pl / g.cig, ci = pl - cb * g.cig;
  const int RW = t.OWt / kRun, units = t.TR * RW;
  constexpr int NV = (kRun - 1) * S + 3;
  float acc[NP * 10];  // [k][9 taps, Σ dy]
#pragma unroll
  for (int a = 0; a < NP * 10; ++a) acc[a] = 0.f;

  for (int n = n0; n < n1; ++n)
    for (int band = 0; band < t.bands; ++band)
      for (int ct = 0; ct < t.ctiles; ++ct) {
        __syncthreads();
        gc_wg_stage(g, t, grp, n, band * t.TR, ct * t.OWt, x, dy, dys, xs);
        __syncthreads();
        if (!live) continue;
        for (int u = sp; u < units; u += t.splits) {
          const int r = (int)fastdiv(u, t.fd_rw), q = u - r * RW;
          float d[NP][kRun];
#pragma unroll
          for (int k = 0; k < NP; ++k) {
            const int co = cb + k * t.CB;
            float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (co < g.cog)
              v4 = *reinterpret_cast<const float4*>(
                  dys + co * t.dper + r * t.OWt + q * kRun);
            d[k][0] = v4.x, d[k][1] = v4.y, d[k][2] = v4.z, d[k][3] = v4.w;
            acc[k * 10 + 9] += (v4.x + v4.y) + (v4.z + v4.w);
          }
          const float* xp = xs + ci * t.xper + r * S * t.XW + q * kRun * S;
#pragma unroll
          for (int ki = 0; ki < 3; ++ki) {
            float v[NV];
#pragma unroll
            for (int c = 0; c < NV; ++c) v[c] = xp[ki * t.XW + c];
#pragma unroll
            for (int k = 0; k < NP; ++k)
#pragma unroll
              for (int kj = 0; kj < 3; ++kj)
#pragma unroll
                for (int i = 0; i < kRun; ++i)
                  acc[k * 10 + ki * 3 + kj] += d[k][i] * v[i * S + kj];
          }
        }
      }
  gc_split_sum<NP * 10>(acc, lds, pl, sp, t);
  if (sp != 0) return;
  const int E = g.cig * 9 + 1;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int co = cb + k * t.CB;
    if (co >= g.cog) break;
    double* out = part + ((long)(grp * t.nb + slice) * g.cog + co) * E;
#pragma unroll
    for (int e = 0; e < 9; ++e) out[ci * 9 + e] = (double)acc[k * 10 + e];
    if (ci == 0) out[E - 1] = (double)acc[k * 10 + 9];
  }
}

// any geometry: unit = (ci, tap), or the bias unit (x == 1) after the last.
// CO bounds the register array: cog rounded up to 4, 8, 16 or 32.
template <int CO>
__global__ __launch_bounds__(kTPB) void k_gconv_wgrad_part_generic(
    GConv g, GcWg t, const float* __restrict__ x,
    const float* __restrict__ dy, int want_bias, double* __restrict__ part) {
  extern __shared__ float lds[];
  float* dys = lds;
  float* xs = lds + t.dy_floats;
  const int taps = g.kh * g.kw;
  const int gs = blockIdx.x / t.upass, up = blockIdx.x - gs * t.upass;
  const int grp = gs / t.nb, slice = gs - grp * t.nb;
  const int n0 = (int)((long)g.N * slice / t.nb);
  const int n1 = (int)((long)g.N * (slice + 1) / t.nb);
  const int sp = threadIdx.x / t.npl, pl = threadIdx.x - sp * t.npl;
  const int unit = up * t.npl + pl;
  const int nunits = g.cig * taps + (want_bias ? 1 : 0);
  const bool live = sp < t.splits && unit < nunits;
  const bool is_bias = unit == g.cig * taps;
  const int ci = is_bias ? 0 : unit / taps, tap = unit - ci * taps;
  const int ki = is_bias ? 0 : tap / g.kw, kj = is_bias ? 0 : tap - ki * g.kw;
  const int RW = t.OWt / kRun, nruns = t.TR * RW;
  float acc[CO];
#pragma unroll
  for (int a = 0; a < CO; ++a) acc[a] = 0.f;

  for (int n = n0; n < n1; ++n)
    for (int band = 0; band < t.bands; ++band)
      for (int ct = 0; ct < t.ctiles; ++ct) {
        __syncthreads();
        gc_wg_stage(g, t, grp, n, band * t.TR, ct * t.OWt, x, dy, dys, xs);
        __syncthreads();
        if (!live) continue;
        const float* xb =
            xs + ci * t.xper + ki * g.dh * t.XW + kj * g.dw;
        for (int u = sp; u < nruns; u += t.splits) {
          const int r = (int)fastdiv(u, t.fd_rw), q = u - r * RW;
          const float* xp = xb + r * g.sh * t.XW + q * kRun * g.sw;
          float xv[kRun];
#pragma unroll
          for (int i = 0; i < kRun; ++i) xv[i] = is_bias ? 1.f : xp[i * g.sw];
          const float* dp = dys + r * t.OWt + q * kRun;
#pragma unroll
          for (int co = 0; co < CO; ++co) {
            if (co >= g.cog) break;
            const float4 d = *reinterpret_cast<const float4*>(
                dp + co * t.dper);
            acc[co] += (d.x * xv[0] + d.y * xv[1]) + (d.z * xv[2] + d.w * xv[3]);
          }
        }
      }
  gc_split_sum<CO>(acc, lds, pl, sp, t);
  if (sp != 0 || unit >= nunits) return;
  const int E = g.cig * taps + 1;
#pragma unroll
  for (int co = 0; co < CO; ++co) {
    if (co >= g.cog) break;
    part[((long)(grp * t.nb + slice) * g.cog + co) * E + unit] =
        (double)acc[co];
  }
}

__global__ void k_gconv_wgrad_fin(const double* __restrict__ part, int nb,
                                  int G, int cog, int E, int want_bias,
                                  float* __restrict__ dw,
                                  float* __restrict__ db) {
  const int total = G * cog * E;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    const int cg = i / E, e = i - cg * E;
    if (e == E - 1 && !want_bias) continue;
    const int grp = cg / cog, co = cg - grp * cog;
    double acc = 0;
    for (int s = 0; s < nb; ++s)
      acc += part[((long)(grp * nb + s) * cog + co) * E + e];
    if (e == E - 1)
      db[cg] = (float)acc;
    else
      dw[cg * (E - 1) + e] = (float)acc;
  }
}

// the kernels index in 32 bits
bool gc_counts_fit(const GConv& g) {
  const long lim = 1L << 31;
  return (long)g.N * g.G * g.cig * g.H * g.W < lim &&
         (long)g.N * g.G * g.cog * g.OH * g.OW < lim;
}

bool gc_wg_k3(const GConv& g) { return gc_kind(g) != kGeneric; }

int gc_var(GcKind k, const GcTile& t) {
  return (int)k * 2 + (t.ty * t.tx == 1 ? 0 : 1);
}

size_t gc_lds_bytes(const GConv& g, const GcTile& t) {
  return sizeof(float) *
         ((size_t)t.xs_floats + (size_t)t.cc * g.kh * g.kw * t.pcp);
}

double gc_flops(const GConv& g) {
  return 2.0 * g.N * g.G * g.cog * g.OH * g.OW * g.cig * g.kh * g.kw;
}

}  // namespace

bool gconv_supported(const GConv& g) {
  return gc_counts_fit(g) && gc_tile(g, false).fits && gc_tile(g, true).fits &&
         gc_wg(g, gc_wg_k3(g), true).fits;
}

#define GC_LAUNCH_KIND(KERNEL, MB, ...)                                      \
  do {                                                                       \
    if (k == kK3S1)                                                          \
      hipLaunchKernelGGL((KERNEL<kK3S1, MB>), grid, block, lds, s,           \
                         __VA_ARGS__);                                       \
    else if (k == kK3S2)                                                     \
      hipLaunchKernelGGL((KERNEL<kK3S2, MB>), grid, block, lds, s,           \
                         __VA_ARGS__);                                       \
    else                                                                     \
      hipLaunchKernelGGL((KERNEL<kGeneric, MB>), grid, block, lds, s,        \
                         __VA_ARGS__);                                       \
  } while (0)

void gconv_fwd(hipStream_t s, const GConv& g, const float* x, const float* w,
               const float* bias, bool relu, float* y) {
  CHECK_(gc_counts_fit(g)) << "grouped conv: tensor of 2^31 elements or more";
  const double nx = (double)g.N * g.G * g.cig * g.H * g.W;
  const double ny = (double)g.N * g.G * g.cog * g.OH * g.OW;
  const double nw = (double)g.G * g.cog * g.cig * g.kh * g.kw;
  PerfScope perf(PERF_CLASS("gconv_fwd"), s, gc_flops(g),
                 4.0 * (nx + ny + nw));
  const GcTile t = gc_tile(g, false);
  CHECK_(t.fits) << "grouped conv: window does not fit the LDS tile";
  const GcKind k = gc_kind(g);
  const size_t lds = gc_lds_bytes(g, t);
  const dim3 grid(t.blocks), block(kTPB);
  if (t.mb == 8)
    GC_LAUNCH_KIND(k_gconv_fwd, 8, g, t, x, w, bias, (int)relu, y);
  else
    GC_LAUNCH_KIND(k_gconv_fwd, 4, g, t, x, w, bias, (int)relu, y);
  const long rec[8] = {g.cig, g.cog, t.chunks, t.P, t.ty, t.tx, 0, t.blocks};
  kernel_trace_gconv(0, gc_var(k, t), rec);
}

void gconv_bwd_data(hipStream_t s, const GConv& g, const float* dy,
                    const float* w, float* dx) {
  CHECK_(gc_counts_fit(g)) << "grouped conv: tensor of 2^31 elements or more";
  const double nx = (double)g.N * g.G * g.cig * g.H * g.W;
  const double ny = (double)g.N * g.G * g.cog * g.OH * g.OW;
  const double nw = (double)g.G * g.cog * g.cig * g.kh * g.kw;
  PerfScope perf(PERF_CLASS("gconv_bwd_data"), s, gc_flops(g),
                 4.0 * (nx + ny + nw));
  const GcTile t = gc_tile(g, true);
  CHECK_(t.fits) << "grouped conv: window does not fit the LDS tile";
  const GcKind k = gc_kind(g);
  const size_t lds = gc_lds_bytes(g, t);
  const dim3 grid(t.blocks), block(kTPB);
  if (t.mb == 8)
    GC_LAUNCH_KIND(k_gconv_bwd_data, 8, g, t, dy, w, dx);
  else
    GC_LAUNCH_KIND(k_gconv_bwd_data, 4, g, t, dy, w, dx);
  const long rec[8] = {g.cig, g.cog, t.chunks, t.P, t.ty, t.tx, 0, t.blocks};
  kernel_trace_gconv(1, gc_var(k, t), rec);
}
#undef GC_LAUNCH_KIND

void gconv_bwd_weight(hipStream_t s, const GConv& g, const float* x,
                      const float* dy, float* dw, float* db) {
  CHECK_(gc_counts_fit(g)) << "grouped conv: tensor of 2^31 elements or more";
  const double nx = (double)g.N * g.G * g.cig * g.H * g.W;
  const double ny = (double)g.N * g.G * g.cog * g.OH * g.OW;
  const double nw = (double)g.G * g.cog * g.cig * g.kh * g.kw;
  PerfScope perf(PERF_CLASS("gconv_bwd_weight"), s, gc_flops(g),
                 4.0 * (nx + ny + nw));
  const GcKind k = gc_kind(g);
  const int want_bias = db != nullptr;
  const GcWg t = gc_wg(g, k != kGeneric, want_bias);
  CHECK_(t.fits) << "grouped conv: window does not fit the LDS tile";
  const int E = g.cig * g.kh * g.kw + 1;
  double* part = (double*)Workspace::get_global().get(
      Workspace::kGcPart, sizeof(double) * (size_t)g.G * t.nb * g.cog * E);
  const size_t lds = sizeof(float) * (size_t)t.lds_floats;
  const dim3 grid(g.G * t.nb * t.upass), block(kTPB);
#define GC_WG(S, NP)                                                       \
  hipLaunchKernelGGL((k_gconv_wgrad_part<S, NP>), grid, block, lds, s, g, \
                     t, x, dy, part)
#define GC_WG_GEN(CO)                                                      \
  hipLaunchKernelGGL((k_gconv_wgrad_part_generic<CO>), grid, block, lds,  \
                     s, g, t, x, dy, want_bias, part)
  if (k == kK3S1) {
    if (t.NP == 1) GC_WG(1, 1);
    else if (t.NP == 2) GC_WG(1, 2);
    else GC_WG(1, 4);
  } else if (k == kK3S2) {
    if (t.NP == 1) GC_WG(2, 1);
    else if (t.NP == 2) GC_WG(2, 2);
    else GC_WG(2, 4);
  } else {
    if (g.cog <= 4) GC_WG_GEN(4);
    else if (g.cog <= 8) GC_WG_GEN(8);
    else if (g.cog <= 16) GC_WG_GEN(16);
    else GC_WG_GEN(32);
  }
#undef GC_WG
#undef GC_WG_GEN
  const int total = g.G * g.cog * E;
  hipLaunchKernelGGL(k_gconv_wgrad_fin,
                     dim3(std::min((total + kTPB - 1) / kTPB, 2048)),
                     dim3(kTPB), 0, s, part, t.nb, g.G, g.cog, E, want_bias,
                     dw, db);
  const long rec[8] = {g.cig,    g.cog, t.bands * t.ctiles,
                       t.NP,     t.nb,  want_bias,
                       t.splits, (long)grid.x};
  kernel_trace_gconv(2, (int)k, rec);
}

}  // namespace gpu
}  // namespace camd
