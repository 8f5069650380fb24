// deconv.hip — forward of the Deconvolution layer (transposed convolution)
// at stride > 1, dilation 1, for gfx950, and backward for few channels per
// group (second half of the file): the output is split by stride phase
// and each phase is a dense stride-1 correlation, so no dcol matrix is ever
// written and no tap multiplies an inserted zero.
//
// Geometry.  Output row oh = sh*q + r: cell q, phase r in [0, sh).  The taps
// that reach it are ki = rk + sh*t with rk = (r + ph) % sh, t < T(r) =
// ceil((kh - rk) / sh), and tap t reads input row q + dq - t with dq =
// (r + ph) / sh.  Columns likewise.  Cells are counted from the OUTPUT origin
// (not from oh + ph, as the phase split is usually written): a 64-row output
// at stride 2 is then exactly 32 cell rows whatever the pad, where the padded
// origin gives 33 and a ragged tile on every edge.  The price is that dq
// differs by at most one between phases, so the LDS window has one more halo
// row / column; every phase of a cell tile still reads that one window.  A
// phase with rk >= kh has no tap at all (stride larger than the kernel) and
// receives the bias only.
//
// k_deconv_pack_w re-lays the weights W[G*cig][cog][kh][kw] once per forward
// as Wp[g][phase][tap slot (t, u)][ci][co]: co innermost and padded to the
// channel tile, ci padded to the MFMA k-step, taps a phase does not have
// zero.  K is ordered (tap, ci), not (ci, tap): the two k of one 32x32x2
// MFMA step are then two input channels of the SAME tap, so a lane's B
// address is base + channel * plane — no index table and no division in the
// K-loop — and a wave's A read is two runs of 32 consecutive floats.
//
// mfma variant: a block of 4 waves owns (image, group, tile of 32 or 64
// output channels, 8 x 16 cells).  It loops over chunks of <= 32 input
// channels; a chunk's window (8 + halo) x (16 + halo) per channel is staged
// once into LDS, zero outside the image, and serves every tap of every
// phase.  Wave w owns cell rows 2w, 2w + 1 as the 32 columns of
// __builtin_amdgcn_mfma_f32_32x32x2f32; A comes straight from Wp (the four
// waves read the same lines, which stay in L1/L2 — at 64 channels x 16 taps
// a chunk's slab would not fit LDS beside the window).  Accumulators of up
// to four phases are live at once (4 x 2 x 16 registers); with more phases
// an outer loop takes them four at a time over the resident window, which
// is re-staged per pass only when there are several channel chunks.
//
// direct variant (few output channels per group: bilinear upsampling with
// group == channels, a generator's last layer): window and the group's
// packed weights in LDS, all input channels at once; for each row phase a
// thread owns output pixels that are ADJACENT along the row (lane -> ow), so
// a wave stores whole row segments, and CB <= 4 output channels each.
//
// Both add the bias in the epilogue and write every output element exactly
// once: no atomics, no zero fill, fixed summation order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../layers.hpp"

namespace camd {
namespace gpu {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kTPB = 256;
constexpr int kLdsFloats = 16384;  // 64 KB per block: two blocks per CU
constexpr int kTQH = 8, kTQW = 16; // cell tile: 32 cells per wave
constexpr int kMaxCc = 32;         // input channels per LDS chunk (even)
// cog at or below which the direct variant is taken: an MFMA tile would use
// at most 4 of its 32 rows.  A policy constant, NOT measured.
constexpr int kDirectMaxCog = 4;
// The direct variant reads one LDS weight per FMA and lost to the GEMM route
// at cig = 64 (profiles/deconv.txt); it won at cig = 1.  Between the two the
// bound is a policy constant, NOT measured.  A layer with cog <= 4 and more
// input channels than this is not supported and keeps the GEMM route.
constexpr int kDirectMaxCig = 4;
constexpr int kUnroll = 8;         // MFMA k-steps loaded ahead

enum { kVarMfma = 0, kVarDirect = 1 };

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return ceil_div(a, b) * b; }

struct DcPlan {
  int var;
  int P, tmh, tmw, slots;  // phases; most taps of a phase per axis; tmh * tmw
  int dqh, dqw;            // smallest dq per axis
  int TQH, ty, tx;         // cell rows per tile (columns: kTQW), tiles
  int LH, LW, per;         // LDS window per channel; plane stride (odd)
  int cc, chunks, cigp;    // channels per chunk, chunks, padded cig
  int mt, cop, cot;        // output channels per block, padded cog, tiles
  int win_floats;          // cc * per, rounded up to a float4
  int wl_floats;           // direct: the group's weights for one channel tile
  long pstride;            // Wp floats per (group, phase): slots * cigp * cop
  int blocks;
  bool fits;
  FastDiv fd_hw, fd_lw, fd_row, fd_sw;
};

DcPlan dc_plan(const Deconv& g) {
  DcPlan t{};
  t.P = g.sh * g.sw;
  t.tmh = ceil_div(g.kh, g.sh);
  t.tmw = ceil_div(g.kw, g.sw);
  t.slots = t.tmh * t.tmw;
  t.dqh = g.ph / g.sh;
  t.dqw = g.pw / g.sw;
  const int ddh = (g.sh - 1 + g.ph) / g.sh - t.dqh;
  const int ddw = (g.sw - 1 + g.pw) / g.sw - t.dqw;
  const int QH = ceil_div(g.OH, g.sh), QW = ceil_div(g.OW, g.sw);
  t.LW = kTQW + t.tmw - 1 + ddw;
  t.tx = ceil_div(QW, kTQW);
  auto per = [&](int tqh) { return ((tqh + t.tmh - 1 + ddh) * t.LW) | 1; };
  t.var = kVarMfma;
  if (g.cog <= kDirectMaxCog) {
    // one chunk: every input channel's window and the weights beside it
    t.mt = g.cog == 1 ? 1 : g.cog == 2 ? 2 : 4;
    t.cop = round_up(g.cog, t.mt);
    t.wl_floats = t.P * t.slots * g.cig * t.mt;
    t.TQH = kTQH;
    auto floats = [&](int tqh) {
      return (long)round_up(g.cig * per(tqh), 4) + t.wl_floats;
    };
    while (floats(t.TQH) > kLdsFloats && t.TQH > 1) t.TQH /= 2;
    t.var = kVarDirect;
    t.cigp = t.cc = g.cig;
    t.chunks = 1;
    t.fits = g.cig <= kDirectMaxCig && floats(t.TQH) <= kLdsFloats;
  }
  if (t.var == kVarMfma) {
    t.mt = g.cog > 32 ? 64 : 32;
    t.cop = round_up(g.cog, t.mt);
    t.wl_floats = 0;
    t.TQH = kTQH;
    t.cigp = round_up(g.cig, 2);
    t.cc = std::min(kMaxCc, t.cigp);
    while ((long)t.cc * per(kTQH) > kLdsFloats && t.cc > 2)
      t.cc = round_up(t.cc / 2, 2);
    t.fits = (long)t.cc * per(kTQH) <= kLdsFloats;
    t.chunks = ceil_div(g.cig, t.cc);
  }
  t.cot = t.cop / t.mt;
  t.LH = t.TQH + t.tmh - 1 + ddh;
  t.per = per(t.TQH);
  t.win_floats = round_up(t.cc * t.per, 4);
  t.ty = ceil_div(QH, t.TQH);
  t.pstride = (long)t.slots * t.cigp * t.cop;
  t.blocks = g.N * g.G * t.cot * t.ty * t.tx;
  t.fd_hw = fastdiv_make((unsigned long)t.LH * t.LW);
  t.fd_lw = fastdiv_make(t.LW);
  t.fd_row = fastdiv_make((unsigned long)kTQW * g.sw);
  t.fd_sw = fastdiv_make(g.sw);
  return t;
}

// the kernels index in 32 bits
bool dc_counts_fit(const Deconv& g, const DcPlan& t) {
  const long lim = 1L << 31;
  return (long)g.N * g.G * g.cig * g.H * g.W < lim &&
         (long)g.N * g.G * g.cog * g.OH * g.OW < lim &&
         (long)g.G * t.P * t.pstride < lim / 2 &&
         (long)g.N * g.G * t.cot * t.ty * t.tx < lim;
}

// one axis of a phase: residue r of the output index mod the stride
struct DcPhase {
  int rk;   // first tap, (r + pad) % stride; tap t is rk + stride * t
  int off;  // window row / column of tap 0 under the tile's first cell
  int T;    // taps
};
__host__ __device__ inline DcPhase dc_phase(int r, int pad, int s, int k,
                                            int tmax, int dqmin) {
  const int a = r + pad, dq = a / s, rk = a - dq * s;
  return {rk, dq - dqmin + tmax - 1, rk < k ? (k - rk + s - 1) / s : 0};
}

// W[g * cig + ci][co][ki][kj] at tap `slot` of phase p; zero for a tap the
// phase does not have and for pad channels
__device__ inline float dc_pack_value(const Deconv& g, int tmh, int tmw,
                                      int dqh, int dqw,
                                      const float* __restrict__ w, int grp,
                                      int p, int slot, int ci, int co) {
  const int tt = slot / tmw, u = slot - tt * tmw;
  const int r = p / g.sw, s = p - r * g.sw;
  const DcPhase fh = dc_phase(r, g.ph, g.sh, g.kh, tmh, dqh);
  const DcPhase fw = dc_phase(s, g.pw, g.sw, g.kw, tmw, dqw);
  if (tt >= fh.T || u >= fw.T || ci >= g.cig || co >= g.cog) return 0.f;
  return w[(((grp * g.cig + ci) * g.cog + co) * g.kh + fh.rk + g.sh * tt) *
               g.kw +
           fw.rk + g.sw * u];
}

// Wp[g][p][slot][ci][co] from W[g * cig + ci][co][kh][kw]; pads are zero
__global__ void k_deconv_pack_w(Deconv g, DcPlan t,
                                const float* __restrict__ w,
                                float* __restrict__ wp) {
  const int total = (int)(g.G * t.P * t.pstride);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    int e = i / t.cop;
    const int co = i - e * t.cop;
    const int ci = e % t.cigp;
    e /= t.cigp;
    const int slot = e % t.slots;
    e /= t.slots;
    wp[i] = dc_pack_value(g, t.tmh, t.tmw, t.dqh, t.dqw, w, e / t.P, e % t.P,
                          slot, ci, co);
  }
}

// the block's image, group, channel tile and first cell
struct DcBlock {
  int n, grp, ct, q0h, q0w;
};
template <class Plan>  // DcPlan, or backward's DbPlan (cells of the input)
__device__ inline DcBlock dc_block(const Deconv& g, const Plan& t) {
  int b = blockIdx.x;
  const int txi = b % t.tx;
  b /= t.tx;
  const int tyi = b % t.ty;
  b /= t.ty;
  const int ct = b % t.cot;
  b /= t.cot;
  return {b / g.G, b % g.G, ct, tyi * t.TQH, txi * kTQW};
}

// window of `ccn` channels from ch0 of image n of x[N][chans][H][W], rows
// from h0 and columns from w0: win[c][per] holding [LH][LW], zero outside
// the image and for the chunk's channels past ccn
__device__ inline void dc_stage(float* win, const DcPlan& t,
                                const float* __restrict__ x, int chans,
                                int ch0, int ccn, int n, int h0, int w0,
                                int H, int W) {
  const int hw = t.LH * t.LW;
  for (int i = threadIdx.x; i < t.cc * hw; i += kTPB) {
    const int c = (int)fastdiv(i, t.fd_hw);
    const int rem = i - c * hw;
    const int r = (int)fastdiv(rem, t.fd_lw);
    const int h = h0 + r, wc = w0 + (rem - r * t.LW);
    float v = 0.f;
    if (c < ccn && (unsigned)h < (unsigned)H && (unsigned)wc < (unsigned)W)
      v = x[((n * chans + ch0 + c) * H + h) * W + wc];
    win[c * t.per + rem] = v;
  }
}

// ------------------------------------------------------------------- mfma
// MR: 32-row blocks of output channels per wave; NPH: phases per pass
template <int MR, int NPH>
__global__ __launch_bounds__(kTPB, 2) void k_deconv_mfma(
    Deconv g, DcPlan t, const float* __restrict__ x,
    const float* __restrict__ wp, const float* __restrict__ bias,
    float* __restrict__ y) {
  extern __shared__ float win[];  // [cc][per]
  const DcBlock b = dc_block(g, t);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, ksel = lane >> 5;   // MFMA column, k of the pair
  const int a = wave * 2 + (col >> 4), bq = col & 15;  // the lane's cell
  const int C = g.G * g.cig, Cout = g.G * g.cog;
  const int h0 = b.q0h + t.dqh - (t.tmh - 1);
  const int w0 = b.q0w + t.dqw - (t.tmw - 1);
  const float* wg = wp + (long)b.grp * t.P * t.pstride + b.ct * (MR * 32) + col;
  const long tap_stride = (long)t.cigp * t.cop;

  for (int pg = 0; pg < t.P; pg += NPH) {
    f32x16 acc[NPH][MR];
#pragma unroll
    for (int j = 0; j < NPH; ++j)
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][m][e] = 0.f;

    for (int ch = 0; ch < t.chunks; ++ch) {
      const int c0 = ch * t.cc, ccn = min(t.cc, g.cig - c0);
      if (pg == 0 || t.chunks > 1) {  // one chunk: the window stays resident
        __syncthreads();
        dc_stage(win, t, x, C, b.grp * g.cig + c0, ccn, b.n, h0, w0, g.H,
                 g.W);
        __syncthreads();
      }
      const int npair = (ccn + 1) >> 1;
#pragma unroll
      for (int j = 0; j < NPH; ++j) {
        const int p = pg + j;
        if (p < t.P) {
          const int r = p / g.sw, s = p - r * g.sw;
          const DcPhase fh = dc_phase(r, g.ph, g.sh, g.kh, t.tmh, t.dqh);
          const DcPhase fw = dc_phase(s, g.pw, g.sw, g.kw, t.tmw, t.dqw);
          const float* Ap = wg + p * t.pstride + (long)(c0 + ksel) * t.cop;
          const float* Bp =
              win + ksel * t.per + (a + fh.off) * t.LW + bq + fw.off;
          for (int tt = 0; tt < fh.T; ++tt)
            for (int u = 0; u < fw.T; ++u) {
              const float* Aq = Ap + (tt * t.tmw + u) * tap_stride;
              const float* Bq = Bp - tt * t.LW - u;
              // kUnroll k-steps of loads in flight ahead of their MFMAs (one
              // A load per MFMA comes from L2: issued one at a time, the
              // matrix pipe idled 70% of the time); a step past the chunk
              // re-reads the last one and is not multiplied
              for (int jj = 0; jj < npair; jj += kUnroll) {
                float bv[kUnroll], av[kUnroll][MR];
#pragma unroll
                for (int q = 0; q < kUnroll; ++q) {
                  const int k2 = 2 * min(jj + q, npair - 1);
                  bv[q] = Bq[k2 * t.per];
#pragma unroll
                  for (int m = 0; m < MR; ++m)
                    av[q][m] = Aq[k2 * t.cop + m * 32];
                }
#pragma unroll
                for (int q = 0; q < kUnroll; ++q)
                  if (jj + q < npair) {
#pragma unroll
                    for (int m = 0; m < MR; ++m)
                      acc[j][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                          av[q][m], bv[q], acc[j][m], 0, 0, 0);
                  }
              }
            }
        }
      }
    }

    // C/D map: column = lane & 31, register e holds row (e & 3) + 8 * (e >> 2)
    // + 4 * ksel.  At stride 2 along W the two column phases of a cell sit
    // side by side in y and go out as one 8-byte store where that is aligned.
    const int qh = b.q0h + a, qw = b.q0w + bq;
#pragma unroll
    for (int j = 0; j < NPH; ++j) {
      const int p = pg + j;
      if (p >= t.P) continue;
      const int r = p / g.sw, s = p - r * g.sw;
      const int oh = qh * g.sh + r, ow = qw * g.sw + s;
      if (oh >= g.OH || ow >= g.OW) continue;
      // an odd column phase in range was written with its left neighbour
      if (NPH > 1 && g.sw == 2 && (j & 1)) continue;
      const bool pair = NPH > 1 && g.sw == 2 && ow + 1 < g.OW;
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int co =
              b.ct * (MR * 32) + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * ksel;
          if (co >= g.cog) continue;
          const int cg = b.grp * g.cog + co;
          const float bv = bias ? bias[cg] : 0.f;
          const int o = ((b.n * Cout + cg) * g.OH + oh) * g.OW + ow;
          const float v0 = acc[j][m][e] + bv;
          if (pair) {
            const float v1 = acc[(j | 1) < NPH ? (j | 1) : j][m][e] + bv;
            if ((o & 1) == 0) {
              *reinterpret_cast<float2*>(y + o) = make_float2(v0, v1);
            } else {
              y[o] = v0;
              y[o + 1] = v1;
            }
          } else {
            y[o] = v0;
          }
        }
    }
  }
}

// ----------------------------------------------------------------- direct
// CB: output channels per thread (the block's channel tile)
template <int CB>
__global__ __launch_bounds__(kTPB) void k_deconv_direct(
    Deconv g, DcPlan t, const float* __restrict__ x,
    const float* __restrict__ wp, const float* __restrict__ bias,
    float* __restrict__ y) {
  extern __shared__ float lds[];
  float* win = lds;                  // [cig][per]
  float* wl = lds + t.win_floats;    // [P][slot][ci][CB]
  const DcBlock b = dc_block(g, t);
  const int C = g.G * g.cig, Cout = g.G * g.cog;
  dc_stage(win, t, x, C, b.grp * g.cig, g.cig, b.n,
           b.q0h + t.dqh - (t.tmh - 1), b.q0w + t.dqw - (t.tmw - 1), g.H,
           g.W);
  // Wp rows (p, slot, ci) are cop long and follow one another (cigp == cig)
  const float* wg = wp + (long)b.grp * t.P * t.pstride + b.ct * CB;
  for (int i = threadIdx.x; i < t.wl_floats; i += kTPB) {
    const int e = i / CB;
    wl[i] = wg[(long)e * t.cop + (i - e * CB)];
  }
  __syncthreads();

  const int per_p = t.slots * g.cig * CB;
  const int rowitems = kTQW * g.sw, items = t.TQH * rowitems;
  for (int r = 0; r < g.sh; ++r) {
    const DcPhase fh = dc_phase(r, g.ph, g.sh, g.kh, t.tmh, t.dqh);
    for (int i = threadIdx.x; i < items; i += kTPB) {
      const int a = (int)fastdiv(i, t.fd_row);
      const int c = i - a * rowitems;  // output column within the tile
      const int bq = (int)fastdiv(c, t.fd_sw), s = c - bq * g.sw;
      const int oh = (b.q0h + a) * g.sh + r, ow = b.q0w * g.sw + c;
      if (oh >= g.OH || ow >= g.OW) continue;
      const DcPhase fw = dc_phase(s, g.pw, g.sw, g.kw, t.tmw, t.dqw);
      float acc[CB];
#pragma unroll
      for (int m = 0; m < CB; ++m) acc[m] = 0.f;
      const float* xb = win + (a + fh.off) * t.LW + bq + fw.off;
      const float* wb = wl + (r * g.sw + s) * per_p;
      for (int tt = 0; tt < fh.T; ++tt)
        for (int u = 0; u < fw.T; ++u) {
          const float* xp = xb - tt * t.LW - u;
          const float* wq = wb + (tt * t.tmw + u) * g.cig * CB;
          for (int ci = 0; ci < g.cig; ++ci) {
            const float xv = xp[ci * t.per];
#pragma unroll
            for (int m = 0; m < CB; ++m) acc[m] += xv * wq[ci * CB + m];
          }
        }
#pragma unroll
      for (int m = 0; m < CB; ++m) {
        const int co = b.ct * CB + m;
        if (co >= g.cog) break;
        const int cg = b.grp * g.cog + co;
        y[((b.n * Cout + cg) * g.OH + oh) * g.OW + ow] =
            acc[m] + (bias ? bias[cg] : 0.f);
      }
    }
  }
}

// =============================================================== backward
// For forward's direct zone only (both channel counts per group <= 4:
// bilinear upsampling with group == channels), where the im2col + GEMM route
// is at its worst.  MFMA variants of both passes were written and measured
// (profiles/deconv.txt, "backward"): they lost to im2col + GEMMs by 1.8x at
// 256 -> 128 k4 s2 and 4.2x at 128 -> 64 k2 s2, so every layer outside the
// direct zone is refused here and keeps that route.
//
// Cells are now the INPUT pixels (h, w).  Phase (r, s) of the top gradient,
// dy_rs[q] = dy[sh*q + r][sw*q' + s], reaches input row h through tap t at
// cell row q = h - dq(r) + t, so a tile of TQH x kTQW input cells needs the
// cell rows from q0 - dqmin - ddh on, LH = TQH + tmh - 1 + ddh of them: the
// forward window's extent, per phase.
constexpr int kBwdBlocks = 1024;  // wgrad grid aimed at: 4 blocks per CU
// Most split-K slices of wgrad.  The partials are slices x cell splits x the
// padded dW, written once and read once by the reduce: at 32 slices of 16
// splits a k4 layer of 512 one-channel groups holds 16 MB of them, and a
// thread still accumulates 1 / 32 of its cells in registers.  A policy
// constant, NOT measured.
constexpr int kMaxSlices = 32;

enum { kBwdData = 0, kBwdWeight = 1 };

struct DbPlan {
  int var;
  int P, tmh, tmw, slots, dqh, dqw, ddh, ddw;  // forward's phase geometry
  int TQH, ty, tx;         // input-cell rows per tile (columns: kTQW), tiles
  int LH, LW, plane, per;  // window per phase; plane = LH * LW; P planes | 1
  int cc, chunks;          // dy channels staged; chunks of them (1)
  int mt, cot;             // CB: padded channels per group; channel tiles (1)
  int cells, xst;          // TQH * kTQW; wgrad's x tile stride
  int items, ipb, slices;  // wgrad: (image, tile) items; per slice; slices
  int tpt, nsplit, passes; // wgrad: threads along the taps; threads sharing
                           // a tap, each with its own cells; tap passes
  int win_floats, wl_floats, x_floats;
  long pstride;            // WpT floats per (group, phase): slots * cog * CB
  long part_floats;        // wgrad partials
  int blocks;
  bool fits;
  FastDiv fd_area, fd_rw, fd_sh, fd_sw, fd_cells;
};

DbPlan db_plan(const Deconv& g, int pass) {
  const DcPlan f = dc_plan(g);
  DbPlan t{};
  // outside the direct zone: refused, see above
  if (g.cog > kDirectMaxCog || g.cig > kDirectMaxCig) return t;
  t.P = f.P, t.tmh = f.tmh, t.tmw = f.tmw, t.slots = f.slots;
  t.dqh = f.dqh, t.dqw = f.dqw;
  t.ddh = (g.sh - 1 + g.ph) / g.sh - t.dqh;
  t.ddw = (g.sw - 1 + g.pw) / g.sw - t.dqw;
  t.LW = kTQW + t.tmw - 1 + t.ddw;
  t.tx = ceil_div(g.W, kTQW);
  const int khkw = g.kh * g.kw;
  auto per = [&](int tqh) {
    return (t.P * (tqh + t.tmh - 1 + t.ddh) * t.LW) | 1;
  };
  // window of every output channel, dgrad's packed weights or wgrad's x
  // tile beside it; CB pads both channel counts
  const int m = std::max(g.cig, g.cog), CB = m == 1 ? 1 : m == 2 ? 2 : 4;
  auto xfl = [&](int tqh) {
    return pass == kBwdWeight ? CB * (tqh * kTQW + 1) : 0;
  };
  t.var = kVarDirect;
  t.mt = CB;
  t.cot = 1;
  t.cc = pass == kBwdWeight ? CB : g.cog;
  t.chunks = 1;
  t.pstride = (long)t.slots * g.cog * CB;
  t.wl_floats = pass == kBwdData ? (int)(t.P * t.pstride) : 0;
  t.TQH = 16;
  auto floats = [&](int tqh) {
    return (long)round_up(t.cc * per(tqh), 4) + t.wl_floats + xfl(tqh);
  };
  while (floats(t.TQH) > kLdsFloats && t.TQH > 1) t.TQH /= 2;
  t.fits = floats(t.TQH) <= kLdsFloats;
  t.tpt = std::min(khkw, kTPB);
  t.nsplit = kTPB / t.tpt;
  t.passes = ceil_div(khkw, t.tpt);
  t.LH = t.TQH + t.tmh - 1 + t.ddh;
  t.plane = t.LH * t.LW;
  t.per = per(t.TQH);
  t.win_floats = round_up(t.cc * t.per, 4);
  t.cells = t.TQH * kTQW;
  t.xst = t.cells + 1;
  t.x_floats = xfl(t.TQH);
  t.ty = ceil_div(g.H, t.TQH);
  if (pass == kBwdData) {
    t.blocks = g.N * g.G * t.ty * t.tx;
  } else {
    t.items = g.N * t.ty * t.tx;
    const int want = std::min(
        {t.items, kMaxSlices, std::max(1, ceil_div(kBwdBlocks, g.G))});
    t.ipb = ceil_div(t.items, want);
    t.slices = ceil_div(t.items, t.ipb);
    t.blocks = t.slices * g.G;
    t.part_floats = (long)t.slices * t.nsplit * g.G * khkw * CB * CB;
  }
  t.fd_area = fastdiv_make((unsigned long)t.plane * g.sh * g.sw);
  t.fd_rw = fastdiv_make((unsigned long)t.LW * g.sw);
  t.fd_sh = fastdiv_make(g.sh);
  t.fd_sw = fastdiv_make(g.sw);
  t.fd_cells = fastdiv_make(t.cells);
  return t;
}

bool db_counts_fit(const Deconv& g, const DbPlan& t) {
  const long lim = 1L << 31;
  return (long)g.N * g.G * g.cig * g.H * g.W < lim &&
         (long)g.N * g.G * g.cog * g.OH * g.OW < lim &&
         (long)g.G * t.P * t.pstride < lim / 2 && t.part_floats < lim &&
         (long)g.N * g.G * t.ty * t.tx < lim;
}

// WpT[g][p][slot][co][ci]: ci innermost and padded to CB, the channels a
// dgrad thread accumulates, so its weights of one (tap, co) are one LDS
// vector; pads are zero
__global__ void k_deconv_pack_wt(Deconv g, DbPlan t,
                                 const float* __restrict__ w,
                                 float* __restrict__ wpt) {
  const int total = (int)(g.G * t.P * t.pstride);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    int e = i / t.mt;
    const int ci = i - e * t.mt;
    const int co = e % g.cog;
    e /= g.cog;
    const int slot = e % t.slots;
    e /= t.slots;
    wpt[i] = dc_pack_value(g, t.tmh, t.tmw, t.dqh, t.dqw, w, e / t.P, e % t.P,
                           slot, ci, co);
  }
}

// The top gradient's window of `ccn` channels from ch0 of image n, cells
// from (qbh, qbw): read in row order (coalesced), written split by phase,
// win[c][per] holding [P][LH][LW].  The operand of any (phase, tap) is then
// unit-stride across lanes; laid out as dy is, it would be read at stride sw.
// Zero outside the image and for the chunk's channels past ccn.
__device__ inline void db_stage_dy(float* win, const Deconv& g,
                                   const DbPlan& t,
                                   const float* __restrict__ dy, int ch0,
                                   int ccn, int n, int qbh, int qbw) {
  const int rw = t.LW * g.sw, area = t.plane * g.sh * g.sw;
  const int chans = g.G * g.cog;
  for (int i = threadIdx.x; i < t.cc * area; i += kTPB) {
    const int c = (int)fastdiv(i, t.fd_area);
    const int rem = i - c * area;
    const int R = (int)fastdiv(rem, t.fd_rw), Cc = rem - R * rw;
    const int qa = (int)fastdiv(R, t.fd_sh), r = R - qa * g.sh;
    const int qb = (int)fastdiv(Cc, t.fd_sw), s = Cc - qb * g.sw;
    const int oh = qbh * g.sh + R, ow = qbw * g.sw + Cc;
    float v = 0.f;
    if (c < ccn && (unsigned)oh < (unsigned)g.OH &&
        (unsigned)ow < (unsigned)g.OW)
      v = dy[((n * chans + ch0 + c) * g.OH + oh) * g.OW + ow];
    win[c * t.per + ((r * g.sw + s) * t.LH + qa) * t.LW + qb] = v;
  }
}

// wgrad's x tile: xs[c][xst] holding [TQH][kTQW] cells of `rows` channels,
// zero outside the image and past cn channels
__device__ inline void db_stage_x(float* xs, const Deconv& g, const DbPlan& t,
                                  const float* __restrict__ x, int rows,
                                  int ch0, int cn, int n, int h0, int w0) {
  const int chans = g.G * g.cig;
  for (int i = threadIdx.x; i < rows * t.cells; i += kTPB) {
    const int c = (int)fastdiv(i, t.fd_cells);
    const int cell = i - c * t.cells;
    const int h = h0 + cell / kTQW, w = w0 + cell % kTQW;
    float v = 0.f;
    if (c < cn && h < g.H && w < g.W)
      v = x[((n * chans + ch0 + c) * g.H + h) * g.W + w];
    xs[c * t.xst + cell] = v;
  }
}

// window row (column) offset, under a tile's first cell, of tap 0 of the
// phase whose forward offset is `off`: ddh - (dq - dqmin); tap t adds t
__device__ inline int db_off(int dd, int tmax, int off) {
  return dd + tmax - 1 - off;
}

// ---------------------------------------------------------- dgrad, direct
// CB: input channels per thread.  A thread owns input pixels, lanes along w.
template <int CB>
__global__ __launch_bounds__(kTPB) void k_deconv_bwd_data_direct(
    Deconv g, DbPlan t, const float* __restrict__ dy,
    const float* __restrict__ wpt, float* __restrict__ dx) {
  extern __shared__ float lds[];
  float* win = lds;                // [cog][per]
  float* wl = lds + t.win_floats;  // [P][slot][co][CB]
  const DcBlock b = dc_block(g, t);
  db_stage_dy(win, g, t, dy, b.grp * g.cog, g.cog, b.n,
              b.q0h - t.dqh - t.ddh, b.q0w - t.dqw - t.ddw);
  const float* wg = wpt + (long)b.grp * t.wl_floats;
  for (int i = threadIdx.x; i < t.wl_floats; i += kTPB) wl[i] = wg[i];
  __syncthreads();

  for (int i = threadIdx.x; i < t.cells; i += kTPB) {
    const int a = i / kTQW, bq = i % kTQW;
    const int h = b.q0h + a, w = b.q0w + bq;
    if (h >= g.H || w >= g.W) continue;
    float acc[CB];
#pragma unroll
    for (int m = 0; m < CB; ++m) acc[m] = 0.f;
    for (int r = 0; r < g.sh; ++r) {
      const DcPhase fh = dc_phase(r, g.ph, g.sh, g.kh, t.tmh, t.dqh);
      for (int s = 0; s < g.sw; ++s) {
        const DcPhase fw = dc_phase(s, g.pw, g.sw, g.kw, t.tmw, t.dqw);
        const int p = r * g.sw + s;
        const float* yb = win + p * t.plane +
                          (a + db_off(t.ddh, t.tmh, fh.off)) * t.LW + bq +
                          db_off(t.ddw, t.tmw, fw.off);
        const float* wb = wl + p * t.pstride;
        for (int tt = 0; tt < fh.T; ++tt)
          for (int u = 0; u < fw.T; ++u) {
            const float* yp = yb + tt * t.LW + u;
            const float* wq = wb + (tt * t.tmw + u) * g.cog * CB;
            for (int co = 0; co < g.cog; ++co) {
              const float v = yp[co * t.per];
#pragma unroll
              for (int m = 0; m < CB; ++m) acc[m] += v * wq[co * CB + m];
            }
          }
      }
    }
#pragma unroll
    for (int m = 0; m < CB; ++m)
      if (m < g.cig)
        dx[((b.n * g.G * g.cig + b.grp * g.cig + m) * g.H + h) * g.W + w] =
            acc[m];
  }
}

// tap (ki, kj) of the kernel as wgrad sees it: the phase plane and the
// window offset under a tile's first cell
struct DbTap {
  int p, off;  // phase; offset within the plane
};
__device__ inline DbTap db_tap(const Deconv& g, const DbPlan& t, int tau) {
  const int ki = tau / g.kw, kj = tau - ki * g.kw;
  const int r = ((ki - g.ph) % g.sh + g.sh) % g.sh;
  const int s = ((kj - g.pw) % g.sw + g.sw) % g.sw;
  const DcPhase fh = dc_phase(r, g.ph, g.sh, g.kh, t.tmh, t.dqh);
  const DcPhase fw = dc_phase(s, g.pw, g.sw, g.kw, t.tmw, t.dqw);
  return {r * g.sw + s,
          (db_off(t.ddh, t.tmh, fh.off) + ki / g.sh) * t.LW +
              db_off(t.ddw, t.tmw, fw.off) + kj / g.sw};
}

// the wgrad block's slice item: image and first cell
struct DbItem {
  int n, h0, w0;
};
__device__ inline DbItem db_item(const DbPlan& t, int it) {
  const int n = it / (t.ty * t.tx), rem = it - n * (t.ty * t.tx);
  return {n, rem / t.tx * t.TQH, rem % t.tx * kTQW};
}

// ---------------------------------------------------------- wgrad, direct
// Threads own taps (256 of them at k16); with fewer taps than threads,
// nsplit threads share a tap and take every nsplit-th cell, each writing a
// partial of its own.  x is a broadcast read.  CB pads cig and cog.
template <int CB>
__global__ __launch_bounds__(kTPB) void k_deconv_bwd_weight_direct(
    Deconv g, DbPlan t, const float* __restrict__ x,
    const float* __restrict__ dy, float* __restrict__ part) {
  extern __shared__ float lds[];
  float* win = lds;                // [CB][per]
  float* xs = lds + t.win_floats;  // [CB][xst]
  const int grp = blockIdx.x % g.G, sl = blockIdx.x / g.G;
  const int khkw = g.kh * g.kw;
  const int js = threadIdx.x / t.tpt, tau0 = threadIdx.x - js * t.tpt;
  const int it0 = sl * t.ipb, it1 = min(t.items, it0 + t.ipb);

  for (int pass = 0; pass < t.passes; ++pass) {
    const int tau = tau0 + pass * t.tpt;
    const bool live = js < t.nsplit && tau < khkw;
    const DbTap tap = db_tap(g, t, min(tau, khkw - 1));
    float acc[CB][CB];
#pragma unroll
    for (int i = 0; i < CB; ++i)
#pragma unroll
      for (int o = 0; o < CB; ++o) acc[i][o] = 0.f;
    for (int it = it0; it < it1; ++it) {
      const DbItem m = db_item(t, it);
      __syncthreads();
      db_stage_dy(win, g, t, dy, grp * g.cog, g.cog, m.n,
                  m.h0 - t.dqh - t.ddh, m.w0 - t.dqw - t.ddw);
      db_stage_x(xs, g, t, x, CB, grp * g.cig, g.cig, m.n, m.h0, m.w0);
      __syncthreads();
      if (!live) continue;
      const float* B = win + tap.p * t.plane + tap.off;
      for (int cell = js; cell < t.cells; cell += t.nsplit) {
        const float* Bc = B + cell / kTQW * t.LW + cell % kTQW;
        float dv[CB];
#pragma unroll
        for (int o = 0; o < CB; ++o) dv[o] = Bc[o * t.per];
#pragma unroll
        for (int i = 0; i < CB; ++i) {
          const float xv = xs[i * t.xst + cell];
#pragma unroll
          for (int o = 0; o < CB; ++o) acc[i][o] += xv * dv[o];
        }
      }
    }
    if (!live) continue;
    float* pb = part + ((((long)sl * t.nsplit + js) * g.G + grp) * khkw + tau) *
                           (CB * CB);
#pragma unroll
    for (int i = 0; i < CB; ++i)
#pragma unroll
      for (int o = 0; o < CB; ++o) pb[i * CB + o] = acc[i][o];
  }
}

// dW[g * cig + ci][co][tap] = the sum over `nsl` partial slabs
// [g][tap][CB][CB] in slab order; pad channels are dropped
__global__ void k_deconv_bwd_weight_reduce(Deconv g, int nsl, int CB,
                                           const float* __restrict__ part,
                                           float* __restrict__ dw) {
  const int khkw = g.kh * g.kw;
  const int slab = g.G * khkw * CB * CB;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < slab;
       i += gridDim.x * blockDim.x) {
    int e = i / CB;
    const int co = i - e * CB;
    const int ci = e % CB;
    e /= CB;
    const int tau = e % khkw, grp = e / khkw;
    if (ci >= g.cig || co >= g.cog) continue;
    float sum = 0.f;
    for (int s = 0; s < nsl; ++s) sum += part[(long)s * slab + i];
    dw[((grp * g.cig + ci) * g.cog + co) * khkw + tau] = sum;
  }
}

}  // namespace

bool deconv_supported(const Deconv& g) {
  const DcPlan t = dc_plan(g);
  return t.fits && dc_counts_fit(g, t);
}

void deconv_fwd(hipStream_t s, const Deconv& g, const float* x,
                const float* w, const float* bias, float* y) {
  const DcPlan t = dc_plan(g);
  CHECK_(t.fits) << "deconv: window does not fit the LDS tile";
  CHECK_(dc_counts_fit(g, t)) << "deconv: tensor of 2^31 elements or more";
  const double nx = (double)g.N * g.G * g.cig * g.H * g.W;
  const double ny = (double)g.N * g.G * g.cog * g.OH * g.OW;
  const double nw = (double)g.G * g.cig * g.cog * g.kh * g.kw;
  // every input pixel meets every tap once (edges included: an upper bound)
  PerfScope perf(PERF_CLASS("deconv_fwd"), s, 2.0 * nx * g.cog * g.kh * g.kw,
                 4.0 * (nx + ny + nw));
  const long nwp = (long)g.G * t.P * t.pstride;
  float* wp = (float*)Workspace::get_global().get(Workspace::kDeconvW,
                                                  sizeof(float) * nwp);
  hipLaunchKernelGGL(k_deconv_pack_w,
                     dim3((unsigned)std::min<long>((nwp + kTPB - 1) / kTPB,
                                                   2048)),
                     dim3(kTPB), 0, s, g, t, w, wp);
  const dim3 grid(t.blocks), block(kTPB);
  const size_t lds = sizeof(float) * ((size_t)t.win_floats + t.wl_floats);
#define DC_MFMA(MR, NPH)                                                   \
  hipLaunchKernelGGL((k_deconv_mfma<MR, NPH>), grid, block, lds, s, g, t, \
                     x, wp, bias, y)
#define DC_DIRECT(CB)                                                      \
  hipLaunchKernelGGL((k_deconv_direct<CB>), grid, block, lds, s, g, t, x, \
                     wp, bias, y)
  if (t.var == kVarDirect) {
    if (t.mt == 1) DC_DIRECT(1);
    else if (t.mt == 2) DC_DIRECT(2);
    else DC_DIRECT(4);
  } else if (t.mt == 64) {
    if (t.P == 2) DC_MFMA(2, 2);
    else DC_MFMA(2, 4);
  } else {
    if (t.P == 2) DC_MFMA(1, 2);
    else DC_MFMA(1, 4);
  }
#undef DC_MFMA
#undef DC_DIRECT
  kernel_trace_deconv(t.var, t.P, t.chunks, t.ty, t.tx, t.blocks);
}

bool deconv_bwd_data_supported(const Deconv& g) {
  const DbPlan t = db_plan(g, kBwdData);
  return t.fits && db_counts_fit(g, t);
}

bool deconv_bwd_weight_supported(const Deconv& g) {
  const DbPlan t = db_plan(g, kBwdWeight);
  return t.fits && db_counts_fit(g, t);
}

void deconv_bwd_data(hipStream_t s, const Deconv& g, const float* dy,
                     const float* w, float* dx) {
  const DbPlan t = db_plan(g, kBwdData);
  CHECK_(t.fits) << "deconv dgrad: window does not fit the LDS tile";
  CHECK_(db_counts_fit(g, t)) << "deconv dgrad: 2^31 elements or more";
  const double nx = (double)g.N * g.G * g.cig * g.H * g.W;
  const double ny = (double)g.N * g.G * g.cog * g.OH * g.OW;
  const double nw = (double)g.G * g.cig * g.cog * g.kh * g.kw;
  PerfScope perf(PERF_CLASS("deconv_bwd_data"), s,
                 2.0 * nx * g.cog * g.kh * g.kw, 4.0 * (nx + ny + nw));
  const long nwp = (long)g.G * t.P * t.pstride;
  float* wpt = (float*)Workspace::get_global().get(Workspace::kDeconvWT,
                                                   sizeof(float) * nwp);
  hipLaunchKernelGGL(k_deconv_pack_wt,
                     dim3((unsigned)std::min<long>((nwp + kTPB - 1) / kTPB,
                                                   2048)),
                     dim3(kTPB), 0, s, g, t, w, wpt);
  const dim3 grid(t.blocks), block(kTPB);
  const size_t lds = sizeof(float) * ((size_t)t.win_floats + t.wl_floats);
#define DB_DIRECT(CB)                                                       \
  hipLaunchKernelGGL((k_deconv_bwd_data_direct<CB>), grid, block, lds, s, g, \
                     t, dy, wpt, dx)
  if (t.mt == 1) DB_DIRECT(1);
  else if (t.mt == 2) DB_DIRECT(2);
  else DB_DIRECT(4);
#undef DB_DIRECT
  kernel_trace_deconv_bwd(kBwdData, t.var, t.P, t.chunks, t.ty, t.tx,
                          t.blocks);
}

void deconv_bwd_weight(hipStream_t s, const Deconv& g, const float* x,
                       const float* dy, float* dw) {
  const DbPlan t = db_plan(g, kBwdWeight);
  CHECK_(t.fits) << "deconv wgrad: window does not fit the LDS tile";
  CHECK_(db_counts_fit(g, t)) << "deconv wgrad: 2^31 elements or more";
  const double nx = (double)g.N * g.G * g.cig * g.H * g.W;
  const double ny = (double)g.N * g.G * g.cog * g.OH * g.OW;
  const double nw = (double)g.G * g.cig * g.cog * g.kh * g.kw;
  PerfScope perf(PERF_CLASS("deconv_bwd_weight"), s,
                 2.0 * nx * g.cog * g.kh * g.kw, 4.0 * (nx + ny + nw));
  float* part = (float*)Workspace::get_global().get(
      Workspace::kDeconvPart, sizeof(float) * t.part_floats);
  const dim3 grid(t.blocks), block(kTPB);
  const size_t lds = sizeof(float) * ((size_t)t.win_floats + t.x_floats);
#define DB_DIRECT(CB)                                                      \
  hipLaunchKernelGGL((k_deconv_bwd_weight_direct<CB>), grid, block, lds, s, \
                     g, t, x, dy, part)
  if (t.mt == 1) DB_DIRECT(1);
  else if (t.mt == 2) DB_DIRECT(2);
  else DB_DIRECT(4);
#undef DB_DIRECT
  const int nsl = t.slices * t.nsplit;
  const long slab = t.part_floats / nsl;
  hipLaunchKernelGGL(k_deconv_bwd_weight_reduce,
                     dim3((unsigned)std::min<long>((slab + kTPB - 1) / kTPB,
                                                   2048)),
                     dim3(kTPB), 0, s, g, nsl, t.mt, part, dw);
  kernel_trace_deconv_bwd(kBwdWeight, t.var, t.P, t.ipb, t.slices, 0,
                          t.blocks);
}

}  // namespace gpu
}  // namespace camd
