// gemm_common.hpp — shared pieces of the MFMA GEMM family (fp32 + bf16):
// the kernel argument block, the 16-element operand readers that
// understand plain, channel-view and implicit-im2col-view addressing
// (strides included; the 64-bit reader and the 32-bit staging cursor
// reader), and the kernel parts every family member uses (tile
// swizzle, split-K range, accumulator epilogue, K-waves combine).  See
// gemm_f32.hip for the design notes.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../layers.hpp"

namespace camd {
namespace gpu {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

struct GemmArgs {
  const float* A;
  const float* B;
  float* C;
  long M, N, K;
  long lda, ldb, ldc;
  float alpha, beta;
  // epilogue
  long spad, S, n_stride;  // spad>0 => conv NCHW scatter
  const float* bias;
  int bias_per_col;
  int relu;
  long Srow;               // dest per-row stride (== S unless strided)
  int OWo, osh, osw, Wd;   // strided scatter (OWo>0)
  // operand views (spad==0 => plain)
  GemmView av, bv;
  // split-K
  float* slab;  // partials [SK][M][N] when SK>1
  int SK;
  // swizzle
  long tn, tiles;  // column-tile count, total tiles
  // epilogue scatter divisors (spad, OWo) for the 32-bit kernels
  FastDiv fd_spad, fd_owo;
};

// 16 consecutive elements from p, the first nvalid of them real: one
// aligned float4 quad when all are, else element by element with zero fill.
__device__ __forceinline__ void read16_run(const float* __restrict__ p,
                                           long nvalid, float (&out)[16]) {
  if (nvalid >= 16 && (((uintptr_t)p) & 15) == 0) {
    const f32x4* p4 = (const f32x4*)p;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 t = p4[j];
      out[4 * j + 0] = t.x;
      out[4 * j + 1] = t.y;
      out[4 * j + 2] = t.z;
      out[4 * j + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) out[j] = j < nvalid ? p[j] : 0.f;
  }
}

// Plain operand: base = P + r*ld + q, valid j while q + j < qmax, r < rmax.
__device__ __forceinline__ void read16_plain(const float* __restrict__ P,
                                             long r, long q, long ld,
                                             long rmax, long qmax,
                                             float (&out)[16]) {
  read16_run(P + r * ld + q, (r < rmax && q < qmax) ? qmax - q : 0, out);
}

// Read 16 consecutive elements along the contiguous axis — the 64-bit
// reader of the W64 kernels (sizes past the 32-bit staging's limits, see
// gemm()).
//   plain:  base = P + r*ld + q,      valid j while q + j < qmax, r < rmax
//   view:   n = q / spad, sp = q % spad,
//           base = P + (n*chan + r)*S + sp, valid j while sp + j < S
// (q is 16-aligned and spad % 16 == 0, so a chunk never crosses images)
__device__ __forceinline__ void read16(const float* __restrict__ P, long r,
                                       long q, long ld, long rmax,
                                       long qmax, const GemmView& v,
                                       float (&out)[16]) {
  const float* p;
  long nvalid;  // elements valid from j=0
  if (v.spad && v.kh > 0) {
    // implicit im2col (d1, any stride): r = (c, ki, kj), sp = (oh, ow)
    const long n = q / v.spad;
    const long sp = q - n * v.spad;
    if (r >= rmax || sp >= v.S || q >= qmax) {
#pragma unroll
      for (int j = 0; j < 16; ++j) out[j] = 0.f;
      return;
    }
    const int c = (int)(r / (v.kh * v.kw));
    const int krem = (int)(r - (long)c * v.kh * v.kw);
    const int ki = krem / v.kw, kj = krem - (krem / v.kw) * v.kw;
    int oh = (int)(sp / v.OW);
    int ow = (int)(sp - (long)oh * v.OW);
    int h = oh * v.sh - v.ph + ki;
    int w = ow * v.sw - v.pw + kj;
    const float* xp = P + (n * v.chan + c) * (long)v.H * v.W;
    const long smax = v.S - sp;  // elements left in this image
    // fast path: chunk stays in one output row, fully interior
    if (smax >= 16 && ow + 16 <= v.OW && h >= 0 && h < v.H && w >= 0 &&
        w + 15 * v.sw < v.W) {
      if (v.sw == 1) {
        const float* p = xp + h * v.W + w;
        if ((((uintptr_t)p) & 15) == 0) {
          const f32x4* p4 = (const f32x4*)p;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const f32x4 t = p4[j];
            out[4 * j + 0] = t.x;
            out[4 * j + 1] = t.y;
            out[4 * j + 2] = t.z;
            out[4 * j + 3] = t.w;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 16; ++j) out[j] = p[j];
        }
      } else {  // strided row gather: 16 independent loads
        const float* p = xp + h * v.W + w;
#pragma unroll
        for (int j = 0; j < 16; ++j) out[j] = p[j * v.sw];
      }
      return;
    }
    if (v.OW >= 16) {
      // at most ONE row wrap inside the 16-chunk: all 16 loads become
      // independent (the sequential walk would chain their addresses)
      const int jw = v.OW - ow;       // first j on the next output row
      const int w0 = w;               // input col at j=0
      const int wreset = -v.pw + kj;  // input col after the wrap
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const bool wrapped = j >= jw;
        const int hj = h + (wrapped ? v.sh : 0);
        const int wj = (wrapped ? wreset + (j - jw) * v.sw
                                : w0 + j * v.sw);
        const bool ok =
            j < smax && hj >= 0 && hj < v.H && wj >= 0 && wj < v.W;
        out[j] = ok ? xp[hj * v.W + wj] : 0.f;
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const bool ok = j < smax && h >= 0 && h < v.H && w >= 0 && w < v.W;
      out[j] = ok ? xp[h * v.W + w] : 0.f;
      // next output pixel: ow+1 (input w += sw), wrapping to the next row
      if (++ow == v.OW) {
        ow = 0;
        ++oh;
        h += v.sh;
        w = -v.pw + kj;
      } else {
        w += v.sw;
      }
    }
    return;
  }
  // (written out, not through read16_run: the bf16 kernels, which all read
  // through here, spill 4 bytes/lane more with the helper — DESIGN.md §8,
  // "GEMM helper forms")
  if (v.spad) {
    const long n = q / v.spad;
    const long sp = q - n * v.spad;
    p = P + (n * v.chan + r) * v.S + sp;
    nvalid = (r < rmax && sp < v.S && q < qmax) ? v.S - sp : 0;
  } else {
    p = P + r * ld + q;
    nvalid = (r < rmax && q < qmax) ? qmax - q : 0;
  }
  if (nvalid >= 16 && (((uintptr_t)p) & 15) == 0) {
    const f32x4* p4 = (const f32x4*)p;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 t = p4[j];
      out[4 * j + 0] = t.x;
      out[4 * j + 1] = t.y;
      out[4 * j + 2] = t.z;
      out[4 * j + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) out[j] = j < nvalid ? p[j] : 0.f;
  }
}

// ---- 32-bit staging of viewed operands.  In a K-loop one half of a
// thread's (r, q) never changes: q for an operand stored [K][row] (FIXR
// false: B of the NN and TN kernels), r for one stored [row][K] (FIXR
// true: A and B of the NT kernels).  stage_cursor() decomposes that half
// once, before the loop; read16_cur() is a pure function of the cursor and
// the moving half, so every loop form (plain, K-waves with its two register
// sets, split-K with k_lo > 0) uses it unchanged.  Index arithmetic is
// 32-bit with host-computed reciprocals (fastdiv, math.hpp), and an
// element's address is the operand base plus a 32-bit byte offset.  gemm()
// sends sizes that do not fit, and calls whose B is not a view, to the W64
// kernels, which keep read16().
struct StageCur {
  unsigned off;  // element offset of the fixed half
  int h, w;      // im2col: fixed part of the input row / column
  int ow;        // im2col, q fixed: output column of the chunk's first pixel
  int nv;        // q fixed: pixels left in the image from the chunk start
                 // (0: dead chunk); r fixed: 1 when the row exists
};

__device__ __forceinline__ float ld32(const float* __restrict__ P,
                                      unsigned e) {
  return *(const float*)((const char*)P + (e << 2));
}

// x, but opaque to loop-invariant code motion (no instruction).  The
// register allocation of the K-loops rests on it (read16_cur): `make
// check-gemm-resources` fails when an fp32 GEMM kernel has scratch, and is
// the thing to run after a compiler update.
__device__ __forceinline__ int loop_variant(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

// x is the fixed half (q when !FIXR, r when FIXR), xmax its bound.
template <bool FIXR>
__device__ __forceinline__ StageCur stage_cursor(long x, long xmax,
                                                 const GemmView& v) {
  StageCur c{0, 0, 0, 0, 0};
  if (!v.spad) return c;  // plain operands have nothing to decompose
  const unsigned u = (unsigned)x;
  if (!FIXR) {
    const unsigned n = fastdiv(u, v.fd_spad);
    const unsigned sp = u - n * (unsigned)v.spad;
    c.nv = (x < xmax && sp < (unsigned)v.S) ? (int)((unsigned)v.S - sp) : 0;
    if (v.kh > 0) {
      const unsigned oh = fastdiv(sp, v.fd_ow);
      const unsigned ow = sp - oh * (unsigned)v.OW;
      c.off = n * v.img;
      c.h = (int)oh * v.sh - v.ph;
      c.w = (int)ow * v.sw - v.pw;
      c.ow = (int)ow;
    } else {
      c.off = n * v.img + sp;
    }
  } else {
    c.nv = x < xmax;
    if (v.kh > 0) {
      const unsigned ch = fastdiv(u, v.fd_khkw);
      const unsigned krem = u - ch * (unsigned)(v.kh * v.kw);
      const unsigned ki = fastdiv(krem, v.fd_kw);
      c.off = ch * v.hw;
      c.h = (int)ki - v.ph;
      c.w = (int)(krem - ki * (unsigned)v.kw) - v.pw;
    } else {
      c.off = u * v.hw;
    }
  }
  return c;
}

// 16 output pixels of one im2col row from (h, w, ow): input row / column
// and output column of the first, smax pixels left in the image, xoff the
// element offset of the (image, channel) plane.
__device__ __forceinline__ void im2col_chunk(const float* __restrict__ P,
                                             const GemmView& v,
                                             unsigned xoff, int h, int w,
                                             int ow, int smax,
                                             float (&out)[16]) {
  const unsigned e0 = xoff + (unsigned)(h * v.W + w);  // element at j = 0
  // fast path: chunk stays in one output row, fully interior
  if (smax >= 16 && ow + 16 <= v.OW && h >= 0 && h < v.H && w >= 0 &&
      w + 15 * v.sw < v.W) {
    if (v.sw == 1) {
      const float* p = (const float*)((const char*)P + (e0 << 2));
      if ((((uintptr_t)p) & 15) == 0) {
        const f32x4* p4 = (const f32x4*)p;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 t = p4[j];
          out[4 * j + 0] = t.x;
          out[4 * j + 1] = t.y;
          out[4 * j + 2] = t.z;
          out[4 * j + 3] = t.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) out[j] = p[j];
      }
    } else {  // strided row gather: 16 independent loads
#pragma unroll
      for (int j = 0; j < 16; ++j) out[j] = ld32(P, e0 + j * v.sw);
    }
    return;
  }
  if (v.OW >= 16) {
    // at most ONE row wrap inside the 16-chunk, at j = jw: two row
    // segments, each with one row test and one column limit (the pixels
    // left in the image folded in: columns grow with j), and a select
    // between the two running column / offset bases per element
    const int jw = v.OW - ow;            // first j on the next output row
    const int wB = w - v.OW * v.sw;      // next row's column at j = 0
    const int sm = smax < 16 ? smax : 16;
    const int endA = min(v.W, w + sm * v.sw);
    const int endB = min(v.W, wB + sm * v.sw);
    const unsigned limA =
        (h >= 0 && h < v.H) ? (unsigned)max(endA, 0) : 0u;
    const unsigned limB =
        (h + v.sh >= 0 && h + v.sh < v.H) ? (unsigned)max(endB, 0) : 0u;
    const unsigned baseA = e0 - (unsigned)w;
    const unsigned baseB = baseA + (unsigned)(v.sh * v.W);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const bool wrapped = j >= jw;
      const int col = (wrapped ? wB : w) + j * v.sw;
      const bool ok = (unsigned)col < (wrapped ? limB : limA);
      out[j] =
          ok ? ld32(P, (wrapped ? baseB : baseA) + (unsigned)col) : 0.f;
    }
    return;
  }
  // OW < 16 (CAFFE_IMPLICIT_MIN_OW only): sequential pixel walk
  const int wreset = w - ow * v.sw;  // input col after a wrap
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const bool ok = j < smax && h >= 0 && h < v.H && w >= 0 && w < v.W;
    out[j] = ok ? ld32(P, xoff + (unsigned)(h * v.W + w)) : 0.f;
    if (++ow == v.OW) {
      ow = 0;
      h += v.sh;
      w = wreset;
    } else {
      w += v.sw;
    }
  }
}

// read16() of a viewed operand from its cursor.  (r, q) as in read16: the
// half the cursor was built from is passed again but not decomposed.
template <bool FIXR>
__device__ __forceinline__ void read16_cur(const float* __restrict__ P,
                                           const StageCur& c, long r_,
                                           long q_, long rmax_, long qmax_,
                                           const GemmView& v,
                                           float (&out)[16]) {
  const unsigned r = (unsigned)r_, q = (unsigned)q_;
  const unsigned rmax = (unsigned)rmax_, qmax = (unsigned)qmax_;
  unsigned e;   // element offset at j = 0
  int nvalid;   // elements valid from j = 0 (im2col: pixels left)
  // The chunk's pixel count and output column are K-invariant when q is
  // fixed, and so is every per-element test on them (j < nv, j >= OW - ow):
  // left visible, the compiler hoists those 16-wide lane masks out of the
  // K-loop and spills scalar registers to keep them.  Re-read per tile.
  const int cnv = FIXR ? c.nv : loop_variant(c.nv);
  const int cow = FIXR ? c.ow : loop_variant(c.ow);
  if (v.kh > 0) {
    int h, w, ow;
    if (!FIXR) {  // r moves: (c, ki, kj) per tile
      const unsigned ch = fastdiv(r, v.fd_khkw);
      const unsigned krem = r - ch * (unsigned)(v.kh * v.kw);
      const unsigned ki = fastdiv(krem, v.fd_kw);
      e = c.off + ch * v.hw;
      h = c.h + (int)ki;
      w = c.w + (int)(krem - ki * (unsigned)v.kw);
      ow = cow;
      nvalid = r < rmax ? cnv : 0;
    } else {  // q moves: (n, oh, ow) per tile
      const unsigned n = fastdiv(q, v.fd_spad);
      const unsigned sp = q - n * (unsigned)v.spad;
      const unsigned oh = fastdiv(sp, v.fd_ow);
      ow = (int)(sp - oh * (unsigned)v.OW);
      e = n * v.img + c.off;
      h = (int)oh * v.sh + c.h;
      w = ow * v.sw + c.w;
      nvalid = (c.nv && sp < (unsigned)v.S && q < qmax)
                   ? (int)((unsigned)v.S - sp)
                   : 0;
    }
    if (nvalid == 0) {
#pragma unroll
      for (int j = 0; j < 16; ++j) out[j] = 0.f;
      return;
    }
    im2col_chunk(P, v, e, h, w, ow, nvalid, out);
    return;
  }
  if (!FIXR) {
    e = c.off + r * v.hw;
    nvalid = r < rmax ? cnv : 0;
  } else {
    const unsigned n = fastdiv(q, v.fd_spad);
    const unsigned sp = q - n * (unsigned)v.spad;
    e = n * v.img + c.off + sp;
    nvalid = (c.nv && sp < (unsigned)v.S && q < qmax)
                 ? (int)((unsigned)v.S - sp)
                 : 0;
  }
  read16_run((const float*)((const char*)P + (e << 2)), nvalid, out);
}

// What the kernels call.  W64 kernels read through read16() and their
// cursor is empty; the others read plain operands with read16_plain() and
// viewed ones from the cursor.  PLAIN: the operand cannot be a view (a
// transposed A — gemm() checks), so no view code is built for it.
template <bool FIXR, bool W64>
__device__ __forceinline__ StageCur make_cursor(long x, long xmax,
                                                const GemmView& v) {
  if (W64) return StageCur{0, 0, 0, 0, 0};
  return stage_cursor<FIXR>(x, xmax, v);
}
template <bool FIXR, bool W64, bool PLAIN = false>
__device__ __forceinline__ void read16v(const float* __restrict__ P,
                                        const StageCur& c, long r, long q,
                                        long ld, long rmax, long qmax,
                                        const GemmView& v,
                                        float (&out)[16]) {
  if (W64)
    read16(P, r, q, ld, rmax, qmax, v, out);
  else if (PLAIN || !v.spad)
    read16_plain(P, r, q, ld, rmax, qmax, out);
  else
    read16_cur<FIXR>(P, c, r, q, rmax, qmax, v, out);
}

// ---- kernel parts shared by every GEMM kernel (fp32, slim, bf16, wide)

// Tile of this block.  Bijective XCD-aware swizzle
// (cdna_hip_programming.md T1): contiguous tile chunks per XCD so
// neighbouring tiles share L2-resident panels.
__device__ __forceinline__ void tile_origin(const GemmArgs& g, long& tile_m,
                                            long& tile_n) {
  long flat = blockIdx.x;
  const long nwg = g.tiles;
  const long q = nwg / 8, rr = nwg % 8;
  const long xcd = flat % 8, idx = flat / 8;
  flat = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + idx;
  tile_m = flat / g.tn;
  tile_n = flat - tile_m * g.tn;
}

// K range of split-K slice blockIdx.z; starts BK-aligned so read16 chunks
// stay 16-aligned.  False when the slice is empty (cannot happen for
// SK <= ceil(K / 4BK)).
template <int BK>
__device__ __forceinline__ bool splitk_range(const GemmArgs& g, long& k_lo,
                                             long& k_hi) {
  const int sk = blockIdx.z;
  k_lo = g.K * sk / g.SK / BK * BK;
  k_hi = (sk == g.SK - 1) ? g.K : g.K * (sk + 1) / g.SK / BK * BK;
  return k_lo < k_hi;
}

// Epilogue of one 32x32 MFMA accumulator whose first row is row0; col is
// this lane's column.  C/D map: col = lane&31, acc reg r holds row
// (r&3) + 8*(r>>2) + 4*ksel with ksel = lane>>5 (handed in: the kernels
// hold it already, and deriving it from threadIdx again here made
// k_gemm_bf16, which sits at 256 VGPRs, spill 8 bytes/lane more —
// DESIGN.md §8, "GEMM helper forms").  Split-K blocks store alpha*acc
// into their slab; otherwise bias, ReLU and beta are applied in that order
// and the value goes to C (plain, NCHW scatter or strided scatter).
template <bool SPLITK, bool W64>
__device__ __forceinline__ void store_acc(const GemmArgs& g, const f32x16& a,
                                          long row0, long col, int ksel) {
  if (col >= g.N) return;
  // col is constant across the 16 regs — hoist the scatter division
  long col_base = 0;  // n*n_stride + pix for scatter, col for plain
  bool col_ok = true;
  if (!SPLITK && g.spad > 0) {
    long n, sp;
    if (W64) {
      n = col / g.spad;
      sp = col - n * g.spad;
    } else {
      const unsigned n32 = fastdiv((unsigned)col, g.fd_spad);
      n = n32;
      sp = (unsigned)col - n32 * (unsigned)g.spad;
    }
    col_ok = sp < g.S;  // padded scatter column: no destination
    long pix = sp;
    if (g.OWo > 0) {  // strided scatter (1x1/s2 dgrad)
      const int oh = W64 ? (int)(sp / g.OWo)
                         : (int)fastdiv((unsigned)sp, g.fd_owo);
      const int ow = (int)(sp - (long)oh * g.OWo);
      pix = ((long)oh * g.osh) * g.Wd + (long)ow * g.osw;
    }
    col_base = n * g.n_stride + pix;
  }
  if (!col_ok) return;
  const float cbias =
      (!SPLITK && g.bias && g.bias_per_col) ? g.bias[col] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long row = row0 + ((r & 3) + 8 * (r >> 2) + 4 * ksel);
    if (row >= g.M) continue;
    float v = g.alpha * a[r];
    if (SPLITK) {
      g.slab[((long)blockIdx.z * g.M + row) * g.N + col] = v;
      continue;
    }
    if (g.bias) v += g.bias_per_col ? cbias : g.bias[row];
    if (g.relu) v = fmaxf(v, 0.f);
    const long off =
        g.spad > 0 ? col_base + row * g.Srow : row * g.ldc + col;
    if (g.beta != 0.f) v += g.beta * g.C[off];
    g.C[off] = v;
  }
}

// K-waves combine of the 128-tile kernels: the waves with wk > 0 hold
// K-range partials of output sub-tile `sub` (= wc*mwaves + wr).  They park
// their accumulators in the (now idle) staging LDS and the wk == 0 wave
// adds them in ascending wk order — deterministic.  False for the parked
// waves, which are done.  The wave coordinates are handed in, not derived
// from threadIdx again: the kernels hold them, and re-deriving them moved
// the register allocation of the K-loops.
__device__ __forceinline__ bool kwaves_combine(float* lds, int lane, int wave,
                                               int wk, int sub, int mn,
                                               int kwaves, f32x16& acc00,
                                               f32x16& acc01, f32x16& acc10,
                                               f32x16& acc11) {
  __syncthreads();  // all reads of the staging buffers are done
  if (wk > 0) {
    float* slot = lds + (long)(wave - mn) * 4096 + lane * 64;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      slot[r] = acc00[r];
      slot[16 + r] = acc01[r];
      slot[32 + r] = acc10[r];
      slot[48 + r] = acc11[r];
    }
  }
  __syncthreads();
  if (wk > 0) return false;
  for (int k2 = 1; k2 < kwaves; ++k2) {
    const int src_wave = k2 * mn + sub;
    const float* slot = lds + (long)(src_wave - mn) * 4096 + lane * 64;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc00[r] += slot[r];
      acc01[r] += slot[16 + r];
      acc10[r] += slot[32 + r];
      acc11[r] += slot[48 + r];
    }
  }
  return true;
}

// Runtime (transA, transB, splitk) -> template arguments: calls
// f(TA, TB, SPLITK) with std::bool_constant values.  transA && transB has
// no caller and no instantiation.
template <class F>
void with_gemm_variant(bool ta, bool tb, bool splitk, F&& f) {
  CHECK_(!(ta && tb)) << "transA && transB has no kernel";
  auto with_sk = [&](auto TA, auto TB) {
    if (splitk)
      f(TA, TB, std::true_type{});
    else
      f(TA, TB, std::false_type{});
  };
  if (ta)
    with_sk(std::true_type{}, std::false_type{});
  else if (tb)
    with_sk(std::false_type{}, std::true_type{});
  else
    with_sk(std::false_type{}, std::false_type{});
}

}  // namespace gpu
}  // namespace camd
