// gemm_f32.hip — hand-written fp32 MFMA GEMM for gfx950 (CDNA4).
//
// The kernel family carrying the conv/IP contractions (SURVEY.md §8a
// a1-a4), built on the f32-input MFMA `v_mfma_f32_32x32x2_f32` (exact f32,
// 157.3 TF chip peak; no xf32 on gfx950 — cdna_hip_programming.md §3).
//
// Structure: 128×128 block tile, 256 threads = 4 waves (2×2), each wave a
// 64×64 sub-tile as 2×2 MFMA 32×32 accumulators; BK=32 K-steps staged
// through double-buffered LDS [BK][128+1] (+1 pad → conflict-free b32
// banking), T14 issue-early/write-late, vectorized float4 staging loads on
// the aligned in-bounds fast path, bijective XCD-aware block swizzle (T1).
//
// Operands can be NCHW *views* (GemmView): conv GEMMs read x / dY straight
// from NCHW layout — no transpose pass, and 1×1/s1 convolutions run with no
// im2col/col2im at all.  Fused epilogue: bias (per row/col), optional
// ReLU, NCHW scatter.  Deterministic split-K (partial slabs + fixed-order
// reduce, no atomics — SURVEY.md §7 hard part (b)) for the few-tile/huge-K
// wgrad shapes.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "gemm_common.hpp"

namespace camd {
namespace gpu {

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int LDS_S = BM + 1;  // LDS row stride (floats), BM == BN

// bf16 tensor-core variant (gemm_bf16.hip): same call surface, selected
// by Engine::gemm_bf16 (mixed precision — fp32 storage, bf16 MFMA)
void gemm_launch_bf16(hipStream_t s, bool transA, bool transB, dim3 grid,
                      const GemmArgs& g, bool splitk, bool wide);

// ---- staging of one 128-row operand tile: global -> regs (load) and
// regs -> LDS (write).  The tile is held k-major in LDS, S[k][row] (A rows
// are the M axis, B rows the N axis).  KCONTIG: the operand is stored
// [row][K], contiguous along K (view axis allowed) — A when !TA, B when
// TB; otherwise it is stored [K][row], contiguous along the row axis.
// The thread's tile row (KCONTIG) or 16-row chunk is the half of its
// staging address the K-loop never changes: tile_cursor() takes it apart
// once, stage_load() reads a K-tile from the cursor and k0.
template <bool KCONTIG, bool W64>
__device__ __forceinline__ StageCur tile_cursor(long r0, long R,
                                                const GemmView& v) {
  const int t = threadIdx.x;
  return make_cursor<KCONTIG, W64>(
      r0 + (KCONTIG ? (t & 127) : (t >> 5) * 16), R, v);
}
template <bool KCONTIG, bool W64, bool PLAIN = false>
__device__ __forceinline__ void stage_load(const float* P,
                                           const StageCur& c, long r0,
                                           long k0, long ld, long R, long K,
                                           const GemmView& v,
                                           float (&r)[16]) {
  const int t = threadIdx.x;
  if (KCONTIG)
    read16v<true, W64, PLAIN>(P, c, r0 + (t & 127), k0 + (t >> 7) * 16, ld,
                              R, K, v, r);
  else
    read16v<false, W64, PLAIN>(P, c, k0 + (t & 31), r0 + (t >> 5) * 16, ld,
                               K, R, v, r);
}

template <bool KCONTIG>
__device__ __forceinline__ void stage_write(float* S, const float (&r)[16]) {
  const int t = threadIdx.x;
  if (KCONTIG) {
    const int row = t & 127;
    const int kb = (t >> 7) * 16;
#pragma unroll
    for (int j = 0; j < 16; ++j) S[(kb + j) * LDS_S + row] = r[j];
  } else {
    const int k = t & 31;
    const int rb = (t >> 5) * 16;
#pragma unroll
    for (int j = 0; j < 16; ++j) S[k * LDS_S + rb + j] = r[j];
  }
}
// both operands of a 128x128 block tile at K offset k0
template <bool TA, bool TB, bool W64>
__device__ __forceinline__ void load_tile(const GemmArgs& g,
                                          const StageCur& ca,
                                          const StageCur& cb, long m0,
                                          long n0, long k0, float (&a)[16],
                                          float (&b)[16]) {
  stage_load<!TA, W64, TA>(g.A, ca, m0, k0, g.lda, g.M, g.K, g.av, a);
  stage_load<TB, W64>(g.B, cb, n0, k0, g.ldb, g.N, g.K, g.bv, b);
}
template <bool TA, bool TB>
__device__ __forceinline__ void write_tile(float* As, float* Bs,
                                           const float (&a)[16],
                                           const float (&b)[16]) {
  stage_write<!TA>(As, a);
  stage_write<TB>(Bs, b);
}

template <bool TA, bool TB, bool SPLITK, bool W64>
__launch_bounds__(256, 2) __global__ void k_gemm_f32(GemmArgs g) {
  // one LDS arena carved into As[2] | Bs[2]; the K-waves combine below
  // reuses it after the K-loop
  __shared__ float smem[4 * BK * LDS_S];
  auto As = [&](int buf) -> float* { return smem + buf * (BK * LDS_S); };
  auto Bs = [&](int buf) -> float* {
    return smem + (2 + buf) * (BK * LDS_S);
  };

  long tile_m, tile_n;
  tile_origin(g, tile_m, tile_n);
  const long m0 = tile_m * BM, n0 = tile_n * BN;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // wave decomposition: 2x2 over the 128x128 tile normally; when M or N
  // fits in 64 the spare waves take K-ranges instead (intra-block split-K,
  // combined deterministically through LDS) so small-Cout layers keep all
  // 4 waves busy
  const int mwaves = g.M > 64 ? 2 : 1;
  const int nwaves = g.N > 64 ? 2 : 1;
  const int mn = mwaves * nwaves;
  const int kwaves = 4 / mn;
  const int wr = wave % mwaves;
  const int wc = (wave / mwaves) % nwaves;
  const int wk = wave / mn;
  const int row_in = lane & 31;             // MFMA row/col index
  const int ksel = lane >> 5;               // which of the 2 K elems

  long k_lo = 0, k_hi = g.K;
  if (SPLITK && !splitk_range<BK>(g, k_lo, k_hi)) return;
  const long ntiles = (k_hi - k_lo + BK - 1) / BK;

  f32x16 acc00 = {}, acc01 = {}, acc10 = {}, acc11 = {};
  float ra[16], rb[16];
  // staging cursors: the K-invariant half of this thread's A / B addresses
  // (a transposed A is never a view — gemm() checks — and has none)
  const StageCur ca = tile_cursor<!TA, W64 || TA>(m0, g.M, g.av);
  const StageCur cb = tile_cursor<TB, W64>(n0, g.N, g.bv);

  // The 2x2 MFMA step below stands twice on purpose, in the plain loop and
  // in the K-waves loop: with one definition (lambda or function) the
  // compiler schedules the plain K-loop differently and it runs 5-15%
  // slower ("GEMM helper forms").
  load_tile<TA, TB, W64>(g, ca, cb, m0, n0, k_lo, ra, rb);
  write_tile<TA, TB>(As(0), Bs(0), ra, rb);
  __syncthreads();

  if (kwaves == 1) {
    int cur = 0;
    for (long t = 0; t < ntiles; ++t) {
      if (t + 1 < ntiles)  // issue next tile's global loads early (T14)
        load_tile<TA, TB, W64>(g, ca, cb, m0, n0, k_lo + (t + 1) * BK, ra,
                               rb);
      {
        const float* Ab = As(cur);
        const float* Bb = Bs(cur);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
          const int krow = kk + ksel;
          const float a0 = Ab[krow * LDS_S + wr * 64 + row_in];
          const float a1 = Ab[krow * LDS_S + wr * 64 + 32 + row_in];
          const float b0 = Bb[krow * LDS_S + wc * 64 + row_in];
          const float b1 = Bb[krow * LDS_S + wc * 64 + 32 + row_in];
          acc00 =
              __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
          acc01 =
              __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
          acc10 =
              __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
          acc11 =
              __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
        }
      }
      // single barrier per K-tile: writing buf[cur^1] here is safe — its
      // last readers finished before the previous iteration's barrier; the
      // barrier below publishes these writes for the next iteration's reads
      if (t + 1 < ntiles)
        write_tile<TA, TB>(As(cur ^ 1), Bs(cur ^ 1), ra, rb);
      __syncthreads();
      cur ^= 1;
    }
  } else {
    // kwaves path: BOTH LDS buffers are live per iteration — the wave group
    // with (wk & 1) == p computes buffer p, so all 4 waves issue MFMAs
    // concurrently even when the output tile only needs 1 or 2 of them.
    // For kwaves == 4 the two waves sharing a buffer split the K-step in
    // half; the partials are summed in the LDS combine below.
    const int grp = wk & 1;          // which buffer this wave computes
    const int khalf = wk >> 1;       // kwaves==4: kk half within the step
    const int kk0 = (kwaves == 4) ? khalf * (BK / 2) : 0;
    const int kk1 = (kwaves == 4) ? kk0 + BK / 2 : BK;
    // prologue already staged tile 0 into buf0; stage tile 1 into buf1
    if (1 < ntiles) {
      load_tile<TA, TB, W64>(g, ca, cb, m0, n0, k_lo + BK, ra, rb);
      write_tile<TA, TB>(As(1), Bs(1), ra, rb);
    }
    __syncthreads();
    for (long p = 0; p < ntiles; p += 2) {
      const long t_next0 = p + 2, t_next1 = p + 3;
      if (t_next0 < ntiles)
        load_tile<TA, TB, W64>(g, ca, cb, m0, n0, k_lo + t_next0 * BK, ra,
                               rb);
      float ra2[16], rb2[16];
      if (t_next1 < ntiles)
        load_tile<TA, TB, W64>(g, ca, cb, m0, n0, k_lo + t_next1 * BK, ra2,
                               rb2);
      if (p + grp < ntiles) {
        const float* Ab = As(grp);
        const float* Bb = Bs(grp);
        for (int kk = kk0; kk < kk1; kk += 2) {
          const int krow = kk + ksel;
          const float a0 = Ab[krow * LDS_S + wr * 64 + row_in];
          const float a1 = Ab[krow * LDS_S + wr * 64 + 32 + row_in];
          const float b0 = Bb[krow * LDS_S + wc * 64 + row_in];
          const float b1 = Bb[krow * LDS_S + wc * 64 + 32 + row_in];
          acc00 =
              __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
          acc01 =
              __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
          acc10 =
              __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
          acc11 =
              __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
        }
      }
      __syncthreads();  // everyone done computing before rewriting buffers
      if (t_next0 < ntiles) write_tile<TA, TB>(As(0), Bs(0), ra, rb);
      if (t_next1 < ntiles) write_tile<TA, TB>(As(1), Bs(1), ra2, rb2);
      __syncthreads();
    }
  }
  if (kwaves > 1 &&
      !kwaves_combine(smem, lane, wave, wk, wc * mwaves + wr, mn, kwaves,
                      acc00, acc01, acc10, acc11))
    return;

  const long row0 = m0 + wr * 64, col0 = n0 + wc * 64 + row_in;
  store_acc<SPLITK, W64>(g, acc00, row0, col0, ksel);
  store_acc<SPLITK, W64>(g, acc01, row0, col0 + 32, ksel);
  store_acc<SPLITK, W64>(g, acc10, row0 + 32, col0, ksel);
  store_acc<SPLITK, W64>(g, acc11, row0 + 32, col0 + 32, ksel);
}

// ==================================================================
// k_gemm_slim — small-M tile variant (round 2): TM=32 with
// TN=256, or TM=64 with TN=128.  The 128x128 tile leaves most MFMA rows
// empty for the inception-branch and stage-1 shapes (Cout 16..64:
// GoogLeNet conv GEMMs measured 25% of peak, ResNet-50's
// 64x401408x576 41 TF); here each wave owns a 32(M) x 64(N) sub-tile
// with TWO 32x32 accumulators, waves tile (TM/32) x (4/(TM/32)) — every
// MFMA row is a real output row.  Structure otherwise mirrors k_gemm_f32
// (register T14 pipeline, one barrier per K-tile, same epilogue/split-K
// slabs); at TM=64 the LDS footprint (50 KB) admits 3 blocks/CU.
template <bool TA, bool TB, int TM, bool SPLITK, bool W64>
__launch_bounds__(256, TM == 64 ? 3 : 2) __global__
    void k_gemm_slim(GemmArgs g) {
  constexpr int TN = TM == 32 ? 256 : 128;
  constexpr int AS_S = TM + 1;  // +1 pad: conflict-free b32 banking
  constexpr int BS_S = TN + 1;
  __shared__ float smem[2 * BK * AS_S + 2 * BK * BS_S];
  auto As = [&](int buf) -> float* { return smem + buf * (BK * AS_S); };
  auto Bs = [&](int buf) -> float* {
    return smem + 2 * BK * AS_S + buf * (BK * BS_S);
  };

  long tile_m, tile_n;
  tile_origin(g, tile_m, tile_n);
  const long m0 = tile_m * TM, n0 = tile_n * TN;
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  constexpr int mw = TM / 32;
  const int wr = wave % mw;
  const int wc = wave / mw;
  const int row_in = lane & 31;
  const int ksel = lane >> 5;

  long k_lo = 0, k_hi = g.K;
  if (SPLITK && !splitk_range<BK>(g, k_lo, k_hi)) return;
  const long ntiles = (k_hi - k_lo + BK - 1) / BK;

  f32x16 acc0 = {}, acc1 = {};
  float ra[16], rb[16], rb2[16];

  // staging roles (per K-tile), 16-float chunks:
  //  A !TA ([M][K] contig K): TM*BK floats — threads 0..2*TM-1 cover
  //    (row a_m = t % TM, k a_k = 0 or 16)
  //  A TA ([K][M] contig M): thread (k a_k = t&31, rows a_m = (t>>5)*16
  //    while a_m < TM) — read16 zero-fills past M
  //  B !TB ([K][N] contig N): (k b_k = t&31, cols b_n = (t>>5)*TN/8);
  //    TN=256: two chunks, b_n and b_n + 16
  //  B TB ([N][K] contig K): TN=256: (col b_n = t, k 0 and 16), two
  //    chunks; TN=128: (col b_n = t&127, k b_k = (t>>7)*16), one chunk
  const int a_m = TA ? (t >> 5) * 16 : (t & (TM - 1));
  const int a_k = TA ? (t & 31) : ((t >> (TM == 32 ? 5 : 6)) & 1) * 16;
  const bool a_mine = TA ? a_m < TM : t < 2 * TM;
  const int b_n = TB ? (t & (TN - 1)) : (t >> 5) * (TN / 8);
  const int b_k = TB ? (TN == 256 ? 0 : (t >> 7) * 16) : (t & 31);
  // staging cursors: the K-invariant half of the addresses above (A's
  // row, B's column or column chunk(s); a transposed A is never a view —
  // gemm() checks — and has none)
  const StageCur ca = make_cursor<!TA, W64 || TA>(m0 + a_m, g.M, g.av);
  const StageCur cb = make_cursor<TB, W64>(n0 + b_n, g.N, g.bv);
  const StageCur cb2 = (!TB && TN == 256)
                           ? make_cursor<false, W64>(n0 + b_n + 16, g.N, g.bv)
                           : cb;
  auto a_load = [&](long k0) {
    if (!a_mine) return;
    if (!TA)
      read16v<true, W64>(g.A, ca, m0 + a_m, k0 + a_k, g.lda, g.M, g.K, g.av,
                         ra);
    else
      read16v<false, W64, true>(g.A, ca, k0 + a_k, m0 + a_m, g.lda, g.K,
                                g.M, g.av, ra);
  };
  auto a_write = [&](float* A_) {
    if (!a_mine) return;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (!TA)
        A_[(a_k + j) * AS_S + a_m] = ra[j];
      else
        A_[a_k * AS_S + a_m + j] = ra[j];
    }
  };
  auto b_load = [&](long k0) {
    if (!TB) {
      read16v<false, W64>(g.B, cb, k0 + b_k, n0 + b_n, g.ldb, g.K, g.N,
                          g.bv, rb);
      if (TN == 256)
        read16v<false, W64>(g.B, cb2, k0 + b_k, n0 + b_n + 16, g.ldb, g.K,
                            g.N, g.bv, rb2);
    } else {
      read16v<true, W64>(g.B, cb, n0 + b_n, k0 + b_k, g.ldb, g.N, g.K, g.bv,
                         rb);
      if (TN == 256)
        read16v<true, W64>(g.B, cb, n0 + b_n, k0 + b_k + 16, g.ldb, g.N,
                           g.K, g.bv, rb2);
    }
  };
  auto b_write = [&](float* B_) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (!TB) {
        B_[b_k * BS_S + b_n + j] = rb[j];
        if (TN == 256) B_[b_k * BS_S + b_n + 16 + j] = rb2[j];
      } else {
        B_[(b_k + j) * BS_S + b_n] = rb[j];
        if (TN == 256) B_[(b_k + 16 + j) * BS_S + b_n] = rb2[j];
      }
    }
  };

  a_load(k_lo);
  b_load(k_lo);
  a_write(As(0));
  b_write(Bs(0));
  __syncthreads();

  int cur = 0;
  for (long tt = 0; tt < ntiles; ++tt) {
    if (tt + 1 < ntiles) {
      a_load(k_lo + (tt + 1) * BK);
      b_load(k_lo + (tt + 1) * BK);
    }
    {
      const float* Ab = As(cur);
      const float* Bb = Bs(cur);
#pragma unroll
      for (int kk = 0; kk < BK; kk += 2) {
        const int krow = kk + ksel;
        const float a0 = Ab[krow * AS_S + wr * 32 + row_in];
        const float b0 = Bb[krow * BS_S + wc * 64 + row_in];
        const float b1 = Bb[krow * BS_S + wc * 64 + 32 + row_in];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc1, 0, 0, 0);
      }
    }
    if (tt + 1 < ntiles) {
      a_write(As(cur ^ 1));
      b_write(Bs(cur ^ 1));
    }
    __syncthreads();
    cur ^= 1;
  }

  // (same call form as in k_gemm_bf16, the one measured)
  auto store = [&](const f32x16& a, int tj) {
    const long col = n0 + wc * 64 + tj * 32 + row_in;
    if (col >= g.N) return;
    store_acc<SPLITK, W64>(g, a, m0 + wr * 32, col, ksel);
  };
  store(acc0, 0);
  store(acc1, 1);
}

// fixed-order split-K reduce: C[i] = Σ_sk slab[sk][i]
__global__ void k_splitk_reduce(const float* __restrict__ slab, long MN,
                                int SK, float* __restrict__ C) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < MN;
       i += (long)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int s = 0; s < SK; ++s) acc += slab[(long)s * MN + i];
    C[i] = acc;
  }
}

// MN % 4 == 0 fast path (wgrad MN = Cout x C*kh*kw — always a multiple of
// 4 in practice): float4 rows + 4-way slab unroll keeps 16 loads in
// flight per thread instead of 1 — the scalar loop is latency-bound, not
// bandwidth-bound.  Fixed-shape summation (deterministic).
__global__ void k_splitk_reduce_v4(const float* __restrict__ slab, long MN4,
                                   long MN, int SK, float4* __restrict__ C) {
  const float4* s4 = (const float4*)slab;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < MN4;
       i += (long)gridDim.x * blockDim.x) {
    const long mn4 = MN >> 2;  // f4 elements per slab
    float4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
    float4 a2 = {0, 0, 0, 0}, a3 = {0, 0, 0, 0};
    int s = 0;
    for (; s + 4 <= SK; s += 4) {
      const float4 v0 = s4[(long)s * mn4 + i];
      const float4 v1 = s4[(long)(s + 1) * mn4 + i];
      const float4 v2 = s4[(long)(s + 2) * mn4 + i];
      const float4 v3 = s4[(long)(s + 3) * mn4 + i];
      a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
      a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
      a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
      a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
    }
    for (; s < SK; ++s) {
      const float4 v = s4[(long)s * mn4 + i];
      a0.x += v.x; a0.y += v.y; a0.z += v.z; a0.w += v.w;
    }
    float4 r;
    r.x = (a0.x + a1.x) + (a2.x + a3.x);
    r.y = (a0.y + a1.y) + (a2.y + a3.y);
    r.z = (a0.z + a1.z) + (a2.z + a3.z);
    r.w = (a0.w + a1.w) + (a2.w + a3.w);
    C[i] = r;
  }
}

static void launch_splitk_reduce(hipStream_t s, const float* slab, long MN,
                                 int SK, float* C) {
  if (MN % 4 == 0) {
    const long MN4 = MN / 4;
    const int blocks = (int)std::min<long>((MN4 + 255) / 256, 2048);
    hipLaunchKernelGGL(k_splitk_reduce_v4, dim3(blocks), dim3(256), 0, s,
                       slab, MN4, MN, SK, (float4*)C);
  } else {
    const int blocks = (int)std::min<long>((MN + 255) / 256, 2048);
    hipLaunchKernelGGL(k_splitk_reduce, dim3(blocks), dim3(256), 0, s, slab,
                       MN, SK, C);
  }
}

// ---- route: the kernel gemm() picks for a call.  pick_route() fills the
// dispatch fields, which the launch reads; the trace adds the views and
// the epilogue and logs the same record.
enum RouteFam { kSlim32, kSlim64, kF32_128, kBf16_128, kBf16Wide };
struct GemmRoute {
  long M, N, K, tm, tn;  // tm x tn tiles of TM x TN
  int TM, TN, sk, sh, sw;
  unsigned char fam, ta, tb, kw, av, bv, epi, bias, relu;
};

static GemmRoute pick_route(long M, long N, long K, bool transA, bool transB,
                            bool has_epi, float beta, bool bf16) {
  GemmRoute r{};
  r.M = M;
  r.N = N;
  r.K = K;
  r.ta = transA;
  r.tb = transB;
  // small-M slim tile (32x256 / 64x128): every MFMA row a real output row
  // — the 128^2 tile idles most rows for Cout<=64 layers (inception
  // branches, stage-1 convs).  CAFFE_GEMM_SLIM=0 reverts.
  static const int slim_maxm = [] {
    const char* e = getenv("CAFFE_GEMM_SLIM");  // 0 = off, else max M
    return e ? atoi(e) : 64;
  }();
  if (M <= slim_maxm && N > 64) {
    // the slim tile also serves bf16 mode: M<=64 contractions run the fp32
    // slim kernel (better utilization than the bf16 kwaves path AND exact
    // arithmetic — AMP-style per-shape heterogeneity)
    r.fam = M <= 32 ? kSlim32 : kSlim64;
  } else if (!bf16 && N > 64 && M > 128 && M <= 448 && M % 128 >= 1 &&
             M % 128 <= 64) {
    // remainder rule: a 128-tile grid wastes (128 - M%128) rows of its
    // last tile row (e.g. GoogLeNet conv2 M=192: 25% idle MFMA rows);
    // 64-row tiles fit these exactly at the cost of one extra B pass
    r.fam = kSlim64;
  } else if (bf16) {
    // bf16 wide tile (256x256): quadruple MACs per staged byte — the bf16
    // kernel is staging-bound (see gemm_bf16.hip)
    r.fam = (M > 128 && N > 128) ? kBf16Wide : kBf16_128;
  } else {
    r.fam = kF32_128;
  }
  static const int tile[][2] = {
      {32, 256}, {64, 128}, {128, 128}, {128, 128}, {256, 256}};
  r.TM = tile[r.fam][0];
  r.TN = tile[r.fam][1];
  r.tm = (M + r.TM - 1) / r.TM;
  r.tn = (N + r.TN - 1) / r.TN;
  // intra-block K split of the 128-tile kernels: waves not needed for M or
  // N <= 64 take K-ranges (the kernels split their waves by the same rule)
  r.kw = (r.fam == kF32_128 || r.fam == kBf16_128)
             ? 4 / ((M > 64 ? 2 : 1) * (N > 64 ? 2 : 1))
             : 1;
  // split-K when the output grid cannot fill the chip (wgrad shapes);
  // plain-C calls only (no epilogue) — fused-epilogue GEMMs have huge N.
  // Block target: enough tiles*SK to oversubscribe the 256 CUs (A/B-able
  // via CAFFE_SK_TARGET).  Round 2: 2048 re-measured BEST after the slim
  // tiles landed (RN50 1996 -> 2013, GoogLeNet 3223 -> 3248; 4096
  // regresses) — the slim wgrad grids have more, smaller tiles, so deeper
  // K-slicing now pays where it was neutral in round 1.
  static const long sk_target = [] {
    const char* e = getenv("CAFFE_SK_TARGET");
    return e ? atol(e) : 2048L;
  }();
  const long tiles = r.tm * r.tn;
  r.sk = 1;
  if (!has_epi && beta == 0.f && tiles < sk_target && K > 4 * BK) {
    r.sk = (int)std::min<long>(
        {sk_target / tiles + 1, (K + 4 * BK - 1) / (4 * BK), 256});
  }
  return r;
}

// ---- route trace: which kernel gemm() picked for a call, and with which
// views / epilogue.  Host-side only; off by default (one relaxed load per
// call), capped so a forgotten enable cannot grow without bound.
constexpr size_t kTraceCap = 4096;
static std::atomic<bool> g_trace_on{false};
static std::mutex g_trace_mu;
static std::vector<GemmRoute> g_trace_log;
// traced calls by operand reader: [0] staging cursors, [1] 64-bit reader
// (W64 fp32 kernels and every bf16 kernel)
static std::atomic<long> g_reader_calls[2];

static int view_kind(const GemmView* v) {  // 0 none, 1 chan, 2 im2col
  return !v || !v->spad ? 0 : (v->kh > 0 ? 2 : 1);
}

static void trace_route(GemmRoute r, const GemmEpi* epi, const GemmView* av,
                        const GemmView* bv) {
  r.av = (unsigned char)view_kind(av);
  r.bv = (unsigned char)view_kind(bv);
  const GemmView* iv = r.bv == 2 ? bv : (r.av == 2 ? av : nullptr);
  r.sh = iv ? iv->sh : 1;
  r.sw = iv ? iv->sw : 1;
  // 0 none, 1 plain, 2 NCHW scatter, 3 strided scatter
  r.epi = !epi ? 0 : (epi->spad <= 0 ? 1 : (epi->OWo > 0 ? 3 : 2));
  r.bias = !epi || !epi->bias ? 0 : (epi->bias_per_col ? 2 : 1);
  r.relu = epi && epi->relu;
  std::lock_guard<std::mutex> lk(g_trace_mu);
  if (g_trace_log.size() < kTraceCap) g_trace_log.push_back(r);
}

void gemm_trace(bool enable) {
  std::lock_guard<std::mutex> lk(g_trace_mu);
  if (enable) {
    g_trace_log.clear();
    g_trace_log.reserve(kTraceCap);
    g_reader_calls[0] = 0;
    g_reader_calls[1] = 0;
  }
  g_trace_on.store(enable, std::memory_order_relaxed);
}

void gemm_trace_readers(long* cursor, long* wide64) {
  *cursor = g_reader_calls[0].load();
  *wide64 = g_reader_calls[1].load();
}

long gemm_trace_read(char* buf, long cap) {
  static const char* const fam[] = {"slim32", "slim64", "f32_128",
                                    "bf16_128", "bf16_wide"};
  static const char* const view[] = {"none", "chan", "im2col"};
  static const char* const epi[] = {"none", "plain", "scatter", "sscatter"};
  static const char* const bias[] = {"none", "row", "col"};
  std::lock_guard<std::mutex> lk(g_trace_mu);
  long len = 0;
  if (cap > 0) buf[0] = 0;
  for (const GemmRoute& r : g_trace_log) {
    char line[256];
    const int n = snprintf(
        line, sizeof(line),
        "fam=%s ta=%d tb=%d sk=%d kw=%d M=%ld N=%ld K=%ld tm=%ld tn=%ld "
        "av=%s bv=%s sh=%d sw=%d epi=%s bias=%s relu=%d\n",
        fam[r.fam], r.ta, r.tb, r.sk, r.kw, r.M, r.N, r.K, r.tm, r.tn,
        view[r.av], view[r.bv], r.sh, r.sw, epi[r.epi], bias[r.bias],
        r.relu);
    if (len + n < cap) memcpy(buf + len, line, (size_t)n + 1);
    len += n;
  }
  return len;
}

// ---- limits of the 32-bit staging (gemm_common.hpp).  Row, column and K
// indices, a tile's overrun past the edge included, are fastdiv dividends
// and stay below 2^31; a viewed operand is addressed by a 32-bit byte
// offset from its base, so it holds at most 2^30 elements.
// CAFFE_GEMM_W64=1 sends every call to the 64-bit kernels (A/B and tests).
constexpr long kIdx32Max = kFastDivLimit - 4096;
static bool index32_ok(long M, long N, long K, const GemmEpi* epi) {
  static const bool force64 = [] {
    const char* e = getenv("CAFFE_GEMM_W64");
    return e && atoi(e) != 0;
  }();
  if (force64) return false;
  if (M > kIdx32Max || N > kIdx32Max || K > kIdx32Max) return false;
  return !(epi && epi->spad > 0 && epi->spad >= kFastDivLimit);
}
// fills the view's reciprocals and strides; false when it does not fit.
// axis: length of the GEMM axis the view's images lie along.
static bool fill_view32(GemmView& v, long axis) {
  if (!v.spad) return true;
  const long per_chan = v.kh > 0 ? (long)v.H * v.W : v.S;
  const long per_img = v.chan * per_chan;
  const long nimg = (axis + v.spad - 1) / v.spad;
  if (v.spad >= kFastDivLimit || nimg * per_img > (1L << 30)) return false;
  v.fd_spad = fastdiv_make((unsigned long)v.spad);
  v.img = (unsigned)per_img;
  v.hw = (unsigned)per_chan;
  if (v.kh > 0) {
    CHECK_GT_(v.kw, 0);
    CHECK_GT_(v.OW, 0);
    v.fd_ow = fastdiv_make((unsigned long)v.OW);
    v.fd_khkw = fastdiv_make((unsigned long)v.kh * v.kw);
    v.fd_kw = fastdiv_make((unsigned long)v.kw);
  }
  return true;
}

void gemm(hipStream_t s, bool transA, bool transB, long M, long N, long K,
          float alpha, const float* A, long lda, const float* B, long ldb,
          float beta, float* C, long ldc, const GemmEpi* epi,
          const GemmView* aview, const GemmView* bview) {
  CHECK_GT_(M, 0);
  CHECK_GT_(N, 0);
  CHECK_GT_(K, 0);
  CHECK_(!(aview && transA)) << "A view requires no transpose";
  CHECK_(!(transA && transB)) << "transA && transB has no kernel";
  GemmArgs g{};
  g.A = A;
  g.B = B;
  g.C = C;
  g.M = M;
  g.N = N;
  g.K = K;
  g.lda = lda;
  g.ldb = ldb;
  g.ldc = ldc;
  g.alpha = alpha;
  g.beta = beta;
  if (epi) {
    g.spad = epi->spad;
    g.S = epi->S;
    g.n_stride = epi->n_stride;
    g.bias = epi->bias;
    g.bias_per_col = epi->bias_per_col;
    g.relu = epi->relu;
    g.Srow = epi->Srow > 0 ? epi->Srow : epi->S;
    g.OWo = epi->OWo;
    g.osh = epi->osh;
    g.osw = epi->osw;
    g.Wd = epi->Wd;
  }
  if (aview) g.av = *aview;
  if (bview) g.bv = *bview;
  // 32-bit staging (the cursor kernels): for calls whose B is a view, when
  // every index the kernels decompose and every viewed operand's byte
  // offset fit.  Every other call goes to the W64 kernels, which are the
  // 64-bit reader and epilogue division unchanged: sizes past the limits,
  // and calls with a plain B (IP layers, explicit-col convs — wgrad with a
  // dY view as A included), whose plain path measured 6-10 % slower next to
  // the cursor code.  A's image axis is K (views need
  // !transA), B's is K when transposed, N otherwise.
  bool w64 = !bview || !index32_ok(M, N, K, epi);
  if (!w64 && aview && !fill_view32(g.av, K)) w64 = true;
  if (!w64 && !fill_view32(g.bv, transB ? K : N)) w64 = true;
  if (!w64 && epi && epi->spad > 0) {
    g.fd_spad = fastdiv_make((unsigned long)epi->spad);
    if (epi->OWo > 0) g.fd_owo = fastdiv_make((unsigned long)epi->OWo);
  }
  const GemmRoute r = pick_route(M, N, K, transA, transB, epi != nullptr,
                                 beta, Engine::get().gemm_bf16);
  g.tn = r.tn;
  g.tiles = r.tm * r.tn;
  const bool bf16_fam = r.fam == kBf16_128 || r.fam == kBf16Wide;
  if (g_trace_on.load(std::memory_order_relaxed)) {
    trace_route(r, epi, aview, bview);
    g_reader_calls[w64 || bf16_fam].fetch_add(1, std::memory_order_relaxed);
  }

  // ("gemm_tt" has no kernel any more; the class stays registered so perf
  // reports keep their four gemm lines)
  static const char* const pcls[] = {"gemm_nn", "gemm_nt", "gemm_tn",
                                     "gemm_tt"};
  const int cls = transA ? 2 : (transB ? 1 : 0);
  static const bool by_shape = getenv("CAFFE_GEMM_BY_SHAPE") != nullptr;
  PerfClass* pc;
  if (by_shape) {
    pc = &Engine::get().perf(std::string(pcls[cls]) + "_" +
                             std::to_string(M) + "x" + std::to_string(N) +
                             "x" + std::to_string(K));
  } else {
    static PerfClass* const classes[] = {&Engine::get().perf(pcls[0]),
                                         &Engine::get().perf(pcls[1]),
                                         &Engine::get().perf(pcls[2]),
                                         &Engine::get().perf(pcls[3])};
    pc = classes[cls];
  }
  PerfScope perf(pc, s, 2.0 * M * N * K,
                 4.0 * (M * K + N * K + M * N));

  if (r.sk > 1) {  // split-K: partial slabs, then the fixed-order reduce
    g.slab = (float*)Workspace::get_global().get(
        Workspace::kSplitK, sizeof(float) * (size_t)r.sk * M * N);
    g.SK = r.sk;
  }
  const dim3 grid((unsigned)g.tiles, 1, (unsigned)r.sk);
  if (bf16_fam) {
    gemm_launch_bf16(s, transA, transB, grid, g, r.sk > 1,
                     r.fam == kBf16Wide);
  } else {
    with_gemm_variant(
        transA, transB, r.sk > 1, [&](auto ta, auto tb, auto sk) {
          constexpr bool TA = decltype(ta)::value, TB = decltype(tb)::value,
                         SPLITK = decltype(sk)::value;
          auto launch = [&](auto wide) {
            constexpr bool W64 = decltype(wide)::value;
            if (r.fam == kSlim32)
              hipLaunchKernelGGL((k_gemm_slim<TA, TB, 32, SPLITK, W64>),
                                 grid, dim3(256), 0, s, g);
            else if (r.fam == kSlim64)
              hipLaunchKernelGGL((k_gemm_slim<TA, TB, 64, SPLITK, W64>),
                                 grid, dim3(256), 0, s, g);
            else
              hipLaunchKernelGGL((k_gemm_f32<TA, TB, SPLITK, W64>), grid,
                                 dim3(256), 0, s, g);
          };
          if (w64)
            launch(std::true_type{});
          else
            launch(std::false_type{});
        });
  }
  if (r.sk > 1) launch_splitk_reduce(s, g.slab, M * N, r.sk, C);
}

// Wt[g*Cin_g + ci][co_local*kh*kw + ki*kw + kj] =
//   W[g*Coutg + co_local][ci][kh-1-ki][kw-1-kj]
__global__ void k_weight_flip(const float* __restrict__ w, int Cout,
                              int Cin_g, int kh, int kw, int groups,
                              float* __restrict__ wt) {
  const int Coutg = Cout / groups;
  const long total = (long)Cout * Cin_g * kh * kw;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    // destination indexing: [g][ci][co_local][ki][kj]
    long rem = i;
    const int kj = (int)(rem % kw);
    rem /= kw;
    const int ki = (int)(rem % kh);
    rem /= kh;
    const int co_l = (int)(rem % Coutg);
    rem /= Coutg;
    const int ci = (int)(rem % Cin_g);
    const int g = (int)(rem / Cin_g);
    wt[i] = w[((((long)(g * Coutg + co_l) * Cin_g + ci) * kh +
               (kh - 1 - ki)) * kw) + (kw - 1 - kj)];
  }
}
void weight_flip_grouped(hipStream_t s, const float* w, int Cout, int Cin_g,
                         int kh, int kw, int groups, float* wt) {
  const long total = (long)Cout * Cin_g * kh * kw;
  hipLaunchKernelGGL(k_weight_flip, dim3((int)std::min<long>((total + 255) / 256, 2048)),
                     dim3(256), 0, s, w, Cout, Cin_g, kh, kw, groups, wt);
}

// db[c] = Σ_n Σ_s dy[n][c][s] — image-sliced partials + fixed-order sum
__global__ void k_bias_grad_part(const float* __restrict__ dy, int N, int C,
                                 int S, int nb, double* __restrict__ part) {
  const int c = blockIdx.x % C;
  const int slice = blockIdx.x / C;
  const int n0 = (int)((long)N * slice / nb);
  const int n1 = (int)((long)N * (slice + 1) / nb);
  const int span = (n1 - n0) * S;
  const int B = blockDim.x;
  auto addr = [&](int i) {
    const int n = n0 + i / S;
    return ((long)n * C + c) * S + (i - (n - n0) * S);
  };
  double acc = 0, acc2 = 0;
  int i = threadIdx.x;
  for (; i + 3 * B < span; i += 4 * B) {  // 4 loads in flight (MLP)
    const float v0 = dy[addr(i)], v1 = dy[addr(i + B)];
    const float v2 = dy[addr(i + 2 * B)], v3 = dy[addr(i + 3 * B)];
    acc += (double)v0 + v1;
    acc2 += (double)v2 + v3;
  }
  for (; i < span; i += B) acc += dy[addr(i)];
  acc += acc2;
  __shared__ double sh[256];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(long)c * nb + slice] = sh[0];
}
__global__ void k_bias_grad_fin(const double* __restrict__ part, int nb,
                                int C, float* __restrict__ db) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < C;
       c += gridDim.x * blockDim.x) {
    double acc = 0;
    for (int b = 0; b < nb; ++b) acc += part[(long)c * nb + b];
    db[c] = (float)acc;
  }
}
void bias_grad(hipStream_t s, const float* dy, int N, int C, long S,
               float* db) {
  PerfScope perf(PERF_CLASS("reduce"), s, 0, 4.0 * N * C * S);
  const int nb = std::max(1, std::min(N, 2048 / std::max(1, C)));
  double* part = (double*)Workspace::get_global().get(
      Workspace::kBiasPart, sizeof(double) * (size_t)C * nb);
  hipLaunchKernelGGL(k_bias_grad_part, dim3(C * nb), dim3(256), 0, s, dy, N,
                     C, (int)S, nb, part);
  hipLaunchKernelGGL(k_bias_grad_fin, dim3(1), dim3(256), 0, s, part, nb, C,
                     db);
}

}  // namespace gpu
}  // namespace camd
