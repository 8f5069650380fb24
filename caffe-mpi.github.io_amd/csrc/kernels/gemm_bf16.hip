// gemm_bf16.hip — bf16 tensor-core GEMM for gfx950 (CDNA4):
// `v_mfma_f32_32x32x16_bf16` (≈2.52 PF dense chip peak, 16x the fp32 MFMA
// rate) with fp32 accumulation and FP32 STORAGE everywhere — the staging
// pass reads the same fp32 tensors as the fp32 kernel (plain, channel-view
// or implicit-im2col-view operands, strides included) and converts to
// bf16 in-register on the way into LDS.  This is the MI355X-native
// mixed-precision contract (AMP semantics): conv/IP contractions compute
// in bf16, every other op, the master weights, the gradients'
// accumulation and the solver stay fp32.  The reference's analog is the
// NVCaffe Ftype/Btype fp16 machinery (net.cpp:100-156, type.hpp:13-47)
// whose headline was pseudo-fp16 (fp16 storage, fp32 math,
// models/bvlc_alexnet/logs/alexnet_pfp16.log); on CDNA4 the win is in the
// matrix unit, not storage, so the design inverts: storage fp32,
// multiply bf16.
//
// Structure mirrors k_gemm_f32 (the measured-best register pipeline, 2
// blocks/CU): 128x128 tile, 4 waves, 2x2 accs of 32x32, BK=64 (4 MFMA
// k-steps of 16), double-buffered LDS, T14 issue-early/write-late, one
// barrier per K-tile, kwaves intra-block split for M<=64 / N<=64 tiles,
// deterministic split-K with fp32 slabs.
//
// LDS layout (paired-k): element (row r, k) of a ROWS-row tile lives at
// bf16 slot
//   (k>>1)*PS + 2*r + (k&1),  PS = 2*ROWS + 2
// so the MFMA fragment (r fixed, 8 consecutive k) is 4 conflict-free b32
// reads (consecutive lanes -> consecutive words; the +1-word pad per
// pair-row staggers banks for the k-contiguous staging writes).
#include "gemm_common.hpp"

namespace camd {
namespace gpu {

namespace bf16gemm {

using bf16 = __bf16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

constexpr int BK = 64;
// operand image of a ROWS-row tile (128, or 256 for the wide kernel)
template <int ROWS>
constexpr int PSTR = 2 * ROWS + 2;  // bf16 per pair-row (+1 word pad)
template <int ROWS>
constexpr int OPSZ = (BK / 2) * PSTR<ROWS>;  // bf16 per operand image

// ---- staging: fp32 read16 -> bf16 convert -> LDS scatter.  These kernels
// keep the 64-bit reader read16() and the 64-bit epilogue division
// (store_acc<SPLITK, true>), not the fp32 kernels' staging cursors: they sit
// at 256 VGPRs and spill more with the cursors.
// row-contiguous source (thread holds (r, k0..k0+15)): paired b32 writes
template <int PS>
__device__ __forceinline__ void write_rowk(bf16* img, int r, int k0,
                                           const float (&v)[16]) {
#pragma unroll
  for (int j = 0; j < 16; j += 2) {
    bf16x2 p;
    p[0] = (bf16)v[j];
    p[1] = (bf16)v[j + 1];
    *(bf16x2*)&img[((k0 + j) >> 1) * PS + 2 * r] = p;
  }
}
// k-contiguous source (thread holds (k, n0..n0+15)): u16 scatter (2-way
// word sharing across the k-pair lanes — bank-staggered by the pad)
template <int PS>
__device__ __forceinline__ void write_kn(bf16* img, int k, int n0,
                                         const float (&v)[16]) {
  bf16* base = img + (k >> 1) * PS + (k & 1);
#pragma unroll
  for (int j = 0; j < 16; ++j) base[2 * (n0 + j)] = (bf16)v[j];
}

// One ROWS x BK operand tile, staged by 2*ROWS threads with two 16-float
// chunks each (A rows are the M axis, B rows the N axis).  KCONTIG: the
// operand is stored [row][K], contiguous along K — A when !TA, B when TB —
// and a thread holds (row t % ROWS, 32 k); otherwise it is stored
// [K][row] and a thread holds (k t & 63, 32 rows).
template <int ROWS, bool KCONTIG>
__device__ __forceinline__ void stage_load(const float* P, long r0, long k0,
                                           long ld, long R, long K,
                                           const GemmView& v,
                                           float (&r)[16],
                                           float (&r2)[16]) {
  constexpr int LOG2 = ROWS == 128 ? 7 : 8;
  static_assert(ROWS == 1 << LOG2, "128- or 256-row tile");
  const int t = threadIdx.x;
  if (KCONTIG) {
    read16(P, r0 + (t & (ROWS - 1)), k0 + (t >> LOG2) * 32, ld, R, K, v, r);
    read16(P, r0 + (t & (ROWS - 1)), k0 + (t >> LOG2) * 32 + 16, ld, R, K,
           v, r2);
  } else {
    read16(P, k0 + (t & 63), r0 + (t >> 6) * 32, ld, K, R, v, r);
    read16(P, k0 + (t & 63), r0 + (t >> 6) * 32 + 16, ld, K, R, v, r2);
  }
}
template <int ROWS, bool KCONTIG>
__device__ __forceinline__ void stage_write(bf16* S, const float (&r)[16],
                                            const float (&r2)[16]) {
  constexpr int LOG2 = ROWS == 128 ? 7 : 8;
  const int t = threadIdx.x;
  if (KCONTIG) {
    write_rowk<PSTR<ROWS>>(S, t & (ROWS - 1), (t >> LOG2) * 32, r);
    write_rowk<PSTR<ROWS>>(S, t & (ROWS - 1), (t >> LOG2) * 32 + 16, r2);
  } else {
    write_kn<PSTR<ROWS>>(S, t & 63, (t >> 6) * 32, r);
    write_kn<PSTR<ROWS>>(S, t & 63, (t >> 6) * 32 + 16, r2);
  }
}
// both operands of a ROWS x ROWS block tile at K offset k0.  (Functions,
// not lambdas of the kernels: closures over the staging registers made the
// register allocator spill more in these kernels, which sit at 256 VGPRs.)
template <int ROWS, bool TA, bool TB>
__device__ __forceinline__ void load_tile(const GemmArgs& g, long m0,
                                          long n0, long k0, float (&a)[16],
                                          float (&a2)[16], float (&b)[16],
                                          float (&b2)[16]) {
  stage_load<ROWS, !TA>(g.A, m0, k0, g.lda, g.M, g.K, g.av, a, a2);
  stage_load<ROWS, TB>(g.B, n0, k0, g.ldb, g.N, g.K, g.bv, b, b2);
}
template <int ROWS, bool TA, bool TB>
__device__ __forceinline__ void write_tile(bf16* As, bf16* Bs,
                                           const float (&a)[16],
                                           const float (&a2)[16],
                                           const float (&b)[16],
                                           const float (&b2)[16]) {
  stage_write<ROWS, !TA>(As, a, a2);
  stage_write<ROWS, TB>(Bs, b, b2);
}

// fragment: (r, ksel*8 + 0..7) as 4 b32 reads
template <int PS>
__device__ __forceinline__ bf16x8 frag(const bf16* img, int r, int kbase) {
  bf16x8 a;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bf16x2 p =
        *(const bf16x2*)&img[((kbase + 2 * i) >> 1) * PS + 2 * r];
    a[2 * i] = p[0];
    a[2 * i + 1] = p[1];
  }
  return a;
}

template <bool TA, bool TB, bool SPLITK>
__launch_bounds__(256, 2) __global__ void k_gemm_bf16(GemmArgs g) {
  constexpr int T = 128, PS = PSTR<T>;  // tile rows = cols
  __shared__ bf16 smem[4 * OPSZ<T>];
  auto As = [&](int buf) -> bf16* { return smem + buf * OPSZ<T>; };
  auto Bs = [&](int buf) -> bf16* { return smem + (2 + buf) * OPSZ<T>; };

  long tile_m, tile_n;
  tile_origin(g, tile_m, tile_n);
  const long m0 = tile_m * T, n0 = tile_n * T;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int mwaves = g.M > 64 ? 2 : 1;
  const int nwaves = g.N > 64 ? 2 : 1;
  const int mn = mwaves * nwaves;
  const int kwaves = 4 / mn;
  const int wr = wave % mwaves;
  const int wc = (wave / mwaves) % nwaves;
  const int wk = wave / mn;
  const int row_in = lane & 31;
  const int ksel = lane >> 5;  // which 8-deep half of the 16-k step

  long k_lo = 0, k_hi = g.K;
  if (SPLITK && !splitk_range<BK>(g, k_lo, k_hi)) return;
  const long ntiles = (k_hi - k_lo + BK - 1) / BK;

  f32x16 acc00 = {}, acc01 = {}, acc10 = {}, acc11 = {};
  float ra[16], ra2[16], rb[16], rb2[16];

  // K-step kk (16 deep) of one staged tile into the wave's 2x2
  // accumulators; the kk loops stay at the call sites (unrolled over
  // compile-time bounds in the plain loop, rolled in the K-waves loop)
  auto mfma_2x2 = [&](const bf16* Ab, const bf16* Bb, int kk) {
    const int kbase = kk + ksel * 8;
    const bf16x8 a0 = frag<PS>(Ab, wr * 64 + row_in, kbase);
    const bf16x8 a1 = frag<PS>(Ab, wr * 64 + 32 + row_in, kbase);
    const bf16x8 b0 = frag<PS>(Bb, wc * 64 + row_in, kbase);
    const bf16x8 b1 = frag<PS>(Bb, wc * 64 + 32 + row_in, kbase);
    acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc00, 0, 0, 0);
    acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc01, 0, 0, 0);
    acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc10, 0, 0, 0);
    acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc11, 0, 0, 0);
  };

  load_tile<T, TA, TB>(g, m0, n0, k_lo, ra, ra2, rb, rb2);
  write_tile<T, TA, TB>(As(0), Bs(0), ra, ra2, rb, rb2);
  __syncthreads();

  if (kwaves == 1) {
    int cur = 0;
    for (long t = 0; t < ntiles; ++t) {
      if (t + 1 < ntiles)  // issue next tile's global loads early (T14)
        load_tile<T, TA, TB>(g, m0, n0, k_lo + (t + 1) * BK, ra, ra2, rb,
                             rb2);
#pragma unroll
      for (int kk = 0; kk < BK; kk += 16) mfma_2x2(As(cur), Bs(cur), kk);
      if (t + 1 < ntiles)
        write_tile<T, TA, TB>(As(cur ^ 1), Bs(cur ^ 1), ra, ra2, rb, rb2);
      __syncthreads();
      cur ^= 1;
    }
  } else {
    // kwaves path: both buffers live per iteration (small-M/N tiles keep
    // all 4 waves computing); kwaves==4 splits the 64-deep step in half
    const int grp = wk & 1;
    const int khalf = wk >> 1;
    const int kk0 = (kwaves == 4) ? khalf * (BK / 2) : 0;
    const int kk1 = (kwaves == 4) ? kk0 + BK / 2 : BK;
    if (1 < ntiles) {
      load_tile<T, TA, TB>(g, m0, n0, k_lo + BK, ra, ra2, rb, rb2);
      write_tile<T, TA, TB>(As(1), Bs(1), ra, ra2, rb, rb2);
    }
    __syncthreads();
    for (long p = 0; p < ntiles; p += 2) {
      const long t_next0 = p + 2, t_next1 = p + 3;
      if (t_next0 < ntiles)
        load_tile<T, TA, TB>(g, m0, n0, k_lo + t_next0 * BK, ra, ra2, rb,
                             rb2);
      float sa[16], sa2[16], sb[16], sb2[16];
      if (t_next1 < ntiles)
        load_tile<T, TA, TB>(g, m0, n0, k_lo + t_next1 * BK, sa, sa2, sb,
                             sb2);
      if (p + grp < ntiles) {
        for (int kk = kk0; kk < kk1; kk += 16)
          mfma_2x2(As(grp), Bs(grp), kk);
      }
      __syncthreads();
      if (t_next0 < ntiles)
        write_tile<T, TA, TB>(As(0), Bs(0), ra, ra2, rb, rb2);
      if (t_next1 < ntiles)
        write_tile<T, TA, TB>(As(1), Bs(1), sa, sa2, sb, sb2);
      __syncthreads();
    }
  }
  // (the bf16 arena is byte-compatible scratch for the fp32 partials)
  if (kwaves > 1 &&
      !kwaves_combine((float*)smem, lane, wave, wk, wc * mwaves + wr, mn,
                      kwaves, acc00, acc01, acc10, acc11))
    return;

  // This kernel sits at 256 VGPRs and the form of the epilogue call decides
  // where its spills land: only this one (a by-reference lambda that tests
  // its column before store_acc does) keeps them out of the K-loop, as in
  // the inline epilogue it replaces ("GEMM helper forms").
  auto store = [&](const f32x16& a, int ti, int tj) {
    const long col = n0 + wc * 64 + tj * 32 + row_in;
    if (col >= g.N) return;
    store_acc<SPLITK, true>(g, a, m0 + wr * 64 + ti * 32, col, ksel);
  };
  store(acc00, 0, 0);
  store(acc01, 0, 1);
  store(acc10, 1, 0);
  store(acc11, 1, 1);
}

// ---------------------------------------------------------------
// Wide 256x256 tile (round 2): the 128^2 bf16 kernel is STAGING-bound —
// the 16x MFMA rate moved GEMM time only ~13% — so quadruple the MACs
// per staged byte.  512 threads = 8 waves as 4(M) x 2(N), each wave a
// 64(M) x 128(N) sub-tile of 2x4 32x32 accumulators (128 acc VGPRs);
// LDS 2 x (A 256 + B 256 rows) paired-k images = 131.6 KB -> 1 block/CU
// (2 waves/SIMD, same as the 128^2 variant, at half the staging per MAC).
// Dispatched for M > 128 && N > 128; edges masked as usual.
template <bool TA, bool TB, bool SPLITK>
__launch_bounds__(512, 1) __global__ void k_gemm_bf16_wide(GemmArgs g) {
  constexpr int T = 256, PS = PSTR<T>;  // tile rows = cols
  __shared__ bf16 smem[4 * OPSZ<T>];
  auto As = [&](int buf) -> bf16* { return smem + buf * OPSZ<T>; };
  auto Bs = [&](int buf) -> bf16* { return smem + (2 + buf) * OPSZ<T>; };

  long tile_m, tile_n;
  tile_origin(g, tile_m, tile_n);
  const long m0 = tile_m * T, n0 = tile_n * T;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = wave & 3;        // 4 row blocks of 64
  const int wc = wave >> 2;       // 2 col blocks of 128
  const int row_in = lane & 31;
  const int ksel = lane >> 5;

  long k_lo = 0, k_hi = g.K;
  if (SPLITK && !splitk_range<BK>(g, k_lo, k_hi)) return;
  const long ntiles = (k_hi - k_lo + BK - 1) / BK;

  f32x16 acc[2][4] = {};
  float ra[16], ra2[16], rb[16], rb2[16];

  load_tile<T, TA, TB>(g, m0, n0, k_lo, ra, ra2, rb, rb2);
  write_tile<T, TA, TB>(As(0), Bs(0), ra, ra2, rb, rb2);
  __syncthreads();

  int cur = 0;
  for (long tt = 0; tt < ntiles; ++tt) {
    if (tt + 1 < ntiles)
      load_tile<T, TA, TB>(g, m0, n0, k_lo + (tt + 1) * BK, ra, ra2, rb,
                           rb2);
    {
      const bf16* Ab = As(cur);
      const bf16* Bb = Bs(cur);
#pragma unroll
      for (int kk = 0; kk < BK; kk += 16) {
        const int kbase = kk + ksel * 8;
        const bf16x8 a0 = frag<PS>(Ab, wr * 64 + row_in, kbase);
        const bf16x8 a1 = frag<PS>(Ab, wr * 64 + 32 + row_in, kbase);
        bf16x8 b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          b[j] = frag<PS>(Bb, wc * 128 + 32 * j + row_in, kbase);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              a0, b[j], acc[0][j], 0, 0, 0);
          acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              a1, b[j], acc[1][j], 0, 0, 0);
        }
      }
    }
    if (tt + 1 < ntiles)
      write_tile<T, TA, TB>(As(cur ^ 1), Bs(cur ^ 1), ra, ra2, rb, rb2);
    __syncthreads();
    cur ^= 1;
  }

#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
      store_acc<SPLITK, true>(g, acc[ti][tj], m0 + wr * 64 + ti * 32,
                              n0 + wc * 128 + tj * 32 + row_in, ksel);
}

}  // namespace bf16gemm

// launcher used by gemm() in gemm_f32.hip when bf16 compute is enabled;
// `wide` selects the 256x256-tile kernel (grid must be 256-tile-based)
void gemm_launch_bf16(hipStream_t s, bool transA, bool transB, dim3 grid,
                      const GemmArgs& g, bool splitk, bool wide) {
  using namespace bf16gemm;
  with_gemm_variant(transA, transB, splitk, [&](auto ta, auto tb, auto sk) {
    constexpr bool TA = decltype(ta)::value, TB = decltype(tb)::value,
                   SPLITK = decltype(sk)::value;
    if (wide)
      hipLaunchKernelGGL((k_gemm_bf16_wide<TA, TB, SPLITK>), grid, dim3(512),
                         0, s, g);
    else
      hipLaunchKernelGGL((k_gemm_bf16<TA, TB, SPLITK>), grid, dim3(256), 0,
                         s, g);
  });
}

}  // namespace gpu
}  // namespace camd
