// math.hpp — CPU math for the engine's CPU mode and launcher declarations
// for the hand-written gfx950 HIP kernels (implemented in kernels/*.hip).
// Replaces the reference's util/math_functions.{cpp,cu} + util/im2col.* —
// note we deliberately do NOT reproduce the reference's per-call stream
// synchronization (math_functions.cu:26); all launches are async on the
// caller's stream.
#pragma once

#include <cmath>

#include "core.hpp"

namespace camd {

// ------------------------------------------------------------- CPU math
namespace cpu {
// Row-major C[M][N] = alpha*op(A)*op(B) + beta*C (fp32 accumulation, blocked)
void gemm(bool transA, bool transB, long M, long N, long K, float alpha,
          const float* A, const float* B, float beta, float* C);
void axpy(long n, float a, const float* x, float* y);
void axpby(long n, float a, const float* x, float b, float* y);
void scal(long n, float a, float* x);
void im2col(const float* im, int C, int H, int W, int kh, int kw, int ph,
            int pw, int sh, int sw, int dh, int dw, float* col);
void col2im(const float* col, int C, int H, int W, int kh, int kw, int ph,
            int pw, int sh, int sw, int dh, int dw, float* im);
}  // namespace cpu

inline int conv_out_dim(int in, int k, int pad, int stride, int dil) {
  return (in + 2 * pad - (dil * (k - 1) + 1)) / stride + 1;
}
void pool_out_dim(int H, int W, int kh, int kw, int ph, int pw, int sh,
                  int sw, int* OH, int* OW);  // ceil + clip, pooling_layer.cpp:86

// ------------------------------------------------------ solver update rules
// The reference's six solver types (solvers/*_solver.{cpp,cu}; registry names
// SGD, Nesterov, AdaGrad, RMSProp, AdaDelta, Adam).  One per-element function
// serves the CPU loops (solver.cpp) and the GPU kernel (k_solver_seg), so the
// two modes cannot drift apart.
enum SolverRule {
  kRuleSgd = 0, kRuleNesterov, kRuleAdaGrad, kRuleRmsProp, kRuleAdaDelta,
  kRuleAdam, kNumSolverRules
};
inline int solver_rule_slots(int rule) {
  return rule == kRuleAdaDelta || rule == kRuleAdam ? 2 : 1;
}
// per-iteration coefficients, passed by value as kernel arguments; lr and
// decay are the solver-wide values (per-param multipliers come from tables)
struct SolverCoef {
  float mom;     // momentum (Adam: beta1)
  float lr;      // cur lr (Adam: times the bias correction of this iteration)
  float decay;   // weight_decay
  float gscale;  // 1 / (world * iter_size), applied before any square
  float aux;     // RMSProp: rms_decay; Adam: momentum2 (beta2)
  float delta;   // the rule's clamped delta (0 where the rule has none)
};

#if defined(__HIPCC__) || defined(__HIP__)
#define CAMD_HD __host__ __device__
#else
#define CAMD_HD
#endif
// One element of one rule: reads the raw reduced gradient g and the weight
// w, updates the history slot(s) in place and returns the value to subtract
// from w.  lr and decay already carry the param's multipliers.
template <int Rule, bool kL1>
CAMD_HD inline float solver_rule_step(float g, float w, float& h, float& h2,
                                      const SolverCoef& c, float lr,
                                      float decay) {
  const float reg = kL1 ? (float)((0.f < w) - (w < 0.f)) : w;
  const float gr = g * c.gscale + reg * decay;
  if (Rule == kRuleSgd) {
    h = c.mom * h + lr * gr;
    return h;
  } else if (Rule == kRuleNesterov) {
    const float h0 = h;
    h = c.mom * h0 + lr * gr;
    return (1.f + c.mom) * h - c.mom * h0;
  } else if (Rule == kRuleAdaGrad) {
    h += gr * gr;
    return lr * gr / (sqrtf(h) + c.delta);
  } else if (Rule == kRuleRmsProp) {
    h = c.aux * h + (1.f - c.aux) * gr * gr;
    return lr * gr / (sqrtf(h) + c.delta);
  } else if (Rule == kRuleAdaDelta) {
    h = c.mom * h + (1.f - c.mom) * gr * gr;
    const float u = gr * sqrtf((h2 + c.delta) / (h + c.delta));
    h2 = c.mom * h2 + (1.f - c.mom) * u * u;
    return lr * u;
  } else {  // kRuleAdam: h = m, h2 = v
    h = c.mom * h + (1.f - c.mom) * gr;
    h2 = c.aux * h2 + (1.f - c.aux) * gr * gr;
    return lr * h / (sqrtf(h2) + c.delta);
  }
}

// clip_gradients (caffe.proto:241-243; the order of SGDSolver::ApplyUpdate,
// sgd_solver.cpp:102-128: clip, then normalise, regularise, rule).  norm is
// the global L2 norm of the reduced gradient over world, rounded once to
// float.  Written as this comparison: a NaN norm does not clip, and
// clip == 0 zeroes the gradient unless the norm is 0.  The factor multiplies
// SolverCoef::gscale; one function serves the host (CPU mode) and
// k_clip_final.
CAMD_HD inline float clip_factor(float norm, float clip) {
  return norm > clip ? clip / norm : 1.0f;
}

// ------------------------------------------------- sigmoid and its losses
// Per-element formulas of the reference's sigmoid_layer.cpp:10 and
// sigmoid_cross_entropy_loss_layer.cpp:41-44.  As with the solver rules, one
// function serves the CPU loops and the GPU kernels.  expf / logf are the
// IEEE library forms: a NaN input stays NaN, exp overflow gives inf, so the
// sigmoid saturates to exactly 0 or 1 and never produces NaN for finite x.
// log(1 + exp(.)) is written as the reference writes it, not as log1pf: on
// gfx950 log1pf made the loss forward 2.5x slower than HBM allows
// (profiles/sigmoid_loss_kernels.txt), and the argument of the log is in
// [1, 2], where the plain form is off by at most one float rounding of it.
CAMD_HD inline float sigmoid_value(float x) {
  return 1.f / (1.f + expf(-x));
}
// the term the cross-entropy loss SUMS (already negated):
// -(x*(t - [x>=0]) - log(1 + exp(x - 2x*[x>=0])))
CAMD_HD inline float sigmoid_ce_term(float x, float t) {
  const float pos = x >= 0.f ? 1.f : 0.f;
  return logf(1.f + expf(x - 2.f * x * pos)) - x * (t - pos);
}

// -------------------------------------------------------- contrastive loss
// Per-row formulas of the reference's contrastive_loss_layer.cpp:45-58 and
// :86-105, shared by the CPU loops and the GPU kernels.  dsq is the row's
// Σ (a - b)².  sqrtf is the IEEE form and the clamps are written as
// comparisons (not fmaxf, which drops a NaN operand), so both modes take
// the same branch and a NaN row gives a NaN loss.
CAMD_HD inline float contrastive_row_loss(float dsq, bool similar,
                                          float margin, bool legacy) {
  if (similar) return dsq;
  if (legacy) {
    const float m = margin - dsq;
    return m < 0.f ? 0.f : m;
  }
  const float m = margin - sqrtf(dsq);
  return m < 0.f ? 0.f : m * m;
}
// the factor of (a - b) in the row's gradient, alpha = sign * loss_weight / N
// (0 for a dissimilar row at or outside the margin)
CAMD_HD inline float contrastive_row_beta(float dsq, bool similar,
                                          float margin, bool legacy,
                                          float alpha) {
  if (similar) return alpha;
  if (legacy) return margin - dsq > 0.f ? -alpha : 0.f;
  const float d = sqrtf(dsq);
  const float mdist = margin - d;
  return mdist > 0.f ? -alpha * mdist / (d + 1e-4f) : 0.f;
}

// --------------------------------------------------------- exact fast division
// n / d for 0 <= n < 2^31 and 1 <= d <= 2^31 as multiply-high, add and shift
// (Granlund & Montgomery's round-up form: with l = ceil(log2 d) and
// M = ceil(2^(32+l) / d) in [2^32, 2^33), n / d == (n * M) >> (32 + l)
// whenever n * (M*d - 2^(32+l)) < 2^(32+l), which n < 2^31 guarantees; mul
// holds M - 2^32, and mulhi(n, mul) + n cannot overflow below 2^31).  The
// magic is computed on the host; the default divides by 1.  The GEMM
// staging and epilogue decompose their view indices with it.
constexpr long kFastDivLimit = 1L << 31;  // dividends and divisors
struct FastDiv {
  unsigned mul = 0, sh = 0;
};
inline FastDiv fastdiv_make(unsigned long d) {
  FastDiv f;
  while ((1ul << f.sh) < d) ++f.sh;
  f.mul = (unsigned)((((1ul << (32 + f.sh)) + d - 1) / d) - (1ul << 32));
  return f;
}
CAMD_HD inline unsigned fastdiv(unsigned n, FastDiv f) {
  return ((unsigned)(((unsigned long long)n * f.mul) >> 32) + n) >> f.sh;
}

// ------------------------------------------------------------ GPU launchers
namespace gpu {

// Epilogue for the MFMA GEMM (bias/ReLU fusion + the conv NCHW scatter that
// replaces a separate bias/copy pass).
struct GemmEpi {
  // when spad > 0: C column c maps to image n = c / spad, pixel s = c % spad;
  // columns with s >= S are padding and are dropped; output element is
  // C[n * n_stride + row * S + s] (NCHW scatter; the caller pre-offsets C by
  // the group's channel base and passes n_stride = Cout_total * S).
  long spad = 0;
  long S = 0;
  long n_stride = 0;
  const float* bias = nullptr;
  bool bias_per_col = false;  // IP: bias indexed by column, conv: by row
  bool relu = false;
  // strided scatter (1x1/s2 dgrad without a col2im pass): column pixel
  // sp -> (oh, ow) over OWo maps to destination pixel oh*osh*Wd + ow*osw;
  // per-row stride is Srow (= dest H*W).  OWo == 0 -> plain NCHW scatter.
  long Srow = 0;
  int OWo = 0, osh = 1, osw = 1, Wd = 0;
};

// NCHW-view operand: the GEMM axis that is contiguous in the stored tensor
// is an image axis q = n*spad + sp (sp < S valid, rest padding); element
// (r, q) lives at base[(n*chan + r)*S + sp].  Lets conv GEMMs read x / dY
// straight out of NCHW with no transpose/materialization pass.
//
// With kh > 0 the view becomes an IMPLICIT-IM2COL view (the north_star's
// implicit-GEMM conv): r indexes a col row (c, ki, kj), sp an output pixel
// (oh, ow); the element is x[n][c][oh*sh-ph+ki][ow*sw-pw+kj] (0 outside) —
// the col matrix is never materialized.  Strides live in the view (sh, sw);
// dilation is 1 only — dilated convs use the explicit col path.  Which
// convs take a view is the conv plan's decision (layers_gpu.cpp).
struct GemmView {
  long spad = 0;  // 0 = plain operand
  long S = 0;     // valid pixels per image (OH*OW)
  long chan = 0;  // channels of the viewed tensor (address stride term)
  int kh = 0, kw = 0, ph = 0, pw = 0;  // kh>0 => implicit im2col
  int H = 0, W = 0, OW = 0;            // input dims / output row width
  int sh = 1, sw = 1;  // conv strides (round 2: strided implicit im2col —
                       // conv1 7x7s2, the 1x1s2 projections, AlexNet s4)
  // 32-bit staging (filled by gemm(), never by the caller): magics of the
  // divisors the staging decomposes by, and the per-image / per-channel
  // element strides it would otherwise multiply out per element
  FastDiv fd_spad, fd_ow, fd_khkw, fd_kw;
  unsigned img = 0;  // elements per image: chan * (kh > 0 ? H*W : S)
  unsigned hw = 0;   // elements per channel: kh > 0 ? H*W : S
};

// Wt[ci][co*kh*kw + ki*kw + kj] = W[co][ci][kh-1-ki][kw-1-kj] per group —
// the flipped/transposed weights that turn backward-data into a forward
// convolution over dY (s1 only)
void weight_flip_grouped(hipStream_t s, const float* w, int Cout, int Cin_g,
                         int kh, int kw, int groups, float* wt);

void gemm(hipStream_t s, bool transA, bool transB, long M, long N, long K,
          float alpha, const float* A, long lda, const float* B, long ldb,
          float beta, float* C, long ldc, const GemmEpi* epi = nullptr,
          const GemmView* aview = nullptr, const GemmView* bview = nullptr);

// Route trace of gemm()'s dispatch (off by default; for the tests that pin
// which kernel a shape reaches).  Enabling clears the log; disabling keeps
// it readable.  gemm_trace_read() writes one "key=value ..." line per
// traced call into buf (at most cap bytes, always \0-terminated when
// cap > 0) and returns the length of the full text.
void gemm_trace(bool enable);
long gemm_trace_read(char* buf, long cap);
// Of the calls traced since the last enable: how many read their operands
// through the 32-bit staging cursors, and how many through the 64-bit
// reader (the W64 fp32 kernels and every bf16 kernel).
void gemm_trace_readers(long* cursor, long* wide64);

// Variant trace of the elementwise launch wrappers (pooling, BN statistics,
// LRN, softmax, segmented SGD): which specialised kernel a call launched and
// the numbers that shape it.  Same contract as gemm_trace: off by default,
// enabling clears the log, at most 4096 records, one "key=value ..." line
// per record:
//   op=pool_max_fwd var=k3|generic
//   op=pool_max_bwd var=k3s1|k3s2|k3|generic
//   op=pool_ave_fwd          op=pool_ave_bwd
//   op=bn_fwd_stats|bn_bwd_stats var=v4|scalar nb=<slices> span_max=<largest
//       per-block span, in elements (scalar) or float4 packs (v4)>
//   op=lrn_fwd|lrn_bwd var=ring5|generic odd=<(N*H*W) & 1>
//   op=softmax_fwd rows=<outer*inner> C=<C> blocks=<grid>
//   op=sgd_seg lo=<lo> hi=<hi> nseg=<nseg>
//   op=solver_seg rule=<sgd|nesterov|adagrad|rmsprop|adadelta|adam>
//       reg=<L1|L2> lo=<lo> hi=<hi> nseg=<nseg>
//   op=sigmoid_fwd|sigmoid_bwd|sigmoid_ce_bwd|euclid_bwd n=<elements>
//       blocks=<grid> passes=<grid-stride passes of the busiest thread>
//   op=sigmoid_ce_fwd|euclid_fwd n=<elements> blocks=<grid>
//       partials=<doubles the final sum adds> passes=<as above>
//   op=shared_diff_sum lo=<arena lo> hi=<arena hi> nseg=<the owner layer's
//       learnable blobs> nsrc=<sharing blobs added>
//   op=contrastive_fwd|contrastive_bwd var=row_thread|row_wave N=<rows>
//       C=<row width> blocks=<grid>
//   op=grad_sumsq lo=<lo> hi=<hi> blocks=<grid = partials written>
//       passes=<grid-stride passes of the busiest thread>
//   op=clip_final partials=<doubles summed>
// With clip_gradients set, sgd_seg and solver_seg records end in " clip=1"
// (the launch read the factor); without it their text is as above.
void kernel_trace(bool enable);
long kernel_trace_read(char* buf, long cap);

// db[c] = Σ_n Σ_s dy[n][c][s] (deterministic)
void bias_grad(hipStream_t s, const float* dy, int N, int C, long S,
               float* db);

// col[K][Nimg*Spad] from x[Nimg][C][H][W]; pad columns zero-filled.
void im2col_batched(hipStream_t s, const float* x, int Nimg, int C, int H,
                    int W, int kh, int kw, int ph, int pw, int sh, int sw,
                    int dh, int dw, int OH, int OW, long Spad, float* col);
// dx[Nimg][C][H][W] from dcol[K][Nimg*Spad] (gather, deterministic)
void col2im_batched(hipStream_t s, const float* dcol, int Nimg, int C, int H,
                    int W, int kh, int kw, int ph, int pw, int sh, int sw,
                    int dh, int dw, int OH, int OW, long Spad, float* dx);

// y += a*x (iter_size diff accumulation over the padded arena)
void axpy(hipStream_t s, long n, float a, const float* x, float* y);

// y = x * a[c] (+ b[c]) — Scale layer fwd / bwd-data
void chan_affine(hipStream_t s, const float* x, const float* a,
                 const float* b, int N, int C, long S, float* y);

void relu_fwd(hipStream_t s, const float* x, long n, float slope, float* y);
void relu_bwd(hipStream_t s, const float* x, const float* dy, long n,
              float slope, float* dx);

void pool_max_fwd(hipStream_t s, const float* x, int N, int C, int H, int W,
                  int kh, int kw, int ph, int pw, int sh, int sw, int OH,
                  int OW, float* y, int* mask);
void pool_max_bwd(hipStream_t s, const float* dy, const int* mask, int N,
                  int C, int H, int W, int kh, int kw, int ph, int pw,
                  int sh, int sw, int OH, int OW, float* dx);
void pool_ave_fwd(hipStream_t s, const float* x, int N, int C, int H, int W,
                  int kh, int kw, int ph, int pw, int sh, int sw, int OH,
                  int OW, float* y);
void pool_ave_bwd(hipStream_t s, const float* dy, int N, int C, int H, int W,
                  int kh, int kw, int ph, int pw, int sh, int sw, int OH,
                  int OW, float* dx);

// Fused BatchNorm (replaces the reference's ~10-launch GEMV chain,
// batch_norm_layer.hpp:96-120, with 3 kernels fwd / 3 bwd).
// partials: double2[nb*C] workspace. mean/var/inv_std: float[C] device.
int bn_blocks_per_channel(int N, int C);
void bn_fwd_stats(hipStream_t s, const float* x, int N, int C, long S,
                  int nb, void* partials);
void bn_fwd_finalize(hipStream_t s, const void* partials, int nb, int C,
                     long NS, float eps, float* mean, float* var,
                     float* inv_std);
void bn_fwd_norm(hipStream_t s, const float* x, const float* mean,
                 const float* inv_std, const float* scale, const float* bias,
                 int scale_bias, int N, int C, long S, float* y,
                 int fuse_relu = 0, const float* add = nullptr);
void bn_moving_avg(hipStream_t s, const float* mean, const float* var, int C,
                   float maf, int copy_only, float* gmean, float* gvar);
void bn_fwd_test(hipStream_t s, const float* x, const float* gmean,
                 const float* gvar, const float* scale, const float* bias,
                 int scale_bias, int N, int C, long S, float eps, float* y);
void bn_bwd_stats(hipStream_t s, const float* x, const float* dy,
                  const float* mean, const float* inv_std, int N, int C,
                  long S, int nb, const float* scale, const float* bias,
                  int fuse_relu, void* partials);
// writes dscale/dbias (if scale_bias) and the per-channel m_dy/m_dyxn terms
void bn_bwd_finalize(hipStream_t s, const void* partials, int nb, int C,
                     long NS, const float* scale, int scale_bias,
                     float* dscale, float* dbias, float* m_dy,
                     float* m_dyxn);
void bn_bwd_apply(hipStream_t s, const float* x, const float* dy,
                  const float* mean, const float* inv_std,
                  const float* scale, int scale_bias, const float* m_dy,
                  const float* m_dyxn, int N, int C, long S,
                  const float* bias, int fuse_relu, float* dx);

void lrn_fwd(hipStream_t s, const float* x, int N, int C, int H, int W,
             int size, float alpha, float beta, float k, float* scale,
             float* y);
void lrn_bwd(hipStream_t s, const float* x, const float* y, const float* dy,
             const float* scale, int N, int C, int H, int W, int size,
             float alpha, float beta, float* dx);

void softmax_fwd(hipStream_t s, const float* x, int outer, int C, int inner,
                 float* prob);
// loss_out: device float[1]; norm = outer*inner (VALID, no ignore label)
void softmaxloss_fwd(hipStream_t s, const float* prob, const float* label,
                     int outer, int C, int inner, float* loss_out);
void softmaxloss_bwd(hipStream_t s, const float* prob, const float* label,
                     int outer, int C, int inner, float scale, float* dx);

// Sigmoid (sigmoid_layer.cu): y = 1 / (1 + exp(-x)), x == y allowed;
// dx = dy * y * (1 - y) from the TOP data, so in-place needs no saved input.
// Stores past n are masked (the float4 pack at the edge is loaded whole).
void sigmoid_fwd(hipStream_t s, const float* x, long n, float* y);
void sigmoid_bwd(hipStream_t s, const float* y, const float* dy, long n,
                 float* dx);

// Loss sums over n elements, deterministic and two-stage: a fixed grid
// writes one double per block into `partials` (loss_partials(n) doubles),
// then one block adds them in a fixed order and writes loss_out[0].
int loss_partials(long n);
// SigmoidCrossEntropyLoss: Σ sigmoid_ce_term(x, t) / num; σ(x) is never
// materialised, the backward recomputes it: dx = (σ(x) - t) * scale
void sigmoid_ce_fwd(hipStream_t s, const float* x, const float* t, long n,
                    int num, double* partials, float* loss_out);
void sigmoid_ce_bwd(hipStream_t s, const float* x, const float* t, long n,
                    float scale, float* dx);
// EuclideanLoss: Σ (a - b)² / num / 2; backward recomputes a - b and writes
// da = scale_a * (a - b) and/or db = scale_b * (a - b) (null = not wanted)
void euclid_fwd(hipStream_t s, const float* a, const float* b, long n,
                int num, double* partials, float* loss_out);
void euclid_bwd(hipStream_t s, const float* a, const float* b, long n,
                float scale_a, float* da, float scale_b, float* db);

// ContrastiveLoss over a [N][C], b [N][C], sim [N]: the forward writes each
// row's d² into dist_sq (N floats, kept by the layer for the backward) and
// Σ contrastive_row_loss / N / 2 into loss_out through `partials`
// (contrastive_partials(N, C) doubles); the backward recomputes a - b and
// writes da = beta·(a - b) and/or db = -beta·(a - b) (null = not wanted),
// beta = contrastive_row_beta(.., alpha), alpha = loss_weight / N.  One
// thread per row for narrow rows, one wave per row for wide ones.
int contrastive_partials(int N, int C);
void contrastive_fwd(hipStream_t s, const float* a, const float* b,
                     const float* sim, int N, int C, float margin,
                     bool legacy, float* dist_sq, double* partials,
                     float* loss_out);
void contrastive_bwd(hipStream_t s, const float* a, const float* b,
                     const float* sim, const float* dist_sq, int N, int C,
                     float margin, bool legacy, float alpha, float* da,
                     float* db);

// out[n] = Σ_m A[m][n] — IP bias grad (deterministic)
void colsum(hipStream_t s, const float* A, long M, long N, float* out);

void axpby(hipStream_t s, long n, float a, const float* x, float b, float* y);
void copy(hipStream_t s, long n, const float* x, float* y);
void set_const(hipStream_t s, long n, float v, float* y);
void add3(hipStream_t s, long n, const float* a, const float* b, float* y,
          int fuse_relu = 0);
// y[n0..] accumulate: y += x
void acc(hipStream_t s, long n, const float* x, float* y);

// channel-block copy for Concat: src[N][Cs][S] <-> dst[N][Cd][S] at offset
void concat_fwd(hipStream_t s, const float* x, int N, int Cs, long S,
                int Cd, int c_off, float* y);
void concat_bwd(hipStream_t s, const float* dy, int N, int Cs, long S,
                int Cd, int c_off, float* dx);

void dropout_fwd(hipStream_t s, const float* x, long n, uint64_t seed,
                 uint64_t counter, float threshold, float scale, float* y,
                 uint8_t* mask);
void dropout_bwd(hipStream_t s, const float* dy, const uint8_t* mask, long n,
                 float scale, float* dx);

// fused SGD update (reference sgd_solver.cu:10-20 + the 1/nranks scale of
// net.cpp:910): g = g*gscale + decay*w; h = mom*h + lr*g; w -= h; g = 0,
// segmented over a flat arena range (one launch per bucket);
// lrs/decays already folded with the per-param multipliers by the caller
void sgd_update_segmented(hipStream_t s, long lo, long hi, float* g_arena,
                          float* h_arena, const long* seg_off,
                          float* const* w_ptrs, const float* lr_mults,
                          const float* decay_mults, int nseg, float mom,
                          float lr, float decay, float gscale,
                          const float* clip_factor = nullptr);

// segmented fused update for every rule but plain SGD+L2 (which stays on
// sgd_update_segmented): same contract — one launch per bucket over the flat
// arena range [lo, hi), segment tables uploaded once, coefficients as kernel
// arguments — but float4-wide, so lo and hi must be multiples of 4 (arena
// offsets and padded counts are multiples of 16).  h2_arena is the second
// history slot (AdaDelta, Adam); nullptr for the one-slot rules.
//
// Both take clip_factor, a device pointer to the iteration's clip factor
// (clip_finalize's norm_factor + 1), or nullptr without clip_gradients.
// Given, a sibling kernel (k_sgd_seg_clip / k_solver_seg_clip) runs the same
// per-element body with gscale * *clip_factor, folded once per thread; not
// given, the launch is the unclipped kernel, argument for argument.
void solver_update_segmented(hipStream_t s, int rule, bool l1, long lo,
                             long hi, float* g_arena, float* h_arena,
                             float* h2_arena, const long* seg_off,
                             float* const* w_ptrs, const float* lr_mults,
                             const float* decay_mults, int nseg,
                             const SolverCoef& coef,
                             const float* clip_factor = nullptr);

// clip_gradients, stage one: partials[b] = Σ g² (each square and the sum in
// double) of block b's share of the arena range [lo, hi), multiples of 4;
// float4 packs, grid-stride, fixed order, no atomics.  Returns the number of
// partials written, grad_sumsq_partials(hi - lo): the pack grid of the
// range, capped like every flat kernel here.
int grad_sumsq_partials(long n);
int grad_sumsq(hipStream_t s, const float* g_arena, long lo, long hi,
               double* partials);
// stage two, one block: norm = (float)(sqrt(Σ partials[0..np)) / world) and
// clip_factor(norm, clip) into norm_factor[0] and [1], on the device
void clip_finalize(hipStream_t s, const double* partials, int np, int world,
                   float clip, float* norm_factor);

// Shared params (Net::plan_param_sharing): add the sharers' diffs into one
// owner layer's padded arena range [lo, hi), multiples of 4.  seg_off: the
// arena offsets of the layer's nseg learnable blobs; src_begin: nseg + 1
// bounds into srcs, the sharers' diff pointers (nsrc of them in the range);
// tables uploaded once at net build.  Fixed order, no atomics.
void shared_diff_sum(hipStream_t s, long lo, long hi, float* g_arena,
                     const long* seg_off, int nseg, const int* src_begin,
                     const float* const* srcs, int nsrc);

// LMDB batch transform: uint8 -> fp32 crop/mirror/mean/scale
// (data_transformer.cu:14-100 analog); geo = per-image (ho, wo, mirror),
// mean_mode 0 = none, 1 = per-channel, 2 = per-pixel (mean_file)
void transform_u8(hipStream_t s, const uint8_t* in, int N, int C, int inH,
                  int inW, int outH, int outW, const int* geo,
                  const float* mean, int mean_mode, float scale,
                  float* out);

void fill_uniform(hipStream_t s, long n, uint64_t seed, uint64_t counter,
                  float lo, float hi, float* y);
void fill_labels(hipStream_t s, long n, uint64_t seed, uint64_t counter,
                 int classes, float* y);

}  // namespace gpu
}  // namespace camd
