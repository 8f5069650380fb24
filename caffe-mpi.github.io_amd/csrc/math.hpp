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

// ------------------------------------------------- softmax loss, loss_param
// Per-pixel formulas of the reference's softmax_loss_layer.cpp:65-117 for a
// SoftmaxWithLoss layer that carries a loss_param, shared by the CPU loop
// and the dense kernels (kernels/dense_softmax.hip).
enum LossNorm { kNormFull = 0, kNormValid, kNormBatchSize, kNormNone };
// the term the loss SUMS for a pixel whose label has probability p.  The
// clamp is a comparison, not fmaxf (which drops a NaN operand): a NaN p is
// returned as it is, so a contaminated row gives a NaN loss in both modes.
CAMD_HD inline float softmax_nll_term(float p) {
  if (p != p) return p;
  return -logf(p < 1.175494351e-38f ? 1.175494351e-38f : p);
}
// max(1, .) of the count the mode names; valid = the non-ignored labels
// (equal to outer * inner when the layer has no ignore_label)
CAMD_HD inline double softmax_loss_normalizer(int mode, long outer,
                                              long inner, long valid) {
  double n = 1.0;
  if (mode == kNormFull) n = (double)(outer * inner);
  if (mode == kNormValid) n = (double)valid;
  if (mode == kNormBatchSize) n = (double)outer;
  return n < 1.0 ? 1.0 : n;
}

// -------------------------------------------------------------------- PReLU
// Per-element formulas of the reference's prelu_layer.cpp:76-126, shared by
// the CPU loops and the kernels (kernels/prelu.hip).  At x == 0 the gradient
// takes the slope and the element adds dy * 0 to the slope's sum.
CAMD_HD inline float prelu_value(float x, float a) {
  return x > 0.f ? x : a * x;
}
CAMD_HD inline float prelu_dx(float x, float dy, float a) {
  return dy * (x > 0.f ? 1.f : a);
}
// the term the slope gradient SUMS, exact in double
CAMD_HD inline double prelu_da_term(float x, float dy) {
  return x <= 0.f ? (double)dy * (double)x : 0.0;
}

// ------------------------------------------------------ data feed transform
// One output value of the uint8 crop/mirror/mean/scale transform (the
// reference's DataTransformer::Transform): im is one record [C][inH][inW],
// (c, y, x) the destination position in the crop at (ho, wo), outW wide; mir
// reads the source row right to left.  The mean is subtracted in SOURCE
// coordinates (mean_file semantics).  uint8 converts exactly and a subtract
// then a multiply has no fused form: CPU loop and kernel give the same bits.
enum MeanMode { kMeanNone = 0, kMeanPerChannel, kMeanPerPixel };
CAMD_HD inline float transform_u8_at(const uint8_t* im, int c, int y, int x,
                                     int ho, int wo, int mir, int inH,
                                     int inW, int outW, const float* mean,
                                     MeanMode mean_mode, float scale) {
  const int sx = wo + (mir ? outW - 1 - x : x);
  const long src = ((long)c * inH + ho + y) * inW + sx;
  float m = 0.f;
  if (mean_mode == kMeanPerChannel)
    m = mean[c];
  else if (mean_mode == kMeanPerPixel)
    m = mean[src];
  return ((float)im[src] - m) * scale;
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
//   op=dwconv_fwd|dwconv_bwd_data var=k3s1_plane|k3s1_tile|k3s2_plane|
//       k3s2_tile|generic_plane|generic_tile planes=<(n, c) planes per block>
//       tiles_y=<tiles per plane> tiles_x=<likewise> blocks=<grid>
//   op=dwconv_bwd_weight var=k3|generic slices=<batch slices> bias=<0|1: db
//       accumulated in the same pass> blocks=<first-stage grid>
//   op=gconv_fwd|gconv_bwd_data var=<as dwconv_fwd> cig=<C/group>
//       cog=<Cout/group> chunks=<LDS channel chunks per block> planes=<images
//       per block> tiles_y=<tiles per plane> tiles_x=<likewise> blocks=<grid>
//   op=gconv_bwd_weight var=k3s1|k3s2|generic cig=.. cog=.. chunks=<staged
//       tiles per image> pairs=<output channels per thread (3x3)>
//       slices=<batch slices> bias=<0|1> splits=<threads sharing an owner's
//       pixels> blocks=<first-stage grid>
//   op=deconv_fwd var=mfma|direct phases=<sh*sw> chunks=<input-channel
//       chunks per block> tiles_y=<cell tiles per plane> tiles_x=<likewise>
//       blocks=<grid>
//   op=deconv_bwd_data var=direct phases=<sh*sw> chunks=<output-channel
//       chunks per block> tiles_y=<input-cell tiles per plane>
//       tiles_x=<likewise> blocks=<grid>
//   op=deconv_bwd_weight var=direct phases=<sh*sw> chunks=<(image,
//       cell tile) windows a block stages per tap pass> slices=<split-K
//       slices> blocks=<first-stage grid>
//   op=dsm_fwd|dsm_bwd form=resident|stream CR=<padded channels held in
//       registers; 0 when streaming> P=<pixels per thread> vec=<floats per
//       access> rows=<outer*inner> C=<C> blocks=<grid>
//   op=lrn_within_fwd|lrn_within_bwd var=k3|generic split=planes|tiles
//       planes=<(n, c) planes per block> tiles_y=<tiles per plane>
//       tiles_x=<likewise> blocks=<grid>
//   op=prelu_fwd var=v4|scalar|cols vec=<floats per access> slices=<row
//       slices per channel (cols: per column block)> blocks=<grid>
//       inplace=<0|1: x kept for the backward in the same pass>
//   op=prelu_bwd var=.. vec=.. slices=.. blocks=<first-stage grid>
//       dx=<0|1: the bottom gradient was written>
void kernel_trace(bool enable);
long kernel_trace_read(char* buf, long cap);
// The depthwise wrappers (kernels/depthwise.hip) record into the same log:
// which = 0 forward, 1 dgrad, 2 wgrad; var = kind * 2 + (tiled ? 1 : 0) with
// kind 0 k3s1, 1 k3s2, 2 generic (wgrad: 0 k3, 1 generic); a..d as printed.
void kernel_trace_dwconv(int which, int var, long a, long b, long c, long d);

// Depthwise convolution (Convolution with group == C): x[N][C][H][W],
// w[C*mult][1][kh][kw], y[N][C*mult][OH][OW]; output channel c*mult + j
// reads input channel c.  Direct kernels, no col buffer (depthwise.hip).
struct DwConv {
  int N, C, mult, H, W, OH, OW, kh, kw, sh, sw, ph, pw, dh, dw;
};
// false when even the smallest tile's window (kernel extent with dilation)
// does not fit the LDS tile; the conv plan then keeps the GEMM route
bool dwconv_supported(const DwConv& g);
// y = conv(x, w) (+ bias) (then ReLU)
void dwconv_fwd(hipStream_t s, const DwConv& g, const float* x,
                const float* w, const float* bias, bool relu, float* y);
// dx overwritten, every element once (gather form)
void dwconv_bwd_data(hipStream_t s, const DwConv& g, const float* dy,
                     const float* w, float* dx);
// dw (and db = Σ dy when db is given) overwritten; two-stage, deterministic
void dwconv_bwd_weight(hipStream_t s, const DwConv& g, const float* x,
                       const float* dy, float* dw, float* db);

// The grouped wrappers (kernels/grouped_conv.hip) likewise: which as above;
// var = kind * 2 + tiled (wgrad: kind); f = the eight fields as printed.
void kernel_trace_gconv(int which, int var, const long (&f)[8]);

// Grouped convolution with few channels per group: x[N][G*cig][H][W],
// w[G*cog][cig][kh][kw], y[N][G*cog][OH][OW]; group g maps input channels
// g*cig.. to output channels g*cog...  Direct kernels, no col buffer
// (grouped_conv.hip).
struct GConv {
  int N, G, cig, cog, H, W, OH, OW, kh, kw, sh, sw, ph, pw, dh, dw;
};
// false when the smallest forward, dgrad or wgrad tile does not fit the LDS
// budget or a tensor has 2^31 elements or more; the conv plan then keeps the
// GEMM route
bool gconv_supported(const GConv& g);
// y = conv(x, w) (+ bias) (then ReLU)
void gconv_fwd(hipStream_t s, const GConv& g, const float* x, const float* w,
               const float* bias, bool relu, float* y);
// dx overwritten, every element once (gather form)
void gconv_bwd_data(hipStream_t s, const GConv& g, const float* dy,
                    const float* w, float* dx);
// dw (and db = Σ dy when db is given) overwritten; two-stage, deterministic
void gconv_bwd_weight(hipStream_t s, const GConv& g, const float* x,
                      const float* dy, float* dw, float* db);

// The deconvolution wrapper (kernels/deconv.hip) likewise: var 0 mfma,
// 1 direct.
void kernel_trace_deconv(int var, long phases, long chunks, long tiles_y,
                         long tiles_x, long blocks);
// which = 0 dgrad (c, d = tiles_y, tiles_x), 1 wgrad (c = slices)
void kernel_trace_deconv_bwd(int which, int var, long phases, long chunks,
                             long c, long d, long blocks);

// Forward of a transposed convolution at stride > 1 and dilation 1:
// x[N][G*cig][H][W], w[G*cig][cog][kh][kw] (the Deconvolution layer's blob),
// y[N][G*cog][OH][OW] with OH = sh*(H-1) + kh - 2*ph; group g maps input
// channels g*cig.. to output channels g*cog...  Split by stride phase, no
// dcol matrix (deconv.hip).
struct Deconv {
  int N, G, cig, cog, H, W, OH, OW, kh, kw, sh, sw, ph, pw;
};
// false when the smallest window does not fit the LDS budget or a tensor
// (the packed weights included) has 2^31 elements or more; the layer then
// keeps the GEMM + col2im route
bool deconv_supported(const Deconv& g);
// y = deconv(x, w) (+ bias), every element written once; packs the weights
// into the kDeconvW workspace slot first
void deconv_fwd(hipStream_t s, const Deconv& g, const float* x,
                const float* w, const float* bias, float* y);
// Backward of the same layer, split by phase as forward is: no col of the
// top gradient.  false as for deconv_supported() (per pass: the windows and
// workspace slots differ), and where a channel count per group is above 4
// (MFMA variants for those layers measured slower than im2col + GEMMs and
// were cut, profiles/deconv.txt); the layer then keeps im2col + GEMMs for
// that pass
bool deconv_bwd_data_supported(const Deconv& g);
bool deconv_bwd_weight_supported(const Deconv& g);
// dx overwritten, every element once; packs the weights ci-innermost into
// the kDeconvWT workspace slot first
void deconv_bwd_data(hipStream_t s, const Deconv& g, const float* dy,
                     const float* w, float* dx);
// dw overwritten; split-K partials in the kDeconvPart slot, summed in fixed
// order by a second kernel: deterministic, no atomics
void deconv_bwd_weight(hipStream_t s, const Deconv& g, const float* x,
                       const float* dy, float* dw);

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
// batch_norm_layer.hpp:96-120, with 3 kernels fwd / 3 bwd; the forward
// finalize also advances the moving averages).
// partials: double2[nb*C] workspace. mean/var/inv_std: float[C] device.
int bn_blocks_per_channel(int N, int C);
void bn_fwd_stats(hipStream_t s, const float* x, int N, int C, long S,
                  int nb, void* partials);
// mean / var / inv_std from the partials, then the moving averages of the
// global statistics from them: g = (1 - maf) * batch + maf * g, or a plain
// copy of the batch value when copy_only (kernels/join_bn.hip)
void bn_fwd_finalize(hipStream_t s, const void* partials, int nb, int C,
                     long NS, float eps, float maf, int copy_only,
                     float* mean, float* var, float* inv_std, float* gmean,
                     float* gvar);
void bn_fwd_norm(hipStream_t s, const float* x, const float* mean,
                 const float* inv_std, const float* scale, const float* bias,
                 int scale_bias, int N, int C, long S, float* y,
                 int fuse_relu = 0, const float* add = nullptr);
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

// LRN with norm_region WITHIN_CHANNEL (kernels/lrn_within.hip): the window
// is size x size pixels of the element's own plane, zero outside it, the
// divisor size^2 everywhere and the shift 1.  One stencil pass each way:
// forward writes y and scale = s; backward reads x, dy and s (never y) and
// overwrites dx.  Deterministic, no atomics.
constexpr int kLrnWithinMaxSize = 41;  // the largest local_size (LDS budget)
struct LrnWithin {
  int planes, H, W, size;  // planes = N * C
  float alpha, beta;
};
// The window variant (var: 0 k3, 1 generic) and the work split, chosen once
// per Reshape: `planes` (a block owns P whole planes) where a plane with its
// halo fits the LDS budget, `tiles` (a block owns one TH x TW tile of one
// plane) above that.
struct LrnWithinPlan {
  int var, tiled, P, TH, TW, ty, tx, LH, blocks;
  FastDiv fd_per, fd_px, fd_lh, fd_tw, fd_segs_w, fd_segs_h, fd_tx;
};
// errors: an empty or 2^30-pixel plane, an even local_size or one above
// kLrnWithinMaxSize, a grid of 2^31 blocks
LrnWithinPlan lrn_within_plan(const LrnWithin& g);
void lrn_within_fwd(hipStream_t s, const LrnWithin& g, const LrnWithinPlan& t,
                    const float* x, float* scale, float* y);
void lrn_within_bwd(hipStream_t s, const LrnWithin& g, const LrnWithinPlan& t,
                    const float* x, const float* dy, const float* scale,
                    float* dx);
// Their record in the kernel trace: which = 0 forward, 1 backward; var as in
// the plan.
void kernel_trace_lrn_within(int which, int var, bool tiled, long planes,
                             long tiles_y, long tiles_x, long blocks);

// PReLU (kernels/prelu.hip): x, y, dx, dy [N][C][S], slopes a[C], or a[1]
// when shared.  Forward one pass, backward one pass plus a finalize of the
// per-(slice, channel) double partials in the kPReluPart workspace slot;
// deterministic, no atomics.
struct PRelu {
  long N;
  int C;
  long S;
  bool shared;
};
enum PReluVar { kPReluV4 = 0, kPReluScalar, kPReluCols };
constexpr int kPReluThreads = 256;
constexpr int kPReluBlocks = 2048;  // the grid the slices aim at
constexpr int kPReluChunk = 1024;   // most loads in one piece of a plane
constexpr int kPReluColsPerBlock = 64;  // cols: column packs of a block
constexpr int kPReluColsMinRows = 32;   // cols: fewest rows worth a slice
// The layout and the work split, chosen once per Reshape.  v4 (S % 4 == 0)
// and scalar: a plane is `chunks` pieces of `clen` loads of `vec` floats,
// `per` loads in all; a channel has rows = N * chunks pieces, a block owns
// one channel and `rps` of its rows: blocks = C * slices.  cols (S == 1):
// `per` column packs of `vec` columns, cb blocks of them across C, rows = N,
// a block owns `rps` of them: blocks = cb * slices.
struct PReluPlan {
  int var, vec, per, chunks, clen, cb, rows, rps, slices, blocks;
  FastDiv fd_clen, fd_chunks;
};
// errors: an empty tensor, an axis, a channel's rows, a block's loads or the
// grid at 2^31 or more
PReluPlan prelu_plan(const PRelu& g);
// y = prelu(x).  saved given: in-place, y == x, and the x each thread loads
// is stored to saved before y overwrites it
void prelu_fwd(hipStream_t s, const PRelu& g, const PReluPlan& t,
               const float* x, const float* a, float* y, float* saved);
// da overwritten; dx overwritten unless null (not wanted); dx may be dy
void prelu_bwd(hipStream_t s, const PRelu& g, const PReluPlan& t,
               const float* x, const float* dy, const float* a, float* dx,
               float* da);
// Their record in the kernel trace: which = 0 forward (flag = in-place),
// 1 backward (flag = dx written); var as PReluVar.
void kernel_trace_prelu(int which, int var, int vec, long slices, long blocks,
                        bool flag);

void softmax_fwd(hipStream_t s, const float* x, int outer, int C, int inner,
                 float* prob);
// loss_out: device float[1]; norm = outer*inner (VALID, no ignore label)
void softmaxloss_fwd(hipStream_t s, const float* prob, const float* label,
                     int outer, int C, int inner, float* loss_out);
void softmaxloss_bwd(hipStream_t s, const float* prob, const float* label,
                     int outer, int C, int inner, float scale, float* dx);

// SoftmaxWithLoss with a loss_param, pixel-major (kernels/dense_softmax.hip):
// x, prob, dx [outer][C][inner], label [outer][inner].  A thread owns P
// pixels adjacent along inner and walks the channels, so every access is
// unit-stride across lanes; C <= 32 keeps the logits in registers
// (resident), wider rows stream x twice.  The forward writes prob once,
// sums softmax_nll_term over the non-ignored pixels (a non-ignored label
// outside [0, C) adds NaN and is never an index) into `partials`
// (kDsmPartials doubles, fixed grid, no atomics), and one block then writes
// loss_out[0] = sum / normalizer and norm_slot = {valid count,
// 1 / normalizer}.  The backward reads the scale from norm_slot[1], so no
// mode needs a host read-back: dx = (prob - onehot) * loss_weight *
// norm_slot[1], exact zeros at ignored pixels, every element written once.
struct DenseSoftmax {
  int outer, C, inner;
  bool has_ignore;
  int ignore;
  int norm;  // LossNorm
};
constexpr int kDsmMaxBlocks = 1024;  // grid cap; grid-stride beyond it
constexpr int kDsmPartials = 2 * kDsmMaxBlocks;
void dense_softmaxloss_fwd(hipStream_t s, const DenseSoftmax& g,
                           const float* x, const float* label, float* prob,
                           double* partials, float* loss_out,
                           float* norm_slot);
void dense_softmaxloss_bwd(hipStream_t s, const DenseSoftmax& g,
                           const float* prob, const float* label,
                           const float* norm_slot, float loss_weight,
                           float* dx);
// records op=dsm_fwd|dsm_bwd (which = 0 | 1); f = CR, P, vec, rows, C, blocks
void kernel_trace_dsm(int which, bool stream, const long (&f)[6]);

// Crop: a window of x copied into y (forward), or dy laid into a zero dx
// (backward, every dx element written once), over at most four collapsed
// axes: B the bottom's sizes, T the window's, off its start; axis 3 is the
// innermost, where lanes run.  Each tensor has fewer than 2^31 elements.
struct CropGeom {
  unsigned B[4], T[4], off[4];
};
void crop_fwd(hipStream_t s, const CropGeom& g, const float* x, float* y);
void crop_bwd(hipStream_t s, const CropGeom& g, const float* dy, float* dx);

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
// dx = (a + b) * (ref > 0 ? 1 : slope): add3 then relu_bwd in one pass, the
// same two fp32 operations per element; dx may be a or b
// (kernels/join_bn.hip)
void add_relu_bwd(hipStream_t s, long n, const float* a, const float* b,
                  const float* ref, float slope, float* dx);
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

// Data feed batch transform: transform_u8_at at every output element
// (data_transformer.cu:14-100 analog); geo = per-image (ho, wo, mirror)
void transform_u8(hipStream_t s, const uint8_t* in, int N, int C, int inH,
                  int inW, int outH, int outW, const int* geo,
                  const float* mean, MeanMode mean_mode, float scale,
                  float* out);

void fill_uniform(hipStream_t s, long n, uint64_t seed, float lo, float hi,
                  float* y);
void fill_labels(hipStream_t s, long n, uint64_t seed, int classes, float* y);

}  // namespace gpu
}  // namespace camd
