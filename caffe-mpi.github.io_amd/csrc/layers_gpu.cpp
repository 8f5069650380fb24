// layers_gpu.cpp — GPU paths of every hot-path layer, built on the MFMA
// GEMM (kernels/gemm_f32.hip) and the HBM-bound kernels
// (kernels/elementwise.hip).  Conv strategy (MI355X-first, replaces the
// reference's per-image GEMM loop conv_layer.cu:14-21 which is
// launch/sync-bound): whole-batch GEMMs, NCHW-view operands (implicit
// im2col for s1/d1 at OW>=24), fused bias/ReLU/scatter epilogues, explicit
// cached col buffers only for strided/small-OW convs.  Shared scratch comes
// from the named Workspace slots (layers.hpp); a buffer that outlives a call
// is owned by its layer.
#include "layers.hpp"

namespace camd {

using gpu::GemmEpi;
using gpu::GemmView;

// ------------------------------------------------------------------ Conv
// MI355X-first conv, two paths:
//  - IMPLICIT GEMM: the GEMM staging reads x / dY straight from NCHW through
//    im2col/NCHW views; no col buffer, no im2col/col2im kernels; at stride 1
//    backward-data runs as a forward convolution over dY with
//    flipped/transposed weights (Wt), scattered into dx.
//  - explicit batched col buffer [K][N*Spad], cached per layer (forward
//    fills, backward reuses).
// plan_gpu() decides which, once per Reshape (table in DESIGN.md §3).  The
// implicit-im2col staging walks pixel chunks of 16; below OW 24 nearly every
// chunk crosses an output row (slow masked path) — the explicit col wins
// there (measured: stage-4 3x3 at OW=14 ran at 68 vs ~90 TF).  Strides are
// supported by the view, but
// ONLY for conv1-like shapes (kh>1, Cout/group <= 128 so the x view is
// staged once — a strided view re-read per output tile-row pays 2x bytes
// per pass, which measured SLOWER than the explicit col for the large-Cout
// 1x1/s2 projections).  Strided 1x1 p0 keeps the explicit col for fwd/wgrad
// and a zero+scatter dgrad (no dcol GEMM, no col2im: it writes only the
// sampled input pixels).  Dilation stays explicit.  The strided scatter
// never meets the im2col view — a strided view needs kh > 1, the scatter
// kh == 1 — so it is tested on its own, after the stride-1 view.
//
// DEPTHWISE (one input channel per group, any channel multiplier, stride,
// pad and dilation) leaves the GEMM family: the per-group loop would run
// `group` GEMMs of M = multiplier, K = kh*kw per pass, all launch latency.
// It takes the direct kernels of kernels/depthwise.hip when group >= 8 and
// kh*kw <= 49 (and the dilated window fits the kernels' LDS tile, which any
// window that fits a real image does).  The group >= 8 bound is a policy
// constant and has NOT been measured: it is chosen so that no shape in the
// existing suites changes route (they use group <= 4: the geometry sweep
// can draw C = 4 / group 4, the torch cross-check C = 2 / group 2).
// CAFFE_DEPTHWISE=0 forces the per-group loop, for measuring one against
// the other.
//
// GROUPED with few channels per group (ResNeXt / ShuffleNet class) is tested
// right after: cig = C/group in 4..32, cog = Cout/group in 1..32, group >= 8,
// kh*kw <= 49, any stride, pad and dilation, and tiles that fit the LDS
// budget (gconv_supported).  It takes the direct kernels of
// kernels/grouped_conv.hip: no gemm, im2col, col2im or weight flip, no col_.
// group >= 8 and cig >= 4 are policy constants like depthwise's and have
// NOT been measured below: they keep every shape of the existing suites on
// its present route (the geometry sweep uses group <= 4, the GEMM route
// tests group 2, and the depthwise boundary test's cig = 2 at group 8 must
// stay on the loop).  The upper bounds of 32 are where the measured shapes
// end (profiles/grouped_conv.txt).  CAFFE_GROUPED=0 forces
// the per-group loop.
static gpu::DwConv dw_geom(const ConvolutionLayer& l) {
  return {l.N_,  l.C_,  l.Cout_ / l.C_, l.H_,  l.W_,  l.OH_, l.OW_, l.kh_,
          l.kw_, l.sh_, l.sw_,          l.ph_, l.pw_, l.dh_, l.dw_};
}
static gpu::GConv gc_geom(const ConvolutionLayer& l) {
  return {l.N_,  l.group_, l.C_ / l.group_, l.Cout_ / l.group_,
          l.H_,  l.W_,     l.OH_,           l.OW_,
          l.kh_, l.kw_,    l.sh_,           l.sw_,
          l.ph_, l.pw_,    l.dh_,           l.dw_};
}
void ConvolutionLayer::plan_gpu() {
  static const bool depthwise_ok = [] {
    const char* e = getenv("CAFFE_DEPTHWISE");
    return e ? atoi(e) != 0 : true;
  }();
  if (depthwise_ok && C_ / group_ == 1 && group_ >= 8 && kh_ * kw_ <= 49 &&
      gpu::dwconv_supported(dw_geom(*this))) {
    xop_ = kDepthwise;
    dgrad_ = kDwGather;
    return;
  }
  static const bool grouped_ok = [] {
    const char* e = getenv("CAFFE_GROUPED");
    return e ? atoi(e) != 0 : true;
  }();
  const int cig = C_ / group_, cog = Cout_ / group_;
  if (grouped_ok && group_ >= 8 && cig >= 4 && cig <= 32 && cog >= 1 &&
      cog <= 32 && kh_ * kw_ <= 49 && gpu::gconv_supported(gc_geom(*this))) {
    xop_ = kGrouped;
    dgrad_ = kGcGather;
    return;
  }
  static const int min_ow = [] {
    const char* e = getenv("CAFFE_IMPLICIT_MIN_OW");
    return e ? atoi(e) : 24;
  }();
  static const bool strided_ok = [] {
    const char* e = getenv("CAFFE_IMPLICIT_STRIDED");
    return e ? atoi(e) != 0 : true;
  }();
  const bool s1 = sh_ == 1 && sw_ == 1, d1 = dh_ == 1 && dw_ == 1;
  const bool k1p0 = kh_ == 1 && kw_ == 1 && !ph_ && !pw_;
  const bool chan = k1p0 && s1 && d1 && group_ == 1;
  const bool view =
      !chan && d1 &&
      (s1 ? kh_ == 1 || OW_ >= min_ow
          : strided_ok && kh_ > 1 && OW_ >= min_ow && Cout_ / group_ <= 128);
  xop_ = chan ? kChanView : view ? kIm2colView : kExplicitCol;
  dgrad_ = chan                ? kTnScatter
           : view && s1        ? kFlipConv
           : !s1 && k1p0 && d1 ? kStridedScatter
                               : kCol2im;
}

// elements in one group's slice of each conv operand (group g's slice starts
// g of them in): w = W, dW and the flipped weights; x = x, dx; y = y, dy;
// col = col, dcol, whose rows are ns = N*Spad long
struct ConvGroup {
  long w, x, y, bias, col;
};
static ConvGroup conv_group(const ConvolutionLayer& l, long ns) {
  const long cig = l.C_ / l.group_, cog = l.Cout_ / l.group_;
  const long K = cig * l.kh_ * l.kw_;
  return {cog * K, cig * l.H_ * l.W_, cog * l.S_, cog, K * ns};
}

// The operands of one conv's per-group GEMMs: Cout output channels of S
// pixels (Spad padded) from K = C/group * kh * kw col rows per group.
// Convolution passes its own geometry; Deconvolution's backward passes the
// conv that maps its top gradient to its bottom.
struct ConvGemms {
  int group;
  long Cout, K, S, Spad, NS;
  ConvGroup o;
};
static ConvGemms conv_gemms(const ConvolutionLayer& l) {
  const long NS = (long)l.N_ * l.Spad_;
  return {l.group_, l.Cout_, (long)l.C_ / l.group_ * l.kh_ * l.kw_,
          l.S_,     l.Spad_, NS,
          conv_group(l, NS)};
}
// y = W·B per group, scattered to NCHW by epi (bias per group added there):
// B is x through the view xv, or, with col, the col buffer b
static void conv_fwd_gemms(const ConvGemms& c, const float* w, const float* b,
                           bool col, const GemmView& xv, GemmEpi epi,
                           const float* bias, float* y) {
  hipStream_t s = Engine::get().stream;
  for (int g = 0; g < c.group; ++g) {
    epi.bias = bias ? bias + g * c.o.bias : nullptr;
    gpu::gemm(s, false, false, c.Cout / c.group, c.NS, c.K, 1.f,
              w + g * c.o.w, c.K, b + g * (col ? c.o.col : c.o.x),
              col ? c.NS : 0, 0.f, y + g * c.o.y, c.S, &epi, nullptr,
              col ? nullptr : &xv);
  }
}
// dW = dY-view · Bᵀ per group, B as in forward
static void conv_wgrad_gemms(const ConvGemms& c, const float* dy,
                             const float* b, bool col, const GemmView& xv,
                             float* dw) {
  hipStream_t s = Engine::get().stream;
  const GemmView dyv{c.Spad, c.S, c.Cout};  // dY[N][Cout][S] as [Cout][N*Spad]
  for (int g = 0; g < c.group; ++g)
    gpu::gemm(s, false, true, c.Cout / c.group, c.K, c.NS, 1.f,
              dy + g * c.o.y, 0, b + g * (col ? c.o.col : c.o.x),
              col ? c.NS : 0, 0.f, dw + g * c.o.w, c.K, nullptr, &dyv,
              col ? nullptr : &xv);
}

// NCHW-scatter epilogue: column n*spad + s of GEMM row r lands at
// C[(n*chan + r)*S + s]
static GemmEpi nchw_scatter(long spad, long S, long chan) {
  GemmEpi epi;
  epi.spad = spad;
  epi.S = S;
  epi.n_stride = chan * S;
  return epi;
}

// x as forward's and wgrad's B operand: the plan's view (the explicit col
// passes its buffer as a plain B instead and no view)
static GemmView conv_x_view(const ConvolutionLayer& l) {
  if (l.xop_ == ConvolutionLayer::kChanView) return {l.Spad_, l.S_, l.C_};
  return {l.Spad_, l.S_,  l.C_, l.kh_, l.kw_, l.ph_,  // strides in the view
          l.pw_,   l.H_,  l.W_, l.OW_, l.sh_, l.sw_};
}

void ConvolutionLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                                   const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  const long NS = (long)N_ * Spad_;
  const float* x = bottom[0]->gpu_data();
  const float* w = blobs_[0]->gpu_data();
  const float* bias = bias_ ? blobs_[1]->gpu_data() : nullptr;
  float* y = top[0]->mutable_gpu_data();
  if (xop_ == kDepthwise) {
    gpu::dwconv_fwd(E.stream, dw_geom(*this), x, w, bias, fuse_relu_, y);
    return;
  }
  if (xop_ == kGrouped) {
    gpu::gconv_fwd(E.stream, gc_geom(*this), x, w, bias, fuse_relu_, y);
    return;
  }

  // B is x through the plan's view, or the col buffer (cached for backward)
  const bool col = xop_ == kExplicitCol;
  const GemmView xv = conv_x_view(*this);
  const float* b = x;
  if (col) {
    b = (float*)col_.reserve(sizeof(float) * (size_t)C_ * kh_ * kw_ * NS);
    gpu::im2col_batched(E.stream, x, N_, C_, H_, W_, kh_, kw_, ph_, pw_, sh_,
                        sw_, dh_, dw_, OH_, OW_, Spad_, (float*)col_.p);
  }
  GemmEpi epi = nchw_scatter(Spad_, S_, Cout_);
  epi.relu = fuse_relu_;
  conv_fwd_gemms(conv_gemms(*this), w, b, col, xv, epi, bias, y);
}

void ConvolutionLayer::Backward_gpu(const std::vector<Blob*>& top,
                                    const std::vector<bool>& prop_down,
                                    const std::vector<Blob*>& bottom) {
  Engine& E = Engine::get();
  const int K = C_ / group_ * kh_ * kw_;
  const long NS = (long)N_ * Spad_;
  Workspace& ws = Workspace::get_global();
  const float* x = bottom[0]->gpu_data();
  const float* w = blobs_[0]->gpu_data();
  const float* dy = top[0]->gpu_diff();
  GemmView dyv{Spad_, S_, Cout_};  // dY[N][Cout][S] as [Cout][N*Spad]

  if (xop_ == kDepthwise) {  // wgrad's pass over dy also sums db
    const gpu::DwConv g = dw_geom(*this);
    gpu::dwconv_bwd_weight(E.stream, g, x, dy, blobs_[0]->mutable_gpu_diff(),
                           bias_ ? blobs_[1]->mutable_gpu_diff() : nullptr);
    if (prop_down[0])
      gpu::dwconv_bwd_data(E.stream, g, dy, w, bottom[0]->mutable_gpu_diff());
    return;
  }
  if (xop_ == kGrouped) {  // likewise
    const gpu::GConv g = gc_geom(*this);
    gpu::gconv_bwd_weight(E.stream, g, x, dy, blobs_[0]->mutable_gpu_diff(),
                          bias_ ? blobs_[1]->mutable_gpu_diff() : nullptr);
    if (prop_down[0])
      gpu::gconv_bwd_data(E.stream, g, dy, w, bottom[0]->mutable_gpu_diff());
    return;
  }

  if (bias_)
    gpu::bias_grad(E.stream, dy, N_, Cout_, S_,
                   blobs_[1]->mutable_gpu_diff());

  // wgrad: dW = dY-view · Bᵀ, B as in forward (the col buffer is the one
  // this iteration's forward filled)
  const bool col = xop_ == kExplicitCol;
  const size_t colbytes = sizeof(float) * (size_t)C_ * kh_ * kw_ * NS;
  CHECK_(!col || col_.bytes >= colbytes) << "conv backward before forward";
  const GemmView xv = conv_x_view(*this);
  const float* b = col ? (const float*)col_.p : x;
  float* dw = blobs_[0]->mutable_gpu_diff();
  const ConvGroup o = conv_group(*this, NS);
  conv_wgrad_gemms(conv_gemms(*this), dy, b, col, xv, dw);
  if (!prop_down[0]) return;

  float* dx = bottom[0]->mutable_gpu_diff();
  switch (dgrad_) {
    case kTnScatter: {  // dx = Wᵀ·dY scattered to NCHW; group 1 by the plan
      const GemmEpi epi = nchw_scatter(Spad_, S_, C_);
      gpu::gemm(E.stream, true, false, K, NS, Cout_, 1.f, w, K, dy, 0, 0.f,
                dx, S_, &epi, nullptr, &dyv);
      break;
    }
    case kFlipConv: {
      // dgrad = forward conv of dY with flipped/transposed weights:
      // dx[ci] = Σ_{co,ki,kj} dy[co][h-ki+ (kh-1-ph) ...] · Wt
      float* wt = (float*)ws.get(Workspace::kFlipW,
                                 sizeof(float) * blobs_[0]->count());
      gpu::weight_flip_grouped(E.stream, w, Cout_, C_ / group_, kh_, kw_,
                               group_, wt);
      const long S_in = (long)H_ * W_;
      const long spad_in = (S_in + 15) / 16 * 16;
      const int Kd = Cout_ / group_ * kh_ * kw_;
      const GemmEpi epi = nchw_scatter(spad_in, S_in, C_);
      // dY viewed with the transposed-conv geometry: input dims (OH,OW),
      // pad (k-1-p), output dims (H,W)
      GemmView dyc{spad_in, S_in, Cout_, kh_, kw_, kh_ - 1 - ph_,
                   kw_ - 1 - pw_, OH_, OW_, W_};
      for (int g = 0; g < group_; ++g)
        gpu::gemm(E.stream, false, false, C_ / group_, N_ * spad_in, Kd, 1.f,
                  wt + g * o.w, Kd, dy + g * o.y, 0, 0.f, dx + g * o.x, S_in,
                  &epi, nullptr, &dyc);
      break;
    }
    case kStridedScatter: {
      // strided 1x1 (projection shortcuts): dgrad touches only the sampled
      // input pixels — zero dx, then a GEMM whose epilogue scatters column
      // (oh, ow) to input pixel (oh*sh, ow*sw).  No dcol, no col2im.
      gpu::set_const(E.stream, bottom[0]->count(), 0.f, dx);
      GemmEpi epi = nchw_scatter(Spad_, S_, C_);
      epi.Srow = (long)H_ * W_;  // rows are input channels of H*W pixels
      epi.n_stride = C_ * epi.Srow;
      epi.OWo = OW_;
      epi.osh = sh_;
      epi.osw = sw_;
      epi.Wd = W_;
      for (int g = 0; g < group_; ++g)
        gpu::gemm(E.stream, true, false, C_ / group_, NS, Cout_ / group_,
                  1.f, w + g * o.w, K, dy + g * o.y, 0, 0.f, dx + g * o.x, 0,
                  &epi, nullptr, &dyv);
      break;
    }
    case kCol2im: {
      // dcol = Wᵀ·dY, then gather col2im (a strided im2col-view conv gets
      // here only when prop_down, which a first layer never is)
      float* dcol = (float*)ws.get(Workspace::kDcol, colbytes);
      for (int g = 0; g < group_; ++g)
        gpu::gemm(E.stream, true, false, K, NS, Cout_ / group_, 1.f,
                  w + g * o.w, K, dy + g * o.y, 0, 0.f, dcol + g * o.col, NS,
                  nullptr, nullptr, &dyv);
      gpu::col2im_batched(E.stream, dcol, N_, C_, H_, W_, kh_, kw_, ph_, pw_,
                          sh_, sw_, dh_, dw_, OH_, OW_, Spad_, dx);
      break;
    }
    case kDwGather:  // returned above
    case kGcGather:
      break;
  }
}

// -------------------------------------------------------- Deconvolution
// Forward is the backward-data of the conv that maps the top to the bottom
// (layers.hpp).  At stride > 1 and dilation 1 it takes the phase-split
// kernels of kernels/deconv.hip: no dcol matrix, bias in the epilogue
// (deconv_supported: the window fits LDS, 32-bit indices).  Inside that
// route deconv.hip picks its direct variant at Cout/group <= 4 and the MFMA
// variant above; that threshold is a policy constant and has NOT been
// measured.  Stride 1, dilation > 1 and CAFFE_DECONV=0 take the form the
// conv dgrad's kCol2im has: dcol = Wᵀ·x per group, col2im_batched, then a
// bias pass.  Backward on the same conditions (and CAFFE_DECONV_BWD not 0,
// which switches backward alone for A/B timing) is phase-split too, one
// flag per pass: deconv_bwd_weight (x and the top gradient's phase planes
// from LDS, split-K partials and a fixed-order reduce) and deconv_bwd_data
// (one accumulator set per pixel over every phase and tap); the bias
// gradient stays bias_grad.  A pass its predicate refuses (more than 4
// channels per group on either side, a window that does not fit LDS) keeps the explicit-col conv of the top gradient: one im2col into
// col_ serves the wgrad GEMMs and, when it propagates, the forward GEMMs
// that give dx; both are Convolution's own GEMM loops.  col_ is reserved
// only when a pass that runs needs it.
static float* zeros_ones(Blob& zo, int C);

static gpu::Deconv dc_geom(const DeconvolutionLayer& l) {
  return {l.N_, l.group_, l.C_ / l.group_, l.Cout_ / l.group_,
          l.H_, l.W_,     l.OH_,           l.OW_,
          l.kh_, l.kw_,   l.sh_,           l.sw_,
          l.ph_, l.pw_};
}
void DeconvolutionLayer::plan_gpu() {
  static const bool split_ok = [] {
    const char* e = getenv("CAFFE_DECONV");
    return e ? atoi(e) != 0 : true;
  }();
  static const bool bwd_ok = [] {
    const char* e = getenv("CAFFE_DECONV_BWD");
    return e ? atoi(e) != 0 : true;
  }();
  const bool zone = split_ok && dh_ == 1 && dw_ == 1 && (sh_ > 1 || sw_ > 1);
  const gpu::Deconv g = dc_geom(*this);
  phase_split_ = zone && gpu::deconv_supported(g);
  split_dgrad_ = zone && bwd_ok && gpu::deconv_bwd_data_supported(g);
  split_wgrad_ = zone && bwd_ok && gpu::deconv_bwd_weight_supported(g);
}

// the conv from the top [N][Cout][OH][OW] to the bottom [N][C][H][W]: its
// output channels are C_, its col rows Cout/group * kh * kw per group
static ConvGemms deconv_gemms(const DeconvolutionLayer& l) {
  const long NS = (long)l.N_ * l.Spad_;
  const long cig = l.C_ / l.group_, cog = l.Cout_ / l.group_;
  const long K = cog * l.kh_ * l.kw_;
  return {l.group_, l.C_, K, l.S_, l.Spad_, NS,
          {cig * K, cog * l.OH_ * l.OW_, cig * l.S_, cig, K * NS}};
}

void DeconvolutionLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                                     const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  const float* x = bottom[0]->gpu_data();
  const float* w = blobs_[0]->gpu_data();
  const float* bias = bias_ ? blobs_[1]->gpu_data() : nullptr;
  float* y = top[0]->mutable_gpu_data();
  if (phase_split_) {
    gpu::deconv_fwd(E.stream, dc_geom(*this), x, w, bias, y);
    return;
  }
  const ConvGemms c = deconv_gemms(*this);
  float* dcol = (float*)Workspace::get_global().get(
      Workspace::kDcol, sizeof(float) * (size_t)group_ * c.o.col);
  const GemmView xv{Spad_, S_, C_};  // x[N][C][S] as [C][N*Spad]
  for (int g = 0; g < group_; ++g)
    gpu::gemm(E.stream, true, false, c.K, c.NS, C_ / group_, 1.f,
              w + g * c.o.w, c.K, x + g * c.o.y, 0, 0.f, dcol + g * c.o.col,
              c.NS, nullptr, nullptr, &xv);
  gpu::col2im_batched(E.stream, dcol, N_, Cout_, OH_, OW_, kh_, kw_, ph_, pw_,
                      sh_, sw_, dh_, dw_, H_, W_, Spad_, y);
  if (bias)  // y = y*1 + b[c]
    gpu::chan_affine(E.stream, y, zeros_ones(zo_, Cout_) + Cout_, bias, N_,
                     Cout_, (long)OH_ * OW_, y);
}

void DeconvolutionLayer::Backward_gpu(const std::vector<Blob*>& top,
                                      const std::vector<bool>& prop_down,
                                      const std::vector<Blob*>& bottom) {
  Engine& E = Engine::get();
  const float* dy = top[0]->gpu_diff();
  if (bias_)
    gpu::bias_grad(E.stream, dy, N_, Cout_, (long)OH_ * OW_,
                   blobs_[1]->mutable_gpu_diff());
  const bool dgrad = prop_down[0];
  const ConvGemms c = deconv_gemms(*this);
  const float* col = nullptr;
  if (!split_wgrad_ || (dgrad && !split_dgrad_)) {
    col = (float*)col_.reserve(sizeof(float) * (size_t)group_ * c.o.col);
    gpu::im2col_batched(E.stream, dy, N_, Cout_, OH_, OW_, kh_, kw_, ph_, pw_,
                        sh_, sw_, dh_, dw_, H_, W_, Spad_, (float*)col_.p);
  }
  if (split_wgrad_)
    gpu::deconv_bwd_weight(E.stream, dc_geom(*this), bottom[0]->gpu_data(),
                           dy, blobs_[0]->mutable_gpu_diff());
  else  // the wgrad's "dY" is the bottom data: dW[ci][co, ki, kj] = x · colᵀ
    conv_wgrad_gemms(c, bottom[0]->gpu_data(), col, true, GemmView{},
                     blobs_[0]->mutable_gpu_diff());
  if (!dgrad) return;
  if (split_dgrad_)
    gpu::deconv_bwd_data(E.stream, dc_geom(*this), dy, blobs_[0]->gpu_data(),
                         bottom[0]->mutable_gpu_diff());
  else
    conv_fwd_gemms(c, blobs_[0]->gpu_data(), col, true, GemmView{},
                   nchw_scatter(Spad_, S_, C_), nullptr,
                   bottom[0]->mutable_gpu_diff());
}

// -------------------------------------------------------------------- IP
void InnerProductLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                                    const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  GemmEpi epi;
  epi.bias = bias_ ? blobs_[1]->gpu_data() : nullptr;
  epi.bias_per_col = true;
  gpu::gemm(E.stream, false, true, M_, Nout_, K_, 1.f, bottom[0]->gpu_data(),
            K_, blobs_[0]->gpu_data(), K_, 0.f, top[0]->mutable_gpu_data(),
            Nout_, &epi);
}

void InnerProductLayer::Backward_gpu(const std::vector<Blob*>& top,
                                     const std::vector<bool>& prop_down,
                                     const std::vector<Blob*>& bottom) {
  Engine& E = Engine::get();
  const float* dy = top[0]->gpu_diff();
  // dW[Nout][K] = dYᵀ · x
  gpu::gemm(E.stream, true, false, Nout_, K_, M_, 1.f, dy, Nout_,
            bottom[0]->gpu_data(), K_, 0.f, blobs_[0]->mutable_gpu_diff(),
            K_, nullptr);
  if (bias_)
    gpu::colsum(E.stream, dy, M_, Nout_, blobs_[1]->mutable_gpu_diff());
  if (prop_down[0])
    gpu::gemm(E.stream, false, false, M_, K_, Nout_, 1.f, dy, Nout_,
              blobs_[0]->gpu_data(), K_, 0.f,
              bottom[0]->mutable_gpu_diff(), K_, nullptr);
}

// ---------------------------------------------------------------- Pooling
void PoolingLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                               const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  if (max_)
    gpu::pool_max_fwd(E.stream, bottom[0]->gpu_data(), N_, C_, H_, W_, kh_,
                      kw_, ph_, pw_, sh_, sw_, OH_, OW_,
                      top[0]->mutable_gpu_data(),
                      (int*)mask_.mutable_gpu_data());
  else
    gpu::pool_ave_fwd(E.stream, bottom[0]->gpu_data(), N_, C_, H_, W_, kh_,
                      kw_, ph_, pw_, sh_, sw_, OH_, OW_,
                      top[0]->mutable_gpu_data());
}

void PoolingLayer::Backward_gpu(const std::vector<Blob*>& top,
                                const std::vector<bool>& prop_down,
                                const std::vector<Blob*>& bottom) {
  if (!prop_down[0]) return;
  Engine& E = Engine::get();
  if (max_)
    gpu::pool_max_bwd(E.stream, top[0]->gpu_diff(),
                      (const int*)mask_.gpu_data(), N_, C_, H_, W_, kh_,
                      kw_, ph_, pw_, sh_, sw_, OH_, OW_,
                      bottom[0]->mutable_gpu_diff());
  else
    gpu::pool_ave_bwd(E.stream, top[0]->gpu_diff(), N_, C_, H_, W_, kh_,
                      kw_, ph_, pw_, sh_, sw_, OH_, OW_,
                      bottom[0]->mutable_gpu_diff());
}

// -------------------------------------------------------------------- BN
void BatchNormLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                                 const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  const int N = bottom[0]->num();
  const long S = bottom[0]->count() / ((long)N * C_);
  const float* x = bottom[0]->gpu_data();
  float* y = top[0]->mutable_gpu_data();
  const float* sc = scale_bias_ ? blobs_[3]->gpu_data() : nullptr;
  const float* bi = scale_bias_ ? blobs_[4]->gpu_data() : nullptr;
  if (top[0] == bottom[0] && phase_ == Phase::TRAIN) {
    // in-place BN: keep the original x for backward's x̂ recompute
    saved_x_.ReshapeLike(*bottom[0]);
    gpu::copy(E.stream, bottom[0]->count(), x, saved_x_.mutable_gpu_data());
    x = saved_x_.gpu_data();  // stats/norm read the stable copy
  }
  if (phase_ == Phase::TEST) {
    gpu::bn_fwd_test(E.stream, x, blobs_[0]->gpu_data(),
                     blobs_[1]->gpu_data(), sc, bi, scale_bias_, N, C_, S,
                     eps_, y);
    return;
  }
  const int nb = gpu::bn_blocks_per_channel(N, C_);
  partials_.Reshape({(int)(C_ * nb * 4)});  // double2 = 4 floats
  void* parts = partials_.mutable_gpu_data();
  gpu::bn_fwd_stats(E.stream, x, N, C_, S, nb, parts);
  // the finalize also advances the global statistics, which nothing else
  // in the TRAIN forward reads or writes
  gpu::bn_fwd_finalize(E.stream, parts, nb, C_, (long)N * S, eps_, maf_,
                       iter_ <= 1 ? 1 : 0, mean_.mutable_gpu_data(),
                       var_.mutable_gpu_data(), inv_std_.mutable_gpu_data(),
                       blobs_[0]->mutable_gpu_data(),
                       blobs_[1]->mutable_gpu_data());
  const float* add = nullptr;
  int frelu = fuse_relu_;
  if (fuse_add_out_) {  // fused residual add: write the sum's top directly
    y = fuse_add_out_->mutable_gpu_data();
    add = fuse_add_other_->gpu_data();
    frelu = fuse_add_relu_;
  }
  gpu::bn_fwd_norm(E.stream, x, mean_.gpu_data(), inv_std_.gpu_data(), sc,
                   bi, scale_bias_, N, C_, S, y, frelu, add);
  ++iter_;
}

void BatchNormLayer::Backward_gpu(const std::vector<Blob*>& top,
                                  const std::vector<bool>& prop_down,
                                  const std::vector<Blob*>& bottom) {
  Engine& E = Engine::get();
  const int N = bottom[0]->num();
  const long S = bottom[0]->count() / ((long)N * C_);
  const float* x = bwd_x(bottom, top, true);  // saved copy when in-place
  const float* dy = top[0]->gpu_diff();
  const int nb = gpu::bn_blocks_per_channel(N, C_);
  partials_.Reshape({(int)(C_ * nb * 4)});
  void* parts = partials_.mutable_gpu_data();
  // fused in-place ReLU backward: the activation's sign is recomputed
  // from xn*scale+bias inside the BN kernels (bit-identical to the
  // forward's op sequence) — no extra memory stream
  const float* sc_p = scale_bias_ ? blobs_[3]->gpu_data() : nullptr;
  const float* bi_p = scale_bias_ ? blobs_[4]->gpu_data() : nullptr;
  gpu::bn_bwd_stats(E.stream, x, dy, mean_.gpu_data(), inv_std_.gpu_data(),
                    N, C_, S, nb, sc_p, bi_p, fuse_relu_ ? 1 : 0, parts);
  gpu::bn_bwd_finalize(
      E.stream, parts, nb, C_, (long)N * S, sc_p, scale_bias_,
      scale_bias_ ? blobs_[3]->mutable_gpu_diff() : nullptr,
      scale_bias_ ? blobs_[4]->mutable_gpu_diff() : nullptr,
      m_dy_.mutable_gpu_data(), m_dyxn_.mutable_gpu_data());
  if (prop_down[0])
    gpu::bn_bwd_apply(E.stream, x, dy, mean_.gpu_data(),
                      inv_std_.gpu_data(), sc_p, scale_bias_,
                      m_dy_.gpu_data(), m_dyxn_.gpu_data(), N, C_, S, bi_p,
                      fuse_relu_ ? 1 : 0, bottom[0]->mutable_gpu_diff());
}

// ----------------------------------------------------------------- Scale
// Scale's and Bias's GPU constants + scratch, [zeros C][ones C][scratch 2C]
// (the scratch starts as ones too), filled when C changes
static float* zeros_ones(Blob& zo, int C) {
  if (zo.count() != 4 * C) {
    hipStream_t s = Engine::get().stream;
    zo.Reshape({4 * C});
    gpu::set_const(s, C, 0.f, zo.mutable_gpu_data());
    gpu::set_const(s, 3L * C, 1.f, zo.mutable_gpu_data() + C);
  }
  return zo.mutable_gpu_data();
}

void ScaleLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                             const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  const int N = bottom[0]->num();
  const long S = bottom[0]->count() / ((long)N * C_);
  if (bottom[0] == top[0]) {  // in-place: keep x for backward
    temp_.ReshapeLike(*bottom[0]);
    gpu::copy(E.stream, bottom[0]->count(), bottom[0]->gpu_data(),
              temp_.mutable_gpu_data());
  }
  gpu::chan_affine(E.stream, bottom[0]->gpu_data(), blobs_[0]->gpu_data(),
                   bias_ ? blobs_[1]->gpu_data() : nullptr, N, C_, S,
                   top[0]->mutable_gpu_data());
}

void ScaleLayer::Backward_gpu(const std::vector<Blob*>& top,
                              const std::vector<bool>& prop_down,
                              const std::vector<Blob*>& bottom) {
  Engine& E = Engine::get();
  const int N = bottom[0]->num();
  const long S = bottom[0]->count() / ((long)N * C_);
  const float* x = bottom[0] == top[0] ? temp_.gpu_data()
                                       : bottom[0]->gpu_data();
  const float* dy = top[0]->gpu_diff();
  // per-channel {sum dy, sum dy*x} via the BN bwd-stats reduction with
  // mean 0 / inv_std 1 (xn == x there); finalize writes dscale/dbias and
  // scratch means we ignore.
  float* zo = zeros_ones(zo_, C_);
  const int nb = gpu::bn_blocks_per_channel(N, C_);
  partials_.Reshape({(int)(C_ * nb * 4)});
  void* parts = partials_.mutable_gpu_data();
  gpu::bn_bwd_stats(E.stream, x, dy, /*mean=*/zo, /*inv_std=*/zo + C_, N,
                    C_, S, nb, nullptr, nullptr, 0, parts);
  gpu::bn_bwd_finalize(E.stream, parts, nb, C_, (long)N * S,
                       blobs_[0]->gpu_data(), 1,
                       blobs_[0]->mutable_gpu_diff(),
                       bias_ ? blobs_[1]->mutable_gpu_diff() : zo + 2 * C_,
                       zo + 2 * C_, zo + 3 * C_);
  if (prop_down[0])
    gpu::chan_affine(E.stream, dy, blobs_[0]->gpu_data(), nullptr, N, C_,
                     S, bottom[0]->mutable_gpu_diff());
}

// ------------------------------------------------------------------ Bias
void BiasLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                            const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  const int N = bottom[0]->num();
  const long S = bottom[0]->count() / ((long)N * C_);
  // y = x*1 + b[c]: the ones live in zo_
  gpu::chan_affine(E.stream, bottom[0]->gpu_data(), zeros_ones(zo_, C_) + C_,
                   blobs_[0]->gpu_data(), N, C_, S,
                   top[0]->mutable_gpu_data());
}

void BiasLayer::Backward_gpu(const std::vector<Blob*>& top,
                             const std::vector<bool>& prop_down,
                             const std::vector<Blob*>& bottom) {
  Engine& E = Engine::get();
  const int N = bottom[0]->num();
  const long S = bottom[0]->count() / ((long)N * C_);
  const float* dy = top[0]->gpu_diff();
  // db[c] = sum dy — reuse the deterministic conv bias-grad reduction
  gpu::bias_grad(E.stream, dy, N, C_, S, blobs_[0]->mutable_gpu_diff());
  if (prop_down[0]) {
    float* dx = bottom[0]->mutable_gpu_diff();
    if (dx != dy) gpu::copy(E.stream, bottom[0]->count(), dy, dx);
  }
}

// ------------------------------------------------------------------ ReLU
void ReLULayer::Forward_gpu(const std::vector<Blob*>& bottom,
                            const std::vector<Blob*>& top) {
  if (fused_away_) return;  // producer already applied the activation
  auto rp = param_->sub("relu_param");
  const float slope = rp ? (float)rp->num("negative_slope", 0) : 0.f;
  gpu::relu_fwd(Engine::get().stream, bottom[0]->gpu_data(),
                bottom[0]->count(), slope, top[0]->mutable_gpu_data());
}

void ReLULayer::Backward_gpu(const std::vector<Blob*>& top,
                             const std::vector<bool>& prop_down,
                             const std::vector<Blob*>& bottom) {
  if (!prop_down[0]) return;
  if (fused_away_ && bwd_fused_) return;  // absorbed into BN backward
  if (bwd_in_split_) return;  // the Split above already wrote our bottom diff
  const float slope = this->slope();
  // bwd_from_top_: the pre-activation was never materialized (fused
  // producer wrote post-ReLU into our top); for slope 0 the top's sign
  // is the same mask
  const float* ref =
      bwd_from_top_ ? top[0]->gpu_data() : bottom[0]->gpu_data();
  gpu::relu_bwd(Engine::get().stream, ref, top[0]->gpu_diff(),
                bottom[0]->count(), slope, bottom[0]->mutable_gpu_diff());
}

// ----------------------------------------------------------------- PReLU
void PReLULayer::Forward_gpu(const std::vector<Blob*>& bottom,
                             const std::vector<Blob*>& top) {
  // in-place: the one launch stores x to saved_x_ and y over x
  gpu::prelu_fwd(Engine::get().stream, geom_, plan_, bottom[0]->gpu_data(),
                 blobs_[0]->gpu_data(), top[0]->mutable_gpu_data(),
                 keeps_x(bottom, top) ? saved_x_.mutable_gpu_data() : nullptr);
}

void PReLULayer::Backward_gpu(const std::vector<Blob*>& top,
                              const std::vector<bool>& prop_down,
                              const std::vector<Blob*>& bottom) {
  gpu::prelu_bwd(Engine::get().stream, geom_, plan_, bwd_x(bottom, top, true),
                 top[0]->gpu_diff(), blobs_[0]->gpu_data(),
                 prop_down[0] ? bottom[0]->mutable_gpu_diff() : nullptr,
                 blobs_[0]->mutable_gpu_diff());
}

// --------------------------------------------------------------- Eltwise
void EltwiseLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                               const std::vector<Blob*>& top) {
  if (fused_away_) return;  // the producing BN already wrote bn(x)+other
  Engine& E = Engine::get();
  const long n = top[0]->count();
  float* y = top[0]->mutable_gpu_data();
  if (bottom.size() == 2 && unit_sum()) {
    gpu::add3(E.stream, n, bottom[0]->gpu_data(), bottom[1]->gpu_data(), y,
              fuse_relu_);
    return;
  }
  CHECK_(op_ == "SUM") << "Eltwise " << op_ << " has no GPU kernel";
  gpu::set_const(E.stream, n, 0.f, y);
  for (size_t i = 0; i < bottom.size(); ++i)
    gpu::axpby(E.stream, n, coeffs_[i], bottom[i]->gpu_data(), 1.f, y);
}

void EltwiseLayer::Backward_gpu(const std::vector<Blob*>& top,
                                const std::vector<bool>& prop_down,
                                const std::vector<Blob*>& bottom) {
  Engine& E = Engine::get();
  const long n = top[0]->count();
  CHECK_(op_ == "SUM") << "Eltwise " << op_ << " has no GPU kernel";
  const bool unit = unit_sum();
  for (size_t i = 0; i < bottom.size(); ++i) {
    // dx_i == dy exactly in a unit sum: nothing to launch for a bottom that
    // shares dy's memory (Net::plan_diff_sharing), a copy for one that
    // keeps its own
    if (!prop_down[i] || (unit && alias_diff_[i])) continue;
    const float* dy = top[0]->gpu_diff();
    float* dx = bottom[i]->mutable_gpu_diff();
    if (unit)
      gpu::copy(E.stream, n, dy, dx);
    else
      gpu::axpby(E.stream, n, coeffs_[i], dy, 0.f, dx);
  }
}

// ------------------------------------------------------------------- LRN
void LRNLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                           const std::vector<Blob*>& top) {
  if (within_) {
    gpu::lrn_within_fwd(Engine::get().stream, within_geom_, within_plan_,
                        bottom[0]->gpu_data(), scale_.mutable_gpu_data(),
                        top[0]->mutable_gpu_data());
    return;
  }
  gpu::lrn_fwd(Engine::get().stream, bottom[0]->gpu_data(),
               bottom[0]->num(), bottom[0]->channels(), bottom[0]->height(),
               bottom[0]->width(), size_, alpha_, beta_, k_,
               scale_.mutable_gpu_data(), top[0]->mutable_gpu_data());
}

void LRNLayer::Backward_gpu(const std::vector<Blob*>& top,
                            const std::vector<bool>& prop_down,
                            const std::vector<Blob*>& bottom) {
  if (!prop_down[0]) return;
  if (within_) {
    gpu::lrn_within_bwd(Engine::get().stream, within_geom_, within_plan_,
                        bottom[0]->gpu_data(), top[0]->gpu_diff(),
                        scale_.gpu_data(), bottom[0]->mutable_gpu_diff());
    return;
  }
  gpu::lrn_bwd(Engine::get().stream, bottom[0]->gpu_data(),
               top[0]->gpu_data(), top[0]->gpu_diff(), scale_.gpu_data(),
               bottom[0]->num(), bottom[0]->channels(), bottom[0]->height(),
               bottom[0]->width(), size_, alpha_, beta_,
               bottom[0]->mutable_gpu_diff());
}

// --------------------------------------------------------------- Dropout
void DropoutLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                               const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  const long n = bottom[0]->count();
  if (phase_ != Phase::TRAIN) {
    gpu::copy(E.stream, n, bottom[0]->gpu_data(),
              top[0]->mutable_gpu_data());
    return;
  }
  const uint64_t key =
      h_splitmix64(E.seed ^ 0xD0D0ull ^ ((uint64_t)E.rank << 40) ^
                   E.data_iter);
  gpu::dropout_fwd(E.stream, bottom[0]->gpu_data(), n, key, 0, ratio_,
                   scale_, top[0]->mutable_gpu_data(),
                   (uint8_t*)mask_.mutable_gpu_data());
  ++iter_;
}

void DropoutLayer::Backward_gpu(const std::vector<Blob*>& top,
                                const std::vector<bool>& prop_down,
                                const std::vector<Blob*>& bottom) {
  if (!prop_down[0]) return;
  Engine& E = Engine::get();
  const long n = bottom[0]->count();
  if (phase_ != Phase::TRAIN) {
    gpu::copy(E.stream, n, top[0]->gpu_diff(),
              bottom[0]->mutable_gpu_diff());
    return;
  }
  gpu::dropout_bwd(E.stream, top[0]->gpu_diff(),
                   (const uint8_t*)mask_.gpu_data(), n, scale_,
                   bottom[0]->mutable_gpu_diff());
}

// ---------------------------------------------------------------- Concat
void ConcatLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                              const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  const int N = top[0]->num(), Cd = top[0]->channels();
  const long S = top[0]->count(2);
  float* y = top[0]->mutable_gpu_data();
  int off = 0;
  for (auto* b : bottom) {
    gpu::concat_fwd(E.stream, b->gpu_data(), N, b->channels(), S, Cd, off,
                    y);
    off += b->channels();
  }
}

void ConcatLayer::Backward_gpu(const std::vector<Blob*>& top,
                               const std::vector<bool>& prop_down,
                               const std::vector<Blob*>& bottom) {
  Engine& E = Engine::get();
  const int N = top[0]->num(), Cd = top[0]->channels();
  const long S = top[0]->count(2);
  const float* dy = top[0]->gpu_diff();
  int off = 0;
  for (size_t i = 0; i < bottom.size(); ++i) {
    if (prop_down[i])
      gpu::concat_bwd(E.stream, dy, N, bottom[i]->channels(), S, Cd, off,
                      bottom[i]->mutable_gpu_diff());
    off += bottom[i]->channels();
  }
}

// ------------------------------------------------------- SoftmaxWithLoss
void SoftmaxLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                               const std::vector<Blob*>& top) {
  gpu::softmax_fwd(Engine::get().stream, bottom[0]->gpu_data(), outer_, C_,
                   inner_, top[0]->mutable_gpu_data());
}

void SoftmaxWithLossLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                                       const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  if (dense_) {
    gpu::dense_softmaxloss_fwd(
        E.stream, dense_geom(), bottom[0]->gpu_data(), bottom[1]->gpu_data(),
        prob_.mutable_gpu_data(),
        (double*)Workspace::get_global().get(
            Workspace::kLossPart, sizeof(double) * gpu::kDsmPartials),
        top[0]->mutable_gpu_data(),
        (float*)norm_slot_.reserve(2 * sizeof(float)));
    return;
  }
  gpu::softmax_fwd(E.stream, bottom[0]->gpu_data(), outer_, C_, inner_,
                   prob_.mutable_gpu_data());
  gpu::softmaxloss_fwd(E.stream, prob_.gpu_data(), bottom[1]->gpu_data(),
                       outer_, C_, inner_, top[0]->mutable_gpu_data());
}

void SoftmaxWithLossLayer::Backward_gpu(const std::vector<Blob*>& top,
                                        const std::vector<bool>& prop_down,
                                        const std::vector<Blob*>& bottom) {
  if (!prop_down[0]) return;
  if (dense_) {
    CHECK_GE_(norm_slot_.bytes, 2 * sizeof(float)) << "Backward before Forward";
    gpu::dense_softmaxloss_bwd(
        Engine::get().stream, dense_geom(), prob_.gpu_data(),
        bottom[1]->gpu_data(), (const float*)norm_slot_.p, loss(0),
        bottom[0]->mutable_gpu_diff());
    return;
  }
  const float scale = loss(0) / ((float)outer_ * inner_);
  gpu::softmaxloss_bwd(Engine::get().stream, prob_.gpu_data(),
                       bottom[1]->gpu_data(), outer_, C_, inner_, scale,
                       bottom[0]->mutable_gpu_diff());
  (void)top;
}

// ------------------------------------------------------------------- Crop
void CropLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                            const std::vector<Blob*>& top) {
  gpu::crop_fwd(Engine::get().stream, geom_, bottom[0]->gpu_data(),
                top[0]->mutable_gpu_data());
}

void CropLayer::Backward_gpu(const std::vector<Blob*>& top,
                             const std::vector<bool>& prop_down,
                             const std::vector<Blob*>& bottom) {
  if (!prop_down[0]) return;
  gpu::crop_bwd(Engine::get().stream, geom_, top[0]->gpu_diff(),
                bottom[0]->mutable_gpu_diff());
}

// ---------------------------------------------------------------- Sigmoid
void SigmoidLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                               const std::vector<Blob*>& top) {
  gpu::sigmoid_fwd(Engine::get().stream, bottom[0]->gpu_data(),
                   bottom[0]->count(), top[0]->mutable_gpu_data());
}

void SigmoidLayer::Backward_gpu(const std::vector<Blob*>& top,
                                const std::vector<bool>& prop_down,
                                const std::vector<Blob*>& bottom) {
  if (!prop_down[0]) return;
  gpu::sigmoid_bwd(Engine::get().stream, top[0]->gpu_data(),
                   top[0]->gpu_diff(), bottom[0]->count(),
                   bottom[0]->mutable_gpu_diff());
}

// ------------------------------------- SigmoidCrossEntropyLoss, Euclidean
static double* loss_partials_ws(long n) {
  return (double*)Workspace::get_global().get(
      Workspace::kLossPart, sizeof(double) * gpu::loss_partials(n));
}

void SigmoidCrossEntropyLossLayer::Forward_gpu(
    const std::vector<Blob*>& bottom, const std::vector<Blob*>& top) {
  const long n = bottom[0]->count();
  gpu::sigmoid_ce_fwd(Engine::get().stream, bottom[0]->gpu_data(),
                      bottom[1]->gpu_data(), n, bottom[0]->num(),
                      loss_partials_ws(n), top[0]->mutable_gpu_data());
}

void SigmoidCrossEntropyLossLayer::Backward_gpu(
    const std::vector<Blob*>&, const std::vector<bool>& prop_down,
    const std::vector<Blob*>& bottom) {
  if (!prop_down[0]) return;
  gpu::sigmoid_ce_bwd(Engine::get().stream, bottom[0]->gpu_data(),
                      bottom[1]->gpu_data(), bottom[0]->count(),
                      loss(0) / (float)bottom[0]->num(),
                      bottom[0]->mutable_gpu_diff());
}

void EuclideanLossLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                                     const std::vector<Blob*>& top) {
  const long n = bottom[0]->count();
  gpu::euclid_fwd(Engine::get().stream, bottom[0]->gpu_data(),
                  bottom[1]->gpu_data(), n, bottom[0]->num(),
                  loss_partials_ws(n), top[0]->mutable_gpu_data());
}

void EuclideanLossLayer::Backward_gpu(const std::vector<Blob*>&,
                                      const std::vector<bool>& prop_down,
                                      const std::vector<Blob*>& bottom) {
  if (!prop_down[0] && !prop_down[1]) return;
  gpu::euclid_bwd(
      Engine::get().stream, bottom[0]->gpu_data(), bottom[1]->gpu_data(),
      bottom[0]->count(), loss(0) / bottom[0]->num(),
      prop_down[0] ? bottom[0]->mutable_gpu_diff() : nullptr,
      -loss(0) / bottom[1]->num(),
      prop_down[1] ? bottom[1]->mutable_gpu_diff() : nullptr);
}

// -------------------------------------------------------- ContrastiveLoss
void ContrastiveLossLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                                       const std::vector<Blob*>& top) {
  const int N = bottom[0]->num(), C = bottom[0]->channels();
  double* partials = (double*)Workspace::get_global().get(
      Workspace::kLossPart, sizeof(double) * gpu::contrastive_partials(N, C));
  gpu::contrastive_fwd(Engine::get().stream, bottom[0]->gpu_data(),
                       bottom[1]->gpu_data(), bottom[2]->gpu_data(), N, C,
                       margin_, legacy_,
                       (float*)dist_sq_dev_.reserve(sizeof(float) * N),
                       partials, top[0]->mutable_gpu_data());
}

void ContrastiveLossLayer::Backward_gpu(const std::vector<Blob*>&,
                                        const std::vector<bool>& prop_down,
                                        const std::vector<Blob*>& bottom) {
  if (!prop_down[0] && !prop_down[1]) return;
  const int N = bottom[0]->num(), C = bottom[0]->channels();
  CHECK_GE_(dist_sq_dev_.bytes, sizeof(float) * N) << "Backward before Forward";
  gpu::contrastive_bwd(
      Engine::get().stream, bottom[0]->gpu_data(), bottom[1]->gpu_data(),
      bottom[2]->gpu_data(), (const float*)dist_sq_dev_.p, N, C, margin_,
      legacy_, loss(0) / (float)N,
      prop_down[0] ? bottom[0]->mutable_gpu_diff() : nullptr,
      prop_down[1] ? bottom[1]->mutable_gpu_diff() : nullptr);
}

// ---------------------------------------------------------------- Slice
void SliceLayer::Forward_gpu(const std::vector<Blob*>& bottom,
                             const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  const float* x = bottom[0]->gpu_data();
  int off = 0;
  for (auto* t : top) {
    const int Ct = t->shape(axis_);
    gpu::concat_bwd(E.stream, x, outer_, Ct, inner_, C_, off,
                    t->mutable_gpu_data());
    off += Ct;
  }
}

void SliceLayer::Backward_gpu(const std::vector<Blob*>& top,
                              const std::vector<bool>& prop_down,
                              const std::vector<Blob*>& bottom) {
  if (!prop_down[0]) return;
  Engine& E = Engine::get();
  float* dx = bottom[0]->mutable_gpu_diff();
  int off = 0;
  for (auto* t : top) {
    const int Ct = t->shape(axis_);
    gpu::concat_fwd(E.stream, t->gpu_diff(), outer_, Ct, inner_, C_, off, dx);
    off += Ct;
  }
}

}  // namespace camd
