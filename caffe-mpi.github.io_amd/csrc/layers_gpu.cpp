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

void DataLayer::Forward_gpu(const std::vector<Blob*>&,
                            const std::vector<Blob*>& top) {
  if (feed_) {
    forward_lmdb_gpu(top);
    ++iter_;
    return;
  }
  Engine& E = Engine::get();
  const uint64_t key =
      h_splitmix64(E.seed ^ ((uint64_t)E.rank << 40) ^ (E.data_iter << 8));
  gpu::fill_uniform(E.stream, top[0]->count(), key, 0, -1.f, 1.f,
                    top[0]->mutable_gpu_data());
  if (top.size() > 1)
    gpu::fill_labels(E.stream, top[1]->count(), key, 0, E.syn_classes,
                     top[1]->mutable_gpu_data());
  ++iter_;
}

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
void ConvolutionLayer::plan_gpu() {
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
  const int K = C_ / group_ * kh_ * kw_;
  const long NS = (long)N_ * Spad_;
  const float* x = bottom[0]->gpu_data();
  const float* w = blobs_[0]->gpu_data();
  const float* bias = bias_ ? blobs_[1]->gpu_data() : nullptr;
  float* y = top[0]->mutable_gpu_data();

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
  const ConvGroup o = conv_group(*this, NS);
  for (int g = 0; g < group_; ++g) {
    epi.bias = bias ? bias + g * o.bias : nullptr;
    gpu::gemm(E.stream, false, false, Cout_ / group_, NS, K, 1.f,
              w + g * o.w, K, b + g * (col ? o.col : o.x), col ? NS : 0, 0.f,
              y + g * o.y, S_, &epi, nullptr, col ? nullptr : &xv);
  }
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
  for (int g = 0; g < group_; ++g)
    gpu::gemm(E.stream, false, true, Cout_ / group_, K, NS, 1.f,
              dy + g * o.y, 0, b + g * (col ? o.col : o.x), col ? NS : 0,
              0.f, dw + g * o.w, K, nullptr, &dyv, col ? nullptr : &xv);
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
  }
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
  gpu::bn_fwd_finalize(E.stream, parts, nb, C_, (long)N * S, eps_,
                       mean_.mutable_gpu_data(), var_.mutable_gpu_data(),
                       inv_std_.mutable_gpu_data());
  const float* add = nullptr;
  int frelu = fuse_relu_;
  if (fuse_add_out_) {  // fused residual add: write the sum's top directly
    y = fuse_add_out_->mutable_gpu_data();
    add = fuse_add_other_->gpu_data();
    frelu = fuse_add_relu_;
  }
  gpu::bn_fwd_norm(E.stream, x, mean_.gpu_data(), inv_std_.gpu_data(), sc,
                   bi, scale_bias_, N, C_, S, y, frelu, add);
  gpu::bn_moving_avg(E.stream, mean_.gpu_data(), var_.gpu_data(), C_, maf_,
                     iter_ <= 1 ? 1 : 0, blobs_[0]->mutable_gpu_data(),
                     blobs_[1]->mutable_gpu_data());
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
  auto rp = param_->sub("relu_param");
  const float slope = rp ? (float)rp->num("negative_slope", 0) : 0.f;
  // bwd_from_top_: the pre-activation was never materialized (fused
  // producer wrote post-ReLU into our top); for slope 0 the top's sign
  // is the same mask
  const float* ref =
      bwd_from_top_ ? top[0]->gpu_data() : bottom[0]->gpu_data();
  gpu::relu_bwd(Engine::get().stream, ref, top[0]->gpu_diff(),
                bottom[0]->count(), slope, bottom[0]->mutable_gpu_diff());
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
  gpu::lrn_fwd(Engine::get().stream, bottom[0]->gpu_data(),
               bottom[0]->num(), bottom[0]->channels(), bottom[0]->height(),
               bottom[0]->width(), size_, alpha_, beta_, k_,
               scale_.mutable_gpu_data(), top[0]->mutable_gpu_data());
}

void LRNLayer::Backward_gpu(const std::vector<Blob*>& top,
                            const std::vector<bool>& prop_down,
                            const std::vector<Blob*>& bottom) {
  if (!prop_down[0]) return;
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
  gpu::softmax_fwd(E.stream, bottom[0]->gpu_data(), outer_, C_, inner_,
                   prob_.mutable_gpu_data());
  gpu::softmaxloss_fwd(E.stream, prob_.gpu_data(), bottom[1]->gpu_data(),
                       outer_, C_, inner_, top[0]->mutable_gpu_data());
}

void SoftmaxWithLossLayer::Backward_gpu(const std::vector<Blob*>& top,
                                        const std::vector<bool>& prop_down,
                                        const std::vector<Blob*>& bottom) {
  if (!prop_down[0]) return;
  const float scale = loss(0) / ((float)outer_ * inner_);
  gpu::softmaxloss_bwd(Engine::get().stream, prob_.gpu_data(),
                       bottom[1]->gpu_data(), outer_, C_, inner_, scale,
                       bottom[0]->mutable_gpu_diff());
  (void)top;
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
