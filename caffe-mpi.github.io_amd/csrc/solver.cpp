#include "solver.hpp"

#include <chrono>
#include <cmath>
#include <filesystem>
#include <fstream>

#include "proto_wire.hpp"

namespace camd {

namespace {
// registry names (reference SolverRegistry) and the deprecated enum idents
// (caffe.proto:288-295), both indexed by SolverRule
const char* const kTypeNames[kNumSolverRules] = {
    "SGD", "Nesterov", "AdaGrad", "RMSProp", "AdaDelta", "Adam"};
const char* const kEnumNames[kNumSolverRules] = {
    "SGD", "NESTEROV", "ADAGRAD", "RMSPROP", "ADADELTA", "ADAM"};

// CPU-mode update of one param: the per-element rule the GPU kernels run
template <int Rule, bool kL1>
void cpu_rule_loop(long n, float* g, float* w, float* h, float* h2,
                   const SolverCoef& c, float lr, float decay) {
  float unused = 0.f;
  for (long i = 0; i < n; ++i) {
    w[i] -= solver_rule_step<Rule, kL1>(g[i], w[i], h[i],
                                        h2 ? h2[i] : unused, c, lr, decay);
    g[i] = 0.f;
  }
}
void cpu_rule_update(int rule, bool l1, long n, float* g, float* w, float* h,
                     float* h2, const SolverCoef& c, float lr, float decay) {
#define CPU_RULE(R)                                              \
  case R:                                                        \
    if (l1)                                                      \
      cpu_rule_loop<R, true>(n, g, w, h, h2, c, lr, decay);      \
    else                                                         \
      cpu_rule_loop<R, false>(n, g, w, h, h2, c, lr, decay);     \
    break;
  switch (rule) {
    CPU_RULE(kRuleSgd)
    CPU_RULE(kRuleNesterov)
    CPU_RULE(kRuleAdaGrad)
    CPU_RULE(kRuleRmsProp)
    CPU_RULE(kRuleAdaDelta)
    CPU_RULE(kRuleAdam)
  }
#undef CPU_RULE
}
}  // namespace

// type / regularization_type and the rule's constants, checked once
// (reference: SolverRegistry::CreateSolver, the constructor_sanity_check of
// adagrad/rmsprop in sgd_solvers.hpp, upgrade_proto.cpp:1003 for the
// deprecated solver_type enum)
void Solver::parse_type() {
  const PMsg& sp = *param_;
  if (sp.has("type") && sp.has("solver_type"))
    CAMD_FATAL << "solver gives both type: \"" << sp.str("type")
               << "\" and the deprecated solver_type: "
               << sp.str("solver_type") << " — give type only";
  rule_ = -1;
  if (sp.has("solver_type")) {
    const std::string st = sp.str("solver_type");
    for (int r = 0; r < kNumSolverRules; ++r)
      // text format takes the enum by name or by number
      if (st == kEnumNames[r] || st == std::to_string(r)) rule_ = r;
    if (rule_ < 0)
      CAMD_FATAL << "unknown solver_type: " << st
                 << " (SGD | NESTEROV | ADAGRAD | RMSPROP | ADADELTA | ADAM)";
  } else {
    const std::string t = sp.str("type", "SGD");
    for (int r = 0; r < kNumSolverRules; ++r)
      if (t == kTypeNames[r]) rule_ = r;
    if (rule_ < 0)
      CAMD_FATAL << "unknown solver type: \"" << t
                 << "\" (SGD | Nesterov | AdaGrad | RMSProp | AdaDelta | Adam)";
  }
  type_name_ = kTypeNames[rule_];
  const std::string reg = sp.str("regularization_type", "L2");
  if (reg != "L1" && reg != "L2")
    CAMD_FATAL << "unknown regularization_type: \"" << reg
               << "\" (L1 | L2)";
  l1_ = reg == "L1";
  const float delta = (float)sp.num("delta", 1e-8);  // caffe.proto:272
  if ((rule_ == kRuleAdaGrad || rule_ == kRuleRmsProp) &&
      sp.num("momentum", 0.0) != 0.0)
    CAMD_FATAL << type_name_ << " solver requires momentum == 0, got momentum: "
               << sp.str("momentum");
  // the delta floors are the reference's own (solvers/*_solver.cpp)
  switch (rule_) {
    case kRuleAdaGrad:
      delta_ = std::max(delta, 1e-3f);
      break;
    case kRuleRmsProp: {
      const double rho = sp.num("rms_decay", 0.0);  // caffe.proto:278
      if (!(rho >= 0.0 && rho < 1.0))
        CAMD_FATAL << "RMSProp solver requires 0 <= rms_decay < 1, got "
                      "rms_decay: " << sp.str("rms_decay");
      aux_ = (float)rho;
      delta_ = std::max(delta, 1e-4f);
      break;
    }
    case kRuleAdaDelta:
      delta_ = std::max(delta, 1e-3f);
      break;
    case kRuleAdam:
      aux_ = (float)sp.num("momentum2", 0.999);  // caffe.proto:274
      delta_ = std::max(delta, 1e-4f);
      break;
    default:
      break;
  }
}

Solver::Solver(const PMsgPtr& sp, int batch_override) : param_(sp) {
  parse_type();
  PMsgPtr net_msg;
  if (sp->has("net")) {
    net_msg = parse_prototxt_file(sp->str("net"));
  } else if (sp->sub("net_param")) {
    net_msg = sp->sub("net_param");
  } else {
    CAMD_FATAL << "solver has no net";
  }
  net_msg_ = net_msg;
  // solver-pinned seed (models use random_seed; `caffe time` pins 1371)
  Engine& E = Engine::get();
  if (sp->has("random_seed")) {
    E.seed = (uint64_t)sp->inum("random_seed");
    E.cpu_rng.seed(E.seed + (uint64_t)E.rank);  // +rank: parallel.cpp:179-187
  }
  parse_states();
  net_.reset(new Net(net_msg, train_state_, batch_override));
  weight_decay_ = (float)sp->num("weight_decay", 0.0);
  clip_ = (float)sp->num("clip_gradients", -1.0);  // caffe.proto:243
  const long buckets = sp->inum("reduce_buckets", 6);  // caffe.proto:140
  bucket_budget_ =
      std::max<long>(1, net_->learnable_count() / std::max<long>(1, buckets));
  for (int slot = 0; slot < history_slots(); ++slot)
    history_[slot].alloc(net_->learnable_count());
  if (E.mode == Mode::GPU) tables_.build(*net_, clipping());
}

Solver::~Solver() { Engine::get().sync(); }

// Safe at construction: a param blob's device pointer is fixed once allocated
// (no param blob is reshaped after the net build, sharers were re-pointed
// during it, and every later write of the weights goes through the host copy
// into the same device memory).  This uploads the weights.
void Solver::UpdateTables::build(Net& net, bool clipping) {
  auto& params = net.learnable_params();
  nseg = (int)params.size();
  std::vector<long> offs(nseg);
  std::vector<float*> wps(nseg);
  std::vector<float> lrms(nseg), dcms(nseg);
  for (int i = 0; i < nseg; ++i) {
    offs[i] = params[i].offset;
    wps[i] = params[i].blob->mutable_gpu_data();
    lrms[i] = params[i].lr_mult;
    dcms[i] = params[i].decay_mult;
  }
  seg_off.upload(offs.data(), nseg * sizeof(long));
  w_ptrs.upload(wps.data(), nseg * sizeof(float*));
  lrs.upload(lrms.data(), nseg * sizeof(float));
  decays.upload(dcms.data(), nseg * sizeof(float));
  if (clipping && nseg > 0) {  // no params: no finalize ever writes a slot
    // a bucket's grid is at most the sum of its params' grids (ceil and the
    // block cap are both subadditive), so this holds any bucketing
    for (int i = 0; i < nseg; ++i)
      clip_partials_cap +=
          gpu::grad_sumsq_partials((long)padded(params[i].count));
    clip_partials.reserve(sizeof(double) * clip_partials_cap);
    clip_slot.reserve(2 * sizeof(float));
  }
}

void StateBuf::alloc(long count) {
  count_ = count;
  if (Engine::get().mode == Mode::GPU)
    dev_.reserve(sizeof(float) * count);
  else
    host_.resize(count);
  zero();
}

void StateBuf::zero() {
  if (dev_.p)
    HIP_CHECK(hipMemsetAsync(dev_.p, 0, sizeof(float) * count_,
                             Engine::get().stream));
  else
    std::fill(host_.begin(), host_.end(), 0.f);
}

void StateBuf::read(long offset, long count, float* out) {
  if (dev_.p)
    HIP_CHECK(hipMemcpy(out, dev_.as<float>() + offset, sizeof(float) * count,
                        hipMemcpyDeviceToHost));
  else
    memcpy(out, host_.data() + offset, sizeof(float) * count);
}

void StateBuf::write(long offset, const float* in, long count) {
  if (dev_.p)
    HIP_CHECK(hipMemcpy(dev_.as<float>() + offset, in, sizeof(float) * count,
                        hipMemcpyHostToDevice));
  else
    memcpy(host_.data() + offset, in, sizeof(float) * count);
}

// acc += diff (merge_back=false, after each non-final sub-pass) or
// diff += acc then zero acc (merge_back=true, after the final sub-pass)
void Solver::accumulate_diffs(bool merge_back) {
  Engine& E = Engine::get();
  const long total = net_->learnable_count();
  if (acc_.empty()) acc_.alloc(total);
  if (E.mode == Mode::GPU) {
    // the device diffs are one arena
    if (!merge_back)
      gpu::axpy(E.stream, total, 1.f, net_->diff_arena(), acc_.ptr());
    else
      gpu::axpy(E.stream, total, 1.f, acc_.ptr(), net_->diff_arena());
  } else {
    // the host diffs are per blob
    for (auto& p : net_->learnable_params()) {
      float* diff = p.blob->mutable_cpu_diff();
      float* acc = acc_.ptr() + p.offset;
      if (!merge_back)
        cpu::axpy(p.count, 1.f, diff, acc);
      else
        cpu::axpy(p.count, 1.f, acc, diff);
    }
  }
  if (merge_back) acc_.zero();
}

float Solver::GetLearningRate() const {
  // sgd_solver.cpp:24-66 (+ rampup :27-33)
  const double base_lr = param_->num("base_lr");
  const long rampup = param_->inum("rampup_interval", 0);
  if (iter_ < rampup) {
    const double r0 = param_->num("rampup_lr", 0.0);
    return (float)(r0 + (base_lr - r0) * ((double)iter_ / rampup));
  }
  const std::string policy = param_->str("lr_policy", "fixed");
  if (policy == "fixed") return (float)base_lr;
  if (policy == "step") {
    const long step = iter_ / std::max<long>(1, param_->inum("stepsize", 1));
    return (float)(base_lr * std::pow(param_->num("gamma", 0.1), step));
  }
  if (policy == "exp")
    return (float)(base_lr * std::pow(param_->num("gamma", 0.1), iter_));
  if (policy == "inv")
    return (float)(base_lr *
                   std::pow(1.0 + param_->num("gamma") * iter_,
                            -param_->num("power")));
  if (policy == "multistep") {
    auto sv = param_->inums("stepvalue");
    while (current_step_ < (int)sv.size() && iter_ >= sv[current_step_])
      ++current_step_;
    return (float)(base_lr *
                   std::pow(param_->num("gamma", 0.1), current_step_));
  }
  if (policy == "poly") {
    const double min_lr = param_->num("min_lr", 0.0);
    return (float)(min_lr +
                   (base_lr - min_lr) *
                       std::pow(1.0 - (double)iter_ /
                                          param_->num("max_iter", 1),
                                param_->num("power")));
  }
  if (policy == "sigmoid")
    return (float)(base_lr /
                   (1.0 + std::exp(-param_->num("gamma") *
                                   (double)(iter_ -
                                            param_->inum("stepsize")))));
  CAMD_FATAL << "unknown lr_policy " << policy;
}

void Solver::bcast_weights() {
  if (!comm_ || comm_->world() < 2) return;
  Engine& E = Engine::get();
  for (auto& p : net_->learnable_params()) {
    float* ptr = E.mode == Mode::GPU ? p.blob->mutable_gpu_data()
                                     : p.blob->mutable_cpu_data();
    comm_->bcast(ptr, p.count, 0, E.stream);
  }
  E.sync();
}

void Reducer::start_iteration() {
  bucket_start_ = bucket_end_ = 0;
  deferred_.clear();
  partials_ = 0;
  sumsq_ = 0.0;
}

std::pair<long, long> Reducer::range(long begin, long end) const {
  auto& params = solver_->net().learnable_params();
  const auto& last = params[end - 1];
  return {params[begin].offset, last.offset + (long)padded(last.count)};
}

void Reducer::param_ready(int param_id, hipEvent_t done) {
  CHECK_EQ_((long)param_id, bucket_end_) << "params must arrive in order";
  bucket_end_ = param_id + 1;
  const auto [lo, hi] = range(bucket_start_, bucket_end_);
  if (hi - lo >= solver_->bucket_budget_) flush(done);
}

void Reducer::flush(hipEvent_t ev) {
  if (bucket_end_ == bucket_start_) return;
  Solver& S = *solver_;
  Engine& E = Engine::get();
  auto& params = S.net().learnable_params();
  const auto [lo, hi] = range(bucket_start_, bucket_end_);
  if (E.mode == Mode::GPU) {
    if (ev) HIP_CHECK(hipStreamWaitEvent(E.comm_stream, ev, 0));
    if (S.world() > 1) {
      PerfScope ps("allreduce", E.comm_stream, 0, 2.0 * (hi - lo) * 4);
      S.comm_->allreduce(S.net().diff_arena() + lo, hi - lo, E.comm_stream);
    }
    if (S.clipping()) {
      // the bucket's share of the global norm, behind its all-reduce on the
      // comm stream; its update waits for the factor (iteration_end)
      const int nb = gpu::grad_sumsq_partials(hi - lo);
      CHECK_LE_(partials_ + nb, S.tables_.clip_partials_cap);
      partials_ += gpu::grad_sumsq(
          E.comm_stream, S.net().diff_arena(), lo, hi,
          S.tables_.clip_partials.as<double>() + partials_);
    }
  } else {
    if (S.world() > 1) {
      // CPU buckets: gather the param diffs into one flat range is
      // unnecessary — host diffs are per-blob; reduce each param
      for (long k = bucket_start_; k < bucket_end_; ++k)
        S.comm_->allreduce(params[k].blob->mutable_cpu_diff(),
                           params[k].count, nullptr);
    }
    if (S.clipping())
      // each square and each add in double, per param in learnable order
      for (long k = bucket_start_; k < bucket_end_; ++k) {
        const float* g = params[k].blob->cpu_diff();
        double sum = 0.0;
        for (long i = 0; i < params[k].count; ++i)
          sum += (double)g[i] * (double)g[i];
        sumsq_ += sum;
      }
  }
  if (S.clipping())
    deferred_.emplace_back(bucket_start_, bucket_end_);
  else
    update(bucket_start_, bucket_end_);
  bucket_start_ = bucket_end_;
}

// One bucket's update: params [begin, end).  Without clip_gradients it runs
// straight from flush; with it, from iteration_end once the factor is known
// (on the device in GPU mode, in coef() in CPU mode).
void Reducer::update(long begin, long end) {
  Solver& S = *solver_;
  Engine& E = Engine::get();
  auto& params = S.net().learnable_params();
  if (E.mode == Mode::GPU) {
    const auto [lo, hi] = range(begin, end);
    const Solver::UpdateTables& T = S.tables_;
    const float* factor =
        S.clipping() ? T.clip_slot.as<const float>() + 1 : nullptr;
    // the kernel writes the weights through the table's cached pointers,
    // behind the blobs' backs: mark each blob's device copy as the newer
    // one, or a host copy made by an earlier read (param get, snapshot)
    // would be served again, stale, after this update
    for (long k = begin; k < end; ++k)
      params[k].blob->mutable_gpu_data();
    // bucket-fused update: one launch over the flat arena range
    if (S.rule_ == kRuleSgd && !S.l1_)
      gpu::sgd_update_segmented(
          E.comm_stream, lo, hi, S.net().diff_arena(), S.history(),
          T.seg_off.as<long>(), T.w_ptrs.as<float*>(), T.lrs.as<float>(),
          T.decays.as<float>(), T.nseg, S.cur_mom_, S.cur_lr_,
          S.weight_decay_, S.grad_scale_, factor);
    else
      gpu::solver_update_segmented(
          E.comm_stream, S.rule_, S.l1_, lo, hi, S.net().diff_arena(),
          S.history(0), S.history(1), T.seg_off.as<long>(),
          T.w_ptrs.as<float*>(), T.lrs.as<float>(), T.decays.as<float>(),
          T.nseg, S.coef(), factor);
  } else {
    for (long k = begin; k < end; ++k) {
      const auto& p = params[k];
      float* g = p.blob->mutable_cpu_diff();
      float* w = p.blob->mutable_cpu_data();
      float* h = S.history(0) + p.offset;
      float* h2 = S.history_slots() == 2 ? S.history(1) + p.offset : nullptr;
      cpu_rule_update(S.rule_, S.l1_, p.count, g, w, h, h2, S.coef(),
                      S.upd_lr_ * p.lr_mult, S.weight_decay_ * p.decay_mult);
    }
  }
}

void Reducer::iteration_end(hipEvent_t backward_done) {
  flush(backward_done);
  Engine& E = Engine::get();
  Solver& S = *solver_;
  if (S.clipping()) {
    if (E.mode == Mode::GPU) {
      // (a net without learnable params has no bucket and no launch)
      if (partials_ > 0)
        gpu::clip_finalize(E.comm_stream,
                           S.tables_.clip_partials.as<const double>(),
                           partials_, S.world(), S.clip_,
                           S.tables_.clip_slot.as<float>());
    } else {
      S.clip_norm_ = (float)(std::sqrt(sumsq_) / S.world());
      S.clip_factor_ = clip_factor(S.clip_norm_, S.clip_);
    }
    for (const auto& b : deferred_) update(b.first, b.second);
    deferred_.clear();
    ++S.clip_iters_;
  }
  if (E.mode == Mode::GPU) {
    comm_done_ev_.create();
    HIP_CHECK(hipEventRecord(comm_done_ev_.get(), E.comm_stream));
    // next iteration's forward must see the updated weights
    HIP_CHECK(hipStreamWaitEvent(E.stream, comm_done_ev_.get(), 0));
  }
}

void Solver::Step(int iters) {
  Engine& E = Engine::get();
  using clock = std::chrono::steady_clock;
  const long display = param_->inum("display", 0);
  const long test_interval = param_->inum("test_interval", 0);
  const long snap_interval = param_->inum("snapshot", 0);
  // gradient accumulation: iter_size fwd/bwd passes per update, diffs
  // accumulate in the arena, one reduce+update scaled by 1/iter_size
  // (reference solver.cpp:279-297 Step loop + SGDSolver::Normalize)
  const long iter_size = std::max<long>(1, param_->inum("iter_size", 1));
  // this fork always runs a 1-iter test at iter 0 regardless of
  // test_initialization (reference solver.cpp:243-248)
  if (iter_ == 0 && test_interval > 0 && test_net()) TestAll(1);
  // reference-style perf accounting (solver.cpp:299 skips warmup): the
  // first Step call (warmup/compile) is excluded; later calls are timed at
  // call granularity with a single sync so the launch-ahead pipeline stays
  // intact (no per-iteration host synchronization in this engine)
  const bool timed = skipped_iters_ > 0;
  std::chrono::time_point<clock> tstep0;
  if (timed) {
    E.sync();
    tstep0 = clock::now();
  }
  int done_iters = 0;
  for (int i = 0; i < iters; ++i) {
    if (action_fn_) {
      const SolverAction a = action_fn_();
      if (a == SolverAction::SNAPSHOT) {
        if (snapshot_enabled_) Snapshot();
      } else if (a == SolverAction::STOP) {
        early_exit_ = true;
        break;
      }
    }
    if (test_interval > 0 && iter_ > 0 && iter_ % test_interval == 0 &&
        test_net())
      TestAll();
    cur_lr_ = GetLearningRate();
    cur_mom_ = GetMomentum();
    upd_lr_ = cur_lr_;
    if (rule_ == kRuleAdam) {
      // bias correction at t = iter_ + 1, in float, once per iteration and
      // folded into the rate (adam_solver.cpp:42-43); iter_ comes back from
      // Restore, so a resumed run continues the same sequence
      const float t = (float)(iter_ + 1);
      upd_lr_ *= std::sqrt(1.f - std::pow(aux_, t)) /
                 (1.f - std::pow(cur_mom_, t));
    }
    grad_scale_ = 1.f / ((float)world() * (float)iter_size);
    reducer_.start_iteration();
    if (iter_size == 1) {
      E.data_iter = (uint64_t)iter_;
      net_->Forward();
      net_->Backward(&reducer_);
    } else {
      // layer backwards overwrite their param diffs, so the accumulation
      // runs hookless with a side buffer; the reducer is driven once at
      // the end (overlap is moot — sub-passes serialize by construction)
      for (long sub = 0; sub < iter_size; ++sub) {
        // sub-iteration granularity: each pass sees a fresh synthetic batch
        E.data_iter = (uint64_t)(iter_ * iter_size + sub);
        net_->Forward();
        net_->Backward(nullptr);
        if (sub + 1 < iter_size) accumulate_diffs(false);
      }
      accumulate_diffs(true);
      E.sync();  // diffs final on E.stream before comm_stream consumes them
      const int nparams = (int)net_->learnable_params().size();
      for (int k = 0; k < nparams; ++k) reducer_.param_ready(k, nullptr);
      reducer_.iteration_end(nullptr);
    }
    ++iter_;
    ++done_iters;
    if (snap_interval > 0 && iter_ % snap_interval == 0 &&
        snapshot_enabled_)
      Snapshot();
    if (display > 0 && iter_ % display == 0) {
      const float l = net_->loss();
      fprintf(stderr, "[caffe_amd] Iteration %ld, loss = %g, lr = %g\n",
              iter_, l, cur_lr_);
      if (clipping()) report_clipping();
    }
  }
  if (timed) {
    E.sync();
    perf_seconds_ +=
        std::chrono::duration<double>(clock::now() - tstep0).count();
    perf_iters_ += done_iters;
  } else {
    skipped_iters_ += done_iters;
  }
}

void Solver::copy_history(int slot, int param_index, float* out, long count) {
  CHECK_(slot >= 0 && slot < history_slots())
      << "history slot " << slot << " of this " << type_name_ << " solver ("
      << history_slots() << " slots)";
  auto& params = net_->learnable_params();
  CHECK_(param_index >= 0 && param_index < (int)params.size())
      << "param index " << param_index;
  const auto& p = params[param_index];
  CHECK_LE_(count, p.count);
  Engine::get().sync();  // the updates run on comm_stream
  history_[slot].read(p.offset, count, out);
}

void Solver::grad_norm(float* norm, float* factor) {
  CHECK_(clipping()) << "grad_norm: this solver has no clip_gradients "
                        "(the norm is computed only for clipping)";
  CHECK_(clip_iters_ > 0) << "grad_norm: no iteration has finished yet";
  Engine& E = Engine::get();
  float nf[2] = {clip_norm_, clip_factor_};
  if (E.mode == Mode::GPU && tables_.clip_slot.p) {
    // the finalize and the updates run on the comm stream
    HIP_CHECK(hipStreamSynchronize(E.comm_stream));
    HIP_CHECK(hipMemcpy(nf, tables_.clip_slot.p, sizeof(nf),
                        hipMemcpyDeviceToHost));
  }
  *norm = nf[0];
  *factor = nf[1];
}

// the reference's line (sgd_solver.cpp:122-125), on display iterations only:
// Step reads the loss back there anyway
void Solver::report_clipping() {
  float norm = 0.f, factor = 1.f;
  grad_norm(&norm, &factor);
  if (norm > clip_)
    fprintf(stderr,
            "[caffe_amd] Gradient clipping: scaling down gradients (L2 norm "
            "%g > %g) by scale factor %g\n",
            norm, clip_, factor);
}

std::shared_ptr<Solver> create_solver_from_file(const std::string& path,
                                                int batch_override) {
  return std::make_shared<Solver>(parse_prototxt_file(path), batch_override);
}

long Solver::train_batch() const {
  for (auto& l : net_->layers())
    if (auto* d = dynamic_cast<const DataLayer*>(l.get())) return d->batch_;
  return 0;
}

double Solver::perf_img_per_sec() const {
  if (perf_iters_ == 0 || perf_seconds_ <= 0) return 0.0;
  return perf_iters_ / perf_seconds_ * train_batch();
}

void Solver::print_perf_report() const {
  if (perf_iters_ == 0 || perf_seconds_ <= 0) return;
  const long batch = train_batch();
  const double ratio = perf_iters_ / perf_seconds_;
  fprintf(stderr,
          "Solver performance on device %d: %.4g * %ld = %.5g img/sec\n",
          Engine::get().device, ratio, batch, ratio * batch);
}

// train_state and every test_state of the solver file (reference
// Solver::InitTrainNet / InitTestNets: the phase is fixed, level and stages
// come from the state message), and the test_iter of every test net
void Solver::parse_states() {
  auto read = [](const PMsgPtr& m, Phase phase) {
    NetState st;
    st.phase = phase;
    if (m) {
      st.level = (int)m->inum("level", 0);
      st.stages = m->strs("stage");
    }
    return st;
  };
  train_state_ = read(param_->sub("train_state"), Phase::TRAIN);
  for (auto& m : param_->subs("test_state"))
    test_states_.push_back(read(m, Phase::TEST));
  test_iters_ = param_->inums("test_iter");
  if (!test_states_.empty()) {
    if (test_iters_.size() != test_states_.size())
      CAMD_FATAL << "solver gives " << test_states_.size()
                 << " test_state entries but " << test_iters_.size()
                 << " test_iter entries: test_iter must be given once per "
                    "test net";
  } else {
    // no test_state: at most one default TEST net, one test_iter (default 1)
    if (test_iters_.size() > 1)
      CAMD_FATAL << "solver gives " << test_iters_.size()
                 << " test_iter entries but 1 test net (no test_state): "
                    "test_iter must be given once per test net";
    if (test_iters_.empty()) test_iters_.push_back(1);
  }
}

int Solver::num_test_nets() {
  if (!test_nets_built_) {
    test_nets_built_ = true;
    std::vector<NetState> states = test_states_;
    if (states.empty()) {
      // only build when the net defines TEST-phase layers
      bool has_test = false;
      for (auto& lm : net_msg_->subs("layer")) {
        for (auto& inc : lm->subs("include"))
          if (inc->str("phase") == "TEST") has_test = true;
      }
      if (has_test) {
        NetState st;
        st.phase = Phase::TEST;
        states.push_back(st);
      }
    }
    for (auto& st : states) {
      test_nets_.emplace_back(new Net(net_msg_, st));
      test_nets_.back()->ShareTrainedLayersWith(*net_);
    }
  }
  return (int)test_nets_.size();
}

Net* Solver::test_net(int i) {
  return i >= 0 && i < num_test_nets() ? test_nets_[i].get() : nullptr;
}

void Solver::TestAll(long iters_override) {
  // reference: the test pass runs on the root solver only (solver.cpp:439;
  // cross-rank SharedScores aggregation is multi-node machinery)
  if (Engine::get().rank != 0) return;
  const int n = num_test_nets();
  for (int i = 0; i < n; ++i) {
    if (n > 1)
      fprintf(stderr, "[caffe_amd] Iteration %ld, Testing net (#%d)\n", iter_,
              i);
    const long iters = iters_override > 0 ? iters_override : test_iters_[i];
    // average every scored top over the test iterations (reference
    // Solver::Test, solver.cpp:439-540)
    for (auto& sc : test_nets_[i]->test_scores(iters)) {
      fprintf(stderr, "[caffe_amd] Test net output: %s = %g\n",
              sc.label.c_str(), sc.value);
      if (!std::isfinite(sc.value))
        fprintf(stderr,
                "[caffe_amd] WARNING: non-finite test score for %s — the net "
                "is diverging (or untrained BN stats at iter 0)\n",
                sc.label.c_str());
    }
  }
}

void Solver::Snapshot() {
  const std::string prefix = param_->str("snapshot_prefix", "snapshot");
  const std::string model =
      prefix + "_iter_" + std::to_string(iter_) + ".caffemodel";
  const std::string state =
      prefix + "_iter_" + std::to_string(iter_) + ".solverstate";
  net_->SaveWeights(model);
  // SolverState { iter=1, learned_net=2, history=3 (BlobProto),
  // current_step=4 } — caffe.proto:303-308
  wire::Writer sw;
  sw.vint(1, iter_);
  sw.str(2, model);
  std::vector<float> host;
  // history blobs go out in FORWARD learnable-param order — the order the
  // reference writes (sgd_solver.cpp:262-353); the arena itself is
  // reverse-layer order, so walk the permutation.  The two-slot rules
  // write slot 0 of every param, then slot 1 of every param — the
  // reference's history_[i + N] (adam_solver.cpp:37-39)
  auto& aparams = net_->learnable_params();
  for (int slot = 0; slot < history_slots(); ++slot)
    for (int pi : net_->forward_param_order()) {
      const auto& p = aparams[pi];
      host.resize(p.count);
      history_[slot].read(p.offset, p.count, host.data());
      sw.blob(3, host.data(), p.count, p.blob->shape());
    }
  sw.vint(4, current_step_);
  {
    const auto dir = std::filesystem::path(state).parent_path();
    if (!dir.empty()) std::filesystem::create_directories(dir);
  }
  std::ofstream f(state, std::ios::binary);
  CHECK_(f.good()) << "cannot write " << state;
  f.write(sw.out.data(), (long)sw.out.size());
  fprintf(stderr, "[caffe_amd] Snapshotting to %s\n", model.c_str());
}

void Solver::Restore(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  CHECK_(f.good()) << "cannot read " << path;
  std::string buf((std::istreambuf_iterator<char>(f)),
                  std::istreambuf_iterator<char>());
  wire::Reader r(buf.data(), buf.size());
  wire::Field fld;
  std::string learned;
  size_t hidx = 0;
  auto& params = net_->learnable_params();
  // the wire carries history in forward learnable-param order (reference
  // sgd_solver.cpp:307-353) — map each blob back to its arena slot
  const std::vector<int> order = net_->forward_param_order();
  const size_t nparams = order.size();
  if (rule_ != kRuleSgd) {
    // the other solvers take exactly slots * N blobs (reference
    // sgd_solver.cpp RestoreSolverStateFromBinaryProto); checked before
    // anything is overwritten
    size_t nhist = 0;
    wire::Reader count_r(buf.data(), buf.size());
    while (count_r.next(&fld))
      if (fld.num == 3 && fld.wt == 2) ++nhist;
    if (nhist != (size_t)history_slots() * nparams)
      CAMD_FATAL << "Incorrect length of history blobs: " << path << " has "
                 << nhist << ", this " << type_name_ << " solver of "
                 << nparams << " params takes " << history_slots() * nparams;
  }
  while (r.next(&fld)) {
    if (fld.num == 1 && fld.wt == 0) iter_ = (long)fld.vint;
    else if (fld.num == 2 && fld.wt == 2) learned.assign(fld.data, fld.len);
    else if (fld.num == 4 && fld.wt == 0) current_step_ = (int)fld.vint;
    else if (fld.num == 3 && fld.wt == 2) {
      auto b = wire::parse_blob(fld.data, fld.len);
      CHECK_LT_(hidx, nparams * history_slots());
      const int slot = (int)(hidx / nparams);
      const auto& p = params[order[hidx % nparams]];
      CHECK_EQ_((long)b.data.size(), p.count);
      history_[slot].write(p.offset, b.data.data(), p.count);
      ++hidx;
    }
  }
  if (!learned.empty()) net_->LoadWeights(learned);
  fprintf(stderr, "[caffe_amd] Restored iter %ld from %s\n", iter_,
          path.c_str());
}

}  // namespace camd
