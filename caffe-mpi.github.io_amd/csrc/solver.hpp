// solver.hpp — the solver (SGD, Nesterov, AdaGrad, RMSProp, AdaDelta, Adam)
// + the bucketed gradient reducer.
//
// Reference semantics: solver.cpp Step :187-353, sgd_solver.cpp lr/momentum
// policies :24-91 and fused update :143-149 / sgd_solver.cu:10-20; the other
// update rules solvers/{nesterov,adagrad,rmsprop,adadelta,adam}_solver.*;
// Net::ReduceAndUpdate bucketing net.cpp:757-877 (reduce_buckets default 6,
// caffe.proto:140).  MI355X re-design: the reduce thread is replaced by
// launch-chaining — each bucket's ncclAllReduce (RCCL over xGMI) and the
// per-param fused SGD updates are enqueued on the side comm stream behind a
// hipEvent recorded after the producing layer's backward, so the collective
// overlaps the rest of backward exactly as the reference's thread did, with
// no host synchronization in the loop.
//
// clip_gradients (caffe.proto:241-243, SGDSolver::ClipGradients
// sgd_solver.cpp:111-128) needs the norm of the whole reduced gradient, known
// only after the last bucket: with the field set, a bucket's flush still
// runs its all-reduce at once and follows it with the bucket's sum of
// squares instead of its update; iteration_end launches the finalize
// ({norm, factor} into a device slot) and then the deferred updates, which
// read the factor from device memory.  Still no host wait in the loop.
#pragma once

#include "net.hpp"

namespace camd {

// communicator abstraction: RCCL on GPU, host callback for gloo-based CPU
// tests (tests/test_dist_cpu.py), none for single-GPU
struct Comm {
  virtual void allreduce(float* buf, long count, hipStream_t s) = 0;
  virtual int world() const = 0;
  virtual void bcast(float* buf, long count, int root, hipStream_t s) = 0;
  virtual ~Comm() = default;
};

void rccl_unique_id(void* out_bytes128);
// multi-node uid bootstrap over TCP (csrc/bootstrap.cpp — the reference's
// Clusters/MPI_Bcast replacement, clusters.cpp + parallel.cpp:42-45)
int uid_serve(const void* payload, int len, int port, int nclients);
int uid_fetch(void* out, int len, const char* host, int port,
              int timeout_s);
int rccl_selftest();  // world-1 RCCL linkage/call smoke (GPU mode)
std::unique_ptr<Comm> make_rccl_comm(int rank, int world,
                                     const void* uid_bytes128);
using HostAllreduceFn = void (*)(float*, long, void*);
std::unique_ptr<Comm> make_callback_comm(HostAllreduceFn fn, void* ud,
                                         int world);

class Solver;

// Solver state in diff-arena layout (SGD history, the iter_size
// accumulator): zero-filled floats that live on the device in GPU mode and
// in a host vector in CPU mode.  The device side is a DeviceBuf: the solver
// that owns it waits before it goes back to the allocator.
class StateBuf {
 public:
  void alloc(long count);  // once; zero-filled on the compute stream
  bool empty() const { return count_ == 0; }
  // null while empty
  float* ptr() { return dev_.p ? dev_.as<float>() : host_.data(); }
  // blocking copies out of and into [offset, offset + count)
  void read(long offset, long count, float* out);
  void write(long offset, const float* in, long count);
  void zero();  // on the compute stream

 private:
  DeviceBuf dev_;
  std::vector<float> host_;
  long count_ = 0;
};

// reference SolverAction (include/caffe/solver.hpp + util/signal_handler):
// polled once per iteration inside Step — NONE continue, STOP break out
// (requested_early_exit_), SNAPSHOT snapshot and continue
enum class SolverAction { NONE = 0, STOP = 1, SNAPSHOT = 2 };
using ActionRequestFn = SolverAction (*)();

class Reducer : public ReduceHook {
 public:
  Reducer(Solver* s) : solver_(s) {}
  void start_iteration();
  void param_ready(int param_id, hipEvent_t done) override;
  void iteration_end(hipEvent_t backward_done) override;

 private:
  void flush(hipEvent_t ev);
  // the update of params [begin, end), one bucket
  void update(long begin, long end);
  // the padded arena range [lo, hi) of params [begin, end), one bucket
  std::pair<long, long> range(long begin, long end) const;
  Solver* solver_;
  long bucket_start_ = 0;   // param index where current bucket starts
  long bucket_end_ = 0;     // one past last ready param
  GpuEvent comm_done_ev_;   // created at the first GPU iteration's end
  // clip_gradients: the buckets whose update waits for the factor, in
  // arrival order, and the iteration's sum of squares so far — partials
  // written to the solver's device buffer, or the host sum in CPU mode
  std::vector<std::pair<long, long>> deferred_;
  int partials_ = 0;
  double sumsq_ = 0.0;
};

class Solver {
 public:
  explicit Solver(const PMsgPtr& solver_param, int batch_override = 0);

  void Step(int iters);
  float GetLearningRate() const;  // sgd_solver.cpp:24-66 policies + rampup
  float GetMomentum() const { return (float)param_->num("momentum", 0.0); }

  Net& net() { return *net_; }
  // TEST nets sharing the train weights, built lazily: one per test_state
  // of the solver file, or one default TEST net when it has none and the
  // net defines TEST-phase layers (reference Solver::InitTestNets)
  int num_test_nets();
  Net* test_net(int i = 0);  // null when there is none
  // every test net for its own test_iter (solver.cpp:439-540 semantics), or
  // for `iters_override` iterations each when that is > 0
  void TestAll(long iters_override = 0);
  void Snapshot();           // .caffemodel + .solverstate (solver.cpp:542)
  // reference per-GPU perf report (solver.cpp:619-628): iters/sec x batch,
  // skipping the first two measured iterations like the reference (:299)
  void print_perf_report() const;
  void Restore(const std::string& state_path);
  void LoadWeights(const std::string& model_path) {
    net_->LoadWeights(model_path);
  }
  long iter() const { return iter_; }
  // SolverParameter.type (caffe.proto:269), with the deprecated solver_type
  // enum mapped onto it (upgrade_proto.cpp:1003)
  const char* type() const { return type_name_; }
  int rule() const { return rule_; }
  bool l1() const { return l1_; }
  int history_slots() const { return solver_rule_slots(rule_); }
  // copies history slot `slot` of learnable param `param_index` (arena
  // order, as Net::learnable_params) to out, from the device or the host
  void copy_history(int slot, int param_index, float* out, long count);
  float last_loss() { return net_->loss(); }
  // SolverParameter.clip_gradients (caffe.proto:241-243); < 0 = off
  float clip_gradients() const { return clip_; }
  bool clipping() const { return clip_ >= 0.f; }
  // the last finished iteration's gradient norm and clip factor; syncs the
  // comm stream.  An error with clipping off or before the first step.
  void grad_norm(float* norm, float* factor);
  const PMsgPtr& param() const { return param_; }

  void set_action_request(ActionRequestFn fn) { action_fn_ = fn; }
  bool early_exit() const { return early_exit_; }
  // reference: only the root solver snapshots (rank 0's moving averages /
  // params are the ones persisted) — non-root CLI ranks disable the
  // snapshot-interval and signal-triggered snapshots; direct Snapshot()
  // calls (C ABI) are unaffected
  void set_snapshot_enabled(bool e) { snapshot_enabled_ = e; }
  bool snapshot_enabled() const { return snapshot_enabled_; }
  // measured throughput of the timed Step calls (img/sec), 0 before any
  double perf_img_per_sec() const;

  void set_comm(std::unique_ptr<Comm> c) { comm_ = std::move(c); }
  Comm* comm() { return comm_.get(); }
  // history slot in diff-arena layout, device or host by mode; null for a
  // slot the rule does not have
  float* history(int slot = 0) { return history_[slot].ptr(); }
  void bcast_weights();  // initial weight broadcast (parallel.cpp:208-227)
  ~Solver();  // waits: updates may still run on the comm stream

 private:
  int world() const { return comm_ && comm_->world() > 1 ? comm_->world() : 1; }
  // per-iteration cached coefficients for the fused update
  float cur_lr_ = 0.f, cur_mom_ = 0.f, weight_decay_ = 0.f;
  float grad_scale_ = 1.f;
  // clip_gradients, CPU mode: the iteration's factor, folded into coef()'s
  // gscale (1 when off or not firing, which leaves grad_scale_'s bits); in
  // GPU mode the factor stays on the device and this stays 1
  float clip_factor_ = 1.f;
  float clip_norm_ = 0.f;
  // cur_lr_ for the update: Adam folds this iteration's bias correction in
  float upd_lr_ = 0.f;
  long bucket_budget_ = 0;  // elements per bucket
  SolverCoef coef() const {
    return SolverCoef{cur_mom_, upd_lr_, weight_decay_,
                      grad_scale_ * clip_factor_, aux_, delta_};
  }

  PMsgPtr param_;
  PMsgPtr net_msg_;
  std::unique_ptr<Net> net_;
  std::vector<std::unique_ptr<Net>> test_nets_;
  bool test_nets_built_ = false;
  std::vector<NetState> test_states_;  // parsed at construction
  std::vector<long> test_iters_;       // one per test net
  void parse_states();
  NetState train_state_;
  std::unique_ptr<Comm> comm_;
  Reducer reducer_{this};
  ActionRequestFn action_fn_ = nullptr;
  bool early_exit_ = false;
  bool snapshot_enabled_ = true;
  long iter_ = 0;
  mutable int current_step_ = 0;
  // allocated at construction; the second slot by AdaDelta and Adam only
  StateBuf history_[2];
  // the update rule, parsed once at construction
  int rule_ = kRuleSgd;
  bool l1_ = false;
  const char* type_name_ = "SGD";
  float aux_ = 0.f;    // RMSProp rms_decay / Adam momentum2
  float delta_ = 0.f;  // the rule's clamped delta
  void parse_type();
  // What the bucket updates read on the device (GPU mode), built once at
  // construction.  The segment table of the bucket-fused update, one entry
  // per learnable param: arena offset, weight base pointer, lr and decay
  // MULTIPLIERS (immutable after the net build; the per-iteration rate and
  // decay are kernel arguments, so no H2D copy runs in the iteration loop).
  // With clip_gradients also one double per block of every bucket's sum-of-
  // squares launch, and the {norm, factor} slot the finalize writes and the
  // updates read.
  struct UpdateTables {
    int nseg = 0;
    DeviceBuf seg_off, w_ptrs, lrs, decays;  // long, float*, float, float
    DeviceBuf clip_partials, clip_slot;      // double, float[2]
    int clip_partials_cap = 0;
    void build(Net& net, bool clipping);
  };
  UpdateTables tables_;
  float clip_ = -1.f;
  long clip_iters_ = 0;  // iterations that went through the clip path
  void report_clipping();
  // iter_size accumulation buffer (diff-arena layout; only allocated when
  // iter_size > 1 — layer backwards overwrite their param diffs, so cross-
  // pass accumulation happens here instead of in every wgrad kernel)
  StateBuf acc_;
  void accumulate_diffs(bool merge_back);
  long train_batch() const;  // of the train net's data layer, 0 without one
  // perf-report bookkeeping
  double perf_seconds_ = 0.0;
  long perf_iters_ = 0;
  long skipped_iters_ = 0;

  friend class Reducer;
};

std::shared_ptr<Solver> create_solver_from_file(const std::string& path,
                                                int batch_override = 0);

}  // namespace camd
