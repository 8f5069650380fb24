// net.hpp — prototxt-defined layer graph with topological execution and the
// backward→reduce producer hook (reference src/caffe/net.cpp: Init :64-405,
// ForwardFromTo :669, BackwardFromToAu :722-751, InitializeLearnableDiffSpace
// :1350-1374).  MI355X re-design notes:
//  - one contiguous device arena for learnable diffs (and a parallel arena
//    for SGD history), laid out in BACKWARD COMPLETION order so the bucketed
//    all-reduce flushes flat ascending ranges;
//  - instead of the reference's reduce thread + blocking queue
//    (net.cpp:757-877), backward records a hipEvent per layer and hands
//    (param_id, event) to the reducer, which chains the collective and the
//    fused update on the side comm stream — same overlap, no host threads.
#pragma once

#include "layers.hpp"

namespace camd {

struct ReduceHook {
  // called right after the producing layer's backward kernels are launched;
  // `done` is recorded on the compute stream (null in CPU mode)
  virtual void param_ready(int param_id, hipEvent_t done) = 0;
  virtual void iteration_end(hipEvent_t backward_done) = 0;
  virtual ~ReduceHook() = default;
};

// reference NetState (caffe.proto): what a layer's include / exclude rules
// are matched against
struct NetState {
  Phase phase = Phase::TRAIN;
  int level = 0;
  std::vector<std::string> stages;
};
// reference Net::StateMeetsRule (net.cpp:435-499): phase equal, level within
// [min_level, max_level], every `stage` present, no `not_stage` present
bool state_meets_rule(const NetState& state, const PMsg& rule);
// reference Net::FilterNet (net.cpp:407-433): included by default unless an
// exclude rule is met; with include rules, only when one of them is met
bool layer_in_state(const PMsg& layer_msg, const NetState& state);

class Net {
 public:
  // level 0, no stages
  Net(const PMsgPtr& net_param, Phase phase, int batch_override = 0);
  Net(const PMsgPtr& net_param, const NetState& state,
      int batch_override = 0);

  void Forward();
  void Backward(ReduceHook* hook = nullptr);
  float loss();  // syncs; Σ loss_weight · loss-top
  // test-score outputs: every top of a loss layer (also at loss_weight 0,
  // which the reference reports too), every other loss-weighted top and
  // every Accuracy top, one entry per (layer, top) in net order
  struct Score {
    std::string layer, top;  // names of the layer and of the top blob
    double value;
    // what the score is printed under: the layer name, or the top blob's
    // name (as the reference prints) where two scored tops share a layer
    // name
    std::string label;
  };
  std::vector<Score> scores();
  // reference Solver::Test (solver.cpp:439-540) for one net: `iters`
  // forwards over successive batches from data position 0, every score
  // averaged; sorted by label.  Leaves Engine::data_iter as it found it.
  std::vector<Score> test_scores(long iters);

  struct LParam {
    Blob* blob;
    Layer* layer;
    int blob_idx;
    float lr_mult, decay_mult;
    long offset;  // elements into the diff arena (GPU mode), padded
    long count;
  };
  std::vector<LParam>& learnable_params() { return params_; }
  long learnable_count() const { return arena_count_; }
  // params_ is arena (reverse-layer) order; the reference serializes SGD
  // history in FORWARD learnable-param order (sgd_solver.cpp:262-353) —
  // snapshot/restore must walk this permutation for wire compatibility
  std::vector<int> forward_param_order() const {
    std::map<const Layer*, int> pos;
    for (size_t i = 0; i < layers_.size(); ++i) pos[layers_[i].get()] = (int)i;
    std::vector<int> idx(params_.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int)i;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) {
      const int la = pos.at(params_[a].layer), lb = pos.at(params_[b].layer);
      if (la != lb) return la < lb;
      return params_[a].blob_idx < params_[b].blob_idx;
    });
    return idx;
  }
  float* diff_arena() { return diff_arena_.as<float>(); }

  const std::vector<std::shared_ptr<Layer>>& layers() const {
    return layers_;
  }
  Blob* blob_by_name(const std::string& n) {
    auto it = blob_map_.find(n);
    return it == blob_map_.end() ? nullptr : it->second.get();
  }
  std::vector<std::string> blob_names() const;
  const std::string& name() const { return name_; }
  Phase phase() const { return phase_; }
  const NetState& state() const { return state_; }

  // copy weights from another net (test-net sharing / snapshot restore)
  void ShareTrainedLayersWith(Net& other);

  // .caffemodel binaryproto interop (reference Net weight load/save,
  // net.cpp:1055-1248; format: proto_wire.hpp)
  void SaveWeights(const std::string& path);
  void LoadWeights(const std::string& path);

  // `caffe time`-style per-layer forward/backward timing report
  void time_layers(int iters);

  // One producer layer absorbing the work of the layer(s) after it.  The
  // plan is a function of the built graph alone and is made in both modes;
  // only GPU mode applies it (no CPU layer path fuses).
  struct Fusion {
    enum Kind {
      BN_RELU,      // BN + in-place ReLU: forward and backward absorbed
      CONV_RELU,    // Conv + in-place ReLU: forward only
      SUM_RELU,     // Eltwise SUM + in-place ReLU: forward only
      BN_ADD,       // BN + residual add (TRAIN): the BN writes the sum's top
      BN_ADD_RELU,  // ... and a following out-of-place ReLU, which then
                    // masks its backward by its own top
    };
    Kind kind;
    int producer;               // layer index
    std::vector<int> absorbed;  // layer indices, in layer order
    // the producer's epilogue applies a ReLU: always, but for a BN_ADD only
    // when the sum has an in-place ReLU (their own SUM_RELU entry) to take
    // along
    bool relu;
  };
  // in layer order of the producers
  const std::vector<Fusion>& fusions() const { return fusions_; }

  // A bottom whose gradient equals its layer's top gradient (a unit Eltwise
  // SUM, a Split with one top) either shares the top's diff memory, so the
  // layer's backward launches nothing for it, or keeps its own and gets a
  // copy.  Planned from the built graph in both modes like the fusions;
  // only GPU mode applies it (the CPU layers always copy).
  struct DiffShare {
    int layer, bottom;  // layer index, index among its bottoms
    bool alias;
  };
  // in layer order, then bottom order
  const std::vector<DiffShare>& diff_sharing() const { return diff_sharing_; }

  // Named param blobs (reference Net::AppendParam, net.cpp:576-667): the
  // first blob of a name owns it, every later one is a sharer.  A sharer
  // uses the owner's data memory, is no learnable param, and keeps a diff
  // of its own that Backward adds into the owner's right after the owner
  // layer's backward.  Planned from the built layers in both modes.
  struct ParamShare {
    int layer, blob;              // the sharer
    std::string name;             // the ParamSpec name
    int owner_layer, owner_blob;  // the first blob of that name
    // the owner's multipliers once this sharer's spec is merged in: a side
    // that does not set one adopts the other side's
    float lr_mult, decay_mult;
  };
  // in layer order, then blob order
  const std::vector<ParamShare>& param_sharing() const {
    return param_sharing_;
  }
  ~Net();
  Net(const Net&) = delete;
  Net& operator=(const Net&) = delete;

 private:
  // the net build, in order; each step reads and writes the members below
  void init(const PMsgPtr& msg, int batch_override);
  std::vector<PMsgPtr> filter_layers(const PMsg& msg);
  void insert_splits(std::vector<PMsgPtr>& layer_msgs);
  void append_layer(const PMsgPtr& layer_msg, int batch_override);
  void set_backward_flags(bool force_backward);
  std::vector<ParamShare> plan_param_sharing() const;
  void apply_param_sharing();
  void collect_params();
  std::vector<Fusion> plan_fusions() const;
  void apply_fusions();
  std::vector<DiffShare> plan_diff_sharing() const;
  void apply_diff_sharing();
  void setup_arena();
  void setup_shared_sums();

  // the graph predicates the two plans are made of
  bool in_place(int i) const {
    return !bottoms_[i].empty() && !tops_[i].empty() &&
           bottoms_[i][0] == tops_[i][0];
  }
  bool slope0_relu(int i) const;  // one-bottom one-top ReLU, slope 0
  bool unit_sum2(int i) const;    // Eltwise SUM of two bottoms, coeffs 1
  // layer i-1 has one top and that top is `blob`
  bool fed_by_previous(int i, const Blob* blob) const {
    return i >= 1 && tops_[i - 1].size() == 1 && tops_[i - 1][0] == blob;
  }
  // every bottom's gradient is the top's: unit Eltwise SUM, one-top Split
  bool passes_diff_through(int i) const;
  int producer(const Blob* blob) const;  // the first layer with this top
  // the last layer below `i` whose backward writes `blob`'s diff in place,
  // or -1
  int last_diff_writer(int i, const Blob* blob) const;
  // bottom `b` of layer `i` may share the top's diff memory
  bool may_alias_diff(int i, int b) const;

  // one layer's dispatch under its error scope
  void forward_layer(size_t i);
  void backward_layer(size_t i);
  // owner layer i: add its sharers' diffs into its own (no-op elsewhere)
  void sum_shared_diffs(int i);

  std::string name_;
  Phase phase_;
  std::vector<std::shared_ptr<Layer>> layers_;
  std::vector<std::vector<Blob*>> bottoms_, tops_;
  std::vector<std::vector<std::string>> top_names_;
  NetState state_;
  std::vector<std::vector<bool>> prop_down_;
  std::vector<bool> layer_need_bwd_;
  std::map<std::string, std::shared_ptr<Blob>> blob_map_;
  std::vector<LParam> params_;
  std::vector<Fusion> fusions_;
  std::vector<DiffShare> diff_sharing_;
  std::vector<ParamShare> param_sharing_;
  // What sum_shared_diffs runs for one owner layer: the sharers of its
  // learnable blobs in plan order and, in GPU mode, the layer's arena range
  // and its slice of the device tables (uploaded once at build).
  struct SharedSum {
    struct Src {
      Blob* owner;
      Blob* sharer;
    };
    std::vector<Src> srcs;
    long lo = 0, hi = 0;          // padded arena range of the layer's params
    int seg_start = 0, nseg = 0;  // into d_sum_seg_off_ / d_sum_src_begin_
  };
  std::map<int, SharedSum> shared_sums_;  // by owner layer index
  // Device tables.  The segments of all owner layers stand one after
  // another, in owner-layer order, and so do their sources: segment k's
  // sources are srcs[src_begin[k] .. src_begin[k + 1]), with ONE closing
  // bound after the last segment of the last layer (a layer's slice starts
  // at its seg_start in both tables).
  DeviceBuf d_sum_seg_off_;    // long: arena offset of every segment
  DeviceBuf d_sum_src_begin_;  // int: segments + 1 source bounds
  DeviceBuf d_sum_srcs_;       // const float*: the sharers' diff pointers
  long arena_count_ = 0;
  // declared after layers_: the arena goes before the blobs whose diffs are
  // non-owning views of it
  DeviceBuf diff_arena_;
  std::vector<GpuEvent> layer_events_;
};

}  // namespace camd
