#include "net.hpp"

#include <chrono>

namespace camd {

bool state_meets_rule(const NetState& state, const PMsg& rule) {
  auto has_stage = [&](const std::string& st) {
    for (auto& s : state.stages)
      if (s == st) return true;
    return false;
  };
  if (rule.has("phase") &&
      rule.str("phase") != (state.phase == Phase::TRAIN ? "TRAIN" : "TEST"))
    return false;
  if (rule.has("min_level") && state.level < rule.inum("min_level"))
    return false;
  if (rule.has("max_level") && state.level > rule.inum("max_level"))
    return false;
  for (auto& st : rule.strs("stage"))
    if (!has_stage(st)) return false;
  for (auto& st : rule.strs("not_stage"))
    if (has_stage(st)) return false;
  return true;
}

bool layer_in_state(const PMsg& lm, const NetState& state) {
  auto incs = lm.subs("include");
  auto excs = lm.subs("exclude");
  CHECK_(incs.empty() || excs.empty())
      << "layer '" << lm.str("name")
      << "': specify either include rules or exclude rules; not both";
  bool included = incs.empty();
  for (auto& r : excs)
    if (included && state_meets_rule(state, *r)) included = false;
  for (auto& r : incs)
    if (!included && state_meets_rule(state, *r)) included = true;
  return included;
}

Net::Net(const PMsgPtr& net_param, Phase phase, int batch_override)
    : phase_(phase) {
  state_.phase = phase;
  init(net_param, batch_override);
}

Net::Net(const PMsgPtr& net_param, const NetState& state, int batch_override)
    : phase_(state.phase), state_(state) {
  init(net_param, batch_override);
}

namespace {
// the Split layer that gives each of `n` consumers of `blob` its own top
PMsgPtr split_msg(const std::string& blob, const std::string& producer,
                  int n) {
  auto sp = std::make_shared<PMsg>();
  auto addf = [&](const std::string& name, const std::string& v) {
    PVal pv;
    pv.kind = PVal::SCALAR;
    pv.scalar = v;
    sp->fields.emplace_back(name, pv);
  };
  addf("name", blob + "_" + producer + "_split");
  addf("type", "Split");
  addf("bottom", blob);
  for (int c = 0; c < n; ++c) addf("top", blob + "_split_" + std::to_string(c));
  return sp;
}
}  // namespace

// reference src/caffe/util/insert_splits.cpp behaviour: any blob consumed by
// more than one layer below its producer gets a Split layer so every
// consumer owns a private diff that Split's backward sums.
void Net::insert_splits(std::vector<PMsgPtr>& msgs) {
  // count consumptions of each (versioned) blob name
  std::map<std::string, int> last_producer;  // name -> producing msg idx
  std::map<std::string, int> consumers;      // versioned key -> count
  auto vkey = [&](const std::string& b) {
    return b + "#" + std::to_string(last_producer.count(b)
                                        ? last_producer[b]
                                        : -1);
  };
  std::vector<std::vector<std::string>> bkeys(msgs.size());
  for (size_t i = 0; i < msgs.size(); ++i) {
    for (auto& b : msgs[i]->strs("bottom")) {
      const std::string k = vkey(b);
      consumers[k]++;
      bkeys[i].push_back(k);
    }
    for (auto& t : msgs[i]->strs("top")) last_producer[t] = (int)i;
  }
  // rewire
  std::map<std::string, int> split_next;  // key -> next split-top index
  std::map<std::string, std::string> split_base;
  std::vector<PMsgPtr> out;
  last_producer.clear();
  for (size_t i = 0; i < msgs.size(); ++i) {
    // rewrite bottoms that consume split blobs
    auto& m = msgs[i];
    size_t bi = 0;
    for (auto& f : m->fields) {
      if (f.first != "bottom") continue;
      const std::string k = bkeys[i][bi++];
      auto it = split_base.find(k);
      if (it != split_base.end())
        f.second.scalar =
            it->second + "_split_" + std::to_string(split_next[k]++);
    }
    out.push_back(m);
    // after this layer, split any of its tops with >1 consumers
    for (auto& t : m->strs("top")) {
      last_producer[t] = (int)i;
      const std::string k = t + "#" + std::to_string(i);
      if (consumers[k] > 1) {
        out.push_back(split_msg(t, m->str("name"), consumers[k]));
        split_base[k] = t;
        split_next[k] = 0;
      }
    }
  }
  msgs = std::move(out);
}

namespace {
// "layer 'conv1' (Convolution) Forward" around one dispatch into layer code
struct LayerScope : ErrorScope {
  LayerScope(Layer& l, const char* stage)
      : ErrorScope("layer '" + l.name() + "' (" + l.type() + ") " + stage) {}
};
}  // namespace

void Net::init(const PMsgPtr& msg, int batch_override) {
  name_ = msg->str("name");
  for (auto& lm : filter_layers(*msg)) append_layer(lm, batch_override);
  set_backward_flags(msg->boolean("force_backward", false));
  param_sharing_ = plan_param_sharing();
  apply_param_sharing();
  collect_params();
  fusions_ = plan_fusions();
  diff_sharing_ = plan_diff_sharing();
  if (Engine::get().mode == Mode::GPU) {
    apply_fusions();
    apply_diff_sharing();
    setup_arena();
  }
  setup_shared_sums();
}

// the layers of this net's state, with Splits inserted
std::vector<PMsgPtr> Net::filter_layers(const PMsg& msg) {
  std::vector<PMsgPtr> lmsgs;
  for (auto& lm : msg.subs("layer"))
    if (layer_in_state(*lm, state_)) {
      // shallow-clone: insert_splits rewrites bottom names in place, and
      // the source tree is shared with other nets (train/test pair)
      auto copy = std::make_shared<PMsg>(*lm);
      lmsgs.push_back(copy);
    }
  CHECK_(!lmsgs.empty()) << "net has no layers for this phase";
  insert_splits(lmsgs);
  return lmsgs;
}

// create one layer, wire it to the blob map and set it up
void Net::append_layer(const PMsgPtr& lm, int batch_override) {
  auto layer = create_layer(lm);
  layer->set_phase(phase_);
  // wire bottoms
  std::vector<Blob*> bottom, top;
  for (auto& b : lm->strs("bottom")) {
    auto it = blob_map_.find(b);
    CHECK_(it != blob_map_.end())
        << "layer " << layer->name() << ": unknown bottom blob " << b;
    bottom.push_back(it->second.get());
  }
  for (auto& t : lm->strs("top")) {
    auto it = blob_map_.find(t);
    if (it != blob_map_.end()) {
      // in-place: top name equals an existing blob (must be a bottom).
      // A layer WITHOUT bottoms cannot be in-place: its top would
      // overwrite another layer's (reference net.cpp AppendTop) — two
      // staged Data layers that the net state did not tell apart
      CHECK_(!lm->strs("bottom").empty())
          << "layer '" << layer->name() << "': top blob '" << t
          << "' is produced by more than one layer (do its include "
             "rules need a stage or level of the net state?)";
      top.push_back(it->second.get());
    } else {
      auto nb = std::make_shared<Blob>();
      blob_map_[t] = nb;
      top.push_back(nb.get());
    }
  }
  {
    LayerScope scope(*layer, "SetUp");
    layer->SetUp(bottom, top);
    if (batch_override > 0 && layer->type() == "Data") {
      // per-rank batch override (reference divides the prototxt batch
      // across GPUs, parallel.cpp:284-348)
      static_cast<DataLayer*>(layer.get())->batch_ = batch_override;
      layer->Reshape(bottom, top);
    }
  }
  // loss weights
  auto lw = lm->nums("loss_weight");
  for (size_t i = 0; i < top.size(); ++i) {
    float w = i < lw.size() ? (float)lw[i]
                            : (i == 0 ? layer->default_loss_weight() : 0.f);
    layer->set_loss((int)i, w);
  }
  layers_.push_back(layer);
  bottoms_.push_back(bottom);
  tops_.push_back(top);
  top_names_.push_back(lm->strs("top"));
}

// need-backward / propagate-down flags (net.cpp Init bottom-up logic;
// force_backward marks every non-data path like the reference does)
void Net::set_backward_flags(bool force) {
  std::map<Blob*, bool> blob_needs;
  layer_need_bwd_.resize(layers_.size(), false);
  prop_down_.resize(layers_.size());
  for (size_t i = 0; i < layers_.size(); ++i) {
    const bool is_source = layers_[i]->type() == "Data" ||
                           layers_[i]->type() == "Accuracy";
    bool need = !layers_[i]->blobs().empty();
    prop_down_[i].resize(bottoms_[i].size(), false);
    for (size_t b = 0; b < bottoms_[i].size(); ++b) {
      prop_down_[i][b] = blob_needs[bottoms_[i][b]];
      need = need || prop_down_[i][b];
    }
    // LayerParameter.propagate_down (reference net.cpp Init): one entry per
    // bottom, false cuts that bottom's gradient
    const auto pd = layers_[i]->param()->strs("propagate_down");
    if (!pd.empty()) {
      CHECK_EQ_(pd.size(), bottoms_[i].size())
          << "layer '" << layers_[i]->name()
          << "': propagate_down must be given for every bottom or for none";
      need = !layers_[i]->blobs().empty();
      for (size_t b = 0; b < bottoms_[i].size(); ++b) {
        if (pd[b] != "true" && pd[b] != "1") prop_down_[i][b] = false;
        need = need || prop_down_[i][b];
      }
    }
    if (is_source) need = false;
    if (force && !is_source) {
      need = true;
      for (size_t b = 0; b < bottoms_[i].size(); ++b)
        prop_down_[i][b] =
            blob_needs.count(bottoms_[i][b]) && blob_needs[bottoms_[i][b]] &&
            (pd.empty() || pd[b] == "true" || pd[b] == "1");
    }
    layer_need_bwd_[i] = need;
    for (auto* t : tops_[i])
      blob_needs[t] =
          need || (force && !is_source && !layers_[i]->is_loss_layer());
  }
}

// ----------------------------------------------------- param-sharing plan
// reference Net::AppendParam (net.cpp:576-667).  The first blob whose
// ParamSpec carries a name owns the name; a later blob of that name, in any
// layer of any type, is a sharer.  Shapes must agree (share_mode STRICT,
// the default) or counts (PERMISSIVE, read from the sharer's spec as the
// reference does); lr_mult / decay_mult given on both sides must agree, and
// a side that gives none adopts the other's.
std::vector<Net::ParamShare> Net::plan_param_sharing() const {
  struct Owner {
    int layer, blob;
    bool has_lr, has_decay;
    float lr, decay;
  };
  std::map<std::string, Owner> owners;
  std::vector<ParamShare> plan;
  for (int i = 0; i < (int)layers_.size(); ++i) {
    const auto specs = layers_[i]->param()->subs("param");
    auto& lb = layers_[i]->blobs();
    for (int j = 0; j < (int)lb.size() && j < (int)specs.size(); ++j) {
      const PMsg& sp = *specs[j];
      const std::string name = sp.str("name");
      if (name.empty()) continue;
      const float lr = (float)sp.num("lr_mult", 1.0);
      const float decay = (float)sp.num("decay_mult", 1.0);
      auto it = owners.find(name);
      if (it == owners.end()) {
        owners[name] = {i, j, sp.has("lr_mult"), sp.has("decay_mult"), lr,
                        decay};
        continue;
      }
      Owner& o = it->second;
      Blob& mine = *lb[j];
      Blob& theirs = *layers_[o.layer]->blobs()[o.blob];
      std::ostringstream who;
      who << "param '" << name << "' owned by layer '"
          << layers_[o.layer]->name() << "' with layer '"
          << layers_[i]->name() << "'";
      if (sp.str("share_mode", "STRICT") == "PERMISSIVE") {
        if (mine.count() != theirs.count())
          CAMD_FATAL << "Cannot share " << who.str()
                     << "; count mismatch.  Owner layer param shape is "
                     << theirs.shape_string() << "; sharing layer shape is "
                     << mine.shape_string();
      } else if (mine.shape() != theirs.shape()) {
        CAMD_FATAL << "Cannot share " << who.str()
                   << "; shape mismatch.  Owner layer param shape is "
                   << theirs.shape_string()
                   << "; sharing layer expects shape " << mine.shape_string();
      }
      if (sp.has("lr_mult")) {
        if (o.has_lr && o.lr != lr)
          CAMD_FATAL << "Cannot share " << who.str()
                     << "; mismatched lr_mult (" << o.lr << " vs " << lr
                     << ")";
        o.has_lr = true;
        o.lr = lr;
      }
      if (sp.has("decay_mult")) {
        if (o.has_decay && o.decay != decay)
          CAMD_FATAL << "Cannot share " << who.str()
                     << "; mismatched decay_mult (" << o.decay << " vs "
                     << decay << ")";
        o.has_decay = true;
        o.decay = decay;
      }
      plan.push_back({i, j, name, o.layer, o.blob, o.lr, o.decay});
    }
  }
  return plan;
}

// a sharer's blob uses the owner's data memory for the life of the net; its
// diff stays its own
void Net::apply_param_sharing() {
  for (auto& s : param_sharing_)
    layers_[s.layer]->blobs()[s.blob]->ShareData(
        *layers_[s.owner_layer]->blobs()[s.owner_blob]);
}

// learnable params in backward-completion order (reverse layer order);
// sharers are none (reference learnable_params_)
void Net::collect_params() {
  std::map<std::pair<int, int>, const ParamShare*> sharer, last_share;
  for (auto& s : param_sharing_) {
    sharer[{s.layer, s.blob}] = &s;
    last_share[{s.owner_layer, s.owner_blob}] = &s;  // the merged multipliers
  }
  for (int i = (int)layers_.size() - 1; i >= 0; --i) {
    auto& lb = layers_[i]->blobs();
    for (size_t j = 0; j < lb.size(); ++j) {
      if (layers_[i]->skip_apply_update((int)j)) continue;
      if (sharer.count({i, (int)j})) continue;
      LParam p;
      p.blob = lb[j].get();
      p.layer = layers_[i].get();
      p.blob_idx = (int)j;
      p.lr_mult = layers_[i]->lr_mult((int)j);
      p.decay_mult = layers_[i]->decay_mult((int)j);
      auto own = last_share.find({i, (int)j});
      if (own != last_share.end()) {
        p.lr_mult = own->second->lr_mult;
        p.decay_mult = own->second->decay_mult;
      }
      p.count = p.blob->count();
      p.offset = arena_count_;
      arena_count_ += (long)padded(p.count);
      params_.push_back(p);
    }
  }
}

// ------------------------------------------------------------ fusion plan
bool Net::slope0_relu(int i) const {
  if (!dynamic_cast<ReLULayer*>(layers_[i].get())) return false;
  if (bottoms_[i].size() != 1 || tops_[i].size() != 1) return false;
  auto rp = layers_[i]->param()->sub("relu_param");
  return !rp || rp->num("negative_slope", 0) == 0;
}

bool Net::unit_sum2(int i) const {
  auto* el = dynamic_cast<EltwiseLayer*>(layers_[i].get());
  return el && bottoms_[i].size() == 2 && el->unit_sum();
}

// Which producers absorb which followers.  First every in-place slope-0
// ReLU directly after the BatchNorm, Convolution or unit SUM that produced
// its blob: the producer applies it in its epilogue (a BN also masks dy in
// its backward; after a conv or a sum the ReLU keeps its backward, which
// reads its own output).  Then, TRAIN only (the TEST BN path has no
// epilogue), the residual add: a unit SUM whose operand comes from the
// out-of-place BatchNorm immediately before it, that operand having no
// other consumer — the BN's norm epilogue writes bn(x)+other straight into
// the sum's top (the ResNet block pattern; kills one full read-add-write
// pass over the activation per block).  It takes the sum's in-place ReLU
// along, or absorbs an out-of-place slope-0 ReLU that is the sum's only
// consumer: the sum is then never materialized and that ReLU's backward
// masks by its top's sign instead.
std::vector<Net::Fusion> Net::plan_fusions() const {
  const int L = (int)layers_.size();
  std::map<const Blob*, int> consumers;
  for (auto& bs : bottoms_)
    for (auto* b : bs) ++consumers[b];
  std::vector<Fusion> plan;
  std::vector<int> made(L, -1);  // the kind layer i produces, or -1
  auto add = [&](Fusion::Kind k, int producer, std::vector<int> absorbed,
                 bool relu) {
    made[producer] = k;
    plan.push_back({k, producer, std::move(absorbed), relu});
  };
  for (int i = 1; i < L; ++i) {
    if (!slope0_relu(i) || !in_place(i)) continue;
    if (!fed_by_previous(i, bottoms_[i][0])) continue;
    Layer* prev = layers_[i - 1].get();
    if (dynamic_cast<BatchNormLayer*>(prev))
      add(Fusion::BN_RELU, i - 1, {i}, true);
    else if (dynamic_cast<ConvolutionLayer*>(prev))
      add(Fusion::CONV_RELU, i - 1, {i}, true);  // GemmEpi.relu
    else if (unit_sum2(i - 1))
      add(Fusion::SUM_RELU, i - 1, {i}, true);
  }
  for (int i = 1; i < L && phase_ == Phase::TRAIN; ++i) {
    if (!unit_sum2(i)) continue;
    if (!dynamic_cast<BatchNormLayer*>(layers_[i - 1].get())) continue;
    if (made[i - 1] != -1) continue;  // fused with a ReLU or another add
    if (!fed_by_previous(i, bottoms_[i][0]) &&
        !fed_by_previous(i, bottoms_[i][1]))
      continue;
    if (in_place(i - 1) || consumers[tops_[i - 1][0]] != 1) continue;
    const Blob* sum = tops_[i][0];
    if (i + 1 < L && slope0_relu(i + 1) && !in_place(i + 1) &&
        bottoms_[i + 1][0] == sum && consumers[sum] == 1)
      add(Fusion::BN_ADD_RELU, i - 1, {i, i + 1}, true);
    else
      add(Fusion::BN_ADD, i - 1, {i}, made[i] == Fusion::SUM_RELU);
  }
  std::stable_sort(plan.begin(), plan.end(),
                   [](const Fusion& a, const Fusion& b) {
                     return a.producer < b.producer;
                   });
  return plan;
}

// set the layer flags the GPU paths read (layers.hpp)
void Net::apply_fusions() {
  for (auto& f : fusions_) {
    Layer* p = layers_[f.producer].get();
    const int a = f.absorbed[0];
    // the absorbed ReLU; none in a BN_ADD, whose last absorbed is the sum
    auto* relu = dynamic_cast<ReLULayer*>(layers_[f.absorbed.back()].get());
    if (relu) relu->fused_away_ = true;
    switch (f.kind) {
      case Fusion::BN_RELU:
        static_cast<BatchNormLayer*>(p)->fuse_relu_ = true;
        relu->bwd_fused_ = true;  // BN backward masks dy by the activation
        break;
      case Fusion::CONV_RELU:
        static_cast<ConvolutionLayer*>(p)->fuse_relu_ = true;
        break;
      case Fusion::SUM_RELU:
        static_cast<EltwiseLayer*>(p)->fuse_relu_ = true;
        break;
      case Fusion::BN_ADD_RELU:
        relu->bwd_from_top_ = true;
        [[fallthrough]];
      case Fusion::BN_ADD: {
        auto* bn = static_cast<BatchNormLayer*>(p);
        bn->fuse_add_other_ =
            bottoms_[a][tops_[f.producer][0] == bottoms_[a][0] ? 1 : 0];
        bn->fuse_add_out_ = tops_[f.absorbed.back()][0];
        bn->fuse_add_relu_ = f.relu;
        static_cast<EltwiseLayer*>(layers_[a].get())->fused_away_ = true;
      }
    }
  }
}

// ------------------------------------------------------ diff-sharing plan
bool Net::passes_diff_through(int i) const {
  if (auto* el = dynamic_cast<EltwiseLayer*>(layers_[i].get()))
    return el->unit_sum();
  return dynamic_cast<SplitLayer*>(layers_[i].get()) && tops_[i].size() == 1;
}

int Net::producer(const Blob* blob) const {
  for (int i = 0; i < (int)layers_.size(); ++i)
    for (auto* t : tops_[i])
      if (t == blob) return i;
  return -1;
}

int Net::last_diff_writer(int i, const Blob* blob) const {
  for (int k = i - 1; k >= 0; --k) {
    if (!in_place(k) || tops_[k][0] != blob) continue;
    // every in-place backward writes the diff but that of a ReLU a BN
    // absorbed in both directions, which launches nothing
    bool absorbed = false;
    for (auto& f : fusions_)
      absorbed = absorbed || (f.kind == Fusion::BN_RELU && f.absorbed[0] == k);
    if (!absorbed) return k;
  }
  return -1;
}

// Backward runs from the last layer to the first on one stream.  A bottom
// that shares the top's diff memory is read last by its producer; an
// in-place layer on it writes that memory before.  If the write comes
// while another bottom of the same layer still waits to be read (its
// producer is not above the writer), that bottom would read the written
// gradient: this one keeps its own memory.  The top of a Flatten already
// shares its diff with the Flatten's bottom and is never re-pointed.
bool Net::may_alias_diff(int i, int b) const {
  const Blob* blob = bottoms_[i][b];
  if (dynamic_cast<FlattenLayer*>(layers_[producer(blob)].get())) return false;
  const int writer = last_diff_writer(i, blob);
  for (int j = 0; j < (int)bottoms_[i].size() && writer >= 0; ++j)
    if (j != b && prop_down_[i][j] && producer(bottoms_[i][j]) <= writer)
      return false;
  return true;
}

std::vector<Net::DiffShare> Net::plan_diff_sharing() const {
  std::vector<DiffShare> plan;
  for (int i = 0; i < (int)layers_.size(); ++i)
    for (int b = 0; passes_diff_through(i) && b < (int)bottoms_[i].size(); ++b)
      if (prop_down_[i][b]) plan.push_back({i, b, may_alias_diff(i, b)});
  return plan;
}

// Share the diffs once, last layer first as backward would meet them: a top
// that is itself an aliased bottom of a later layer is re-pointed before
// its own bottoms take its memory.  No blob is reshaped after the build.
void Net::apply_diff_sharing() {
  for (auto s = diff_sharing_.rbegin(); s != diff_sharing_.rend(); ++s) {
    if (!s->alias) continue;
    bottoms_[s->layer][s->bottom]->ShareDiff(*tops_[s->layer][0]);
    Layer* l = layers_[s->layer].get();
    if (auto* el = dynamic_cast<EltwiseLayer*>(l))
      el->alias_diff_[s->bottom] = true;
    else
      static_cast<SplitLayer*>(l)->alias_diff_ = true;
  }
}

void Net::setup_arena() {
  if (params_.empty()) return;
  Engine& E = Engine::get();
  const size_t bytes = sizeof(float) * (size_t)arena_count_;
  HIP_CHECK(hipMemsetAsync(diff_arena_.reserve(bytes), 0, bytes, E.stream));
  for (auto& p : params_)
    p.blob->diff_mem().set_gpu_view(diff_arena() + p.offset);
  layer_events_.resize(layers_.size());
  for (auto& ev : layer_events_) ev.create();
}

// What Backward adds after each owner layer: the sharers of the layer's
// learnable blobs, in plan order (a shared statistics blob shares data only
// and has no gradient to add).  GPU mode: one launch per owner layer over
// the layer's padded arena range, so the tables hold one segment per
// learnable blob of the layer (with or without sharers) and the sharers'
// diff pointers by segment; uploaded once, synchronously, like the solver's
// segment table.  The pointers stay good: no param blob is reshaped after
// the build.
void Net::setup_shared_sums() {
  if (param_sharing_.empty()) return;
  std::map<const Blob*, bool> learnable;
  for (auto& p : params_) learnable[p.blob] = true;
  for (auto& s : param_sharing_) {
    Blob* owner = layers_[s.owner_layer]->blobs()[s.owner_blob].get();
    if (!learnable.count(owner)) continue;
    shared_sums_[s.owner_layer].srcs.push_back(
        {owner, layers_[s.layer]->blobs()[s.blob].get()});
  }
  if (Engine::get().mode != Mode::GPU || shared_sums_.empty()) return;
  std::vector<long> seg_off;
  std::vector<int> src_begin;
  std::vector<const float*> srcs;
  for (auto& kv : shared_sums_) {
    SharedSum& ss = kv.second;
    ss.seg_start = (int)seg_off.size();
    bool first = true;
    for (auto& p : params_) {  // a layer's params: consecutive, ascending
      if (p.layer != layers_[kv.first].get()) continue;
      if (first) ss.lo = p.offset;
      first = false;
      ss.hi = p.offset + (long)padded(p.count);
      seg_off.push_back(p.offset);
      src_begin.push_back((int)srcs.size());
      for (auto& src : ss.srcs)
        if (src.owner == p.blob) srcs.push_back(src.sharer->mutable_gpu_diff());
    }
    ss.nseg = (int)seg_off.size() - ss.seg_start;
  }
  src_begin.push_back((int)srcs.size());  // the one closing bound
  d_sum_seg_off_.upload(seg_off.data(), seg_off.size() * sizeof(long));
  d_sum_src_begin_.upload(src_begin.data(), src_begin.size() * sizeof(int));
  d_sum_srcs_.upload(srcs.data(), srcs.size() * sizeof(float*));
}

// The arena and the sum tables go back to the caching allocator, which may
// hand them to the next owner: wait first, on both streams (the reducer
// reads the arena on the comm stream).
Net::~Net() {
  if (diff_arena_.p || d_sum_seg_off_.p) Engine::get().sync();
}

// Layer backwards overwrite their param diffs, so a sharer writes its own
// diff and the owner's gets the sum here.  Owners come first in layer order:
// when the owner layer's backward has run, every sharer's has.
void Net::sum_shared_diffs(int i) {
  auto it = shared_sums_.find(i);
  if (it == shared_sums_.end()) return;
  const SharedSum& ss = it->second;
  Engine& E = Engine::get();
  if (E.mode == Mode::GPU) {
    gpu::shared_diff_sum(E.stream, ss.lo, ss.hi, diff_arena(),
                         d_sum_seg_off_.as<long>() + ss.seg_start, ss.nseg,
                         d_sum_src_begin_.as<int>() + ss.seg_start,
                         d_sum_srcs_.as<const float*>(), (int)ss.srcs.size());
  } else {
    for (auto& src : ss.srcs)
      cpu::axpy(src.owner->count(), 1.f, src.sharer->cpu_diff(),
                src.owner->mutable_cpu_diff());
  }
}

void Net::forward_layer(size_t i) {
  LayerScope scope(*layers_[i], "Forward");
  layers_[i]->Forward(bottoms_[i], tops_[i]);
}

void Net::backward_layer(size_t i) {
  LayerScope scope(*layers_[i], "Backward");
  layers_[i]->Backward(tops_[i], prop_down_[i], bottoms_[i]);
}

void Net::Forward() {
  for (size_t i = 0; i < layers_.size(); ++i) forward_layer(i);
}

void Net::Backward(ReduceHook* hook) {
  Engine& E = Engine::get();
  // param ids grouped by layer, in backward order == ascending arena offset
  size_t pidx = 0;
  hipEvent_t last_ev = nullptr;
  for (int i = (int)layers_.size() - 1; i >= 0; --i) {
    if (layer_need_bwd_[i]) backward_layer(i);
    if (!shared_sums_.empty()) sum_shared_diffs(i);
    if (hook) {
      // emit this layer's params (consecutive in params_, ascending offset)
      const size_t start = pidx;
      while (pidx < params_.size() &&
             params_[pidx].layer == layers_[i].get())
        ++pidx;
      if (pidx > start) {
        hipEvent_t ev = nullptr;
        if (E.mode == Mode::GPU) {
          ev = layer_events_[i].get();
          HIP_CHECK(hipEventRecord(ev, E.stream));
          last_ev = ev;
        }
        for (size_t k = start; k < pidx; ++k) hook->param_ready((int)k, ev);
      }
    }
  }
  if (hook) {
    hipEvent_t ev = last_ev;
    if (E.mode == Mode::GPU && !ev) {
      ev = layer_events_[0].get();
      HIP_CHECK(hipEventRecord(ev, E.stream));
    }
    hook->iteration_end(ev);
  }
}

float Net::loss() {
  Engine::get().sync();
  float total = 0.f;
  for (size_t i = 0; i < layers_.size(); ++i)
    for (size_t t = 0; t < tops_[i].size(); ++t) {
      const float w = layers_[i]->loss((int)t);
      if (w != 0.f && layers_[i]->type() != "Accuracy")
        total += w * tops_[i][t]->cpu_data()[0];
    }
  return total;
}

std::vector<Net::Score> Net::scores() {
  Engine::get().sync();
  std::vector<Score> out;
  for (size_t i = 0; i < layers_.size(); ++i)
    for (size_t t = 0; t < tops_[i].size(); ++t) {
      const bool acc = layers_[i]->type() == "Accuracy";
      if (layers_[i]->loss((int)t) != 0.f || acc ||
          layers_[i]->is_loss_layer())
        out.push_back({layers_[i]->name(), top_names_[i][t],
                       (double)tops_[i][t]->cpu_data()[0], std::string()});
    }
  for (auto& s : out) {
    int same = 0;
    for (auto& o : out) same += o.layer == s.layer;
    s.label = same > 1 ? s.top : s.layer;
  }
  return out;
}

std::vector<Net::Score> Net::test_scores(long iters) {
  // the data feeds key on Engine::data_iter: advance it per forward so
  // successive test iterations see successive batches (with LMDB this
  // walks the set in order from record 0 — a fixed eval set)
  Engine& E = Engine::get();
  const uint64_t saved_iter = E.data_iter;
  std::vector<Score> sum;
  for (long it = 0; it < iters; ++it) {
    E.data_iter = (uint64_t)it;
    Forward();
    auto sc = scores();
    if (it == 0) {
      sum = sc;
    } else {
      for (size_t k = 0; k < sum.size(); ++k) sum[k].value += sc[k].value;
    }
  }
  E.data_iter = saved_iter;
  for (auto& s : sum) s.value /= (double)iters;
  std::stable_sort(sum.begin(), sum.end(), [](const Score& a, const Score& b) {
    return a.label < b.label;
  });
  return sum;
}

std::vector<std::string> Net::blob_names() const {
  std::vector<std::string> out;
  for (auto& kv : blob_map_) out.push_back(kv.first);
  return out;
}

void Net::ShareTrainedLayersWith(Net& other) {
  std::map<std::string, Layer*> by_name;
  for (auto& l : other.layers_) by_name[l->name()] = l.get();
  for (auto& l : layers_) {
    auto it = by_name.find(l->name());
    if (it == by_name.end()) continue;
    auto& src = it->second->blobs();
    auto& dst = l->blobs();
    for (size_t i = 0; i < dst.size() && i < src.size(); ++i)
      dst[i]->ShareData(*src[i]);
  }
}

}  // namespace camd

// ------------------------------------------------- snapshot interop
// .caffemodel = binary NetParameter carrying each parametered layer's blobs
// (reference Net::ToProto / CopyTrainedLayersFrom, net.cpp:1055-1248).
#include <filesystem>
#include <fstream>

#include "proto_wire.hpp"

namespace camd {

void Net::SaveWeights(const std::string& path) {
  Engine::get().sync();
  wire::Writer net_w;
  net_w.str(1, name_);
  for (size_t i = 0; i < layers_.size(); ++i) {
    auto& lb = layers_[i]->blobs();
    if (lb.empty()) continue;
    wire::Writer lw;
    lw.str(1, layers_[i]->name());
    lw.str(2, layers_[i]->type());
    for (auto& b : lb) lw.blob(7, b->cpu_data(), b->count(), b->shape());
    net_w.submsg(100, lw.out);
  }
  const auto dir = std::filesystem::path(path).parent_path();
  if (!dir.empty()) std::filesystem::create_directories(dir);
  std::ofstream f(path, std::ios::binary);
  CHECK_(f.good()) << "cannot write " << path;
  f.write(net_w.out.data(), (long)net_w.out.size());
}

void Net::LoadWeights(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  CHECK_(f.good()) << "cannot read " << path;
  std::string buf((std::istreambuf_iterator<char>(f)),
                  std::istreambuf_iterator<char>());
  std::map<std::string, Layer*> by_name;
  for (auto& l : layers_) by_name[l->name()] = l.get();
  wire::Reader r(buf.data(), buf.size());
  wire::Field fld;
  int loaded = 0;
  while (r.next(&fld)) {
    if (fld.num != 100 || fld.wt != 2) continue;  // LayerParameter
    wire::Reader lr(fld.data, fld.len);
    wire::Field lf;
    std::string lname;
    std::vector<wire::BlobData> blobs;
    while (lr.next(&lf)) {
      if (lf.num == 1 && lf.wt == 2)
        lname.assign(lf.data, lf.len);
      else if (lf.num == 7 && lf.wt == 2)
        blobs.push_back(wire::parse_blob(lf.data, lf.len));
    }
    auto it = by_name.find(lname);
    if (it == by_name.end()) continue;  // reference skips unknown layers
    auto& lb = it->second->blobs();
    for (size_t j = 0; j < blobs.size() && j < lb.size(); ++j) {
      CHECK_EQ_((long)blobs[j].data.size(), lb[j]->count())
          << "blob size mismatch in " << lname << " blob " << j;
      memcpy(lb[j]->mutable_cpu_data(), blobs[j].data.data(),
             blobs[j].data.size() * sizeof(float));
      ++loaded;
    }
  }
  CHECK_GT_(loaded, 0) << "no matching layer blobs in " << path;
}

void Net::time_layers(int iters) {
  Engine& E = Engine::get();
  const size_t L = layers_.size();
  std::vector<double> fwd_ms(L, 0), bwd_ms(L, 0);
  auto tick = [&]() {
    E.sync();
    return std::chrono::steady_clock::now();
  };
  Forward();  // warmup + shapes
  Backward(nullptr);
  for (int it = 0; it < iters; ++it) {
    for (size_t i = 0; i < L; ++i) {
      auto t0 = tick();
      forward_layer(i);
      auto t1 = tick();
      fwd_ms[i] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    }
    for (size_t i = L; i-- > 0;) {
      if (!layer_need_bwd_[i]) continue;
      auto t0 = tick();
      backward_layer(i);
      auto t1 = tick();
      bwd_ms[i] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    }
  }
  double ftot = 0, btot = 0;
  fprintf(stderr, "%-28s %12s %12s\n", "layer", "forward(ms)",
          "backward(ms)");
  for (size_t i = 0; i < L; ++i) {
    fprintf(stderr, "%-28s %12.3f %12.3f\n", layers_[i]->name().c_str(),
            fwd_ms[i] / iters, bwd_ms[i] / iters);
    ftot += fwd_ms[i] / iters;
    btot += bwd_ms[i] / iters;
  }
  fprintf(stderr, "%-28s %12.3f %12.3f  (total %.3f ms/iter)\n", "TOTAL",
          ftot, btot, ftot + btot);
}

}  // namespace camd
