// capi.cpp — C-ABI implementation (see include/caffe_amd.h for the mapping
// to reference interfaces).
#include "../../include/caffe_amd.h"
#include "solver.hpp"

namespace camd {
extern int g_syn_shape[3];  // defined in layers_cpu.cpp
}

using namespace camd;

namespace {
thread_local std::string g_err;
// the live handles; never deleted, like the Engine (Engine::get): a handle
// is freed by caffe_solver_free / caffe_net_free or not at all
auto* const g_solvers = new std::map<void*, std::shared_ptr<Solver>>;
auto* const g_nets = new std::map<void*, std::shared_ptr<Net>>;

#define API_TRY try {
#define API_CATCH                      \
  }                                    \
  catch (const std::exception& e) {    \
    g_err = e.what();                  \
    return -1;                         \
  }
#define API_CATCH_NULL                 \
  }                                    \
  catch (const std::exception& e) {    \
    g_err = e.what();                  \
    return nullptr;                    \
  }

Solver* S(caffe_solver_t s) { return (Solver*)s; }
Net* N(caffe_net_t n) { return (Net*)n; }
}  // namespace

extern "C" {

const char* caffe_last_error(void) { return g_err.c_str(); }

int caffe_set_mode(int mode, int device) {
  API_TRY
  if (mode == 1)
    Engine::get().set_mode_gpu(device);
  else
    Engine::get().mode = Mode::CPU;
  return 0;
  API_CATCH
}

// multi-node uid bootstrap (csrc/bootstrap.cpp) — exposed so the TCP
// exchange is testable without GPUs or multiple boxes
int caffe_uid_serve(const uint8_t* uid, int port, int nclients) {
  API_TRY
  return uid_serve(uid, 128, port, nclients);
  API_CATCH
}
int caffe_uid_fetch(uint8_t* out, const char* host, int port,
                    int timeout_s) {
  API_TRY
  return uid_fetch(out, 128, host, port, timeout_s);
  API_CATCH
}

// data-stream iteration counter (the LMDB cursor / synthetic stream
// position; Solver::Step drives it during training — tests reset it)
int caffe_set_data_iter(uint64_t iter) {
  API_TRY
  Engine::get().data_iter = iter;
  return 0;
  API_CATCH
}

// rank/world without a communicator (single-process tests of the
// rank-sharded data feed; comm_init sets the same fields when a real
// collective attaches — reference P2PSync rank plumbing)
int caffe_set_rank_world(int rank, int world) {
  API_TRY
  Engine& E = Engine::get();
  E.rank = rank;
  E.world = world;
  E.cpu_rng.seed(E.seed + (uint64_t)rank);
  return 0;
  API_CATCH
}

// GEMM compute dtype: "f32" (exact MFMA, default) or "bf16" (bf16 MFMA,
// fp32 accumulation — mixed precision, the reference Ftype/Btype analog).
// Storage and every non-GEMM op stay fp32.
int caffe_set_compute(const char* dtype) {
  API_TRY
  std::string d = dtype ? dtype : "";
  if (d == "f32" || d == "fp32" || d == "float")
    Engine::get().gemm_bf16 = false;
  else if (d == "bf16" || d == "bfloat16")
    Engine::get().gemm_bf16 = true;
  else
    CAMD_FATAL << "unknown compute dtype " << d;
  return 0;
  API_CATCH
}

int caffe_set_random_seed(uint64_t seed) {
  API_TRY
  Engine& E = Engine::get();
  E.seed = seed;
  E.cpu_rng.seed(seed + (uint64_t)E.rank);
  return 0;
  API_CATCH
}

int caffe_set_synthetic_shape(int c, int h, int w, int num_classes) {
  API_TRY
  camd::g_syn_shape[0] = c;
  camd::g_syn_shape[1] = h;
  camd::g_syn_shape[2] = w;
  if (num_classes > 0) Engine::get().syn_classes = num_classes;
  return 0;
  API_CATCH
}

int caffe_set_perf_timing(int enable) {
  Engine::get().perf_timing = enable != 0;
  return 0;
}

caffe_solver_t caffe_solver_create(const char* path, int batch_override) {
  API_TRY
  auto s = create_solver_from_file(path, batch_override);
  (*g_solvers)[s.get()] = s;
  return (caffe_solver_t)s.get();
  API_CATCH_NULL
}

caffe_solver_t caffe_solver_create_from_text(const char* text,
                                             int batch_override) {
  API_TRY
  auto s = std::make_shared<Solver>(parse_prototxt(text), batch_override);
  (*g_solvers)[s.get()] = s;
  return (caffe_solver_t)s.get();
  API_CATCH_NULL
}

void caffe_solver_free(caffe_solver_t s) { g_solvers->erase(s); }

int caffe_solver_step(caffe_solver_t s, int iters) {
  API_TRY
  S(s)->Step(iters);
  return 0;
  API_CATCH
}

long caffe_solver_iter(caffe_solver_t s) { return S(s)->iter(); }

float caffe_solver_loss(caffe_solver_t s) {
  try {
    return S(s)->last_loss();
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1.f;
  }
}

caffe_net_t caffe_solver_net(caffe_solver_t s) {
  return (caffe_net_t)&S(s)->net();
}

int caffe_solver_num_test_nets(caffe_solver_t s) {
  API_TRY
  return S(s)->num_test_nets();
  API_CATCH
}

caffe_net_t caffe_solver_test_net(caffe_solver_t s, int i) {
  API_TRY
  Net* n = S(s)->test_net(i);
  CHECK_(n) << "no test net " << i << " (the solver has "
            << S(s)->num_test_nets() << ")";
  return (caffe_net_t)n;
  API_CATCH_NULL
}

int caffe_solver_test(caffe_solver_t s, int i, int iters, char* names_out,
                      int name_cap, float* values_out, int max_scores) {
  API_TRY
  Net* n = S(s)->test_net(i);
  CHECK_(n) << "no test net " << i << " (the solver has "
            << S(s)->num_test_nets() << ")";
  CHECK_GT_(iters, 0);
  const auto scores = n->test_scores(iters);
  std::string joined;
  for (size_t k = 0; k < scores.size(); ++k) {
    if (k) joined += "\n";
    joined += scores[k].top;
    if ((int)k < max_scores) values_out[k] = (float)scores[k].value;
  }
  if (name_cap > 0) snprintf(names_out, name_cap, "%s", joined.c_str());
  return (int)scores.size();
  API_CATCH
}

int caffe_solver_snapshot(caffe_solver_t s) {
  API_TRY
  S(s)->Snapshot();
  return 0;
  API_CATCH
}

int caffe_solver_restore(caffe_solver_t s, const char* state_path) {
  API_TRY
  S(s)->Restore(state_path);
  return 0;
  API_CATCH
}

const char* caffe_solver_type(caffe_solver_t s) { return S(s)->type(); }

int caffe_solver_history_slots(caffe_solver_t s) {
  return S(s)->history_slots();
}

int caffe_solver_history(caffe_solver_t s, int slot, int param_index,
                         float* out, long count) {
  API_TRY
  S(s)->copy_history(slot, param_index, out, count);
  return 0;
  API_CATCH
}

float caffe_solver_clip_gradients(caffe_solver_t s) {
  return S(s)->clip_gradients();
}

int caffe_solver_grad_norm(caffe_solver_t s, float* norm, float* factor) {
  API_TRY
  S(s)->grad_norm(norm, factor);
  return 0;
  API_CATCH
}

int caffe_net_save_weights(caffe_net_t n, const char* path) {
  API_TRY
  N(n)->SaveWeights(path);
  return 0;
  API_CATCH
}

int caffe_net_load_weights(caffe_net_t n, const char* path) {
  API_TRY
  N(n)->LoadWeights(path);
  return 0;
  API_CATCH
}

int caffe_comm_selftest(void) {
  API_TRY
  return rccl_selftest();
  API_CATCH
}

int caffe_comm_unique_id(uint8_t out[128]) {
  API_TRY
  rccl_unique_id(out);
  return 0;
  API_CATCH
}

int caffe_comm_init(caffe_solver_t s, int rank, int world,
                    const uint8_t id[128]) {
  API_TRY
  Engine& E = Engine::get();
  E.rank = rank;
  E.world = world;
  E.cpu_rng.seed(E.seed + (uint64_t)rank);
  S(s)->set_comm(make_rccl_comm(rank, world, id));
  return 0;
  API_CATCH
}

int caffe_comm_bcast_weights(caffe_solver_t s) {
  API_TRY
  S(s)->bcast_weights();
  return 0;
  API_CATCH
}

int caffe_comm_set_callback(caffe_solver_t s, caffe_allreduce_cb cb,
                            void* ud, int world) {
  API_TRY
  Engine::get().world = world;
  S(s)->set_comm(make_callback_comm(cb, ud, world));
  return 0;
  API_CATCH
}

caffe_net_t caffe_net_create(const char* path, int phase,
                             int batch_override) {
  API_TRY
  auto n = std::make_shared<Net>(parse_prototxt_file(path),
                                 phase ? Phase::TEST : Phase::TRAIN,
                                 batch_override);
  (*g_nets)[n.get()] = n;
  return (caffe_net_t)n.get();
  API_CATCH_NULL
}

caffe_net_t caffe_net_create_state(const char* path, int phase, int level,
                                   const char* stages, int batch_override) {
  API_TRY
  NetState st;
  st.phase = phase ? Phase::TEST : Phase::TRAIN;
  st.level = level;
  const std::string list = stages ? stages : "";
  for (size_t pos = 0; pos < list.size();) {
    size_t next = list.find(',', pos);
    if (next == std::string::npos) next = list.size();
    if (next > pos) st.stages.push_back(list.substr(pos, next - pos));
    pos = next + 1;
  }
  auto n = std::make_shared<Net>(parse_prototxt_file(path), st,
                                 batch_override);
  (*g_nets)[n.get()] = n;
  return (caffe_net_t)n.get();
  API_CATCH_NULL
}

void caffe_net_free(caffe_net_t n) { g_nets->erase(n); }

int caffe_net_forward(caffe_net_t n) {
  API_TRY
  N(n)->Forward();
  return 0;
  API_CATCH
}

int caffe_net_backward(caffe_net_t n) {
  API_TRY
  N(n)->Backward(nullptr);
  return 0;
  API_CATCH
}

float caffe_net_loss(caffe_net_t n) {
  try {
    return N(n)->loss();
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1.f;
  }
}

int caffe_net_blob_shape(caffe_net_t n, const char* name, int* shape_out,
                         int max_dims, int* ndims_out) {
  API_TRY
  Blob* b = N(n)->blob_by_name(name);
  CHECK_(b) << "no blob " << name;
  const auto& s = b->shape();
  *ndims_out = (int)s.size();
  for (int i = 0; i < (int)s.size() && i < max_dims; ++i) shape_out[i] = s[i];
  return 0;
  API_CATCH
}

int caffe_net_blob_get(caffe_net_t n, const char* name, int diff, float* out,
                       long count) {
  API_TRY
  Blob* b = N(n)->blob_by_name(name);
  CHECK_(b) << "no blob " << name;
  CHECK_LE_(count, b->count());
  Engine::get().sync();
  const float* src = diff ? b->cpu_diff() : b->cpu_data();
  memcpy(out, src, sizeof(float) * count);
  return 0;
  API_CATCH
}

int caffe_net_blob_set(caffe_net_t n, const char* name, int diff,
                       const float* in, long count) {
  API_TRY
  Blob* b = N(n)->blob_by_name(name);
  CHECK_(b) << "no blob " << name;
  CHECK_LE_(count, b->count());
  float* dst = diff ? b->mutable_cpu_diff() : b->mutable_cpu_data();
  memcpy(dst, in, sizeof(float) * count);
  return 0;
  API_CATCH
}

// ---- pycaffe-shim surface (round 2): zero-copy CPU pointers with the
// SyncedMemory head semantics pycaffe relied on (mutable access marks the
// host copy dirty; the next GPU use re-syncs), plus layer enumeration so
// `net.blobs` / `net.params` / `net.layers` can be dict-shaped.
float* caffe_net_blob_cpu_ptr(caffe_net_t n, const char* name, int diff,
                              int writable) {
  try {
    Blob* b = N(n)->blob_by_name(name);
    CHECK_(b) << "no blob " << name;
    Engine::get().sync();
    if (writable)
      return diff ? b->mutable_cpu_diff() : b->mutable_cpu_data();
    return const_cast<float*>(diff ? b->cpu_diff() : b->cpu_data());
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}

int caffe_net_num_layers(caffe_net_t n) {
  return (int)N(n)->layers().size();
}

// newline-joined blob names in topological order
int caffe_net_blob_names(caffe_net_t n, char* out, int cap) {
  API_TRY
  std::string joined;
  for (auto& nm : N(n)->blob_names()) {
    if (!joined.empty()) joined += "\n";
    joined += nm;
  }
  snprintf(out, cap, "%s", joined.c_str());
  return 0;
  API_CATCH
}

int caffe_net_layer_info(caffe_net_t n, int idx, char* name_out,
                         int name_cap, char* type_out, int type_cap,
                         int* num_blobs_out) {
  API_TRY
  auto& ls = N(n)->layers();
  CHECK_LT_(idx, (int)ls.size());
  snprintf(name_out, name_cap, "%s", ls[idx]->name().c_str());
  snprintf(type_out, type_cap, "%s", ls[idx]->type().c_str());
  *num_blobs_out = (int)ls[idx]->blobs().size();
  return 0;
  API_CATCH
}

static Layer* find_layer(caffe_net_t n, const char* lname) {
  for (auto& l : N(n)->layers())
    if (l->name() == lname) return l.get();
  CAMD_FATAL << "no layer " << lname;
}

int caffe_net_layer_blob_shape(caffe_net_t n, const char* lname, int bidx,
                               int* shape_out, int max_dims,
                               int* ndims_out) {
  API_TRY
  Layer* l = find_layer(n, lname);
  CHECK_LT_(bidx, (int)l->blobs().size());
  const auto& s = l->blobs()[bidx]->shape();
  *ndims_out = (int)s.size();
  for (int i = 0; i < (int)s.size() && i < max_dims; ++i)
    shape_out[i] = s[i];
  return 0;
  API_CATCH
}

float* caffe_net_layer_blob_cpu_ptr(caffe_net_t n, const char* lname,
                                    int bidx, int diff, int writable) {
  try {
    Layer* l = find_layer(n, lname);
    CHECK_LT_(bidx, (int)l->blobs().size());
    Blob* b = l->blobs()[bidx].get();
    Engine::get().sync();
    if (writable)
      return diff ? b->mutable_cpu_diff() : b->mutable_cpu_data();
    return const_cast<float*>(diff ? b->cpu_diff() : b->cpu_data());
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}

int caffe_net_num_params(caffe_net_t n) {
  return (int)N(n)->learnable_params().size();
}

int caffe_net_param_info(caffe_net_t n, int idx, char* name_out,
                         int name_cap, int* blob_idx_out, long* count_out) {
  API_TRY
  auto& ps = N(n)->learnable_params();
  CHECK_LT_(idx, (int)ps.size());
  snprintf(name_out, name_cap, "%s", ps[idx].layer->name().c_str());
  *blob_idx_out = ps[idx].blob_idx;
  *count_out = ps[idx].count;
  return 0;
  API_CATCH
}

int caffe_net_param_get(caffe_net_t n, int idx, int diff, float* out,
                        long count) {
  API_TRY
  auto& ps = N(n)->learnable_params();
  CHECK_LT_(idx, (int)ps.size());
  Blob* b = ps[idx].blob;
  CHECK_LE_(count, b->count());
  Engine::get().sync();
  memcpy(out, diff ? b->cpu_diff() : b->cpu_data(), sizeof(float) * count);
  return 0;
  API_CATCH
}

int caffe_net_param_set(caffe_net_t n, int idx, const float* in, long count) {
  API_TRY
  auto& ps = N(n)->learnable_params();
  CHECK_LT_(idx, (int)ps.size());
  Blob* b = ps[idx].blob;
  CHECK_LE_(count, b->count());
  memcpy(b->mutable_cpu_data(), in, sizeof(float) * count);
  return 0;
  API_CATCH
}

int caffe_device_synchronize(void) {
  API_TRY
  Engine::get().sync();
  Engine::get().drain_events();
  return 0;
  API_CATCH
}

size_t caffe_device_live_bytes(void) {
  return Engine::get().dalloc.live_bytes();
}

int caffe_perf_snapshot(char* names, int name_cap, long* launches,
                        double* flops, double* bytes, double* ns,
                        int max_rows) {
  API_TRY
  Engine& E = Engine::get();
  int row = 0;
  for (auto& kv : E.perf()) {
    if (row >= max_rows) break;
    snprintf(names + (size_t)row * name_cap, name_cap, "%s",
             kv.first.c_str());
    launches[row] = kv.second.launches.load();
    flops[row] = kv.second.flops.load();
    bytes[row] = kv.second.bytes.load();
    ns[row] = kv.second.ns.load();
    ++row;
  }
  return row;
  API_CATCH
}

int caffe_gemm_trace(int enable) {
  API_TRY
  gpu::gemm_trace(enable != 0);
  return 0;
  API_CATCH
}

int caffe_gemm_trace_read(char* buf, int cap) {
  API_TRY
  return (int)gpu::gemm_trace_read(buf, cap);
  API_CATCH
}

int caffe_gemm_trace_readers(long* cursor, long* wide64) {
  API_TRY
  gpu::gemm_trace_readers(cursor, wide64);
  return 0;
  API_CATCH
}

long caffe_fastdiv_selftest(unsigned d_lo, unsigned d_hi) {
  API_TRY
  CHECK_GT_(d_lo, 0u);
  CHECK_LE_((long)d_hi, kFastDivLimit);
  long bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(dynamic, 16)
  for (long dl = d_lo; dl <= (long)d_hi; ++dl) {
    const unsigned d = (unsigned)dl;
    const FastDiv f = fastdiv_make(d);
    auto check = [&](long n) {
      if (n < 0 || n >= kFastDivLimit) return;
      const unsigned u = (unsigned)n, q = fastdiv(u, f);
      bad += q != u / d || u - q * d != u % d;
    };
    for (long n = 0; n <= (1L << 20); ++n) check(n);
    for (long n = kFastDivLimit - 4096; n < kFastDivLimit; ++n) check(n);
    // the multiples of d next to the limit, and their neighbours
    const long top = (kFastDivLimit - 1) / d;
    for (long k = std::max(0L, top - 4096); k <= top + 1; ++k)
      for (long e = -1; e <= 1; ++e) check(k * (long)d + e);
  }
  return bad;
  API_CATCH
}

int caffe_kernel_trace(int enable) {
  API_TRY
  gpu::kernel_trace(enable != 0);
  return 0;
  API_CATCH
}

int caffe_kernel_trace_read(char* buf, int cap) {
  API_TRY
  return (int)gpu::kernel_trace_read(buf, cap);
  API_CATCH
}

// a build-time plan as text, one entry per line: whole lines only, like the
// trace readers; returns the full length
static int plan_lines(const std::vector<std::string>& lines, char* buf,
                      int cap) {
  std::string text;
  if (cap > 0) buf[0] = 0;
  for (auto& line : lines) {
    if ((long)(text.size() + line.size() + 1) < (long)cap)
      memcpy(buf + text.size(), (line + "\n").c_str(), line.size() + 2);
    text += line + "\n";
  }
  return (int)text.size();
}

int caffe_net_fusions(caffe_net_t n, char* buf, int cap) {
  API_TRY
  static const char* const kinds[] = {"bn_relu", "conv_relu", "sum_relu",
                                      "bn_add", "bn_add_relu"};
  auto& layers = N(n)->layers();
  std::vector<std::string> lines;
  for (auto& f : N(n)->fusions()) {
    std::string line = std::string(kinds[f.kind]) + " " +
                       layers[f.producer]->name();
    for (size_t k = 0; k < f.absorbed.size(); ++k)
      line += (k ? "," : " ") + layers[f.absorbed[k]]->name();
    lines.push_back(line);
  }
  return plan_lines(lines, buf, cap);
  API_CATCH
}

int caffe_net_diff_sharing(caffe_net_t n, char* buf, int cap) {
  API_TRY
  auto& layers = N(n)->layers();
  std::vector<std::string> lines;
  for (auto& s : N(n)->diff_sharing())
    lines.push_back(layers[s.layer]->name() + " " +
                    layers[s.layer]->param()->strs("bottom")[s.bottom] +
                    (s.alias ? " alias" : " copy"));
  return plan_lines(lines, buf, cap);
  API_CATCH
}

int caffe_net_param_sharing(caffe_net_t n, char* buf, int cap) {
  API_TRY
  auto& layers = N(n)->layers();
  std::vector<std::string> lines;
  for (auto& s : N(n)->param_sharing())
    lines.push_back(layers[s.layer]->name() + " " + std::to_string(s.blob) +
                    " " + s.name + " " + layers[s.owner_layer]->name() + " " +
                    std::to_string(s.owner_blob));
  return plan_lines(lines, buf, cap);
  API_CATCH
}

int caffe_perf_reset(void) {
  for (auto& kv : Engine::get().perf()) {
    kv.second.launches = 0;
    kv.second.flops = 0;
    kv.second.bytes = 0;
    kv.second.ns = 0;
  }
  return 0;
}

}  // extern "C"
