/* caffe_amd.h — C-ABI of the MI355X-native Caffe-MPI training engine.
 *
 * Each entry point names the reference interface it replaces (file:line in
 * the Caffe-MPI tree).  The reference exposes no C ABI of its own (pycaffe
 * is boost::python); this ABI is the FFI a maintainer would bind to reach
 * the same Layer/Net/Solver surface — see INTEGRATION.md for the ctypes
 * binding the in-repo python mirror uses.
 *
 * Conventions: plain pointers + sizes, fp32 host buffers, 0 = success /
 * nonzero = error (last message via caffe_last_error).  No torch types.
 */
#ifndef CAFFE_AMD_H_
#define CAFFE_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* caffe_solver_t; /* caffe::Solver,  solver.hpp:73 */
typedef void* caffe_net_t;    /* caffe::Net,     net.hpp */

const char* caffe_last_error(void);

/* Caffe::set_mode / SetDevice (common.hpp): mode 0 = CPU, 1 = GPU */
int caffe_set_mode(int mode, int device);
/* GEMM compute dtype: "f32" (default, exact) or "bf16" (bf16 MFMA with
 * fp32 accumulation — the MI355X-native mixed-precision mode; replaces
 * the reference's NetParameter default_forward_type/default_backward_type
 * FLOAT16 machinery, net.cpp:100-156 / type.hpp:13-47, with fp32 storage
 * and tensor-core math instead of fp16 storage). */
int caffe_set_compute(const char* dtype);
/* rank/world for the sharded data feed without a communicator (tests);
 * caffe_comm_init sets the same engine fields. */
int caffe_set_rank_world(int rank, int world);
/* data-stream position (LMDB cursor analog; Solver::Step drives it). */
int caffe_set_data_iter(uint64_t iter);
/* multi-node ncclUniqueId bootstrap over TCP (the reference's
 * Clusters/MPI_Bcast replacement, clusters.cpp + parallel.cpp:42-45):
 * global rank 0 serves the 128-byte id to world-1 clients; the `caffe`
 * CLI drives this from CAFFE_NNODES/CAFFE_NODE_RANK/MASTER_ADDR/PORT. */
int caffe_uid_serve(const uint8_t* uid, int port, int nclients);
int caffe_uid_fetch(uint8_t* out, const char* host, int port,
                    int timeout_s);
/* Caffe::set_random_seed (common.cpp); rank offsets seed like
 * parallel.cpp:179-187 */
int caffe_set_random_seed(uint64_t seed);
/* synthetic data source configuration (replaces the LMDB DataReader,
 * data_reader.cpp, for dataset-less benching): shape of one sample and the
 * label range */
int caffe_set_synthetic_shape(int c, int h, int w, int num_classes);
/* enable per-kernel-class event timing (for roofline measurement) */
int caffe_set_perf_timing(int enable);

/* SolverRegistry::CreateSolver + Solver::Solve entry
 * (tools/caffe.cpp:213-241, solver.cpp:187).  batch_override > 0 replaces
 * the train data layer's batch_size (the reference divides the prototxt
 * batch across GPUs, parallel.cpp:284-348). */
caffe_solver_t caffe_solver_create(const char* solver_prototxt_path,
                                   int batch_override);
caffe_solver_t caffe_solver_create_from_text(const char* solver_prototxt,
                                             int batch_override);
void caffe_solver_free(caffe_solver_t s);
/* Solver::Step(iters) (solver.cpp:187-353): forward, backward with the
 * bucketed all-reduce overlapped on the side stream, fused update by the
 * solver's rule (ComputeUpdateValue of sgd_solver.cpp and the five
 * solvers beside it) */
int caffe_solver_step(caffe_solver_t s, int iters);
long caffe_solver_iter(caffe_solver_t s);
/* current net loss (the reference additionally smooths over the display
 * window, solver.cpp:606-617; this returns the raw last-iteration loss)
 * — syncs */
float caffe_solver_loss(caffe_solver_t s);
caffe_net_t caffe_solver_net(caffe_solver_t s);
/* Solver::test_nets() (solver.hpp): one TEST net per test_state of the
 * solver file, or one default TEST net when the net has TEST-phase layers
 * (Solver::InitTestNets, solver.cpp); they share the trained weights and
 * are owned by the solver.  -1 / NULL on error. */
int caffe_solver_num_test_nets(caffe_solver_t s);
caffe_net_t caffe_solver_test_net(caffe_solver_t s, int i);
/* Solver::Test(test_net_id) (solver.cpp:439-540): `iters` forwards of test
 * net i over successive batches, every scored top averaged.  Writes up to
 * max_scores values and the newline-joined top-blob names of ALL scores
 * (truncated to name_cap); returns the number of scores, -1 on error. */
int caffe_solver_test(caffe_solver_t s, int i, int iters, char* names_out,
                      int name_cap, float* values_out, int max_scores);

/* Solver::Snapshot / Restore (solver.cpp:542-604; .caffemodel binaryproto
 * weights + .solverstate with SGD history, sgd_solver.cpp:262-353) */
int caffe_solver_snapshot(caffe_solver_t s);
int caffe_solver_restore(caffe_solver_t s, const char* state_path);
/* Solver::type() (solver.hpp, the SolverRegistry name: "SGD", "Nesterov",
 * "AdaGrad", "RMSProp", "AdaDelta" or "Adam"; SolverParameter.type,
 * caffe.proto:269, with the deprecated solver_type enum mapped onto it,
 * upgrade_proto.cpp:1003).  The string lives as long as the library. */
const char* caffe_solver_type(caffe_solver_t s);
/* history blobs per learnable param: SGDSolver::history() holds N blobs,
 * AdaDelta and Adam append N more (AdaDeltaPreSolve / AdamPreSolve,
 * adam_solver.cpp:8-16) — 1 or 2 */
int caffe_solver_history_slots(caffe_solver_t s);
/* SGDSolver::history()[param_index + slot * N] (sgd_solvers.hpp), copied
 * out of device or host memory; param_index as in caffe_net_param_get,
 * count <= the param's element count — syncs */
int caffe_solver_history(caffe_solver_t s, int slot, int param_index,
                         float* out, long count);
/* SolverParameter.clip_gradients as parsed (caffe.proto:241-243; the bound
 * of SGDSolver::ClipGradients, sgd_solver.cpp:111-128); negative = off */
float caffe_solver_clip_gradients(caffe_solver_t s);
/* the last finished iteration's global L2 gradient norm (over all learnable
 * params, after the all-reduce, over world) and the factor it was scaled by:
 * l2norm_diff and scale_factor of SGDSolver::ClipGradients
 * (sgd_solver.cpp:111-128), taken once per iteration — syncs the comm
 * stream.  -1 with clip_gradients off or before the first step. */
int caffe_solver_grad_norm(caffe_solver_t s, float* norm, float* factor);
/* Net weight interop (net.cpp:1055-1248) */
int caffe_net_save_weights(caffe_net_t n, const char* path);
int caffe_net_load_weights(caffe_net_t n, const char* path);

/* one-process-per-GPU collective bootstrap (replaces Clusters::Init +
 * MPI_Bcast of ncclUniqueId, clusters.cpp:8 / parallel.cpp:42-45):
 * rank 0 generates the 128-byte id, the launcher distributes it, every
 * rank calls comm_init */
int caffe_comm_unique_id(uint8_t out[128]);
/* world-1 RCCL linkage/call smoke (GPU mode) */
int caffe_comm_selftest(void);
int caffe_comm_init(caffe_solver_t s, int rank, int world,
                    const uint8_t id[128]);
/* initial weight broadcast from rank 0 (P2PSync::on_start,
 * parallel.cpp:208-227) */
int caffe_comm_bcast_weights(caffe_solver_t s);
/* CPU-mode collective for multi-process gloo tests: the callback receives
 * (grad_ptr, count, userdata) at every bucket flush */
typedef void (*caffe_allreduce_cb)(float*, long, void*);
int caffe_comm_set_callback(caffe_solver_t s, caffe_allreduce_cb cb,
                            void* ud, int world);

/* Net construction for inference/parity runs (Net::Init, net.cpp:64) */
caffe_net_t caffe_net_create(const char* net_prototxt_path, int phase,
                             int batch_override);
/* the same with a NetState (the reference's Net(param_file, phase, level,
 * stages) constructor, net.hpp; NetState level / stage, caffe.proto):
 * `stages` is a comma-separated list, NULL or "" for none.  Layers are kept
 * by Net::FilterNet / StateMeetsRule (net.cpp:407-499) */
caffe_net_t caffe_net_create_state(const char* net_prototxt_path, int phase,
                                   int level, const char* stages,
                                   int batch_override);
void caffe_net_free(caffe_net_t n);
int caffe_net_forward(caffe_net_t n);           /* net.cpp:692 */
int caffe_net_backward(caffe_net_t n);          /* net.cpp:1031 */
float caffe_net_loss(caffe_net_t n);            /* syncs */

/* blob access by name (Net::blob_by_name, net.hpp): data or diff */
int caffe_net_blob_shape(caffe_net_t n, const char* name, int* shape_out,
                         int max_dims, int* ndims_out);
int caffe_net_blob_get(caffe_net_t n, const char* name, int diff,
                       float* out, long count);
int caffe_net_blob_set(caffe_net_t n, const char* name, int diff,
                       const float* in, long count);

/* learnable params (Net::learnable_params, net.cpp:1350): idx ordering is
 * the arena (backward-completion) order */
/* pycaffe-shim surface: zero-copy CPU pointers with SyncedMemory head
 * semantics (mutable access dirties the host copy; next GPU use re-syncs
 * — the contract python/caffe/_caffe.cpp exposed through Blob.data /
 * Blob.diff), plus layer enumeration for net.blobs/net.params/net.layers
 * dict shapes. */
float* caffe_net_blob_cpu_ptr(caffe_net_t n, const char* name, int diff,
                              int writable);
int caffe_net_num_layers(caffe_net_t n);
int caffe_net_blob_names(caffe_net_t n, char* out, int cap);
int caffe_net_layer_info(caffe_net_t n, int idx, char* name_out,
                         int name_cap, char* type_out, int type_cap,
                         int* num_blobs_out);
int caffe_net_layer_blob_shape(caffe_net_t n, const char* lname, int bidx,
                               int* shape_out, int max_dims,
                               int* ndims_out);
float* caffe_net_layer_blob_cpu_ptr(caffe_net_t n, const char* lname,
                                    int bidx, int diff, int writable);

int caffe_net_num_params(caffe_net_t n);
int caffe_net_param_info(caffe_net_t n, int idx, char* layer_name_out,
                         int name_cap, int* blob_idx_out, long* count_out);
int caffe_net_param_get(caffe_net_t n, int idx, int diff, float* out,
                        long count);
int caffe_net_param_set(caffe_net_t n, int idx, const float* in, long count);

/* device + perf introspection */
int caffe_device_synchronize(void);
/* device bytes the engine's caching allocator has handed out and not got
 * back, as requested; blocks it caches for reuse are not counted.  Back at
 * its earlier value after caffe_solver_free / caffe_net_free. */
size_t caffe_device_live_bytes(void);
/* perf counters per kernel class: returns number of classes; each row of
 * `names` gets a \0-terminated class name (cap bytes), and launches /
 * flops / bytes / ns land in the parallel arrays */
int caffe_perf_snapshot(char* names, int name_cap, long* launches,
                        double* flops, double* bytes, double* ns, int max_rows);
int caffe_perf_reset(void);
/* GEMM route trace (off by default): while enabled, every conv/IP
 * contraction records which kernel the dispatch picked (family, transposes,
 * split-K, tile grid, operand views, epilogue).  Enabling clears the log;
 * it holds at most 4096 records.  _read writes one "key=value ..." line per
 * record into buf (\0-terminated, truncated at a line boundary to cap) and
 * returns the length of the full text, so a caller can size the buffer with
 * a first call of cap 0. */
int caffe_gemm_trace(int enable);
int caffe_gemm_trace_read(char* buf, int cap);
/* Of the calls traced since the trace was last enabled: how many read their
 * operands through the 32-bit staging cursors (*cursor) and how many through
 * the 64-bit reader (*wide64: calls with a plain B, sizes past the 32-bit
 * limits, CAFFE_GEMM_W64=1, and every bf16 kernel). */
int caffe_gemm_trace_readers(long* cursor, long* wide64);
/* Kernel variant trace (off by default), same contract as the GEMM route
 * trace: while enabled, the pooling, BatchNorm-statistics, LRN, softmax and
 * segmented-SGD launch wrappers record one line per call, e.g.
 * "op=pool_max_bwd var=k3s1", "op=bn_fwd_stats var=v4 nb=2 span_max=1056",
 * "op=lrn_fwd var=ring5 odd=1", "op=softmax_fwd rows=8450 C=3 blocks=2048",
 * "op=sgd_seg lo=0 hi=272 nseg=6"; the segmented update of the other solver
 * rules (and SGD with L1) records
 * "op=solver_seg rule=adam reg=L2 lo=0 hi=272 nseg=6".  The sum of shared
 * params' gradients into their owner layer's arena range records
 * "op=shared_diff_sum lo=0 hi=32 nseg=2 nsrc=2" (segments = the owner
 * layer's learnable blobs, sources = the sharing blobs), and the
 * ContrastiveLoss kernels record
 * "op=contrastive_fwd var=row_thread N=64 C=2 blocks=1" and
 * "op=contrastive_bwd var=row_wave N=3 C=257 blocks=1" (one thread or one
 * wave per row). */
int caffe_kernel_trace(int enable);
int caffe_kernel_trace_read(char* buf, int cap);
/* The graph fusions planned for a net at build time, same buffer contract
 * as the _trace_read calls: one line "kind producer absorbed[,absorbed]"
 * per fusion, in layer order of the producer, the names being layer names.
 * kind: bn_relu | conv_relu | sum_relu (the producer applies the in-place
 * ReLU after it) | bn_add (a TRAIN BatchNorm writes the residual sum after
 * it) | bn_add_relu (and the out-of-place ReLU after that sum).  The plan
 * depends on the graph alone and is the same in CPU mode, where nothing
 * is fused. */
int caffe_net_fusions(caffe_net_t net, char* buf, int cap);
/* Which bottoms share their layer's top gradient memory, planned at build
 * time like the fusions and read the same way: one line "layer bottom
 * alias|copy" (a layer name, then the name of one of its bottom blobs) per
 * propagating bottom of an Eltwise SUM with every coefficient 1 and of a
 * Split with one top, in layer order, then bottom order.  alias: the GPU
 * backward launches nothing for that bottom; copy: a layer in place on the
 * bottom would write the shared memory while another bottom's gradient is
 * still unread, or the bottom is a Flatten's top, so it keeps its own memory
 * and gets one copy.  The same in CPU mode, where every such bottom is
 * copied. */
int caffe_net_diff_sharing(caffe_net_t net, char* buf, int cap);
/* The shared params of a net (reference Net::AppendParam, net.cpp:576-667),
 * planned at build time and read like the two plans above: one line
 * "layer blob_idx name owner_layer owner_blob_idx" per sharer, in layer
 * order, then blob order.  The first param blob whose ParamSpec carries
 * `name` owns it; every later blob of that name shares the owner's weights
 * (share_mode STRICT: equal shapes, PERMISSIVE: equal counts), is no
 * learnable param (caffe_net_num_params counts owners only) and has its
 * gradient added into the owner's right after the owner layer's backward.
 * The same in CPU mode. */
int caffe_net_param_sharing(caffe_net_t net, char* buf, int cap);
/* Self-test of the exact fast division the GEMM staging decomposes its view
 * indices with (host code, no GPU): for every divisor in [d_lo, d_hi]
 * compares quotient and remainder with / and % over the dividends 0..2^20,
 * the 4096 values below the 2^31 dividend limit and the last 4096 multiples
 * of the divisor below that limit, each +-1.  Returns the number of
 * mismatches (0 = exact), -1 on a bad range. */
long caffe_fastdiv_selftest(unsigned d_lo, unsigned d_hi);

#ifdef __cplusplus
}
#endif
#endif /* CAFFE_AMD_H_ */
