// parallel.cpp — RCCL communicator (the reference's NCCL call-site set is
// tiny: ncclGetUniqueId/ncclCommInitRank parallel.cpp:42-45,:166-169,
// ncclBcast :217-222, ncclAllReduce :233-239/:248-250, ncclCommDestroy :140).
// One process per GPU; the unique id travels over torch.distributed's store
// in bench.py (the reference used MPI_Bcast; single-node needs no MPI).
#include <rccl/rccl.h>

#include "solver.hpp"

namespace camd {

#define NCCL_CHECK(x)                                                  \
  do {                                                                 \
    ncclResult_t r_ = (x);                                             \
    if (r_ != ncclSuccess)                                             \
      CAMD_FATAL << "RCCL error: " << ncclGetErrorString(r_)           \
                 << " at " #x;                                         \
  } while (0)

void rccl_unique_id(void* out) {
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  ncclUniqueId id;
  NCCL_CHECK(ncclGetUniqueId(&id));
  memcpy(out, &id, sizeof(id));
}

namespace {

class RcclComm : public Comm {
 public:
  RcclComm(int rank, int world, const void* uid) : world_(world) {
    ncclUniqueId id;
    memcpy(&id, uid, sizeof(id));
    NCCL_CHECK(ncclCommInitRank(&comm_, world, id, rank));
  }
  ~RcclComm() override { ncclCommDestroy(comm_); }
  void allreduce(float* buf, long count, hipStream_t s) override {
    NCCL_CHECK(ncclAllReduce(buf, buf, (size_t)count, ncclFloat, ncclSum,
                             comm_, s));
  }
  void bcast(float* buf, long count, int root, hipStream_t s) override {
    NCCL_CHECK(
        ncclBcast(buf, (size_t)count, ncclFloat, root, comm_, s));
  }
  int world() const override { return world_; }

 private:
  ncclComm_t comm_;
  int world_;
};

class CallbackComm : public Comm {
 public:
  CallbackComm(HostAllreduceFn fn, void* ud, int world)
      : fn_(fn), ud_(ud), world_(world) {}
  void allreduce(float* buf, long count, hipStream_t) override {
    fn_(buf, count, ud_);
  }
  void bcast(float* buf, long count, int /*root*/, hipStream_t) override {
    // CPU test comm: callback semantics give every rank identical data via
    // identical seeds; bcast is the identity here
    (void)buf;
    (void)count;
  }
  int world() const override { return world_; }

 private:
  HostAllreduceFn fn_;
  void* ud_;
  int world_;
};

}  // namespace

std::unique_ptr<Comm> make_rccl_comm(int rank, int world, const void* uid) {
  return std::unique_ptr<Comm>(new RcclComm(rank, world, uid));
}

// world-1 smoke of the whole RCCL path (comm init + allreduce + bcast):
// proves the librccl linkage and call sequence on the box without needing
// multiple GPUs (the driver's 8-GPU run is the real collective test)
int rccl_selftest() {
  Engine& E = Engine::get();
  CHECK_(E.mode == Mode::GPU) << "rccl selftest needs GPU mode";
  ncclUniqueId id;
  NCCL_CHECK(ncclGetUniqueId(&id));
  RcclComm comm(0, 1, &id);
  const long n = 4096;
  std::vector<float> host(n);
  for (long i = 0; i < n; ++i) host[i] = (float)(i % 97) * 0.5f;
  DeviceBuf dev;
  float* buf = (float*)dev.upload(host.data(), n * sizeof(float));
  comm.allreduce(buf, n, E.stream);
  comm.bcast(buf, n, 0, E.stream);
  HIP_CHECK(hipStreamSynchronize(E.stream));
  std::vector<float> out(n);
  HIP_CHECK(hipMemcpy(out.data(), buf, n * 4, hipMemcpyDeviceToHost));
  for (long i = 0; i < n; ++i)
    CHECK_EQ_(out[i], host[i]) << "rccl world-1 allreduce mismatch at " << i;
  return 0;
}

std::unique_ptr<Comm> make_callback_comm(HostAllreduceFn fn, void* ud,
                                         int world) {
  return std::unique_ptr<Comm>(new CallbackComm(fn, ud, world));
}

}  // namespace camd
