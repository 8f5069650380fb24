"""caffe_amd — host-side mirror of the Caffe-MPI Layer/Net/Solver surface.

ctypes binding over libcaffe_amd.so's C ABI (include/caffe_amd.h; each entry
point there cites the reference interface it replaces).  PyTorch is used by
callers only for torch.distributed rendezvous — the engine itself is C++/HIP.
"""
import ctypes
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(_PKG, "libcaffe_amd.so")


def _load():
    if not os.path.exists(_SO):
        subprocess.check_call(["make", "-C", _PKG, "-j8"])
    try:
        return ctypes.CDLL(_SO)
    except OSError as e:
        raise ImportError(
            f"libcaffe_amd.so failed to load ({e}); the HIP engine is "
            "mandatory — no fallback") from e


_lib = _load()

_lib.caffe_last_error.restype = ctypes.c_char_p
# declare handle argtypes (void*) — without these ctypes truncates to int
_vp = ctypes.c_void_p
_lib.caffe_solver_create.argtypes = [ctypes.c_char_p, ctypes.c_int]
_lib.caffe_solver_create_from_text.argtypes = [ctypes.c_char_p, ctypes.c_int]
_lib.caffe_solver_free.argtypes = [_vp]
_lib.caffe_solver_step.argtypes = [_vp, ctypes.c_int]
_lib.caffe_solver_iter.argtypes = [_vp]
_lib.caffe_solver_loss.argtypes = [_vp]
_lib.caffe_solver_net.argtypes = [_vp]
_lib.caffe_comm_unique_id.argtypes = [ctypes.POINTER(ctypes.c_uint8)]
_lib.caffe_comm_init.argtypes = [_vp, ctypes.c_int, ctypes.c_int,
                                 ctypes.POINTER(ctypes.c_uint8)]
_lib.caffe_comm_bcast_weights.argtypes = [_vp]
_lib.caffe_net_create.argtypes = [ctypes.c_char_p, ctypes.c_int,
                                  ctypes.c_int]
_lib.caffe_net_create_state.argtypes = [ctypes.c_char_p, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_char_p,
                                        ctypes.c_int]
_lib.caffe_net_create_state.restype = ctypes.c_void_p
_lib.caffe_solver_num_test_nets.argtypes = [_vp]
_lib.caffe_solver_test_net.argtypes = [_vp, ctypes.c_int]
_lib.caffe_solver_test_net.restype = ctypes.c_void_p
_lib.caffe_solver_test.argtypes = [_vp, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_char_p, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_float),
                                   ctypes.c_int]
_lib.caffe_net_free.argtypes = [_vp]
_lib.caffe_net_num_layers.argtypes = [_vp]
_lib.caffe_net_blob_names.argtypes = [_vp, ctypes.c_char_p, ctypes.c_int]
_lib.caffe_net_layer_info.argtypes = [_vp, ctypes.c_int, ctypes.c_char_p,
                                      ctypes.c_int, ctypes.c_char_p,
                                      ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_int)]
_lib.caffe_net_blob_cpu_ptr.restype = ctypes.POINTER(ctypes.c_float)
_lib.caffe_net_blob_cpu_ptr.argtypes = [_vp, ctypes.c_char_p, ctypes.c_int,
                                        ctypes.c_int]
_lib.caffe_net_forward.argtypes = [_vp]
_lib.caffe_net_backward.argtypes = [_vp]
_lib.caffe_net_loss.argtypes = [_vp]
_lib.caffe_net_blob_shape.argtypes = [_vp, ctypes.c_char_p,
                                      ctypes.POINTER(ctypes.c_int),
                                      ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_int)]
_lib.caffe_net_num_params.argtypes = [_vp]
_lib.caffe_solver_snapshot.argtypes = [_vp]
_lib.caffe_solver_restore.argtypes = [_vp, ctypes.c_char_p]
_lib.caffe_net_save_weights.argtypes = [_vp, ctypes.c_char_p]
_lib.caffe_net_load_weights.argtypes = [_vp, ctypes.c_char_p]
_lib.caffe_solver_create.restype = ctypes.c_void_p
_lib.caffe_solver_create_from_text.restype = ctypes.c_void_p
_lib.caffe_solver_net.restype = ctypes.c_void_p
_lib.caffe_solver_loss.restype = ctypes.c_float
_lib.caffe_solver_iter.restype = ctypes.c_long
_lib.caffe_net_create.restype = ctypes.c_void_p
_lib.caffe_net_loss.restype = ctypes.c_float
_lib.caffe_set_random_seed.argtypes = [ctypes.c_uint64]
_lib.caffe_set_compute.argtypes = [ctypes.c_char_p]
_lib.caffe_gemm_trace_read.argtypes = [ctypes.c_char_p, ctypes.c_int]
_lib.caffe_kernel_trace_read.argtypes = [ctypes.c_char_p, ctypes.c_int]
_lib.caffe_net_fusions.argtypes = [_vp, ctypes.c_char_p, ctypes.c_int]
_lib.caffe_net_diff_sharing.argtypes = [_vp, ctypes.c_char_p, ctypes.c_int]
_lib.caffe_net_param_sharing.argtypes = [_vp, ctypes.c_char_p, ctypes.c_int]
_lib.caffe_fastdiv_selftest.argtypes = [ctypes.c_uint, ctypes.c_uint]
_lib.caffe_fastdiv_selftest.restype = ctypes.c_long
_lib.caffe_device_live_bytes.restype = ctypes.c_size_t

_f32p = ctypes.POINTER(ctypes.c_float)
_lib.caffe_net_blob_get.argtypes = [_vp, ctypes.c_char_p, ctypes.c_int,
                                    _f32p, ctypes.c_long]
_lib.caffe_net_blob_set.argtypes = [_vp, ctypes.c_char_p, ctypes.c_int,
                                    _f32p, ctypes.c_long]
_lib.caffe_net_param_info.argtypes = [_vp, ctypes.c_int, ctypes.c_char_p,
                                      ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(ctypes.c_long)]
_lib.caffe_net_param_get.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _f32p,
                                     ctypes.c_long]
_lib.caffe_net_param_set.argtypes = [_vp, ctypes.c_int, _f32p, ctypes.c_long]
_lib.caffe_solver_type.argtypes = [_vp]
_lib.caffe_solver_type.restype = ctypes.c_char_p
_lib.caffe_solver_history_slots.argtypes = [_vp]
_lib.caffe_solver_history.argtypes = [_vp, ctypes.c_int, ctypes.c_int, _f32p,
                                      ctypes.c_long]
_lib.caffe_solver_clip_gradients.argtypes = [_vp]
_lib.caffe_solver_clip_gradients.restype = ctypes.c_float
_lib.caffe_solver_grad_norm.argtypes = [_vp, _f32p, _f32p]

ALLREDUCE_CB = ctypes.CFUNCTYPE(None, _f32p, ctypes.c_long, ctypes.c_void_p)
_lib.caffe_comm_set_callback.argtypes = [_vp, ALLREDUCE_CB, ctypes.c_void_p,
                                         ctypes.c_int]


class CaffeError(RuntimeError):
    pass


def _ck(rc):
    """status-code return: 0 = ok"""
    if rc is None or rc != 0:
        raise CaffeError(_lib.caffe_last_error().decode())
    return rc


def _ckp(ptr):
    """pointer return: NULL = error"""
    if not ptr:
        raise CaffeError(_lib.caffe_last_error().decode())
    return ptr


def set_mode(mode, device=0):
    _ck(_lib.caffe_set_mode(1 if mode == "gpu" else 0, device))


def set_data_iter(i):
    """Data-stream position (LMDB cursor / synthetic counter)."""
    _ck(_lib.caffe_set_data_iter(ctypes.c_uint64(i)))


def set_rank_world(rank, world):
    """Engine rank/world for the sharded data feed (no communicator)."""
    _ck(_lib.caffe_set_rank_world(rank, world))


def set_compute(dtype):
    """GEMM compute dtype: "f32" (exact, default) or "bf16" (bf16 MFMA
    with fp32 accumulation — mixed precision; storage stays fp32)."""
    _ck(_lib.caffe_set_compute(dtype.encode()))


def set_random_seed(seed):
    _ck(_lib.caffe_set_random_seed(seed))


def set_synthetic_shape(c, h, w, num_classes=1000):
    _ck(_lib.caffe_set_synthetic_shape(c, h, w, num_classes))


def set_perf_timing(enable):
    _ck(_lib.caffe_set_perf_timing(1 if enable else 0))


def device_synchronize():
    _ck(_lib.caffe_device_synchronize())


def device_live_bytes():
    """Device bytes the engine's allocator has handed out and not got back
    (blocks it caches for reuse are not counted)."""
    return _lib.caffe_device_live_bytes()


def perf_snapshot():
    cap, rows = 64, 256
    names = ctypes.create_string_buffer(cap * rows)
    launches = (ctypes.c_long * rows)()
    flops = (ctypes.c_double * rows)()
    bytes_ = (ctypes.c_double * rows)()
    ns = (ctypes.c_double * rows)()
    n = _lib.caffe_perf_snapshot(names, cap, launches, flops, bytes_, ns,
                                 rows)
    if n < 0:
        raise CaffeError(_lib.caffe_last_error().decode())
    out = {}
    for i in range(n):
        name = names.raw[i * cap:(i + 1) * cap].split(b"\0")[0].decode()
        out[name] = dict(launches=launches[i], flops=flops[i],
                         bytes=bytes_[i], ns=ns[i])
    return out


def perf_reset():
    _ck(_lib.caffe_perf_reset())


def gemm_trace(enable):
    """Record which GEMM kernel every conv/IP contraction is dispatched to
    (off by default; enabling clears the log, which holds 4096 records)."""
    _ck(_lib.caffe_gemm_trace(1 if enable else 0))


def gemm_trace_read():
    """The recorded routes, one dict per gemm call: fam (slim32 | slim64 |
    f32_128 | bf16_128 | bf16_wide), ta, tb, sk (1 = no split-K), kw (the
    128-tile kernels' intra-block K split), M, N, K, tm, tn (tile rows /
    columns), av, bv (none | chan | im2col) with sh, sw, epi (none | plain |
    scatter | sscatter), bias (none | row | col), relu."""
    return _trace_records(_lib.caffe_gemm_trace_read)


def gemm_trace_readers():
    """(cursor, wide64): of the gemm calls traced since gemm_trace(True),
    how many read their operands through the 32-bit staging cursors and how
    many through the 64-bit reader."""
    cur, wide = ctypes.c_long(0), ctypes.c_long(0)
    _ck(_lib.caffe_gemm_trace_readers(ctypes.byref(cur), ctypes.byref(wide)))
    return cur.value, wide.value


def fastdiv_selftest(d_lo, d_hi):
    """Mismatches of the GEMM staging's exact fast division against / and %
    for every divisor in [d_lo, d_hi] (host code; see caffe_amd.h)."""
    n = _lib.caffe_fastdiv_selftest(d_lo, d_hi)
    if n < 0:
        raise CaffeError(_lib.caffe_last_error().decode())
    return n


def _trace_records(read):
    n = read(None, 0)
    if n < 0:
        raise CaffeError(_lib.caffe_last_error().decode())
    buf = ctypes.create_string_buffer(n + 1)
    if read(buf, n + 1) < 0:
        raise CaffeError(_lib.caffe_last_error().decode())
    out = []
    for line in buf.value.decode().splitlines():
        rec = dict(kv.split("=", 1) for kv in line.split())
        out.append({k: int(v) if v.lstrip("-").isdigit() else v
                    for k, v in rec.items()})
    return out


def kernel_trace(enable):
    """Record which specialised kernel the pooling, BatchNorm-statistics,
    LRN, softmax and segmented solver-update launch wrappers pick (off by
    default; enabling clears the log, which holds 4096 records)."""
    _ck(_lib.caffe_kernel_trace(1 if enable else 0))


def kernel_trace_read():
    """The recorded launches in call order, one dict per wrapper call:
    op (pool_max_fwd | pool_max_bwd | pool_ave_fwd | pool_ave_bwd |
    bn_fwd_stats | bn_bwd_stats | lrn_fwd | lrn_bwd | softmax_fwd | sgd_seg |
    solver_seg) and, by op: var (k3 | k3s1 | k3s2 | generic for max pooling,
    v4 | scalar for BN, ring5 | generic for LRN); nb and span_max (BN batch
    slices and the largest per-block span); odd (LRN: N*H*W is odd); rows,
    C, blocks (softmax); lo, hi, nseg (update bucket range in the param
    arena: sgd_seg for SGD with L2, solver_seg for every other solver type
    and for L1, which adds rule (sgd | nesterov | adagrad | rmsprop |
    adadelta | adam) and reg (L1 | L2)); shared_diff_sum (the sum of shared
    params' gradients after an owner layer's backward) with lo, hi, nseg,
    nsrc; contrastive_fwd | contrastive_bwd with var (row_thread | row_wave),
    N, C, blocks.  With clip_gradients set: grad_sumsq (a bucket's sum of
    squares) with lo, hi, blocks, passes; clip_final with partials; and the
    sgd_seg / solver_seg records carry clip=1."""
    return _trace_records(_lib.caffe_kernel_trace_read)


class Net:
    def __init__(self, handle, owned=False):
        self._h = handle
        self._owned = owned

    @classmethod
    def from_file(cls, path, phase=0, batch_override=0, stages=(), level=0):
        """stages / level: the NetState the layers' include / exclude rules
        are matched against (stage, not_stage, min_level, max_level)."""
        if not stages and level == 0:
            h = _ckp(_lib.caffe_net_create(path.encode(), phase,
                                           batch_override))
        else:
            h = _ckp(_lib.caffe_net_create_state(
                path.encode(), phase, level, ",".join(stages).encode(),
                batch_override))
        return cls(h, owned=True)

    def forward(self):
        _ck(_lib.caffe_net_forward(self._h))

    def backward(self):
        _ck(_lib.caffe_net_backward(self._h))

    def loss(self):
        v = _lib.caffe_net_loss(self._h)
        if v == -1.0:
            err = _lib.caffe_last_error().decode()
            if err:
                raise CaffeError(err)
        return v

    def blob_shape(self, name):
        shape = (ctypes.c_int * 8)()
        nd = ctypes.c_int()
        _ck(_lib.caffe_net_blob_shape(self._h, name.encode(), shape, 8,
                                      ctypes.byref(nd)))
        return tuple(shape[i] for i in range(nd.value))

    def blob_names(self):
        buf = ctypes.create_string_buffer(65536)
        _ck(_lib.caffe_net_blob_names(self._h, buf, 65536))
        return [s for s in buf.value.decode().split("\n") if s]

    def layer_names(self):
        nbuf = ctypes.create_string_buffer(256)
        tbuf = ctypes.create_string_buffer(256)
        nb = ctypes.c_int()
        out = []
        for i in range(_lib.caffe_net_num_layers(self._h)):
            _ck(_lib.caffe_net_layer_info(self._h, i, nbuf, 256, tbuf, 256,
                                          ctypes.byref(nb)))
            out.append(nbuf.value.decode())
        return out

    def fusions(self):
        """The graph fusions planned at build time, in layer order: one
        (kind, producer layer, [absorbed layers]) per fusion, kind being
        bn_relu | conv_relu | sum_relu | bn_add | bn_add_relu (see
        caffe_amd.h).  The same in CPU mode, where nothing is fused."""
        return [(kind, prod, absorbed.split(","))
                for kind, prod, absorbed in
                self._plan_lines(_lib.caffe_net_fusions)]

    def diff_sharing(self):
        """Which bottoms share their layer's top gradient memory in GPU
        mode, planned at build time, in layer order: one (layer, bottom
        blob, "alias" | "copy") per propagating bottom of a unit Eltwise SUM
        and of a one-top Split (see caffe_amd.h).  The same in CPU mode,
        where every such bottom is copied."""
        return [tuple(f) for f in
                self._plan_lines(_lib.caffe_net_diff_sharing)]

    def param_sharing(self):
        """The shared params planned at build time, in layer order: one
        (layer, blob index, param name, owner layer, owner blob index) per
        param blob that shares an earlier blob of the same ParamSpec name
        (see caffe_amd.h).  A sharer uses the owner's weights and is not
        among num_params() / param(); its gradient is added into the
        owner's during backward.  The same in CPU mode."""
        return [(layer, int(bi), name, owner, int(obi))
                for layer, bi, name, owner, obi in
                self._plan_lines(_lib.caffe_net_param_sharing)]

    def _plan_lines(self, read):
        # a build-time plan: one entry per line, fields split by blanks
        n = read(self._h, None, 0)
        buf = ctypes.create_string_buffer(max(n, 0) + 1)
        if n < 0 or read(self._h, buf, n + 1) < 0:
            raise CaffeError(_lib.caffe_last_error().decode())
        return [line.split(" ") for line in buf.value.decode().splitlines()]

    def blob(self, name, diff=False):
        shape = self.blob_shape(name)
        out = np.empty(shape if shape else (1,), np.float32)
        _ck(_lib.caffe_net_blob_get(
            self._h, name.encode(), int(diff),
            out.ctypes.data_as(_f32p), out.size))
        return out

    def set_blob(self, name, arr, diff=False):
        arr = np.ascontiguousarray(arr, np.float32)
        _ck(_lib.caffe_net_blob_set(
            self._h, name.encode(), int(diff),
            arr.ctypes.data_as(_f32p), arr.size))

    def num_params(self):
        return _lib.caffe_net_num_params(self._h)

    def param_info(self, idx):
        buf = ctypes.create_string_buffer(256)
        bi = ctypes.c_int()
        cnt = ctypes.c_long()
        _ck(_lib.caffe_net_param_info(self._h, idx, buf, 256,
                                      ctypes.byref(bi), ctypes.byref(cnt)))
        return buf.value.decode(), bi.value, cnt.value

    def param(self, idx, diff=False):
        _, _, cnt = self.param_info(idx)
        out = np.empty(cnt, np.float32)
        _ck(_lib.caffe_net_param_get(self._h, idx, int(diff),
                                     out.ctypes.data_as(_f32p), cnt))
        return out

    def set_param(self, idx, arr):
        arr = np.ascontiguousarray(arr, np.float32)
        _ck(_lib.caffe_net_param_set(self._h, idx,
                                     arr.ctypes.data_as(_f32p), arr.size))

    def params(self):
        return {i: self.param_info(i) for i in range(self.num_params())}

    def save_weights(self, path):
        """NetParameter binaryproto with every layer blob (incl. BN stats)
        — net.cpp ToProto / tools/caffe.cpp -weights surface."""
        _ck(_lib.caffe_net_save_weights(self._h, path.encode()))

    def load_weights(self, path):
        _ck(_lib.caffe_net_load_weights(self._h, path.encode()))


class Solver:
    def __init__(self, path=None, text=None, batch_override=0):
        if path is not None:
            self._h = _ckp(_lib.caffe_solver_create(path.encode(),
                                                   batch_override))
        else:
            self._h = _ckp(_lib.caffe_solver_create_from_text(
                text.encode(), batch_override))
        self.net = Net(_ckp(_lib.caffe_solver_net(self._h)))
        self._cb_keepalive = None

    def step(self, iters=1):
        _ck(_lib.caffe_solver_step(self._h, iters))

    @property
    def test_nets(self):
        """The solver's TEST nets (one per test_state of the solver file, or
        one default TEST net), sharing the trained weights."""
        n = _lib.caffe_solver_num_test_nets(self._h)
        if n < 0:
            raise CaffeError(_lib.caffe_last_error().decode())
        return [Net(_ckp(_lib.caffe_solver_test_net(self._h, i)))
                for i in range(n)]

    def test(self, i, iters):
        """Run test net i for `iters` batches from the start of its data:
        {top blob name: averaged value} of every scored top."""
        cap, rows = 4096, 64
        names = ctypes.create_string_buffer(cap)
        vals = (ctypes.c_float * rows)()
        n = _lib.caffe_solver_test(self._h, i, iters, names, cap, vals, rows)
        if n < 0:
            raise CaffeError(_lib.caffe_last_error().decode())
        keys = names.value.decode().split("\n") if n else []
        return {k: vals[j] for j, k in enumerate(keys[:rows])}

    @property
    def iter(self):
        return _lib.caffe_solver_iter(self._h)

    def loss(self):
        return _lib.caffe_solver_loss(self._h)

    @property
    def type(self):
        """The solver's registry name: SGD | Nesterov | AdaGrad | RMSProp |
        AdaDelta | Adam (a deprecated solver_type enum is mapped onto it)."""
        return _lib.caffe_solver_type(self._h).decode()

    @property
    def history_slots(self):
        """History blobs per param: 2 for AdaDelta and Adam, else 1."""
        return _lib.caffe_solver_history_slots(self._h)

    def history(self, i, slot=0):
        """History slot `slot` of param i (indexed as Net.param)."""
        _, _, cnt = self.net.param_info(i)
        out = np.empty(cnt, np.float32)
        _ck(_lib.caffe_solver_history(self._h, slot, i,
                                      out.ctypes.data_as(_f32p), cnt))
        return out

    @property
    def clip_gradients(self):
        """SolverParameter.clip_gradients as parsed; negative = off."""
        return _lib.caffe_solver_clip_gradients(self._h)

    def grad_norm(self):
        """(norm, factor) of the last finished iteration: the global L2 norm
        of the reduced gradient over world, and the clip factor applied
        (1.0 when the norm was within clip_gradients).  Syncs.  An error
        with clip_gradients off or before the first step."""
        norm, factor = ctypes.c_float(), ctypes.c_float()
        _ck(_lib.caffe_solver_grad_norm(self._h, ctypes.byref(norm),
                                        ctypes.byref(factor)))
        return np.float32(norm.value), np.float32(factor.value)

    def comm_unique_id(self):
        buf = (ctypes.c_uint8 * 128)()
        _ck(_lib.caffe_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, rank, world, uid_bytes):
        buf = (ctypes.c_uint8 * 128)(*uid_bytes)
        _ck(_lib.caffe_comm_init(self._h, rank, world, buf))

    def bcast_weights(self):
        _ck(_lib.caffe_comm_bcast_weights(self._h))

    def set_allreduce_callback(self, fn, world):
        """CPU-mode collective for gloo tests: fn(np_array) reduced in place."""
        def _trampoline(ptr, count, _ud):
            arr = np.ctypeslib.as_array(ptr, shape=(count,))
            fn(arr)
        cb = ALLREDUCE_CB(_trampoline)
        self._cb_keepalive = cb
        _ck(_lib.caffe_comm_set_callback(self._h, cb, None, world))
