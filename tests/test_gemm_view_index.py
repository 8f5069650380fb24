"""32-bit view indexing of the GEMM staging (gemm_common.hpp).

The conv GEMMs read their NCHW / implicit-im2col operands through a
per-thread staging cursor built once before the K-loop and a per-tile read
that decomposes only the K-dependent half of the index, all in 32-bit
arithmetic with host-computed reciprocals (fastdiv, math.hpp).  Two things
can go wrong: the division, and an address or a validity mask of the reader.

* The division is compared exhaustively with / and % on the host.
* The reader is checked through conv parity against the float64 oracle at
  the project's TOL = 1e-4 (layer_checks.check_conv), on the smallest shapes
  at which each piece of the reader runs; the route trace proves that the
  kernel classes the pieces live in were reached.
"""
import json
import os
import subprocess
import sys

import pytest

import caffe_amd as ca
from engine_util import REPO
from layer_checks import check_conv

# ---------------------------------------------------------------- fastdiv

MODELS = ("lenet", "alexnet", "googlenet", "resnet50")


def _fields(msg, key):
    return [v for k, v in msg if k == key]


def _first(msg, key, default=None):
    vals = _fields(msg, key)
    return vals[0] if vals else default


def model_divisors(model):
    """spad, OW, kh*kw and kw of every convolution of a model spec, from a
    spatial-shape walk over its layers (conv / pool change H x W, every
    other layer hands its first bottom's on)."""
    with open(os.path.join(REPO, "models", "specs", f"{model}.json")) as f:
        net = json.load(f)
    crop = 28  # LeNet: MNIST, no crop
    dims, out = {}, set()
    for layer in _fields(net, "layer"):
        tp = _first(layer, "transform_param")
        if tp and _first(tp, "crop_size"):
            crop = int(_first(tp, "crop_size"))
        bottoms, tops = _fields(layer, "bottom"), _fields(layer, "top")
        kind = _first(layer, "type")
        if not bottoms:
            for t in tops:
                dims[t] = (crop, crop)
            continue
        h, w = dims.get(bottoms[0], (1, 1))
        p = _first(layer, {"Convolution": "convolution_param",
                           "Pooling": "pooling_param"}.get(kind, ""), None)
        if p is not None:
            def geo(name, axis, default):
                v = _first(p, f"{name}_{axis}") or _first(p, name)
                return int(v) if v is not None else default
            if _first(p, "global_pooling") == "true":
                kh, kw = h, w
            else:
                kh = geo("kernel", "h", None) or int(_first(p, "kernel_size"))
                kw = geo("kernel", "w", None) or int(_first(p, "kernel_size"))
            sh, sw = geo("stride", "h", 1), geo("stride", "w", 1)
            ph, pw = geo("pad", "h", 0), geo("pad", "w", 0)
            if kind == "Convolution":
                h = (h + 2 * ph - kh) // sh + 1
                w = (w + 2 * pw - kw) // sw + 1
                out |= {(h * w + 15) // 16 * 16, w, kh * kw, kw}
            else:  # pooling rounds up
                h = -((h + 2 * ph - kh) // -sh) + 1
                w = -((w + 2 * pw - kw) // -sw) + 1
        for t in tops:
            dims[t] = (h, w)
    return out


def test_model_divisors_found():
    # the walk sees the shapes it is meant to: ResNet-50's conv1 (112 x 112,
    # 7 x 7) and last stage (7 x 7 -> spad 64), AlexNet's conv1 (55 x 55,
    # 11 x 11), LeNet's conv2 (8 x 8, 5 x 5)
    rn = model_divisors("resnet50")
    assert {112 * 112, 112, 49, 7, 64, 9, 3} <= rn, sorted(rn)
    assert {3040, 55, 121, 11} <= model_divisors("alexnet")
    assert {64, 8, 25, 5} <= model_divisors("lenet")
    assert {9, 25, 49, 28, 14} <= model_divisors("googlenet")


def test_fastdiv_exact_1_to_4096():
    """Every divisor 1...4096 against / and %: all dividends 0...2^20, the
    4096 values below the 2^31 limit, and the multiples of the divisor next
    to that limit with their neighbours (caffe_fastdiv_selftest)."""
    assert ca.fastdiv_selftest(1, 4096) == 0


@pytest.mark.parametrize("model", MODELS)
def test_fastdiv_exact_model_divisors(model):
    for d in sorted(model_divisors(model)):
        assert ca.fastdiv_selftest(d, d) == 0, d


def test_fastdiv_exact_at_the_limit():
    # the largest divisors the helper takes, powers of two and neighbours
    for d in (2**31, 2**31 - 1, 2**30 + 1, 2**30, 2**30 - 1, 65537, 65536,
              65535, 12544 * 128):
        assert ca.fastdiv_selftest(d, d) == 0, d


def test_fastdiv_selftest_rejects_bad_range():
    with pytest.raises(ca.CaffeError):
        ca.fastdiv_selftest(0, 4)


# ------------------------------------------------------------- conv parity

# N, C, H, W -> Co, k / s / p / group: the smallest shapes at which each
# piece of the cursor reader can go wrong.
CASES = {
    # K = 45: two K-tiles with a ragged tail, (c, ki, kj) crossing a channel
    # inside a tile
    "a": dict(N=3, C=5, H=6, W=30, Co=8, k=3, s=1, p=1),
    # K = 175: kh*kw = 25, M > 64 on the 128-tile
    "b": dict(N=2, C=7, H=5, W=28, Co=72, k=5, s=1, p=2),
    # strided view, OW = 27, conv1-like
    "c": dict(N=3, C=3, H=53, W=53, Co=16, k=7, s=2, p=3),
    # S = 16 = Spad: in wgrad a 32-pixel K-tile spans two whole images.
    # (Co = 72, not 48, so that the forward runs the 128-tile with two
    # K-waves: M > 64, N = 32.)
    "d": dict(N=2, C=40, H=4, W=4, Co=72, k=1, s=1, p=0),
    # S = 9, Spad = 16: every chunk mostly padding
    "e": dict(N=5, C=24, H=3, W=3, Co=24, k=1, s=1, p=0),
    # full padding p = k - 1: both edge masks active in one chunk
    "f": dict(N=2, C=12, H=5, W=27, Co=20, k=3, s=1, p=2),
    # grouped conv
    "g": dict(N=2, C=16, H=5, W=27, Co=16, k=3, s=1, p=1, grp=2),
    # slim64 route with split-K wgrad, k_lo > 0
    "h": dict(N=2, C=136, H=6, W=26, Co=160, k=3, s=1, p=1),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_conv_view_index_cpu(name):
    check_conv("cpu", **CASES[name])


@pytest.fixture(scope="module")
def gpu_runs():
    """Cases (a)-(h) on the GPU, once per module: per case the routes
    traced, the (cursor, 64-bit) reader counts, the relerrs and the error
    check_conv raised, if any — so that no test depends on another having
    run before it."""
    runs = {}
    for name in sorted(CASES):
        errs, exc = {}, None
        ca.gemm_trace(True)
        try:
            check_conv("gpu", errs=errs, **CASES[name])
        except AssertionError as e:
            exc = e
        finally:
            ca.gemm_trace(False)
        runs[name] = dict(routes=ca.gemm_trace_read(),
                          readers=ca.gemm_trace_readers(), errs=errs,
                          exc=exc)
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_conv_view_index_gpu(gpu_runs, name):
    run = gpu_runs[name]
    print("relerr", {k: f"{v:.2e}" for k, v in run["errs"].items()})
    if run["exc"] is not None:
        raise run["exc"]
    # forward, wgrad and dgrad all have a viewed B: every call read through
    # the staging cursors, none fell back to the 64-bit reader
    cursor, wide64 = run["readers"]
    assert wide64 == 0 and cursor == len(run["routes"]) > 0, run
    if name == "h":
        wgrad = [r for r in run["routes"] if r["tb"] == 1]
        assert wgrad and all(r["fam"] == "slim64" and r["sk"] > 1
                             for r in wgrad), wgrad


@pytest.mark.gpu
def test_conv_view_index_classes_reached(gpu_runs):
    """Cases (a)-(g) between them ran every kernel class the reader's
    pieces live in."""
    routes = [r for n in "abcdefg" for r in gpu_runs[n]["routes"]]
    classes = {
        "kw=2": lambda r: r["kw"] == 2,
        "kw=4": lambda r: r["kw"] == 4,
        "sk>1": lambda r: r["sk"] > 1,
        "bv=im2col sh=2": lambda r: r["bv"] == "im2col" and r["sh"] == 2,
        "av=chan bv=im2col": lambda r: (r["av"] == "chan"
                                         and r["bv"] == "im2col"),
    }
    for what, pred in classes.items():
        assert any(pred(r) for r in routes), f"no route with {what}: {routes}"


_CHILD = """
import sys
sys.path[:0] = {paths!r}
import caffe_amd as ca
from layer_checks import check_conv
ca.gemm_trace(True)
for cfg in {cfgs!r}:
    check_conv("gpu", **cfg)
ca.gemm_trace(False)
routes = ca.gemm_trace_read()
assert any(r["bv"] == "im2col" for r in routes), routes
print("ok", len(routes), *ca.gemm_trace_readers())
"""


def _child_check(cfgs, **env):
    """check_conv on the GPU in a fresh process: the engine reads its
    environment switches once.  Returns (calls, cursor, wide64)."""
    paths = [os.path.join(REPO, "tests"), REPO,
             os.path.join(REPO, "caffe-mpi.github.io_amd")]
    out = subprocess.run(
        [sys.executable, "-c", _CHILD.format(paths=paths, cfgs=cfgs)],
        env=dict(os.environ, **env), capture_output=True, text=True,
        timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok", out.stdout
    return tuple(int(x) for x in last[1:])


@pytest.mark.gpu
def test_conv_small_ow_walk_gpu():
    """3x3 on 7x13 through the implicit view (OW = 13 < 16: the sequential
    pixel walk), reachable only with CAFFE_IMPLICIT_MIN_OW."""
    calls, cursor, wide64 = _child_check(
        [dict(N=2, C=6, H=7, W=13, Co=8, k=3, s=1, p=1)],
        CAFFE_IMPLICIT_MIN_OW="1")
    assert (calls, cursor, wide64) == (3, 3, 0)


@pytest.mark.gpu
def test_conv_w64_fallback_gpu():
    """The 64-bit reader that sizes past the 32-bit limits fall back to,
    forced with CAFFE_GEMM_W64: an im2col case and a 1x1 case, every call
    counted on the 64-bit reader."""
    calls, cursor, wide64 = _child_check([CASES["a"], CASES["d"]],
                                         CAFFE_GEMM_W64="1")
    assert calls == 6 and cursor == 0 and wide64 == 6


@pytest.mark.gpu
def test_plain_b_keeps_64bit_reader_gpu():
    """Calls without a viewed B stay on the 64-bit kernels, whose plain path
    is the faster one.  A 3x3 at OW = 13 < 24 runs over an explicit col
    buffer: forward (no view) and wgrad (dY view as A, col as B) are such
    calls; its dgrad reads dY through a B view and takes the cursors."""
    ca.gemm_trace(True)
    try:
        check_conv("gpu", N=2, C=6, H=7, W=13, Co=8, k=3, s=1, p=1)
    finally:
        ca.gemm_trace(False)
    routes = ca.gemm_trace_read()
    plain_b = [r for r in routes if r["bv"] == "none"]
    assert len(routes) == 3 and len(plain_b) == 2, routes
    assert any(r["av"] == "chan" for r in plain_b), routes
    assert ca.gemm_trace_readers() == (1, 2)
