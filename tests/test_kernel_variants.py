"""Per-variant parity for the non-GEMM kernels (elementwise.hip).

The launch wrappers of pooling, the BatchNorm statistics, LRN and softmax
each pick between specialised kernels, or shape a launch (batch slices, a
two-positions-per-thread tail, a capped grid) from the tensor's sizes.  The
tables below hold, for each shape, what the wrapper must do with it —
written down from the wrappers, so they double as the variant-to-shape map.
Each row is checked against the float64 oracle in CPU mode and on the GPU
at the project's tolerances (TOL = 1e-4 relerr on tensors, 1e-5 relative on
the scalar loss); the GPU run records the wrappers with ca.kernel_trace()
and requires the traced lines to be exactly the listed ones, in call order.

Besides reaching every variant, the rows use inputs on which a wrong kernel
actually fails: max pooling also runs on tie-heavy input (real inputs are
post-ReLU, full of equal zeros), LRN runs at alpha = 1.0, and BatchNorm has
a small-variance row that sees eps.  test_*_discriminates pins, with the
oracle alone, how far a perturbed operation lands from the true one on
exactly these inputs.
"""
import numpy as np
import pytest

import caffe_amd as ca
from engine_util import TOL, relerr
from layer_checks import (bn_inputs, check_bn, check_lrn, check_pool_bwd,
                          check_relu, check_softmaxloss,
                          check_softmaxloss_spatial, lrn_inputs)
from oracle import oracle as orc

# ---------------------------------------------------------------- pooling
# id: H, W, (kh, kw), (sh, sw), (ph, pw), forward variant, backward variant.
# All with N = 2, C = 3 through the identity 1x1 conv of check_pool_bwd.
MAXPOOL_CASES = {
    # inception pool
    "P1": (7, 7, (3, 3), (1, 1), (1, 1), "k3", "k3s1"),
    # ceil mode: the last window hangs over the edge (OH = 4)
    "P2": (8, 8, (3, 3), (2, 2), (0, 0), "k3", "k3s2"),
    # padded, and the last window clipped away by the --oh rule
    "P3": (9, 9, (3, 3), (2, 2), (1, 1), "k3", "k3s2"),
    "P4": (10, 10, (3, 3), (3, 3), (0, 0), "k3", "k3"),
    # sh != sw
    "P5": (9, 8, (3, 3), (2, 1), (0, 1), "k3", "k3"),
    # stride > kernel: pixels in no window must get exactly 0
    "P6": (9, 11, (3, 3), (4, 4), (1, 1), "k3", "k3"),
    # LeNet
    "P7": (12, 12, (2, 2), (2, 2), (0, 0), "generic", "generic"),
    # asymmetric everything
    "P8": (7, 11, (2, 5), (1, 2), (1, 2), "generic", "generic"),
}

# id: H, W, (kh, kw), (sh, sw), (ph, pw).  One kernel per direction.
AVEPOOL_CASES = {
    "A1": (9, 9, (3, 3), (2, 2), (1, 1)),      # padded divisor
    "A2": (7, 7, (7, 7), (1, 1), (0, 0)),      # global
    "A3": (14, 14, (5, 5), (3, 3), (0, 0)),    # GoogLeNet aux head
    "A4": (7, 7, (3, 3), (1, 1), (1, 1)),
    "A5": (8, 8, (3, 3), (2, 2), (0, 0)),      # window clipped at H + ph
    "A6": (7, 11, (2, 5), (1, 2), (1, 2)),     # asymmetric
}

POOL_N, POOL_C = 2, 3


def _pool_cfg(H, W, k, s, p):
    return dict(N=POOL_N, C=POOL_C, H=H, W=W, kernel_h=k[0], kernel_w=k[1],
                stride_h=s[0], stride_w=s[1], pad_h=p[0], pad_w=p[1])


def _windows(H, W, k, s, p):
    """(oh, ow, h0, h1, w0, w1): every pooling window clipped to the image,
    with the output size of the layer's ceil-and-clip rule."""
    OH, OW = orc.pool_out_dim(H, W, k[0], k[1], p[0], p[1], s[0], s[1])
    for oh in range(OH):
        for ow in range(OW):
            h0, w0 = oh * s[0] - p[0], ow * s[1] - p[1]
            yield (oh, ow, max(h0, 0), min(h0 + k[0], H), max(w0, 0),
                   min(w0 + k[1], W))


def _tie_input(name, H, W):
    seed = 7100 + sorted(MAXPOOL_CASES).index(name)
    r = np.random.default_rng(seed)
    x = np.maximum(np.round(r.standard_normal((POOL_N, POOL_C, H, W))), 0)
    return x.astype(np.float32)


def _tie_fraction(x, wins):
    tied = total = 0
    for _, _, h0, h1, w0, w1 in wins:
        win = x[:, :, h0:h1, w0:w1].reshape(x.shape[0], x.shape[1], -1)
        hits = (win == win.max(axis=2, keepdims=True)).sum(axis=2)
        tied += int((hits >= 2).sum())
        total += hits.size
    return tied / total


def _last_max_bwd(x, dy, wins):
    """Max-pool backward that routes each window's gradient to the LAST
    position (row-major) attaining the maximum — the wrong tie order."""
    dx = np.zeros(x.shape, np.float64)
    for oh, ow, h0, h1, w0, w1 in wins:
        for n in range(x.shape[0]):
            for c in range(x.shape[1]):
                win = x[n, c, h0:h1, w0:w1]
                flat = np.flatnonzero(win.ravel() == win.max())[-1]
                dh, dw = divmod(int(flat), w1 - w0)
                dx[n, c, h0 + dh, w0 + dw] += dy[n, c, oh, ow]
    return dx


def _run_maxpool(mode, name, ties):
    H, W, k, s, p, fwd, bwd = MAXPOOL_CASES[name]
    x = _tie_input(name, H, W) if ties else None
    out = _run(mode, check_pool_bwd,
               dict(_pool_cfg(H, W, k, s, p), pool="MAX", x=x),
               [f"op=pool_max_fwd var={fwd}", f"op=pool_max_bwd var={bwd}"])
    wins = list(_windows(H, W, k, s, p))
    if ties:
        # the input is full of ties, and the tie order is visible in dx
        frac = _tie_fraction(out["x"], wins)
        assert frac >= 0.25, frac
        wrong = _last_max_bwd(out["x"], out["dy"], wins)
        assert relerr(wrong, out["dx_ref"]) > 10 * TOL
    if name == "P6":
        covered = np.zeros((H, W), bool)
        for _, _, h0, h1, w0, w1 in wins:
            covered[h0:h1, w0:w1] = True
        assert (~covered).sum() > 0
        assert np.all(out["dx"][:, :, ~covered] == 0.0)


def _run_avepool(mode, name):
    H, W, k, s, p = AVEPOOL_CASES[name]
    _run(mode, check_pool_bwd, dict(_pool_cfg(H, W, k, s, p), pool="AVE"),
         ["op=pool_ave_fwd", "op=pool_ave_bwd"])


# -------------------------------------------------------------- BatchNorm
# TRAIN, forward and backward.  nb = min(N, 2048 / C) batch slices per
# channel; span_max is the largest per-block span, in float4 packs for v4.
# The 4x-unrolled main loops need span > 3 * 256 (forward) / 256 (backward).
_B1 = dict(N=2, C=4, H=64, W=66)
BN_CASES = {
    # v4 unrolled bodies (S4 = 1056 > 768) plus tail
    "B1": (_B1, "var=v4 nb=2 span_max=1056"),
    # scalar unrolled bodies
    "B2": (dict(N=2, C=3, H=33, W=33), "var=scalar nb=2 span_max=1089"),
    # nb < N: uneven slices [0,1) and [1,3), two images in one block, S4 = 1
    "B3": (dict(N=3, C=1024, H=2, W=2), "var=v4 nb=2 span_max=2"),
    # slices of 1/2/2 images, S = 3: every float4 pack of the norm / apply
    # kernels straddles a channel boundary
    "B4": (dict(N=5, C=600, H=1, W=3), "var=scalar nb=3 span_max=6"),
    "B5": (dict(_B1, scale_bias=False), "var=v4 nb=2 span_max=1056"),
    # variance 1e-4 == eps: the output depends on eps (see the
    # discrimination test)
    "B6": (dict(N=4, C=6, H=5, W=5, std=0.01, eps=1e-4),
           "var=scalar nb=4 span_max=25"),
    # E[x^2] - m^2 cancellation (2501 - 2500)
    "B7": (dict(N=4, C=6, H=8, W=8, mean=50.0, std=1.0),
           "var=v4 nb=4 span_max=16"),
    # fused in-place ReLU (named to sort after B7: the rows above keep their
    # seeds): the backward statistics and apply kernels recompute the
    # activation's sign, in the v4 and the scalar kernel and, with B4's
    # shape, on packs that straddle a channel.  The fused ReLU launches
    # nothing, so the trace is the unfused one.
    "R1": (dict(_B1, relu=True), "var=v4 nb=2 span_max=1056"),
    "R2": (dict(N=2, C=3, H=33, W=33, relu=True),
           "var=scalar nb=2 span_max=1089"),
    "R3": (dict(N=5, C=600, H=1, W=3, relu=True),
           "var=scalar nb=3 span_max=6"),
}


def _bn_seed(name):
    return 8200 + sorted(BN_CASES).index(name)


def _run_bn(mode, name):
    cfg, line = BN_CASES[name]
    _run(mode, check_bn, dict(cfg, seed=_bn_seed(name)),
         [f"op=bn_fwd_stats {line}", f"op=bn_bwd_stats {line}"])


# -------------------------------------------------------------------- LRN
# alpha = 1.0, beta = 0.75 throughout.  Two (n, h, w) positions per thread;
# odd = 1 leaves the last thread with one.
LRN_CASES = {
    "ring5_c7": (dict(size=5, N=1, C=7, H=3, W=3), "var=ring5 odd=1"),
    # C below the window
    "ring5_c1": (dict(size=5, N=3, C=1, H=1, W=1), "var=ring5 odd=1"),
    "ring5_c2": (dict(size=5, N=1, C=2, H=1, W=5), "var=ring5 odd=1"),
    # AlexNet norm1 depth: the running add / subtract over 96 channels
    "ring5_c96": (dict(size=5, N=1, C=96, H=2, W=2), "var=ring5 odd=0"),
    "size3": (dict(size=3, N=1, C=4, H=3, W=3), "var=generic odd=1"),
    "size7": (dict(size=7, N=1, C=5, H=3, W=3), "var=generic odd=1"),
    # the legacy default shape, at an alpha that sees the window
    "default": (dict(size=5, N=2, C=8, H=6, W=6), "var=ring5 odd=0"),
}
LRN_ALPHA, LRN_BETA = 1.0, 0.75


def _lrn_seed(name):
    return 9300 + sorted(LRN_CASES).index(name)


def _run_lrn(mode, name):
    cfg, line = LRN_CASES[name]
    _run(mode, check_lrn,
         dict(cfg, alpha=LRN_ALPHA, beta=LRN_BETA, seed=_lrn_seed(name)),
         [f"op=lrn_fwd {line}", f"op=lrn_bwd {line}"])


# ------------------------------------------------------- softmax and loss
# One wave per row, lanes stride the classes by 64; the grid is capped at
# 2048 blocks of 4 rows.
SOFTMAX_CASES = {
    # a full pass plus one lane of the second
    "c65": (check_softmaxloss, dict(N=5, C=65),
            "op=softmax_fwd rows=5 C=65 blocks=2"),
    # ImageNet head: 15 full passes plus 40 lanes
    "c1000": (check_softmaxloss, dict(N=3, C=1000),
              "op=softmax_fwd rows=3 C=1000 blocks=1"),
    # rows = 8450 > 4 * 2048: the row loop wraps
    "spatial_wrap": (check_softmaxloss_spatial, dict(N=2, C=3, H=65, W=65),
                     "op=softmax_fwd rows=8450 C=3 blocks=2048"),
}


def _run_softmax(mode, name):
    check, cfg, line = SOFTMAX_CASES[name]
    _run(mode, check, cfg, [line])


# ------------------------------------------------------------------- ReLU
# count 90 = 4 * 22 + 2: the float4 body's last pack is half padding.  The
# ReLU wrappers have a single variant and record nothing.
RELU_CASES = {
    "slope0": dict(shape=(2, 5, 3, 3), negative_slope=0.0),
    "slope0.1": dict(shape=(2, 5, 3, 3), negative_slope=0.1),
}


def _run_relu(mode, name):
    _run(mode, check_relu, RELU_CASES[name], [])


# ---------------------------------------------------------------- harness
def traced(fn):
    """fn() with the variant trace on; returns (fn's result, trace lines)."""
    ca.kernel_trace(True)
    try:
        out = fn()
    finally:
        ca.kernel_trace(False)
    return out, ca.kernel_trace_read()


def parse_line(text):
    return {k: int(v) if v.isdigit() else v
            for k, v in (kv.split("=") for kv in text.split())}


def _run(mode, check, cfg, lines):
    errs = {}
    if mode == "cpu":
        return check("cpu", errs=errs, **cfg)
    try:
        out, trace = traced(lambda: check("gpu", errs=errs, **cfg))
    finally:
        print("relerr", {k: f"{v:.2e}" for k, v in errs.items()})
    assert trace == [parse_line(t) for t in lines], trace
    return out


_MAXPOOL_IDS = [(n, t) for n in sorted(MAXPOOL_CASES) for t in (False, True)]


def _mp_id(v):
    return {False: "normal", True: "ties"}.get(v, v)


@pytest.mark.parametrize("name,ties", _MAXPOOL_IDS, ids=_mp_id)
def test_maxpool_cpu(name, ties):
    _run_maxpool("cpu", name, ties)


@pytest.mark.gpu
@pytest.mark.parametrize("name,ties", _MAXPOOL_IDS, ids=_mp_id)
def test_maxpool_gpu(name, ties):
    _run_maxpool("gpu", name, ties)


@pytest.mark.parametrize("name", sorted(AVEPOOL_CASES))
def test_avepool_cpu(name):
    _run_avepool("cpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(AVEPOOL_CASES))
def test_avepool_gpu(name):
    _run_avepool("gpu", name)


@pytest.mark.parametrize("name", sorted(BN_CASES))
def test_bn_cpu(name):
    _run_bn("cpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BN_CASES))
def test_bn_gpu(name):
    _run_bn("gpu", name)


@pytest.mark.parametrize("name", sorted(LRN_CASES))
def test_lrn_cpu(name):
    _run_lrn("cpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LRN_CASES))
def test_lrn_gpu(name):
    _run_lrn("gpu", name)


@pytest.mark.parametrize("name", sorted(SOFTMAX_CASES))
def test_softmax_cpu(name):
    _run_softmax("cpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SOFTMAX_CASES))
def test_softmax_gpu(name):
    _run_softmax("gpu", name)


@pytest.mark.parametrize("name", sorted(RELU_CASES))
def test_relu_cpu(name):
    _run_relu("cpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RELU_CASES))
def test_relu_gpu(name):
    _run_relu("gpu", name)


# ---------------------------------------------------- the table as a whole
def _all_expected_lines():
    lines = []
    for _, _, _, _, _, fwd, bwd in MAXPOOL_CASES.values():
        lines += [f"op=pool_max_fwd var={fwd}", f"op=pool_max_bwd var={bwd}"]
    lines += ["op=pool_ave_fwd", "op=pool_ave_bwd"]
    for _, line in BN_CASES.values():
        lines += [f"op=bn_fwd_stats {line}", f"op=bn_bwd_stats {line}"]
    for _, line in LRN_CASES.values():
        lines += [f"op=lrn_fwd {line}", f"op=lrn_bwd {line}"]
    lines += [line for _, _, line in SOFTMAX_CASES.values()]
    return [parse_line(t) for t in lines]


def test_table_names_every_variant():
    """Every variant the trace can emit is some row's expectation (the
    sgd_seg buckets are in test_param_multipliers.py).  Fails when a row is
    dropped and leaves a kernel unreached."""
    recs = _all_expected_lines()

    def seen(op, key):
        return {r[key] for r in recs if r["op"] == op}

    assert seen("pool_max_fwd", "var") == {"k3", "generic"}
    assert seen("pool_max_bwd", "var") == {"k3s1", "k3s2", "k3", "generic"}
    assert {r["op"] for r in recs} >= {"pool_ave_fwd", "pool_ave_bwd"}
    for op in ("bn_fwd_stats", "bn_bwd_stats"):
        assert seen(op, "var") == {"v4", "scalar"}
        for var in ("v4", "scalar"):
            # the 4x-unrolled main loop: span > 3 * 256 forward, > 256 backward
            assert any(r["op"] == op and r["var"] == var
                       and r["span_max"] > 3 * 256 for r in recs), (op, var)
    # fewer batch slices than images, for both BN variants
    assert {parse_line(line)["var"] for cfg, line in BN_CASES.values()
            if parse_line(line)["nb"] < cfg["N"]} == {"v4", "scalar"}
    for op in ("lrn_fwd", "lrn_bwd"):
        assert {(r["var"], r["odd"]) for r in recs if r["op"] == op} >= {
            ("ring5", 0), ("ring5", 1), ("generic", 1)}
    sm = [r for r in recs if r["op"] == "softmax_fwd"]
    assert any(r["rows"] > 4 * r["blocks"] for r in sm)  # wrapped grid
    assert any(r["C"] > 64 and r["C"] % 64 for r in sm)


def test_kernel_trace_off_and_empty():
    # tracing is off by default and reading an empty log is well defined
    ca.kernel_trace(True)
    ca.kernel_trace(False)
    assert ca.kernel_trace_read() == []


@pytest.mark.gpu
def test_kernel_trace_disabled_records_nothing():
    ca.kernel_trace(True)
    ca.kernel_trace(False)
    check_lrn("gpu")
    check_bn("gpu")
    assert ca.kernel_trace_read() == []
    # enabling clears what an earlier enable recorded
    _, first = traced(lambda: check_lrn("gpu"))
    assert [r["op"] for r in first] == ["lrn_fwd", "lrn_bwd"]
    _, second = traced(lambda: None)
    assert second == []


# ------------------------------------------ what the inputs can tell apart
# Oracle only: a perturbed operation must land more than 10 * TOL from the
# true one on the inputs of the tables above, or the rows could not fail.
@pytest.mark.parametrize("name", sorted(LRN_CASES))
def test_lrn_inputs_discriminate(name):
    """local_size +- 2 and alpha / 2 on the row's own x and dy."""
    cfg, _ = LRN_CASES[name]
    size = cfg["size"]
    x, dy = lrn_inputs(np.random.default_rng(_lrn_seed(name)), cfg["N"],
                       cfg["C"], cfg["H"], cfg["W"])

    def run(size, alpha):
        y, scale = orc.lrn_fwd(x, size, alpha, LRN_BETA)
        return y, orc.lrn_bwd(x, y, dy, scale, size, alpha, LRN_BETA)

    y, dx = run(size, LRN_ALPHA)
    for psize, palpha in ((size - 2, LRN_ALPHA), (size + 2, LRN_ALPHA),
                          (size, 0.5 * LRN_ALPHA)):
        py, pdx = run(psize, palpha)
        assert relerr(py, y) > 10 * TOL, (psize, palpha, relerr(py, y))
        assert relerr(pdx, dx) > 10 * TOL, (psize, palpha, relerr(pdx, dx))


def test_bn_small_variance_input_sees_eps():
    """eps = 0 on B6's own input."""
    cfg, _ = BN_CASES["B6"]
    x, sc, bi, dy = bn_inputs(np.random.default_rng(_bn_seed("B6")),
                              cfg["N"], cfg["C"], cfg["H"], cfg["W"],
                              std=cfg["std"])

    def run(eps):
        y, _, _, inv_std, xnorm = orc.bn_fwd_train(x, eps, sc, bi)
        return y, orc.bn_bwd(xnorm, dy, inv_std, sc)[0]

    y, dx = run(cfg["eps"])
    y0, dx0 = run(0.0)
    assert relerr(y0, y) > 10 * TOL, relerr(y0, y)
    assert relerr(dx0, dx) > 10 * TOL, relerr(dx0, dx)
