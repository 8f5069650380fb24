"""Sigmoid, SigmoidCrossEntropyLoss, EuclideanLoss and Flatten, one layer at
a time, in CPU mode and on the GPU, against float64 numpy restatements of
the reference formulas (sigmoid_layer.cpp:10,
sigmoid_cross_entropy_loss_layer.cpp:41-44, euclidean_loss_layer.cpp).
Tolerance: the project's per-layer class, relerr <= TOL.

Element counts: 1, 3, 5 (tail inside the first float4 pack), 1023 and 1025
(across one block's packs) and BIG, which the GPU trace must report with more
than one block (= more than one loss partial) and more than one grid-stride
pass per thread.  num = 1 is among the shapes.
"""
import ctypes

import numpy as np
import pytest

import engine_util as eu

ca = eu.ca
_lib = ca._lib
TOL = eu.TOL

MODES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]
# (num, per-sample count): num * count elements in all
SMALL = [(1, 1), (1, 3), (1, 5), (3, 341), (1, 1025), (5, 41)]
# the flat pack kernels launch ceil(n / 4 / 1024) blocks of 256 threads
# (4 packs per thread before a block is added, capped at 2048 blocks):
# 5000 elements = 1250 packs = 2 blocks of 512 threads, 3 passes
BIG = (2, 2500)
COUNTS = SMALL + [BIG]

SIG = 'layer { name: "l" type: "Sigmoid" bottom: "in0" top: "%s" }'
SCE = ('layer { name: "l" type: "SigmoidCrossEntropyLoss" bottom: "in0" '
       'bottom: "in1" top: "out" %s }')
EUC = ('layer { name: "l" type: "EuclideanLoss" bottom: "in0" bottom: "in1" '
       'top: "out" %s }')


def sig64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def sce64(x, t):
    x = np.asarray(x, np.float64)
    t = np.asarray(t, np.float64)
    pos = (x >= 0).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        terms = x * (t - pos) - np.log1p(np.exp(x - 2 * x * pos))
        return -terms.sum() / x.shape[0]


def euc64(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return ((a.ravel() - b.ravel()) ** 2).sum() / a.shape[0] / 2


def _pad_view(net, name, diff):
    """The floats between a blob's count and its 16-float padded allocation
    (legally allocated; the float4 pack at the edge covers some of them)."""
    n = int(np.prod(net.blob_shape(name)))
    padded = (n + 15) // 16 * 16
    ptr = _lib.caffe_net_blob_cpu_ptr(net._h, name.encode(), int(diff), 1)
    assert ptr
    return np.ctypeslib.as_array(ptr, shape=(padded,))[n:]


def run(mode, shapes, body, inputs, top="out", top_diff=None, poison=None,
        prefill_diff=None):
    """engine_util.run_layer with two hooks: `poison` is written past the
    count of every input (data) and of the output (data), as a blob filled
    at a larger shape and reshaped smaller would hold; prefill_diff
    {blob: value} fills input diffs before backward."""
    ca.set_mode(mode)
    net = eu.net_from_text(eu.input_net(shapes, body))
    names = [f"in{i}" for i in range(len(inputs))]
    if poison is not None:
        for nm in names + ([top] if top not in names else []):
            _pad_view(net, nm, False)[:] = poison
            _pad_view(net, nm, True)[:] = poison
    for nm, x in zip(names, inputs):
        net.set_blob(nm, x)
    for nm, v in (prefill_diff or {}).items():
        net.set_blob(nm, np.full(net.blob_shape(nm), v, np.float32),
                     diff=True)
    net.forward()
    out = net.blob(top)
    if top_diff is not None:
        net.set_blob(top, top_diff, diff=True)
        net.backward()
    return net, out


def rnd(seed, *shape, scale=3.0):
    return (np.random.default_rng(seed).standard_normal(shape) *
            scale).astype(np.float32)


ONE = np.ones(1, np.float32)


# ----------------------------------------------------------------- Sigmoid
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("num,cnt", COUNTS)
def test_sigmoid_forward_backward(mode, inplace, num, cnt):
    x = rnd(1, num, cnt)
    dy = rnd(2, num, cnt, scale=1.0)
    top = "in0" if inplace else "out"
    net, y = run(mode, [(num, cnt)], SIG % top, [x], top=top, top_diff=dy,
                 poison=1e30)
    y64 = sig64(x)
    assert eu.relerr(y, y64) <= TOL
    dx = net.blob("in0", diff=True)
    assert eu.relerr(dx, dy * y64 * (1 - y64)) <= TOL
    # nothing was stored past the count, in data or diff
    assert np.all(_pad_view(net, top, False) == np.float32(1e30))
    assert np.all(_pad_view(net, "in0", True) == np.float32(1e30))


@pytest.mark.parametrize("mode", MODES)
def test_sigmoid_saturates_finite_monotone(mode):
    x = np.sort(np.concatenate([
        np.array([-1e4, -100, -30, 30, 100, 1e4], np.float32),
        np.linspace(-20, 20, 95).astype(np.float32)]))
    x = x.reshape(1, -1)
    _, y = run(mode, [x.shape], SIG % "out", [x])
    y = y.ravel()
    assert np.all(np.isfinite(y))
    assert y.min() >= 0.0 and y.max() <= 1.0
    assert np.all(np.diff(y) >= 0)
    assert y[0] == 0.0 and y[-1] == 1.0  # |x| = 1e4: exactly saturated
    assert eu.relerr(y, sig64(x)) <= TOL


# ------------------------------------------------- SigmoidCrossEntropyLoss
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("num,cnt", COUNTS)
def test_sigmoid_ce_forward_backward(mode, num, cnt):
    x = rnd(3, num, cnt)
    t = np.random.default_rng(4).random((num, cnt)).astype(np.float32)
    # NaN past the count: a masked lane that is read turns the sum into NaN
    net, loss = run(mode, [(num, cnt)] * 2, SCE % "loss_weight: 2", [x, t],
                    top_diff=ONE, poison=np.nan,
                    prefill_diff={"in1": 7.0})
    assert eu.relerr(loss, sce64(x, t)) <= TOL
    dx = net.blob("in0", diff=True)
    assert eu.relerr(dx, (sig64(x) - t) * 2.0 / num) <= TOL
    # the target takes no gradient; nothing stored past the count
    assert np.all(net.blob("in1", diff=True) == 7.0)
    assert np.all(np.isnan(_pad_view(net, "in0", True)))


@pytest.mark.parametrize("mode", MODES)
def test_sigmoid_ce_extreme_logits(mode):
    """Logits at +-30, +-100, +-1e4 against targets 0, 1 and 0.3: the naive
    -t log s - (1 - t) log(1 - s) gives inf or NaN here, the stable form is
    finite and equals the float64 value."""
    xs = np.array([30, -30, 100, -100, 1e4, -1e4], np.float32)
    ts = np.array([0, 1, 0.3], np.float32)
    x = np.repeat(xs, 3).reshape(2, 9)
    t = np.tile(ts, 6).reshape(2, 9)
    net, loss = run(mode, [x.shape] * 2, SCE % "", [x, t], top_diff=ONE)
    ref = sce64(x, t)
    assert np.isfinite(loss[0]) and np.isfinite(ref)
    assert eu.relerr(loss, ref) <= TOL
    dx = net.blob("in0", diff=True)
    assert np.all(np.isfinite(dx))
    assert eu.relerr(dx, (sig64(x) - t) / 2.0) <= TOL


@pytest.mark.parametrize("mode", MODES)
def test_sigmoid_ce_nan_logit_gives_nan_loss(mode):
    x = rnd(5, 2, 37)
    x[1, 20] = np.nan
    t = np.random.default_rng(6).random((2, 37)).astype(np.float32)
    _, loss = run(mode, [x.shape] * 2, SCE % "", [x, t])
    assert np.isnan(loss[0])


def _cls(v):
    return "nan" if np.isnan(v) else "inf" if np.isinf(v) else "finite"


@pytest.mark.gpu
@pytest.mark.parametrize("inf,t", [(np.inf, 0.3), (-np.inf, 0.3),
                                   (np.inf, 1.0), (-np.inf, 0.0)])
def test_sigmoid_ce_inf_logit_same_class_cpu_gpu(inf, t):
    x = rnd(7, 1, 9)
    x[0, 4] = inf
    tt = np.full((1, 9), t, np.float32)
    got = [_cls(run(m, [x.shape] * 2, SCE % "", [x, tt])[1][0])
           for m in ("cpu", "gpu")]
    assert got[0] == got[1], got


# ----------------------------------------------------------- EuclideanLoss
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pd", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("num,cnt", COUNTS)
def test_euclidean_forward_backward(mode, pd, num, cnt):
    a = rnd(8, num, cnt)
    b = rnd(9, num, cnt)
    extra = "loss_weight: 3 " + " ".join(
        f"propagate_down: {'true' if p else 'false'}" for p in pd)
    net, loss = run(mode, [(num, cnt)] * 2, EUC % extra, [a, b],
                    top_diff=ONE, poison=np.nan,
                    prefill_diff={"in0": 7.0, "in1": 7.0})
    assert eu.relerr(loss, euc64(a, b)) <= TOL
    d = (a.astype(np.float64) - b) * 3.0 / num
    for k, sign in ((0, 1.0), (1, -1.0)):
        got = net.blob(f"in{k}", diff=True)
        if pd[k]:
            assert eu.relerr(got, sign * d) <= TOL
        else:
            assert np.all(got == 7.0)
        assert np.all(np.isnan(_pad_view(net, f"in{k}", True)))


@pytest.mark.parametrize("mode", MODES)
def test_losses_4d_bottom_against_flattened_2d_target(mode):
    """The autoencoder's data / flatdata case: a 4-D bottom against the 2-D
    Flatten of another 4-D blob with the same count.  The Flatten top shares
    its bottom's memory, so the gradient of the 2-D side lands in the 4-D
    blob's diff."""
    a = rnd(10, 2, 1, 3, 5)
    b = np.random.default_rng(11).random((2, 1, 3, 5)).astype(np.float32)
    body = ('layer { name: "f" type: "Flatten" bottom: "in1" top: "flat" }\n'
            + EUC.replace('"in1"', '"flat"') % "")
    net, loss = run(mode, [a.shape, b.shape], body, [a, b], top_diff=ONE)
    assert net.blob_shape("flat") == (2, 15)
    assert np.array_equal(net.blob("flat").ravel(), b.ravel())
    assert eu.relerr(loss, euc64(a, b)) <= TOL
    d = (a.astype(np.float64) - b) / 2.0
    assert eu.relerr(net.blob("in0", diff=True), d) <= TOL
    assert eu.relerr(net.blob("in1", diff=True), -d) <= TOL
    body = ('layer { name: "f" type: "Flatten" bottom: "in1" top: "flat" }\n'
            + SCE.replace('"in1"', '"flat"') % "")
    net, loss = run(mode, [a.shape, b.shape], body, [a, b], top_diff=ONE)
    assert eu.relerr(loss, sce64(a.reshape(2, -1), b.reshape(2, -1))) <= TOL


@pytest.mark.parametrize("mode", MODES)
def test_flatten_axes(mode):
    x = rnd(12, 2, 3, 4, 5)
    for param, shape in [("", (2, 60)),
                         ("flatten_param { axis: 0 end_axis: 1 }", (6, 4, 5)),
                         ("flatten_param { axis: 2 }", (2, 3, 20)),
                         ("flatten_param { axis: 1 end_axis: -2 }", (2, 12, 5))]:
        body = ('layer { name: "f" type: "Flatten" bottom: "in0" top: "out" '
                '%s }' % param)
        dy = rnd(13, *shape)
        net, y = run(mode, [x.shape], body, [x], top_diff=dy)
        assert y.shape == shape
        assert np.array_equal(y.ravel(), x.ravel())
        assert np.array_equal(net.blob("in0", diff=True).ravel(), dy.ravel())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("body", [SCE, EUC])
def test_zero_loss_weight_backward_writes_zeros(mode, body):
    """loss_weight: 0 must write zeros, not skip the write: the split above
    the bottom sums this diff."""
    a = rnd(14, 2, 37)
    b = np.random.default_rng(15).random((2, 37)).astype(np.float32)
    net, _ = run(mode, [a.shape] * 2, body % "loss_weight: 0", [a, b],
                 top_diff=ONE, prefill_diff={"in0": 1.0})
    assert np.all(net.blob("in0", diff=True) == 0.0)


def test_shape_and_blob_count_checks():
    ca.set_mode("cpu")
    for body, shapes in [
            (SCE % "", [(2, 5), (2, 6)]),
            (EUC % "", [(2, 6), (3, 4)]),
            (SCE % "propagate_down: true propagate_down: true",
             [(2, 5), (2, 5)]),
            ('layer { name: "l" type: "EuclideanLoss" bottom: "in0" '
             'top: "out" }', [(2, 5)]),
            ('layer { name: "l" type: "Sigmoid" bottom: "in0" bottom: "in1" '
             'top: "out" }', [(2, 5), (2, 5)])]:
        with pytest.raises(ca.CaffeError):
            eu.net_from_text(eu.input_net(shapes, body))


# ------------------------------------------------- which kernel body ran
@pytest.mark.gpu
def test_gpu_trace_names_the_kernels_and_big_count_splits():
    num, cnt = BIG
    n = num * cnt
    x = rnd(16, num, cnt)
    t = np.random.default_rng(17).random((num, cnt)).astype(np.float32)
    ca.set_mode("gpu")
    ca.kernel_trace(True)
    try:
        run("gpu", [(num, cnt)], SIG % "out", [x], top_diff=x)
        run("gpu", [(num, cnt)] * 2, SCE % "", [x, t], top_diff=ONE)
        run("gpu", [(num, cnt)] * 2, EUC % "", [x, t], top_diff=ONE)
        small = run("gpu", [(1, 5)] * 2, EUC % "", [x[:1, :5], t[:1, :5]])
        recs = ca.kernel_trace_read()
    finally:
        ca.kernel_trace(False)
    assert small is not None
    ops = [r["op"] for r in recs]
    assert ops == ["sigmoid_fwd", "sigmoid_bwd", "sigmoid_ce_fwd",
                   "sigmoid_ce_bwd", "euclid_fwd", "euclid_bwd",
                   "euclid_fwd"], ops
    for r in recs[:6]:
        assert r["n"] == n
        assert r["blocks"] > 1 and r["passes"] > 1, r
    for r in (recs[2], recs[4]):
        assert r["partials"] == r["blocks"]
    assert recs[6]["blocks"] == 1 and recs[6]["partials"] == 1
    assert recs[6]["passes"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("body", [SCE, EUC])
def test_gpu_loss_is_bitwise_reproducible(body):
    num, cnt = BIG
    x = rnd(18, num, cnt)
    t = np.random.default_rng(19).random((num, cnt)).astype(np.float32)
    net, l1 = run("gpu", [(num, cnt)] * 2, body % "", [x, t])
    net.forward()
    l2 = net.blob("out")
    assert l1.view(np.uint32)[0] == l2.view(np.uint32)[0]


# ------------------------------------- finite differences (CPU, float32)
def _fd_check(body, shapes, inputs, wrt, w):
    """Central differences of the objective sum(out * w) in the style of
    test_gradient_check.py.  eps = 1e-2 on inputs of order 1: the truncation
    error is eps^2 f'''/6 <= 2e-5 relative, the rounding error of a float32
    objective of order 10 is 1e-6 / eps = 1e-4 absolute; the bound 2e-2 of
    the largest analytic entry leaves a factor 10 over both."""
    net, _ = run("cpu", shapes, body, inputs, top_diff=w)
    an = net.blob(f"in{wrt}", diff=True).astype(np.float64).ravel()
    eps = 1e-2
    rng = np.random.default_rng(20)
    idx = rng.choice(an.size, size=min(10, an.size), replace=False)
    for i in idx:
        obj = []
        for s in (+1, -1):
            xs = [np.array(v, np.float32) for v in inputs]
            xs[wrt].ravel()[i] += s * eps
            _, out = run("cpu", shapes, body, xs)
            obj.append(float((out.astype(np.float64) * w).sum()))
        fd = (obj[0] - obj[1]) / (2 * eps)
        assert abs(fd - an[i]) <= 2e-2 * max(np.abs(an).max(), 1e-3), \
            (i, fd, an[i])


def test_fd_sigmoid():
    x = rnd(21, 2, 13, scale=1.0)
    _fd_check(SIG % "out", [x.shape], [x], 0, rnd(22, 2, 13, scale=1.0))


def test_fd_sigmoid_ce():
    x = rnd(23, 2, 13, scale=1.0)
    t = np.random.default_rng(24).random((2, 13)).astype(np.float32)
    _fd_check(SCE % "", [x.shape] * 2, [x, t], 0, ONE)


@pytest.mark.parametrize("wrt", [0, 1])
def test_fd_euclidean(wrt):
    a = rnd(25, 2, 13, scale=1.0)
    b = rnd(26, 2, 13, scale=1.0)
    _fd_check(EUC % "", [a.shape] * 2, [a, b], wrt, ONE)
