"""ContrastiveLoss (reference layers/contrastive_loss_layer.cpp/.cu) against
a float64 numpy replay written here, in CPU mode and, marked gpu, through
k_contrastive_fwd / k_contrastive_bwd in both row mappings.

Tolerance: engine_util.TOL (1e-4 relative to the tensor's largest value).
The float32 steps are a - b (one rounding), d² (double sum, one rounding),
sqrtf, margin - d and one division: a few 1e-7 relative each.  The only
amplifier is the cancellation in margin - d, which the inputs bound: every
drawn dissimilar row keeps |margin - d| > 1e-3 (see draw()), so that term
is off by at most ~1e-7 * margin / 1e-3 = 1e-4 of its own value and far
less of the tensor's maximum.
"""
import numpy as np
import pytest

import caffe_amd as ca
from engine_util import TOL, input_net, net_from_text, relerr
from test_gradient_check import build_net, check_gradients

# the issue's five shapes, and a wide one that holds every planted row
SHAPES = [(1, 1), (5, 2), (70, 3), (3, 257), (1025, 2), (9, 257)]
MODES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]
WAVE = 64  # rows at least a wave wide take the wave-per-row kernels


@pytest.fixture(autouse=True)
def cpu_after():
    yield
    ca.set_mode("cpu")


def layer(margin, legacy, lw, prop=None):
    pd = "".join(f" propagate_down: {str(p).lower()}" for p in prop or [])
    return (f'layer {{ name: "loss" type: "ContrastiveLoss" bottom: "in0" '
            f'bottom: "in1" bottom: "in2" top: "out" loss_weight: {lw}{pd} '
            f'contrastive_loss_param {{ margin: {margin} '
            f'legacy_version: {str(legacy).lower()} }} }}')


def build(N, C, margin=1.0, legacy=False, lw=1.0, prop=None):
    return net_from_text(input_net([(N, C), (N, C), (N,)],
                                   layer(margin, legacy, lw, prop)))


def replay64(a, b, sim, margin, legacy, lw):
    """-> (loss, da, db) in float64 from the float32 inputs."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    N = a.shape[0]
    diff = a - b
    dsq = (diff * diff).sum(1)
    similar = np.trunc(sim.astype(np.float64)) != 0
    d = np.sqrt(dsq)
    if legacy:
        md = margin - dsq
        term = np.maximum(md, 0.0)
        beta = -np.ones(N)
    else:
        md = margin - d
        term = np.maximum(md, 0.0) ** 2
        beta = -md / (d + 1e-4)
    loss = np.where(similar, dsq, term).sum() / N / 2
    coef = np.where(similar, 1.0, np.where(md > 0, beta, 0.0)) * lw / N
    da = coef[:, None] * diff
    return loss, da, -da


def engine_mdist(delta, margin, legacy):
    """mdist of a row with a - b = delta as the float32 engine computes it:
    d² summed in double and rounded to float once, IEEE sqrt, one
    subtraction."""
    dsq = np.float32((delta.astype(np.float64) ** 2).sum())
    return np.float32(margin) - (dsq if legacy else np.sqrt(dsq))


def mdist0_delta(C, margin, legacy):
    """a - b with mdist exactly 0 in float32, or None.  At margin 5 it is
    the (3, 4, 0...) row; the other margins scale it ((0.6f, 0.8f) squares
    to 1 + 4.8e-8, which rounds to 1.0f), legacy takes d² = margin."""
    two = {(1.0, False): (0.6, 0.8), (2.5, False): (1.5, 2.0),
           (5.0, False): (3.0, 4.0), (1.0, True): (0.6, 0.8),
           (2.5, True): (0.5, 1.5), (5.0, True): (1.0, 2.0)}
    delta = np.zeros(C, np.float32)
    if C > 1:
        delta[:2] = two[margin, legacy]
    else:
        delta[0] = np.sqrt(np.float32(margin)) if legacy else margin
    return delta if engine_mdist(delta, margin, legacy) == 0 else None


def draw(N, C, margin, legacy, seed):
    """Inputs with d around the margin, the planted rows (the most telling
    first: small N takes what fits, and from N = 3 on random rows stay among
    them), and the fraction of rows redrawn to keep |margin - d| (legacy:
    |margin - d²|) > 1e-3."""
    rng = np.random.default_rng(seed)
    target = np.sqrt(margin) if legacy else margin  # d at the hinge
    scale = target / np.sqrt(2.0 * C)

    def rows(n):
        return (rng.standard_normal((n, C)) * scale).astype(np.float32), \
               (rng.standard_normal((n, C)) * scale).astype(np.float32)

    a, b = rows(N)
    sim = (rng.random(N) < 0.5).astype(np.float32)
    zero = np.zeros(C, np.float32)
    far = np.zeros(C, np.float32)
    far[:2] = [30, 40] if C > 1 else [50]  # d = 50, outside every margin
    hinge = mdist0_delta(C, margin, legacy)
    plants = [
        # mdist exactly 0: the gradient must be exactly 0
        ("dis_mdist0", 0.0, hinge) if hinge is not None
        else ("dis_equal0", 0.0, zero),
        ("sim_0.9", 0.9, None),             # truncates to dissimilar; drawn
        ("sim_2", 2.0, None),               # similar; drawn
        ("dis_equal", 0.0, zero),           # the 1e-4 matters
        ("sim_equal", 1.0, zero),
        ("dis_far", 0.0, far),              # gradient exactly 0
        ("dis_far100", 0.0, 20 * far),
    ]
    planted, fixed = {}, set()
    for i, (name, s, delta) in enumerate(plants[:N]):
        sim[i] = s
        planted[name] = i
        if delta is not None:  # a - b == delta exactly
            fixed.add(i)
            if np.any(delta):
                a[i] = 0
            b[i] = a[i] - delta
            assert np.array_equal(a[i] - b[i], delta)
        elif s < 1:  # halved: well inside the margin, a non-zero beta
            a[i] *= np.float32(0.5)
            b[i] *= np.float32(0.5)
    redrawn = 0
    for i in range(N):
        while i not in fixed and np.trunc(sim[i]) == 0:
            diff = a[i].astype(np.float64) - b[i].astype(np.float64)
            dsq = (diff * diff).sum()
            gap = margin - (dsq if legacy else np.sqrt(dsq))
            if abs(gap) > 1e-3:
                break
            a[i], b[i] = (r[0] for r in rows(1))
            redrawn += 1
    return a, b, sim, planted, redrawn / N


def run(net, a, b, sim):
    net.set_blob("in0", a)
    net.set_blob("in1", b)
    net.set_blob("in2", sim)
    net.forward()
    loss = float(net.blob("out")[0])
    net.backward()
    return loss, net.blob("in0", diff=True), net.blob("in1", diff=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("lw", [1.0, 2.0])
@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("margin", [1.0, 2.5, 5.0])
@pytest.mark.parametrize("N,C", SHAPES)
def test_contrastive_against_float64(mode, N, C, margin, legacy, lw):
    ca.set_mode(mode)
    a, b, sim, planted, redrawn = draw(N, C, margin, legacy, seed=N * 1000 + C)
    assert redrawn <= 0.05, redrawn
    want_loss, want_da, want_db = replay64(a, b, sim, margin, legacy, lw)
    net = build(N, C, margin, legacy, lw)
    if mode == "gpu":
        ca.kernel_trace(True)
    loss, da, db = run(net, a, b, sim)
    if mode == "gpu":
        ca.kernel_trace(False)
        recs = [r for r in ca.kernel_trace_read()
                if r["op"].startswith("contrastive")]
        assert [r["op"] for r in recs] == ["contrastive_fwd",
                                           "contrastive_bwd"]
        var = "row_wave" if C >= WAVE else "row_thread"
        rows_per_block = 4 if C >= WAVE else 256
        for r in recs:
            assert (r["var"], r["N"], r["C"]) == (var, N, C), r
            assert r["blocks"] == -(-N // rows_per_block), r
        if N == 1025:
            assert recs[0]["blocks"] > 1  # more than one block of partials
    print(f"loss {loss} want {want_loss} "
          f"da {relerr(da, want_da) if np.any(want_da) else 0} "
          f"db {relerr(db, want_db) if np.any(want_db) else 0}")
    # the loss top is the unweighted loss; the weight scales the gradient
    assert abs(loss - want_loss) <= TOL * max(abs(want_loss), 1e-8)
    # only the one-row shape has nothing but a zero-gradient planted row
    assert np.any(want_da) == ((N, C) != (1, 1))
    # the exact-zero mdist row is in every case (one element cannot square
    # to 2.5 or 5 exactly: legacy at C = 1 plants a == b there)
    assert "dis_mdist0" in planted or (C == 1 and legacy and margin != 1.0)
    if np.any(want_da):
        assert relerr(da, want_da) <= TOL
        assert relerr(db, want_db) <= TOL
        random_rows = [planted[k] for k in ("sim_0.9", "sim_2")
                       if k in planted]
        for i in random_rows:  # non-zero over the whole width of the row
            assert np.count_nonzero(want_da[i]) == C
            assert relerr(da[i], want_da[i]) <= TOL
    else:
        assert not np.any(da) and not np.any(db)
    assert np.array_equal(db, -da)
    for name in ("dis_mdist0", "dis_equal0", "dis_equal", "sim_equal",
                 "dis_far", "dis_far100"):
        if name in planted:  # exactly zero, not merely small
            i = planted[name]
            assert np.all(np.isfinite(da[i])), name
            assert not np.any(da[i]) and not np.any(db[i]), name
    # two runs agree bit for bit
    loss2, da2, db2 = run(net, a, b, sim)
    assert loss2 == loss
    assert np.array_equal(da2, da) and np.array_equal(db2, db)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,C", [(5, 2), (9, 257)])
def test_contrastive_mdist_exactly_zero(mode, N, C):
    """a - b = (3, 4) at margin 5: d² = 25 and d = 5 are exact in float, so
    mdist is exactly 0 and the row's gradient must be exactly 0 — and its
    loss term 0."""
    ca.set_mode(mode)
    a, b, sim, _, _ = draw(N, C, 5.0, False, seed=3)
    sim[:] = 0
    delta = np.zeros(C, np.float32)
    delta[:2] = [3, 4]
    a[1] = 0
    b[1] = -delta
    want_loss, want_da, _ = replay64(a, b, sim, 5.0, False, 1.0)
    loss, da, db = run(build(N, C, 5.0), a, b, sim)
    assert not np.any(da[1]) and not np.any(db[1])
    assert abs(loss - want_loss) <= TOL * want_loss
    assert relerr(da, want_da) <= TOL


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("prop", [(True, False, False), (False, True, False),
                                  (True, True, True)])
def test_contrastive_prop_down_false_leaves_the_diff(mode, prop):
    """sim never propagates, also where propagate_down asks for it."""
    ca.set_mode(mode)
    N, C = 5, 2
    a, b, sim, _, _ = draw(N, C, 1.0, False, seed=4)
    _, want_da, want_db = replay64(a, b, sim, 1.0, False, 1.0)
    net = build(N, C, prop=prop)
    mark = np.full((N, C), 7.5, np.float32)
    net.set_blob("in0", mark, diff=True)
    net.set_blob("in1", mark, diff=True)
    net.set_blob("in2", mark[:, 0], diff=True)
    _, da, db = run(net, a, b, sim)
    assert np.array_equal(net.blob("in2", diff=True), mark[:, 0])
    if prop[0]:
        assert relerr(da, want_da) <= TOL
    else:
        assert np.array_equal(da, mark)
    if prop[1]:
        assert relerr(db, want_db) <= TOL
    else:
        assert np.array_equal(db, mark)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("similar", [1.0, 0.0])
@pytest.mark.parametrize("N,C", [(5, 2), (3, 257)])
def test_contrastive_nan_row(mode, N, C, similar):
    """A NaN in one row: the loss is NaN (also for a dissimilar row, where a
    max() that drops NaN operands would hide it), every other row's diff is
    what it was, and a similar row shows the NaN in its own diff."""
    ca.set_mode(mode)
    a, b, sim, _, _ = draw(N, C, 1.0, False, seed=5)
    net = build(N, C)
    _, da0, db0 = run(net, a, b, sim)
    a[2, 0] = np.nan
    sim[2] = similar
    loss, da, db = run(net, a, b, sim)
    assert np.isnan(loss)
    keep = [i for i in range(N) if i != 2]
    assert np.array_equal(da[keep], da0[keep])
    assert np.array_equal(db[keep], db0[keep])
    assert np.all(np.isfinite(da[keep]))
    if similar:
        assert np.isnan(da[2, 0]) and np.isnan(db[2, 0])


def test_contrastive_shape_errors():
    ca.set_mode("cpu")
    for shapes, needle in [
            ([(4, 2), (4, 3), (4,)], "same channels"),
            ([(4, 2, 2), (4, 2, 2), (4,)], "trailing dims 1"),
            ([(4, 2), (4, 2), (3,)], "one value per row"),
            ([(4, 2), (4, 2), (4, 2)], "one channel")]:
        with pytest.raises(ca.CaffeError) as e:
            net_from_text(input_net(shapes, layer(1.0, False, 1.0)))
        assert "'loss'" in str(e.value) and needle in str(e.value)


def test_contrastive_is_a_loss_layer_with_default_weight_one():
    ca.set_mode("cpu")
    body = ('layer { name: "loss" type: "ContrastiveLoss" bottom: "in0" '
            'bottom: "in1" bottom: "in2" top: "out" }')
    net = net_from_text(input_net([(4, 2), (4, 2), (4,)], body))
    a, b, sim, _, _ = draw(4, 2, 1.0, False, seed=6)
    loss, da, _ = run(net, a, b, sim)
    want_loss, want_da, _ = replay64(a, b, sim, 1.0, False, 1.0)
    assert net.loss() == pytest.approx(want_loss, rel=TOL)
    assert relerr(da, want_da) <= TOL


@pytest.mark.parametrize("legacy", [False, True])
def test_contrastive_finite_differences(legacy):
    """test_gradient_check.py's checker on (5, 2), rows kept away from the
    kinks (d = 0, d = margin) by more than ten steps."""
    ca.set_mode("cpu")
    N, C = 5, 2
    net = build_net(layer(1.0, legacy, 1.0), [(N, C), (N, C), (N,)])
    a = np.array([[.1, .2], [.5, -.4], [-.3, .3], [.6, .1], [0, .25]],
                 np.float32)
    b = np.array([[.4, -.1], [.1, -.1], [.2, .1], [.2, .6], [.3, -.2]],
                 np.float32)
    d = np.sqrt(((a - b) ** 2).sum(1))
    gap = 1.0 - (d * d if legacy else d)
    assert np.all(d > 0.2) and np.all(np.abs(gap) > 0.2), (d, gap)
    net.set_blob("in0", a)
    net.set_blob("in1", b)
    net.set_blob("in2", np.array([1, 0, 0, 1, 0], np.float32))
    check_gradients(net, "out", perturb_inputs=("in0", "in1"),
                    loss_top=True)
