"""clip_gradients (caffe.proto:241-243; SGDSolver::ClipGradients,
sgd_solver.cpp:111-128), taken once per iteration over the whole reduced
gradient, in the order ApplyUpdate states: clip -> normalise by iter_size ->
regularise -> rule.

  sumsq  = sum of g^2 over every learnable param (owners; after the
           all-reduce), each square and the sum in double
  norm   = float32(sqrt(sumsq) / world)
  factor = clip / norm if norm > clip else 1       (float32)
  every rule sees g * (gscale * factor), gscale = 1 / (world * iter_size)

Float64 replays of the update against the engine, in CPU mode and (marked
gpu) through the kernels: k_grad_sumsq per bucket, k_clip_final, then the
deferred k_sgd_seg_clip / k_solver_seg_clip launches.  The replay pattern,
the net and the bound are those of test_solver_types.py.
"""
import numpy as np
import pytest

import caffe_amd as ca

F = np.float32

# The three-layer net of test_solver_types.py: six params of 135 / 5 / 560 /
# 7 / 21 / 3 elements, none a multiple of 4 or of the arena's 16-float
# padding, each with its own multipliers, one frozen; reduce_buckets 3 gives
# several buckets.
SOLVER3 = """base_lr: 0.05
lr_policy: "fixed"
momentum: 0.9
weight_decay: 0.02
reduce_buckets: 3
random_seed: 5
net_param {
  name: "pm3"
  layer {
    name: "input"
    type: "Input"
    top: "in0"
    top: "in1"
    input_param {
      shape { dim: 4 dim: 3 dim: 6 dim: 6 }
      shape { dim: 4 }
    }
  }
  layer {
    name: "conv"
    type: "Convolution"
    bottom: "in0"
    top: "conv"
    param { lr_mult: 1.0 decay_mult: 1.0 }
    param { lr_mult: 2.0 decay_mult: 0.0 }
    convolution_param { num_output: 5 kernel_size: 3
      weight_filler { type: "gaussian" std: 0.2 }
      bias_filler { type: "constant" value: 0.1 } }
  }
  layer {
    name: "ip1"
    type: "InnerProduct"
    bottom: "conv"
    top: "fc1"
    param { lr_mult: 0.5 decay_mult: 2.0 }
    param { lr_mult: 0.0 decay_mult: 0.0 }
    inner_product_param { num_output: 7
      weight_filler { type: "gaussian" std: 0.1 }
      bias_filler { type: "constant" value: 0.25 } }
  }
  layer {
    name: "ip2"
    type: "InnerProduct"
    bottom: "fc1"
    top: "fc2"
    param { lr_mult: 3.0 decay_mult: 0.5 }
    param { lr_mult: 1.0 decay_mult: 1.0 }
    inner_product_param { num_output: 3
      weight_filler { type: "gaussian" std: 0.3 }
      bias_filler { type: "constant" value: -0.1 } }
  }
  layer {
    name: "loss"
    type: "SoftmaxWithLoss"
    bottom: "fc2"
    bottom: "in1"
    top: "loss"
  }
}
"""
# (layer, blob) -> count, lr_mult, decay_mult
MULTS3 = {
    ("conv", 0): (135, 1.0, 1.0), ("conv", 1): (5, 2.0, 0.0),
    ("ip1", 0): (560, 0.5, 2.0), ("ip1", 1): (7, 0.0, 0.0),
    ("ip2", 0): (21, 3.0, 0.5), ("ip2", 1): (3, 1.0, 1.0),
}
ARENA_PAD = 16  # floats; params sit in the arena in net.params() order
BASE_LR, WEIGHT_DECAY = 0.05, 0.02
RTOL, ATOL = 1e-5, 1e-6  # the project's SGD-replay bound
# the engine sums exact double squares and rounds the norm once to float
NORM_RTOL = 1e-6

# type -> (momentum, extra solver lines, delta floor)
HYPER = {
    "SGD": (0.9, "", 0.0),
    "Nesterov": (0.9, "", 0.0),
    "AdaGrad": (0.0, "", 1e-3),
    "RMSProp": (0.0, "rms_decay: 0.95\n", 1e-4),
    "AdaDelta": (0.9, "", 1e-3),
    "Adam": (0.9, "momentum2: 0.999\n", 1e-4),
}
RMS_DECAY, MOMENTUM2, DELTA = 0.95, 0.999, 1e-8
TWO_SLOT = ("AdaDelta", "Adam")


def solver_text(kind="SGD", reg="L2", clip=None, extra=""):
    mom, lines, _ = HYPER[kind]
    head = f'type: "{kind}"\n{lines}{extra}'
    if clip is not None:
        head += f"clip_gradients: {float(clip)!r}\n"
    if reg != "L2":
        head += f'regularization_type: "{reg}"\n'
    return head + SOLVER3.replace("momentum: 0.9", f"momentum: {mom}")


def adam_correction(t):
    t = F(t)
    return np.sqrt(F(1) - np.power(F(MOMENTUM2), t)) / (
        F(1) - np.power(F(HYPER["Adam"][0]), t))


def replay(kind, reg, g, w, h, h2, lr_mult, decay_mult, c=None,
           base_lr=BASE_LR, weight_decay=WEIGHT_DECAY):
    """One float64 update of one param from the already scaled gradient g;
    hyper-parameters rounded to float32 first.  h, h2 are updated in place;
    returns the new weights."""
    mom = float(F(HYPER[kind][0]))
    d = float(max(F(DELTA), F(HYPER[kind][2])))
    lr = float(F(base_lr)) * float(F(lr_mult))
    decay = float(F(weight_decay)) * float(F(decay_mult))
    g = np.asarray(g, np.float64)
    w = w.astype(np.float64)
    gr = g + (w if reg == "L2" else np.sign(w)) * decay
    if kind == "SGD":
        h[:] = mom * h + lr * gr
        upd = h
    elif kind == "Nesterov":
        h0 = h.copy()
        h[:] = mom * h0 + lr * gr
        upd = (1 + mom) * h - mom * h0
    elif kind == "AdaGrad":
        h += gr * gr
        upd = lr * gr / (np.sqrt(h) + d)
    elif kind == "RMSProp":
        rho = float(F(RMS_DECAY))
        h[:] = rho * h + (1 - rho) * gr * gr
        upd = lr * gr / (np.sqrt(h) + d)
    elif kind == "AdaDelta":
        h[:] = mom * h + (1 - mom) * gr * gr
        u = gr * np.sqrt((h2 + d) / (h + d))
        h2[:] = mom * h2 + (1 - mom) * u * u
        upd = lr * u
    else:
        b2 = float(F(MOMENTUM2))
        h[:] = mom * h + (1 - mom) * gr
        h2[:] = b2 * h2 + (1 - b2) * gr * gr
        upd = lr * float(c) * h / (np.sqrt(h2) + d)
    return w - upd


def norm64(grads, world=1):
    """sqrt(sum g^2) / world in float64 over a list of gradients."""
    return np.sqrt(sum(np.sum(g.astype(np.float64) ** 2)
                       for g in grads)) / world


def factor32(norm, clip):
    """The formula in float32, written as the engine's comparison."""
    norm, clip = F(norm), F(clip)
    return clip / norm if norm > clip else F(1)


def make_solver(text):
    solver = ca.Solver(text=text)
    rng = np.random.default_rng(12)
    x = rng.standard_normal((4, 3, 6, 6)).astype(np.float32)
    labels = np.array([2, 0, 1, 2], np.float32)
    solver.net.set_blob("in0", x)
    solver.net.set_blob("in1", labels)
    return solver


def grads_of(net):
    net.forward()
    net.backward()
    return [net.param(i, diff=True).copy() for i in range(net.num_params())]


_NORM0 = {}


def norm_of_step0(mode):
    """||g|| of the first step of SOLVER3 (the same for every rule: the
    fillers and the inputs are seeded), measured with numpy once per mode."""
    if mode not in _NORM0:
        ca.set_mode(mode)
        _NORM0[mode] = float(norm64(grads_of(make_solver(SOLVER3).net)))
        assert _NORM0[mode] > 0
    return _NORM0[mode]


def state_of(solver):
    n = solver.net.num_params()
    out = [solver.net.param(i) for i in range(n)]
    for slot in range(solver.history_slots):
        out += [solver.history(i, slot) for i in range(n)]
    return out


def clip_records():
    return [r for r in ca.kernel_trace_read()
            if r["op"] in ("grad_sumsq", "clip_final", "sgd_seg",
                           "solver_seg")]


def traced_step(solver, iters=1):
    ca.kernel_trace(True)
    try:
        solver.step(iters)
    finally:
        ca.kernel_trace(False)
    return clip_records()


# ------------------------------------------------- 1: clipped replay, rules
def _clipped_replay(mode, kind, reg):
    clip = norm_of_step0(mode) / 2  # step 0 clips by construction
    ca.set_mode(mode)
    solver = make_solver(solver_text(kind, reg, clip=clip))
    net = solver.net
    assert solver.clip_gradients == F(clip)
    slots = 2 if kind in TWO_SLOT else 1
    info = net.params()
    mults = [MULTS3[info[i][:2]][1:] for i in range(6)]
    frozen = next(i for i in range(6) if info[i][:2] == ("ip1", 1))
    live = [i for i in range(6) if i != frozen]
    start = [net.param(i).copy() for i in range(6)]
    hist = [[np.zeros(info[i][2], np.float64) for i in range(6)]
            for _ in range(2)]

    worst = 0.0
    for step in range(3):
        w = [net.param(i).copy() for i in range(6)]
        g = grads_of(net)
        solver.step(1)
        factor = factor32(norm64(g), clip)
        if step == 0:
            assert factor < 1
            # unclipped: what the parent, ignoring the field, computes
            plain = [replay(kind, reg, g[i], w[i], hist[0][i].copy(),
                            hist[1][i].copy(), *mults[i],
                            adam_correction(1) if kind == "Adam" else None)
                     for i in live]
            assert not np.allclose(
                np.concatenate([net.param(i) for i in live]),
                np.concatenate(plain), rtol=RTOL, atol=ATOL)
        c = adam_correction(step + 1) if kind == "Adam" else None
        for i, (lr_mult, decay_mult) in enumerate(mults):
            assert np.abs(g[i]).max() > 0, (step, i)
            want = replay(kind, reg, g[i].astype(np.float64) * float(factor),
                          w[i], hist[0][i], hist[1][i], lr_mult, decay_mult,
                          c)
            got = net.param(i)
            worst = max(worst, float(np.abs(got - want).max()
                                     / np.abs(want).max()))
            assert np.allclose(got, want, rtol=RTOL, atol=ATOL), \
                (step, info[i], np.abs(got - want).max())
            for slot in range(slots):
                hgot = solver.history(i, slot)
                assert np.allclose(hgot, hist[slot][i], rtol=RTOL,
                                   atol=ATOL), \
                    (step, info[i], slot,
                     np.abs(hgot - hist[slot][i]).max())
            assert not net.param(i, diff=True).any(), (step, info[i])
        assert np.array_equal(net.param(frozen), start[frozen])
    print(f"relerr {{'w': '{worst:.2e}'}}")


CASES = [(k, "L2") for k in ("SGD", "Nesterov", "AdaGrad", "RMSProp",
                             "AdaDelta", "Adam")]
CASES += [("SGD", "L1"), ("Adam", "L1")]


@pytest.mark.parametrize("kind,reg", CASES)
def test_clipped_replay(kind, reg):
    _clipped_replay("cpu", kind, reg)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,reg", CASES)
def test_clipped_replay_gpu(kind, reg):
    _clipped_replay("gpu", kind, reg)


# ------------------------------------------------------ 2: norm and factor
def _norm_and_factor(mode):
    """-> the engine's norm of step 0, clipped at half the numpy norm."""
    clip = norm_of_step0(mode) / 2
    ca.set_mode(mode)
    solver = make_solver(solver_text(clip=clip))
    with pytest.raises(ca.CaffeError, match="no iteration"):
        solver.grad_norm()
    g = grads_of(solver.net)
    solver.step(1)
    norm, factor = solver.grad_norm()
    want = norm64(g)
    print(f"norm {norm!r} numpy {want!r} factor {factor!r}")
    assert np.isclose(norm, want, rtol=NORM_RTOL, atol=0)
    assert norm > F(clip) and factor == F(clip) / F(norm)
    # the frozen param (lr_mult 0) counts: without it the norm is another
    info = solver.net.params()
    frozen = next(i for i in range(6) if info[i][:2] == ("ip1", 1))
    without = norm64([g[i] for i in range(6) if i != frozen])
    assert not np.isclose(norm, without, rtol=100 * NORM_RTOL, atol=0)
    # within the bound: the norm is reported, the factor is 1
    loose = make_solver(solver_text(clip=2 * want))
    loose.step(1)
    norm2, factor2 = loose.grad_norm()
    assert np.isclose(norm2, want, rtol=NORM_RTOL, atol=0) and factor2 == 1
    return norm


def test_norm_and_factor():
    _norm_and_factor("cpu")


@pytest.mark.gpu
def test_norm_and_factor_gpu():
    gpu = _norm_and_factor("gpu")
    cpu = _norm_and_factor("cpu")
    print(f"norm cpu {cpu!r} gpu {gpu!r}")
    assert np.isclose(cpu, gpu, rtol=NORM_RTOL, atol=0)


def test_grad_norm_needs_the_field():
    ca.set_mode("cpu")
    solver = make_solver(SOLVER3)
    assert solver.clip_gradients == -1
    solver.step(1)
    with pytest.raises(ca.CaffeError, match="clip_gradients"):
        solver.grad_norm()


def test_pycaffe_and_display_line(tmp_path, capfd):
    import caffe_amd.pycaffe as pycaffe
    ca.set_mode("cpu")
    clip = norm_of_step0("cpu") / 2
    path = tmp_path / "clip.prototxt"
    path.write_text(solver_text(clip=clip, extra="display: 1\n"))
    solver = pycaffe.SGDSolver(str(path))
    rng = np.random.default_rng(12)
    solver.net.blobs["in0"].data[...] = rng.standard_normal((4, 3, 6, 6))
    solver.net.blobs["in1"].data[...] = [2, 0, 1, 2]
    assert solver.clip_gradients == F(clip)
    solver.step(1)
    norm, factor = solver.grad_norm()
    assert norm > F(clip) and factor == F(clip) / norm
    err = capfd.readouterr().err
    assert "Gradient clipping: scaling down gradients (L2 norm " in err
    assert f"> {F(clip):g}) by scale factor {factor:g}" in err


# ----------------------------------------- 3: not firing is not acting
def _not_firing(mode, kind):
    ca.set_mode(mode)
    probe = make_solver(solver_text(kind, clip=1e30))
    top = 0.0
    for _ in range(3):
        probe.step(1)
        top = max(top, float(probe.grad_norm()[0]))
    assert top > 0
    plain = make_solver(solver_text(kind))
    records = traced_step(plain, 3)  # no records in CPU mode
    clipped = make_solver(solver_text(kind, clip=2 * top))
    for _ in range(3):
        clipped.step(1)
        assert clipped.grad_norm()[1] == 1
    for a, b in zip(state_of(plain), state_of(clipped)):
        assert np.array_equal(a, b)
    if mode == "gpu":
        # without the field: the parent's records, nothing of the clip path
        assert len(records) > 3, records
        for r in records:
            if kind == "SGD":
                assert r["op"] == "sgd_seg", records
                assert set(r) == {"op", "lo", "hi", "nseg"}, records
            else:
                assert r["op"] == "solver_seg", records
                assert set(r) == {"op", "rule", "reg", "lo", "hi",
                                  "nseg"}, records


@pytest.mark.parametrize("kind", ["SGD", "Adam"])
def test_not_firing_is_not_acting(kind):
    _not_firing("cpu", kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["SGD", "Adam"])
def test_not_firing_is_not_acting_gpu(kind):
    _not_firing("gpu", kind)


# ------------------------------------------------------------- 4: edges
def _clip_zero(mode):
    # factor 0: the gradient is gone, decay and momentum stay
    ca.set_mode(mode)
    solver = make_solver(solver_text(clip=0))
    net = solver.net
    info = net.params()
    mults = [MULTS3[info[i][:2]][1:] for i in range(6)]
    hist = [np.zeros(info[i][2], np.float64) for i in range(6)]
    for step in range(2):
        w = [net.param(i).copy() for i in range(6)]
        solver.step(1)
        norm, factor = solver.grad_norm()
        assert norm > 0 and factor == 0
        for i in range(6):
            want = replay("SGD", "L2", np.zeros(info[i][2]), w[i], hist[i],
                          None, *mults[i])
            assert np.allclose(net.param(i), want, rtol=RTOL, atol=ATOL), \
                (step, info[i])
            assert not net.param(i, diff=True).any()
    # and it did move: decay alone
    assert np.abs(net.param(0) - w[0]).max() > 0


def test_clip_zero_is_decay_only():
    _clip_zero("cpu")


@pytest.mark.gpu
def test_clip_zero_is_decay_only_gpu():
    _clip_zero("gpu")


def test_nan_norm_does_not_clip():
    # The net without its loss layer: backward starts from the diff planted
    # in fc2, the blob the loss would read, so a NaN there reaches ip2's
    # gradients and, through them, the norm.  norm > clip is false for NaN.
    ca.set_mode("cpu")
    text = solver_text(clip=1e-3)
    cut = text.index('  layer {\n    name: "loss"')
    text = text[:cut] + "}\n"
    solver = make_solver(text)
    net = solver.net
    assert net.num_params() == 6
    seed = np.full((4, 3), 0.25, np.float32)
    net.set_blob("fc2", seed, diff=True)
    solver.step(1)
    norm, factor = solver.grad_norm()
    assert np.isfinite(norm) and norm > F(1e-3)
    assert factor == F(1e-3) / norm
    seed[1, 2] = np.nan
    net.set_blob("fc2", seed, diff=True)
    solver.step(1)
    norm, factor = solver.grad_norm()
    assert np.isnan(norm) and factor == 1


# ------------------------------------------------------- 5: iter_size 2
def _iter_size_two(mode):
    # The Input blobs hold one fixed batch: two sub-passes accumulate 2g,
    # norm 2||g||.  A clip of 1.5||g|| lies between the norm of the mean and
    # the norm of the sum, so the two readings give factors 1 and 0.75.
    ca.set_mode(mode)
    n0 = norm_of_step0(mode)
    clip = 1.5 * n0
    solver = make_solver(solver_text(clip=clip, extra="iter_size: 2\n"))
    net = solver.net
    info = net.params()
    mults = [MULTS3[info[i][:2]][1:] for i in range(6)]
    w = [net.param(i).copy() for i in range(6)]
    g = grads_of(net)
    solver.step(1)
    norm, factor = solver.grad_norm()
    assert np.isclose(norm, 2 * norm64(g), rtol=NORM_RTOL, atol=0)
    assert factor == F(clip) / norm and factor < 0.8
    got = np.concatenate([net.param(i) for i in range(6)])
    of_sum, of_mean = [], []
    for i in range(6):
        g2 = 2 * g[i].astype(np.float64)
        scale = float(F(0.5) * factor)  # clip, then 1 / iter_size
        of_sum.append(replay("SGD", "L2", g2 * scale, w[i],
                             np.zeros(info[i][2]), None, *mults[i]))
        mean_factor = float(factor32(norm64(g), clip))
        assert mean_factor == 1
        of_mean.append(replay("SGD", "L2", g2 * 0.5 * mean_factor, w[i],
                              np.zeros(info[i][2]), None, *mults[i]))
    assert np.allclose(got, np.concatenate(of_sum), rtol=RTOL, atol=ATOL)
    assert not np.allclose(got, np.concatenate(of_mean), rtol=RTOL,
                           atol=ATOL)


def test_iter_size_norm_is_of_the_sum():
    _iter_size_two("cpu")


@pytest.mark.gpu
def test_iter_size_norm_is_of_the_sum_gpu():
    _iter_size_two("gpu")


# ------------------------------------------- 6: world 2 in one process
@pytest.mark.parametrize("kind", ["SGD", "Adam"])
def test_world_two_equals_world_one(kind):
    # Two ranks with identical data: the callback doubles the buffer.  The
    # squares sum to 4x, the root to 2x and the division by world gives the
    # world-1 norm back, all exactly (powers of two); 2g * (factor / 2) is
    # g * factor exactly, so the update is the world-1 update bit for bit.
    ca.set_mode("cpu")
    clip = norm_of_step0("cpu") / 2
    one = make_solver(solver_text(kind, clip=clip))
    norms1 = []
    for _ in range(3):
        one.step(1)
        norms1.append(one.grad_norm())
    calls = []

    def double(buf):
        calls.append(buf.size)
        buf *= 2

    norms2 = []
    try:
        two = make_solver(solver_text(kind, clip=clip))
        two.set_allreduce_callback(double, world=2)
        for _ in range(3):
            two.step(1)
            norms2.append(two.grad_norm())
    finally:
        ca.set_rank_world(0, 1)
    assert calls
    assert norms1[0][1] < 1
    assert norms1 == norms2
    for a, b in zip(state_of(one), state_of(two)):
        assert np.array_equal(a, b)


# ------------------------------------------------------ 7: grid shape, GPU
def check_clip_records(records, arena, update_op):
    """One sum per bucket tiling [0, arena), one finalize over all their
    partials, then the updates, over the same ranges in the same order."""
    ops = [r["op"] for r in records]
    k = ops.index("clip_final")
    sums, final, updates = records[:k], records[k], records[k + 1:]
    assert ops.count("clip_final") == 1, ops
    assert sums and len(sums) == len(updates), ops
    assert all(r["op"] == "grad_sumsq" for r in sums), ops
    assert all(r["op"] == update_op and r["clip"] == 1 for r in updates), \
        records
    assert final["partials"] == sum(r["blocks"] for r in sums), records
    assert sums[0]["lo"] == 0 and sums[-1]["hi"] == arena, records
    for a, b in zip(sums, sums[1:]):
        assert a["hi"] == b["lo"], records
    assert [(r["lo"], r["hi"]) for r in sums] == \
        [(r["lo"], r["hi"]) for r in updates], records
    return sums


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["SGD", "Adam"])
def test_launch_order_gpu(kind):
    ca.set_mode("gpu")
    solver = make_solver(solver_text(kind, clip=norm_of_step0("gpu") / 2))
    info = solver.net.params()
    arena = sum(-(-info[i][2] // ARENA_PAD) * ARENA_PAD for i in range(6))
    for _ in range(2):
        records = traced_step(solver)
        sums = check_clip_records(
            records, arena, "sgd_seg" if kind == "SGD" else "solver_seg")
        assert len(sums) > 1, records


# One InnerProduct layer whose weight alone is past the block cap of the
# pack grid: 2048 blocks x 256 threads x 4 packs x 4 floats.
BIG_IN, BIG_OUT = 3000, 3072
PACK_CAP = 2048 * 256 * 4 * 4
BIG = f"""base_lr: 0.05
lr_policy: "fixed"
momentum: 0.9
weight_decay: 0.02
reduce_buckets: 1
random_seed: 5
net_param {{
  name: "big"
  layer {{ name: "input" type: "Input" top: "x" top: "t"
    input_param {{ shape {{ dim: 2 dim: {BIG_IN} }}
                  shape {{ dim: 2 dim: {BIG_OUT} }} }} }}
  layer {{ name: "ip" type: "InnerProduct" bottom: "x" top: "y"
    inner_product_param {{ num_output: {BIG_OUT}
      weight_filler {{ type: "uniform" min: -0.02 max: 0.02 }}
      bias_filler {{ type: "constant" value: 0.1 }} }} }}
  layer {{ name: "loss" type: "EuclideanLoss" bottom: "y" bottom: "t"
    top: "loss" }}
}}
"""


@pytest.mark.gpu
def test_one_bucket_past_the_block_cap_gpu():
    assert BIG_IN * BIG_OUT > PACK_CAP
    ca.set_mode("gpu")

    def build(text):
        solver = ca.Solver(text=text)
        rng = np.random.default_rng(3)
        solver.net.set_blob(
            "x", rng.standard_normal((2, BIG_IN)).astype(np.float32))
        solver.net.set_blob(
            "t", rng.standard_normal((2, BIG_OUT)).astype(np.float32))
        return solver

    probe = build(BIG)
    n0 = float(norm64(grads_of(probe.net)))
    clip = n0 / 2
    solver = build(f"clip_gradients: {clip!r}\n" + BIG)
    net = solver.net
    assert [net.param_info(i)[2] for i in range(2)] == \
        [BIG_IN * BIG_OUT, BIG_OUT]
    w = [net.param(i).copy() for i in range(2)]
    g = grads_of(net)
    records = traced_step(solver)
    sums = check_clip_records(records, BIG_IN * BIG_OUT + BIG_OUT, "sgd_seg")
    assert len(sums) == 1
    # capped grid: every thread makes more than its four uncapped passes
    assert sums[0]["blocks"] == 2048 and sums[0]["passes"] > 4, sums
    norm, factor = solver.grad_norm()
    want = norm64(g)
    print(f"norm {norm!r} numpy {want!r}")
    assert np.isclose(norm, want, rtol=NORM_RTOL, atol=0)
    assert factor == F(clip) / norm and factor < 1
    for i in range(2):
        new = replay("SGD", "L2", g[i].astype(np.float64) * float(factor),
                     w[i], np.zeros(g[i].size), None, 1.0, 1.0)
        assert np.allclose(net.param(i), new, rtol=RTOL, atol=ATOL), i
        assert not net.param(i, diff=True).any()


# --------------------------------------------------- 8: param sharing
# The two-tower net of test_param_sharing.py: both towers share all four
# params by name, so the net has four learnable params, the owners, whose
# gradients are the sums over both towers.
def tower(sfx, bottom, conv_params, ip_params):
    return f"""layer {{ name: "conv{sfx}" type: "Convolution" bottom: "{bottom}"
  top: "conv{sfx}" {conv_params}
  convolution_param {{ num_output: 2 kernel_size: 3
    weight_filler {{ type: "xavier" }} }} }}
layer {{ name: "pool{sfx}" type: "Pooling" bottom: "conv{sfx}" top: "pool{sfx}"
  pooling_param {{ pool: MAX kernel_size: 2 stride: 2 }} }}
layer {{ name: "ip{sfx}" type: "InnerProduct" bottom: "pool{sfx}"
  top: "ip{sfx}" {ip_params}
  inner_product_param {{ num_output: 3
    weight_filler {{ type: "xavier" }} }} }}
"""


def two_towers(conv_b='param { name: "cw" } param { name: "cb" }',
               ip_b='param { name: "iw" } param { name: "ib" }'):
    return ("""name: "towers"
layer { name: "input" type: "Input" top: "pair"
  input_param { shape { dim: 2 dim: 2 dim: 8 dim: 8 } } }
layer { name: "sl" type: "Slice" bottom: "pair" top: "d" top: "d_p"
  slice_param { slice_dim: 1 slice_point: 1 } }
""" + tower("", "d", 'param { name: "cw" } param { name: "cb" }',
            'param { name: "iw" } param { name: "ib" }')
        + tower("_p", "d_p", conv_b, ip_b) +
        """layer { name: "loss" type: "EuclideanLoss" bottom: "ip"
  bottom: "ip_p" top: "loss" }
""")


def _shared_params(mode):
    ca.set_mode(mode)

    def build(head):
        solver = ca.Solver(text=head + f"""base_lr: 0.05
lr_policy: "fixed"
momentum: 0.9
weight_decay: 0.02
reduce_buckets: 2
random_seed: 5
net_param {{
{two_towers()}}}
""")
        rng = np.random.default_rng(4)
        solver.net.set_blob(
            "pair", rng.standard_normal((2, 2, 8, 8)).astype(np.float32))
        return solver

    probe = build("")
    assert probe.net.num_params() == 4 and len(probe.net.param_sharing()) == 4
    clip = float(norm64(grads_of(probe.net))) / 2
    solver = build(f"clip_gradients: {clip!r}\n")
    net = solver.net
    w = [net.param(i).copy() for i in range(4)]
    g = grads_of(net)  # the owners' diffs: already the sums
    solver.step(1)
    norm, factor = solver.grad_norm()
    assert np.isclose(norm, norm64(g), rtol=NORM_RTOL, atol=0)
    assert factor == F(clip) / norm and factor < 1
    # (the shared ip bias takes +dy from one tower and -dy from the other:
    # its summed gradient is zero, so the weights carry the comparison)
    plain = []
    for i in range(4):
        want = replay("SGD", "L2", g[i].astype(np.float64) * float(factor),
                      w[i], np.zeros(g[i].size), None, 1.0, 1.0)
        assert np.allclose(net.param(i), want, rtol=RTOL, atol=ATOL), i
        plain.append(replay("SGD", "L2", g[i], w[i], np.zeros(g[i].size),
                            None, 1.0, 1.0))
        assert not net.param(i, diff=True).any()
    assert not np.allclose(np.concatenate([net.param(i) for i in range(4)]),
                           np.concatenate(plain), rtol=RTOL, atol=ATOL)


def test_shared_params():
    _shared_params("cpu")


@pytest.mark.gpu
def test_shared_params_gpu():
    _shared_params("gpu")
