"""The six solver types (reference solvers/*_solver.{cpp,cu}): SGD, Nesterov,
AdaGrad, RMSProp, AdaDelta, Adam, each with L2 or L1 regularisation.

Per-element float64 replay of every update rule against the engine, in CPU
mode and (marked gpu) through the segmented fused kernel k_solver_seg; world
scaling, snapshot/resume, construction-time validation and the pycaffe
solver classes.  With g the reduced gradient times 1/(world*iter_size),
lr = cur_lr*lr_mult, decay = weight_decay*decay_mult, reg = w (L2) or
sign(w) (L1), every rule starts with gr = g + reg*decay and ends w -= update:

  SGD       h = mom*h + lr*gr;                update = h
  Nesterov  h' = mom*h + lr*gr;               update = (1+mom)*h' - mom*h
  AdaGrad   h += gr^2;                        update = lr*gr/(sqrt(h)+d)
  RMSProp   h = rho*h + (1-rho)*gr^2;         update = lr*gr/(sqrt(h)+d)
  AdaDelta  h = mom*h + (1-mom)*gr^2; u = gr*sqrt((h2+d)/(h+d));
            h2 = mom*h2 + (1-mom)*u^2;        update = lr*u
  Adam      m = b1*m + (1-b1)*gr; v = b2*v + (1-b2)*gr^2;
            update = lr*c*m/(sqrt(v)+d),  c = sqrt(1-b2^t)/(1-b1^t), t=iter+1

with d = max(delta, floor): floor 1e-3 for AdaGrad and AdaDelta, 1e-4 for
RMSProp and Adam.
"""
import numpy as np
import pytest

import caffe_amd as ca
import caffe_amd.pycaffe as pycaffe

F = np.float32

# Three layers, six params of 135 / 5 / 560 / 7 / 21 / 3 elements — none a
# multiple of 4 or of the arena's 16-float padding, so every segment ends in
# a partial float4 pack followed by pad — each with its own multipliers, one
# frozen; reduce_buckets 3 splits the arena into more than one update launch.
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


def solver_text(kind, reg="L2", extra=""):
    mom, lines, _ = HYPER[kind]
    head = f'type: "{kind}"\n{lines}{extra}'
    if reg != "L2":
        head += f'regularization_type: "{reg}"\n'
    return head + SOLVER3.replace("momentum: 0.9", f"momentum: {mom}")


def adam_correction(t):
    """c = sqrt(1 - b2^t) / (1 - b1^t) in float32, as the engine computes it
    on the host once per iteration."""
    t = F(t)
    return np.sqrt(F(1) - np.power(F(MOMENTUM2), t)) / (
        F(1) - np.power(F(HYPER["Adam"][0]), t))


def replay(kind, reg, g, w, h, h2, lr_mult, decay_mult, c=None):
    """One float64 update of one param; hyper-parameters rounded to float32
    first.  h, h2 are updated in place; returns the new weights."""
    mom = float(F(HYPER[kind][0]))
    d = float(max(F(DELTA), F(HYPER[kind][2])))
    lr = float(F(BASE_LR)) * float(F(lr_mult))
    decay = float(F(WEIGHT_DECAY)) * float(F(decay_mult))
    g = g.astype(np.float64)
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


def make_solver(text):
    solver = ca.Solver(text=text)
    rng = np.random.default_rng(12)
    x = rng.standard_normal((4, 3, 6, 6)).astype(np.float32)
    labels = np.array([2, 0, 1, 2], np.float32)
    solver.net.set_blob("in0", x)
    solver.net.set_blob("in1", labels)
    return solver


def update_launches():
    return [r for r in ca.kernel_trace_read()
            if r["op"] in ("sgd_seg", "solver_seg")]


def _replay_case(mode, kind, reg):
    ca.set_mode(mode)
    solver = make_solver(solver_text(kind, reg))
    net = solver.net
    slots = 2 if kind in TWO_SLOT else 1
    assert solver.type == kind
    assert solver.history_slots == slots

    info = net.params()
    assert len(info) == 6
    mults = []
    for i in range(6):
        layer, blob, count = info[i]
        want_count, lr_mult, decay_mult = MULTS3[(layer, blob)]
        assert count == want_count
        mults.append((lr_mult, decay_mult))
    frozen = next(i for i in range(6) if info[i][:2] == ("ip1", 1))
    start = [net.param(i).copy() for i in range(6)]
    hist = [[np.zeros(info[i][2], np.float64) for i in range(6)]
            for _ in range(2)]
    arena = sum(-(-info[i][2] // ARENA_PAD) * ARENA_PAD for i in range(6))
    for slot in range(slots):
        for i in range(6):
            assert not solver.history(i, slot).any()

    worst = 0.0
    for step in range(3):
        w = [net.param(i).copy() for i in range(6)]
        net.forward()
        net.backward()
        g = [net.param(i, diff=True).copy() for i in range(6)]
        if mode == "gpu":
            ca.kernel_trace(True)
        try:
            solver.step(1)
        finally:
            ca.kernel_trace(False)
        c = adam_correction(step + 1) if kind == "Adam" else None
        for i, (lr_mult, decay_mult) in enumerate(mults):
            assert np.abs(g[i]).max() > 0, (step, i)
            if kind == "Adam" and step == 1 and i != frozen:
                # a stale iteration count (c frozen at t = 1) must not pass
                stale = replay(kind, reg, g[i], w[i], hist[0][i].copy(),
                               hist[1][i].copy(), lr_mult, decay_mult,
                               adam_correction(1))
                assert not np.allclose(net.param(i), stale, rtol=RTOL,
                                       atol=ATOL), (step, info[i])
            want = replay(kind, reg, g[i], w[i], hist[0][i], hist[1][i],
                          lr_mult, decay_mult, c)
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
                if slot == 1 and step >= 1:
                    assert np.abs(hgot).max() > 0, (step, info[i])
            assert not net.param(i, diff=True).any(), (step, info[i])
        assert np.array_equal(net.param(frozen), start[frozen])
        if mode == "gpu":
            # one launch per bucket; together they tile the padded arena
            segs = update_launches()
            assert len(segs) > 1, segs
            for r in segs:
                assert r["op"] == "solver_seg", segs
                assert r["rule"] == kind.lower() and r["reg"] == reg, segs
                assert r["lo"] < r["hi"] and r["nseg"] == 6, segs
            assert segs[0]["lo"] == 0 and segs[-1]["hi"] == arena, segs
            for a, b in zip(segs, segs[1:]):
                assert a["hi"] == b["lo"], segs
    print(f"relerr {{'w': '{worst:.2e}'}}")


# the five new rules and SGD with L1 (the issue's cases), plus L1 for the
# five: each (rule, reg) pair is its own kernel instantiation
CASES = [(k, "L2") for k in ("Nesterov", "AdaGrad", "RMSProp", "AdaDelta",
                             "Adam")]
CASES += [(k, "L1") for k in ("SGD", "Nesterov", "AdaGrad", "RMSProp",
                              "AdaDelta", "Adam")]


@pytest.mark.parametrize("kind,reg", CASES)
def test_rule_replay(kind, reg):
    _replay_case("cpu", kind, reg)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,reg", CASES)
def test_rule_replay_gpu(kind, reg):
    _replay_case("gpu", kind, reg)


@pytest.mark.gpu
def test_sgd_l2_keeps_its_kernel_gpu():
    # type "SGD" (given or absent) with L2 stays on k_sgd_seg
    ca.set_mode("gpu")
    for text in (solver_text("SGD"), SOLVER3):
        solver = make_solver(text)
        assert solver.type == "SGD" and solver.history_slots == 1
        ca.kernel_trace(True)
        try:
            solver.step(2)
        finally:
            ca.kernel_trace(False)
        segs = update_launches()
        assert len(segs) > 2, segs
        assert all(r["op"] == "sgd_seg" for r in segs), segs


def _state(solver):
    out = [solver.net.param(i) for i in range(6)]
    for slot in range(solver.history_slots):
        out += [solver.history(i, slot) for i in range(6)]
    return out


@pytest.mark.parametrize("kind", TWO_SLOT)
def test_world_scaling_is_exact(kind):
    # two identical ranks: the callback doubles the buffer and the engine
    # scales by 1/world.  2g * 0.5 == g exactly, so weights and histories
    # are bit-equal to a world-1 run — provided the scale is applied to g
    # before any square is taken.  (The callback comm hands the callback a
    # host pointer, so this is a CPU-mode test.)
    ca.set_mode("cpu")
    one = make_solver(solver_text(kind))
    one.step(3)
    calls = []

    def double(buf):
        calls.append(buf.size)
        buf *= 2

    try:
        two = make_solver(solver_text(kind))
        two.set_allreduce_callback(double, world=2)
        two.step(3)
    finally:
        ca.set_rank_world(0, 1)
    assert calls
    for a, b in zip(_state(one), _state(two)):
        assert np.abs(a).max() > 0
        assert np.array_equal(a, b)


def _iter_size_exact(mode, kind):
    # the Input blobs hold one fixed batch, so two accumulated sub-passes
    # give 2g and the 1/iter_size scale gives g back exactly: bit-equal to
    # iter_size 1 if the scale reaches g before the rule squares it
    ca.set_mode(mode)
    one = make_solver(solver_text(kind))
    one.step(3)
    two = make_solver(solver_text(kind, extra="iter_size: 2\n"))
    two.step(3)
    for a, b in zip(_state(one), _state(two)):
        assert np.abs(a).max() > 0
        assert np.array_equal(a, b)


@pytest.mark.parametrize("kind", TWO_SLOT)
def test_iter_size_scaling_is_exact(kind):
    _iter_size_exact("cpu", kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", TWO_SLOT)
def test_iter_size_scaling_is_exact_gpu(kind):
    _iter_size_exact("gpu", kind)


def _varint(buf, pos):
    v = shift = 0
    while True:
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return v, pos


def _fields(buf):
    """(field number, wire type, value) of one protobuf message: value is
    the int of a varint or the bytes of a length-delimited field."""
    pos = 0
    while pos < len(buf):
        key, pos = _varint(buf, pos)
        num, wt = key >> 3, key & 7
        if wt == 0:
            val, pos = _varint(buf, pos)
        elif wt == 2:
            n, pos = _varint(buf, pos)
            val, pos = buf[pos:pos + n], pos + n
        elif wt == 5:
            val, pos = buf[pos:pos + 4], pos + 4
        elif wt == 1:
            val, pos = buf[pos:pos + 8], pos + 8
        else:
            raise AssertionError(f"wire type {wt}")
        yield num, wt, val


def _history_blobs(state_path):
    """The float data (BlobProto field 5, packed) of every SolverState
    history blob (field 3), in file order."""
    blobs = []
    for num, wt, val in _fields(open(state_path, "rb").read()):
        if num == 3 and wt == 2:
            data = [v for n, t, v in _fields(val) if n == 5 and t == 2]
            assert len(data) == 1
            blobs.append(np.frombuffer(data[0], np.float32))
    return blobs


def _forward_order(net):
    info = net.params()
    layers = ["conv", "ip1", "ip2"]
    return sorted(range(6),
                  key=lambda i: (layers.index(info[i][0]), info[i][1]))


def _snapshot(solver):
    ca._ck(ca._lib.caffe_solver_snapshot(solver._h))


def _restore(solver, state):
    ca._ck(ca._lib.caffe_solver_restore(solver._h, str(state).encode()))


def _snapshot_resume(mode, kind, tmp_path):
    ca.set_mode(mode)
    prefix = f'snapshot_prefix: "{tmp_path}/{kind}"\n'
    solver = make_solver(solver_text(kind, extra=prefix))
    solver.step(3)
    _snapshot(solver)
    slot0 = [solver.history(i, 0) for i in range(6)]
    slot1 = [solver.history(i, 1) for i in range(6)]
    solver.step(2)
    a = _state(solver)

    state = tmp_path / f"{kind}_iter_3.solverstate"
    blobs = _history_blobs(state)
    assert len(blobs) == 2 * 6
    order = _forward_order(solver.net)
    for k, i in enumerate(order):
        assert np.array_equal(blobs[k], slot0[i]), (k, i)
        assert np.array_equal(blobs[6 + k], slot1[i]), (k, i)

    fresh = make_solver(solver_text(kind, extra=prefix))
    _restore(fresh, state)
    assert fresh.iter == 3
    fresh.step(2)
    for x, y in zip(a, _state(fresh)):
        assert np.array_equal(x, y)

    # an SGD state holds 6 history blobs: not an Adam / AdaDelta state
    sgd = make_solver(f'snapshot_prefix: "{tmp_path}/sgd"\n' + SOLVER3)
    sgd.step(1)
    _snapshot(sgd)
    sgd_state = tmp_path / "sgd_iter_1.solverstate"
    assert len(_history_blobs(sgd_state)) == 6
    other = make_solver(solver_text(kind, extra=prefix))
    before = _state(other)
    with pytest.raises(ca.CaffeError, match="Incorrect length of history"):
        _restore(other, sgd_state)
    for x, y in zip(before, _state(other)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kind", TWO_SLOT)
def test_snapshot_resume(kind, tmp_path):
    _snapshot_resume("cpu", kind, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", TWO_SLOT)
def test_snapshot_resume_gpu(kind, tmp_path):
    _snapshot_resume("gpu", kind, tmp_path)


@pytest.mark.parametrize("head,keys", [
    ('type: "Adamax"\n', ["type", "Adamax"]),
    ('type: "AdaGrad"\n', ["AdaGrad", "momentum", "0.9"]),
    ('type: "RMSProp"\n', ["RMSProp", "momentum", "0.9"]),
    ('type: "RMSProp"\nrms_decay: 1.0\n', ["rms_decay", "1.0"]),
    ('regularization_type: "L3"\n', ["regularization_type", "L3"]),
    ('type: "Adam"\nsolver_type: ADAM\n', ["type", "solver_type"]),
])
def test_validation_errors(head, keys):
    ca.set_mode("cpu")
    text = head + SOLVER3
    if "rms_decay" in head:
        text = text.replace("momentum: 0.9", "momentum: 0.0")
    with pytest.raises(ca.CaffeError) as err:
        ca.Solver(text=text)
    for key in keys:
        assert key in str(err.value), (key, str(err.value))


def test_deprecated_solver_type_enum():
    ca.set_mode("cpu")
    solver = ca.Solver(text="solver_type: ADAM\n" + SOLVER3)
    assert solver.type == "Adam" and solver.history_slots == 2
    assert ca.Solver(text=SOLVER3).type == "SGD"


def test_pycaffe_solver_classes(tmp_path):
    ca.set_mode("cpu")
    adam = tmp_path / "adam.prototxt"
    adam.write_text(solver_text("Adam"))
    adadelta = tmp_path / "adadelta.prototxt"
    adadelta.write_text(solver_text("AdaDelta"))
    sgd = tmp_path / "sgd.prototxt"
    sgd.write_text(SOLVER3)  # no type given

    assert type(pycaffe.get_solver(str(adam))) is pycaffe.AdamSolver
    assert type(pycaffe.get_solver(str(sgd))) is pycaffe.SGDSolver
    pycaffe.SGDSolver(str(sgd))
    with pytest.raises(ca.CaffeError) as err:
        pycaffe.AdamSolver(str(sgd))
    assert "Adam" in str(err.value) and "SGD" in str(err.value)
    with pytest.raises(ca.CaffeError):
        pycaffe.SGDSolver(str(adam))

    solver = pycaffe.AdaDeltaSolver(str(adadelta))
    rng = np.random.default_rng(12)
    solver.net.blobs["in0"].data[...] = rng.standard_normal((4, 3, 6, 6))
    solver.net.blobs["in1"].data[...] = [2, 0, 1, 2]
    w0 = solver.net.params["conv"][0].data.copy()
    solver.step(2)
    assert solver.iter == 2
    assert np.abs(solver.net.params["conv"][0].data - w0).max() > 0
