"""Per-param lr_mult / decay_mult closed forms (reference layer param
specs, net.cpp params_lr/params_weight_decay): weight delta after one
momentum-free step must equal lr*lr_mult*(grad + decay*decay_mult*w);
lr_mult 0 freezes the blob.

Each test runs in CPU mode and, marked gpu, through the segmented fused
update kernel (k_sgd_seg: one launch per reducer bucket over the padded
param arena, per-segment multipliers found by binary search).
"""
import numpy as np
import pytest

import caffe_amd as ca
from oracle import oracle as orc

SOLVER = """base_lr: 0.1
lr_policy: "fixed"
momentum: 0.0
weight_decay: 0.01
random_seed: 2
net_param {
  name: "pm"
  layer {
    name: "input"
    type: "Input"
    top: "in0"
    top: "in1"
    input_param {
      shape { dim: 4 dim: 6 }
      shape { dim: 4 }
    }
  }
  layer {
    name: "ip"
    type: "InnerProduct"
    bottom: "in0"
    top: "fc"
    param { lr_mult: 2.0 decay_mult: 0.5 }
    param { lr_mult: 0.0 decay_mult: 0.0 }
    inner_product_param { num_output: 3
      weight_filler { type: "gaussian" std: 0.3 }
      bias_filler { type: "constant" value: 0.25 } }
  }
  layer {
    name: "loss"
    type: "SoftmaxWithLoss"
    bottom: "fc"
    bottom: "in1"
    top: "loss"
  }
}
"""


def _momentum_history_two_steps(mode):
    # h_t = m*h_{t-1} + lr*g_t ; w -= h_t  (sgd_solver.cpp:143-252):
    # with the SAME batch both steps (=> same loss surface point drifting),
    # replay the recurrence from captured per-step gradients
    ca.set_mode(mode)
    text = SOLVER.replace("momentum: 0.0", "momentum: 0.9").replace(
        "weight_decay: 0.01", "weight_decay: 0.0")
    rng = np.random.default_rng(6)
    x = rng.standard_normal((4, 6)).astype(np.float32)
    labels = np.array([2, 1, 0, 1], np.float32)

    # gradient probes: run a shadow solver to harvest g1 at w0 and g2 at w1
    solver = ca.Solver(text=text)
    net = solver.net
    net.set_blob("in0", x)
    net.set_blob("in1", labels)
    w0 = net.param(0).copy()
    net.forward()
    net.backward()
    g1 = net.param(0, diff=True).copy()
    solver.step(1)
    w1 = net.param(0).copy()
    net.forward()
    net.backward()
    g2 = net.param(0, diff=True).copy()
    solver.step(1)
    w2 = net.param(0).copy()

    lr_mult = 2.0  # SOLVER's ip weight param
    h1 = 0.1 * lr_mult * g1
    assert np.allclose(w1, w0 - h1, rtol=1e-5, atol=1e-6)
    h2 = 0.9 * h1 + 0.1 * lr_mult * g2
    assert np.allclose(w2, w1 - h2, rtol=1e-5, atol=1e-6), \
        np.abs(w2 - (w1 - h2)).max()


def test_momentum_history_two_steps():
    _momentum_history_two_steps("cpu")


@pytest.mark.gpu
def test_momentum_history_two_steps_gpu():
    # also the read-back path: w1 is read between two updates, and the read
    # of w2 must not be served from the host copy that read left behind
    _momentum_history_two_steps("gpu")


def _lr_and_decay_multipliers(mode):
    ca.set_mode(mode)
    solver = ca.Solver(text=SOLVER)
    net = solver.net
    rng = np.random.default_rng(4)
    x = rng.standard_normal((4, 6)).astype(np.float32)
    labels = np.array([0, 1, 2, 0], np.float32)
    net.set_blob("in0", x)
    net.set_blob("in1", labels)

    w0 = net.param(0).copy()
    b0 = net.param(1).copy()
    # raw gradient via hookless forward/backward on the same data
    net.forward()
    net.backward()
    g = net.param(0, diff=True).copy()

    # now the real step on the same data (backward overwrites diffs, so
    # the probe above does not perturb it)
    net.set_blob("in0", x)
    net.set_blob("in1", labels)
    solver.step(1)

    w1 = net.param(0)
    b1 = net.param(1)
    # expected: w -= base_lr*lr_mult * (g + weight_decay*decay_mult*w0)
    expect = w0 - 0.1 * 2.0 * (g + 0.01 * 0.5 * w0)
    assert np.allclose(w1, expect, rtol=1e-5, atol=1e-6), \
        np.abs(w1 - expect).max()
    # lr_mult 0: bias frozen exactly
    assert np.array_equal(b1, b0)


def test_lr_and_decay_multipliers():
    _lr_and_decay_multipliers("cpu")


@pytest.mark.gpu
def test_lr_and_decay_multipliers_gpu():
    _lr_and_decay_multipliers("gpu")


# Three layers, six params of 135 / 5 / 560 / 7 / 21 / 3 elements — none a
# multiple of the arena's 16-float padding, so every segment is followed by
# pad elements — each with its own multipliers; reduce_buckets 3 splits the
# arena into more than one update launch.
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


def _three_layer_replay(mode):
    ca.set_mode(mode)
    solver = ca.Solver(text=SOLVER3)
    net = solver.net
    rng = np.random.default_rng(12)
    x = rng.standard_normal((4, 3, 6, 6)).astype(np.float32)
    labels = np.array([2, 0, 1, 2], np.float32)
    net.set_blob("in0", x)
    net.set_blob("in1", labels)

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
    hist = [np.zeros(info[i][2], np.float32) for i in range(6)]
    arena = sum(-(-info[i][2] // ARENA_PAD) * ARENA_PAD for i in range(6))

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
        for i, (lr_mult, decay_mult) in enumerate(mults):
            assert np.abs(g[i]).max() > 0, (step, i)
            orc.sgd_update(g[i], w[i], hist[i], 0.9, 0.05 * lr_mult,
                           0.02 * decay_mult)
            got = net.param(i)
            worst = max(worst, float(np.abs(got - w[i]).max()
                                     / np.abs(w[i]).max()))
            assert np.allclose(got, w[i], rtol=1e-5, atol=1e-6), \
                (step, info[i], np.abs(got - w[i]).max())
        assert np.array_equal(net.param(frozen), start[frozen])
        if mode == "gpu":
            # one launch per bucket; together they tile the padded arena
            segs = [r for r in ca.kernel_trace_read() if r["op"] == "sgd_seg"]
            assert len(segs) > 1, segs
            assert segs[0]["lo"] == 0 and segs[-1]["hi"] == arena, segs
            for a, b in zip(segs, segs[1:]):
                assert a["hi"] == b["lo"], segs
            assert all(r["lo"] < r["hi"] and r["nseg"] == 6 for r in segs)
    print(f"relerr {{'w': '{worst:.2e}'}}")


def test_three_layer_multipliers_replay():
    _three_layer_replay("cpu")


@pytest.mark.gpu
def test_three_layer_multipliers_replay_gpu():
    _three_layer_replay("gpu")
