"""The fused join backward (Split + ReLU backward in one kernel) against the
two separate kernels, bit for bit.

Each net of tests/test_join_backward_plan.py with a planned join is built
twice in GPU mode with the same seed, once with CAFFE_JOIN_BWD=0 (read at
net build), fed the same inputs and top gradient, and run through one
forward / backward.  The add and the multiply are the same two fp32
operations in the same order, so every gradient must be array_equal.  The
one blob left out is the gradient of an out-of-place ReLU's top: the fused
kernel never writes it, and nothing reads it.
"""
import os

import numpy as np
import pytest

import caffe_amd as ca
from engine_util import net_from_text
from test_join_backward_plan import EXPECTED, join_net

pytestmark = pytest.mark.gpu

# count 90: the last float4 pack is half padding; count 128: whole packs
SHAPES = [(2, 5, 3, 3), (2, 4, 4, 4)]
CASES = [("sum_relu", None), ("sum_relu", 0.1), ("conv_relu_out", None),
         ("conv_relu_out", 0.1)]


def _inputs(shape):
    """The ReLU's input, chosen on the CPU: by position modulo 6 it is
    +0.0, -0.0, negative, positive, positive, negative, so a third of the
    elements are exact zeros of both signs, half are masked besides and a
    third are open."""
    n = int(np.prod(shape))
    rng = np.random.default_rng(5)
    mag = (rng.integers(1, 64, n) / 8.0).astype(np.float32)  # exact eighths
    kind = np.arange(n) % 6
    pre = np.where(np.isin(kind, (3, 4)), mag, -mag).astype(np.float32)
    pre[kind == 0] = 0.0
    pre[kind == 1] = -0.0
    return pre.reshape(shape), rng


def _run(kind, slope, shape, fused):
    pre, rng = _inputs(shape)
    # sum_relu: in0 + in1 == pre exactly (halves of eighths; -0.0 + -0.0 is
    # -0.0, x + -x is +0.0); conv_relu_out: c0 is the identity, in0 == pre
    half = (pre / 2).astype(np.float32)
    in0, in1 = (half, half) if kind == "sum_relu" else (pre, half)
    if kind == "sum_relu":
        in0 = in0.copy()
        in1 = in1.copy()
        z = (pre == 0) & ~np.signbit(pre)
        in0[z], in1[z] = 3.0, -3.0
    if fused:
        os.environ.pop("CAFFE_JOIN_BWD", None)
    else:
        os.environ["CAFFE_JOIN_BWD"] = "0"
    try:
        ca.set_mode("gpu")
        ca.set_random_seed(77)
        net = net_from_text(join_net(kind, shape, slope))
    finally:
        os.environ.pop("CAFFE_JOIN_BWD", None)
    assert net.join_backward() == EXPECTED[(kind, None)]
    c = shape[1]
    for i in range(net.num_params()):
        layer, blob, count = net.param_info(i)
        if layer == "c0":
            net.set_param(i, np.eye(c, dtype=np.float32).ravel() if blob == 0
                          else np.zeros(count, np.float32))
    net.set_blob("in0", in0)
    net.set_blob("in1", in1)
    net.forward()
    dg = rng.standard_normal(shape).astype(np.float32)
    net.set_blob("g", dg, diff=True)
    net.backward()
    ca.device_synchronize()
    relu_in, relu_out = ("e", "e") if kind == "sum_relu" else ("a", "f")
    grads = {"in0": net.blob("in0", diff=True), relu_in: net.blob(relu_in,
                                                                 diff=True)}
    if kind == "sum_relu":
        grads["in1"] = net.blob("in1", diff=True)
    for i in range(net.num_params()):
        layer, blob, _ = net.param_info(i)
        grads[f"{layer}.{blob}"] = net.param(i, diff=True)
    # both readers' gradients, as the join sums them
    tops = [net.blob(f"{relu_out}_split_{k}", diff=True) for k in (0, 1)]
    return pre, net.blob(relu_out), tops, grads


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind,slope", CASES)
def test_fused_join_matches_the_two_kernels(kind, slope, shape):
    pre, out, tops, unfused = _run(kind, slope, shape, fused=False)
    _, out_f, tops_f, fused = _run(kind, slope, shape, fused=True)
    open_ = pre > 0
    print(f"{kind} slope={slope} {shape}: open {open_.mean():.3f}, masked "
          f"{(~open_).mean():.3f}")
    assert open_.mean() >= 0.25 and (~open_).mean() >= 0.25
    # the ReLU's output holds exact zeros, of both signs where the plain
    # ReLU kernel wrote it (0 * negative is -0.0; the sum's fused epilogue
    # clamps with fmaxf instead)
    zeros = out[out == 0]
    assert zeros.size > 0
    if kind == "conv_relu_out" and not slope:
        assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()
    assert np.array_equal(out, out_f)
    # both readers hand down a non-zero gradient where the mask is open
    for a, b in zip(tops, tops_f):
        assert np.array_equal(a, b)
        assert np.all(a[open_] != 0)
    assert fused.keys() == unfused.keys()
    for name in unfused:
        assert np.array_equal(unfused[name], fused[name]), name
    # and the mask did something: the join's gradient is zero (slope 0) or
    # scaled (slope 0.1) exactly where it is closed
    relu_in = "e" if kind == "sum_relu" else "a"
    want = (tops[0] + tops[1]) * np.where(open_, np.float32(1),
                                          np.float32(slope or 0))
    assert np.array_equal(fused[relu_in], want.astype(np.float32))
