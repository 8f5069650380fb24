"""PReLU against float64 torch.nn.functional.prelu with autograd against a
random top gradient: y, dx and the slope gradient da.  In GPU mode the layer
runs kernels/prelu.hip; the trace record pins the layout (v4 | scalar | cols)
and the work split each row reaches.  x is N(0, 1) with a few exact zeros
(dx = a * dy there, nothing added to da); one slope is 0 and one negative, so
an in-place backward that tried to recover x from y would fail; dx starts as
NaN wherever it is not the top gradient's own memory.
"""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import caffe_amd as ca
from engine_util import TOL, input_net, net_from_text, relerr

# prelu.hip's plan: the grid the slices aim at, the most loads in one piece
# of a plane, the column packs of a cols block, the fewest rows of a cols
# slice
BLOCKS, CHUNK, COLS, MIN_ROWS = 2048, 1024, 64, 32

# id: (shape, layout, row slices, channel_shared, in-place)
ROWS = {
    "v4": ((2, 3, 4, 4), "v4", 2, False, False),
    "scalar": ((2, 3, 3, 5), "scalar", 2, False, False),
    "scalar_s2": ((3, 5, 1, 2), "scalar", 3, False, False),
    "scalar_3axis": ((2, 3, 5), "scalar", 2, False, False),
    "cols": ((4, 7), "cols", 1, False, False),
    "cols_vec": ((5, 8), "cols", 1, False, False),
    # two column blocks, the second of 3 columns; row slices of 19 and 18
    "cols_wide": ((MIN_ROWS + 5, COLS + 3), "cols", 2, False, False),
    # C so large that a channel gets two slices: 3 images and 2
    "v4_slices": ((5, BLOCKS // 2, 2, 2), "v4", 2, False, False),
    "scalar_slices": ((5, BLOCKS // 2, 1, 3), "scalar", 2, False, False),
    # a plane of CHUNK + 3 loads is two pieces of 514 and 513
    "v4_long": ((1, 2, CHUNK + 3, 4), "v4", 2, False, False),
    "scalar_long": ((1, 2, 13, (CHUNK + 3) // 13), "scalar", 2, False, False),
    "v4_shared": ((2, 3, 4, 4), "v4", 2, True, False),
    "cols_shared": ((4, 7), "cols", 1, True, False),
    "v4_inplace": ((2, 3, 4, 4), "v4", 2, False, True),
    "scalar_inplace": ((2, 3, 3, 5), "scalar", 2, False, True),
    "cols_inplace": ((4, 7), "cols", 1, False, True),
}
MODES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture(autouse=True)
def cpu_after():
    yield
    ca.kernel_trace(False)
    ca.set_mode("cpu")


def layer(param="", top="out"):
    return (f'layer {{ name: "act" type: "PReLU" bottom: "in0" top: "{top}" '
            f'prelu_param {{ {param} }} }}')


def inputs(name):
    shape, shared = ROWS[name][0], ROWS[name][3]
    r = np.random.default_rng(sorted(ROWS).index(name))
    x = r.standard_normal(shape).astype(np.float32)
    x.ravel()[r.choice(x.size, 5, replace=False)] = 0.0
    a = r.uniform(-0.5, 1.5, 1 if shared else shape[1]).astype(np.float32)
    a[0], a[-1] = 0.0, -0.3
    return x, r.standard_normal(shape).astype(np.float32), a


def reference(x, dy, a):
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    at = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    y = F.prelu(xt, at)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    return y.detach().numpy(), xt.grad.numpy(), at.grad.numpy()


def run(mode, x, dy, a, shared=False, inplace=False, text=None):
    ca.set_mode(mode)
    top = "in0" if inplace else "out"
    net = net_from_text(text or input_net(
        [x.shape], layer(f"channel_shared: {str(shared).lower()}", top)))
    net.set_param(0, a)
    net.set_blob("in0", x)
    net.forward()
    y = net.blob(top)
    if not inplace:
        net.set_blob("in0", np.full(x.shape, np.nan, np.float32), diff=True)
    net.set_blob(top, dy, diff=True)
    net.backward()
    return y, net.blob("in0", diff=True), net.param(0, diff=True)


def planned(shape):
    """The record fields the plan of prelu.hip gives this shape."""
    N, C, S = shape[0], shape[1], int(np.prod(shape[2:]))
    if S == 1:
        var, vec = "cols", 4 if C % 4 == 0 else 1
        rows, cb = N, -(-(C // vec) // COLS)
        want = min(max(1, BLOCKS // cb), -(-N // MIN_ROWS))
    else:
        var, vec = ("v4", 4) if S % 4 == 0 else ("scalar", 1)
        rows, cb, want = N * -(-(S // vec) // CHUNK), C, max(1, BLOCKS // C)
    rps = -(-rows // min(want, rows))
    return dict(var=var, vec=vec, slices=-(-rows // rps),
                blocks=cb * -(-rows // rps))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(ROWS))
def test_parity(mode, name):
    shape, var, slices, shared, inplace = ROWS[name]
    plan = planned(shape)
    assert (plan["var"], plan["slices"]) == (var, slices)
    x, dy, a = inputs(name)
    y_ref, dx_ref, da_ref = reference(x, dy, a)
    ca.kernel_trace(True)
    y, dx, da = run(mode, x, dy, a, shared, inplace)
    ca.kernel_trace(False)
    print(name, mode, "y err", relerr(y, y_ref), "dx err", relerr(dx, dx_ref),
          "da err", relerr(da, da_ref))
    assert relerr(y, y_ref) < TOL
    assert relerr(dx, dx_ref) < TOL
    assert relerr(da, da_ref) < TOL
    recs = [r for r in ca.kernel_trace_read() if r["op"].startswith("prelu")]
    if mode == "cpu":
        assert recs == []
        return
    assert recs == [dict(op="prelu_fwd", **plan, inplace=int(inplace)),
                    dict(op="prelu_bwd", **plan, dx=1)]


@pytest.mark.parametrize("mode", MODES)
def test_frozen_bottom_still_gets_slope_gradient(mode):
    x, dy, a = inputs("scalar")
    text = input_net([x.shape], layer()).replace("force_backward: true", "")
    ca.kernel_trace(True)
    _, dx, da = run(mode, x, dy, a, text=text)
    ca.kernel_trace(False)
    assert relerr(da, reference(x, dy, a)[2]) < TOL
    assert np.isnan(dx).all()
    if mode == "gpu":
        assert ca.kernel_trace_read()[-1] == dict(
            op="prelu_bwd", **planned(x.shape), dx=0)


@pytest.mark.gpu
def test_rerun_is_bit_identical():
    x, dy, a = inputs("v4_slices")
    first = run("gpu", x, dy, a)
    again = run("gpu", x, dy, a)
    assert all(np.array_equal(p, q) for p, q in zip(first, again))


@pytest.mark.parametrize("param,count,value", [
    ("", 3, 0.25),
    ('filler { type: "constant" value: 0.1 }', 3, 0.1),
    ("channel_shared: true", 1, 0.25),
])
def test_fillers(param, count, value):
    ca.set_mode("cpu")
    net = net_from_text(input_net([(2, 3, 4, 4)], layer(param)))
    assert net.param_info(0) == ("act", 0, count)
    assert np.array_equal(net.param(0), np.full(count, value, np.float32))


def test_construction_errors():
    ca.set_mode("cpu")
    with pytest.raises(ca.CaffeError, match="PReLU layer 'act'.*2 axes"):
        net_from_text(input_net([(5,)], layer()))
    path = os.path.join(tempfile.mkdtemp(), "three.caffemodel")
    net_from_text(input_net([(2, 3, 4, 4)], layer())).save_weights(path)
    with pytest.raises(ca.CaffeError, match="Negative slope size is "
                       "inconsistent with prototxt config"):
        net_from_text(input_net([(2, 5, 4, 4)], layer())).load_weights(path)


TRAIN_NET = """
layer { name: "in" type: "Input" top: "data" top: "target"
  input_param { shape { dim: 2 dim: 1 dim: 8 dim: 8 }
                shape { dim: 2 dim: 1 dim: 16 dim: 16 } } }
layer { name: "conv" type: "Convolution" bottom: "data" top: "c"
  convolution_param { num_output: 4 kernel_size: 3 pad: 1
    weight_filler { type: "gaussian" std: 0.5 } } }
layer { name: "act" type: "PReLU" bottom: "c" top: "c" }
layer { name: "up" type: "Deconvolution" bottom: "c" top: "u"
  convolution_param { num_output: 1 kernel_size: 4 stride: 2 pad: 1
    weight_filler { type: "gaussian" std: 0.5 } } }
layer { name: "loss" type: "EuclideanLoss" bottom: "u" bottom: "target"
  top: "l" }
"""


def trained(mode):
    ca.set_mode(mode)
    solver = ca.Solver(text='base_lr: 0.05\nlr_policy: "fixed"\nmomentum: 0.9'
                       "\nrandom_seed: 7\nnet_param {" + TRAIN_NET + "}\n")
    r = np.random.default_rng(3)
    solver.net.set_blob("data", r.standard_normal((2, 1, 8, 8)))
    solver.net.set_blob("target", r.standard_normal((2, 1, 16, 16)))
    solver.step(1)
    return solver.net


def test_slopes_round_trip_through_caffemodel():
    cpu = trained("cpu")
    act = [cpu.param_info(i)[0] for i in range(cpu.num_params())].index("act")
    assert np.all(cpu.param(act) != 0.25)  # the step moved every slope
    path = os.path.join(tempfile.mkdtemp(), "net.caffemodel")
    cpu.save_weights(path)
    other = net_from_text('name: "t"' + TRAIN_NET)
    other.load_weights(path)
    assert np.array_equal(other.param(act), cpu.param(act))


@pytest.mark.gpu
def test_training_step_matches_across_modes():
    cpu, gpu = trained("cpu"), trained("gpu")
    assert cpu.num_params() == 5  # conv w, b; slopes; deconv w, b
    for i in range(cpu.num_params()):
        assert relerr(gpu.param(i), cpu.param(i)) < TOL, cpu.param_info(i)
