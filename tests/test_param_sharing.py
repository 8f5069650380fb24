"""Shared params (reference Net::AppendParam, net.cpp:576-667): the plan
against hand-written lists, the construction errors, the summed gradient and
the update against float64 replays, snapshots, and the pycaffe view.

All CPU mode: the plan is the same in both modes, and what the GPU launches
for it is tests/test_reference_siamese.py.
"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import caffe_amd as ca
from engine_util import REPO, TOL, net_from_text, relerr
from test_caffemodel_wire import decode_blob, walk
from test_diff_sharing_plan import MODEL_ALIASES
from test_fusion_plan import MODEL_FUSIONS, MODEL_SHAPES


@pytest.fixture(autouse=True)
def cpu():
    ca.set_mode("cpu")
    yield
    ca.set_mode("cpu")


# ------------------------------------------------------------------- plan
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


def test_two_tower_plan():
    net = net_from_text(two_towers())
    assert net.param_sharing() == [
        ("conv_p", 0, "cw", "conv", 0), ("conv_p", 1, "cb", "conv", 1),
        ("ip_p", 0, "iw", "ip", 0), ("ip_p", 1, "ib", "ip", 1)]
    # 8 blobs, 4 learnable params: the owners, in backward order
    assert net.num_params() == 4
    assert [net.param_info(i)[:2] for i in range(4)] == [
        ("ip", 0), ("ip", 1), ("conv", 0), ("conv", 1)]


def test_one_shared_one_anonymous_blob_in_a_layer():
    net = net_from_text(two_towers(conv_b='param { name: "cw" } param { }',
                                   ip_b=""))
    assert net.param_sharing() == [("conv_p", 0, "cw", "conv", 0)]
    assert net.num_params() == 7
    infos = [net.param_info(i)[:2] for i in range(7)]
    assert ("conv_p", 1) in infos and ("conv_p", 0) not in infos


def test_name_shared_three_times():
    text = """name: "three"
layer { name: "input" type: "Input" top: "x"
  input_param { shape { dim: 2 dim: 4 } } }
"""
    bottom = "x"
    for name in ("a", "b", "c"):
        text += f"""layer {{ name: "{name}" type: "InnerProduct"
  bottom: "{bottom}" top: "{name}" param {{ name: "w" }}
  inner_product_param {{ num_output: 4 bias_term: false
    weight_filler {{ type: "xavier" }} }} }}
"""
        bottom = name
    net = net_from_text(text)
    assert net.param_sharing() == [("b", 0, "w", "a", 0),
                                   ("c", 0, "w", "a", 0)]
    assert net.num_params() == 1 and net.param_info(0)[:2] == ("a", 0)


PERMISSIVE = """name: "perm"
layer {{ name: "input" type: "Input" top: "x" top: "v"
  input_param {{ shape {{ dim: 2 dim: 1 dim: 5 dim: 5 }}
                shape {{ dim: 2 dim: {fan_in} }} }} }}
layer {{ name: "conv" type: "Convolution" bottom: "x" top: "conv"
  param {{ name: "w" }}
  convolution_param {{ num_output: 2 kernel_size: 3 bias_term: false
    weight_filler {{ type: "xavier" }} }} }}
layer {{ name: "ip" type: "InnerProduct" bottom: "v" top: "ip"
  param {{ name: "w" {mode} }}
  inner_product_param {{ num_output: 3 bias_term: false
    weight_filler {{ type: "xavier" }} }} }}
"""


def test_permissive_conv_weight_shared_with_ip_weight():
    # conv weight [2][1][3][3] and IP weight [3][6]: 18 values each
    net = net_from_text(PERMISSIVE.format(fan_in=6,
                                          mode="share_mode: PERMISSIVE"))
    assert net.param_sharing() == [("ip", 0, "w", "conv", 0)]
    assert net.num_params() == 1


@pytest.mark.parametrize("model", list(MODEL_SHAPES))
def test_benchmark_models_share_nothing_and_keep_their_plans(model):
    path = os.path.join(REPO, "models", "generated",
                        f"{model}_train_val.prototxt")
    if not os.path.exists(path):
        subprocess.check_call([sys.executable,
                               os.path.join(REPO, "models", "gen_models.py")])
    ca.set_synthetic_shape(*MODEL_SHAPES[model])
    net = ca.Net.from_file(path, phase=0, batch_override=2)
    assert net.param_sharing() == []
    counts = {}
    for kind, _, _ in net.fusions():
        counts[kind] = counts.get(kind, 0) + 1
    assert counts == MODEL_FUSIONS[model, 0]
    assert [d for _, _, d in net.diff_sharing()] == \
        ["alias"] * MODEL_ALIASES[model]


# ----------------------------------------------------------------- errors
def test_strict_shape_mismatch():
    with pytest.raises(ca.CaffeError) as e:
        net_from_text(PERMISSIVE.format(fan_in=6, mode=""))
    msg = str(e.value)
    assert "'w'" in msg and "'conv'" in msg and "'ip'" in msg
    assert "shape mismatch" in msg
    assert "2 1 3 3 (18)" in msg and "3 6 (18)" in msg


def test_permissive_count_mismatch():
    with pytest.raises(ca.CaffeError) as e:
        net_from_text(PERMISSIVE.format(fan_in=5,
                                        mode="share_mode: PERMISSIVE"))
    msg = str(e.value)
    assert "'w'" in msg and "'conv'" in msg and "'ip'" in msg
    assert "count mismatch" in msg
    assert "2 1 3 3 (18)" in msg and "3 5 (15)" in msg


@pytest.mark.parametrize("field", ["lr_mult", "decay_mult"])
def test_multiplier_mismatch(field):
    text = two_towers(conv_b=f'param {{ name: "cw" {field}: 3 }} '
                             'param { name: "cb" }')
    text = text.replace('param { name: "cw" } param { name: "cb" }',
                        f'param {{ name: "cw" {field}: 2 }} '
                        'param { name: "cb" }', 1)
    with pytest.raises(ca.CaffeError) as e:
        net_from_text(text)
    msg = str(e.value)
    assert "'cw'" in msg and "'conv'" in msg and "'conv_p'" in msg
    assert f"mismatched {field}" in msg


# ------------------------------------------------- gradient and update
N, D = 4, 5
LR, DECAY = 0.1, 0.01


def tied_solver(rule="", owner_spec="", sharer_spec="", iter_size=1,
                prefix=None):
    """y = W relu(W x + b) + b against a target, W and b shared by name."""
    snap = f'snapshot_prefix: "{prefix}"' if prefix else ""
    return f"""base_lr: {LR}
lr_policy: "fixed"
weight_decay: {DECAY}
random_seed: 5
iter_size: {iter_size}
{rule}
{snap}
net_param {{
  name: "tied"
  layer {{ name: "input" type: "Input" top: "x" top: "t"
    input_param {{ shape {{ dim: {N} dim: {D} }}
                  shape {{ dim: {N} dim: {D} }} }} }}
  layer {{ name: "a" type: "InnerProduct" bottom: "x" top: "h"
    param {{ name: "w" }} param {{ name: "b" {owner_spec} }}
    inner_product_param {{ num_output: {D}
      weight_filler {{ type: "gaussian" std: 0.5 }}
      bias_filler {{ type: "constant" value: 0.1 }} }} }}
  layer {{ name: "relu" type: "ReLU" bottom: "h" top: "r" }}
  layer {{ name: "a_p" type: "InnerProduct" bottom: "r" top: "y"
    param {{ name: "w" }} param {{ name: "b" {sharer_spec} }}
    inner_product_param {{ num_output: {D}
      weight_filler {{ type: "gaussian" std: 0.5 }}
      bias_filler {{ type: "constant" value: 0.7 }} }} }}
  layer {{ name: "loss" type: "EuclideanLoss" bottom: "y" bottom: "t"
    top: "loss" }}
}}
"""


def tied_inputs(net):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, D)).astype(np.float32)
    t = rng.standard_normal((N, D)).astype(np.float32)
    net.set_blob("x", x)
    net.set_blob("t", t)
    return x.astype(np.float64), t.astype(np.float64)


def tied_params(net):
    idx = {net.param_info(i)[:2]: i for i in range(net.num_params())}
    assert set(idx) == {("a", 0), ("a", 1)}
    return idx["a", 0], idx["a", 1]


def tied_grads64(W, b, x, t):
    """-> (first use, second use) of (dW, db)."""
    h = x @ W.T + b
    r = np.maximum(h, 0)
    y = r @ W.T + b
    dy = (y - t) / N
    dh = (dy @ W) * (h > 0)
    return (dh.T @ x, dh.sum(0)), (dy.T @ r, dy.sum(0))


def test_owner_diff_is_the_sum_of_both_uses():
    solver = ca.Solver(text=tied_solver())
    net = solver.net
    x, t = tied_inputs(net)
    wi, bi = tied_params(net)
    W = net.param(wi).astype(np.float64).reshape(D, D)
    b = net.param(bi).astype(np.float64)
    assert np.all(b == np.float32(0.1))  # the owner's filler, not 0.7
    (gw1, gb1), (gw2, gb2) = tied_grads64(W, b, x, t)
    for _ in range(2):  # backward overwrites: a second pass adds nothing
        net.forward()
        net.backward()
        gw, gb = net.param(wi, diff=True), net.param(bi, diff=True)
        assert relerr(gw, gw1 + gw2) <= TOL
        assert relerr(gb, gb1 + gb2) <= TOL
    for single in (gw1, gw2):
        assert relerr(gw, single) > 100 * TOL
    for single in (gb1, gb2):
        assert relerr(gb, single) > 100 * TOL


def test_summed_diff_under_iter_size_2():
    """Two sub-passes over the same inputs, scaled by 1/2: one momentum-free
    SGD step moves W by lr * (summed gradient + decay * W)."""
    solver = ca.Solver(text=tied_solver("momentum: 0.0", iter_size=2))
    net = solver.net
    x, t = tied_inputs(net)
    wi, bi = tied_params(net)
    W = net.param(wi).astype(np.float64).reshape(D, D)
    b = net.param(bi).astype(np.float64)
    (gw1, gb1), (gw2, gb2) = tied_grads64(W, b, x, t)
    solver.step(1)
    assert relerr(net.param(wi), W - LR * (gw1 + gw2 + DECAY * W)) <= TOL
    assert relerr(net.param(bi), b - LR * (gb1 + gb2 + DECAY * b)) <= TOL
    only_one = W - LR * (gw1 + DECAY * W)
    assert relerr(net.param(wi), only_one) > 100 * TOL


@pytest.mark.parametrize("side", ["owner", "sharer"])
@pytest.mark.parametrize("rule", ["SGD", "Adam"])
def test_update_applies_the_rule_once_to_the_sum(rule, side):
    """lr_mult 2 on the shared bias, given on one side only: the other side
    adopts it.  One step from zero history."""
    spec = dict(owner_spec="", sharer_spec="")
    spec[side + "_spec"] = "lr_mult: 2"
    rule_txt = ("momentum: 0.9" if rule == "SGD" else
                'type: "Adam" momentum: 0.9 momentum2: 0.999 delta: 1e-8')
    solver = ca.Solver(text=tied_solver(rule_txt, **spec))
    net = solver.net
    x, t = tied_inputs(net)
    wi, bi = tied_params(net)
    W = net.param(wi).astype(np.float64).reshape(D, D)
    b = net.param(bi).astype(np.float64)
    (gw1, gb1), (gw2, gb2) = tied_grads64(W, b, x, t)
    solver.step(1)
    for idx, p, g, lr_mult in ((wi, W, gw1 + gw2, 1.0),
                               (bi, b, gb1 + gb2, 2.0)):
        g = g + DECAY * p
        if rule == "SGD":
            want = p - LR * lr_mult * g
        else:  # t = 1; the engine floors Adam's delta at 1e-4
            m, v = 0.1 * g, 0.001 * g * g
            lr_t = LR * lr_mult * np.sqrt(1 - 0.999) / (1 - 0.9)
            want = p - lr_t * m / (np.sqrt(v) + 1e-4)
        assert relerr(net.param(idx), want) <= TOL, (rule, idx)
        # not the rule applied with the other multiplier
        other = p - (want - p) * (0.5 if lr_mult == 2.0 else 2.0)
        assert relerr(net.param(idx), other) > 100 * TOL


# --------------------------------------------------------------- snapshot
def layer_blobs(caffemodel):
    layers = {}
    for fnum, wt, v in walk(open(caffemodel, "rb").read()):
        if fnum == 100 and wt == 2:
            name, blobs = None, []
            for f2, w2, v2 in walk(v):
                if f2 == 1 and w2 == 2:
                    name = v2.decode()
                elif f2 == 7 and w2 == 2:
                    blobs.append(decode_blob(v2))
            layers[name] = blobs
    return layers


def test_snapshot_and_restore():
    with tempfile.TemporaryDirectory() as tmp:
        text = tied_solver("momentum: 0.9", prefix=os.path.join(tmp, "s"))
        solver = ca.Solver(text=text)
        tied_inputs(solver.net)
        wi, bi = tied_params(solver.net)
        solver.step(3)
        assert ca._lib.caffe_solver_snapshot(solver._h) == 0
        state = os.path.join(tmp, "s_iter_3.solverstate")
        hist = [decode_blob(v) for fnum, wt, v in walk(open(state, "rb").read())
                if fnum == 3 and wt == 2]
        # one history blob per owner, forward order: W then b
        assert [h[0] for h in hist] == [[D, D], [D]]
        assert np.array_equal(hist[0][1], solver.history(wi))
        layers = layer_blobs(os.path.join(tmp, "s_iter_3.caffemodel"))
        assert set(layers) == {"a", "a_p"}
        for (sa, da), (sp, dp) in zip(layers["a"], layers["a_p"]):
            assert sa == sp and np.array_equal(da, dp)
        assert np.array_equal(layers["a"][0][1], solver.net.param(wi))
        solver.step(2)
        want = solver.net.param(wi), solver.net.param(bi)

        resumed = ca.Solver(text=text)
        tied_inputs(resumed.net)
        assert ca._lib.caffe_solver_restore(resumed._h, state.encode()) == 0
        assert resumed.iter == 3
        resumed.step(2)
        assert np.array_equal(resumed.net.param(wi), want[0])
        assert np.array_equal(resumed.net.param(bi), want[1])
        assert not glob.glob(os.path.join(tmp, "*_iter_5*"))


# ---------------------------------------------------------------- pycaffe
def test_pycaffe_params_are_views_of_one_memory():
    from caffe_amd import pycaffe
    solver_text = tied_solver()
    net_text = solver_text[solver_text.index("net_param {") + 11:
                           solver_text.rindex("}")]
    with tempfile.NamedTemporaryFile("w", suffix=".prototxt",
                                     delete=False) as f:
        f.write(net_text)
    try:
        net = pycaffe.Net(f.name, 0)
    finally:
        os.unlink(f.name)
    a, a_p = net.params["a"][0].data, net.params["a_p"][0].data
    assert a.shape == a_p.shape == (D, D)
    assert np.array_equal(a, a_p)
    a_p[1, 2] = 42.5
    assert net.params["a"][0].data[1, 2] == 42.5
    assert a.ctypes.data == a_p.ctypes.data
    net.params["a"][1].data[...] = 3.0
    assert np.all(net.params["a_p"][1].data == 3.0)
