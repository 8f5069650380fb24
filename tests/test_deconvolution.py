"""Deconvolution (transposed convolution) and the bilinear filler against
torch.nn.functional.conv_transpose2d in float64 on the CPU, with autograd
for dx, dW and db.  In GPU mode a layer with stride > 1 and dilation 1 must
run the phase-split kernel of kernels/deconv.hip (one deconv_fwd record, no
GEMM in forward); stride 1, dilation > 1 and CAFFE_DECONV=0 keep the GEMM +
col2im form."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import caffe_amd as ca
from engine_util import TOL, input_net, net_from_text, relerr, run_layer

GPU = pytest.param("gpu", marks=pytest.mark.gpu)

# Kernel of deconv.hip each row launches (extend the rows of the one you edit):
# mfma<1,2> V1 | mfma<2,2> V2 | mfma<1,4> T2 T4-T9 V3 V4 V6 V7 V8 V13
# | mfma<2,4> T1 T3 V5 V14 | direct<1> T10 V12 | direct<2> V9
# | direct<4> V10 V11 | none (GEMM + col2im) S1 D2 R1
# id: (N, Ci, Co, group, H, W, kernel, stride, pad, bias, dilation, var)
ROWS = {
    "T1": (2, 32, 64, 1, 5, 5, 4, 2, 1, True, 1, "mfma"),
    "T2": (3, 32, 32, 1, 6, 7, 3, 2, 0, False, 1, "mfma"),
    "T3": (2, 24, 40, 1, 5, 6, 2, 2, 0, True, 1, "mfma"),
    "T4": (2, 32, 32, 1, 6, 5, (3, 5), (2, 3), (1, 2), False, 1, "mfma"),
    "T5": (2, 32, 32, 1, 4, 4, 2, 3, 0, True, 1, "mfma"),
    "T6": (2, 64, 64, 2, 5, 5, 4, 2, 1, False, 1, "mfma"),
    "T7": (1, 16, 16, 1, 19, 37, 4, 2, 1, False, 1, None),
    "T8": (2, 192, 32, 1, 4, 4, 4, 2, 1, False, 1, "mfma"),
    "T9": (2, 32, 32, 1, 3, 3, 8, 4, 2, True, 1, "mfma"),
    "T10": (2, 21, 21, 21, 6, 6, 4, 2, 1, False, 1, "direct"),
    # the fallback boundary: stride 1, dilation 2
    "S1": (2, 16, 24, 1, 6, 7, 3, 1, 1, True, 1, None),
    "D2": (2, 16, 24, 2, 5, 6, 3, 2, 1, True, 2, None),
    # P == 2: stride along one axis only; pad >= stride on the stride-1 axis
    "V1": (2, 16, 24, 1, 5, 6, (4, 3), (2, 1), (1, 1), True, 1, "mfma"),
    # the paired 8-byte store with an odd OW (13)
    "V2": (2, 16, 40, 1, 5, 6, (3, 3), (1, 2), (1, 0), False, 1, "mfma"),
    # pad >= stride (dq > 0): the k5 s2 p2 layer; OH = 9 is odd
    "V3": (2, 32, 32, 1, 5, 6, 5, 2, 2, True, 1, "mfma"),
    # dq = (2, 1), phases whose dq differs along H, two passes of phases
    "V4": (2, 16, 16, 1, 6, 5, (7, 6), (2, 3), (5, 3), False, 1, "mfma"),
    # Cout/group 96: two channel tiles of 64, the second half empty
    "V5": (2, 20, 192, 2, 4, 5, 4, 2, 1, True, 1, "mfma"),
    # odd C/group: the zeroed second channel of the last k-pair
    "V6": (2, 7, 8, 1, 5, 5, 3, 2, 1, True, 1, "mfma"),
    # a last chunk of one channel; chunks >= 2 with more than four phases
    "V7": (1, 33, 16, 1, 4, 4, 3, 3, 1, False, 1, "mfma"),
    # the FCN 21-class 8x upsampler, ungrouped: 64 phases in 16 passes
    "V8": (1, 21, 21, 1, 3, 3, 16, 8, 4, False, 1, "mfma"),
    # direct, two channels per thread, 2 x 2 cell tiles
    "V9": (1, 12, 8, 4, 10, 20, 4, 2, 1, True, 1, "direct"),
    # direct, Cout/group 3 padded to 4: the pad channel is not stored
    "V10": (2, 8, 6, 2, 5, 6, 3, 2, 0, True, 1, "direct"),
    "V11": (2, 5, 20, 5, 4, 5, (5, 4), (3, 2), (2, 1), False, 1, "direct"),
    "V12": (2, 3, 3, 3, 5, 6, 5, 2, 2, True, 1, "direct"),
    # the window, not the channel count, sets the chunk: 16 of 32 channels
    "V13": (1, 32, 32, 1, 2, 2, 24, 2, 0, False, 1, "mfma"),
    # three chunks and three passes of phases
    "V14": (2, 96, 40, 1, 3, 3, 3, 3, 0, True, 1, "mfma"),
    # Cout/group <= 4 with C/group > 4: refused, keeps the GEMM route
    "R1": (2, 16, 3, 1, 5, 5, 4, 2, 1, True, 1, None),
}

# what dc_plan() of deconv.hip gives for a row, as the deconv_fwd record shows
PLAN = {
    "V1": {"chunks": 1},
    "V2": {"blocks": 2},
    "V5": {"blocks": 8},
    "V6": {"chunks": 1},
    "V7": {"chunks": 2},
    "V9": {"tiles_y": 2, "tiles_x": 2, "blocks": 16},
    "V13": {"chunks": 2, "tiles_y": 2},
    "V14": {"chunks": 3},
}


def pair(v):
    return v if isinstance(v, tuple) else (v, v)


def layer_text(row, relu=False, extra="", name="up", bottom="in0", top="out"):
    Co, g, bias, d = row[2], row[3], row[9], row[10]
    (kh, kw), (sh, sw), (ph, pw) = pair(row[6]), pair(row[7]), pair(row[8])
    text = f"""layer {{
  name: "{name}" type: "Deconvolution" bottom: "{bottom}" top: "{top}"
  convolution_param {{
    num_output: {Co} group: {g} dilation: {d}
    kernel_h: {kh} kernel_w: {kw} stride_h: {sh} stride_w: {sw}
    pad_h: {ph} pad_w: {pw} bias_term: {"true" if bias else "false"} {extra}
  }}
}}"""
    if relu:
        text += '\nlayer { name: "relu" type: "ReLU" bottom: "out" top: "out" }'
    return text


@functools.lru_cache(maxsize=None)
def case(rid, relu=False):
    """Inputs and the float64 reference of a row, computed once:
    (x, w, b, dy, (y, dx, dW, db))"""
    N, Ci, Co, g, H, W, k, s, p, bias, d = ROWS[rid][:11]
    r = np.random.default_rng(sum(map(ord, rid)))
    x = r.standard_normal((N, Ci, H, W)).astype(np.float32)
    w = (r.standard_normal((Ci, Co // g) + pair(k)) * 0.3).astype(np.float32)
    b = r.standard_normal(Co).astype(np.float32) if bias else None
    tx, tw, tb = (None if a is None else
                  torch.tensor(a, dtype=torch.float64, requires_grad=True)
                  for a in (x, w, b))
    y = torch.nn.functional.conv_transpose2d(
        tx, tw, tb, stride=pair(s), padding=pair(p), groups=g, dilation=d)
    dy = r.standard_normal(tuple(y.shape)).astype(np.float32)
    if relu:
        dy[np.abs(y.detach().numpy()) < 1e-3] = 0
        y = torch.relu(y)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    ref = [y.detach().numpy(), tx.grad.numpy(), tw.grad.numpy()]
    return x, w, b, dy, ref + ([tb.grad.numpy()] if bias else [])


def run_row(mode, rid, relu=False):
    """Forward with both traces on, then backward.  Returns (net, [y, dx,
    dW, db], deconv_fwd records, GEMM records of forward)."""
    x, w, b, dy, _ = case(rid, relu)
    ca.kernel_trace(True)
    ca.gemm_trace(True)
    try:
        net, y = run_layer(mode, [x.shape], layer_text(ROWS[rid], relu), [x],
                           params=[w] if b is None else [w, b])
    finally:
        ca.kernel_trace(False)
        ca.gemm_trace(False)
    recs = [k for k in ca.kernel_trace_read() if k["op"] == "deconv_fwd"]
    gemms = ca.gemm_trace_read()
    net.set_blob("out", dy, diff=True)
    net.backward()
    got = [y, net.blob("in0", diff=True), net.param(0, diff=True)]
    return net, got + ([] if b is None else [net.param(1, diff=True)]), \
        recs, gemms


def check_values(got, ref):
    assert len(got) == len(ref)
    for name, a, b in zip(("y", "dx", "dW", "db"), got, ref):
        err = relerr(a, b)
        print(name, err)
        assert err < TOL, (name, err)


@pytest.mark.parametrize("mode", ["cpu", GPU])
@pytest.mark.parametrize("rid", [r for r in ROWS if r[0] in "TV"])
def test_matches_conv_transpose2d(rid, mode):
    row = ROWS[rid]
    _, got, recs, gemms = run_row(mode, rid)
    if mode == "gpu":
        sh, sw = pair(row[7])
        assert gemms == []
        assert len(recs) == 1 and recs[0]["phases"] == sh * sw, recs
        assert row[11] is None or recs[0]["var"] == row[11], recs
        want = PLAN.get(rid, {})
        assert {k: recs[0][k] for k in want} == want, recs
        if rid == "T7":
            assert recs[0]["tiles_y"] >= 2 and recs[0]["tiles_x"] >= 2
        if rid == "T8":
            assert recs[0]["chunks"] >= 2
    check_values(got, case(rid)[4])


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ["S1", "D2"])
def test_stride1_and_dilation_stay_on_gemm(rid):
    _, got, recs, gemms = run_row("gpu", rid)
    assert recs == [] and len(gemms) >= ROWS[rid][3], (recs, gemms)
    check_values(got, case(rid)[4])


@pytest.mark.parametrize("mode", ["cpu", GPU])
def test_refused_zone_stays_on_gemm(mode):
    """Cout/group <= 4 with C/group > 4 is refused by deconv_supported()"""
    _, got, recs, gemms = run_row(mode, "R1")
    if mode == "gpu":
        assert recs == [] and len(gemms) >= ROWS["R1"][3], (recs, gemms)
    check_values(got, case("R1")[4])


def traced_forward(net):
    """net.forward() with the kernel trace on: its deconv_fwd records"""
    ca.kernel_trace(True)
    try:
        net.forward()
    finally:
        ca.kernel_trace(False)
    return [k for k in ca.kernel_trace_read() if k["op"] == "deconv_fwd"]


def row_net(mode, rid):
    """run_row() up to the forward: the net with its input and params set"""
    x, w, b, _, _ = case(rid)
    ca.set_mode(mode)
    net = net_from_text(input_net([x.shape], layer_text(ROWS[rid])))
    net.set_blob("in0", x)
    for i, p in enumerate([w] if b is None else [w, b]):
        net.set_param(i, p.ravel())
    return net


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ["T1", "T2", "V2", "V5", "V9", "V10"])
def test_every_output_element_is_written(rid):
    """The top starts as NaN, not as the zeros a fresh blob holds: an element
    the kernel skips cannot pass as a small value"""
    ref = case(rid)[4]
    net = row_net("gpu", rid)
    net.set_blob("out", np.full(ref[0].shape, np.nan, np.float32))
    assert np.isnan(net.blob("out")).all()
    assert len(traced_forward(net)) == 1
    y = net.blob("out")
    assert np.isfinite(y).all(), np.argwhere(~np.isfinite(y))[:8]
    check_values([y], ref[:1])


@pytest.mark.parametrize("mode", ["cpu", GPU])
def test_new_weights_are_packed_again(mode):
    """The packed copy of the weights is made per forward: after set_param
    the next forward computes with the new ones"""
    rid = "V3"
    x, w, b, _, ref = case(rid)
    net = row_net(mode, rid)
    net.forward()
    y1 = net.blob("out")
    check_values([y1], ref[:1])
    r = np.random.default_rng(5)
    w2 = (r.standard_normal(w.shape) * 0.3).astype(np.float32)
    b2 = r.standard_normal(b.shape).astype(np.float32)
    net.set_param(0, w2.ravel())
    net.set_param(1, b2)
    recs = traced_forward(net)
    assert mode == "cpu" or len(recs) == 1, recs
    y2 = net.blob("out")
    s, p = pair(ROWS[rid][7]), pair(ROWS[rid][8])
    ref2 = torch.nn.functional.conv_transpose2d(
        *(torch.tensor(a, dtype=torch.float64) for a in (x, w2, b2)),
        stride=s, padding=p).numpy()
    check_values([y2], [ref2])
    assert relerr(y2, y1) > 0.1


# up2 on the 8 channels of up1 (row V6): Cout 96, so its packed weights are
# larger than up1's and the workspace slot they share grows between the two
UP2 = (2, 8, 96, 1, 9, 9, 4, 2, 1, True, 1)


@functools.lru_cache(maxsize=None)
def two_layer_case():
    """(x, [w1, b1, w2, b2], dy, [y, dx, dW1, db1, dW2, db2]) of in0 -> up1
    (row V6) -> up2 (UP2), float64"""
    r = np.random.default_rng(77)
    x = case("V6")[0]
    params = []
    for row in (ROWS["V6"], UP2):
        shape = (row[1], row[2] // row[3]) + pair(row[6])
        params += [(r.standard_normal(shape) * 0.3).astype(np.float32),
                   r.standard_normal(row[2]).astype(np.float32)]
    tx, *tp = (torch.tensor(a, dtype=torch.float64, requires_grad=True)
               for a in [x] + params)
    y = tx
    for i, row in enumerate((ROWS["V6"], UP2)):
        y = torch.nn.functional.conv_transpose2d(
            y, tp[2 * i], tp[2 * i + 1], stride=pair(row[7]),
            padding=pair(row[8]))
    dy = r.standard_normal(tuple(y.shape)).astype(np.float32)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    return x, params, dy, [y.detach().numpy(), tx.grad.numpy()] + \
        [p.grad.numpy() for p in tp]


@pytest.mark.parametrize("mode", ["cpu", GPU])
def test_two_layers_share_the_weight_slot(mode):
    """A decoder's shape: two Deconvolution layers of different size in one
    net, forward and backward twice without rebuilding"""
    x, params, dy, ref = two_layer_case()
    ca.set_mode(mode)
    net = net_from_text(input_net(
        [x.shape], layer_text(ROWS["V6"], name="up1", top="mid") + "\n" +
        layer_text(UP2, name="up2", bottom="mid")))
    net.set_blob("in0", x)
    # the net lists its params in an order of its own: find them by layer
    at = {info[:2]: i for i, info in net.params().items()}
    idx = [at[key] for key in (("up1", 0), ("up1", 1), ("up2", 0), ("up2", 1))]
    for i, p in zip(idx, params):
        net.set_param(i, p.ravel())
    runs = []
    for _ in range(2):
        recs = traced_forward(net)
        if mode == "gpu":
            assert [k["var"] for k in recs] == ["mfma", "mfma"], recs
        y = net.blob("out")
        net.set_blob("out", dy, diff=True)
        net.backward()
        got = [y, net.blob("in0", diff=True)] + \
            [net.param(i, diff=True) for i in idx]
        for name, a, b in zip(("y", "dx", "dW1", "db1", "dW2", "db2"), got,
                              ref):
            err = relerr(a, b)
            print(name, err)
            assert err < TOL, (name, err)
        runs.append(got)
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# torch-free (its bundled ROCm runtime must not load after the engine's)
_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {tests!r})
from engine_util import run_layer
import caffe_amd as ca
d = np.load({path!r})
ca.kernel_trace(True)
ca.gemm_trace(True)
net, y = run_layer("gpu", [d["x"].shape], {body!r}, [d["x"]],
                   params=[d["w"], d["b"]])
assert all(k["op"] != "deconv_fwd" for k in ca.kernel_trace_read())
assert ca.gemm_trace_read()
net.set_blob("out", d["dy"], diff=True)
net.backward()
np.savez({out!r}, y, net.blob("in0", diff=True), net.param(0, diff=True),
         net.param(1, diff=True))
"""


@pytest.mark.gpu
def test_env_switch_forces_the_fallback(tmp_path):
    """CAFFE_DECONV=0 is read once per process: T1 in a child that gets the
    inputs and returns y, dx, dW, db through one file"""
    x, w, b, dy, ref = case("T1")
    path, res = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(path, x=x, w=w, b=b, dy=dy)
    code = _CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)),
                         path=path, out=res, body=layer_text(ROWS["T1"]))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True,
                         env=dict(os.environ, CAFFE_DECONV="0"), text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.load(res)
    check_values([got[k] for k in got.files], ref)


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ["T1", "V2", "V9", "V14"])
def test_rerun_is_bit_identical(rid):
    """mfma<2,4>, the paired store, direct, and several chunks and passes"""
    runs = [[np.asarray(a).copy() for a in run_row("gpu", rid)[1][:3]]
            for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("mode", ["cpu", GPU])
def test_in_place_relu_is_not_fused(mode):
    net, got, _, _ = run_row(mode, "T1", relu=True)
    assert net.fusions() == []
    assert np.asarray(got[0]).min() >= 0
    check_values(got, case("T1", True)[4])


def bilinear_net(mode, C, k, s, p, H):
    ca.set_mode(mode)
    row = (1, C, C, C, H, H, k, s, p, False, 1)
    return net_from_text(input_net(
        [(1, C, H, H)], layer_text(row, extra='weight_filler { type: '
                                   '"bilinear" }').replace(
            'top: "out"', 'top: "out" param { lr_mult: 0 }')))


def test_bilinear_filler_closed_form():
    k = 4
    f = (k + 1) // 2
    c = (2 * f - 1 - f % 2) / (2.0 * f)
    v = 1 - np.abs(np.arange(k) / f - c)
    got = np.asarray(bilinear_net("cpu", 3, k, 2, 1, 5).param(0))
    assert relerr(got, np.tile(np.outer(v, v), (3, 1, 1, 1))) < 1e-6


@pytest.mark.parametrize("mode", ["cpu", GPU])
def test_bilinear_upsampling_keeps_a_constant(mode):
    net = bilinear_net(mode, 3, 4, 2, 1, 6)
    net.set_blob("in0", np.full((1, 3, 6, 6), 2.5, np.float32))
    net.forward()
    out = np.asarray(net.blob("out")).reshape(1, 3, 12, 12)
    assert np.abs(out[..., 1:-1, 1:-1] - 2.5).max() < 1e-6


@pytest.mark.parametrize("row,what", [
    ((1, 6, 8, 4, 5, 5, 3, 2, 1, True, 1), "input channels"),
    ((1, 8, 6, 4, 5, 5, 3, 2, 1, True, 1), "num_output"),
    ((1, 4, 4, 1, 2, 2, 1, 1, 1, True, 1), "top size"),
], ids=["channels", "num_output", "top_size"])
def test_construction_errors_name_the_layer(row, what):
    ca.set_mode("cpu")
    with pytest.raises(Exception) as e:
        net_from_text(input_net([(row[0], row[1], row[4], row[5])],
                                layer_text(row)))
    assert "Deconvolution layer 'up'" in str(e.value) and what in str(e.value)
