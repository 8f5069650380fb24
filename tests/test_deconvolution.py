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
}


def pair(v):
    return v if isinstance(v, tuple) else (v, v)


def layer_text(row, relu=False, extra=""):
    Co, g, bias, d = row[2], row[3], row[9], row[10]
    (kh, kw), (sh, sw), (ph, pw) = pair(row[6]), pair(row[7]), pair(row[8])
    text = f"""layer {{
  name: "up" type: "Deconvolution" bottom: "in0" top: "out"
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
@pytest.mark.parametrize("rid", [r for r in ROWS if r.startswith("T")])
def test_matches_conv_transpose2d(rid, mode):
    row = ROWS[rid]
    _, got, recs, gemms = run_row(mode, rid)
    if mode == "gpu":
        sh, sw = pair(row[7])
        assert gemms == []
        assert len(recs) == 1 and recs[0]["phases"] == sh * sw, recs
        assert row[11] is None or recs[0]["var"] == row[11], recs
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
def test_rerun_is_bit_identical():
    runs = [[np.asarray(a).copy() for a in run_row("gpu", "T1")[1][:3]]
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
