"""Depthwise convolution (Convolution with group == C): the direct gfx950
kernels against the float64 oracle, and the route that picks them.

In GPU mode a depthwise layer (group >= 8, kh*kw <= 49) must run the three
dwconv kernels and not a single GEMM; everything else keeps the GEMM route.
The same rows run in CPU mode for the values alone."""
import numpy as np
import pytest

import caffe_amd as ca
from engine_util import TOL, relerr, run_layer
from oracle import oracle as orc

GPU = pytest.param("gpu", marks=pytest.mark.gpu)

# id: (N, C, Co, H, W, (kh, kw), (sh, sw), (ph, pw), d, bias, var of fwd/dgrad)
# The forward / dgrad tile is at most 64 columns, balanced, and then as many
# rows as fill 256 threads at 4 pixels each: 41x70 is cut into 2x2 tiles of
# 21x36, ragged both ways (20 rows, 34 columns in the last).  D4s2 is the
# same for stride 2: y 41x67 in 2x2 tiles of 21x36, dx 81x133 in 4x3 of 21x48.
ROWS = {
    "D1": (2, 8, 8, 7, 7, (3, 3), (1, 1), (1, 1), 1, True, "k3s1_plane"),
    "D2": (3, 8, 8, 15, 15, (3, 3), (2, 2), (1, 1), 1, False, "k3s2_plane"),
    "D3": (2, 8, 16, 9, 9, (3, 3), (1, 1), (1, 1), 1, True, "k3s1_plane"),
    "D4": (2, 8, 8, 41, 70, (3, 3), (1, 1), (1, 1), 1, False, "k3s1_tile"),
    "D4s2": (2, 8, 8, 81, 133, (3, 3), (2, 2), (1, 1), 1, False, "k3s2_tile"),
    "D5k5": (2, 8, 8, 12, 12, (5, 5), (1, 1), (2, 2), 1, False,
             "generic_plane"),
    "D5d2": (2, 8, 8, 12, 12, (3, 3), (1, 1), (2, 2), 2, False,
             "generic_plane"),
    "D6": (2, 8, 8, 11, 14, (2, 5), (2, 1), (1, 2), 1, False,
           "generic_plane"),
    "D7": (5, 16, 16, 14, 14, (3, 3), (1, 1), (1, 1), 1, True, "k3s1_plane"),
    "D8": (2, 8, 8, 7, 7, (3, 3), (1, 1), (0, 0), 1, False, "k3s1_plane"),
}


def run_dw(mode, row, grp=None, relu=False, seed=0):
    """One Convolution layer (group = C unless given, optional in-place
    ReLU) forward and backward.  Returns the net, y and the oracle's
    (y, dx, dW, db); with relu, of the masked dy as check_conv_relu has it."""
    N, C, Co, H, W, (kh, kw), (sh, sw), (ph, pw), d, bias = row[:10]
    grp = C if grp is None else grp
    r = np.random.default_rng(seed)
    x = r.standard_normal((N, C, H, W)).astype(np.float32)
    w = (r.standard_normal((Co, C // grp, kh, kw)) * 0.3).astype(np.float32)
    b = r.standard_normal(Co).astype(np.float32) if bias else None
    body = f"""layer {{
  name: "conv" type: "Convolution" bottom: "in0" top: "out"
  convolution_param {{
    num_output: {Co} group: {grp} dilation: {d}
    kernel_h: {kh} kernel_w: {kw} stride_h: {sh} stride_w: {sw}
    pad_h: {ph} pad_w: {pw} bias_term: {"true" if bias else "false"}
  }}
}}"""
    if relu:
        body += '\nlayer { name: "relu" type: "ReLU" bottom: "out" top: "out" }'
    geo = dict(pad=(ph, pw), stride=(sh, sw), dil=(d, d), group=grp)
    pre = orc.conv_fwd(x, w, b, **geo)
    dy = r.standard_normal(pre.shape).astype(np.float32)
    y_ref, dpre = pre, dy
    if relu:
        dy[np.abs(pre) < 1e-3] = 0
        y_ref, dpre = np.maximum(pre, 0), (dy * (pre > 0)).astype(np.float32)
    net, y = run_layer(mode, [x.shape], body, [x],
                       params=[w, b] if bias else [w], top_diff=dy)
    return net, y, (y_ref,) + tuple(orc.conv_bwd(x, w, dpre, want_db=bias,
                                                 **geo))


def engine_grads(net, bias):
    return [net.blob("in0", diff=True), net.param(0, diff=True)] + (
        [net.param(1, diff=True)] if bias else [])


def check_values(net, y, ref, bias):
    got = [y] + engine_grads(net, bias)
    for name, a, b in zip(("y", "dx", "dW", "db"), got, ref):
        err = relerr(a, b)
        print(name, err)
        assert err < TOL, (name, err)


def traced(fn):
    """fn() with both traces on: (fn's result, dwconv records, GEMM records)"""
    ca.kernel_trace(True)
    ca.gemm_trace(True)
    try:
        out = fn()
    finally:
        ca.kernel_trace(False)
        ca.gemm_trace(False)
    dw = [k for k in ca.kernel_trace_read() if k["op"].startswith("dwconv")]
    return out, dw, ca.gemm_trace_read()


def check_dw_trace(dw, gemms, row):
    assert gemms == []
    assert [k["op"] for k in dw] == ["dwconv_fwd", "dwconv_bwd_weight",
                                     "dwconv_bwd_data"]
    assert dw[0]["var"] == dw[2]["var"] == row[10]
    assert dw[1]["var"] == ("k3" if row[5] == (3, 3) else "generic")
    assert dw[1]["bias"] == int(row[9])
    if row[10].endswith("tile"):
        assert dw[0]["tiles_y"] >= 2 and dw[0]["tiles_x"] >= 2
        assert dw[2]["tiles_y"] >= 2 and dw[2]["tiles_x"] >= 2


@pytest.mark.parametrize("mode", ["cpu", GPU])
@pytest.mark.parametrize("rid", list(ROWS))
def test_depthwise_matches_oracle(rid, mode):
    row = ROWS[rid]
    if mode == "cpu":
        net, y, ref = run_dw(mode, row)
    else:
        (net, y, ref), dw, gemms = traced(lambda: run_dw(mode, row))
        check_dw_trace(dw, gemms, row)
        if rid == "D1":
            assert dw[0]["planes"] > 1  # several whole planes per block
        if rid == "D7":  # uneven batch slices, channels over several blocks
            assert 5 % dw[1]["slices"] != 0 and dw[0]["blocks"] > 1
    check_values(net, y, ref, row[9])


@pytest.mark.parametrize("mode", ["cpu", GPU])
def test_fused_relu(mode):
    row = ROWS["D1"]
    if mode == "cpu":
        net, y, ref = run_dw(mode, row, relu=True)
    else:
        (net, y, ref), dw, gemms = traced(
            lambda: run_dw(mode, row, relu=True))
        check_dw_trace(dw, gemms, row)
    assert [f[0] for f in net.fusions()] == ["conv_relu"]
    assert np.asarray(y).min() >= 0
    check_values(net, y, ref, True)


@pytest.mark.gpu
def test_deterministic():
    runs = []
    for _ in range(2):
        net, y, _ = run_dw("gpu", ROWS["D7"])
        runs.append([np.asarray(a).copy()
                     for a in [y] + engine_grads(net, True)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("row,grp", [
    ((2, 4, 4, 9, 9, (3, 3), (1, 1), (1, 1), 1, True), 4),    # group < 8
    ((2, 16, 16, 9, 9, (3, 3), (1, 1), (1, 1), 1, True), 8),  # cig = 2
    ((2, 8, 8, 12, 12, (8, 8), (1, 1), (3, 3), 1, True), 8),  # 64 taps
], ids=["group4", "cig2", "k8x8"])
def test_route_boundary_stays_on_gemm(row, grp):
    (net, y, ref), dw, gemms = traced(lambda: run_dw("gpu", row, grp=grp))
    assert dw == [] and len(gemms) >= 3 * grp
    check_values(net, y, ref, True)


@pytest.mark.gpu
def test_bf16_compute_runs_the_same_fp32_kernels():
    row = ROWS["D3"]
    ca.set_compute("bf16")
    try:
        (net, y, ref), dw, gemms = traced(lambda: run_dw("gpu", row))
    finally:
        ca.set_compute("f32")
    check_dw_trace(dw, gemms, row)
    check_values(net, y, ref, True)  # fp32 TOL, not the bf16 class


@pytest.mark.gpu
def test_live_bytes_return_after_free():
    def cycle():
        net, _, _ = run_dw("gpu", ROWS["D7"])
        ca._lib.caffe_net_free(net._h)

    cycle()  # the first cycle grows the process-lifetime workspace slots
    before = ca.device_live_bytes()
    cycle()
    assert ca.device_live_bytes() == before
