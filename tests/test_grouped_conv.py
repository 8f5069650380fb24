"""Grouped convolution with few channels per group (group >= 8, C/group in
4..32, Cout/group in 1..32, kh*kw <= 49): the direct gfx950 kernels against
the float64 oracle, and the route that picks them.

In GPU mode such a layer must run the three gconv kernels and not a single
GEMM; everything else keeps the per-group GEMM loop.  The same rows run in
CPU mode for the values alone."""
import numpy as np
import pytest

import caffe_amd as ca
from engine_util import TOL, relerr, run_layer
from oracle import oracle as orc

GPU = pytest.param("gpu", marks=pytest.mark.gpu)
GROUP = 8

# id: (N, C, Co, H, W, (kh, kw), (sh, sw), (ph, pw), d, bias, var of fwd/dgrad)
# all at group 8.  G4: 41x70 is cut into 2x2 tiles of 21x36, ragged both
# ways.  G8: 32 * 25 * 32 weights alone exceed the 64 KB LDS budget, so the
# block loops over channel chunks.  G9: 5 images in 4 batch slices.  G10
# (beyond the issue's nine): 32 x 32 pairs of a 3x3, four output channels
# per wgrad thread.
ROWS = {
    "G1": (2, 32, 32, 7, 7, (3, 3), (1, 1), (1, 1), 1, True, "k3s1_plane"),
    "G2": (3, 32, 64, 15, 15, (3, 3), (2, 2), (1, 1), 1, False, "k3s2_plane"),
    "G3": (2, 64, 32, 9, 9, (3, 3), (1, 1), (1, 1), 1, True, "k3s1_plane"),
    "G4": (2, 32, 32, 41, 70, (3, 3), (1, 1), (1, 1), 1, False, "k3s1_tile"),
    "G5": (2, 40, 24, 11, 14, (2, 5), (2, 1), (1, 2), 1, False,
           "generic_plane"),
    "G6": (2, 32, 32, 12, 12, (3, 3), (1, 1), (2, 2), 2, False,
           "generic_plane"),
    "G7": (2, 96, 96, 8, 8, (1, 1), (1, 1), (0, 0), 1, False,
           "generic_plane"),
    "G8": (2, 256, 256, 6, 6, (5, 5), (1, 1), (2, 2), 1, False,
           "generic_plane"),
    "G9": (5, 128, 128, 14, 14, (3, 3), (1, 1), (1, 1), 1, True,
           "k3s1_plane"),
    "G10": (2, 256, 256, 5, 5, (3, 3), (1, 1), (1, 1), 1, True, "k3s1_plane"),
}


def run_gc(mode, row, grp=GROUP, relu=False, seed=0):
    """One Convolution layer (optional in-place ReLU) forward and backward.
    Returns the net, y and the oracle's (y, dx, dW, db); with relu, of the
    masked dy as check_conv_relu has it."""
    N, C, Co, H, W, (kh, kw), (sh, sw), (ph, pw), d, bias = row[:10]
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
    """fn() with both traces on: (fn's result, gconv records, GEMM records)"""
    ca.kernel_trace(True)
    ca.gemm_trace(True)
    try:
        out = fn()
    finally:
        ca.kernel_trace(False)
        ca.gemm_trace(False)
    gc = [k for k in ca.kernel_trace_read() if k["op"].startswith("gconv")]
    return out, gc, ca.gemm_trace_read()


def check_gc_trace(gc, gemms, row, grp=GROUP):
    assert gemms == []
    assert [k["op"] for k in gc] == ["gconv_fwd", "gconv_bwd_weight",
                                     "gconv_bwd_data"]
    assert gc[0]["var"] == gc[2]["var"] == row[10]
    assert gc[1]["var"] == row[10].split("_")[0]
    assert gc[1]["bias"] == int(row[9])
    for k in gc:
        assert (k["cig"], k["cog"]) == (row[1] // grp, row[2] // grp)
    if row[10].endswith("tile"):
        assert gc[0]["tiles_y"] >= 2 and gc[0]["tiles_x"] >= 2
        assert gc[2]["tiles_y"] >= 2 and gc[2]["tiles_x"] >= 2


@pytest.mark.parametrize("mode", ["cpu", GPU])
@pytest.mark.parametrize("rid", list(ROWS))
def test_grouped_matches_oracle(rid, mode):
    row = ROWS[rid]
    if mode == "cpu":
        net, y, ref = run_gc(mode, row)
    else:
        (net, y, ref), gc, gemms = traced(lambda: run_gc(mode, row))
        check_gc_trace(gc, gemms, row)
        if rid == "G1":
            assert gc[0]["planes"] > 1  # several whole planes per block
        if rid == "G8":  # the weights do not fit LDS at once
            assert gc[0]["chunks"] >= 2 and gc[2]["chunks"] >= 2
        if rid == "G9":  # uneven batch slices
            assert 5 % gc[1]["slices"] != 0
        if rid == "G10":  # several output channels per wgrad thread
            assert gc[1]["pairs"] == 4
    check_values(net, y, ref, row[9])


@pytest.mark.parametrize("mode", ["cpu", GPU])
def test_fused_relu(mode):
    row = ROWS["G1"]
    if mode == "cpu":
        net, y, ref = run_gc(mode, row, relu=True)
    else:
        (net, y, ref), gc, gemms = traced(
            lambda: run_gc(mode, row, relu=True))
        check_gc_trace(gc, gemms, row)
    assert [f[0] for f in net.fusions()] == ["conv_relu"]
    assert np.asarray(y).min() >= 0
    check_values(net, y, ref, True)


@pytest.mark.gpu
def test_deterministic():
    runs = []
    for _ in range(2):
        net, y, _ = run_gc("gpu", ROWS["G9"])
        runs.append([np.asarray(a).copy()
                     for a in [y] + engine_grads(net, True)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("row,grp", [
    ((2, 16, 16, 9, 9, (3, 3), (1, 1), (1, 1), 1, True), 4),     # group < 8
    ((2, 264, 64, 5, 5, (3, 3), (1, 1), (1, 1), 1, True), 8),    # cig = 33
    ((2, 32, 32, 12, 12, (8, 8), (1, 1), (3, 3), 1, True), 8),   # 64 taps
], ids=["group4", "cig33", "k8x8"])
def test_route_boundary_stays_on_gemm(row, grp):
    (net, y, ref), gc, gemms = traced(lambda: run_gc("gpu", row, grp=grp))
    assert gc == [] and len(gemms) >= 3 * grp
    check_values(net, y, ref, True)


@pytest.mark.gpu
def test_bf16_compute_runs_the_same_fp32_kernels():
    row = ROWS["G3"]
    ca.set_compute("bf16")
    try:
        (net, y, ref), gc, gemms = traced(lambda: run_gc("gpu", row))
    finally:
        ca.set_compute("f32")
    check_gc_trace(gc, gemms, row)
    check_values(net, y, ref, True)  # fp32 TOL, not the bf16 class
