"""Backward of Deconvolution against float64 conv_transpose2d autograd.  In
GPU mode a layer with stride > 1 and dilation 1 must run the phase-split
kernels of kernels/deconv.hip for both passes (one deconv_bwd_data and one
deconv_bwd_weight record, no GEMM and no im2col in backward); stride 1,
dilation > 1, a window that does not fit LDS and CAFFE_DECONV_BWD=0 keep
im2col + GEMMs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import caffe_amd as ca
import test_deconvolution as fwd
from engine_util import TOL, input_net, net_from_text, relerr
from test_deconvolution import layer_text, pair

GPU = pytest.param("gpu", marks=pytest.mark.gpu)

# id: (N, Ci, Co, group, H, W, kernel, stride, pad, bias, dilation, var)
# var None: both passes are refused and keep im2col + GEMMs.  B1-B9 and B13
# lie outside the direct zone (the MFMA variants lost to that route when
# measured, profiles/deconv.txt, and were cut); their values are checked on it.
BROWS = {
    "B1": (2, 32, 64, 1, 5, 5, 4, 2, 1, True, 1, None),
    # odd Cout/group
    "B2": (2, 8, 7, 1, 5, 5, 3, 2, 1, False, 1, None),
    "B3": (2, 32, 40, 1, 4, 4, 4, 2, 1, False, 1, None),
    # C/group 96 with groups
    "B4": (2, 192, 20, 2, 4, 5, 4, 2, 1, False, 1, None),
    # stride > kernel: five of nine phases have no tap
    "B5": (2, 32, 32, 1, 4, 4, 2, 3, 0, False, 1, None),
    # pad >= stride (dq > 0), odd OH
    "B6": (2, 32, 32, 1, 5, 6, 5, 2, 2, False, 1, None),
    # dq differing between phases
    "B7": (2, 16, 16, 1, 6, 5, (7, 6), (2, 3), (5, 3), False, 1, None),
    "B8": (1, 16, 16, 1, 19, 37, 4, 2, 1, False, 1, None),
    # stride on one axis only (P = 2)
    "B9": (2, 16, 24, 1, 5, 6, (4, 3), (2, 1), (1, 1), False, 1, None),
    # direct<1>, one channel per group; 16 taps shared by 16 threads each
    "B10": (2, 21, 21, 21, 6, 6, 4, 2, 1, False, 1, "direct"),
    # direct<4>, Cout/group 3 and C/group 4; 9 taps: 4 of 256 threads idle
    "B11": (2, 8, 6, 2, 5, 6, 3, 2, 0, True, 1, "direct"),
    # direct, 64 phases, one thread per tap: the bilinear upsampler in small;
    # the window shrinks the tile to 8 rows, so 9 rows are two tiles
    "B12": (1, 3, 3, 3, 9, 3, 16, 8, 4, False, 1, "direct"),
    # 64 phases ungrouped
    "B13": (1, 21, 21, 1, 3, 3, 16, 8, 4, False, 1, None),
    # direct<2>; 2 x 3 ragged cell tiles of 16 x 16; stride > kernel on W and
    # pad >= stride with differing dq on H; wgrad's 42 (image, tile) items go
    # to 21 slices of two
    "B14": (7, 4, 4, 2, 17, 37, (5, 2), (2, 3), (3, 0), False, 1, "direct"),
    # direct<2>, 45 items in 23 slices, the last slice one item; stride on
    # one axis only
    "B15": (5, 4, 2, 2, 33, 40, (4, 3), (2, 1), (1, 1), True, 1, "direct"),
    # k20: 400 taps are two tap passes of 256 threads
    "B16": (1, 2, 2, 2, 9, 5, 20, 4, 8, False, 1, "direct"),
}
fwd.ROWS.update(BROWS)  # case() and layer_text() look rows up there

# what db_plan() of deconv.hip gives, as the records show: (dgrad, wgrad)
PLAN = {
    "B10": ({"tiles_y": 1, "tiles_x": 1, "blocks": 42},
            {"chunks": 1, "slices": 2, "blocks": 42}),
    "B12": ({"phases": 64, "tiles_y": 2, "blocks": 6},
            {"slices": 2, "blocks": 6}),
    "B14": ({"phases": 6, "tiles_y": 2, "tiles_x": 3, "blocks": 84},
            {"chunks": 2, "slices": 21, "blocks": 42}),
    "B15": ({"tiles_y": 3, "tiles_x": 3, "blocks": 90},
            {"chunks": 2, "slices": 23, "blocks": 46}),
    "B16": ({"phases": 16, "tiles_y": 1}, {"slices": 1}),
}


def traced_backward(net):
    """net.backward() with both traces on: (deconv_bwd_* records, GEMMs)"""
    ca.kernel_trace(True)
    ca.gemm_trace(True)
    try:
        net.backward()
    finally:
        ca.kernel_trace(False)
        ca.gemm_trace(False)
    return [k for k in ca.kernel_trace_read()
            if k["op"].startswith("deconv_bwd")], ca.gemm_trace_read()


def run_backward(mode, rid):
    """Forward, NaN in the bottom diff, traced backward: (net, [dx, dW, db],
    records, GEMM records)"""
    x, w, b, dy, _ = fwd.case(rid)
    net = fwd.row_net(mode, rid)
    net.forward()
    net.set_blob("out", dy, diff=True)
    net.set_blob("in0", np.full(x.shape, np.nan, np.float32), diff=True)
    recs, gemms = traced_backward(net)
    got = [net.blob("in0", diff=True), net.param(0, diff=True)]
    return net, got + ([] if b is None else [net.param(1, diff=True)]), \
        recs, gemms


def check_grads(got, ref, names=("dx", "dW", "db")):
    assert len(got) == len(ref)
    for name, a, b in zip(names, got, ref):
        err = relerr(a, b)
        print(name, err)
        assert err < TOL, (name, err)


@pytest.mark.parametrize("mode", ["cpu", GPU])
@pytest.mark.parametrize("rid", list(BROWS))
def test_backward_matches_autograd(rid, mode):
    _, got, recs, gemms = run_backward(mode, rid)
    var = BROWS[rid][11]
    if mode == "gpu" and var is None:
        assert recs == [] and len(gemms) >= 2 * BROWS[rid][3], (recs, gemms)
    elif mode == "gpu":
        assert gemms == []
        assert [k["op"] for k in recs] == ["deconv_bwd_weight",
                                           "deconv_bwd_data"], recs
        assert [k["var"] for k in recs] == [var, var], recs
        for rec, want in zip(recs[::-1], PLAN.get(rid, ({}, {}))):
            assert {k: rec[k] for k in want} == want, rec
    check_grads(got, fwd.case(rid)[4][1:])


@pytest.mark.gpu
def test_wgrad_is_deterministic():
    net, first, _, _ = run_backward("gpu", "B15")
    first = [np.asarray(a).copy() for a in first]
    net.backward()
    again = [net.blob("in0", diff=True), net.param(0, diff=True)]
    for a, b in zip(first, again):
        assert np.array_equal(a, b)


# two stacked layers of the direct zone: up1 packs 64 floats, up2 288
UPS = ((2, 4, 4, 4, 5, 6, 4, 2, 1, True, 1), (2, 4, 8, 2, 10, 12, 3, 2, 0, True, 1))


def two_layer_ref(x, params, dy):
    tx, *tp = (torch.tensor(a, dtype=torch.float64, requires_grad=True)
               for a in [x] + params)
    y = tx
    for i, row in enumerate(UPS):
        y = torch.nn.functional.conv_transpose2d(
            y, tp[2 * i], tp[2 * i + 1], stride=pair(row[7]),
            padding=pair(row[8]), groups=row[3])
    y.backward(torch.tensor(dy, dtype=torch.float64))
    return [tx.grad.numpy()] + [p.grad.numpy() for p in tp]


@pytest.mark.gpu
def test_two_layers_share_the_pack_slots():
    """Backward runs up2 first, so each workspace slot is refilled by the
    smaller layer after the larger one; then new weights without rebuilding"""
    r = np.random.default_rng(78)
    x = r.standard_normal((2, 4, 5, 6)).astype(np.float32)
    dy = r.standard_normal((2, 8, 21, 25)).astype(np.float32)
    sets = [[(r.standard_normal(shape) * 0.3).astype(np.float32)
             for row in UPS
             for shape in ((row[1], row[2] // row[3]) + pair(row[6]),
                           (row[2],))] for _ in range(2)]
    ca.set_mode("gpu")
    net = net_from_text(input_net(
        [x.shape], layer_text(UPS[0], name="up1", top="mid") + "\n" +
        layer_text(UPS[1], name="up2", bottom="mid")))
    net.set_blob("in0", x)
    at = {info[:2]: i for i, info in net.params().items()}
    idx = [at[key] for key in (("up1", 0), ("up1", 1), ("up2", 0), ("up2", 1))]
    refs = [two_layer_ref(x, ps, dy) for ps in sets]
    for ps, want in zip(sets, refs):
        for i, p in zip(idx, ps):
            net.set_param(i, p.ravel())
        net.forward()
        net.set_blob("out", dy, diff=True)
        recs, gemms = traced_backward(net)
        assert [k["op"] for k in recs] == [
            "deconv_bwd_weight", "deconv_bwd_data"] * 2 and gemms == [], recs
        check_grads([net.blob("in0", diff=True)] +
                    [net.param(i, diff=True) for i in idx], want,
                    ("dx", "dW1", "db1", "dW2", "db2"))
    assert relerr(refs[1][0], refs[0][0]) > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ["S1", "D2"])
def test_fallbacks_keep_the_gemm_route(rid):
    _, got, recs, gemms = run_backward("gpu", rid)
    assert recs == [] and len(gemms) >= fwd.ROWS[rid][3], (recs, gemms)
    check_grads(got, fwd.case(rid)[4][1:])


# torch-free (its bundled ROCm runtime must not load after the engine's)
_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {tests!r})
from engine_util import run_layer
import caffe_amd as ca
d = np.load({path!r})
ca.kernel_trace(True)
net, y = run_layer("gpu", [d["x"].shape], {body!r}, [d["x"]],
                   params=[d["w"], d["b"]])
net.set_blob("out", d["dy"], diff=True)
ca.gemm_trace(True)
net.backward()
ops = [k["op"] for k in ca.kernel_trace_read() if "deconv" in k["op"]]
assert ops == ["deconv_fwd"], ops
assert len(ca.gemm_trace_read()) >= 2
np.savez({out!r}, net.blob("in0", diff=True), net.param(0, diff=True),
         net.param(1, diff=True))
"""


@pytest.mark.gpu
def test_env_switch_forces_backward_alone_onto_gemm(tmp_path):
    """CAFFE_DECONV_BWD=0 is read once per process: B11 in a fresh child"""
    x, w, b, dy, ref = fwd.case("B11")
    path, res = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(path, x=x, w=w, b=b, dy=dy)
    code = _CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)),
                         path=path, out=res, body=layer_text(BROWS["B11"]))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True,
                         env=dict(os.environ, CAFFE_DECONV_BWD="0"), text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.load(res)
    check_grads([got[k] for k in got.files], ref[1:])
