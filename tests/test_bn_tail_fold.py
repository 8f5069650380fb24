"""BatchNorm with the moving average folded into the forward finalize.

The TRAIN forward is statistics -> finalize -> norm; the finalize kernel
also advances the global mean / var (it used to be a launch of its own after
the norm).  Checked here: forward and backward against the oracle at the
shapes that take each statistics path, repeated rounds on one layer object
giving the same bits every time, and the global statistics following the
recurrence exactly: a copy of the batch statistics for the first two
forwards, then g = (1 - maf) * batch + maf * g in float32, two products and
one sum (numpy does not fuse them, and neither may the kernel).
"""
import os
import tempfile

import numpy as np
import pytest

import caffe_amd as ca
from engine_util import input_net, net_from_text
from layer_checks import check_bn
from test_param_sharing import layer_blobs

# N, C, H, W -> batch slices per channel nb = max(1, min(N, 2048 // C))
SHAPES = {
    "nb5_scalar": (5, 3, 3, 3),      # S = 9: scalar loads
    "nb1_wide_v4": (2, 1100, 2, 2),  # C beyond one block's threads, float4
    "nb3_s1": (4, 600, 1, 1),
}
MAF = 0.9


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forward_backward_vs_oracle(shape):
    N, C, H, W = SHAPES[shape]
    errs = {}
    check_bn("gpu", N=N, C=C, H=H, W=W, seed=3, errs=errs)
    print(shape, errs)


def _inputs(shape):
    rng = np.random.default_rng(9)
    x = (rng.standard_normal(shape) * 2 + 0.5).astype(np.float32)
    x2 = (rng.standard_normal(shape) * 3 - 1.5).astype(np.float32)
    return x, x2, rng.standard_normal(shape).astype(np.float32)


def _rounds(mode, shape, xs):
    """One forward / backward pass of one BatchNorm layer object per input
    in xs; per round (y, dx, dscale, dbias, global mean, global var)."""
    dy = _inputs(shape)[2]
    body = f"""layer {{
  name: "bn"
  type: "BatchNorm"
  bottom: "in0"
  top: "out"
  batch_norm_param {{ moving_average_fraction: {MAF} scale_bias: true }}
}}"""
    ca.set_mode(mode)
    ca.set_random_seed(4)
    net = net_from_text(input_net([shape], body))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bn.caffemodel")
        for x in xs:
            net.set_blob("in0", x)
            net.forward()
            y = net.blob("out").copy()
            net.set_blob("out", dy, diff=True)
            net.backward()
            net.save_weights(path)
            blobs = layer_blobs(path)["bn"]
            out.append((y, net.blob("in0", diff=True).copy(),
                        net.param(0, diff=True).copy(),
                        net.param(1, diff=True).copy(),
                        blobs[0][1].copy(), blobs[1][1].copy()))
    return out


def _check_rounds(mode, shape):
    x, x2, _ = _inputs(shape)
    out = _rounds(mode, shape, [x, x, x, x2])
    # the layer's own statistics of x2: what a fresh layer copies
    fresh = _rounds(mode, shape, [x2])[0]
    for r in (1, 2):
        for a, b in zip(out[0][:4], out[r][:4]):
            assert np.array_equal(a, b), f"round {r + 1}"
    # the first two forwards copy the batch statistics: the layer's own
    # mean / var, the same every round
    mean, var = out[0][4], out[0][5]
    ref = x.astype(np.float64)
    assert np.allclose(mean, ref.mean(axis=(0, 2, 3)), rtol=1e-5, atol=1e-6)
    assert np.allclose(var, ref.var(axis=(0, 2, 3)), rtol=1e-4, atol=1e-6)
    assert np.array_equal(out[1][4], mean) and np.array_equal(out[1][5], var)
    maf = np.float32(MAF)
    gm, gv = mean, var
    for r, (m, v) in ((2, (mean, var)), (3, (fresh[4], fresh[5]))):
        gm = (np.float32(1) - maf) * m + maf * gm
        gv = (np.float32(1) - maf) * v + maf * gv
        assert gm.dtype == np.float32
        assert np.array_equal(out[r][4], gm), f"global mean, round {r + 1}"
        assert np.array_equal(out[r][5], gv), f"global var, round {r + 1}"
    # the last round mixed two different statistics
    assert not np.array_equal(out[3][4], mean)
    assert not np.array_equal(out[3][4], fresh[4])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_repeat_rounds_and_moving_average_gpu(shape):
    _check_rounds("gpu", SHAPES[shape])


def test_moving_average_cpu():
    _check_rounds("cpu", SHAPES["nb5_scalar"])


@pytest.mark.gpu
def test_scale_backward_c3():
    # Scale's backward shares the BN backward statistics kernels
    from engine_util import TOL, relerr, run_layer
    shape = (5, 3, 3, 3)
    rng = np.random.default_rng(12)
    x = rng.standard_normal(shape).astype(np.float32)
    sc = (1 + 0.3 * rng.standard_normal(3)).astype(np.float32)
    bi = (0.2 * rng.standard_normal(3)).astype(np.float32)
    dy = rng.standard_normal(shape).astype(np.float32)
    body = """layer { name: "s" type: "Scale" bottom: "in0" top: "out"
  scale_param { bias_term: true } }"""
    net, _ = run_layer("gpu", [shape], body, [x], params=[sc, bi],
                       top_diff=dy)
    scv = sc[None, :, None, None]
    assert relerr(net.blob("in0", diff=True), dy * scv) < TOL
    assert relerr(net.param(0, diff=True),
                  (dy.astype(np.float64) * x).sum(axis=(0, 2, 3))) < TOL
    assert relerr(net.param(1, diff=True),
                  dy.astype(np.float64).sum(axis=(0, 2, 3))) < TOL
