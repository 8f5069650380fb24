"""LRN with norm_region WITHIN_CHANNEL against float64 torch:
s = 1 + alpha * avg_pool2d(x^2, k, stride 1, pad pre, count_include_pad),
y = x * s^-beta, dx by autograd against a random top gradient.  In GPU mode
the layer runs kernels/lrn_within.hip; the trace record pins the window
variant and the work split each row reaches.  Every parity row runs at
alpha = 1 on x = 2 N(0, 1), where s averages about 5 and a wrong halo or
divisor is far outside the bound (at a model's alpha = 5e-5 the layer is
nearly the identity).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import caffe_amd as ca
from engine_util import TOL, input_net, net_from_text, relerr

# lrn_within.hip: the tile, the pixels a thread walks, threads and the most
# planes per block, the LDS budget in floats, the largest local_size
TILE_H, TILE_W, SEG, TPB, MAX_PLANES, LDS, MAX_SIZE = (32, 64, 4, 256, 32,
                                                       16384, 41)


def slot_floats(H, W, k):
    """LDS floats of a whole H x W plane; it is tiled when they exceed LDS."""
    th, tw = -(-H // SEG) * SEG, -(-W // SEG) * SEG
    return (th + k - 1) * (((tw + k - 1) | 1) + (tw | 1)) + 2 * th * tw


# the widest plane of TILE_H rows that goes whole at k = 3
LAST_W = max(w for w in range(1, 4 * TILE_W)
             if slot_floats(TILE_H, w, 3) <= LDS)

# id: ((N, C, H, W), local_size, beta, variant, split)
ROWS = {
    # 8 x 8 planes go 16 to a block: 6 planes leave the one block part
    # empty, 18 planes leave 2 to the last block
    "planes_k3": ((2, 3, 8, 8), 3, 0.75, "k3", "planes"),
    "planes_tail": ((2, 9, 8, 8), 3, 0.75, "k3", "planes"),
    "planes_beta": ((2, 9, 8, 8), 3, 1.5, "k3", "planes"),
    # planes narrower than the window
    "narrow_k5": ((1, 2, 2, 3), 5, 0.75, "generic", "planes"),
    "pixel_k3": ((2, 1, 1, 1), 3, 0.75, "k3", "planes"),
    # partial edge tiles on both axes: one row more than two tiles, one
    # column less (a plane of one tile and a bit goes whole)
    "tiles_k5": ((1, 2, 2 * TILE_H + 1, 2 * TILE_W - 1), 5, 0.75, "generic",
                 "tiles"),
    "tiles_k3": ((1, 1, 2 * TILE_H + 1, TILE_W), 3, 0.75, "k3", "tiles"),
    "generic_planes": ((1, 1, 9, 11), 7, 0.75, "generic", "planes"),
    "generic_tiles": ((1, 1, 2 * TILE_H + 3, TILE_W + 5), 7, 0.75, "generic",
                      "tiles"),
    # the largest plane that goes whole, and one column more: its second
    # tile is one column wide
    "last_plane": ((1, 2, TILE_H, LAST_W), 3, 0.75, "k3", "planes"),
    "first_tiled": ((1, 2, TILE_H, LAST_W + 1), 3, 0.75, "k3", "tiles"),
}
ALPHA = 1.0
MODES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture(autouse=True)
def cpu_after():
    yield
    ca.kernel_trace(False)
    ca.set_mode("cpu")


def layer(size, beta=0.75, region="WITHIN_CHANNEL", top="out"):
    return (f'layer {{ name: "norm" type: "LRN" bottom: "in0" top: "{top}" '
            f'lrn_param {{ local_size: {size} alpha: {ALPHA} beta: {beta} '
            f'norm_region: {region} }} }}')


def inputs(name):
    shape = ROWS[name][0]
    r = np.random.default_rng(sorted(ROWS).index(name))
    return ((2 * r.standard_normal(shape)).astype(np.float32),
            r.standard_normal(shape).astype(np.float32))


def reference(x, dy, k, beta):
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    s = 1 + ALPHA * F.avg_pool2d(xt ** 2, k, stride=1, padding=(k - 1) // 2,
                                 count_include_pad=True)
    y = xt * s ** -beta
    y.backward(torch.tensor(dy, dtype=torch.float64))
    return y.detach().numpy(), xt.grad.numpy()


def run(mode, x, dy, k, beta=0.75):
    ca.set_mode(mode)
    net = net_from_text(input_net([x.shape], layer(k, beta)))
    net.set_blob("in0", x)
    net.forward()
    net.set_blob("out", dy, diff=True)
    net.set_blob("in0", np.full(x.shape, np.nan, np.float32), diff=True)
    net.backward()
    return net.blob("out"), net.blob("in0", diff=True)


def planned(shape, k, split):
    """The record fields the plan of lrn_within.hip gives this shape."""
    N, C, H, W = shape
    if split == "tiles":
        ty, tx = -(-H // TILE_H), -(-W // TILE_W)
        return dict(planes=1, tiles_y=ty, tiles_x=tx, blocks=N * C * ty * tx)
    walks = -(-H // SEG) * (-(-W // SEG) * SEG)
    P = min(N * C, max(1, min(MAX_PLANES, TPB // walks)))
    return dict(planes=P, tiles_y=1, tiles_x=1, blocks=-(-N * C // P))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(ROWS))
def test_parity(mode, name):
    shape, k, beta, var, split = ROWS[name]
    assert (slot_floats(*shape[2:], k) > LDS) == (split == "tiles")
    x, dy = inputs(name)
    y_ref, dx_ref = reference(x, dy, k, beta)
    ca.kernel_trace(True)
    y, dx = run(mode, x, dy, k, beta)
    ca.kernel_trace(False)
    print(name, mode, "y err", relerr(y, y_ref), "dx err", relerr(dx, dx_ref))
    assert relerr(y, y_ref) < TOL
    assert relerr(dx, dx_ref) < TOL
    recs = [r for r in ca.kernel_trace_read() if r["op"].startswith("lrn")]
    if mode == "cpu":
        assert recs == []
        return
    plan = planned(shape, k, split)
    assert recs == [dict(op=op, var=var, split=split, **plan)
                    for op in ("lrn_within_fwd", "lrn_within_bwd")]


@pytest.mark.gpu
def test_rerun_is_bit_identical():
    x, dy = inputs("tiles_k5")
    y0, dx0 = run("gpu", x, dy, 5)
    y1, dx1 = run("gpu", x, dy, 5)
    assert np.array_equal(y0, y1) and np.array_equal(dx0, dx1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["planes_k3", "tiles_k5"])
def test_corner_gradient_reaches_its_window_only(mode, name):
    shape, k = ROWS[name][:2]
    x, _ = inputs(name)
    dy = np.zeros(shape, np.float32)
    dy[-1, -1, -1, -1] = 1.0
    _, dx = run(mode, x, dy, k)
    want = np.zeros(shape, bool)
    want[-1, -1, -(k // 2 + 1):, -(k // 2 + 1):] = True
    assert np.array_equal(dx != 0, want)


@pytest.mark.parametrize("body,message", [
    (layer(4), "size_ % 2"),
    (layer(3, top="in0"), "'norm'.*WITHIN_CHANNEL does not run in-place"),
    (layer(MAX_SIZE + 2), f"'norm'.*local_size {MAX_SIZE + 2} is above "
                          f"{MAX_SIZE}"),
])
def test_construction_errors(body, message):
    ca.set_mode("cpu")
    with pytest.raises(ca.CaffeError, match=message):
        net_from_text(input_net([(1, 1, 4, 4)], body))
    net_from_text(input_net([(1, 1, 4, 4)], layer(MAX_SIZE)))


@pytest.mark.gpu
def test_across_channels_keeps_its_kernels():
    ca.set_mode("gpu")
    net = net_from_text(input_net([(2, 8, 6, 6)],
                                  layer(5, region="ACROSS_CHANNELS")))
    ca.kernel_trace(True)
    net.forward()
    ca.kernel_trace(False)
    assert [r["op"] for r in ca.kernel_trace_read()] == ["lrn_fwd"]
