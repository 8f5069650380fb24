"""SoftmaxWithLoss with a loss_param (ignore_label, normalization) against
float64 torch: log_softmax + nll_loss(ignore_index, reduction='sum') over
the hand-computed normalizer, dx by autograd.  In GPU mode the layer runs the
pixel-major kernels of kernels/dense_softmax.hip; the trace record pins the
form and widths each row reaches.  Bounds are check_softmaxloss_spatial's.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import caffe_amd as ca
from engine_util import TOL, input_net, net_from_text, relerr

# id: (N, C, H, W, ignore, loss_param body, normalizer kind, extra layer
#      text, GPU plan (form, CR, P, vec), all labels ignored)
ROWS = {
    # FCN's own setting; inner = 65: one past a wave, scalar accesses
    "fcn": (2, 21, 5, 13, 255, "ignore_label: 255 normalize: false", "batch",
            "", ("resident", 32, 1, 1), False),
    # an in-range ignore label, 16-byte runs
    "ign0": (2, 5, 4, 16, 0, "ignore_label: 0", "valid", "",
             ("resident", 8, 4, 4), False),
    # the last resident width and the first streaming one, 8-byte runs
    "c32": (1, 32, 3, 6, 7, "ignore_label: 7 normalization: FULL", "full", "",
            ("resident", 32, 2, 2), False),
    "c33": (1, 33, 3, 6, 7, "ignore_label: 7 normalization: FULL", "full", "",
            ("stream", 0, 2, 2), False),
    # streaming, several channel chunks, the last one partial
    "c150": (1, 150, 2, 9, 255, "ignore_label: 255 normalization: NONE",
             "none", "", ("stream", 0, 2, 2), False),
    "inner1": (3, 2, 1, 1, 1, "ignore_label: 1 normalization: VALID", "valid",
               "", ("resident", 4, 1, 1), False),
    "c1": (2, 1, 3, 3, None, "normalization: VALID", "valid", "",
           ("resident", 4, 1, 1), False),
    "all_ignored": (1, 3, 2, 4, 2, "ignore_label: 2", "valid", "",
                    ("resident", 4, 4, 4), True),
    "weight": (2, 4, 3, 5, 3, "ignore_label: 3 normalization: VALID", "valid",
               "loss_weight: 2.5", ("resident", 4, 1, 1), False),
    # 513 * 513 pixels, one per thread: one more than the 1024 x 256 grid
    # holds in a pass
    "two_passes": (1, 2, 513, 513, 1, "ignore_label: 1", "valid", "",
                   ("resident", 4, 1, 1), False),
}
MODES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture(autouse=True)
def cpu_after():
    yield
    ca.kernel_trace(False)
    ca.set_mode("cpu")


def layer(body, extra=""):
    lp = f"loss_param {{ {body} }}" if body is not None else ""
    return (f'layer {{ name: "loss" type: "SoftmaxWithLoss" bottom: "in0" '
            f'bottom: "in1" top: "out" {extra} {lp} }}')


def inputs(name):
    N, C, H, W, ign, *_, all_ign = ROWS[name]
    r = np.random.default_rng(sorted(ROWS).index(name))
    x = (r.standard_normal((N, C, H, W)) * 2).astype(np.float32)
    lab = r.integers(0, C, (N, H, W))
    if ign is not None:  # about a quarter of the labels
        lab[r.random((N, H, W)) < (1.0 if all_ign else 0.25)] = ign
    return x, lab


def reference(name, x, lab):
    N, C, H, W, ign, _, kind, extra = ROWS[name][:8]
    lw = 2.5 if extra else 1.0
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    lt = torch.tensor(lab)
    ii = -100 if ign is None else ign
    total = F.nll_loss(F.log_softmax(xt, 1), lt, ignore_index=ii,
                       reduction="sum")
    valid = int((lab != ign).sum()) if ign is not None else lab.size
    norm = max(1, {"full": N * H * W, "valid": valid, "batch": N,
                   "none": 1}[kind])
    loss = total / norm
    (loss * lw).backward()
    return loss.item(), xt.grad.numpy()


def run(mode, name, x, lab):
    ca.set_mode(mode)
    _, _, _, _, _, body, _, extra = ROWS[name][:8]
    net = net_from_text(input_net([x.shape, lab.shape], layer(body, extra)))
    net.set_blob("in0", x)
    net.set_blob("in1", lab.astype(np.float32))
    net.forward()
    net.set_blob("in0", np.full(x.shape, np.nan, np.float32), diff=True)
    net.backward()
    return float(net.blob("out").ravel()[0]), net.blob("in0", diff=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(ROWS))
def test_loss_and_gradient(mode, name):
    x, lab = inputs(name)
    loss_ref, dx_ref = reference(name, x, lab)
    ca.kernel_trace(True)
    loss, dx = run(mode, name, x, lab)
    ca.kernel_trace(False)
    print(name, mode, "loss", loss, "ref", loss_ref, "dx err",
          relerr(dx, dx_ref))
    assert abs(loss - loss_ref) < 1e-5 * max(1, abs(loss_ref))
    assert relerr(dx, dx_ref) < TOL
    ign = ROWS[name][4]
    if ign is not None:  # exact zeros, every channel of an ignored pixel
        assert not dx[np.broadcast_to((lab == ign)[:, None], dx.shape)].any()
    if ROWS[name][9]:
        assert loss == 0.0 and not dx.any()
    recs = [r for r in ca.kernel_trace_read() if r["op"].startswith("dsm_")]
    if mode == "cpu":
        assert recs == []
        return
    form, CR, P, vec = ROWS[name][8]
    rows = lab.size
    blocks = min(-(-(rows // P) // 256), 1024)
    assert recs == [dict(op=op, form=form, CR=CR, P=P, vec=vec, rows=rows,
                         C=x.shape[1], blocks=blocks)
                    for op in ("dsm_fwd", "dsm_bwd")]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fcn", "c150"])
def test_rerun_is_bit_identical(name):
    x, lab = inputs(name)
    loss0, dx0 = run("gpu", name, x, lab)
    loss1, dx1 = run("gpu", name, x, lab)
    assert loss0 == loss1 and np.array_equal(dx0, dx1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["fcn", "c33"])
@pytest.mark.parametrize("value,ignored,want_nan", [
    (np.nan, False, True), (np.inf, False, True),
    (np.nan, True, False), (np.inf, True, False), (-np.inf, False, False)])
def test_non_finite_logits(mode, name, value, ignored, want_nan):
    """NaN and +inf contaminate their pixel's row and so the loss, unless
    the pixel is ignored; -inf is benign (channel 1, the label is 0)."""
    x, lab = inputs(name)
    lab[0, 1, 2] = ROWS[name][4] if ignored else 0
    x[0, 1, 1, 2] = value
    loss, dx = run(mode, name, x, lab)
    assert np.isnan(loss) == want_nan
    if not want_nan:
        px = np.zeros(lab.shape, bool)
        px[0, 1, 2] = True
        others = ~np.broadcast_to(px[:, None], dx.shape)
        x[0, 1, 1, 2] = -1e30 if value == -np.inf else 0.0
        assert relerr(dx[others], reference(name, x, lab)[1][others]) < TOL
        assert np.isfinite(dx[0, :, 1, 2]).all()


def test_out_of_range_label_is_an_error_on_the_cpu():
    x, lab = inputs("ign0")
    lab[1, 2, 3] = 5
    with pytest.raises(ca.CaffeError, match=r"'loss'.*label 5.*\[0, 5\)"):
        run("cpu", "ign0", x, lab)


@pytest.mark.gpu
def test_out_of_range_label_is_a_nan_loss_on_the_gpu():
    x, lab = inputs("ign0")
    lab[1, 2, 3] = 5
    loss, _ = run("gpu", "ign0", x, lab)
    assert np.isnan(loss)


def test_unknown_normalization_names_the_layer():
    ca.set_mode("cpu")
    with pytest.raises(ca.CaffeError, match="'loss'.*normalization 'SOME'"):
        net_from_text(input_net([(2, 3), (2,)],
                                layer("normalization: SOME")))


@pytest.mark.gpu
def test_layer_without_loss_param_keeps_the_class_per_row_kernels():
    ca.set_mode("gpu")
    net = net_from_text(input_net([(2, 3, 65, 65), (2, 65, 65)], layer(None)))
    r = np.random.default_rng(5)
    net.set_blob("in0", r.standard_normal((2, 3, 65, 65)).astype(np.float32))
    net.set_blob("in1", r.integers(0, 3, (2, 65, 65)).astype(np.float32))
    ca.kernel_trace(True)
    net.forward()
    net.backward()
    ca.kernel_trace(False)
    ops = [rec["op"] for rec in ca.kernel_trace_read()]
    assert "softmax_fwd" in ops and not [o for o in ops if "dsm" in o]
