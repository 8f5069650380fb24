"""Crop (reference layers/crop_layer.cpp): forward and backward against numpy
slicing, both exact (the layer only moves floats); the construction errors;
and the FCN head end to end (Convolution -> Deconvolution -> Crop ->
SoftmaxWithLoss with an ignore label) against a float64 torch replay.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import caffe_amd as ca
from engine_util import TOL, input_net, net_from_text, relerr

# (bottom 0 shape, bottom 1 shape, crop_param body, the window as slices)
CASES = [
    ((2, 3, 10, 12), (2, 5, 6, 8), "axis: 2 offset: 4",       # float4 packs
     np.s_[:, :, 4:10, 4:12]),
    ((2, 3, 9, 11), (1, 1, 5, 6), "axis: 2 offset: 3 offset: 2",
     np.s_[:, :, 3:8, 2:8]),
    ((2, 5, 7, 6), (9, 2, 4, 3), "axis: 1 offset: 2 offset: 0 offset: 3",
     np.s_[:, 2:4, 0:4, 3:6]),
    ((2, 3, 4, 9), (7, 7, 7, 5), "axis: -1 offset: 1", np.s_[:, :, :, 1:6]),
    ((2, 3, 4, 8), (2, 3, 4, 8), "offset: 0", np.s_[:, :, :, :]),
]
MODES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture(autouse=True)
def cpu_after():
    yield
    ca.kernel_trace(False)
    ca.set_mode("cpu")


def crop_layer(body, b0="in0", b1="in1"):
    return (f'layer {{ name: "cr" type: "Crop" bottom: "{b0}" bottom: "{b1}" '
            f'top: "out" crop_param {{ {body} }} }}')


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("s0,s1,body,win", CASES)
def test_crop_forward_backward(mode, s0, s1, body, win):
    ca.set_mode(mode)
    net = net_from_text(input_net([s0, s1], crop_layer(body)))
    rng = np.random.default_rng(sum(s0))
    x = rng.standard_normal(s0).astype(np.float32)
    net.set_blob("in0", x)
    net.forward()
    assert net.blob_shape("out") == x[win].shape
    assert np.array_equal(net.blob("out"), x[win])
    dy = rng.standard_normal(x[win].shape).astype(np.float32)
    mark = rng.standard_normal(s1).astype(np.float32)
    net.set_blob("out", dy, diff=True)
    net.set_blob("in0", np.full(s0, np.nan, np.float32), diff=True)
    net.set_blob("in1", mark, diff=True)
    net.backward()
    want = np.zeros(s0, np.float32)
    want[win] = dy
    assert np.array_equal(net.blob("in0", diff=True), want)
    assert np.array_equal(net.blob("in1", diff=True), mark)


@pytest.mark.parametrize("s0,s1,body,needle", [
    ((2, 3, 9, 11), (2, 3, 5, 6), "axis: 1 offset: 1 offset: 2",
     "offset values"),
    ((2, 3, 9, 11), (2, 3, 5, 6), "axis: 2 offset: 5", "leaves axis 2"),
    ((2, 3, 9, 11), (2, 3, 5, 12), "axis: 2", "leaves axis 3"),
    ((2, 3, 9, 11), (2, 3, 5, 6), "axis: 4", "out of range"),
    ((2, 3, 9, 11), (2, 3, 5, 6), "axis: -5", "out of range"),
])
def test_crop_errors_name_the_layer(s0, s1, body, needle):
    ca.set_mode("cpu")
    with pytest.raises(ca.CaffeError) as e:
        net_from_text(input_net([s0, s1], crop_layer(body)))
    assert "'cr'" in str(e.value) and needle in str(e.value), str(e.value)


FCN_HEAD = f"""name: "fcn_head"
layer {{ name: "input" type: "Input" top: "data" top: "label"
  input_param {{ shape {{ dim: 2 dim: 3 dim: 9 dim: 11 }}
                shape {{ dim: 2 dim: 9 dim: 11 }} }} }}
layer {{ name: "score" type: "Convolution" bottom: "data" top: "score"
  convolution_param {{ num_output: 4 kernel_size: 3
    weight_filler {{ type: "gaussian" std: 0.3 }} }} }}
layer {{ name: "up" type: "Deconvolution" bottom: "score" top: "up"
  param {{ lr_mult: 0 }}
  convolution_param {{ num_output: 4 group: 4 kernel_size: 4 stride: 2
    bias_term: false weight_filler {{ type: "bilinear" }} }} }}
{crop_layer("axis: 2 offset: 3", "up", "data")}
layer {{ name: "loss" type: "SoftmaxWithLoss" bottom: "out" bottom: "label"
  top: "loss" loss_param {{ ignore_label: 255 normalize: false }} }}
"""


@pytest.mark.parametrize("mode", MODES)
def test_fcn_head_end_to_end(mode):
    ca.set_mode(mode)
    ca.kernel_trace(True)
    net = net_from_text(FCN_HEAD)
    rng = np.random.default_rng(911)
    x = rng.standard_normal((2, 3, 9, 11)).astype(np.float32)
    lab = rng.integers(0, 4, (2, 9, 11))
    lab[rng.random(lab.shape) < 0.25] = 255
    net.set_blob("data", x)
    net.set_blob("label", lab.astype(np.float32))
    net.forward()
    net.backward()
    ca.kernel_trace(False)
    par = {net.param_info(i)[:2]: i for i in range(net.num_params())}
    w, b, wu = (torch.tensor(net.param(par[k]), dtype=torch.float64)
                for k in (("score", 0), ("score", 1), ("up", 0)))
    w = w.reshape(4, 3, 3, 3).requires_grad_()
    up = F.conv_transpose2d(
        F.conv2d(torch.tensor(x, dtype=torch.float64), w, b),
        wu.reshape(4, 1, 4, 4), stride=2, groups=4)
    loss = F.nll_loss(F.log_softmax(up[:, :, 3:12, 3:14], 1),
                      torch.tensor(lab), ignore_index=255,
                      reduction="sum") / 2
    loss.backward()
    assert abs(net.loss() - loss.item()) < 1e-5 * max(1, abs(loss.item()))
    assert relerr(net.param(par[("score", 0)], diff=True), w.grad) < TOL
    if mode == "gpu":  # the direct deconvolution route and the dense loss
        recs = {r["op"]: r for r in ca.kernel_trace_read()}
        assert recs["deconv_fwd"]["var"] == "direct"
        assert recs["deconv_bwd_data"]["var"] == "direct"
        assert recs["dsm_fwd"]["form"] == "resident"
