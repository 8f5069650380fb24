"""Slice (reference layers/slice_layer.cpp): forward against numpy slicing,
backward against the concatenation of the top diffs, both exact (the layer
only moves floats), the construction errors, and that a Data-fed Slice
launches nothing in the GPU backward.
"""
import numpy as np
import pytest

import caffe_amd as ca
from engine_util import input_net, net_from_text

# (bottom shape, slice_param body, axis, cut points along that axis)
CASES = [
    ((2, 2, 3, 3), "axis: 1 slice_point: 1", 1, [1]),      # the siamese cut
    ((3, 7, 1, 5), "axis: 1 slice_point: 2 slice_point: 3", 1, [2, 3]),
    ((4, 6, 2, 2), "", 1, [2, 4]),                         # no points, 3 tops
    ((6, 3), "axis: 0 slice_point: 4", 0, [4]),
    ((2, 3, 4, 5), "axis: -1 slice_point: 1", 3, [1]),     # inner = 1
]
MODES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]


def slice_layer(body, ntops, bottom="in0"):
    tops = " ".join(f'top: "t{i}"' for i in range(ntops))
    return (f'layer {{ name: "sl" type: "Slice" bottom: "{bottom}" {tops} '
            f'slice_param {{ {body} }} }}')


@pytest.fixture(autouse=True)
def cpu_after():
    yield
    ca.set_mode("cpu")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,body,axis,cuts", CASES)
def test_slice_forward_backward(mode, shape, body, axis, cuts):
    ca.set_mode(mode)
    ntops = len(cuts) + 1
    # force_backward on an Input-fed net: the bottom propagates
    net = net_from_text(input_net([shape], slice_layer(body, ntops)))
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(np.float32)
    net.set_blob("in0", x)
    net.forward()
    want = np.split(x, cuts, axis=axis)
    diffs = []
    for i, w in enumerate(want):
        assert net.blob_shape(f"t{i}") == w.shape
        assert np.array_equal(net.blob(f"t{i}"), w), i
        d = rng.standard_normal(w.shape).astype(np.float32)  # one per top
        net.set_blob(f"t{i}", d, diff=True)
        diffs.append(d)
    net.backward()
    assert np.array_equal(net.blob("in0", diff=True),
                          np.concatenate(diffs, axis=axis))


@pytest.mark.parametrize("mode", MODES)
def test_slice_backward_under_inner_product(mode):
    """The bottom is an InnerProduct's top, so it propagates without
    force_backward; the IP's bias gradient is the column sum of the Slice's
    bottom diff, which pins that diff: exact for the 0/1 values used."""
    ca.set_mode(mode)
    text = f"""name: "s"
layer {{ name: "input" type: "Input" top: "in0"
  input_param {{ shape {{ dim: 6 dim: 4 }} }} }}
layer {{ name: "ip" type: "InnerProduct" bottom: "in0" top: "fc"
  inner_product_param {{ num_output: 3
    weight_filler {{ type: "gaussian" std: 0.5 }} }} }}
{slice_layer("axis: 0 slice_point: 4", 2, bottom="fc")}
"""
    net = net_from_text(text)
    net.set_blob("in0", np.ones((6, 4), np.float32))
    net.forward()
    fc = net.blob("fc")
    assert np.array_equal(net.blob("t0"), fc[:4])
    assert np.array_equal(net.blob("t1"), fc[4:])
    d0 = np.arange(12, dtype=np.float32).reshape(4, 3)
    d1 = -np.arange(6, dtype=np.float32).reshape(2, 3)
    net.set_blob("t0", d0, diff=True)
    net.set_blob("t1", d1, diff=True)
    net.backward()
    assert np.array_equal(net.blob("fc", diff=True), np.concatenate([d0, d1]))
    bias = [i for i in range(net.num_params())
            if net.param_info(i)[:2] == ("ip", 1)][0]
    assert np.array_equal(net.param(bias, diff=True),
                          np.concatenate([d0, d1]).sum(0))


def test_one_top_slice_copies_and_is_not_diff_shared():
    ca.set_mode("cpu")
    net = net_from_text(input_net([(2, 3)], slice_layer("axis: 1", 1)))
    x = np.arange(6, dtype=np.float32).reshape(2, 3)
    net.set_blob("in0", x)
    net.forward()
    assert np.array_equal(net.blob("t0"), x)
    assert net.diff_sharing() == []


@pytest.mark.parametrize("shape,body,ntops,needle", [
    ((2, 6), "axis: 1 slice_point: 3 slice_point: 3", 3, "increasing"),
    ((2, 6), "axis: 1 slice_point: 4 slice_point: 2", 3, "increasing"),
    ((2, 6), "axis: 1 slice_point: 6", 2, "outside"),
    ((2, 6), "axis: 1 slice_point: 9", 2, "outside"),
    ((2, 6), "axis: 1 slice_point: 2", 3, "slice_point entries"),
    ((2, 6), "axis: 1 slice_point: 2 slice_point: 4", 2,
     "slice_point entries"),
    ((2, 7), "axis: 1", 2, "evenly divide"),
    ((2, 6), "axis: 2", 2, "out of range"),
    ((2, 6), "axis: 1 slice_dim: 1", 2, "not both"),
])
def test_slice_errors_name_the_layer(shape, body, ntops, needle):
    ca.set_mode("cpu")
    with pytest.raises(ca.CaffeError) as e:
        net_from_text(input_net([shape], slice_layer(body, ntops)))
    assert "'sl'" in str(e.value) and needle in str(e.value), str(e.value)


def test_slice_needs_a_bottom_and_a_top():
    ca.set_mode("cpu")
    with pytest.raises(ca.CaffeError) as e:
        net_from_text(input_net(
            [(2, 6)], 'layer { name: "sl" type: "Slice" bottom: "in0" }'))
    assert "'sl'" in str(e.value) and "top blob" in str(e.value)


@pytest.mark.gpu
def test_data_fed_slice_launches_nothing_in_backward():
    """The siamese form: the bottom is a Data top, which takes no gradient.
    Slice copies through the `concat` kernel class: two launches in the
    forward (one per top), none in the backward."""
    ca.set_mode("gpu")
    ca.set_synthetic_shape(2, 6, 6, 2)
    text = """name: "s"
layer { name: "pair" type: "Data" top: "pair" top: "sim"
  data_param { batch_size: 4 } }
layer { name: "sl" type: "Slice" bottom: "pair" top: "d0" top: "d1"
  slice_param { slice_dim: 1 slice_point: 1 } }
layer { name: "f0" type: "InnerProduct" bottom: "d0" top: "f0"
  inner_product_param { num_output: 2 weight_filler { type: "xavier" } } }
layer { name: "f1" type: "InnerProduct" bottom: "d1" top: "f1"
  inner_product_param { num_output: 2 weight_filler { type: "xavier" } } }
layer { name: "loss" type: "ContrastiveLoss" bottom: "f0" bottom: "f1"
  bottom: "sim" top: "loss" }
"""
    net = net_from_text(text)
    ca.perf_reset()
    net.forward()
    ca.device_synchronize()
    assert ca.perf_snapshot()["concat"]["launches"] == 2
    pair = net.blob("pair")
    assert np.array_equal(net.blob("d0"), pair[:, :1])
    assert np.array_equal(net.blob("d1"), pair[:, 1:])
    net.backward()
    ca.device_synchronize()
    assert ca.perf_snapshot()["concat"]["launches"] == 2
    assert np.isfinite(net.loss())
