"""The join-backward plan (Net.join_backward()) against exact expected lists.

A Split with two propagating tops directly after a ReLU that runs its own
backward, and whose top nothing else reads, takes that ReLU's backward into
its own (one kernel on the GPU).  Like the other build-time plans it is a
function of the built graph and is made in CPU mode too, so none of this
needs a GPU; what the GPU computes with and without it is
tests/test_join_backward_gpu.py.  The expected lists were written from the
rule, not read off the code.
"""
import os
import subprocess
import sys

import pytest

import caffe_amd as ca
from engine_util import REPO, net_from_text
import fusion_graphs as fg
from test_fusion_plan import MODEL_SHAPES


def _conv(name, bottom, top, c):
    return (f'layer {{ name: "{name}" type: "Convolution" bottom: "{bottom}" '
            f'top: "{top}" convolution_param {{ num_output: {c} '
            f'kernel_size: 1 weight_filler {{ type: "gaussian" std: 0.5 }} '
            f'bias_filler {{ type: "gaussian" std: 0.1 }} }} }}')


def join_net(kind, shape=(2, 4, 4, 4), slope=None):
    """Two inputs of `shape` (in0, in1), force_backward, no loss: the caller
    sets the gradient of the last top, "g".  The ReLU is r1; the readers of
    its top are 1x1 convs k1, k2 (k3) whose outputs are summed into g.

    sum_relu        in0 + in1 -> e, ReLU in place, two readers
    conv_relu_out   conv c0(in0) -> a, ReLU a -> f, two readers
    bn_relu         BatchNorm b1(in0) -> b, ReLU in place, two readers
    three_readers   conv_relu_out with three readers
    one_reader      conv_relu_out with one reader
    conv_twice      conv c0(in0) -> a, two readers, no ReLU
    """
    c = shape[1]
    dims = " ".join(f"dim: {d}" for d in shape)
    head = (f'name: "join"\nforce_backward: true\n'
            f'layer {{ name: "input" type: "Input" top: "in0" top: "in1" '
            f'input_param {{ shape {{ {dims} }} shape {{ {dims} }} }} }}')
    if kind == "sum_relu":
        body = [fg.elt("e1", ("in0", "in1"), "e"), fg.relu("r1", "e", "e", slope)]
        out = "e"
    elif kind == "bn_relu":
        body = [fg.bn("b1", "in0", "b"), fg.relu("r1", "b", "b", slope)]
        out = "b"
    elif kind == "conv_twice":
        body = [_conv("c0", "in0", "a", c)]
        out = "a"
    else:
        body = [_conv("c0", "in0", "a", c), fg.relu("r1", "a", "f", slope)]
        out = "f"
    readers = {"three_readers": 3, "one_reader": 1}.get(kind, 2)
    tops = [f"p{i}" for i in range(1, readers + 1)]
    body += [_conv(f"k{i}", out, f"p{i}", c) for i in range(1, readers + 1)]
    if readers > 1:
        body.append(fg.elt("e2", tops, "g"))
    else:
        body.append(fg.split("sp", "p1", "g"))
    return head + "\n" + "\n".join(body) + "\n"


# (kind, slope) -> expected Net.join_backward().  An inserted Split is named
# <blob>_<producer layer>_split.
EXPECTED = {
    ("sum_relu", None): [("e_r1_split", "r1")],
    ("conv_relu_out", None): [("f_r1_split", "r1")],
    ("conv_relu_out", 0.1): [("f_r1_split", "r1")],
    # the BN took the mask into its own backward: r1 launches nothing
    ("bn_relu", None): [],
    ("three_readers", None): [],
    ("one_reader", None): [],
    ("conv_twice", None): [],
}


@pytest.mark.parametrize("kind,slope", list(EXPECTED))
def test_hand_graph(kind, slope):
    ca.set_mode("cpu")
    net = net_from_text(join_net(kind, slope=slope))
    assert net.join_backward() == EXPECTED[(kind, slope)]
    names = net.layer_names()
    for split, relu in net.join_backward():
        assert names.index(split) == names.index(relu) + 1
    # the other two plans do not move with this one
    # (in-place slope-0 ReLUs go into their producer's forward)
    assert net.fusions() == {"bn_relu": [("bn_relu", "b1", ["r1"])],
                             "sum_relu": [("sum_relu", "e1", ["r1"])]
                             }.get(kind, [])
    sharing = [("e2", f"p{i}", "alias")
               for i in range(1, {"three_readers": 4}.get(kind, 3))]
    if kind == "sum_relu":
        # r1 is in place on e and no other bottom of e1 waits below it
        sharing = [("e1", "in0", "alias"), ("e1", "in1", "alias")] + sharing
    if kind == "one_reader":
        sharing = [("sp", "p1", "alias")]
    assert net.diff_sharing() == sharing


@pytest.mark.parametrize("name", list(fg.all_graphs()))
def test_fusion_graphs_hold_no_join(name):
    # no hand graph of the other plans has a two-top Split behind its ReLU,
    # and their plans are what they were
    ca.set_mode("cpu")
    text, phase, fusions = fg.all_graphs()[name]
    net = net_from_text(text, phase=phase)
    assert net.join_backward() == []
    assert net.fusions() == fusions
    assert net.diff_sharing() == fg.DIFF_SHARING[name]


def test_resnet50_has_one_record_per_two_reader_sum_relu():
    path = os.path.join(REPO, "models", "generated",
                        "resnet50_train_val.prototxt")
    if not os.path.exists(path):
        subprocess.check_call([sys.executable,
                               os.path.join(REPO, "models", "gen_models.py")])
    ca.set_mode("cpu")
    ca.set_synthetic_shape(*MODEL_SHAPES["resnet50"])
    net = ca.Net.from_file(path, phase=0, batch_override=2)
    plan = net.join_backward()
    sum_relus = [absorbed[0] for kind, _, absorbed in net.fusions()
                 if kind == "sum_relu"]
    # 16 residual joins; the last one feeds the global pooling alone, so no
    # Split stands behind it and there is nothing to fold: 15 records
    assert len(sum_relus) == 16
    assert [relu for _, relu in plan] == sum_relus[:-1]
    assert len({split for split, _ in plan}) == 15
    assert not any(sum_relus[-1] in name for name in net.layer_names()
                   if name.endswith("_split"))
