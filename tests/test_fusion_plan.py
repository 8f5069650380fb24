"""The graph-fusion plan (Net.fusions()) against exact expected lists.

The plan is a function of the built graph and is made in CPU mode too, so
none of this needs a GPU.  Every expected value was read off the two fusion
passes Net::init held before they became a plan (commit b1ffb37) and
confirmed by dumping that commit's layer flags after init; the dump is
profiles/net_build_passes.txt, section (a).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import caffe_amd as ca
from engine_util import REPO, net_from_text
import fusion_graphs as fg


@pytest.mark.parametrize("name", list(fg.POSITIVE))
def test_positive_graph(name):
    ca.set_mode("cpu")
    text, phase, expected = fg.POSITIVE[name]
    assert net_from_text(text, phase=phase).fusions() == expected


@pytest.mark.parametrize("name", list(fg.NEGATIVE))
def test_negative_graph(name):
    """Each graph differs from a positive one in one property and loses
    exactly the fusion that property carries.  (`prod` builds in CPU mode
    only: Eltwise PROD has no GPU kernel and is an error there.)"""
    ca.set_mode("cpu")
    base, text, phase, expected = fg.NEGATIVE[name]
    got = net_from_text(text, phase=phase).fusions()
    assert got == expected
    # nothing the positive graph did not have
    assert all(f in fg.POSITIVE[base][2] or f[0] == "bn_add" for f in got)
    assert got != fg.POSITIVE[base][2]


# fusions per kind of the generated models at batch 2; the same numbers as
# the flag dump of commit b1ffb37
MODEL_FUSIONS = {
    ("lenet", 0): {}, ("lenet", 1): {},
    ("alexnet", 0): {"conv_relu": 5}, ("alexnet", 1): {"conv_relu": 5},
    ("googlenet", 0): {"conv_relu": 59}, ("googlenet", 1): {"conv_relu": 59},
    ("resnet50", 0): {"bn_relu": 33, "bn_add": 16, "sum_relu": 16},
    ("resnet50", 1): {"bn_relu": 33, "sum_relu": 16},
}
MODEL_SHAPES = {"lenet": (1, 28, 28, 10), "alexnet": (3, 227, 227, 1000),
                "googlenet": (3, 224, 224, 1000),
                "resnet50": (3, 224, 224, 1000)}


@pytest.mark.parametrize("model,phase", list(MODEL_FUSIONS))
def test_generated_model(model, phase):
    path = os.path.join(REPO, "models", "generated",
                        f"{model}_train_val.prototxt")
    if not os.path.exists(path):
        subprocess.check_call([sys.executable,
                               os.path.join(REPO, "models", "gen_models.py")])
    ca.set_mode("cpu")
    ca.set_synthetic_shape(*MODEL_SHAPES[model])
    net = ca.Net.from_file(path, phase=phase, batch_override=2)
    fusions = net.fusions()
    counts = {}
    for kind, _, _ in fusions:
        counts[kind] = counts.get(kind, 0) + 1
    assert counts == MODEL_FUSIONS[model, phase]
    _check_plan_shape(net, fusions)


def _check_plan_shape(net, fusions):
    names = net.layer_names()
    producers = [names.index(p) for _, p, _ in fusions]
    assert producers == sorted(set(producers))  # layer order, one each
    # no layer is absorbed twice -- in particular no ReLU is applied by two
    # producers
    absorbed = [a for _, _, ab in fusions for a in ab]
    assert len(absorbed) == len(set(absorbed))
    for _, p, ab in fusions:
        assert [names.index(a) for a in ab] == list(
            range(names.index(p) + 1, names.index(p) + 1 + len(ab)))


@pytest.mark.parametrize("name", list(fg.POSITIVE) + list(fg.NEGATIVE))
def test_hand_graph_plan_shape(name):
    ca.set_mode("cpu")
    text, phase = (fg.POSITIVE.get(name) or fg.NEGATIVE[name][1:])[:2]
    net = net_from_text(text, phase=phase)
    _check_plan_shape(net, net.fusions())


def _run_cpu(text, x, labels, params=None):
    ca.set_mode("cpu")
    ca.set_random_seed(7)
    net = net_from_text(text)
    if params is not None:
        for i in range(net.num_params()):
            layer, blob_idx, _ = net.param_info(i)
            net.set_param(i, params[layer, blob_idx])
    net.set_blob("in0", x)
    net.set_blob("in1", labels)
    net.forward()
    net.backward()
    own = {net.param_info(i)[:2]: net.param(i)
           for i in range(net.num_params())}
    return (float(np.asarray(net.blob("loss")).ravel()[0]),
            np.asarray(net.blob("in0", diff=True)).copy(), own, net)


@pytest.mark.parametrize("name", list(fg.POSITIVE))
def test_cpu_results_do_not_depend_on_the_plan(name):
    """CPU mode plans but applies nothing: a graph with fusions planned
    gives the loss and the input gradient of the same layers arranged so
    that nothing can be planned (every ReLU out of place, the shortcut conv
    between the BN and the sum), weights copied over by name.  The two run
    the same CPU layer code on the same values, so they agree exactly."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(fg.SHAPE).astype(np.float32)
    labels = rng.integers(0, 4, fg.SHAPE[0]).astype(np.float32)
    loss, dx, params, net = _run_cpu(fg.POSITIVE[name][0], x, labels)
    assert net.fusions() == fg.POSITIVE[name][2] != []
    tloss, tdx, _, twin = _run_cpu(fg.UNFUSED_TWIN[name], x, labels, params)
    assert twin.fusions() == []
    assert np.isfinite(loss) and np.abs(dx).max() > 0
    assert tloss == loss
    assert np.array_equal(tdx, dx)
