"""The gradient-buffer sharing plan (Net.diff_sharing()) against exact
expected lists.

Like the fusion plan it is a function of the built graph and is made in CPU
mode too, so none of this needs a GPU.  The expected lists of the hand
graphs (fusion_graphs.DIFF_SHARING) were written from the rule, not read
off the code; what the GPU launches and computes for the same graphs is
tests/test_gpu_graph_fuzz.py.
"""
import os
import subprocess
import sys

import pytest

import caffe_amd as ca
from engine_util import REPO, net_from_text
import fusion_graphs as fg
from test_fusion_plan import MODEL_SHAPES

GRAPHS = fg.all_graphs()


def test_every_graph_has_an_expected_plan():
    assert set(GRAPHS) == set(fg.DIFF_SHARING)


def _check_plan_shape(net, plan):
    names = net.layer_names()
    # layer order, and at most one entry per layer and bottom
    where = [(names.index(layer), bottom) for layer, bottom, _ in plan]
    assert [w[0] for w in where] == sorted(w[0] for w in where)
    assert len(where) == len(set(where))
    assert all(d in ("alias", "copy") for _, _, d in plan)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_hand_graph(name):
    ca.set_mode("cpu")
    text, phase, fusions = GRAPHS[name]
    net = net_from_text(text, phase=phase)
    assert net.fusions() == fusions
    plan = net.diff_sharing()
    assert plan == fg.DIFF_SHARING[name]
    _check_plan_shape(net, plan)


@pytest.mark.parametrize("name", ["coeff_half", "prod"])
def test_no_entry_for_a_non_unit_sum(name):
    # e1 is the only sum of these graphs, and nothing else is planned
    ca.set_mode("cpu")
    text, phase, _ = GRAPHS[name]
    assert net_from_text(text, phase=phase).diff_sharing() == []


# ResNet-50 has 16 residual sums of two bottoms each; both bottoms of every
# sum come after the first convolution, so all 32 propagate, in TEST as in
# TRAIN (the flags follow the learnable layers, not the phase).  Every
# BatchNorm of the generated prototxt is out of place and no ReLU is in
# place on a sum's bottom, so nothing is copied.  The other models hold no
# Eltwise, and no net gets a one-top Split unless its prototxt writes one.
MODEL_ALIASES = {"lenet": 0, "alexnet": 0, "googlenet": 0, "resnet50": 2 * 16}


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("model", list(MODEL_ALIASES))
def test_generated_model(model, phase):
    path = os.path.join(REPO, "models", "generated",
                        f"{model}_train_val.prototxt")
    if not os.path.exists(path):
        subprocess.check_call([sys.executable,
                               os.path.join(REPO, "models", "gen_models.py")])
    ca.set_mode("cpu")
    ca.set_synthetic_shape(*MODEL_SHAPES[model])
    net = ca.Net.from_file(path, phase=phase, batch_override=2)
    plan = net.diff_sharing()
    assert [d for _, _, d in plan] == ["alias"] * MODEL_ALIASES[model]
    _check_plan_shape(net, plan)
    if model == "resnet50":
        sums = [layer for layer, _, _ in plan]
        assert len(set(sums)) == 16
        assert all(sums.count(layer) == 2 for layer in sums)
