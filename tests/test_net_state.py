"""Net state (phase, level, stages) against include / exclude rules — the
reference's Net::FilterNet / StateMeetsRule (net.cpp:407-499) — and the
solver's test_state / test_iter handling.  CPU mode."""
import os

import numpy as np
import pytest

import caffe_amd as ca

TRAIN, TEST = 0, 1


@pytest.fixture(autouse=True)
def cpu_mode():
    ca.set_mode("cpu")
    ca.set_synthetic_shape(1, 6, 6, 10)
    ca.set_data_iter(0)
    yield
    ca.set_data_iter(0)


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


# one ReLU per rule, on an Input: the top's name says which rule it carries
RULES = {
    "always": "",
    "inc_train": "include { phase: TRAIN }",
    "inc_test": "include { phase: TEST }",
    "inc_stage_a": 'include { stage: "a" }',
    "inc_stage_ab": 'include { stage: "a" stage: "b" }',
    "inc_not_a": 'include { not_stage: "a" }',
    "inc_test_a_not_b": 'include { phase: TEST stage: "a" not_stage: "b" }',
    "inc_min2": "include { min_level: 2 }",
    "inc_max1": "include { max_level: 1 }",
    "inc_1to2": "include { min_level: 1 max_level: 2 }",
    "inc_a_or_min3": 'include { stage: "a" } include { min_level: 3 }',
    "exc_test": "exclude { phase: TEST }",
    "exc_stage_a": 'exclude { stage: "a" }',
    "exc_a_or_max0": 'exclude { stage: "a" } exclude { max_level: 0 }',
    "exc_train_not_b": 'exclude { phase: TRAIN not_stage: "b" }',
}


def expect(rule, phase, level, stages):
    """The table, written out rule by rule (not through a rule evaluator)."""
    a, b = "a" in stages, "b" in stages
    return {
        "always": True,
        "inc_train": phase == TRAIN,
        "inc_test": phase == TEST,
        "inc_stage_a": a,
        "inc_stage_ab": a and b,
        "inc_not_a": not a,
        "inc_test_a_not_b": phase == TEST and a and not b,
        "inc_min2": level >= 2,
        "inc_max1": level <= 1,
        "inc_1to2": 1 <= level <= 2,
        "inc_a_or_min3": a or level >= 3,
        "exc_test": phase != TEST,
        "exc_stage_a": not a,
        "exc_a_or_max0": not (a or level <= 0),
        "exc_train_not_b": not (phase == TRAIN and not b),
    }[rule]


STATES = [(TRAIN, 0, ()), (TEST, 0, ()), (TEST, 0, ("a",)),
          (TRAIN, 0, ("a", "b")), (TEST, 1, ("b",)), (TRAIN, 2, ("a",)),
          (TEST, 3, ()), (TEST, 2, ("b", "a", "c"))]


@pytest.fixture(scope="module")
def rules_net(tmp_path_factory):
    text = ('name: "rules"\nlayer { name: "in" type: "Input" top: "x" '
            "input_param { shape { dim: 1 dim: 4 } } }\n")
    for name, rule in RULES.items():
        text += (f'layer {{ name: "{name}" type: "ReLU" bottom: "x" '
                 f'top: "{name}" {rule} }}\n')
    p = tmp_path_factory.mktemp("state") / "rules.prototxt"
    p.write_text(text)
    return str(p)


@pytest.mark.parametrize("phase,level,stages", STATES)
def test_rule_table(rules_net, phase, level, stages):
    net = ca.Net.from_file(rules_net, phase=phase, stages=stages, level=level)
    got = set(net.blob_names())
    want = {r for r in RULES if expect(r, phase, level, stages)}
    # x is split among its consumers: compare the rule-named tops only
    assert got & set(RULES) == want
    assert set(net.layer_names()) & set(RULES) == want


def test_include_and_exclude_on_one_layer_is_an_error(tmp_path):
    p = write(tmp_path, "both.prototxt",
              'name: "b"\nlayer { name: "in" type: "Input" top: "x" '
              "input_param { shape { dim: 1 dim: 4 } } }\n"
              'layer { name: "r" type: "ReLU" bottom: "x" top: "y" '
              "include { phase: TRAIN } exclude { phase: TEST } }\n")
    with pytest.raises(ca.CaffeError, match="'r'"):
        ca.Net.from_file(p)


AE_DATA = """name: "three_data"
layer { name: "data" type: "Data" top: "data"
  include { phase: TRAIN } data_param { batch_size: 3 } }
layer { name: "data" type: "Data" top: "data"
  include { phase: TEST stage: "test-on-train" } data_param { batch_size: 5 } }
layer { name: "data" type: "Data" top: "data"
  include { phase: TEST stage: "test-on-test" } data_param { batch_size: 7 } }
layer { name: "flat" type: "Flatten" bottom: "data" top: "flat" }
"""


def test_three_same_named_data_layers_one_survives_per_state(tmp_path):
    p = write(tmp_path, "ae.prototxt", AE_DATA)
    for phase, stages, batch in [(TRAIN, (), 3),
                                 (TEST, ("test-on-train",), 5),
                                 (TEST, ("test-on-test",), 7)]:
        net = ca.Net.from_file(p, phase=phase, stages=stages)
        assert net.layer_names().count("data") == 1
        assert net.blob_shape("data") == (batch, 1, 6, 6)
        assert net.blob_shape("flat") == (batch, 36)
    # TEST without a stage keeps no Data layer; with both stages two layers
    # would write the one top: both are errors that name the layer
    with pytest.raises(ca.CaffeError, match="flat"):
        ca.Net.from_file(p, phase=TEST)
    with pytest.raises(ca.CaffeError, match="'data'.*more than one layer"):
        ca.Net.from_file(p, phase=TEST,
                         stages=("test-on-train", "test-on-test"))


def test_pycaffe_shim_takes_stages_and_level(tmp_path):
    import caffe_amd.pycaffe as caffe
    p = write(tmp_path, "ae.prototxt", AE_DATA)
    net = caffe.Net(p, caffe.TEST, stages=["test-on-test"])
    assert net.blobs["data"].data.shape == (7, 1, 6, 6)
    net = caffe.Net(p, caffe.TRAIN, level=0)
    assert net.blobs["data"].data.shape == (3, 1, 6, 6)


# --------------------------------------------------------- solver test nets
AE_NET = AE_DATA.replace('name: "three_data"', 'name: "tiny_ae"').replace(
    'layer { name: "flat" type: "Flatten" bottom: "data" top: "flat" }',
    'layer { name: "flat" type: "Flatten" bottom: "data" top: "flatdata" }'
) + """layer { name: "enc" type: "InnerProduct" bottom: "data" top: "enc"
  inner_product_param { num_output: 5
    weight_filler { type: "gaussian" std: 0.3 } } }
layer { name: "encn" type: "Sigmoid" bottom: "enc" top: "encn" }
layer { name: "dec" type: "InnerProduct" bottom: "encn" top: "dec"
  inner_product_param { num_output: 36
    weight_filler { type: "gaussian" std: 0.3 } } }
layer { name: "loss" type: "SigmoidCrossEntropyLoss" bottom: "dec"
  bottom: "flatdata" top: "cross_entropy_loss" loss_weight: 1 }
layer { name: "decn" type: "Sigmoid" bottom: "dec" top: "decn" }
layer { name: "loss" type: "EuclideanLoss" bottom: "decn" bottom: "flatdata"
  top: "l2_error" loss_weight: 0 }
"""

AE_SOLVER = """net: "%s"
test_state: { stage: 'test-on-train' }
test_iter: 2
test_state: { stage: 'test-on-test' }
test_iter: 3
test_interval: 100
test_compute_loss: true
base_lr: 0.01 lr_policy: "fixed" momentum: 0.9 max_iter: 10 random_seed: 5
"""


def test_two_test_states_give_two_test_nets(tmp_path, capfd):
    net_path = write(tmp_path, "ae.prototxt", AE_NET)
    solver = ca.Solver(text=AE_SOLVER % net_path)
    nets = solver.test_nets
    assert len(nets) == 2
    assert nets[0].blob_shape("data")[0] == 5  # test-on-train's layer
    assert nets[1].blob_shape("data")[0] == 7  # test-on-test's layer
    assert solver.net.blob_shape("data")[0] == 3
    solver.step(2)
    for i, net in enumerate(nets):
        got = solver.test(i, 2)
        assert set(got) == {"cross_entropy_loss", "l2_error"}
        # a manual forward average over the same two batches, with the
        # trained weights the test net shares
        want = {k: 0.0 for k in got}
        for it in range(2):
            ca.set_data_iter(it)
            net.forward()
            for k in want:
                want[k] += float(net.blob(k)[0]) / 2
        for k in got:
            assert got[k] == pytest.approx(want[k], rel=1e-6), (i, k)
        assert got["l2_error"] > 0  # zero loss weight, still reported
    # the iteration-0 test pass printed one block per net, with the top
    # blobs' names where the two layers share the name `loss`
    err = capfd.readouterr().err
    assert "Testing net (#0)" in err and "Testing net (#1)" in err
    assert err.count("Test net output: cross_entropy_loss = ") == 2
    assert err.count("Test net output: l2_error = ") == 2
    # the shim shows the same nets
    import caffe_amd.pycaffe as caffe
    sp = write(tmp_path, "solver.prototxt", AE_SOLVER % net_path)
    s = caffe.SGDSolver(sp)
    assert len(s.test_nets) == 2
    assert s.test_nets[1].blobs["data"].data.shape[0] == 7


@pytest.mark.parametrize("drop", ["test_iter: 3\n",
                                  "test_state: { stage: 'test-on-test' }\n"])
def test_test_iter_count_mismatch_is_a_construction_error(tmp_path, drop):
    net_path = write(tmp_path, "ae.prototxt", AE_NET)
    text = (AE_SOLVER % net_path).replace(drop, "")
    with pytest.raises(ca.CaffeError) as e:
        ca.Solver(text=text)
    msg = str(e.value)
    assert "test_iter" in msg and "1" in msg and "2" in msg, msg


# ----------------------------------- nothing moved without test_state
PLAIN_NET = """name: "plain"
layer { name: "data" type: "Data" top: "data" top: "label"
  include { phase: TRAIN } data_param { batch_size: 4 } }
layer { name: "data" type: "Data" top: "data" top: "label"
  include { phase: TEST } data_param { batch_size: 4 } }
layer { name: "ip" type: "InnerProduct" bottom: "data" top: "ip"
  inner_product_param { num_output: 10
    weight_filler { type: "gaussian" std: 0.1 }
    bias_filler { type: "constant" value: 0.2 } } }
layer { name: "accuracy" type: "Accuracy" bottom: "ip" bottom: "label"
  top: "accuracy" include { phase: TEST } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "ip" bottom: "label"
  top: "loss" }
"""
PLAIN_SOLVER = """net: "%s"
base_lr: 0.05 lr_policy: "fixed" momentum: 0.9 display: 1 max_iter: 4
test_interval: 2 test_iter: 3 random_seed: 7
"""
# stderr of the commit before net states existed, for exactly this solver
# text, net and seed (CPU mode, synthetic shape 1x6x6, 10 classes)
PLAIN_STDERR = """[caffe_amd] Test net output: accuracy = 0
[caffe_amd] Test net output: loss = 2.38757
[caffe_amd] Iteration 1, loss = 2.38757, lr = 0.05
[caffe_amd] Iteration 2, loss = 2.38714, lr = 0.05
[caffe_amd] Test net output: accuracy = 0.166667
[caffe_amd] Test net output: loss = 2.17959
[caffe_amd] Iteration 3, loss = 2.15447, lr = 0.05
[caffe_amd] Iteration 4, loss = 2.38101, lr = 0.05
"""


def test_solver_without_test_state_prints_the_same_lines(tmp_path, capfd):
    ca.set_rank_world(0, 1)
    net_path = write(tmp_path, "net.prototxt", PLAIN_NET)
    capfd.readouterr()
    solver = ca.Solver(text=PLAIN_SOLVER % net_path)
    solver.step(4)
    assert capfd.readouterr().err == PLAIN_STDERR
    assert len(solver.test_nets) == 1
    assert set(solver.test(0, 3)) == {"accuracy", "loss"}
