"""The reference's MNIST autoencoder (examples/mnist/mnist_autoencoder.prototxt
and its three solver files), end to end.

The model below has the reference's topology at reduced widths — one-top
Data layers (one TRAIN, two TEST told apart by stage), Flatten, eight
InnerProducts with the sparse gaussian filler, Sigmoids, a
SigmoidCrossEntropyLoss and a zero-weight EuclideanLoss that share the layer
name `loss` — under a solver with two test_states.  The verbatim reference
files are read from the read-only mount and skipped where it is absent;
nothing from it is copied.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import caffe_amd as ca
from engine_util import REPO, TOL, relerr

sys.path.insert(0, os.path.join(REPO, "tools"))
from make_lmdb import make_lmdb, record_bytes  # noqa: E402

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF),
                               reason="/root/reference not mounted")

BATCH, N_REC, SEED = 8, 64, 41  # 8 batches: one pass over the database
WIDTHS = [20, 12, 8, 4, 8, 12, 20, 36]
NAMES = ["encode1", "encode2", "encode3", "encode4",
         "decode4", "decode3", "decode2", "decode1"]
SCALE = 0.0039215684


def ae_net(train_db, test_db):
    def data(rule, src):
        return f"""layer {{ name: "data" type: "Data" top: "data"
  include {{ {rule} }}
  transform_param {{ scale: {SCALE} }}
  data_param {{ source: "{src}" batch_size: {BATCH} backend: LMDB }} }}
"""
    text = 'name: "TinyAutoencoder"\n'
    text += data("phase: TRAIN", train_db)
    text += data('phase: TEST stage: "test-on-train"', train_db)
    text += data('phase: TEST stage: "test-on-test"', test_db)
    text += ('layer { name: "flatdata" type: "Flatten" bottom: "data" '
             'top: "flatdata" }\n')
    bottom = "data"
    for name, width in zip(NAMES, WIDTHS):
        # sparse: 3 — the narrowest weight has shape(0) = 4 outputs
        text += f"""layer {{ name: "{name}" type: "InnerProduct"
  bottom: "{bottom}" top: "{name}"
  param {{ lr_mult: 1 decay_mult: 1 }} param {{ lr_mult: 1 decay_mult: 0 }}
  inner_product_param {{ num_output: {width}
    weight_filler {{ type: "gaussian" std: 1 sparse: 3 }}
    bias_filler {{ type: "constant" value: 0 }} }} }}
"""
        if name != "decode1":
            text += (f'layer {{ name: "{name}neuron" type: "Sigmoid" '
                     f'bottom: "{name}" top: "{name}neuron" }}\n')
            bottom = name + "neuron"
    text += """layer { name: "loss" type: "SigmoidCrossEntropyLoss"
  bottom: "decode1" bottom: "flatdata" top: "cross_entropy_loss"
  loss_weight: 1 }
layer { name: "decode1neuron" type: "Sigmoid" bottom: "decode1"
  top: "decode1neuron" }
layer { name: "loss" type: "EuclideanLoss" bottom: "decode1neuron"
  bottom: "flatdata" top: "l2_error" loss_weight: 0 }
"""
    return text


RULES = {
    "Nesterov": 'base_lr: 0.01 momentum: 0.95 type: "Nesterov"',
    "AdaGrad": 'base_lr: 0.01 type: "AdaGrad"',
    "AdaDelta": 'base_lr: 1.0 momentum: 0.95 delta: 1e-8 type: "AdaDelta"',
}
DECAY = 0.0005


def ae_solver(net_path, kind):
    return f"""net: "{net_path}"
test_state: {{ stage: 'test-on-train' }}
test_iter: 8
test_state: {{ stage: 'test-on-test' }}
test_iter: 2
test_interval: 1000
test_compute_loss: true
lr_policy: "fixed"
max_iter: 100
weight_decay: {DECAY}
random_seed: 17
{RULES[kind]}
"""


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ae")
    make_lmdb(str(d / "train_db"), N_REC, 1, 6, 6, SEED)
    make_lmdb(str(d / "test_db"), 2 * BATCH, 1, 6, 6, SEED + 1)
    net = d / "ae.prototxt"
    net.write_text(ae_net(str(d / "train_db"), str(d / "test_db")))
    return d, str(net)


@pytest.fixture(autouse=True)
def reset():
    ca.set_data_iter(0)
    ca.set_rank_world(0, 1)
    yield
    ca.set_data_iter(0)
    ca.set_mode("cpu")


def batch64(it):
    """Batch `it` of the training stream: records it*8 .. it*8+7 (mod 64)."""
    rows = [np.frombuffer(record_bytes(SEED, (it * BATCH + j) % N_REC, 1, 6,
                                       6), np.uint8)
            for j in range(BATCH)]
    return np.stack(rows).astype(np.float64) * np.float64(np.float32(SCALE))


def sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def forward64(P, x):
    """-> (cross-entropy loss, activations per layer)."""
    acts = [x]
    for i, name in enumerate(NAMES):
        z = acts[-1] @ P[name, 0].T + P[name, 1]
        acts.append(z if name == "decode1" else sig(z))
    z = acts[-1]
    pos = (z >= 0).astype(np.float64)
    ce = -(z * (x - pos) - np.log1p(np.exp(z - 2 * z * pos))).sum() / BATCH
    return ce, acts


def grads64(P, x):
    ce, acts = forward64(P, x)
    G = {}
    d = (sig(acts[-1]) - x) / BATCH  # the zero-weight l2 loss adds nothing
    for i in range(len(NAMES) - 1, -1, -1):
        name = NAMES[i]
        G[name, 0] = d.T @ acts[i]
        G[name, 1] = d.sum(0)
        if i > 0:
            d = (d @ P[name, 0]) * acts[i] * (1 - acts[i])
    return ce, G


def update64(kind, P, G, H, H2):
    """One update, the reference's rule per solver type
    (solvers/{nesterov,adagrad,adadelta}_solver.cpp); the deltas are the
    engine's documented floors (DESIGN: 1e-3 for both)."""
    for key in P:
        decay = DECAY if key[1] == 0 else 0.0
        g = G[key] + decay * P[key]
        if kind == "Nesterov":
            lr, mom = 0.01, 0.95
            h0 = H[key]
            H[key] = mom * h0 + lr * g
            P[key] = P[key] - ((1 + mom) * H[key] - mom * h0)
        elif kind == "AdaGrad":
            H[key] = H[key] + g * g
            P[key] = P[key] - 0.01 * g / (np.sqrt(H[key]) + 1e-3)
        else:
            mom, delta = 0.95, 1e-3
            H[key] = mom * H[key] + (1 - mom) * g * g
            u = g * np.sqrt((H2[key] + delta) / (H[key] + delta))
            H2[key] = mom * H2[key] + (1 - mom) * u * u
            P[key] = P[key] - 1.0 * u


def mean_ce64(P):
    return np.mean([forward64(P, batch64(it))[0] for it in range(8)])


def shaped_params(net):
    """{(layer, blob): float64 array}, weights as [out][in]."""
    P = {}
    fan_in = 36
    flat = {}
    for i in range(net.num_params()):
        name, bidx, _ = net.param_info(i)
        flat[name, bidx] = net.param(i).astype(np.float64)
    for name, width in zip(NAMES, WIDTHS):
        P[name, 0] = flat[name, 0].reshape(width, fan_in)
        P[name, 1] = flat[name, 1]
        fan_in = width
    return P


@pytest.mark.parametrize("kind", ["Nesterov", "AdaGrad", "AdaDelta"])
def test_tiny_autoencoder_trains_cpu(files, kind):
    """30 iterations; the cross-entropy over the whole training database
    (test net #0, 8 batches) must fall by the ratio a float64 numpy replay of
    the same net, data, initial weights and rule reaches, with a 1 % margin:
    float32 forward/backward and update differ from float64 by ~1e-6
    relative per step, and 30 steps of this smooth, non-chaotic net (no
    ReLU masks, no dropout) stay orders of magnitude inside 1e-2."""
    _, net_path = files
    ca.set_mode("cpu")
    solver = ca.Solver(text=ae_solver(net_path, kind))
    assert solver.type == kind
    assert len(solver.test_nets) == 2
    P = shaped_params(solver.net)
    # the sparse filler left about 3 of shape(0) weights per column
    assert 0 < np.count_nonzero(P["encode1", 0]) < P["encode1", 0].size / 2
    H = {k: np.zeros_like(v) for k, v in P.items()}
    H2 = {k: np.zeros_like(v) for k, v in P.items()}
    before64 = mean_ce64(P)
    for it in range(30):
        _, G = grads64(P, batch64(it))
        update64(kind, P, G, H, H2)
    ratio64 = mean_ce64(P) / before64
    assert ratio64 < 0.97, ratio64  # the replay itself learns

    before = solver.test(0, 8)["cross_entropy_loss"]
    assert before == pytest.approx(before64, rel=1e-4)
    solver.step(30)
    after = solver.test(0, 8)
    ratio = after["cross_entropy_loss"] / before
    assert ratio <= ratio64 * 1.01, (ratio, ratio64)
    assert ratio >= ratio64 * 0.99, (ratio, ratio64)
    assert after["l2_error"] > 0
    other = solver.test(1, 2)
    assert set(other) == {"cross_entropy_loss", "l2_error"}
    assert np.isfinite(other["cross_entropy_loss"])


@pytest.mark.gpu
def test_tiny_autoencoder_gpu_matches_cpu(files):
    """Same net in GPU mode against CPU mode: 3 steps at the project's
    full-net loss bound (2e-3, test_gpu_parity.py), the first iteration's
    param diffs per layer at TOL, both test nets at 2e-3."""
    _, net_path = files
    res = {}
    for mode in ("cpu", "gpu"):
        ca.set_mode(mode)
        ca.set_data_iter(0)
        solver = ca.Solver(text=ae_solver(net_path, "Nesterov"))
        net = solver.net
        net.forward()
        net.backward()
        diffs = {net.param_info(i)[:2]: net.param(i, diff=True)
                 for i in range(net.num_params())}
        loss0 = net.loss()
        losses = []
        for _ in range(3):
            solver.step(1)
            losses.append(solver.loss())
        tests = [solver.test(0, 8), solver.test(1, 2)]
        res[mode] = (loss0, diffs, losses, tests)
    c, g = res["cpu"], res["gpu"]
    assert abs(c[0] - g[0]) < 2e-3 * max(1.0, abs(c[0]))
    assert set(c[1]) == set(g[1]) and len(c[1]) == 16
    for key in c[1]:
        assert np.abs(c[1][key]).max() > 0, key
        assert relerr(g[1][key], c[1][key]) <= TOL, key
    for lc, lg in zip(c[2], g[2]):
        assert np.isfinite(lg)
        assert abs(lc - lg) < 2e-3 * max(1.0, abs(lc)), (lc, lg)
    for tc, tg in zip(c[3], g[3]):
        assert set(tc) == set(tg) == {"cross_entropy_loss", "l2_error"}
        for k in tc:
            assert abs(tc[k] - tg[k]) < 2e-3 * max(1.0, abs(tc[k])), k


# --------------------------------------------------------------------- CLI
def test_cli_test_with_stage(files):
    _, net_path = files
    caffe_bin = os.path.join(REPO, "caffe-mpi.github.io_amd", "caffe")
    r = subprocess.run([caffe_bin, "test", "-model", net_path, "-stage",
                        "test-on-test", "-iterations", "2"],
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cross_entropy_loss = " in r.stdout and "l2_error = " in r.stdout
    # without -stage no Data layer of the TEST phase is kept
    r = subprocess.run([caffe_bin, "test", "-model", net_path,
                        "-iterations", "2"],
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 1
    assert "FATAL" in r.stderr and "data" in r.stderr
    # with both stages the two Data layers would write the one top `data`:
    # a clean error that names the layer
    r = subprocess.run([caffe_bin, "test", "-model", net_path,
                        "-stage=test-on-train,test-on-test", "-level=0"],
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 1
    assert "layer 'data'" in r.stderr and "more than one layer" in r.stderr
    r = subprocess.run([caffe_bin, "time", "-model", net_path,
                        "-iterations", "1"],
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr
    assert "encode4neuron" in r.stderr and "TOTAL" in r.stderr


# ------------------------------------------------- the reference's own files
@needs_ref
@pytest.mark.parametrize("name,kind", [
    ("mnist_autoencoder_solver_nesterov.prototxt", "Nesterov"),
    ("mnist_autoencoder_solver_adagrad.prototxt", "AdaGrad"),
    ("mnist_autoencoder_solver_adadelta.prototxt", "AdaDelta"),
])
def test_reference_autoencoder_solver_file(name, kind):
    # relative net path: resolved from the reference root as cwd; nothing is
    # written (no snapshot interval is reached in 3 iterations)
    ca.set_mode("cpu")
    ca.set_synthetic_shape(1, 28, 28, 10)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        solver = ca.Solver(path=os.path.join(REF, "examples/mnist", name),
                           batch_override=8)
        solver.step(3)
        loss = solver.loss()
        nets = solver.test_nets
        scores = solver.test(1, 2)
    finally:
        os.chdir(cwd)
    assert solver.type == kind
    assert np.isfinite(loss) and loss > 0, loss
    assert len(nets) == 2
    assert nets[0].blob_shape("flatdata") == (100, 784)
    assert set(scores) == {"cross_entropy_loss", "l2_error"}
    assert all(np.isfinite(v) for v in scores.values())


@needs_ref
def test_reference_cifar10_full_sigmoid():
    """examples/cifar10/cifar10_full_sigmoid_solver.prototxt constructs too,
    now that Sigmoid exists."""
    ca.set_mode("cpu")
    ca.set_synthetic_shape(3, 32, 32, 10)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        solver = ca.Solver(
            path=os.path.join(REF, "examples/cifar10",
                              "cifar10_full_sigmoid_solver.prototxt"),
            batch_override=4)
        solver.step(2)
        loss = solver.loss()
    finally:
        os.chdir(cwd)
    assert np.isfinite(loss) and loss > 0, loss
    assert any(n.lower().startswith("sigmoid")
               for n in solver.net.layer_names()), solver.net.layer_names()
