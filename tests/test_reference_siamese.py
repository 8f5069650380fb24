"""The reference's MNIST siamese net (examples/siamese/), end to end.

The model below has the reference's topology at reduced widths — a two-top
Data layer of 2-channel pairs, a Slice into the two towers, conv / pool /
ip / ReLU / ip per tower with every param shared by name, ContrastiveLoss —
under the reference solver's rule (SGD, momentum 0.9, `inv` policy).  The
verbatim reference files are read from the read-only mount and skipped where
it is absent; nothing from it is copied.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import caffe_amd as ca
from caffe_amd import pycaffe
from engine_util import REPO, TOL, relerr

sys.path.insert(0, os.path.join(REPO, "tools"))
from make_lmdb import make_lmdb, record_bytes  # noqa: E402

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF),
                               reason="/root/reference not mounted")

BATCH, N_REC, SEED = 8, 64, 43  # 8 batches: one pass over the database
HW, K, CONV, IP1, FEAT = 12, 5, 4, 6, 2
POOLED = (HW - K + 1) // 2  # 4
SCALE = 0.00390625
MARGIN = 1.0
BASE_LR, MOM, GAMMA, POWER = 0.05, 0.9, 0.0001, 0.75
OWNERS = ["conv1", "ip1", "feat"]


def tower(sfx, bottom):
    def named(layer):
        return (f'param {{ name: "{layer}_w" lr_mult: 1 }} '
                f'param {{ name: "{layer}_b" lr_mult: 2 }}')
    return f"""layer {{ name: "conv1{sfx}" type: "Convolution" bottom: "{bottom}"
  top: "conv1{sfx}" {named("conv1")}
  convolution_param {{ num_output: {CONV} kernel_size: {K} stride: 1
    weight_filler {{ type: "xavier" }} bias_filler {{ type: "constant" }} }} }}
layer {{ name: "pool1{sfx}" type: "Pooling" bottom: "conv1{sfx}"
  top: "pool1{sfx}" pooling_param {{ pool: MAX kernel_size: 2 stride: 2 }} }}
layer {{ name: "ip1{sfx}" type: "InnerProduct" bottom: "pool1{sfx}"
  top: "ip1{sfx}" {named("ip1")}
  inner_product_param {{ num_output: {IP1}
    weight_filler {{ type: "xavier" }} bias_filler {{ type: "constant" }} }} }}
layer {{ name: "relu1{sfx}" type: "ReLU" bottom: "ip1{sfx}" top: "ip1{sfx}" }}
layer {{ name: "feat{sfx}" type: "InnerProduct" bottom: "ip1{sfx}"
  top: "feat{sfx}" {named("feat")}
  inner_product_param {{ num_output: {FEAT}
    weight_filler {{ type: "xavier" }} bias_filler {{ type: "constant" }} }} }}
"""


def siamese_net(db):
    text = 'name: "TinySiamese"\n'
    for phase in ("TRAIN", "TEST"):
        text += f"""layer {{ name: "pair_data" type: "Data" top: "pair_data"
  top: "sim" include {{ phase: {phase} }}
  transform_param {{ scale: {SCALE} }}
  data_param {{ source: "{db}" batch_size: {BATCH} backend: LMDB }} }}
"""
    text += """layer { name: "slice_pair" type: "Slice" bottom: "pair_data"
  top: "data" top: "data_p" slice_param { slice_dim: 1 slice_point: 1 } }
"""
    text += tower("", "data") + tower("_p", "data_p")
    text += f"""layer {{ name: "loss" type: "ContrastiveLoss" bottom: "feat"
  bottom: "feat_p" bottom: "sim" top: "loss"
  contrastive_loss_param {{ margin: {MARGIN} }} }}
"""
    return text


def siamese_solver(net_path):
    return f"""net: "{net_path}"
test_iter: 8
test_interval: 1000
base_lr: {BASE_LR}
momentum: {MOM}
weight_decay: 0.0
lr_policy: "inv"
gamma: {GAMMA}
power: {POWER}
max_iter: 100
random_seed: 17
"""


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("siamese")
    make_lmdb(str(d / "pair_db"), N_REC, 2, HW, HW, SEED, label_mod=2)
    net = d / "siamese.prototxt"
    net.write_text(siamese_net(str(d / "pair_db")))
    solver = d / "solver.prototxt"
    solver.write_text(siamese_solver(str(net)))
    return str(net), str(solver)


@pytest.fixture(autouse=True)
def reset():
    ca.set_data_iter(0)
    ca.set_rank_world(0, 1)
    yield
    ca.set_data_iter(0)
    ca.set_mode("cpu")


# ---------------------------------------------------------- float64 replay
def batch64(it):
    """Batch `it`: records it*8 .. it*8+7 (mod 64) -> (pairs, sim)."""
    idx = [(it * BATCH + j) % N_REC for j in range(BATCH)]
    rows = [np.frombuffer(record_bytes(SEED, i, 2, HW, HW), np.uint8)
            for i in idx]
    x = np.stack(rows).astype(np.float64).reshape(BATCH, 2, HW, HW) * SCALE
    return x, np.array([i % 2 for i in idx])


def tower64(P, x):
    """x [B][12][12] -> (feat, what the backward needs)."""
    win = sliding_window_view(x, (K, K), axis=(1, 2))  # [B][8][8][5][5]
    conv = np.einsum("bijuv,kuv->bkij", win, P["conv1", 0][:, 0]) \
        + P["conv1", 1][None, :, None, None]
    blocks = conv.reshape(BATCH, CONV, POOLED, 2, POOLED, 2)
    blocks = blocks.transpose(0, 1, 2, 4, 3, 5).reshape(
        BATCH, CONV, POOLED, POOLED, 4)
    arg = blocks.argmax(-1)
    pool = blocks.max(-1).reshape(BATCH, -1)
    h = pool @ P["ip1", 0].T + P["ip1", 1]
    r = np.maximum(h, 0)
    feat = r @ P["feat", 0].T + P["feat", 1]
    return feat, (win, arg, pool, h, r)


def tower_grads64(P, saved, dfeat):
    win, arg, pool, h, r = saved
    G = {("feat", 0): dfeat.T @ r, ("feat", 1): dfeat.sum(0)}
    dh = (dfeat @ P["feat", 0]) * (h > 0)
    G["ip1", 0] = dh.T @ pool
    G["ip1", 1] = dh.sum(0)
    dpool = (dh @ P["ip1", 0]).reshape(BATCH, CONV, POOLED, POOLED)
    dblocks = np.zeros((BATCH, CONV, POOLED, POOLED, 4))
    np.put_along_axis(dblocks, arg[..., None], dpool[..., None], -1)
    dconv = dblocks.reshape(BATCH, CONV, POOLED, POOLED, 2, 2).transpose(
        0, 1, 2, 4, 3, 5).reshape(BATCH, CONV, 2 * POOLED, 2 * POOLED)
    G["conv1", 0] = np.einsum("bkij,bijuv->kuv", dconv, win)[:, None]
    G["conv1", 1] = dconv.sum((0, 2, 3))
    return G


def contrastive64(fa, fb, sim):
    """-> (loss, dfa); dfb = -dfa."""
    diff = fa - fb
    d = np.sqrt((diff * diff).sum(1))
    md = MARGIN - d
    loss = np.where(sim != 0, d * d, np.maximum(md, 0) ** 2).sum() / BATCH / 2
    coef = np.where(sim != 0, 1.0,
                    np.where(md > 0, -md / (d + 1e-4), 0.0)) / BATCH
    return loss, coef[:, None] * diff


def loss_and_grads64(Pa, Pb, it):
    x, sim = batch64(it)
    fa, sa = tower64(Pa, x[:, 0])
    fb, sb = tower64(Pb, x[:, 1])
    loss, dfa = contrastive64(fa, fb, sim)
    return loss, tower_grads64(Pa, sa, dfa), tower_grads64(Pb, sb, -dfa)


def mean_loss64(Pa, Pb):
    return np.mean([loss_and_grads64(Pa, Pb, it)[0] for it in range(8)])


def sgd64(P, G, H, it):
    lr = BASE_LR * (1 + GAMMA * it) ** -POWER
    for key in P:
        H[key] = MOM * H[key] + lr * (2.0 if key[1] == 1 else 1.0) * G[key]
        P[key] = P[key] - H[key]


def train64(P0, tied, iters=30):
    """Loss ratio over the whole database after `iters` steps.  tied: one
    param set, updated once by the sum of both towers' gradients; untied:
    each tower updates a set of its own from the same start."""
    Pa = {k: v.copy() for k, v in P0.items()}
    Pb = Pa if tied else {k: v.copy() for k, v in P0.items()}
    Ha = {k: np.zeros_like(v) for k, v in P0.items()}
    Hb = {k: np.zeros_like(v) for k, v in P0.items()}
    before = mean_loss64(Pa, Pb)
    for it in range(iters):
        _, Ga, Gb = loss_and_grads64(Pa, Pb, it)
        if tied:
            sgd64(Pa, {k: Ga[k] + Gb[k] for k in Ga}, Ha, it)
        else:
            sgd64(Pa, Ga, Ha, it)
            sgd64(Pb, Gb, Hb, it)
    return before, mean_loss64(Pa, Pb) / before


def shaped_params(net):
    """{(owner layer, blob): float64 array} in the layers' own shapes."""
    shapes = {("conv1", 0): (CONV, 1, K, K), ("conv1", 1): (CONV,),
              ("ip1", 0): (IP1, CONV * POOLED * POOLED), ("ip1", 1): (IP1,),
              ("feat", 0): (FEAT, IP1), ("feat", 1): (FEAT,)}
    P = {}
    for i in range(net.num_params()):
        name, bidx, _ = net.param_info(i)
        P[name, bidx] = net.param(i).astype(np.float64).reshape(
            shapes[name, bidx])
    assert set(P) == set(shapes)
    return P


# -------------------------------------------------------------------- CPU
def test_tiny_siamese_plan(files):
    ca.set_mode("cpu")
    solver = ca.Solver(path=files[1])
    net = solver.net
    assert net.param_sharing() == [
        (layer + "_p", b, f"{layer}_{'wb'[b]}", layer, b)
        for layer in OWNERS for b in (0, 1)]
    assert net.num_params() == 6
    assert net.blob_shape("pair_data") == (BATCH, 2, HW, HW)
    assert net.blob_shape("data_p") == (BATCH, 1, HW, HW)
    assert net.blob_shape("feat") == (BATCH, FEAT)


def test_tiny_siamese_trains_cpu(files):
    """30 iterations; the contrastive loss over the whole database (test
    net, 8 batches) must fall by the ratio a float64 numpy replay of the
    same net, data, initial weights and tied update reaches, within 1 %
    either way (the margin of test_reference_autoencoder.py).  A replay
    whose towers are NOT tied lands outside that band: the test tells
    shared weights from unshared ones."""
    ca.set_mode("cpu")
    solver = ca.Solver(path=files[1])
    assert solver.type == "SGD"
    P0 = shaped_params(solver.net)
    before64, ratio64 = train64(P0, tied=True)
    assert ratio64 < 0.9, ratio64  # the replay itself learns
    _, untied64 = train64(P0, tied=False)
    print(f"ratio64 {ratio64} untied64 {untied64}")
    assert abs(untied64 / ratio64 - 1) > 0.01, (untied64, ratio64)

    before = solver.test(0, 8)["loss"]
    assert before == pytest.approx(before64, rel=1e-4)
    solver.step(30)
    ratio = solver.test(0, 8)["loss"] / before
    print(f"ratio {ratio}")
    assert ratio <= ratio64 * 1.01, (ratio, ratio64)
    assert ratio >= ratio64 * 0.99, (ratio, ratio64)


def test_first_iteration_owner_diffs_cpu(files):
    """The owners' diffs after one backward are the sum of both towers'
    gradients (float64 replay) at TOL, and not one tower's."""
    ca.set_mode("cpu")
    solver = ca.Solver(path=files[1])
    net = solver.net
    P0 = shaped_params(net)
    loss64, Ga, Gb = loss_and_grads64(P0, P0, 0)
    net.forward()
    net.backward()
    assert net.loss() == pytest.approx(loss64, rel=1e-4)
    for i in range(net.num_params()):
        key = net.param_info(i)[:2]
        got = net.param(i, diff=True)
        assert relerr(got, Ga[key] + Gb[key]) <= TOL, key
        assert relerr(got, Ga[key]) > 100 * TOL, key


# -------------------------------------------------------------------- GPU
def run_steps(solver_path, mode, trace=False):
    ca.set_mode(mode)
    ca.set_data_iter(0)
    solver = ca.Solver(path=solver_path)
    net = solver.net
    net.forward()
    if trace:
        ca.kernel_trace(True)
    net.backward()
    sums = []
    if trace:
        ca.kernel_trace(False)
        sums = [r for r in ca.kernel_trace_read()
                if r["op"] == "shared_diff_sum"]
    diffs = {net.param_info(i)[:2]: net.param(i, diff=True)
             for i in range(net.num_params())}
    loss0 = net.loss()
    losses = []
    for _ in range(3):
        solver.step(1)
        losses.append(solver.loss())
    return solver, loss0, diffs, losses, sums


@pytest.mark.gpu
def test_tiny_siamese_gpu_matches_cpu(files):
    """Same net in GPU mode against CPU mode: the first iteration's owner
    diffs at TOL, 3 steps of loss at the project's full-net bound (2e-3),
    both towers still views of one memory, and exactly one shared_diff_sum
    launch per owner layer per backward."""
    _, c_loss0, c_diffs, c_losses, _ = run_steps(files[1], "cpu")
    solver, g_loss0, g_diffs, g_losses, sums = run_steps(files[1], "gpu",
                                                         trace=True)
    assert abs(c_loss0 - g_loss0) < 2e-3 * max(1.0, abs(c_loss0))
    assert set(c_diffs) == set(g_diffs) and len(c_diffs) == 6
    for key in c_diffs:
        # the towers' gradients of the last shared bias are exact negatives
        # (dfeat_p = -dfeat): that sum is exactly 0 in both modes
        assert np.abs(c_diffs[key]).max() > 0 or key == ("feat", 1), key
        assert relerr(g_diffs[key], c_diffs[key]) <= TOL, key
    assert not np.any(c_diffs["feat", 1]) and not np.any(g_diffs["feat", 1])
    for lc, lg in zip(c_losses, g_losses):
        assert np.isfinite(lg)
        assert abs(lc - lg) < 2e-3 * max(1.0, abs(lc)), (lc, lg)
    # one launch per owner layer, last layer first, two blobs and two
    # sharers each, over disjoint ascending arena ranges
    assert len(sums) == 3, sums
    assert all(r["nseg"] == 2 and r["nsrc"] == 2 for r in sums), sums
    assert sums[0]["lo"] == 0
    for prev, nxt in zip(sums, sums[1:]):
        assert prev["hi"] == nxt["lo"]
    assert all(r["lo"] % 16 == 0 and r["hi"] % 16 == 0 for r in sums)
    view = pycaffe._WrappedNet(solver.net)
    for layer in OWNERS:
        for b in (0, 1):
            own = view.params[layer][b].data
            shr = view.params[layer + "_p"][b].data
            assert own.ctypes.data == shr.ctypes.data
            assert np.array_equal(own, shr)
            # (the last bias never moves: its gradient is exactly 0)
            assert np.any(own) or (layer, b) == ("feat", 1)


@pytest.mark.gpu
def test_lenet_launches_no_shared_diff_sum():
    path = os.path.join(REPO, "models", "generated",
                        "lenet_solver.prototxt")
    if not os.path.exists(path):
        subprocess.check_call([sys.executable,
                               os.path.join(REPO, "models", "gen_models.py")])
    ca.set_mode("gpu")
    ca.set_synthetic_shape(1, 28, 28, 10)
    solver = ca.Solver(path=path, batch_override=4)
    assert solver.net.param_sharing() == []
    ca.kernel_trace(True)
    solver.step(2)
    ca.device_synchronize()
    ca.kernel_trace(False)
    ops = [r["op"] for r in ca.kernel_trace_read()]
    assert "sgd_seg" in ops and "shared_diff_sum" not in ops, ops


# -------------------------------------------------------------------- CLI
def test_cli_train_and_time(files):
    net_path, solver_path = files
    caffe_bin = os.path.join(REPO, "caffe-mpi.github.io_amd", "caffe")
    text = open(solver_path).read().replace("max_iter: 100", "max_iter: 4")
    cli_solver = os.path.join(os.path.dirname(solver_path), "cli.prototxt")
    with open(cli_solver, "w") as f:
        f.write(text + "display: 2\nsnapshot_after_train: false\n")
    r = subprocess.run([caffe_bin, "train", "-solver", cli_solver],
                       capture_output=True, text=True, timeout=120,
                       cwd=os.path.dirname(solver_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Solver type: SGD" in r.stderr
    lines = [ln for ln in r.stderr.splitlines()
             if ln.startswith("Sharing parameters")]
    assert lines[:6] == [
        f"Sharing parameters '{layer}_{'wb'[b]}' owned by layer '{layer}', "
        f"param index {b}" for layer in OWNERS for b in (0, 1)], r.stderr
    losses = [float(ln.split("loss = ")[1].split(",")[0])
              for ln in r.stderr.splitlines() if "loss = " in ln]
    assert losses and all(np.isfinite(v) for v in losses), r.stderr
    r = subprocess.run([caffe_bin, "time", "-model", net_path,
                        "-iterations", "1"],
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr
    assert "slice_pair" in r.stderr and "loss" in r.stderr
    assert "TOTAL" in r.stderr


# ------------------------------------------------- the reference's own files
@needs_ref
def test_reference_siamese_solver_file():
    # relative net path: resolved from the reference root as cwd; nothing is
    # written (no snapshot interval is reached in 3 iterations).  The
    # leveldb sources are absent, so the synthetic stream feeds 2-channel
    # pairs with labels 0 / 1.
    ca.set_mode("cpu")
    ca.set_synthetic_shape(2, 28, 28, 2)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        solver = ca.Solver(
            path=os.path.join(REF, "examples/siamese",
                              "mnist_siamese_solver.prototxt"),
            batch_override=8)
        solver.step(3)
        loss = solver.loss()
    finally:
        os.chdir(cwd)
    net = solver.net
    assert np.isfinite(loss) and loss > 0, loss
    # the five parametered layers of one tower, two blobs each
    assert net.num_params() == 10
    assert net.blob_shape("data") == (8, 1, 28, 28)
    assert net.blob_shape("feat") == (8, 2)
    sharing = net.param_sharing()
    assert len(sharing) == 10
    assert all(s[0] == s[3] + "_p" and s[1] == s[4] for s in sharing)


@needs_ref
def test_reference_siamese_deploy_file():
    """examples/siamese/mnist_siamese.prototxt: the Input-fed single tower
    (no named params) builds and forwards."""
    ca.set_mode("cpu")
    net = ca.Net.from_file(os.path.join(REF, "examples/siamese",
                                        "mnist_siamese.prototxt"), phase=1)
    assert net.param_sharing() == [] and net.num_params() == 10
    net.forward()
    assert net.blob_shape("feat") == (10000, 2)
    assert np.all(np.isfinite(net.blob("feat")))
