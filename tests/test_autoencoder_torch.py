"""torch-CPU as a second, independent check of the Sigmoid, the
SigmoidCrossEntropyLoss and the EuclideanLoss CPU paths (the style of
test_torch_crosscheck.py).  CPU only: a file with GPU tests must not import
torch (tests/conftest.py)."""
import numpy as np
import torch

import engine_util as eu
from test_autoencoder_layers import EUC, SCE, SIG, rnd, run

TOL = eu.TOL
F = torch.nn.functional


def test_torch_cpu_agrees():
    x = rnd(27, 4, 33)
    t = np.random.default_rng(28).random((4, 33)).astype(np.float32)
    tx, tt = torch.from_numpy(x).double(), torch.from_numpy(t).double()
    _, y = run("cpu", [x.shape], SIG % "out", [x])
    assert eu.relerr(y, torch.sigmoid(tx).numpy()) <= TOL
    _, l = run("cpu", [x.shape] * 2, SCE % "", [x, t])
    ref = F.binary_cross_entropy_with_logits(tx, tt, reduction="sum") / 4
    assert eu.relerr(l, ref.item()) <= TOL
    _, l = run("cpu", [x.shape] * 2, EUC % "", [x, t])
    ref = F.mse_loss(tx, tt, reduction="sum") / (2 * 4)
    assert eu.relerr(l, ref.item()) <= TOL
