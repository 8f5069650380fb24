"""The reference's CIFAR-10 "full" model (examples/cifar10/cifar10_full*):
its two LRN layers use norm_region WITHIN_CHANNEL.  The files are read from
the read-only mount and skipped where it is absent; nothing is copied.
"""
import os

import numpy as np
import pytest

import caffe_amd as ca
from test_reference_prototxts import REF, needs_ref, train_steps

CIFAR = os.path.join(REF, "examples/cifar10")


@needs_ref
def test_reference_cifar10_full_train_test():
    train_steps(os.path.join(CIFAR, "cifar10_full_train_test.prototxt"),
                (3, 32, 32), 10, steps=2, batch=4)


@needs_ref
def test_reference_cifar10_full_solver_file():
    # verbatim (snapshot_format: HDF5 included; the snapshot interval of
    # 10000 is never reached), relative net path resolved from the reference
    # root as cwd
    ca.set_mode("cpu")
    ca.set_synthetic_shape(3, 32, 32, 10)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        solver = ca.Solver(
            path=os.path.join(CIFAR, "cifar10_full_solver.prototxt"),
            batch_override=4)
        solver.step(2)
        loss = solver.loss()
    finally:
        os.chdir(cwd)
    assert np.isfinite(loss) and loss > 0, loss


@needs_ref
def test_reference_cifar10_full_deploy():
    ca.set_mode("cpu")
    net = ca.Net.from_file(os.path.join(CIFAR, "cifar10_full.prototxt"),
                           phase=1)
    shape = net.blob_shape("data")
    net.set_blob("data", np.random.default_rng(11).standard_normal(shape)
                 .astype(np.float32))
    net.forward()
    prob = net.blob("prob")
    assert np.allclose(prob.reshape(prob.shape[0], -1).sum(1), 1.0, atol=1e-4)
