"""The reference's own Adam / RMSProp / AdaDelta solver prototxts (from the
read-only /root/reference mount) run verbatim, with the update rule their
`type` field names.  Nothing from the reference is copied into the repo —
these CPU tests read the mount directly and skip where it is absent.
"""
import os

import numpy as np
import pytest

import caffe_amd as ca

REF = "/root/reference"

needs_ref = pytest.mark.skipif(not os.path.isdir(REF),
                               reason="/root/reference not mounted")


@needs_ref
@pytest.mark.parametrize("name,kind,slots", [
    ("lenet_solver_adam.prototxt", "Adam", 2),
    ("lenet_solver_rmsprop.prototxt", "RMSProp", 1),
    ("lenet_adadelta_solver.prototxt", "AdaDelta", 2),
])
def test_reference_mnist_solver_file(name, kind, slots):
    # relative net path: resolved from the reference root as cwd; nothing is
    # written (snapshot interval 5000 is never reached and the python API
    # path does not snapshot after train)
    ca.set_mode("cpu")
    ca.set_synthetic_shape(1, 28, 28, 10)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        solver = ca.Solver(path=os.path.join(REF, "examples/mnist", name),
                           batch_override=8)
        solver.step(3)
        loss = solver.loss()
    finally:
        os.chdir(cwd)
    assert np.isfinite(loss) and loss > 0, loss
    assert solver.type == kind
    assert solver.history_slots == slots
    assert np.abs(solver.history(0, 0)).max() > 0
    if slots == 2:
        assert np.abs(solver.history(0, 1)).max() > 0
