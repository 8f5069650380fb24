"""Every device allocation has one owner that gives it back: freeing a
solver or a net returns the allocator's live byte count to where it was, and
a solver built in the memory a freed one gave back computes the same bits.

The nets are the two towers of test_param_sharing.py (one conv and one inner
product each on a 1x8x8 input, batch 2), with and without shared params, so
the cycles cover the diff arena and the per-layer events, the shared-param
sum tables, the history slots, the update tables, the clip buffers and the
iter_size accumulator.
"""
import numpy as np
import pytest

import caffe_amd as ca
from test_param_sharing import two_towers

pytestmark = pytest.mark.gpu

CYCLES = 3
STEPS = 2
PAIR = np.random.default_rng(11).standard_normal((2, 2, 8, 8)).astype(
    np.float32)

OWN = two_towers(conv_b="", ip_b="")  # nothing shared: 8 learnable params
SHARED = two_towers()                 # the second tower shares all four
SGD = 'type: "SGD"\nmomentum: 0.9\n'
# name -> (solver head, net)
CONFIGS = {
    "sgd": (SGD, OWN),
    "adam_clip": ('type: "Adam"\nmomentum: 0.9\nmomentum2: 0.999\n'
                  "clip_gradients: 0.01\n", OWN),
    "shared": (SGD, SHARED),
    "iter_size_2": (SGD + "iter_size: 2\n", OWN),
}


def solver_text(name):
    head, net = CONFIGS[name]
    return (head + 'base_lr: 0.05\nlr_policy: "fixed"\nweight_decay: 0.01\n'
            "reduce_buckets: 2\nrandom_seed: 7\nnet_param {\n" + net + "}\n")


@pytest.fixture(autouse=True)
def gpu_mode():
    ca.set_mode("gpu")
    yield
    ca.set_mode("cpu")


def solver_cycle(name):
    """Create, step, free.  Returns every param and every history slot as
    they stood before the free."""
    solver = ca.Solver(text=solver_text(name))
    net = solver.net
    net.set_blob("pair", PAIR)
    solver.step(STEPS)
    state = [net.param(i) for i in range(net.num_params())]
    state += [solver.history(i, slot) for slot in range(solver.history_slots)
              for i in range(net.num_params())]
    ca._lib.caffe_solver_free(solver._h)
    return state


def net_cycle(path):
    net = ca.Net.from_file(path)
    net.set_blob("pair", PAIR)
    net.forward()
    net.backward()
    assert np.isfinite(net.loss())
    ca._lib.caffe_net_free(net._h)


def assert_cycles_return_to_baseline(cycle):
    # the first cycle also grows the process-lifetime workspace slots
    cycle()
    baseline = ca.device_live_bytes()
    for k in range(CYCLES):
        cycle()
        live = ca.device_live_bytes()
        print(f"cycle {k}: live {live} baseline {baseline}")
        assert live == baseline


@pytest.mark.parametrize("name", list(CONFIGS))
def test_solver_free_returns_every_byte(name):
    assert_cycles_return_to_baseline(lambda: solver_cycle(name))


@pytest.mark.parametrize("net", ["own", "shared"])
def test_net_free_returns_every_byte(net, tmp_path):
    path = tmp_path / "towers.prototxt"
    path.write_text(OWN if net == "own" else SHARED)
    assert_cycles_return_to_baseline(lambda: net_cycle(str(path)))


def test_live_bytes_counts_a_live_solver():
    solver_cycle("sgd")  # workspace growth
    before = ca.device_live_bytes()
    solver = ca.Solver(text=solver_text("sgd"))
    held = ca.device_live_bytes() - before
    # at least the diff arena and one history slot: 4 B per learnable element
    elems = sum(solver.net.param_info(i)[2]
                for i in range(solver.net.num_params()))
    assert held >= 2 * 4 * elems
    ca._lib.caffe_solver_free(solver._h)
    assert ca.device_live_bytes() == before


def test_solver_in_released_memory_computes_the_same_bits():
    """The allocator reuses blocks by exact size, so each later solver lives
    in the blocks the one before gave back: nothing of the freed solver may
    still be writing there."""
    first = solver_cycle("sgd")
    assert any(np.any(h != 0) for h in first[len(first) // 2:])
    for _ in range(CYCLES):
        again = solver_cycle("sgd")
        assert len(again) == len(first)
        for a, b in zip(again, first):
            assert a.tobytes() == b.tobytes()
