"""GPU graph-fusion fuzz: random graphs built to TRIGGER the GPU-only
graph passes (BN+in-place-ReLU fusion, Eltwise+ReLU fusion, the
BN+residual-add epilogue, conv-epilogue ReLU, in-place BN, strided 1x1
scatter-dgrad, strided implicit views) and compared CPU vs GPU on loss,
input gradient and every param gradient.  The fixed model tests cover
these fusions only in the exact ResNet/GoogLeNet shapes; here the
combinations are randomized (fixed seeds — deterministic).
"""
import numpy as np
import pytest

import caffe_amd as ca
from engine_util import net_from_text

pytestmark = pytest.mark.gpu


def gen_graph(rng):
    n = int(rng.integers(2, 4))
    c = int(rng.integers(3, 6))
    hw = int(rng.choice([8, 9, 12]))
    lines = []
    cur = "in0"
    li = 0
    for _ in range(int(rng.integers(2, 5))):
        kind = rng.choice(["convbnrelu", "residual", "conv_inplace_relu",
                           "strided1x1", "inplace_bn", "pool"])
        li += 1
        nm = f"l{li}"
        top = f"t{li}"
        if kind == "convbnrelu":
            co = int(rng.integers(3, 7))
            lines += [
                f'layer {{ name: "{nm}c" type: "Convolution" '
                f'bottom: "{cur}" top: "{top}" convolution_param {{ '
                f'num_output: {co} kernel_size: 3 pad: 1 '
                f'weight_filler {{ type: "gaussian" std: 0.3 }} }} }}',
                f'layer {{ name: "{nm}b" type: "BatchNorm" '
                f'bottom: "{top}" top: "{top}bn" '
                f'batch_norm_param {{ scale_bias: true }} }}',
                # in-place ReLU directly after BN -> fused epilogue
                f'layer {{ name: "{nm}r" type: "ReLU" '
                f'bottom: "{top}bn" top: "{top}bn" }}']
            cur = f"{top}bn"
        elif kind == "residual":
            co = int(rng.integers(3, 6))
            # two branches from cur: conv+BN vs 1x1 conv; SUM; ReLU
            branch = [
                f'layer {{ name: "{nm}a" type: "Convolution" '
                f'bottom: "{cur}" top: "{top}a" convolution_param {{ '
                f'num_output: {co} kernel_size: 3 pad: 1 '
                f'weight_filler {{ type: "gaussian" std: 0.3 }} }} }}',
                f'layer {{ name: "{nm}ab" type: "BatchNorm" '
                f'bottom: "{top}a" top: "{top}abn" '
                f'batch_norm_param {{ scale_bias: true }} }}']
            shortcut = [
                f'layer {{ name: "{nm}s" type: "Convolution" '
                f'bottom: "{cur}" top: "{top}s" convolution_param {{ '
                f'num_output: {co} kernel_size: 1 bias_term: false '
                f'weight_filler {{ type: "gaussian" std: 0.3 }} }} }}']
            # shortcut first: the BN sits right before the sum and the
            # BN + residual-add fusion fires; shortcut second: the conv
            # between them keeps it from firing
            lines += (shortcut + branch if rng.integers(0, 2) else
                      branch + shortcut)
            lines += [
                f'layer {{ name: "{nm}e" type: "Eltwise" '
                f'bottom: "{top}abn" bottom: "{top}s" top: "{top}" '
                f'eltwise_param {{ operation: SUM }} }}',
                f'layer {{ name: "{nm}r" type: "ReLU" '
                f'bottom: "{top}" top: "{top}" }}']
            cur = top
        elif kind == "conv_inplace_relu":
            co = int(rng.integers(3, 6))
            lines += [
                f'layer {{ name: "{nm}c" type: "Convolution" '
                f'bottom: "{cur}" top: "{top}" convolution_param {{ '
                f'num_output: {co} kernel_size: 3 pad: 1 '
                f'weight_filler {{ type: "gaussian" std: 0.3 }} '
                f'bias_filler {{ type: "gaussian" std: 0.1 }} }} }}',
                f'layer {{ name: "{nm}r" type: "ReLU" '
                f'bottom: "{top}" top: "{top}" }}']
            cur = top
        elif kind == "strided1x1":
            co = int(rng.integers(3, 6))
            lines += [
                f'layer {{ name: "{nm}c" type: "Convolution" '
                f'bottom: "{cur}" top: "{top}" convolution_param {{ '
                f'num_output: {co} kernel_size: 1 stride: 2 '
                f'bias_term: false '
                f'weight_filler {{ type: "gaussian" std: 0.3 }} }} }}']
            cur = top
        elif kind == "inplace_bn":
            lines += [
                f'layer {{ name: "{nm}b" type: "BatchNorm" '
                f'bottom: "{cur}" top: "{cur}" '
                f'batch_norm_param {{ scale_bias: true }} }}']
        else:
            lines += [
                f'layer {{ name: "{nm}p" type: "Pooling" bottom: "{cur}" '
                f'top: "{top}" pooling_param {{ pool: MAX kernel_size: 2 '
                f'stride: 1 }} }}']
            cur = top
    lines += [
        f'layer {{ name: "ip" type: "InnerProduct" bottom: "{cur}" '
        f'top: "fc" inner_product_param {{ num_output: 4 '
        f'weight_filler {{ type: "gaussian" std: 0.2 }} }} }}',
        f'layer {{ name: "loss" type: "SoftmaxWithLoss" bottom: "fc" '
        f'bottom: "in1" top: "loss" }}']
    head = (f'name: "fz"\nforce_backward: true\n'
            f'layer {{ name: "input" type: "Input" top: "in0" '
            f'top: "in1" input_param {{ '
            f'shape {{ dim: {n} dim: {c} dim: {hw} dim: {hw} }} '
            f'shape {{ dim: {n} }} }} }}\n')
    return head + "\n".join(lines), (n, c, hw)


SEEDS = [5, 19, 42, 77, 101, 137]


def test_fuzz_seeds_plan_every_in_place_fusion():
    # what the seeds are for: between them the generated graphs fuse a ReLU
    # into a BN, a conv and a sum, and a residual add into a BN, and one
    # of them holds a residual block that must not fuse its add
    ca.set_mode("cpu")
    kinds, unfused_add = set(), False
    for seed in SEEDS:
        text, _ = gen_graph(np.random.default_rng(seed))
        mine = [k for k, _, _ in net_from_text(text).fusions()]
        kinds |= set(mine)
        unfused_add |= mine.count("sum_relu") > mine.count("bn_add")
    assert kinds == {"bn_relu", "conv_relu", "sum_relu", "bn_add"}
    assert unfused_add


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_graph_fusion_parity(seed, dtype):
    # tol: exact-class for f32, the bf16 mixed-precision class otherwise
    tol = 1e-3 if dtype == "f32" else 4e-2
    rng = np.random.default_rng(seed)
    text, (n, c, hw) = gen_graph(rng)
    x = rng.standard_normal((n, c, hw, hw)).astype(np.float32)
    labels = rng.integers(0, 4, n).astype(np.float32)
    results = {}
    try:
        for mode in ("cpu", "gpu"):
            ca.set_mode(mode)
            if mode == "gpu":
                ca.set_compute(dtype)
            ca.set_random_seed(1000 + seed)
            net = net_from_text(text)
            net.set_blob("in0", x)
            net.set_blob("in1", labels)
            net.forward()
            net.backward()
            results[mode] = (
                float(np.asarray(net.blob("loss")).ravel()[0]),
                np.asarray(net.blob("in0", diff=True)).copy(),
                [np.asarray(net.param(i, diff=True)).copy()
                 for i in range(net.num_params())])
    finally:
        ca.set_compute("f32")
    lc, dc, pc = results["cpu"]
    lg, dg, pg = results["gpu"]
    assert abs(lg - lc) < tol * max(1.0, abs(lc)), (lc, lg)
    scale = max(np.abs(dc).max(), 1e-3)
    assert np.abs(dg - dc).max() < tol * scale
    for i, (a, b) in enumerate(zip(pc, pg)):
        s = max(np.abs(a).max(), 1e-3)
        assert np.abs(b - a).max() < tol * s, f"param {i}"


# eltwise-class launches (add3, axpby, copy, ... of one forward + backward)
# of the hand graphs as measured on a parent commit on the MI355X: the first
# eight on b1ffb37, when the fusion flags moved from two passes in Net::init
# to a plan, the others on 69f1c0a, when the diff sharing moved from the
# Eltwise and Split backward to a plan.  What the GPU launches for a graph
# must not move with either, but for one copy per "copy" entry of the diff
# sharing plan, where the parent shared memory that was still to be read.
PARENT_ELTWISE_LAUNCHES = {
    "bn_relu": 0, "conv_relu": 0, "residual": 1, "residual_bn_second": 1,
    "residual_relu_out": 1, "leaky_relu": 0, "conv_between": 2,
    "sum_twice": 3,
    "bn_relu_out_of_place": 0, "bn_out_twice": 4, "coeff_half": 5,
    "three_bottoms": 6, "in_place_bn": 3, "test_phase": 2,
    "in_place_bn_shortcut_second": 3, "in_place_relu_bottom": 2,
    "bn_relu_bottom": 2, "three_bottoms_in_place": 7, "flatten_into_sum": 2,
    "single_top_split": 0, "single_top_split_after_flatten": 0,
}

# every hand graph but `prod`, which builds in CPU mode only
HAND_GRAPHS = [
    "bn_relu", "conv_relu", "residual", "residual_bn_second",
    "residual_relu_out", "leaky_relu", "bn_relu_out_of_place",
    "conv_between", "bn_out_twice", "sum_twice", "coeff_half",
    "three_bottoms", "in_place_bn", "test_phase",
    "in_place_bn_shortcut_second", "in_place_relu_bottom", "bn_relu_bottom",
    "three_bottoms_in_place", "flatten_into_sum", "single_top_split",
    "single_top_split_after_flatten",
]


@pytest.mark.parametrize("name", HAND_GRAPHS)
def test_hand_graph_launches_and_parity(name):
    import fusion_graphs as fg
    text, phase, expected = fg.all_graphs()[name]
    rng = np.random.default_rng(11)
    x = rng.standard_normal(fg.SHAPE).astype(np.float32)
    labels = rng.integers(0, 4, fg.SHAPE[0]).astype(np.float32)
    results = {}
    for mode in ("cpu", "gpu"):
        ca.set_mode(mode)
        ca.set_random_seed(2024)
        net = net_from_text(text, phase=phase)
        assert net.fusions() == expected
        assert net.diff_sharing() == fg.DIFF_SHARING[name]
        net.set_blob("in0", x)
        net.set_blob("in1", labels)
        ca.device_synchronize()
        ca.perf_reset()
        net.forward()
        net.backward()
        ca.device_synchronize()
        perf = ca.perf_snapshot()
        results[mode] = (
            float(np.asarray(net.blob("loss")).ravel()[0]),
            np.asarray(net.blob("in0", diff=True)).copy(),
            [np.asarray(net.param(i, diff=True)).copy()
             for i in range(net.num_params())])
    relu = perf.get("relu", {}).get("launches", 0)
    eltwise = perf.get("eltwise", {}).get("launches", 0)
    copies = [d for _, _, d in fg.DIFF_SHARING[name]].count("copy")
    print(f"{name}: relu launches {relu}, eltwise launches {eltwise}, "
          f"{copies} of them planned copies")
    assert relu == fg.relu_launches(expected)
    assert eltwise == PARENT_ELTWISE_LAUNCHES[name] + copies
    lc, dc, pc = results["cpu"]
    lg, dg, pg = results["gpu"]
    tol = 1e-3
    assert abs(lg - lc) < tol * max(1.0, abs(lc)), (lc, lg)
    assert np.abs(dg - dc).max() < tol * max(np.abs(dc).max(), 1e-3)
    for i, (a, b) in enumerate(zip(pc, pg)):
        assert np.abs(b - a).max() < tol * max(np.abs(a).max(), 1e-3), \
            f"param {i}"


def test_eltwise_prod_is_an_error_in_gpu_mode():
    # PROD runs in CPU mode only; with no GPU kernel for it, building the
    # net in GPU mode fails by name instead of computing it somewhere else
    import fusion_graphs as fg
    ca.set_mode("gpu")
    try:
        net_from_text(fg.NEGATIVE["prod"][1])
        raise AssertionError("expected Eltwise PROD to be refused")
    except ca.CaffeError as e:
        assert "PROD has no GPU kernel" in str(e), str(e)
        assert "[in layer 'e1' (Eltwise) SetUp]" in str(e), str(e)
    finally:
        ca.set_mode("cpu")
