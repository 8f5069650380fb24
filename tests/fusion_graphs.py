"""Hand-written graphs for the two build-time plans of a net, the graph
fusions (Net.fusions()) and the gradient-buffer sharing (Net.diff_sharing()),
shared by tests/test_fusion_plan.py and tests/test_diff_sharing_plan.py (the
plans, without a GPU) and tests/test_gpu_graph_fuzz.py (what the GPU
launches for them).

Every graph reads an Input of 2x4x8x8 (in0) with labels (in1), is closed by
InnerProduct + SoftmaxWithLoss and holds exactly one ReLU.  Layer names:
c1 conv, b1 BatchNorm, s1 / s2 shortcut 1x1 convs, e1 the sum, r1 the ReLU,
e2 / x1 extra consumers, f1 / f2 Flatten, sp an explicit Split.
"""

SHAPE = (2, 4, 8, 8)


def conv(name, bottom, top, k=3):
    return (f'layer {{ name: "{name}" type: "Convolution" bottom: "{bottom}" '
            f'top: "{top}" convolution_param {{ num_output: 4 '
            f'kernel_size: {k} pad: {k // 2} '
            f'weight_filler {{ type: "gaussian" std: 0.3 }} '
            f'bias_filler {{ type: "gaussian" std: 0.1 }} }} }}')


def bn(name, bottom, top):
    return (f'layer {{ name: "{name}" type: "BatchNorm" bottom: "{bottom}" '
            f'top: "{top}" batch_norm_param {{ scale_bias: true }} }}')


def relu(name, bottom, top, slope=None):
    p = "" if slope is None else f" relu_param {{ negative_slope: {slope} }}"
    return (f'layer {{ name: "{name}" type: "ReLU" bottom: "{bottom}" '
            f'top: "{top}"{p} }}')


def elt(name, bottoms, top, param="operation: SUM"):
    bs = " ".join(f'bottom: "{b}"' for b in bottoms)
    return (f'layer {{ name: "{name}" type: "Eltwise" {bs} top: "{top}" '
            f'eltwise_param {{ {param} }} }}')


def flatten(name, bottom, top):
    return (f'layer {{ name: "{name}" type: "Flatten" bottom: "{bottom}" '
            f'top: "{top}" }}')


def split(name, bottom, top):
    return (f'layer {{ name: "{name}" type: "Split" bottom: "{bottom}" '
            f'top: "{top}" }}')


def net(layers, out):
    n, c, h, w = SHAPE
    head = (f'name: "fp"\nforce_backward: true\n'
            f'layer {{ name: "input" type: "Input" top: "in0" top: "in1" '
            f'input_param {{ shape {{ dim: {n} dim: {c} dim: {h} dim: {w} }} '
            f'shape {{ dim: {n} }} }} }}\n')
    tail = [
        f'layer {{ name: "ip" type: "InnerProduct" bottom: "{out}" '
        f'top: "fc" inner_product_param {{ num_output: 4 '
        f'weight_filler {{ type: "gaussian" std: 0.2 }} }} }}',
        'layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc" '
        'bottom: "in1" top: "loss" }']
    return head + "\n".join(list(layers) + tail) + "\n"


def residual(e1_bottoms=("b", "s"), e1_param="operation: SUM", r1=None,
             after=()):
    """shortcut conv first, then Conv -> BN -> SUM(bn, shortcut) -> ReLU"""
    r1 = r1 or relu("r1", "e", "e")
    out = "g" if after else ("f" if 'top: "f"' in r1 else "e")
    return net([conv("s1", "in0", "s", k=1), conv("c1", "in0", "a"),
                bn("b1", "a", "b"), elt("e1", e1_bottoms, "e", e1_param),
                r1, *after], out)


# name -> (prototxt, phase, expected Net.fusions())
POSITIVE = {
    "bn_relu": (net([conv("c1", "in0", "a"), bn("b1", "a", "b"),
                     relu("r1", "b", "b")], "b"), 0,
                [("bn_relu", "b1", ["r1"])]),
    "conv_relu": (net([conv("c1", "in0", "a"), relu("r1", "a", "a")], "a"), 0,
                  [("conv_relu", "c1", ["r1"])]),
    "residual": (residual(), 0,
                 [("bn_add", "b1", ["e1"]), ("sum_relu", "e1", ["r1"])]),
    "residual_bn_second": (residual(e1_bottoms=("s", "b")), 0,
                           [("bn_add", "b1", ["e1"]),
                            ("sum_relu", "e1", ["r1"])]),
    "residual_relu_out": (residual(r1=relu("r1", "e", "f")), 0,
                          [("bn_add_relu", "b1", ["e1", "r1"])]),
}

# name -> (the positive graph it differs from in one property, prototxt,
#          phase, expected Net.fusions())
NEGATIVE = {
    "leaky_relu": ("bn_relu",
                   net([conv("c1", "in0", "a"), bn("b1", "a", "b"),
                        relu("r1", "b", "b", slope=0.1)], "b"), 0, []),
    "bn_relu_out_of_place": ("bn_relu",
                             net([conv("c1", "in0", "a"), bn("b1", "a", "b"),
                                  relu("r1", "b", "f")], "f"), 0, []),
    # the shortcut conv sits between the BN and the sum
    "conv_between": ("residual",
                     net([conv("c1", "in0", "a"), bn("b1", "a", "b"),
                          conv("s1", "in0", "s", k=1),
                          elt("e1", ("b", "s"), "e"), relu("r1", "e", "e")],
                         "e"), 0,
                     [("sum_relu", "e1", ["r1"])]),
    # a second consumer of the BN output (which puts a Split behind the BN)
    "bn_out_twice": ("residual",
                     residual(after=[elt("e2", ("e", "b"), "g")]), 0,
                     [("sum_relu", "e1", ["r1"])]),
    # a second consumer of the sum: the out-of-place ReLU stays on its own
    "sum_twice": ("residual_relu_out",
                  residual(r1=relu("r1", "e", "f"),
                           after=[elt("e2", ("f", "e"), "g")]), 0,
                  [("bn_add", "b1", ["e1"])]),
    "coeff_half": ("residual",
                   residual(e1_param="operation: SUM coeff: 1 coeff: 0.5"),
                   0, []),
    "prod": ("residual", residual(e1_param="operation: PROD"), 0, []),
    "three_bottoms": ("residual",
                      net([conv("s1", "in0", "s", k=1),
                           conv("s2", "in0", "t", k=1),
                           conv("c1", "in0", "a"), bn("b1", "a", "b"),
                           elt("e1", ("b", "s", "t"), "e"),
                           relu("r1", "e", "e")], "e"), 0, []),
    "in_place_bn": ("residual",
                    net([conv("s1", "in0", "s", k=1), conv("c1", "in0", "a"),
                         bn("b1", "a", "a"), elt("e1", ("a", "s"), "e"),
                         relu("r1", "e", "e")], "e"), 0,
                    [("sum_relu", "e1", ["r1"])]),
    "test_phase": ("residual", residual(), 1, [("sum_relu", "e1", ["r1"])]),
}

# the positive graphs with nothing to fuse: every ReLU out of place and the
# shortcut conv between the BN and the sum.  Same layers, same names, so
# the weights of a positive graph can be copied over by name.
UNFUSED_TWIN = {
    "bn_relu": NEGATIVE["bn_relu_out_of_place"][1],
    "conv_relu": net([conv("c1", "in0", "a"), relu("r1", "a", "f")], "f"),
    "residual": net([conv("c1", "in0", "a"), bn("b1", "a", "b"),
                     conv("s1", "in0", "s", k=1),
                     elt("e1", ("b", "s"), "e"), relu("r1", "e", "f")], "f"),
}
UNFUSED_TWIN["residual_bn_second"] = UNFUSED_TWIN["residual"].replace(
    'bottom: "b" bottom: "s"', 'bottom: "s" bottom: "b"')
UNFUSED_TWIN["residual_relu_out"] = UNFUSED_TWIN["residual"]


# Graphs for the diff-sharing plan: an in-place layer, a Flatten or a
# one-top Split next to a unit sum.  name -> (prototxt, phase, expected
# Net.fusions())
SHARING = {
    # in_place_bn with the shortcut conv after the in-place BN
    "in_place_bn_shortcut_second": (
        net([conv("c1", "in0", "a"), bn("b1", "a", "a"),
             conv("s1", "in0", "s", k=1), elt("e1", ("a", "s"), "e"),
             relu("r1", "e", "e")], "e"), 0, [("sum_relu", "e1", ["r1"])]),
    "in_place_relu_bottom": (
        net([conv("s1", "in0", "s", k=1), conv("c1", "in0", "a"),
             relu("r1", "a", "a"), elt("e1", ("a", "s"), "e")], "e"), 0,
        [("conv_relu", "c1", ["r1"])]),
    "bn_relu_bottom": (
        net([conv("s1", "in0", "s", k=1), conv("c1", "in0", "a"),
             bn("b1", "a", "b"), relu("r1", "b", "b"),
             elt("e1", ("b", "s"), "e")], "e"), 0,
        [("bn_relu", "b1", ["r1"])]),
    "three_bottoms_in_place": (
        net([conv("s1", "in0", "s", k=1), conv("s2", "in0", "t", k=1),
             conv("c1", "in0", "a"), bn("b1", "a", "a"),
             elt("e1", ("a", "s", "t"), "e"), relu("r1", "e", "e")], "e"),
        0, []),
    "flatten_into_sum": (
        net([conv("s1", "in0", "s", k=1), conv("c1", "in0", "a"),
             flatten("f1", "a", "fa"), flatten("f2", "s", "fs"),
             elt("e1", ("fa", "fs"), "e"), relu("r1", "e", "e")], "e"), 0,
        [("sum_relu", "e1", ["r1"])]),
    "single_top_split": (
        net([conv("c1", "in0", "a"), split("sp", "a", "a1"),
             relu("r1", "a1", "f")], "f"), 0, []),
    "single_top_split_after_flatten": (
        net([conv("c1", "in0", "a"), flatten("f1", "a", "fa"),
             split("sp", "fa", "fb"), relu("r1", "fb", "f")], "f"), 0, []),
}


def _alias(layer, *bottoms):
    return [(layer, b, "alias") for b in bottoms]


# name -> expected Net.diff_sharing(), for every graph above.  Written from
# the rule ("Gradient-buffer sharing"): an entry per propagating
# bottom of a unit sum or a one-top Split; "copy" where a layer in place on
# the bottom writes its gradient at or above the producer of another bottom
# of the same layer (a ReLU absorbed by a bn_relu fusion writes nothing),
# and for the top of a Flatten; "alias" otherwise.
DIFF_SHARING = {
    "bn_relu": [], "conv_relu": [], "leaky_relu": [],
    "bn_relu_out_of_place": [], "coeff_half": [], "prod": [],
    "residual": _alias("e1", "b", "s"),
    "residual_bn_second": _alias("e1", "s", "b"),
    "residual_relu_out": _alias("e1", "b", "s"),
    "test_phase": _alias("e1", "b", "s"),
    "conv_between": _alias("e1", "b", "s"),
    "three_bottoms": _alias("e1", "b", "s", "t"),
    # the Split of e behind e1 has two tops and is not in the plan
    "sum_twice": _alias("e1", "b", "s") + _alias("e2", "f", "e_split_1"),
    # b1 (in place on a) runs its backward before s1, which reads s
    "in_place_bn": [("e1", "a", "copy"), ("e1", "s", "alias")],
    # r1 is in place on e, only its forward is fused, and it sits above
    # the Split that produces b_split_1
    "bn_out_twice": (_alias("e1", "b_split_0", "s") +
                     [("e2", "e", "copy"), ("e2", "b_split_1", "alias")]),
    # the shortcut conv after the BN: s1 has read s by the time b1 writes
    "in_place_bn_shortcut_second": _alias("e1", "a", "s"),
    "in_place_relu_bottom": [("e1", "a", "copy"), ("e1", "s", "alias")],
    # b1 absorbed r1's backward: nothing writes b's gradient in place
    "bn_relu_bottom": _alias("e1", "b", "s"),
    "three_bottoms_in_place": ([("e1", "a", "copy")] +
                               _alias("e1", "s", "t")),
    "flatten_into_sum": [("e1", "fa", "copy"), ("e1", "fs", "copy")],
    "single_top_split": _alias("sp", "a"),
    "single_top_split_after_flatten": [("sp", "fa", "copy")],
}


def all_graphs():
    """name -> (prototxt, phase, expected Net.fusions()) of every graph"""
    out = dict(POSITIVE)
    out.update({n: v[1:] for n, v in NEGATIVE.items()})
    out.update(SHARING)
    return out


def relu_launches(fusions):
    """relu-class launches of one forward + backward of a graph with one
    ReLU: none when a BN absorbed both directions, the backward alone when
    only the forward was absorbed, both otherwise."""
    for kind, _, absorbed in fusions:
        if "r1" in absorbed:
            return 0 if kind == "bn_relu" else 1
    return 2
