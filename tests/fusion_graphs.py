"""Hand-written graphs for the graph-fusion plan (Net.fusions()), shared by
tests/test_fusion_plan.py (the plan, without a GPU) and
tests/test_gpu_graph_fuzz.py (what the GPU launches for it).

Every graph reads an Input of 2x4x8x8 (in0) with labels (in1), is closed by
InnerProduct + SoftmaxWithLoss and holds exactly one ReLU.  Layer names:
c1 conv, b1 BatchNorm, s1 / s2 shortcut 1x1 convs, e1 the sum, r1 the ReLU,
e2 / x1 extra consumers.
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


def relu_launches(fusions):
    """relu-class launches of one forward + backward of a graph with one
    ReLU: none when a BN absorbed both directions, the backward alone when
    only the forward was absorbed, both otherwise."""
    for kind, _, absorbed in fusions:
        if "r1" in absorbed:
            return 0 if kind == "bn_relu" else 1
    return 2
