"""Layer-level parity checks: engine (CPU or GPU mode) vs oracle/.

Each check builds a one-layer net through the engine's own prototxt path,
drives it with seeded inputs, and compares every output and gradient with
the oracle at 1e-4 relative fp32 (the reference's own tolerance class,
test_convolution_layer.cpp:247).  Used by test_engine_cpu.py (CPU mode,
runs everywhere) and test_gpu_parity.py (@gpu, MI355X).
"""
import numpy as np

from engine_util import TOL, relerr, run_layer
from oracle import oracle as orc

rng = np.random.default_rng(20250915)


def round_bf16(a):
    """float32 -> nearest bfloat16 (ties to even) -> float32, in numpy (the
    engine's tests never import torch, see conftest.py)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    u = (u + (((u >> 16) & 1) + 0x7FFF)) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def check_conv(mode, N=2, C=8, H=13, W=13, Co=16, k=3, s=1, p=1, grp=1,
               bias=True, d=1, quant=None, errs=None):
    """quant: applied to x, w, b and dy before both the engine and the
    oracle see them (e.g. round_bf16).  errs: a dict that receives the
    measured relerr of y / dx / dw / db before each is asserted."""
    quant = quant or (lambda a: a)
    errs = {} if errs is None else errs
    x = quant(rng.standard_normal((N, C, H, W)).astype(np.float32))
    w = quant(
        (rng.standard_normal((Co, C // grp, k, k)) * 0.2).astype(np.float32))
    b = quant(rng.standard_normal(Co).astype(np.float32)) if bias else None
    body = f"""layer {{
  name: "conv"
  type: "Convolution"
  bottom: "in0"
  top: "out"
  convolution_param {{
    num_output: {Co}
    kernel_size: {k}
    stride: {s}
    pad: {p}
    group: {grp}
    dilation: {d}
    bias_term: {"true" if bias else "false"}
  }}
}}"""
    y_ref = orc.conv_fwd(x, w, b, pad=(p, p), stride=(s, s), dil=(d, d),
                         group=grp)
    dy = quant(rng.standard_normal(y_ref.shape).astype(np.float32))
    net, y = run_layer(mode, [(N, C, H, W)], body, [x],
                       params=[w, b] if bias else [w], top_diff=dy)
    errs["y"] = relerr(y, y_ref)
    assert errs["y"] < TOL, f"conv fwd {errs['y']}"
    dx_ref, dw_ref, db_ref = orc.conv_bwd(x, w, dy, pad=(p, p),
                                          stride=(s, s), dil=(d, d),
                                          group=grp, want_db=bias)
    errs["dx"] = relerr(net.blob("in0", diff=True), dx_ref)
    assert errs["dx"] < TOL, f"conv dx {errs['dx']}"
    errs["dw"] = relerr(net.param(0, diff=True), dw_ref.ravel())
    assert errs["dw"] < TOL, f"conv dw {errs['dw']}"
    if bias:
        errs["db"] = relerr(net.param(1, diff=True), db_ref)
        assert errs["db"] < TOL, f"conv db {errs['db']}"


def check_conv_relu(mode, N=2, C=8, H=13, W=13, Co=16, k=3, s=1, p=1,
                    errs=None):
    """Conv with bias followed by an in-place ReLU (in GPU mode the net
    folds the ReLU into the GEMM epilogue): y against relu(oracle conv),
    dx / dW against the oracle's conv backward of dy * (y > 0).  dy is
    zeroed where the pre-activation lies within 1e-3 of 0, so a sign that
    legitimately differs in the last fp32 bits cannot move a gradient."""
    errs = {} if errs is None else errs
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    w = (rng.standard_normal((Co, C, k, k)) * 0.2).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    body = f"""layer {{
  name: "conv"
  type: "Convolution"
  bottom: "in0"
  top: "out"
  convolution_param {{
    num_output: {Co} kernel_size: {k} stride: {s} pad: {p}
  }}
}}
layer {{ name: "relu" type: "ReLU" bottom: "out" top: "out" }}"""
    pre = orc.conv_fwd(x, w, b, pad=(p, p), stride=(s, s))
    y_ref = np.maximum(pre, 0)
    dy = rng.standard_normal(pre.shape).astype(np.float32)
    dy[np.abs(pre) < 1e-3] = 0
    net, y = run_layer(mode, [(N, C, H, W)], body, [x], params=[w, b],
                       top_diff=dy)
    errs["y"] = relerr(y, y_ref)
    assert errs["y"] < TOL, f"conv+relu fwd {errs['y']}"
    assert np.asarray(y).min() >= 0
    dpre = (dy * (pre > 0)).astype(np.float32)
    dx_ref, dw_ref, db_ref = orc.conv_bwd(x, w, dpre, pad=(p, p),
                                          stride=(s, s), want_db=True)
    errs["dx"] = relerr(net.blob("in0", diff=True), dx_ref)
    assert errs["dx"] < TOL, f"conv+relu dx {errs['dx']}"
    errs["dw"] = relerr(net.param(0, diff=True), dw_ref.ravel())
    assert errs["dw"] < TOL, f"conv+relu dw {errs['dw']}"
    errs["db"] = relerr(net.param(1, diff=True), db_ref)
    assert errs["db"] < TOL, f"conv+relu db {errs['db']}"


def check_ip(mode, M=4, K=32, Nout=10, errs=None):
    errs = {} if errs is None else errs
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = rng.standard_normal((Nout, K)).astype(np.float32) * 0.2
    w = w.astype(np.float32)
    b = rng.standard_normal(Nout).astype(np.float32)
    body = f"""layer {{
  name: "ip"
  type: "InnerProduct"
  bottom: "in0"
  top: "out"
  inner_product_param {{ num_output: {Nout} }}
}}"""
    y_ref = orc.ip_fwd(x, w, b)
    dy = rng.standard_normal(y_ref.shape).astype(np.float32)
    net, y = run_layer(mode, [(M, K)], body, [x], params=[w, b],
                       top_diff=dy)
    errs["y"] = relerr(y, y_ref)
    assert errs["y"] < TOL, f"ip fwd {errs['y']}"
    dx_ref, dw_ref, db_ref = orc.ip_bwd(x, w, dy)
    errs["dx"] = relerr(net.blob("in0", diff=True), dx_ref)
    assert errs["dx"] < TOL, f"ip dx {errs['dx']}"
    errs["dw"] = relerr(net.param(0, diff=True), dw_ref.ravel())
    assert errs["dw"] < TOL, f"ip dw {errs['dw']}"
    errs["db"] = relerr(net.param(1, diff=True), db_ref)
    assert errs["db"] < TOL, f"ip db {errs['db']}"


def check_pool(mode, pool="MAX", N=2, C=4, H=13, W=13, k=3, s=2, p=0):
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    body = f"""layer {{
  name: "pool"
  type: "Pooling"
  bottom: "in0"
  top: "out"
  pooling_param {{ pool: {pool} kernel_size: {k} stride: {s} pad: {p} }}
}}"""
    if pool == "MAX":
        y_ref, mask = orc.pool_max_fwd(x, k, k, p, p, s, s)
    else:
        y_ref = orc.pool_ave_fwd(x, k, k, p, p, s, s)
    dy = rng.standard_normal(y_ref.shape).astype(np.float32)
    net, y = run_layer(mode, [(N, C, H, W)], body, [x], top_diff=None)
    assert relerr(y, y_ref) < TOL
    # pooling has no params; drive backward through an explicit top diff —
    # pooling's prop_down is False in a net without params below, so check
    # via a conv underneath instead? Simpler: pooling alone won't backprop.
    # Covered at full-net level; here forward only.
    if pool == "MAX":
        _ = mask


def check_pool_bwd(mode, pool="MAX", N=2, C=4, H=13, W=13, k=3, s=2,
                   p=0, kernel_h=None, kernel_w=None, stride_h=None,
                   stride_w=None, pad_h=None, pad_w=None, x=None, errs=None):
    """kernel_h/w, stride_h/w, pad_h/w: per-axis geometry (each defaults to
    k / s / p; giving any of them writes the per-axis prototxt fields).
    x: the input, when the caller needs a particular one (e.g. full of
    ties).  errs receives the measured relerr of y / dx before each is
    asserted.  Returns x, dy, the oracle's mask (MAX) and dx, and the
    engine's dx, for checks beyond the relerr bound."""
    errs = {} if errs is None else errs
    per_axis = any(v is not None for v in (kernel_h, kernel_w, stride_h,
                                           stride_w, pad_h, pad_w))
    kh = k if kernel_h is None else kernel_h
    kw = k if kernel_w is None else kernel_w
    sh = s if stride_h is None else stride_h
    sw = s if stride_w is None else stride_w
    ph = p if pad_h is None else pad_h
    pw = p if pad_w is None else pad_w
    geom = (f"kernel_h: {kh} kernel_w: {kw} stride_h: {sh} stride_w: {sw} "
            f"pad_h: {ph} pad_w: {pw}" if per_axis
            else f"kernel_size: {k} stride: {s} pad: {p}")
    # pool preceded by a 1x1 conv so prop_down[0] is true
    if x is None:
        x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    assert x.shape == (N, C, H, W) and x.dtype == np.float32
    w = np.eye(C, dtype=np.float32).reshape(C, C, 1, 1).copy()
    body = f"""layer {{
  name: "c1"
  type: "Convolution"
  bottom: "in0"
  top: "mid"
  convolution_param {{ num_output: {C} kernel_size: 1 bias_term: false }}
}}
layer {{
  name: "pool"
  type: "Pooling"
  bottom: "mid"
  top: "out"
  pooling_param {{ pool: {pool} {geom} }}
}}"""
    mask = None
    if pool == "MAX":
        y_ref, mask = orc.pool_max_fwd(x, kh, kw, ph, pw, sh, sw)
    else:
        y_ref = orc.pool_ave_fwd(x, kh, kw, ph, pw, sh, sw)
    dy = rng.standard_normal(y_ref.shape).astype(np.float32)
    net, y = run_layer(mode, [(N, C, H, W)], body, [x], params=[w],
                       top_diff=dy)
    errs["y"] = relerr(y, y_ref)
    assert errs["y"] < TOL, f"pool {pool} fwd {errs['y']}"
    if pool == "MAX":
        dx_ref = orc.pool_max_bwd(dy, mask, H, W)
    else:
        dx_ref = orc.pool_ave_bwd(dy, H, W, kh, kw, ph, pw, sh, sw)
    # dx lands in "mid"'s diff == conv's top diff; identity conv passes it on
    dx = net.blob("mid", diff=True)
    errs["dx"] = relerr(dx, dx_ref)
    assert errs["dx"] < TOL, f"pool {pool} dx {errs['dx']}"
    return dict(x=x, dy=dy, mask=mask, dx_ref=dx_ref, dx=dx)


def bn_inputs(r, N, C, H, W, mean=0.0, std=1.0):
    """check_bn's x, scale, bias and dy, drawn from the generator r."""
    x = r.standard_normal((N, C, H, W)).astype(np.float32)
    if mean != 0.0 or std != 1.0:
        x = (x * np.float32(std) + np.float32(mean)).astype(np.float32)
    sc = (r.standard_normal(C) + 1.5).astype(np.float32)
    bi = r.standard_normal(C).astype(np.float32)
    dy = r.standard_normal(x.shape).astype(np.float32)
    return x, sc, bi, dy


def check_bn(mode, N=4, C=6, H=5, W=5, scale_bias=True, mean=0.0, std=1.0,
             eps=1e-4, seed=None, errs=None, relu=False):
    """mean, std: of the normal input.  seed: draw the inputs from a
    generator of their own, bn_inputs(default_rng(seed), ...), so that a
    test can restate them.  errs receives the measured relerr of y / dx /
    dscale / dbias before each is asserted.

    relu: an in-place ReLU follows on "out" (in GPU mode the net folds it
    into the BN kernels, forward and backward; in CPU mode it runs as a
    layer).  The reference is max(y_ref, 0), and the oracle's backward gets
    dy zeroed where y_ref <= 0.  The oracle's y must stay 5e-5 clear of 0
    (the fp32 forward is within about 1.5e-6 of it), so that no sign can
    differ between the fp32 and the fp64 forward.

    The default input (unit variance, eps 1e-4) cannot see eps: the oracle
    with eps = 0 differs from the true output by relerr 3.7e-5, below TOL.
    test_kernel_variants.py adds a std 0.01 case, where it gives 0.42."""
    errs = {} if errs is None else errs
    x, sc, bi, dy = bn_inputs(rng if seed is None
                              else np.random.default_rng(seed),
                              N, C, H, W, mean, std)
    body = f"""layer {{
  name: "bn"
  type: "BatchNorm"
  bottom: "in0"
  top: "out"
  batch_norm_param {{
    moving_average_fraction: 0.9
    eps: {eps}
    scale_bias: {"true" if scale_bias else "false"}
  }}
}}"""
    if relu:
        body += '\nlayer { name: "relu" type: "ReLU" bottom: "out" top: "out" }'
    y_ref, _, _, inv_std, xnorm = orc.bn_fwd_train(
        x, eps, sc if scale_bias else None, bi if scale_bias else None)
    if relu:
        assert np.abs(y_ref).min() >= 5e-5, np.abs(y_ref).min()
        # the engine gets the whole dy: masking it is the ReLU's work
        dy_ref = np.where(y_ref <= 0, 0, dy).astype(np.float32)
        y_ref = np.maximum(y_ref, 0)
    else:
        dy_ref = dy
    # learnable params of BN are [scale, bias] (stats blobs skipped)
    params = [sc, bi] if scale_bias else None
    net, y = run_layer(mode, [(N, C, H, W)], body, [x], params=params,
                       top_diff=dy)
    errs["y"] = relerr(y, y_ref)
    assert errs["y"] < TOL, f"bn fwd {errs['y']}"
    dx_ref, dsc_ref, dbi_ref = orc.bn_bwd(xnorm, dy_ref, inv_std,
                                          sc if scale_bias else None)
    errs["dx"] = relerr(net.blob("in0", diff=True), dx_ref)
    assert errs["dx"] < TOL, f"bn dx {errs['dx']}"
    if scale_bias:
        # learnable params (arena order): scale=idx 0, bias=idx 1 of this
        # layer; BN stats blobs are skipped (skip_apply_update)
        errs["dscale"] = relerr(net.param(0, diff=True), dsc_ref)
        assert errs["dscale"] < TOL, f"bn dscale {errs['dscale']}"
        errs["dbias"] = relerr(net.param(1, diff=True), dbi_ref)
        assert errs["dbias"] < TOL, f"bn dbias {errs['dbias']}"


def check_relu(mode, n=1000, shape=(2, 5, 10, 10), negative_slope=0.0,
               errs=None):
    errs = {} if errs is None else errs
    C = shape[1]
    x = rng.standard_normal(shape).astype(np.float32)
    rp = (f" relu_param {{ negative_slope: {negative_slope} }}"
          if negative_slope else "")
    body = f"""layer {{
  name: "c1"
  type: "Convolution"
  bottom: "in0"
  top: "mid"
  convolution_param {{ num_output: {C} kernel_size: 1 bias_term: false }}
}}
layer {{ name: "r" type: "ReLU" bottom: "mid" top: "out"{rp} }}"""
    w = np.eye(C, dtype=np.float32).reshape(C, C, 1, 1).copy()
    y_ref = orc.relu_fwd(x, negative_slope)
    dy = rng.standard_normal(x.shape).astype(np.float32)
    net, y = run_layer(mode, [x.shape], body, [x], params=[w], top_diff=dy)
    errs["y"] = relerr(y, y_ref)
    assert errs["y"] < TOL, f"relu fwd {errs['y']}"
    errs["dx"] = relerr(net.blob("mid", diff=True),
                        orc.relu_bwd(x, dy, negative_slope))
    assert errs["dx"] < TOL, f"relu dx {errs['dx']}"


def lrn_inputs(r, N, C, H, W):
    """check_lrn's x and dy, drawn from the generator r."""
    x = r.standard_normal((N, C, H, W)).astype(np.float32)
    dy = r.standard_normal(x.shape).astype(np.float32)
    return x, dy


def check_lrn(mode, N=2, C=8, H=6, W=6, size=5, alpha=1e-4, beta=0.75,
              seed=None, errs=None):
    """seed: as in check_bn, with lrn_inputs.

    The default alpha = 1e-4 on unit-normal input gives scale ~ 1.0001,
    so the case barely sees the window: the oracle with local_size 3 in
    place of 5 differs from the true output by relerr 1.05e-4 forward and
    1.2e-4 backward, and y = x by 1.8e-4, against TOL = 1e-4.
    test_kernel_variants.py runs every LRN shape at alpha = 1.0, where the
    same perturbation gives 0.24."""
    errs = {} if errs is None else errs
    x, dy = lrn_inputs(rng if seed is None else np.random.default_rng(seed),
                       N, C, H, W)
    w = np.eye(C, dtype=np.float32).reshape(C, C, 1, 1).copy()
    body = f"""layer {{
  name: "c1"
  type: "Convolution"
  bottom: "in0"
  top: "mid"
  convolution_param {{ num_output: {C} kernel_size: 1 bias_term: false }}
}}
layer {{
  name: "lrn"
  type: "LRN"
  bottom: "mid"
  top: "out"
  lrn_param {{ local_size: {size} alpha: {alpha} beta: {beta} }}
}}"""
    y_ref, scale = orc.lrn_fwd(x, size, alpha, beta)
    net, y = run_layer(mode, [x.shape], body, [x], params=[w], top_diff=dy)
    errs["y"] = relerr(y, y_ref)
    assert errs["y"] < TOL, f"lrn fwd {errs['y']}"
    dx_ref = orc.lrn_bwd(x, y_ref, dy, scale, size, alpha, beta)
    errs["dx"] = relerr(net.blob("mid", diff=True), dx_ref)
    assert errs["dx"] < TOL, f"lrn dx {errs['dx']}"


def check_softmaxloss(mode, N=8, C=10, errs=None):
    errs = {} if errs is None else errs
    x = (rng.standard_normal((N, C)) * 3).astype(np.float32)
    lab = rng.integers(0, C, N).astype(np.float32)
    body = """layer {
  name: "ip"
  type: "InnerProduct"
  bottom: "in0"
  top: "fc"
  inner_product_param { num_output: %d }
}
layer {
  name: "loss"
  type: "SoftmaxWithLoss"
  bottom: "fc"
  bottom: "in1"
  top: "out"
}""" % C
    w = np.eye(C, dtype=np.float32)
    prob = orc.softmax_fwd(x, N, C, 1)
    loss_ref = orc.softmaxloss_fwd(prob, lab, N, C, 1)
    net, y = run_layer(mode, [(N, C), (N,)], body, [x, lab],
                       params=[w, np.zeros(C, np.float32)])
    errs["loss"] = abs(y[0] - loss_ref) / max(1, abs(loss_ref))
    assert abs(y[0] - loss_ref) < 1e-5 * max(1, abs(loss_ref)), errs["loss"]
    net.backward()
    dx_ref = orc.softmaxloss_bwd(prob, lab, N, C, 1)
    errs["dx"] = relerr(net.blob("fc", diff=True), dx_ref)
    assert errs["dx"] < TOL, f"softmaxloss dx {errs['dx']}"


def check_softmaxloss_spatial(mode, N=2, C=5, H=3, W=4, errs=None):
    errs = {} if errs is None else errs
    # FCN-style spatial loss: inner = H*W > 1 exercises the inner-stride
    # walk of the softmax/NLL kernels (softmax_layer.cu's inner_num_ path)
    x = (rng.standard_normal((N, C, H, W)) * 2).astype(np.float32)
    lab = rng.integers(0, C, (N, H, W)).astype(np.float32)
    inner = H * W
    prob = orc.softmax_fwd(x, N, C, inner)
    loss_ref = orc.softmaxloss_fwd(prob, lab.ravel(), N, C, inner)
    body = """layer {
  name: "loss"
  type: "SoftmaxWithLoss"
  bottom: "in0"
  bottom: "in1"
  top: "out"
}"""
    net, y = run_layer(mode, [(N, C, H, W), (N, H, W)], body, [x, lab])
    errs["loss"] = abs(y.ravel()[0] - loss_ref) / max(1, abs(loss_ref))
    assert abs(y.ravel()[0] - loss_ref) < 1e-5 * max(1, abs(loss_ref)), \
        errs["loss"]
    net.backward()
    dx_ref = orc.softmaxloss_bwd(prob, lab.ravel(), N, C, inner)
    errs["dx"] = relerr(net.blob("in0", diff=True), dx_ref)
    assert errs["dx"] < TOL, f"softmaxloss spatial dx {errs['dx']}"


def check_eltwise_concat(mode):
    N, C, H, W = 2, 4, 5, 5
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    w1 = np.eye(C, dtype=np.float32).reshape(C, C, 1, 1).copy()
    w2 = (np.eye(C) * 2).astype(np.float32).reshape(C, C, 1, 1).copy()
    body = f"""layer {{
  name: "a"
  type: "Convolution"
  bottom: "in0"
  top: "a"
  convolution_param {{ num_output: {C} kernel_size: 1 bias_term: false }}
}}
layer {{
  name: "b"
  type: "Convolution"
  bottom: "in0"
  top: "b"
  convolution_param {{ num_output: {C} kernel_size: 1 bias_term: false }}
}}
layer {{
  name: "sum"
  type: "Eltwise"
  bottom: "a"
  bottom: "b"
  top: "sum"
  eltwise_param {{ operation: SUM }}
}}
layer {{
  name: "cat"
  type: "Concat"
  bottom: "sum"
  bottom: "a"
  top: "out"
}}"""
    dy = rng.standard_normal((N, 2 * C, H, W)).astype(np.float32)
    # learnable order is backward-completion (reverse layers): conv b, conv a
    net, y = run_layer(mode, [x.shape], body, [x], params=[w2, w1],
                       top_diff=dy)
    a, b = x, 2 * x
    y_ref = np.concatenate([a + b, a], axis=1)
    assert relerr(y, y_ref) < TOL
    # backward: d(sum)=dy[:, :C], d(a)=dy[:, :C] (via sum) + dy[:, C:]
    assert relerr(net.blob("sum", diff=True), dy[:, :C]) < TOL
    assert relerr(net.blob("a", diff=True), dy[:, :C] + dy[:, C:]) < TOL
    # in0 diff: conv a contributes 1*d(a), conv b contributes 2*d(sum)
    din_ref = (dy[:, :C] + dy[:, C:]) + 2 * dy[:, :C]
    assert relerr(net.blob("in0", diff=True), din_ref) < TOL


def check_dropout(mode, N=2, C=4, H=7, W=7, ratio=0.4, seed=4242):
    """Dropout TRAIN mask is the engine's counter RNG — restated here from
    core.hpp h_splitmix64/h_u01 and the layer key (layers_cpu.cpp
    Forward_cpu: splitmix64(seed ^ 0xD0D0 ^ rank<<40 ^ data_iter)); CPU and
    GPU must both reproduce it bit-exactly (reference dropout semantics:
    dropout_layer.cpp — mask*scale with scale=1/(1-ratio))."""
    import caffe_amd as ca

    M64 = (1 << 64) - 1

    def smix(v):
        v = (v + 0x9E3779B97F4A7C15) & M64
        v = ((v ^ (v >> 30)) * 0xBF58476D1CE4E5B9) & M64
        v = ((v ^ (v >> 27)) * 0x94D049BB133111EB) & M64
        return v ^ (v >> 31)

    ca.set_mode(mode)
    ca.set_random_seed(seed)
    x = rng.standard_normal((N, C, H, W)).astype(np.float32) + 3.0
    w = np.eye(C, dtype=np.float32).reshape(C, C, 1, 1).copy()
    body = f"""layer {{
  name: "c1"
  type: "Convolution"
  bottom: "in0"
  top: "mid"
  convolution_param {{ num_output: {C} kernel_size: 1 bias_term: false }}
}}
layer {{
  name: "drop"
  type: "Dropout"
  bottom: "mid"
  top: "out"
  dropout_param {{ dropout_ratio: {ratio} }}
}}"""
    dy = rng.standard_normal(x.shape).astype(np.float32)
    net, y = run_layer(mode, [x.shape], body, [x], params=[w], top_diff=dy)
    n = x.size
    # x is offset by +3 so a zero output can only mean "dropped" — recover
    # the mask the layer actually used, then pin it bit-exactly to the
    # restated counter RNG for SOME data_iter (earlier in-process tests may
    # have stepped a solver, so the exact iter is not known here)
    y_arr = np.asarray(y).reshape(x.shape)
    mask_obs = (y_arr != 0).astype(np.float32)

    def mask_for(data_iter):
        key = smix(seed ^ 0xD0D0 ^ data_iter)
        return np.array([
            np.float32((smix(key ^ i) >> 11)
                       * (1.0 / 9007199254740992.0))
            >= np.float32(ratio) for i in range(n)],
            dtype=np.float32).reshape(x.shape)

    matched = any(np.array_equal(mask_for(di), mask_obs)
                  for di in range(256))
    assert matched, "dropout mask does not come from the engine counter RNG"
    scale = np.float32(1.0 / (1.0 - np.float32(ratio)))
    assert relerr(y_arr, x * mask_obs * scale) < TOL, "dropout fwd"
    kept = float(mask_obs.mean())
    assert 0.4 < kept < 0.8, kept  # ratio=0.4 → ~60% kept
    assert relerr(net.blob("mid", diff=True), dy * mask_obs * scale) < TOL
    ca.set_random_seed(1371)  # restore the default for later checks


def check_bn_global(mode, N=4, C=6, H=5, W=5):
    """TEST-phase BN (use-global-stats inference path, batch_norm_layer
    .cpp:154 / layers_gpu.cpp Forward_gpu TEST branch) THROUGH a weights
    round-trip: TRAIN forward populates the moving averages (iter<=1 copy),
    SaveWeights/LoadWeights carries all 5 BN blobs into a TEST-phase net,
    whose output must match the closed-form (x-mean)/sqrt(var+eps)*sc+bi."""
    import tempfile

    from engine_util import input_net, net_from_text

    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    sc = (rng.standard_normal(C) + 1.5).astype(np.float32)
    bi = rng.standard_normal(C).astype(np.float32)
    eps = 1e-3
    body = f"""layer {{
  name: "bn"
  type: "BatchNorm"
  bottom: "in0"
  top: "out"
  batch_norm_param {{ eps: {eps} scale_bias: true }}
}}"""
    net, _ = run_layer(mode, [x.shape], body, [x], params=[sc, bi])
    f = tempfile.NamedTemporaryFile(suffix=".caffemodel", delete=False)
    f.close()
    net.save_weights(f.name)
    net2 = net_from_text(input_net([x.shape], body), phase=1)
    net2.load_weights(f.name)
    net2.set_blob("in0", x)
    net2.forward()
    y = net2.blob("out")
    mean = x.mean(axis=(0, 2, 3))
    var = x.var(axis=(0, 2, 3))  # biased, as the layer computes it
    y_ref = ((x - mean[:, None, None]) / np.sqrt(var + eps)[:, None, None]
             * sc[:, None, None] + bi[:, None, None])
    assert relerr(y, y_ref) < TOL, f"bn inference {relerr(y, y_ref)}"


def check_accuracy(mode, N=12, C=10, top_k=3):
    """Accuracy layer (CPU-resident in both modes, as in the reference —
    accuracy_layer.cpp has no .cu) vs the oracle's restatement."""
    pred = rng.standard_normal((N, C)).astype(np.float32)
    label = rng.integers(0, C, N).astype(np.float32)
    body = f"""layer {{
  name: "acc"
  type: "Accuracy"
  bottom: "in0"
  bottom: "in1"
  top: "out"
  accuracy_param {{ top_k: {top_k} }}
}}"""
    _, y = run_layer(mode, [(N, C), (N,)], body, [pred, label])
    ref = orc.accuracy(pred, label, N, C, 1, top_k)
    assert abs(float(np.asarray(y).ravel()[0]) - ref) < 1e-6
    # top_k=1 via a fresh net on the same data
    body1 = body.replace(f"top_k: {top_k}", "top_k: 1")
    _, y1 = run_layer(mode, [(N, C), (N,)], body1, [pred, label])
    assert abs(float(np.asarray(y1).ravel()[0])
               - orc.accuracy(pred, label, N, C, 1, 1)) < 1e-6


def check_conv_asym(mode, N=2, C=5, H=14, W=11, Co=6, kh=3, kw=5, sh=2,
                    sw=1, ph=1, pw=2):
    # asymmetric kernel/stride/pad (kernel_h != kernel_w): exercises the
    # separate h/w plumbing through im2col / the GemmView walks — a
    # swapped-axis bug is invisible to every square-shape test
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    w = (rng.standard_normal((Co, C, kh, kw)) * 0.2).astype(np.float32)
    body = f"""layer {{
  name: "conv"
  type: "Convolution"
  bottom: "in0"
  top: "out"
  convolution_param {{
    num_output: {Co}
    kernel_h: {kh} kernel_w: {kw}
    stride_h: {sh} stride_w: {sw}
    pad_h: {ph} pad_w: {pw}
    bias_term: false
  }}
}}"""
    y_ref = orc.conv_fwd(x, w, None, pad=(ph, pw), stride=(sh, sw))
    dy = rng.standard_normal(y_ref.shape).astype(np.float32)
    net, y = run_layer(mode, [(N, C, H, W)], body, [x], params=[w],
                       top_diff=dy)
    assert relerr(y, y_ref) < TOL, f"asym fwd {relerr(y, y_ref)}"
    dx_ref, dw_ref, _ = orc.conv_bwd(x, w, dy, pad=(ph, pw),
                                     stride=(sh, sw), want_db=False)
    assert relerr(net.blob("in0", diff=True), dx_ref) < TOL, "asym dx"
    assert relerr(net.param(0, diff=True), dw_ref) < TOL, "asym dw"


ALL_CHECKS = {
    "conv_3x3": lambda m: check_conv(m),
    "conv_asym": check_conv_asym,
    "conv_asym_tall": lambda m: check_conv_asym(m, kh=5, kw=1, sh=1, sw=3,
                                                ph=2, pw=0, H=11, W=16),
    # OW >= 24 so the GPU routes these through the IMPLICIT im2col views
    # (s1 branch / the strided conv1-like branch) with kh != kw
    "conv_asym_implicit": lambda m: check_conv_asym(
        m, kh=3, kw=5, sh=1, sw=1, ph=1, pw=2, H=12, W=26, Co=8),
    "conv_asym_strided_view": lambda m: check_conv_asym(
        m, kh=3, kw=2, sh=2, sw=1, ph=1, pw=0, H=14, W=26, Co=8),
    "conv_7x7s2": lambda m: check_conv(m, C=3, H=19, W=19, Co=8, k=7, s=2,
                                       p=3),
    "conv_1x1": lambda m: check_conv(m, k=1, p=0, bias=False),
    "conv_1x1s2": lambda m: check_conv(m, k=1, p=0, s=2, bias=False),
    "conv_group": lambda m: check_conv(m, C=8, Co=16, k=5, p=2, grp=2),
    # dilation>1 forces the explicit im2col path (implicit GEMM is s1/d1
    # only — layers_gpu.cpp conv policy); reference supports it via
    # conv_param.dilation (caffe.proto:518)
    "conv_3x3_dilated": lambda m: check_conv(m, N=2, C=4, H=15, W=15, Co=8,
                                             k=3, s=1, p=2, d=2),
    "conv_5x5_odd": lambda m: check_conv(m, N=3, C=5, H=11, W=17, Co=7, k=5,
                                         s=3, p=2),
    # implicit-im2col eligible shapes (s1/d1, OW >= 24 on the GPU path):
    # interior fast path + row-crossing boundary chunks + image edges
    "conv_3x3_implicit": lambda m: check_conv(m, N=2, C=4, H=32, W=32, Co=8,
                                              k=3, s=1, p=1),
    "conv_3x3_implicit_odd": lambda m: check_conv(m, N=3, C=3, H=29, W=37,
                                                  Co=6, k=3, s=1, p=1),
    "conv_5x5_implicit_group": lambda m: check_conv(m, N=2, C=8, H=27, W=27,
                                                    Co=16, k=5, s=1, p=2,
                                                    grp=2),
    "conv_7x7_implicit": lambda m: check_conv(m, N=2, C=3, H=30, W=30, Co=8,
                                              k=7, s=1, p=3),
    "conv_11x11s4": lambda m: check_conv(m, N=2, C=3, H=47, W=47, Co=8,
                                         k=11, s=4, p=0),  # AlexNet conv1
    # round 2: STRIDED implicit-im2col views (strides folded into the GEMM
    # staging walk — no im2col/col2im kernels).  Shapes chosen so OW >= 24
    # (kh>1) / OW >= 16 (one-wrap strided walk) to hit each fast path:
    # conv1-style 7x7s2 (strided interior gather + row wraps + dcol-free
    # wgrad), 1x1s2 projection (zero+scatter dgrad), 11x11s4 wide.
    "conv_7x7s2_implicit": lambda m: check_conv(m, N=2, C=3, H=55, W=55,
                                                Co=8, k=7, s=2, p=3),
    "conv_1x1s2_wide": lambda m: check_conv(m, N=2, C=6, H=40, W=40, Co=8,
                                            k=1, s=2, p=0, bias=False),
    "conv_11x11s4_wide": lambda m: check_conv(m, N=2, C=3, H=79, W=79, Co=8,
                                              k=11, s=4, p=0),
    "ip": check_ip,
    "ip_large": lambda m: check_ip(m, M=130, K=260, Nout=140),
    "pool_max": lambda m: check_pool(m, "MAX"),
    "pool_ave": lambda m: check_pool(m, "AVE"),
    "pool_max_bwd": lambda m: check_pool_bwd(m, "MAX"),
    # 3x3 s2 pad1 (ResNet pool1 shape class -> k_pool_max_bwd3s2 padded)
    "pool_max_bwd_p1": lambda m: check_pool_bwd(m, "MAX", H=14, W=14,
                                                p=1),
    "pool_ave_bwd": lambda m: check_pool_bwd(m, "AVE"),
    "bn": check_bn,
    "bn_large_s": lambda m: check_bn(m, N=3, C=4, H=17, W=17),
    "relu": check_relu,
    "lrn": check_lrn,
    # C smaller than the window (prologue/head guards of the size-5
    # register-ring kernels) and a non-5 size (generic fallback)
    "lrn_smallc": lambda m: check_lrn(m, C=3),
    "lrn_size3": lambda m: check_lrn(m, size=3),
    "softmaxloss": check_softmaxloss,
    "softmaxloss_spatial": check_softmaxloss_spatial,
    "eltwise_concat": check_eltwise_concat,
    "dropout": check_dropout,
    "bn_global_stats": check_bn_global,
    "accuracy": check_accuracy,
}
