"""Per-route parity for the conv / InnerProduct GEMM kernel family.

Every conv and IP contraction goes through gpu::gemm() (gemm_f32.hip),
which picks one kernel from M, N, K, the operand views and the compute
mode.  The case table below holds, for each shape, the routes the DEFAULT
dispatch takes for forward, wgrad and dgrad — written down from the
dispatch code (gemm() and the conv policy in layers_gpu.cpp), so the table
doubles as the kernel-to-shape map.  Each case is checked against the
float64 oracle at TOL = 1e-4 (check_conv / check_ip) in CPU mode and on the
GPU; the GPU run records the dispatch with ca.gemm_trace() and requires the
traced routes to be exactly the listed ones, so a retune that moves a shape
onto another kernel fails here instead of silently dropping coverage.

Route notation (one string per gemm call; a key left out has the default
in _DEFAULTS):
  fam   slim32 | slim64 | f32_128 | bf16_128 | bf16_wide
  ta tb operand transposes          sk  split-K slices (1 = none)
  kw    intra-block K split of the 128-tile kernels (M or N <= 64)
  tm tn tile rows / columns         av bv  none | chan | im2col (sh = sw)
  epi   none | plain | scatter | sscatter     bias none | row | col
"""
import numpy as np
import pytest

import caffe_amd as ca
from engine_util import input_net, net_from_text
from layer_checks import check_conv, check_conv_relu, check_ip

_DEFAULTS = dict(kw=1, av="none", bv="none", sh=1, bias="none", relu=0)


def parse_route(text):
    r = dict(_DEFAULTS)
    for kv in text.split():
        k, v = kv.split("=")
        r[k] = int(v) if v.isdigit() else v
    r["sw"] = r["sh"]
    return r


def route_key(r):
    return tuple(sorted(r.items()))


# conv cases: N, C, H, W -> Co, k / s / p / group / dilation.  Routes in the
# order forward, wgrad, dgrad.
CONV_CASES = {
    # 1x1: fwd/dgrad on the 64-row slim tile through the channel view (NN
    # and TN) with the NCHW scatter; wgrad NT, both operands channel views,
    # 128-tile with 4 K-waves and split-K.  S = 135 is odd: unaligned rows
    # take read16's scalar fallback.
    "A": (dict(N=2, C=40, H=5, W=27, Co=48, k=1, s=1, p=0), [
        "fam=slim64 ta=0 tb=0 sk=1 M=48 N=288 K=40 tm=1 tn=3 bv=chan "
        "epi=scatter bias=row",
        "fam=f32_128 ta=0 tb=1 sk=3 kw=4 M=48 N=40 K=288 tm=1 tn=1 av=chan "
        "bv=chan epi=none",
        "fam=slim64 ta=1 tb=0 sk=1 M=40 N=288 K=48 tm=1 tn=3 bv=chan "
        "epi=scatter",
    ]),
    # case A with 24 input channels: the dgrad is the 32-row slim tile with
    # a transposed A (staged by threads 0..63 only) and the NCHW scatter
    "A24": (dict(N=2, C=24, H=5, W=27, Co=48, k=1, s=1, p=0), [
        "fam=slim64 ta=0 tb=0 sk=1 M=48 N=288 K=24 tm=1 tn=3 bv=chan "
        "epi=scatter bias=row",
        "fam=f32_128 ta=0 tb=1 sk=3 kw=4 M=48 N=24 K=288 tm=1 tn=1 av=chan "
        "bv=chan epi=none",
        "fam=slim32 ta=1 tb=0 sk=1 M=24 N=288 K=48 tm=1 tn=2 bv=chan "
        "epi=scatter",
    ]),
    # 128-tile with the implicit-im2col B view + scatter, M tail 80 of 128;
    # dgrad via flipped weights and the transposed-geometry view
    "B": (dict(N=2, C=72, H=5, W=27, Co=80, k=3, s=1, p=1), [
        "fam=f32_128 ta=0 tb=0 sk=1 M=80 N=288 K=648 tm=1 tn=3 bv=im2col "
        "epi=scatter bias=row",
        "fam=f32_128 ta=0 tb=1 sk=3 M=80 N=648 K=288 tm=1 tn=6 av=chan "
        "bv=im2col epi=none",
        "fam=f32_128 ta=0 tb=0 sk=1 M=72 N=288 K=720 tm=1 tn=3 bv=im2col "
        "epi=scatter",
    ]),
    # OW < 24: explicit col, plain B at ldb = NS; dgrad TN with 6 tile rows
    "C": (dict(N=2, C=72, H=7, W=13, Co=80, k=3, s=1, p=1), [
        "fam=f32_128 ta=0 tb=0 sk=1 M=80 N=192 K=648 tm=1 tn=2 epi=scatter "
        "bias=row",
        "fam=f32_128 ta=0 tb=1 sk=2 M=80 N=648 K=192 tm=1 tn=6 av=chan "
        "epi=none",
        "fam=f32_128 ta=1 tb=0 sk=1 M=648 N=192 K=80 tm=6 tn=2 bv=chan "
        "epi=none",
    ]),
    # remainder rule (M = 160, 136): slim64 with 3 tile rows
    "D1": (dict(N=2, C=136, H=6, W=26, Co=160, k=3, s=1, p=1), [
        "fam=slim64 ta=0 tb=0 sk=1 M=160 N=320 K=1224 tm=3 tn=3 bv=im2col "
        "epi=scatter bias=row",
        "fam=slim64 ta=0 tb=1 sk=3 M=160 N=1224 K=320 tm=3 tn=10 av=chan "
        "bv=im2col epi=none",
        "fam=slim64 ta=0 tb=0 sk=1 M=136 N=320 K=1440 tm=3 tn=3 bv=im2col "
        "epi=scatter",
    ]),
    "D2": (dict(N=2, C=136, H=7, W=13, Co=160, k=3, s=1, p=1), [
        "fam=slim64 ta=0 tb=0 sk=1 M=160 N=192 K=1224 tm=3 tn=2 epi=scatter "
        "bias=row",
        "fam=slim64 ta=0 tb=1 sk=2 M=160 N=1224 K=192 tm=3 tn=10 av=chan "
        "epi=none",
        "fam=f32_128 ta=1 tb=0 sk=2 M=1224 N=192 K=160 tm=10 tn=2 bv=chan "
        "epi=none",
    ]),
    # 128-tile with 3 tile rows, M tail 72
    "E1": (dict(N=2, C=200, H=6, W=26, Co=328, k=3, s=1, p=1), [
        "fam=f32_128 ta=0 tb=0 sk=1 M=328 N=320 K=1800 tm=3 tn=3 bv=im2col "
        "epi=scatter bias=row",
        "fam=f32_128 ta=0 tb=1 sk=3 M=328 N=1800 K=320 tm=3 tn=15 av=chan "
        "bv=im2col epi=none",
        "fam=f32_128 ta=0 tb=0 sk=1 M=200 N=320 K=2952 tm=2 tn=3 bv=im2col "
        "epi=scatter",
    ]),
    # explicit; dgrad contracts over Cout = 328 > 128: TN split-K with a
    # channel-view B into dcol
    "E2": (dict(N=2, C=200, H=7, W=13, Co=328, k=3, s=1, p=1), [
        "fam=f32_128 ta=0 tb=0 sk=1 M=328 N=192 K=1800 tm=3 tn=2 epi=scatter "
        "bias=row",
        "fam=f32_128 ta=0 tb=1 sk=2 M=328 N=1800 K=192 tm=3 tn=15 av=chan "
        "epi=none",
        "fam=f32_128 ta=1 tb=0 sk=3 M=1800 N=192 K=328 tm=15 tn=2 bv=chan "
        "epi=none",
    ]),
    "E3": (dict(N=2, C=200, H=5, W=27, Co=328, k=1, s=1, p=0), [
        "fam=f32_128 ta=0 tb=0 sk=1 M=328 N=288 K=200 tm=3 tn=3 bv=chan "
        "epi=scatter bias=row",
        "fam=f32_128 ta=0 tb=1 sk=3 M=328 N=200 K=288 tm=3 tn=2 av=chan "
        "bv=chan epi=none",
        "fam=f32_128 ta=1 tb=0 sk=1 M=200 N=288 K=328 tm=2 tn=3 bv=chan "
        "epi=scatter",
    ]),
    # strided implicit view on the 128-tile; dgrad via dcol + col2im
    "F1": (dict(N=1, C=72, H=5, W=51, Co=80, k=3, s=2, p=1), [
        "fam=f32_128 ta=0 tb=0 sk=1 M=80 N=80 K=648 tm=1 tn=1 bv=im2col "
        "sh=2 epi=scatter bias=row",
        "fam=f32_128 ta=0 tb=1 sk=1 M=80 N=648 K=80 tm=1 tn=6 av=chan "
        "bv=im2col sh=2 epi=none",
        "fam=f32_128 ta=1 tb=0 sk=1 M=648 N=80 K=80 tm=6 tn=1 bv=chan "
        "epi=none",
    ]),
    # strided explicit at large M
    "F2": (dict(N=2, C=200, H=13, W=13, Co=328, k=3, s=2, p=1), [
        "fam=f32_128 ta=0 tb=0 sk=1 M=328 N=128 K=1800 tm=3 tn=1 epi=scatter "
        "bias=row",
        "fam=f32_128 ta=0 tb=1 sk=1 M=328 N=1800 K=128 tm=3 tn=15 av=chan "
        "epi=none",
        "fam=f32_128 ta=1 tb=0 sk=3 M=1800 N=128 K=328 tm=15 tn=1 bv=chan "
        "epi=none",
    ]),
    # 1x1/s2: zero-fill + strided-scatter dgrad epilogue.  With N*Spad = 64
    # columns G1 and G2 stay on the 128-tile (2 / 4 K-waves); G3's third
    # image makes 96 columns and moves the same shape onto slim64.
    "G1": (dict(N=2, C=200, H=9, W=11, Co=328, k=1, s=2, p=0), [
        "fam=f32_128 ta=0 tb=0 sk=1 kw=2 M=328 N=64 K=200 tm=3 tn=1 "
        "epi=scatter bias=row",
        "fam=f32_128 ta=0 tb=1 sk=1 M=328 N=200 K=64 tm=3 tn=2 av=chan "
        "epi=none",
        "fam=f32_128 ta=1 tb=0 sk=1 kw=2 M=200 N=64 K=328 tm=2 tn=1 bv=chan "
        "epi=sscatter",
    ]),
    "G2": (dict(N=2, C=40, H=9, W=11, Co=48, k=1, s=2, p=0), [
        "fam=f32_128 ta=0 tb=0 sk=1 kw=4 M=48 N=64 K=40 tm=1 tn=1 "
        "epi=scatter bias=row",
        "fam=f32_128 ta=0 tb=1 sk=1 kw=4 M=48 N=40 K=64 tm=1 tn=1 av=chan "
        "epi=none",
        "fam=f32_128 ta=1 tb=0 sk=1 kw=4 M=40 N=64 K=48 tm=1 tn=1 bv=chan "
        "epi=sscatter",
    ]),
    "G3": (dict(N=3, C=40, H=9, W=11, Co=48, k=1, s=2, p=0), [
        "fam=slim64 ta=0 tb=0 sk=1 M=48 N=96 K=40 tm=1 tn=1 epi=scatter "
        "bias=row",
        "fam=f32_128 ta=0 tb=1 sk=1 kw=4 M=48 N=40 K=96 tm=1 tn=1 av=chan "
        "epi=none",
        "fam=slim64 ta=1 tb=0 sk=1 M=40 N=96 K=48 tm=1 tn=1 bv=chan "
        "epi=sscatter",
    ]),
    # group 2: per-group pointer offsets into A, B, C and the views
    "H1": (dict(N=2, C=144, H=5, W=27, Co=160, k=3, s=1, p=1, grp=2), [
        "fam=f32_128 ta=0 tb=0 sk=1 M=80 N=288 K=648 tm=1 tn=3 bv=im2col "
        "epi=scatter bias=row",
        "fam=f32_128 ta=0 tb=1 sk=3 M=80 N=648 K=288 tm=1 tn=6 av=chan "
        "bv=im2col epi=none",
        "fam=f32_128 ta=0 tb=0 sk=1 M=72 N=288 K=720 tm=1 tn=3 bv=im2col "
        "epi=scatter",
    ]),
    "H2": (dict(N=2, C=400, H=5, W=27, Co=416, k=3, s=1, p=1, grp=2), [
        "fam=f32_128 ta=0 tb=0 sk=1 M=208 N=288 K=1800 tm=2 tn=3 bv=im2col "
        "epi=scatter bias=row",
        "fam=f32_128 ta=0 tb=1 sk=3 M=208 N=1800 K=288 tm=2 tn=15 av=chan "
        "bv=im2col epi=none",
        "fam=f32_128 ta=0 tb=0 sk=1 M=200 N=288 K=1872 tm=2 tn=3 bv=im2col "
        "epi=scatter",
    ]),
    # group 2 on the explicit col (OW < 24): forward and wgrad read the
    # group's K rows of the cached col buffer, dgrad writes the group's rows
    # of dcol before the one col2im.  M = Cout/group = 8.
    "H3": (dict(N=2, C=16, H=7, W=13, Co=16, k=3, s=1, p=1, grp=2), [
        "fam=slim32 ta=0 tb=0 sk=1 M=8 N=192 K=72 tm=1 tn=1 epi=scatter "
        "bias=row",
        "fam=slim32 ta=0 tb=1 sk=2 M=8 N=72 K=192 tm=1 tn=1 av=chan "
        "epi=none",
        "fam=f32_128 ta=1 tb=0 sk=1 M=72 N=192 K=8 tm=1 tn=2 bv=chan "
        "epi=none",
    ]),
    # group 2 on the strided 1x1: explicit col forward / wgrad (N = 8 keeps
    # wgrad on the 128-tile with 4 K-waves), per-group strided-scatter dgrad
    "H4": (dict(N=3, C=16, H=9, W=11, Co=16, k=1, s=2, p=0, grp=2), [
        "fam=slim32 ta=0 tb=0 sk=1 M=8 N=96 K=8 tm=1 tn=1 epi=scatter "
        "bias=row",
        "fam=f32_128 ta=0 tb=1 sk=1 kw=4 M=8 N=8 K=96 tm=1 tn=1 av=chan "
        "epi=none",
        "fam=slim32 ta=1 tb=0 sk=1 M=8 N=96 K=8 tm=1 tn=1 bv=chan "
        "epi=sscatter",
    ]),
    # group 2 on the 1x1/s1: not the single-call 1x1 (group > 1), so the
    # im2col view with kh = 1 and the flipped-weight dgrad
    "H5": (dict(N=2, C=16, H=5, W=27, Co=16, k=1, s=1, p=0, grp=2), [
        "fam=slim32 ta=0 tb=0 sk=1 M=8 N=288 K=8 tm=1 tn=2 bv=im2col "
        "epi=scatter bias=row",
        "fam=f32_128 ta=0 tb=1 sk=3 kw=4 M=8 N=8 K=288 tm=1 tn=1 av=chan "
        "bv=im2col epi=none",
        "fam=slim32 ta=0 tb=0 sk=1 M=8 N=288 K=8 tm=1 tn=2 bv=im2col "
        "epi=scatter",
    ]),
    # 1x1 with pad 1 (output 7x29): im2col view with kh = 1; the dgrad view
    # of dY has pad kh-1-ph = -1
    "P1": (dict(N=2, C=8, H=5, W=27, Co=16, k=1, s=1, p=1), [
        "fam=slim32 ta=0 tb=0 sk=1 M=16 N=416 K=8 tm=1 tn=2 bv=im2col "
        "epi=scatter bias=row",
        "fam=f32_128 ta=0 tb=1 sk=4 kw=4 M=16 N=8 K=416 tm=1 tn=1 av=chan "
        "bv=im2col epi=none",
        "fam=slim32 ta=0 tb=0 sk=1 M=8 N=288 K=16 tm=1 tn=2 bv=im2col "
        "epi=scatter",
    ]),
    # dilation 2 (always the explicit col): S32's GEMMs between a dilated
    # im2col and col2im
    "DIL": (dict(N=2, C=8, H=13, W=13, Co=16, k=3, s=1, p=2, d=2), [
        "fam=slim32 ta=0 tb=0 sk=1 M=16 N=352 K=72 tm=1 tn=2 epi=scatter "
        "bias=row",
        "fam=slim32 ta=0 tb=1 sk=3 M=16 N=72 K=352 tm=1 tn=1 av=chan "
        "epi=none",
        "fam=f32_128 ta=1 tb=0 sk=1 M=72 N=352 K=16 tm=1 tn=3 bv=chan "
        "epi=none",
    ]),
    # the class every older per-layer conv check sits in (Cout <= 16):
    # the 32-row slim tile, with and without split-K
    "S32": (dict(N=2, C=8, H=13, W=13, Co=16, k=3, s=1, p=1), [
        "fam=slim32 ta=0 tb=0 sk=1 M=16 N=352 K=72 tm=1 tn=2 epi=scatter "
        "bias=row",
        "fam=slim32 ta=0 tb=1 sk=3 M=16 N=72 K=352 tm=1 tn=1 av=chan "
        "epi=none",
        "fam=f32_128 ta=1 tb=0 sk=1 M=72 N=352 K=16 tm=1 tn=3 bv=chan "
        "epi=none",
    ]),
}

# case B with bias and an in-place ReLU: the net folds the ReLU into the
# forward GEMM's epilogue
RELU_CASE = (dict(N=2, C=72, H=5, W=27, Co=80, k=3, s=1, p=1), [
    "fam=f32_128 ta=0 tb=0 sk=1 M=80 N=288 K=648 tm=1 tn=3 bv=im2col "
    "epi=scatter bias=row relu=1",
    "fam=f32_128 ta=0 tb=1 sk=3 M=80 N=648 K=288 tm=1 tn=6 av=chan "
    "bv=im2col epi=none",
    "fam=f32_128 ta=0 tb=0 sk=1 M=72 N=288 K=720 tm=1 tn=3 bv=im2col "
    "epi=scatter",
])

# InnerProduct cases: batch M, inputs K, outputs Nout.  Forward is NT with
# the per-column bias, wgrad TN, dgrad NN; all plain operands.
IP_CASES = {
    # 2 K-waves forward over 7 K-tiles (odd: the second wave group idles in
    # the last pair)
    "ip_72_200_48": (dict(M=72, K=200, Nout=48), [
        "fam=f32_128 ta=0 tb=1 sk=1 kw=2 M=72 N=48 K=200 tm=1 tn=1 "
        "epi=plain bias=col",
        "fam=slim64 ta=1 tb=0 sk=1 M=48 N=200 K=72 tm=1 tn=2 epi=none",
        "fam=f32_128 ta=0 tb=0 sk=1 M=72 N=200 K=48 tm=1 tn=2 epi=none",
    ]),
    # remainder rule, NT plain, per-column bias
    "ip_136_300_72": (dict(M=136, K=300, Nout=72), [
        "fam=slim64 ta=0 tb=1 sk=1 M=136 N=72 K=300 tm=3 tn=1 epi=plain "
        "bias=col",
        "fam=f32_128 ta=1 tb=0 sk=2 M=72 N=300 K=136 tm=1 tn=3 epi=none",
        "fam=slim64 ta=0 tb=0 sk=1 M=136 N=300 K=72 tm=3 tn=3 epi=none",
    ]),
    "ip_200_264_40": (dict(M=200, K=264, Nout=40), [
        "fam=f32_128 ta=0 tb=1 sk=1 kw=2 M=200 N=40 K=264 tm=2 tn=1 "
        "epi=plain bias=col",
        "fam=slim64 ta=1 tb=0 sk=2 M=40 N=264 K=200 tm=1 tn=3 epi=none",
        "fam=f32_128 ta=0 tb=0 sk=1 M=200 N=264 K=40 tm=2 tn=3 epi=none",
    ]),
    "ip_264_520_136": (dict(M=264, K=520, Nout=136), [
        "fam=slim64 ta=0 tb=1 sk=1 M=264 N=136 K=520 tm=5 tn=2 epi=plain "
        "bias=col",
        "fam=slim64 ta=1 tb=0 sk=3 M=136 N=520 K=264 tm=3 tn=5 epi=none",
        "fam=slim64 ta=0 tb=0 sk=2 M=264 N=520 K=136 tm=5 tn=5 epi=none",
    ]),
    # K = 161: the last K-tile of the plain 128-tile loop holds 1 element
    "ip_72_161_80": (dict(M=72, K=161, Nout=80), [
        "fam=f32_128 ta=0 tb=1 sk=1 M=72 N=80 K=161 tm=1 tn=1 epi=plain "
        "bias=col",
        "fam=f32_128 ta=1 tb=0 sk=1 M=80 N=161 K=72 tm=1 tn=2 epi=none",
        "fam=f32_128 ta=0 tb=0 sk=1 M=72 N=161 K=80 tm=1 tn=2 epi=none",
    ]),
    # K = 24: the K-waves path sees exactly one (partial) K-tile forward,
    # three in wgrad (4 K-waves), two in dgrad
    "ip_72_24_48": (dict(M=72, K=24, Nout=48), [
        "fam=f32_128 ta=0 tb=1 sk=1 kw=2 M=72 N=48 K=24 tm=1 tn=1 epi=plain "
        "bias=col",
        "fam=f32_128 ta=1 tb=0 sk=1 kw=4 M=48 N=24 K=72 tm=1 tn=1 epi=none",
        "fam=f32_128 ta=0 tb=0 sk=1 kw=2 M=72 N=24 K=48 tm=1 tn=1 epi=none",
    ]),
    # wgrad on the 32-row slim tile with a transposed A and split-K; dgrad
    # slim64 by the remainder rule
    "ip_300_200_24": (dict(M=300, K=200, Nout=24), [
        "fam=f32_128 ta=0 tb=1 sk=1 kw=2 M=300 N=24 K=200 tm=3 tn=1 "
        "epi=plain bias=col",
        "fam=slim32 ta=1 tb=0 sk=3 M=24 N=200 K=300 tm=1 tn=1 epi=none",
        "fam=slim64 ta=0 tb=0 sk=1 M=300 N=200 K=24 tm=5 tn=2 epi=none",
    ]),
    # split-K reduce, scalar kernel: wgrad M*N = 37*53 is odd
    "ip_300_53_37": (dict(M=300, K=53, Nout=37), [
        "fam=f32_128 ta=0 tb=1 sk=1 kw=2 M=300 N=37 K=53 tm=3 tn=1 "
        "epi=plain bias=col",
        "fam=f32_128 ta=1 tb=0 sk=3 kw=4 M=37 N=53 K=300 tm=1 tn=1 epi=none",
        "fam=f32_128 ta=0 tb=0 sk=1 kw=2 M=300 N=53 K=37 tm=3 tn=1 epi=none",
    ]),
    # split-K reduce, float4 kernel with SK = 6: one pass of the 4-way
    # unrolled loop plus two of the remainder loop (M*N = 40*52)
    "ip_700_52_40": (dict(M=700, K=52, Nout=40), [
        "fam=f32_128 ta=0 tb=1 sk=1 kw=2 M=700 N=40 K=52 tm=6 tn=1 "
        "epi=plain bias=col",
        "fam=f32_128 ta=1 tb=0 sk=6 kw=4 M=40 N=52 K=700 tm=1 tn=1 epi=none",
        "fam=f32_128 ta=0 tb=0 sk=1 kw=2 M=700 N=52 K=40 tm=6 tn=1 epi=none",
    ]),
}

# bf16 compute mode re-routes M > 64: the 256x256 wide tile when M > 128 and
# N > 128, the bf16 128-tile otherwise; M <= 64 with N > 64 keeps the fp32
# slim kernels and the remainder rule is off.  (test_bf16_gpu.py checks
# these at the fp32 tolerance on bf16-rounded inputs.)
BF16_ROUTES = {
    "A": [
        "fam=slim64 ta=0 tb=0 sk=1 M=48 N=288 K=40 tm=1 tn=3 bv=chan "
        "epi=scatter bias=row",
        "fam=bf16_128 ta=0 tb=1 sk=3 kw=4 M=48 N=40 K=288 tm=1 tn=1 av=chan "
        "bv=chan epi=none",
        "fam=slim64 ta=1 tb=0 sk=1 M=40 N=288 K=48 tm=1 tn=3 bv=chan "
        "epi=scatter",
    ],
    "B": [
        "fam=bf16_128 ta=0 tb=0 sk=1 M=80 N=288 K=648 tm=1 tn=3 bv=im2col "
        "epi=scatter bias=row",
        "fam=bf16_128 ta=0 tb=1 sk=3 M=80 N=648 K=288 tm=1 tn=6 av=chan "
        "bv=im2col epi=none",
        "fam=bf16_128 ta=0 tb=0 sk=1 M=72 N=288 K=720 tm=1 tn=3 bv=im2col "
        "epi=scatter",
    ],
    "C": [
        "fam=bf16_128 ta=0 tb=0 sk=1 M=80 N=192 K=648 tm=1 tn=2 epi=scatter "
        "bias=row",
        "fam=bf16_128 ta=0 tb=1 sk=2 M=80 N=648 K=192 tm=1 tn=6 av=chan "
        "epi=none",
        "fam=bf16_wide ta=1 tb=0 sk=1 M=648 N=192 K=80 tm=3 tn=1 bv=chan "
        "epi=none",
    ],
    # Cout = 328: wide tile with 2 tile rows, M tail 72
    "E1": [
        "fam=bf16_wide ta=0 tb=0 sk=1 M=328 N=320 K=1800 tm=2 tn=2 "
        "bv=im2col epi=scatter bias=row",
        "fam=bf16_wide ta=0 tb=1 sk=3 M=328 N=1800 K=320 tm=2 tn=8 av=chan "
        "bv=im2col epi=none",
        "fam=bf16_wide ta=0 tb=0 sk=1 M=200 N=320 K=2952 tm=1 tn=2 "
        "bv=im2col epi=scatter",
    ],
    "E2": [
        "fam=bf16_wide ta=0 tb=0 sk=1 M=328 N=192 K=1800 tm=2 tn=1 "
        "epi=scatter bias=row",
        "fam=bf16_wide ta=0 tb=1 sk=2 M=328 N=1800 K=192 tm=2 tn=8 av=chan "
        "epi=none",
        "fam=bf16_wide ta=1 tb=0 sk=3 M=1800 N=192 K=328 tm=8 tn=1 bv=chan "
        "epi=none",
    ],
    "E3": [
        "fam=bf16_wide ta=0 tb=0 sk=1 M=328 N=288 K=200 tm=2 tn=2 bv=chan "
        "epi=scatter bias=row",
        "fam=bf16_wide ta=0 tb=1 sk=3 M=328 N=200 K=288 tm=2 tn=1 av=chan "
        "bv=chan epi=none",
        "fam=bf16_wide ta=1 tb=0 sk=1 M=200 N=288 K=328 tm=1 tn=2 bv=chan "
        "epi=scatter",
    ],
    "F1": [
        "fam=bf16_128 ta=0 tb=0 sk=1 M=80 N=80 K=648 tm=1 tn=1 bv=im2col "
        "sh=2 epi=scatter bias=row",
        "fam=bf16_128 ta=0 tb=1 sk=1 M=80 N=648 K=80 tm=1 tn=6 av=chan "
        "bv=im2col sh=2 epi=none",
        "fam=bf16_128 ta=1 tb=0 sk=1 M=648 N=80 K=80 tm=6 tn=1 bv=chan "
        "epi=none",
    ],
    # N = 64 columns: M = 328 stays on the bf16 128-tile (wide needs N > 128)
    "G1": [
        "fam=bf16_128 ta=0 tb=0 sk=1 kw=2 M=328 N=64 K=200 tm=3 tn=1 "
        "epi=scatter bias=row",
        "fam=bf16_wide ta=0 tb=1 sk=1 M=328 N=200 K=64 tm=2 tn=1 av=chan "
        "epi=none",
        "fam=bf16_128 ta=1 tb=0 sk=1 kw=2 M=200 N=64 K=328 tm=2 tn=1 "
        "bv=chan epi=sscatter",
    ],
    "H2": [
        "fam=bf16_wide ta=0 tb=0 sk=1 M=208 N=288 K=1800 tm=1 tn=2 "
        "bv=im2col epi=scatter bias=row",
        "fam=bf16_wide ta=0 tb=1 sk=3 M=208 N=1800 K=288 tm=1 tn=8 av=chan "
        "bv=im2col epi=none",
        "fam=bf16_wide ta=0 tb=0 sk=1 M=200 N=288 K=1872 tm=1 tn=2 "
        "bv=im2col epi=scatter",
    ],
}


def traced(fn):
    """Run fn() with the route trace on; returns the traced route dicts."""
    ca.gemm_trace(True)
    try:
        fn()
    finally:
        ca.gemm_trace(False)
    return ca.gemm_trace_read()


def assert_routes(trace, expected):
    """Every listed route is in the trace, and the trace holds no other."""
    got = {route_key(r) for r in trace}
    want = {route_key(parse_route(t)) for t in expected}
    for t in expected:
        assert route_key(parse_route(t)) in got, (
            f"route not taken: {t}\ntrace: {trace}")
    extra = got - want
    assert not extra, f"unlisted routes: {[dict(k) for k in extra]}"


def _run(mode, check, cfg, routes):
    errs = {}
    if mode == "cpu":
        check("cpu", errs=errs, **cfg)
        return
    try:
        trace = traced(lambda: check("gpu", errs=errs, **cfg))
    finally:
        print("relerr", {k: f"{v:.2e}" for k, v in errs.items()})
    assert_routes(trace, routes)


@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_route_cpu(name):
    _run("cpu", check_conv, *CONV_CASES[name])


@pytest.mark.parametrize("name", sorted(IP_CASES))
def test_ip_route_cpu(name):
    _run("cpu", check_ip, *IP_CASES[name])


def test_conv_relu_route_cpu():
    _run("cpu", check_conv_relu, *RELU_CASE)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_route_gpu(name):
    _run("gpu", check_conv, *CONV_CASES[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(IP_CASES))
def test_ip_route_gpu(name):
    _run("gpu", check_ip, *IP_CASES[name])


@pytest.mark.gpu
def test_conv_relu_route_gpu():
    _run("gpu", check_conv_relu, *RELU_CASE)


def test_route_table_is_wellformed():
    keys = {"fam", "ta", "tb", "sk", "kw", "M", "N", "K", "tm", "tn", "av",
            "bv", "sh", "sw", "epi", "bias", "relu"}
    tables = ([r for _, r in CONV_CASES.values()] + [RELU_CASE[1]]
              + [r for _, r in IP_CASES.values()]
              + list(BF16_ROUTES.values()))
    for routes in tables:
        assert len(routes) == 3  # forward, wgrad, dgrad
        for t in routes:
            assert set(parse_route(t)) == keys, t
    assert set(BF16_ROUTES) <= set(CONV_CASES)


def test_gemm_trace_off_and_empty():
    # tracing is off by default and reading an empty log is well defined
    ca.gemm_trace(True)
    ca.gemm_trace(False)
    assert ca.gemm_trace_read() == []


def _step(shape, body):
    """Forward + backward of a one-layer net on arbitrary data (the union
    test below needs the dispatch only, not the numbers)."""
    net = net_from_text(input_net([shape], body))
    net.set_blob("in0", np.ones(shape, np.float32))
    net.forward()
    net.backward()


def _conv_step(N, C, H, W, Co, k, s, p, grp=1, d=1, relu=False):
    body = f"""layer {{ name: "conv" type: "Convolution" bottom: "in0"
  top: "out" convolution_param {{ num_output: {Co} kernel_size: {k}
  stride: {s} pad: {p} group: {grp} dilation: {d} }} }}"""
    if relu:
        body += '\nlayer { name: "r" type: "ReLU" bottom: "out" top: "out" }'
    _step((N, C, H, W), body)


def _ip_step(M, K, Nout):
    _step((M, K), f"""layer {{ name: "ip" type: "InnerProduct" bottom: "in0"
  top: "out" inner_product_param {{ num_output: {Nout} }} }}""")


@pytest.mark.gpu
def test_route_union_covers_every_kernel():
    """The table as a whole reaches every kernel family with and without
    split-K, every operand-view kind (stride-1 and strided im2col), every
    epilogue and bias kind and the fused ReLU — in the default dispatch.
    Fails when a retune orphans one of them."""
    ca.set_mode("gpu")
    seen = []
    try:
        for name, (cfg, routes) in sorted(CONV_CASES.items()):
            seen += traced(lambda: _conv_step(**cfg))
        seen += traced(lambda: _conv_step(relu=True, **RELU_CASE[0]))
        for name, (cfg, routes) in sorted(IP_CASES.items()):
            seen += traced(lambda: _ip_step(**cfg))
        ca.set_compute("bf16")
        for name in sorted(BF16_ROUTES):
            seen += traced(lambda: _conv_step(**CONV_CASES[name][0]))
    finally:
        ca.set_compute("f32")
    allr = seen
    fam_split = {(r["fam"], r["sk"] > 1) for r in allr}
    want = {(f, s) for f in ("slim32", "slim64", "f32_128", "bf16_128",
                             "bf16_wide") for s in (False, True)}
    assert want <= fam_split, sorted(want - fam_split)
    assert {r["av"] for r in allr} >= {"none", "chan"}
    assert {(r["bv"], r["sh"]) for r in allr} >= {
        ("none", 1), ("chan", 1), ("im2col", 1), ("im2col", 2)}
    assert {r["epi"] for r in allr} >= {"none", "plain", "scatter",
                                        "sscatter"}
    assert {r["bias"] for r in allr} >= {"none", "row", "col"}
    assert {r["relu"] for r in allr} == {0, 1}
    assert {r["kw"] for r in allr} == {1, 2, 4}
