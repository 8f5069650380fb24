"""Forward time of Deconvolution layers: the phase-split kernels of
kernels/deconv.hip against the GEMM + col2im form (profiles/deconv.txt).

  python tools/deconv_bench.py [--repeats 3] [--iters 20] [--backward]

With --backward an iteration is one forward and one backward, the routes are
"split" and "bwd_gemm" (CAFFE_DECONV_BWD=0: forward stays phase-split,
backward takes im2col + GEMMs), every perf class is reported as median
[min..max] over the repeats, and the parent compares the routes' dx and dW.

Every (shape, route) pair runs in a process of its own, the routes
alternating shape by shape and repeat by repeat: "split" (the default
route) and "gemm" (CAFFE_DECONV=0).  A child warms up, then prints one JSON
line: device-event time per kernel class of one forward (deconv_fwd includes
the weight packing), and the largest difference between the two routes'
outputs is checked by the parent.  Rates are algorithmic flops and bytes
(every input pixel meets every tap; x, W and y moved once) over that time.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (N, C_in, num_output, group, H = W, kernel, stride, pad)
SHAPES = [(32, 256, 128, 1, 32, 4, 2, 1), (32, 128, 64, 1, 64, 2, 2, 0),
          (32, 64, 3, 1, 64, 4, 2, 1), (8, 21, 21, 21, 64, 16, 8, 4)]


def net_text(N, Ci, Co, G, H, k, s, p, backward=False):
    return f"""name: "up"
force_backward: {"true" if backward else "false"}
layer {{ name: "input" type: "Input" top: "in0"
  input_param {{ shape {{ dim: {N} dim: {Ci} dim: {H} dim: {H} }} }} }}
layer {{ name: "up" type: "Deconvolution" bottom: "in0" top: "out"
  convolution_param {{ num_output: {Co} group: {G} kernel_size: {k}
    stride: {s} pad: {p} weight_filler {{ type: "xavier" }}
    bias_filler {{ type: "constant" value: 0.1 }} }} }}
"""


def child(shape, iters, backward=False):
    sys.path.insert(0, os.path.join(REPO, "caffe-mpi.github.io_amd"))
    import numpy as np
    import caffe_amd as ca
    ca.set_mode("gpu", 0)
    ca.set_random_seed(7)
    f = tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False)
    f.write(net_text(*shape, backward=backward))
    f.close()
    net = ca.Net.from_file(f.name)
    N, Ci, _, _, H = shape[:5]
    net.set_blob("in0", np.random.default_rng(0).standard_normal(
        (N, Ci, H, H)).astype(np.float32))
    def step():
        net.forward()
        if backward:
            net.backward()

    if backward:
        net.forward()
        net.set_blob("out", np.random.default_rng(1).standard_normal(
            np.asarray(net.blob("out")).shape).astype(np.float32), diff=True)
    for _ in range(3):
        step()
    ca.device_synchronize()
    ca.perf_reset()
    ca.set_perf_timing(True)
    for _ in range(iters):
        step()
    ca.device_synchronize()
    ca.set_perf_timing(False)
    us = {k: v["ns"] / iters / 1e3 for k, v in ca.perf_snapshot().items()
          if v["ns"]}
    y = np.asarray(net.blob("out"), np.float64)
    res = {"us": us, "sum": float(np.abs(y).sum()),
           "probe": y.ravel()[::9973].tolist()}
    if backward:
        for key, a in (("dx", net.blob("in0", diff=True)),
                       ("dw", net.param(0, diff=True))):
            res[key] = np.asarray(a, np.float64).ravel()[::997].tolist()
    print(json.dumps(res))


def probe_diff(a, b):
    return max(abs(u - v) for u, v in zip(a, b)) / max(map(abs, b))


def main_backward(args):
    for i, (N, Ci, Co, G, H, k, s, p) in enumerate(SHAPES):
        runs = {"split": [], "bwd_gemm": []}
        for _ in range(args.repeats):
            for name, flag in (("split", "1"), ("bwd_gemm", "0")):
                res = subprocess.run(
                    [sys.executable, __file__, "--iters", str(args.iters),
                     "--backward", "--child", str(i)],
                    env=dict(os.environ, CAFFE_DECONV_BWD=flag), timeout=300,
                    capture_output=True, text=True, check=True)
                runs[name].append(json.loads(res.stdout.splitlines()[-1]))
        a, b = runs["split"][0], runs["bwd_gemm"][0]
        col = 4 * (Co // G) * k * k * G * N * ((H * H + 15) // 16 * 16)
        print(f"== N={N} {Ci}->{Co} group {G} at {H}x{H} k{k} s{s} p{p}: "
              f"col of the top gradient {col / 1e6:.0f} MB; routes differ by "
              f"dx {probe_diff(a['dx'], b['dx']):.1e}, "
              f"dW {probe_diff(a['dw'], b['dw']):.1e} of the largest")
        for name, rs in runs.items():
            bwd = [sum(v for c, v in r["us"].items() if c != "deconv_fwd")
                   for r in rs]
            print(f"{name:>9}: backward us {statistics.median(bwd):9.1f} "
                  f"[{min(bwd):.1f}..{max(bwd):.1f}]")
            for c in sorted(rs[0]["us"]):
                v = [r["us"].get(c, 0.0) for r in rs]
                print(f"{'':>11}{c:<20}{statistics.median(v):9.1f} "
                      f"[{min(v):.1f}..{max(v):.1f}]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--child", type=int)
    ap.add_argument("--backward", action="store_true")
    args = ap.parse_args()
    if args.child is not None:
        return child(SHAPES[args.child], args.iters, args.backward)
    if args.backward:
        return main_backward(args)
    for i, (N, Ci, Co, G, H, k, s, p) in enumerate(SHAPES):
        runs = {"split": [], "gemm": []}
        for _ in range(args.repeats):
            for name, flag in (("split", "1"), ("gemm", "0")):
                res = subprocess.run(
                    [sys.executable, __file__, "--iters", str(args.iters),
                     "--child", str(i)], env=dict(os.environ, CAFFE_DECONV=flag),
                    timeout=300, capture_output=True, text=True, check=True)
                runs[name].append(json.loads(res.stdout.splitlines()[-1]))
        OH = s * (H - 1) + k - 2 * p
        flops = 2.0 * N * Ci * H * H * (Co // G) * k * k
        nbytes = 4.0 * (N * Ci * H * H + N * Co * OH * OH + Ci * (Co // G) * k * k)
        a, b = runs["split"][0]["probe"], runs["gemm"][0]["probe"]
        diff = max(abs(u - v) for u, v in zip(a, b)) / max(map(abs, b))
        print(f"== N={N} {Ci}->{Co} group {G} at {H}x{H} k{k} s{s} p{p}: "
              f"{flops / 1e9:.2f} GFLOP, {nbytes / 1e6:.1f} MB, "
              f"routes differ by {diff:.1e} of the largest output")
        for name, rs in runs.items():
            tot = [sum(r["us"].values()) for r in rs]
            med = statistics.median(tot)
            print(f"{name:>6}: fwd us {med:9.1f} [{min(tot):.1f}..{max(tot):.1f}]"
                  f"  {flops / med / 1e6:7.2f} TFLOP/s {nbytes / med / 1e3:7.1f} GB/s"
                  f"  {json.dumps({k: round(v, 1) for k, v in rs[0]['us'].items()})}",
                  flush=True)


if __name__ == "__main__":
    main()
