"""Forward and backward time of the PReLU layer (kernels/prelu.hip) against
what the engine already runs over the same tensor (profiles/prelu.txt):
ReLU with a leaky slope, which moves the same bytes and computes no
parameter gradient, and Scale, whose backward is the composed form of a
per-channel parameter sum (bn_bwd_stats + bn_bwd_finalize, then chan_affine
for dx).

  python tools/prelu_bench.py [--repeats 5] [--iters 50]

One process; the nets of a tensor alternate repeat by repeat.  Times are
device events summed per perf class (prelu | relu | bn | eltwise), median
[min..max] over the repeats, so Scale's two reduction launches (bn) are
apart from its dx pass (eltwise).  Bytes are the algorithm's: 8 per element
forward (12 in-place: the saved x), 12 backward.
"""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "caffe-mpi.github.io_amd"))
import caffe_amd as ca  # noqa: E402

# a ResNet-class early and late stage at batch 128, and an InnerProduct
# output (S = 1)
SHAPES = [(128, 64, 56, 56), (128, 256, 14, 14), (1024, 4096)]
LAYERS = {
    "prelu": ('type: "PReLU"', "out"),
    "prelu in-place": ('type: "PReLU"', "in0"),
    "relu leaky": ('type: "ReLU" relu_param { negative_slope: 0.25 }', "out"),
    "scale": ('type: "Scale"', "out"),
}


def net(shape, body, top):
    dims = " ".join(f"dim: {d}" for d in shape)
    f = tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False)
    f.write(f'name: "b"\nforce_backward: true\nlayer {{ name: "input" type: '
            f'"Input" top: "in0" input_param {{ shape {{ {dims} }} }} }}\n'
            f'layer {{ name: "act" {body} bottom: "in0" top: "{top}" }}\n')
    f.close()
    return ca.Net.from_file(f.name)


def timed(fn, iters):
    """us per call by perf class."""
    ca.device_synchronize()
    ca.perf_reset()
    ca.set_perf_timing(True)
    for _ in range(iters):
        fn()
    ca.device_synchronize()
    ca.set_perf_timing(False)
    return {k: v["ns"] / iters / 1e3 for k, v in ca.perf_snapshot().items()
            if v["ns"] > 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    ca.set_mode("gpu", 0)
    for shape in SHAPES:
        rng = np.random.default_rng(0)
        x = rng.standard_normal(shape).astype(np.float32)
        dy = rng.standard_normal(shape).astype(np.float32)
        nets, plans = {}, {}
        for k, (body, top) in LAYERS.items():
            if top == "in0" and shape != SHAPES[0]:
                continue
            n = nets[k] = net(shape, body, top)
            n.set_blob("in0", x)
            ca.kernel_trace(True)
            n.forward()  # warm up both directions; keep the records
            n.set_blob(top, dy, diff=True)
            n.backward()
            ca.kernel_trace(False)
            plans[k] = ["  ".join(f"{a}={b}" for a, b in r.items())
                        for r in ca.kernel_trace_read()]
        runs = {}
        for _ in range(args.repeats):
            for k, n in nets.items():
                for d, fn in (("fwd", n.forward), ("bwd", n.backward)):
                    for cls, us in timed(fn, args.iters).items():
                        runs.setdefault((k, d, cls), []).append(us)
        count = float(np.prod(shape))
        print(f"== {'x'.join(map(str, shape))}: {count * 4 / 1e6:.1f} MB a "
              f"tensor")
        for k in nets:
            print(f"  {k}")
            for rec in plans[k]:
                print(f"    {rec}")
            for (kk, d, cls), v in runs.items():
                if kk != k:
                    continue
                per = 8 if d == "fwd" else 12
                if d == "fwd" and k == "prelu in-place":
                    per = 12
                med = statistics.median(v)
                rate = (f"  {per * count / med / 1e6:5.2f} TB/s at {per} "
                        f"B/element" if cls in ("prelu", "relu") else "")
                print(f"    {d} {cls:8s} us {med:8.1f} [{min(v):.1f}.."
                      f"{max(v):.1f}]{rate}", flush=True)


if __name__ == "__main__":
    main()
