"""Forward and backward time of SoftmaxWithLoss over a dense score map: the
pixel-major kernels of kernels/dense_softmax.hip (a layer with a loss_param)
against the class-per-row kernels a layer without one keeps, and
k_euclid_fwd over the same number of bytes as the bandwidth yardstick
(profiles/dense_softmax.txt).

  python tools/dense_softmax_bench.py [--repeats 5] [--iters 20]

One process; the three nets alternate repeat by repeat.  Times are device
events per perf class, median [min..max] over the repeats.  Bytes are the
algorithm's: (2C + 1) * 4 per pixel in either direction (x or prob read,
prob or dx written, the label read).
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

SHAPES = [(1, 21, 500, 500), (8, 21, 512, 512)]


def net(shapes, layer):
    dims = "".join("shape { " + " ".join(f"dim: {d}" for d in s) + " } "
                   for s in shapes)
    tops = " ".join(f'top: "in{i}"' for i in range(len(shapes)))
    f = tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False)
    f.write(f'name: "b"\nforce_backward: true\nlayer {{ name: "input" type: '
            f'"Input" {tops} input_param {{ {dims} }} }}\n{layer}\n')
    f.close()
    return ca.Net.from_file(f.name)


def timed(fn, iters):
    ca.device_synchronize()
    ca.perf_reset()
    ca.set_perf_timing(True)
    for _ in range(iters):
        fn()
    ca.device_synchronize()
    ca.set_perf_timing(False)
    return sum(v["ns"] for v in ca.perf_snapshot().values()) / iters / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    ca.set_mode("gpu", 0)
    for N, C, H, W in SHAPES:
        rng = np.random.default_rng(0)
        x = rng.standard_normal((N, C, H, W)).astype(np.float32)
        lab = rng.integers(0, C, (N, H, W)).astype(np.float32)
        sm = ('layer {{ name: "loss" type: "SoftmaxWithLoss" bottom: "in0" '
              'bottom: "in1" top: "out" {} }}')
        nets = {"dense": net([x.shape, lab.shape], sm.format(
                    "loss_param { normalization: FULL }")),
                "rows": net([x.shape, lab.shape], sm.format(""))}
        for n in nets.values():
            n.set_blob("in0", x)
            n.set_blob("in1", lab)
        nbytes = 4.0 * (2 * C + 1) * N * H * W
        half = int(nbytes // 8)  # two inputs of `half` floats: nbytes read
        nets["euclid"] = net([(1, half), (1, half)],
                             'layer { name: "loss" type: "EuclideanLoss" '
                             'bottom: "in0" bottom: "in1" top: "out" }')
        runs = {(k, d): [] for k in nets for d in ("fwd", "bwd")}
        for n in nets.values():  # warm up both directions
            n.forward()
            n.backward()
        for _ in range(args.repeats):
            for k, n in nets.items():
                runs[k, "fwd"].append(timed(n.forward, args.iters))
                if k != "euclid":
                    runs[k, "bwd"].append(timed(n.backward, args.iters))
        a, b = nets["dense"], nets["rows"]
        dl = abs(a.loss() - b.loss())
        dd = np.abs(a.blob("in0", diff=True) - b.blob("in0", diff=True)).max()
        print(f"== {N}x{C}x{H}x{W}: {nbytes / 1e6:.1f} MB per direction; "
              f"routes differ by loss {dl:.1e}, dx {dd:.1e}")
        for (k, d), v in runs.items():
            if v:
                med = statistics.median(v)
                print(f"{k:>7} {d}: us {med:9.1f} [{min(v):.1f}..{max(v):.1f}]"
                      f"  {nbytes / med / 1e6:6.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
