"""Forward and backward time of LRN with norm_region WITHIN_CHANNEL (the
kernels of kernels/lrn_within.hip) against the ACROSS_CHANNELS kernels on
the same tensor and local_size, which move the same bytes
(profiles/lrn_within.txt).

  python tools/lrn_within_bench.py [--repeats 5] [--iters 50]

One process; the nets of a shape alternate repeat by repeat.  Besides the
layer as it routes itself, each shape is timed in tiles where it would go
as whole planes (CAFFE_LRN_WITHIN_TILES) and with the generic window body
in place of the k = 3 one (CAFFE_LRN_WITHIN_GENERIC);
the layer reads both at every Reshape, so they are set around each net's
calls.  Times are device events of the `lrn`
perf class, median [min..max] over the repeats.  Bytes are the algorithm's:
12 per element forward (x read, y and s written), 16 backward (x, dy and s
read, dx written; the across-channel backward reads y as well: 20).
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

# CIFAR-10 full norm1 and norm2 at the solver's batch; an ImageNet-class
# map; planes too large to go whole
SHAPES = [((100, 32, 16, 16), 3), ((100, 32, 8, 8), 3),
          ((32, 96, 55, 55), 5), ((8, 64, 112, 112), 5)]
KNOBS = ("CAFFE_LRN_WITHIN_TILES", "CAFFE_LRN_WITHIN_GENERIC")


def net(shape, size, region):
    dims = " ".join(f"dim: {d}" for d in shape)
    f = tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False)
    f.write(f'name: "b"\nforce_backward: true\nlayer {{ name: "input" type: '
            f'"Input" top: "in0" input_param {{ shape {{ {dims} }} }} }}\n'
            f'layer {{ name: "norm" type: "LRN" bottom: "in0" top: "out" '
            f'lrn_param {{ local_size: {size} alpha: 1.0 beta: 0.75 '
            f'norm_region: {region} }} }}\n')
    f.close()
    return ca.Net.from_file(f.name)


def timed(fn, iters, env={}):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
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
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    ca.set_mode("gpu", 0)
    for shape, size in SHAPES:
        rng = np.random.default_rng(0)
        x = (2 * rng.standard_normal(shape)).astype(np.float32)
        dy = rng.standard_normal(shape).astype(np.float32)
        W = "WITHIN_CHANNEL"
        envs = {"within": {},
                "within tiled": {KNOBS[0]: "1"},
                "within generic": {KNOBS[1]: "1"},
                "across": {}}
        nets = {k: net(shape, size, "ACROSS_CHANNELS" if k == "across" else W)
                for k in envs}
        plans = {}
        for k, n in nets.items():  # warm up both directions; keep the plan
            n.set_blob("in0", x)
            ca.kernel_trace(True)
            timed(n.forward, 1, envs[k])
            ca.kernel_trace(False)
            plans[k] = " ".join(f"{a}={b}" for a, b in
                                ca.kernel_trace_read()[0].items())
            n.set_blob("out", dy, diff=True)
            n.backward()
        runs = {(k, d): [] for k in nets for d in ("fwd", "bwd")}
        for _ in range(args.repeats):
            for k, n in nets.items():
                runs[k, "fwd"].append(timed(n.forward, args.iters, envs[k]))
                runs[k, "bwd"].append(timed(n.backward, args.iters, envs[k]))
        count = float(np.prod(shape))
        print(f"== {'x'.join(map(str, shape))} local_size {size}: "
              f"{12 * count / 1e6:.1f} MB forward, {16 * count / 1e6:.1f} MB "
              f"backward")
        ref = nets["within"]
        for k, n in nets.items():
            note = ""
            if k != "across":  # against the layer as it routes itself
                ey = np.abs(n.blob("out") - ref.blob("out")).max()
                ed = np.abs(n.blob("in0", diff=True) -
                            ref.blob("in0", diff=True)).max()
                note = f"  (y differs by {ey:.1e}, dx by {ed:.1e})"
            print(f"  {k}: {plans[k]}{note}")
            for d, per in (("fwd", 12), ("bwd", 20 if k == "across" else 16)):
                v = runs[k, d]
                med = statistics.median(v)
                print(f"    {d}: us {med:8.1f} [{min(v):.1f}..{max(v):.1f}]  "
                      f"{per * count / med / 1e6:5.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
