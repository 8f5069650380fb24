"""Per-layer time of depthwise Convolution layers: the direct dwconv kernels
against the per-group GEMM loop (profiles/depthwise_conv.txt).

  python tools/depthwise_bench.py [--repeats 3] [--iters 20] [--pkg DIR ...]
                                  [--group G]

With --group G the shapes are the grouped 3x3 layers of ResNeXt-50 32x4d
instead (C = Cout at G groups: the gconv kernels against the loop,
profiles/grouped_conv.txt), "loop" also sets CAFFE_GROUPED=0, and each
direct kernel class is reported with its GFLOP/s and GB/s on algorithmic
flops and bytes.

Every (shape, variant) pair runs in a process of its own, the variants
alternating shape by shape and repeat by repeat: "direct" (the default
route), "loop" (CAFFE_DEPTHWISE=0) and one "pkg:<DIR>" per --pkg, an engine
build to compare with (DIR holds caffe_amd/ and libcaffe_amd.so).  A child
prints one JSON line: device-event time per kernel class for forward,
wgrad (+ db) and dgrad, the host time of a synchronised forward + backward,
and the GEMM records of one pass counted by (fam, M, N, K).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 64
# MobileNet-v1 depthwise layers: (C, H = W, stride), 3x3 pad 1
SHAPES = [(32, 112, 1), (128, 56, 1), (128, 56, 2), (512, 14, 1),
          (512, 14, 2), (1024, 7, 1)]
# ResNeXt-50 32x4d grouped layers, likewise
GROUPED_SHAPES = [(128, 56, 1), (256, 56, 2), (256, 28, 1), (512, 28, 2),
                  (512, 14, 1), (1024, 14, 2), (1024, 7, 1)]


def net_text(C, H, s, force_backward, group):
    return f"""name: "dw"
force_backward: {"true" if force_backward else "false"}
layer {{ name: "input" type: "Input" top: "in0"
  input_param {{ shape {{ dim: {BATCH} dim: {C} dim: {H} dim: {H} }} }} }}
layer {{ name: "conv" type: "Convolution" bottom: "in0" top: "out"
  convolution_param {{ num_output: {C} group: {group or C} kernel_size: 3 stride: {s}
    pad: 1 weight_filler {{ type: "xavier" }} }} }}
"""


def child(C, H, s, iters, pkg, group):
    sys.path.insert(0, pkg)
    import numpy as np
    import caffe_amd as ca
    ca.set_mode("gpu", 0)
    rng = np.random.default_rng(0)

    def build(force_backward):
        f = tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False)
        f.write(net_text(C, H, s, force_backward, group))
        f.close()
        net = ca.Net.from_file(f.name)
        net.set_blob("in0", rng.standard_normal(
            (BATCH, C, H, H)).astype(np.float32))
        net.forward()
        net.set_blob("out", rng.standard_normal(
            np.asarray(net.blob("out")).size).astype(np.float32), diff=True)
        net.backward()
        return net

    def window(fn):
        """device-event ns per call of fn, summed over kernel classes"""
        ca.device_synchronize()
        ca.perf_reset()
        ca.set_perf_timing(True)
        for _ in range(iters):
            fn()
        ca.device_synchronize()
        ca.set_perf_timing(False)
        perf = ca.perf_snapshot()
        rates.update({k: (v["flops"] / v["ns"], v["bytes"] / v["ns"])
                      for k, v in perf.items() if v["ns"]})
        return {k: v["ns"] / iters / 1e3 for k, v in perf.items() if v["ns"]}

    rates = {}  # kernel class -> (GFLOP/s, GB/s)
    full, wonly = build(True), build(False)
    for _ in range(3):  # warm-up of every launch the windows time
        full.forward(), full.backward(), wonly.backward()
    out = {"fwd_us": window(full.forward), "bwd_us": window(full.backward),
           "wgrad_us": window(wonly.backward)}
    ca.device_synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        full.forward()
        full.backward()
    ca.device_synchronize()
    out["host_us"] = (time.perf_counter() - t0) / iters * 1e6
    ca.gemm_trace(True)
    full.forward()
    full.backward()
    ca.gemm_trace(False)
    counts = {}
    for r in ca.gemm_trace_read():
        key = f'{r["fam"]} ta={r["ta"]} tb={r["tb"]} {r["M"]}x{r["N"]}x{r["K"]}'
        counts[key] = counts.get(key, 0) + 1
    out["gemms"] = counts
    out["rates"] = rates
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pkg", action="append", default=[])
    ap.add_argument("--group", type=int, default=0)
    ap.add_argument("--child", nargs=4)
    args = ap.parse_args()
    if args.child:
        C, H, s = map(int, args.child[:3])
        return child(C, H, s, args.iters, args.child[3], args.group)

    here = os.path.join(REPO, "caffe-mpi.github.io_amd")
    variants = [("direct", here, "1"), ("loop", here, "0")]
    variants += [("pkg:" + p, os.path.abspath(p), "1") for p in args.pkg]
    for C, H, s in GROUPED_SHAPES if args.group else SHAPES:
        runs = {name: [] for name, _, _ in variants}
        for _ in range(args.repeats):
            for name, pkg, flag in variants:
                res = subprocess.run(
                    [sys.executable, __file__, "--iters", str(args.iters),
                     "--group", str(args.group),
                     "--child", str(C), str(H), str(s), pkg],
                    env=dict(os.environ, CAFFE_DEPTHWISE=flag,
                             CAFFE_GROUPED=flag), timeout=120,
                    capture_output=True, text=True, check=True)
                runs[name].append(json.loads(res.stdout.splitlines()[-1]))
        print(f"== {C}@{H}x{H} 3x3 s{s} batch {BATCH}"
              + (f" group {args.group}" if args.group else ""))
        for name, _, _ in variants[2:]:  # the loop is the other build's route
            assert runs["loop"][0]["gemms"] == runs[name][0]["gemms"], name
        for name, rs in runs.items():
            def stat(f):
                v = [f(r) for r in rs]
                return f"{statistics.median(v):9.1f} [{min(v):.1f}..{max(v):.1f}]"
            dev = lambda r: sum(r["fwd_us"].values()) + sum(r["bwd_us"].values())
            print(f"{name:>8}: device fwd+bwd us {stat(dev)}  "
                  f"host fwd+bwd us {stat(lambda r: r['host_us'])}")
            print(f"{'':>8}  fwd {stat(lambda r: sum(r['fwd_us'].values()))}  "
                  f"wgrad {stat(lambda r: sum(r['wgrad_us'].values()))}  "
                  f"bwd {stat(lambda r: sum(r['bwd_us'].values()))}")
            print(f"{'':>8}  gemms {json.dumps(rs[0]['gemms'], sort_keys=True)}",
                  flush=True)
            if args.group and name == "direct":
                for k in sorted(rs[0]["rates"]):
                    v = [r["rates"][k] for r in rs]
                    print(f"{'':>8}  {k}: "
                          f"{statistics.median(a for a, _ in v):8.0f} GFLOP/s "
                          f"{statistics.median(b for _, b in v):7.0f} GB/s",
                          flush=True)


if __name__ == "__main__":
    main()
