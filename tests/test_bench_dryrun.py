"""bench.py's own multi-rank plumbing, exercised at world 2 on CPU
(CAFFE_BENCH_CPU=1): gloo rendezvous, warmup/timed barriers,
max-over-ranks reduction and the single rank-0 JSON line.  The RCCL leg
is covered separately (world-1 GPU selftest + the driver's 8-GPU run);
this pins everything else in the script the scaling bench depends on.
"""
import json
import os
import socket
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def run_bench_world2():
    env = dict(os.environ, CAFFE_BENCH_CPU="1",
               MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    procs = []
    for rank in range(2):
        env_r = dict(env, RANK=str(rank), WORLD_SIZE="2",
                     LOCAL_RANK=str(rank))
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(REPO, "bench.py"),
             "--gpus", "2", "--steps", "1", "--warmup", "0",
             "--batch", "2", "--full"],
            env=env_r, cwd=REPO,
            stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    outs = []
    for p in procs:
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, err.decode()[-2000:]
        outs.append(out.decode())
    return outs


def test_bench_world2_cpu_dryrun():
    outs = run_bench_world2()
    # exactly one JSON line, from rank 0
    json_lines = [ln for o in outs for ln in o.splitlines()
                  if ln.startswith("{")]
    assert len(json_lines) == 1, outs
    d = json.loads(json_lines[0])
    assert d["n_gpus"] == 2
    assert d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 4
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["metric"] == "images/sec"
    assert d["roofline"]["peak"] > 0


def test_dump_outputs_holds_solver_state(tmp_path, monkeypatch):
    # dump_outputs() on a live LeNet solver with a budget far below the
    # model's 431k weights: every file must equal what the solver holds at
    # sample_positions(), a second dump must be byte-identical, and the
    # whole must fit the budget.
    import numpy as np
    import caffe_amd as ca
    sys.path.insert(0, REPO)
    import bench
    gen = os.path.join(REPO, "models", "generated", "lenet_solver.prototxt")
    if not os.path.exists(gen):
        subprocess.check_call([sys.executable,
                               os.path.join(REPO, "models", "gen_models.py")])
    ca.set_mode("cpu")
    ca.set_synthetic_shape(1, 28, 28, 10)
    ca.set_random_seed(1371)
    solver = ca.Solver(path=gen, batch_override=4)
    solver.step(2)
    net = solver.net
    budget = 64 << 10
    monkeypatch.setattr(bench, "DUMP_BUDGET", budget)
    bench.dump_outputs(solver, "lenet", str(tmp_path / "a"))
    bench.dump_outputs(solver, "lenet", str(tmp_path / "b"))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    n = net.num_params()
    assert len(files) == n + 2
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == \
            (tmp_path / "b" / f).read_bytes(), f
    got = {f: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= budget
    assert got["loss.npy"][0] == np.float32(solver.loss())
    # the largest array (ip1 weight, 400k) forces sampling; the common cap
    # is the sampled arrays' length
    cap = max(a.size for a in got.values())
    assert cap < 400000
    assert got["blob_ip2.npy"].shape == (4, 10)  # small enough: whole
    np.testing.assert_array_equal(got["blob_ip2.npy"], net.blob("ip2"))
    sampled = 0
    for i in range(n):
        lname, bi, cnt = net.param_info(i)
        a = got[f"param_{i:03d}_{lname}_{bi}.npy"]
        idx = bench.sample_positions(i, cnt, cap)
        want = net.param(i)
        if idx is not None:
            assert len(idx) == cap and np.all(np.diff(idx) > 0)
            assert idx[0] >= 0 and idx[-1] < cnt
            want = want[idx]
            sampled += 1
        np.testing.assert_array_equal(a, want)
    assert sampled >= 1


def test_bench_plain_run_dumps_outputs(tmp_path):
    # a plain run (no --full) times its steps, dumps what the last timed
    # step left, and reports no roofline / CPU-baseline legs.  AlexNet's
    # 61M weights exceed the dump budget, so the sampled path runs too.
    import numpy as np
    out = tmp_path / "dump"
    env = dict(os.environ, CAFFE_BENCH_CPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--model", "alexnet", "--steps", "2", "--warmup", "0",
         "--batch", "2", "--dump-outputs", str(out)],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    json_lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(json_lines) == 1, r.stdout
    d = json.loads(json_lines[0])
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] / 1000 - 2) < 1e-6  # batch 2
    assert d["roofline"] is None and d["cpu_baseline"] is None
    files = sorted(os.listdir(out))
    assert "loss.npy" in files and "blob_fc8.npy" in files
    assert sum(f.startswith("param_") for f in files) == 16
    total = 0
    for f in files:
        a = np.load(out / f)
        assert a.dtype == np.float32 and np.all(np.isfinite(a)), f
        total += a.nbytes
    assert 0 < total <= 64 << 20
    assert np.load(out / "blob_fc8.npy").shape == (2, 1000)
