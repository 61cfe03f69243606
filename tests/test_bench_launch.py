"""CPU: bench.py's multi-rank path as the driver runs it — `bench.py --gpus 2` spawns its own two ranks (no
WORLD_SIZE), they meet over gloo, every rank's analysis is gathered to rank 0, time is the max over ranks and
iterations the sum — with the --selftest stand-in analysis (known outputs) in place of the GPU engine; and (GPU)
the same launch over the real engine."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _run(*extra, env=None):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + list(extra)
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=e)
    return p


def test_bench_spawns_its_ranks():
    p = _run("--gpus", "2", "--selftest", "--full", "--steps", "2", "--warmup", "1")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout  # one JSON line, from rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1
    # stand-in analysis of rank r: 97 + r iterations, 110 + r evaluations; 2 steps each
    assert out["iters"] == 2 * (97 + 98) and out["evals"] == 2 * (110 + 111)
    assert out["gathered"] == [[69, 128, 256], [69, 128, 256]]
    assert out["value"] == out["iters"] / (out["ms_per_step"] * 1e-3 * out["steps"])
    assert out["config"]["T"] == 2  # the default workload is config 3, the metric's 4D-Var config (r05)
    for cid in (2, 4, 5):  # every BASELINE config other than the main one is a sub-record of a --full line
        c = out[f"config{cid}"]
        assert c["n_gpus"] == 2 and c["gathered"] == [[69, 128, 256], [69, 128, 256]] and c["iters"] == 97 + 98
    for k in ("metric", "unit", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in out


def test_bench_spawns_eight_ranks():
    """Config 4's layout (8 analyses, one per GPU of a node) on CPU: `bench.py --gpus 8` spawns 8 ranks over gloo;
    rank 0 receives 8 (69, 128, 256) analyses per step, the iterations are summed over the ranks, the time is the
    slowest rank's (the stand-in analysis of rank r sleeps 10 (1 + r) ms, so rank 7 sets it), and the host-CPU record
    covers all ranks."""
    p = _run("--gpus", "8", "--selftest", "--full", "--steps", "2", "--warmup", "1", env={"OMP_NUM_THREADS": "1"})
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8
    assert out["iters"] == 2 * sum(97 + r for r in range(8)) and out["evals"] == 2 * sum(110 + r for r in range(8))
    assert out["gathered"] == [[69, 128, 256]] * 8
    assert out["ms_per_step"] >= 80.0  # max over ranks: rank 7's 80 ms stand-in
    assert out["value"] == out["iters"] / (out["ms_per_step"] * 1e-3 * out["steps"])
    c4 = out["config4"]
    assert c4["n_gpus"] == 8 and c4["analyses"] == 8 and c4["gathered"] == [[69, 128, 256]] * 8
    assert c4["iters"] == sum(97 + r for r in range(8)) and c4["wall_clock_s"] >= 0.08
    hc = out["host_cpu"]
    assert hc["cpu_s_all_ranks"] >= hc["cpu_s_max_rank"] > 0


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run (no --full) times its steps and prints the headline line only: no sub-records of other configs, no
    baselines, no profile. --steps sets the number of timed steps (the iterations scale with it), and --dump-outputs
    writes what the last timed step returned: both ranks' stand-in analyses (rank r's field is r everywhere), rank 0's
    stand-in latent of that step and the step's own iteration / evaluation counts, as float32 / float64 .npy."""
    import numpy as np

    d = tmp_path / "out"
    p = _run("--gpus", "2", "--selftest", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["iters"] == 3 * (97 + 98) and out["evals"] == 3 * (110 + 111)
    assert out["ms_per_step"] >= 20.0  # rank 1's 20 ms stand-in, per step
    assert out["value"] == out["iters"] / (out["ms_per_step"] * 1e-3 * out["steps"])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out
    for k in ("config2", "config4", "config5", "sc4dvar", "cpu_baseline", "exact_f32", "roofline", "J_start"):
        assert k not in out, k
    assert sorted(f.name for f in d.iterdir()) == ["counts.npy", "xa.npy", "z.npy"]
    xa, counts, z = np.load(d / "xa.npy"), np.load(d / "counts.npy"), np.load(d / "z.npy")
    assert xa.dtype == np.float32 and xa.shape == (2, 69, 128, 256)
    assert np.all(xa[0] == 0.0) and np.all(xa[1] == 1.0)
    # rank 0's stand-in latent is 0.25 x (its analysis calls so far): the 4th call (1 warm-up + 3 steps) is the last
    # timed step; the step before it would give 0.75, a call after the timed region 1.25
    assert z.dtype == np.float32 and z.shape == (1, 32, 128, 256) and np.all(z == 1.0)
    assert counts.dtype == np.float64 and counts.tolist() == [97.0, 110.0]  # rank 0's last step


def test_dump_outputs_samples_large_outputs(tmp_path):
    """dump_outputs keeps the files under its byte budget: a larger set of arrays is cut to a fixed seeded sample (the
    same elements on every call), float64 stays float64, everything else is written as float32."""
    import numpy as np

    import bench

    big = np.arange(20_000_000, dtype=np.float32)  # 80 MB
    small = np.arange(1000, dtype=np.float64)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"big": big, "small": small, "ints": np.arange(5)})
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("big", "small", "ints")}
    b = {n: np.load(tmp_path / "b" / f"{n}.npy") for n in ("big", "small", "ints")}
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 10 ** 6
    assert a["big"].dtype == np.float32 and a["small"].dtype == np.float64 and a["ints"].dtype == np.float32
    assert 10_000_000 < a["big"].size < big.size and np.all(np.diff(a["big"]) >= 0)  # a sorted sample of big itself
    assert np.array_equal(a["small"], small) and np.array_equal(a["ints"], np.arange(5, dtype=np.float32))
    for n in a:
        assert np.array_equal(a[n], b[n])


def test_bench_world_size_must_match():
    p = _run("--gpus", "2", "--selftest", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and "WORLD_SIZE" in p.stderr


@pytest.mark.gpu
def test_bench_dump_is_the_last_analysis(tmp_path, monkeypatch, capsys):
    """The product path's dump (one plain config-3 step in this process): xa / z / counts have the analysis's and the
    latent's shapes, counts are the line's iterations and evaluations, and z is the latent xa was decoded from:
    decoding z.npy on a freshly bound problem gives xa.npy.
    Bound: the decode is deterministic code on the same input, so only fp32 summation order could differ (6e-8 per
    rounding, sums of up to ~1e3 terms): 1e-4 of the largest increment |xa - decode(0)|; a missing or foreign latent
    (zeros, another analysis's) is off by O(1) of that increment."""
    import numpy as np
    import torch

    import bench

    d = tmp_path / "out"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "1", "--warmup", "0",
                                      "--dump-outputs", str(d)])
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert "config2" not in out and "J_start" not in out  # a plain line
    xa, z, counts = np.load(d / "xa.npy"), np.load(d / "z.npy"), np.load(d / "counts.npy")
    assert xa.dtype == np.float32 and xa.shape == (69, 128, 256) and np.isfinite(xa).all()
    assert z.dtype == np.float32 and z.shape == (1, 32, 128, 256) and np.isfinite(z).all() and np.abs(z).max() > 0
    assert counts.tolist() == [out["iters"], out["evals"]]
    w = bench.GpuAnalyses(3, 0, 0)
    xa_z = w.prob.analysis(torch.from_numpy(z).to(w.dev)).cpu().numpy()
    xa_0 = w.prob.analysis(torch.zeros(z.shape, device=w.dev)).cpu().numpy()
    inc = float(np.abs(xa - xa_0).max())
    err = float(np.abs(xa_z - xa).max()) / inc
    print(f"dump: max increment {inc:.4e}, |decode(z.npy) - xa.npy| / increment {err:.2e}")
    assert inc > 0 and err < 1e-4


@pytest.mark.gpu
def test_bench_two_ranks_product_path():
    """The product path with two ranks: `bench.py --gpus 2` spawns two processes that each run a full config-3
    analysis (the default workload: T = 2) on libvaevar (here both on the box's one GPU, over gloo since RCCL refuses
    two ranks per device), gather both analyses to rank 0, take the max time and sum the iterations (G13: J falls to
    0.41 of its start over the budget)."""
    p = _run("--gpus", "2", "--full", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-profile",
             "--no-exact-f32", "--no-config2", "--no-config4", "--no-config5", "--no-sc4dvar", env={"VAEVAR_DIST_BACKEND": "gloo"})
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    print({k: out[k] for k in ("n_gpus", "iters", "evals", "value", "gathered", "J_start", "J_final")})
    assert out["n_gpus"] == 2 and out["gathered"] == [[69, 128, 256], [69, 128, 256]]
    assert 150 <= out["iters"] <= 200 and out["J_final"] < 0.5 * out["J_start"]
