"""bench.py's command line: a plain run is the timed steps and the headline line, --dump-outputs
writes what the last timed step returned, --full adds the rest.

CPU: the argument checks and the size cap of dump_outputs. GPU: one plain run of the smallest
config in a child process (the benchmark is a program), its line and its dumped arrays against the
same path computed here from the same seeds, bit for bit."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("phases_ms", "roofline", "mfma_assign", "recsys", "products", "reddit", "e2e", "cpu_baseline")


def _parse(argv, monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    args = _parse(["--gpus", "1", "--steps", "7", "--warmup", "3"], monkeypatch)
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 3, False, None)
    args = _parse(["--full", "--dump-outputs", "d"], monkeypatch)
    assert args.full and args.dump_outputs == "d"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--steps", "-2"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv, monkeypatch):
    with pytest.raises(SystemExit):
        _parse(argv, monkeypatch)


def _fake_outputs(n, k, d, c):
    g = torch.Generator().manual_seed(3)
    km = types.SimpleNamespace(labels_device_=torch.randint(0, k, (n,), generator=g, dtype=torch.int32),
                               cluster_centers_device_=torch.randn(k, c, generator=g))
    return torch.randn(k, d, generator=g), torch.randint(0, c, (k,), generator=g), km


def test_dump_outputs_whole_arrays(tmp_path):
    import bench
    feat, lab, km = _fake_outputs(1000, 20, 8, 5)
    bench.dump_outputs(str(tmp_path / "o"), feat, lab, km)
    got = {f[:-4]: np.load(tmp_path / "o" / f) for f in sorted(os.listdir(tmp_path / "o"))}
    assert sorted(got) == ["cluster_centers", "feat_syn", "labels", "labels_syn"]
    assert got["feat_syn"].dtype == np.float32 and np.array_equal(got["feat_syn"], feat.numpy())
    assert got["cluster_centers"].dtype == np.float32
    assert np.array_equal(got["cluster_centers"], km.cluster_centers_device_.numpy())
    assert got["labels"].dtype == np.float64 and np.array_equal(got["labels"], km.labels_device_.numpy())
    assert got["labels_syn"].dtype == np.float64 and np.array_equal(got["labels_syn"], lab.numpy())


def test_dump_outputs_caps_its_size_with_a_fixed_sample(tmp_path):
    import bench
    feat, lab, km = _fake_outputs(1000, 20, 8, 5)
    limit = 4 * 800  # a share of 800 bytes each: 100 of the 1000 fp64 labels, the others whole
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), feat, lab, km, limit=limit)
    total = 0
    for f in os.listdir(tmp_path / "a"):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert np.array_equal(a, b)  # the same sample every time
        assert a.nbytes <= limit // 4
        total += a.nbytes
    assert total <= limit
    lab_s = np.load(tmp_path / "a" / "labels.npy")
    assert lab_s.shape == (100,)
    full = km.labels_device_.numpy().astype(np.float64)
    rows = np.sort(np.random.default_rng(0).choice(1000, 100, replace=False))
    assert np.array_equal(lab_s, full[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "feat_syn.npy"), feat.numpy())  # 640 bytes: whole


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    import gdd
    from gdd import synth
    from gdd.pipeline import _lloyd
    out = tmp_path / "dump"
    steps, warmup = 3, 1
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "cora",
                        "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    cfg = synth.CONFIGS["cora"]
    for key in HEADLINE:
        assert key in rec, key
    assert rec["full"] is False and not any(key in rec for key in FULL_ONLY)
    assert rec["steps"] == steps and rec["warmup"] == warmup
    assert len(rec["config"]["kmeans_steps"]) == steps  # one fit per timed step
    assert rec["unit"] == "nodes/s" and rec["higher_is_better"] is True and rec["dtype"] == "fp32"
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(cfg.n / (rec["ms_per_step"] * 1e-3), rel=1e-9)

    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sorted(got) == ["cluster_centers", "feat_syn", "labels", "labels_syn"]
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())

    # the same step from the same seeds (bench.py main): the bench's inputs depend on its arguments alone
    dev = torch.device("cuda", 0)
    A = synth.chung_lu(cfg.n, cfg.avg_degree, cfg.seed)
    X = torch.from_numpy(synth.features(cfg.n, cfg.d, cfg.seed)).to(dev)
    rng = np.random.default_rng(cfg.seed + 3)
    W = torch.from_numpy((rng.standard_normal((cfg.d, cfg.n_classes)) / np.sqrt(cfg.d)).astype(np.float32)).to(dev)
    b = torch.from_numpy((rng.standard_normal(cfg.n_classes) * 0.1).astype(np.float32)).to(dev)
    gn = gdd.normalize_adj(gdd.to_csr(A, device=dev))
    target, _ = gdd.propagate(gn, X, cfg.T, cfg.alpha)
    state = np.random.get_state()
    try:
        np.random.seed(cfg.seed)  # cora's KMeans() draws from the global generator: the last fit of 4
        for _ in range(warmup + steps):
            km = _lloyd(cfg.k, None, device=dev).fit(torch.addmm(b, target, W))
    finally:
        np.random.set_state(state)
    feat_syn, _ = gdd.cluster_mean(target, km.labels_device_, cfg.k)
    labels_syn = gdd.argmax_rows(km.cluster_centers_device_)
    assert got["feat_syn"].shape == (cfg.k, cfg.d) and got["labels"].shape == (cfg.n,)
    assert np.array_equal(got["feat_syn"].view(np.uint32), feat_syn.cpu().numpy().view(np.uint32))
    assert np.array_equal(got["cluster_centers"].view(np.uint32),
                          km.cluster_centers_device_.cpu().numpy().view(np.uint32))
    assert np.array_equal(got["labels"], km.labels_device_.cpu().numpy())
    assert np.array_equal(got["labels_syn"], labels_syn.cpu().numpy())
