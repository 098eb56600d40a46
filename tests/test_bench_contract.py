"""The bench line's contract (driver + tier framing): checked on the line of the round that is committed under
profiles/ (written by `python bench.py --full --steps 20 --warmup 5` on an MI355X) -- no GPU needed here."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_bench_line_has_the_contract_fields():
    import bench
    path = os.path.join(ROOT, "profiles", "%s_bench_default_run.json" % bench.ROUND)
    d = json.load(open(path))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "images/sec" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None                      # BASELINE.md publishes no number for this metric
    assert d["n_gpus"] == 1 and d["dtype"] == "bf16" and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 256 * 1e3 / d["ms_per_step"]) < 0.01 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "mfma" and r["peak"] == 2500.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic"] is None or r["traffic_source"].startswith("profiles/%s_" % bench.ROUND)   # current round only
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["cores"] >= 1
    s = d["roofline_step"]                               # img/s x F_train / peak
    assert abs(s["achieved"] - d["value"] * 47.535 / 1e3) < 0.5 and abs(s["frac"] - s["achieved"] / 2500.0) < 1e-3
    # round 5: box calibration measured in the same run, the normalised headline, both dominant labels on the line
    c = d["calibration"]
    for k in ("mfma_tflops", "mfma_lds_tflops", "copy_tbs", "gemm_tflops", "dominant_tflops", "ref_dominant_tflops",
              "dominant_exponent", "mfma_share_of_kernel_time", "method"):
        assert k in c, k
    assert 300.0 < c["mfma_lds_tflops"] < 2500.0 and 1.0 < c["copy_tbs"] < 8.0 and 0.5 < c["mfma_share_of_kernel_time"] < 0.9
    assert c["dominant_tflops"] == d["roofline"]["achieved"]
    assert abs(d["value_normalised"] - bench.normalise(d["value"], c, d["kernels"])[0]) < 1e-3 * d["value"]
    assert {"N+bn", "T+bnb"} <= set(d["roofline_labels"])
    for v in d["roofline_labels"].values():
        assert abs(v["frac"] - v["achieved"] / 2500.0) < 1e-3
    assert d["config"]["cpu_share"] >= 1


def test_normalised_headline_on_held_out_boxes():
    """`value_normalised` is an AUXILIARY diagnostic (the headline is `value`): it rescales the MFMA families' share of the
    kernel time by (REF / the run's own dominant-launch rate) ^ DOM_EXP.  ADVICE r5: the exponent had been fitted on the same
    19 round-5 lines (profiles/r05_bench_box_a..s.json, one build, the boxes that round saw) the test then checked.  Held-out
    form: the least-squares exponent of lines a..l must be the shipped DOM_EXP to +-0.25, and applied to lines m..s -- which
    the fit never saw -- it must cut their spread below 60 % of the raw one."""
    import glob
    import math
    import bench
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r05_bench_box_*.json")))
    assert len(files) >= 16, files
    ds = [json.load(open(f)) for f in files]
    fit, held = ds[:12], ds[12:]
    spread = lambda v: (max(v) - min(v)) / (sum(v) / len(v))      # noqa: E731

    def nrm(d, e):
        share = bench.normalise(d["value"], d["calibration"], d["kernels"], d["roofline"]["achieved"])[1]
        return d["value"] * (share * (bench.REF_DOMINANT_TFLOPS / d["roofline"]["achieved"]) ** e + (1.0 - share))
    best = min((spread([nrm(d, e / 100.0) for d in fit]), e / 100.0) for e in range(0, 151, 5))[1]
    assert abs(best - bench.DOM_EXP) <= 0.25, best
    raw = [d["value"] for d in held]
    got = [nrm(d, bench.DOM_EXP) for d in held]
    assert all(math.isfinite(v) for v in got)
    assert spread(got) < 0.6 * spread(raw), (spread(raw), spread(got))


def test_pmc_summary_of_the_round_is_keyed_by_bench_labels():
    import bench
    pm = json.load(open(os.path.join(ROOT, "profiles", "%s_pmc_traffic.json" % bench.ROUND)))
    labels = [k for k, v in pm.items() if isinstance(v, dict)]
    assert any(k.startswith("conv T+bnb c256+0->256 14x14") for k in labels)
    assert any(k.startswith("wgrad u256 v256 14x14") and k.endswith("x4") for k in labels)
    for k in labels:
        v = pm[k]
        assert v["hbm_bytes"] > 0 and v["algorithmic_bytes"] > 0
        b, src = bench.pmc_traffic(k)
        assert b == v["hbm_bytes"] and src.endswith("%s_pmc_traffic.json" % bench.ROUND)
    assert bench.pmc_traffic("conv N c3+0->64 1x1 no such launch") == (None, None)


def test_bench_gpus_n_starts_its_own_ranks_and_reports_their_failure():
    """`python bench.py --gpus 2` with no launcher around it (the reference's launch line is
    README.md:33-38) starts two rank processes itself.  Without a GPU both ranks fail at torch.cuda.set_device: the
    launcher must come back promptly with a non-zero exit code and an EMPTY stdout (stdout carries the JSON line
    only) -- the control flow the GPU test test_bench_launches_its_own_ranks runs to the end."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("CPU-side check of the launcher's failure path")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0
    assert r.stdout.strip() == ""
    # with WORLD_SIZE set by an external launcher the script must NOT spawn again: a mismatch is an error message
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True,
                       timeout=120, env=dict(env, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0"), cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE=4" in r.stderr


def test_rank_environment_of_the_self_launcher():
    """bench.launch_ranks' environment for N = 8 on a 16-CPU share: a loopback rendezvous on a free
    port, WORLD_SIZE / LOCAL_WORLD_SIZE, dmabuf IPC, and OpenMP threads from the USABLE CPUs (two per rank), never from
    os.cpu_count() (256 on the GPU boxes); what the caller already set is kept."""
    import bench
    env = bench.rank_env(8, {"PATH": "/bin"}, cpus=16)
    assert env["MASTER_ADDR"] == "127.0.0.1" and 1024 < int(env["MASTER_PORT"]) < 65536
    assert env["WORLD_SIZE"] == env["LOCAL_WORLD_SIZE"] == "8"
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and env["OMP_NUM_THREADS"] == "2"
    assert bench.rank_env(8, {}, cpus=256)["OMP_NUM_THREADS"] == "4" and bench.rank_env(8, {}, cpus=4)["OMP_NUM_THREADS"] == "1"
    kept = bench.rank_env(2, {"MASTER_PORT": "29501", "OMP_NUM_THREADS": "7", "MASTER_ADDR": "10.0.0.1"}, cpus=16)
    assert (kept["MASTER_PORT"], kept["OMP_NUM_THREADS"], kept["MASTER_ADDR"]) == ("29501", "7", "10.0.0.1")
    assert 1 <= bench.usable_cpus() <= (os.cpu_count() or 1)


def test_plain_run_measures_the_headline_only(monkeypatch):
    """`bench.py --gpus 1 --steps N --warmup W` without --full: no kernel-event pass, no extra modes, no CPU baseline (the
    calibration probes run as unreported warm-up unless --no-calibration); --full turns them on again and the --no-*
    switches still drop single parts."""
    import sys
    import bench
    extras = ("no_kernel_events", "no_extra_modes", "no_cpu_baseline")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.steps == 5 and a.warmup == 2 and a.dump_outputs is None
    assert all(getattr(a, k) for k in extras) and not a.no_calibration
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.no_cpu_baseline and a.dump_outputs == "out"
    assert not (a.no_calibration or a.no_kernel_events or a.no_extra_modes)


def test_dump_outputs_float32_and_seeded_sample(tmp_path):
    """--dump-outputs on host tensors standing in for the device ones: every array float32, small ones whole, one over
    DUMP_MAX_ELEMENTS as `<name>_sample` at the same seeded indices in every call, within the 64 MB budget."""
    import types
    import numpy as np
    import torch
    import bench
    n = bench.DUMP_MAX_ELEMENTS
    big = torch.arange(n + 12345, dtype=torch.float32)
    runner = types.SimpleNamespace(opt=types.SimpleNamespace(flat_w=torch.ones(1000)),
                                   opt_pfc=types.SimpleNamespace(flat_w=big))
    out = (torch.tensor(3.5), torch.tensor(0.25, dtype=torch.bfloat16))
    args = types.SimpleNamespace(mode="train")
    bench.dump_outputs(str(tmp_path / "a"), runner, out, args)
    bench.dump_outputs(str(tmp_path / "b"), runner, out, args)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["backbone_weights.npy", "head_weights_sample.npy", "loss.npy", "seg_loss.npy"]
    total = 0
    for f in names:
        x = np.load(tmp_path / "a" / f)
        assert x.dtype == np.float32 and np.array_equal(x, np.load(tmp_path / "b" / f)), f
        total += x.nbytes
    assert total <= 64 << 20
    s = np.load(tmp_path / "a" / "head_weights_sample.npy")
    assert s.shape == (n,) and (np.diff(s) >= 0).all() and s.max() > n     # sorted indices over the whole array
    assert float(np.load(tmp_path / "a" / "loss.npy")) == 3.5
    emb = torch.randn(6, 512)
    bench.dump_outputs(str(tmp_path / "c"), None, (emb, None), types.SimpleNamespace(mode="infer"))
    assert np.array_equal(np.load(tmp_path / "c" / "embeddings.npy"), emb.numpy())
