"""bench.py's multi-GPU entry point.  CPU: argument / launcher consistency fails loudly before anything touches a GPU.
-m gpu: `python bench.py --gpus 2` with NO launcher starts two ranks itself; on the 1-GPU test box both ranks share cuda:0 and the
collective runs over gloo (JSORB_BENCH_SINGLE_DEVICE / JSORB_BENCH_BACKEND test hooks) - the product's N > 1 path (pair sharding,
jsorb_gather_counts_async, jsorb_stream_wait_done, all_gather, double-buffered payload) runs for real and is checked against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra)
    return env


def test_gpus_flag_must_match_the_launcher_world_size():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=_clean_env(WORLD_SIZE="4", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=4" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], env=_clean_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--gpus 1 but WORLD_SIZE=2" in r.stderr


@pytest.mark.gpu
def test_bench_launches_two_ranks_itself_and_gathers_counts():
    args = ["--gpus", "2", "--steps", "3", "--warmup", "1", "--pairs", "6", "--config", "c1", "--min-time", "0.05", "--full", "--no-cpu-baseline", "--no-extras",
            "--profile-steps", "1"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=_clean_env(JSORB_BENCH_SINGLE_DEVICE="1", JSORB_BENCH_BACKEND="gloo"),
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                    # ONE JSON line, from rank 0
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["pairs_per_step_total"] == 12
    assert d["parity_vs_oracle"] is True and d["gathered_counts_ok"] is True and d["parity_pairs_checked"] == 12
    # what makes a first real multi-GPU run diagnosable: every rank's own median block time next to the max the value is made of, and the time of the all_gather itself
    diag = d["multi_gpu_diag"]
    assert len(diag["per_rank"]) == 2 and all(r_["median_block_ms"] > 0 and r_["ms_per_step"] > 0 and r_["all_gather_ms_mean"] >= 0 and r_["all_gather_ms_max"] >= r_["all_gather_ms_mean"]
                                              for r_ in diag["per_rank"])
    assert max(r_["ms_per_step"] for r_ in diag["per_rank"]) <= d["ms_per_step"] * 1.5 and d["summary"]["pairs_per_s"] == d["value"]
    # round 6: the record checks itself (device / PCI / collective checks are "skipped" under the single-device gloo hook, never "failed")
    sc = diag["self_check"]
    assert set(sc["checks"]) == {"distinct_devices", "distinct_pci", "numa_bound", "all_gather_under_100us", "no_straggler_over_5pct"} and isinstance(sc["diagnosis"], str)
    assert isinstance(sc["checks"]["distinct_devices"], str) and isinstance(sc["checks"]["all_gather_under_100us"], str)
    assert all("pci" in r_ and "device_index" in r_ and "numa_bound" in r_ for r_ in diag["per_rank"])
    # --dry-multi: the self-check alone, in seconds; the exit code is non-zero iff a check failed (e.g. the two ranks of this box drift more than 5 % apart;
    # a rank exits with 3, which the launcher reports as a failed worker)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-multi", "--steps", "3", "--warmup", "1", "--pairs", "6", "--config", "c1"],
                       env=_clean_env(JSORB_BENCH_SINGLE_DEVICE="1", JSORB_BENCH_BACKEND="gloo"), capture_output=True, text=True, timeout=600, cwd=ROOT)
    dd = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert dd["multi_gpu_diag"]["self_check"]["ok"] == (r.returncode == 0), r.stderr[-2000:]
    assert dd["cpu_baseline"] is None
    # strong scaling shape (BASELINE C4 style): the total is split over the ranks
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--pairs-total", "8"],
                       env=_clean_env(JSORB_BENCH_SINGLE_DEVICE="1", JSORB_BENCH_BACKEND="gloo"), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["pairs_per_gpu_per_step"] == 4 and d["parity_vs_oracle"] is True


@pytest.mark.gpu
def test_bench_eight_ranks_c4_shape_on_one_device():
    """BASELINE C4 exactly as the driver's 8-GPU run shapes it - `--gpus 8 --pairs-total 64` on the EuRoC configuration: eight ranks (all
    on cuda:0 here, collective over gloo) of eight pairs each, global pair sharding, one all_gather per step, every rank checking every
    row of the gathered table, launch and teardown of eight processes."""
    args = ["--gpus", "8", "--pairs-total", "64", "--config", "c2", "--steps", "3", "--warmup", "1", "--min-time", "0.05", "--full", "--no-cpu-baseline", "--no-extras",
            "--profile-steps", "1"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=_clean_env(JSORB_BENCH_SINGLE_DEVICE="1", JSORB_BENCH_BACKEND="gloo"),
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["scaling"] == "strong" and d["config"]["pairs_per_gpu_per_step"] == 8 and d["config"]["pairs_per_step_total"] == 64
    assert d["parity_vs_oracle"] is True and d["gathered_counts_ok"] is True and d["parity_pairs_checked"] == 64


@pytest.mark.gpu
def test_bench_refuses_more_gpus_than_visible():
    import torch
    n = torch.cuda.device_count()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n + 1)], env=_clean_env(), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "visible" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_plain_run_times_the_given_steps_and_dumps_the_last_step(tmp_path, po):
    """A plain run (no --full) times ONE block of exactly --steps steps, leaves every --full measurement out of its line, and --dump-outputs
    writes what the last timed step computed: float arrays, the same files in two runs with the same arguments, and on the sampled pairs the
    oracle's keypoints, descriptors, uRight and depth."""
    from jetson_slam_amd.synth import synth_stereo_pair
    h, w, L, tile, fx, bf, P = 240, 320, 3, 15, 435.2, 47.906, 6
    args = ["--gpus", "1", "--steps", "4", "--warmup", "1", "--pairs", str(P), "--config", "c1"]
    lines = []
    for name in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(tmp_path / name)], env=_clean_env(),
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        ls = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(ls) == 1
        lines.append(json.loads(ls[0]))
    d = lines[0]
    assert d["steps"] == 4 and d["timing"]["blocks"] == 1 and d["timing"]["block_steps"] == 4 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] / 1e3 / P - 1.0) < 0.01
    assert all(k in d for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"))
    for k in ("parity_vs_oracle", "roofline", "cpu_baseline", "host_streamed", "frame_latency_us", "c4_batch64", "other_configs", "other_inputs"):
        assert d[k] is None, k
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == sorted(n + ".npy" for n in (
        "counts", "sample_pairs", "left_keypoints", "left_descriptors", "right_keypoints", "right_descriptors", "u_right", "depth"))
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) < 64 << 20
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        b_ = np.load(tmp_path / "b" / n)
        assert got[n[:-4]].dtype in (np.float32, np.float64) and b_.dtype == got[n[:-4]].dtype and np.array_equal(got[n[:-4]], b_), n
    # c1, one input set: pair i of every step is the synthetic pair with seed 1 + i
    lo = ro = 0
    for i in range(P):
        left, right = synth_stereo_pair(1 + i, h, w)
        ol = po.OracleExtractor(height=h, width=w, n_levels=L, tile_h=tile, tile_w=tile)
        orr = po.OracleExtractor(height=h, width=w, n_levels=L, tile_h=tile, tile_w=tile)
        ol.extract(left)
        orr.extract(right)
        ou, od, ost = po.stereo_match(ol, orr, bf / fx, bf)
        nl, nr = len(ol.keypoints()) // 6, len(orr.keypoints()) // 6
        assert got["counts"][i].tolist() == [nl, nr, ost["n_final"]], i
        if i in got["sample_pairs"]:
            sl, sr = slice(lo, lo + nl), slice(ro, ro + nr)
            assert np.array_equal(got["left_keypoints"][sl], ol.keypoints().reshape(6, -1).T) and np.array_equal(got["left_descriptors"][sl], ol.descriptors()), i
            assert np.array_equal(got["right_keypoints"][sr], orr.keypoints().reshape(6, -1).T) and np.array_equal(got["right_descriptors"][sr], orr.descriptors()), i
            assert np.array_equal(got["u_right"][sl].view(np.uint32), ou.view(np.uint32)) and np.array_equal(got["depth"][sl].view(np.uint32), od.view(np.uint32)), i
            lo, ro = lo + nl, ro + nr
    assert lo == len(got["left_keypoints"]) == len(got["u_right"]) and ro == len(got["right_keypoints"]) and lo > 0
