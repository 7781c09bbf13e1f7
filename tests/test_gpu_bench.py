"""GPU: bench.py's contract -- one JSON line with roofline + cpu_baseline objects, and `--gpus N` launching N ranks
itself (here 2 ranks sharing the box's single GPU over gloo; RCCL needs one GPU per rank)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env=None, live=False):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--advance", "2",
                        "--rollouts-per-gpu", "2", "--no-extra-stages", "--strong-scenes", "3", "--strong-advance", "1"]
                       + ([] if live else ["--no-live-traffic"]) + extra,
                       capture_output=True, text=True, timeout=1200, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_single_gpu_line(hip):
    d = _run([])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "steps/s" and d["value"] > 0
    assert d["config"]["window_steps"] == [3, 6]
    rf, sc, cpu = d["roofline"], d["roofline_scatter"], d["cpu_baseline"]
    assert rf["bound"] == "mfma" and 0 < rf["frac"] <= 1 and rf["unit"] == "TFLOP/s"
    assert sc["bound"] == "hbm" and 0 < sc["frac"] <= 1 and sc["unit"] == "GB/s"
    assert d["strong_scaling"]["scenes_per_rank"] == [3] and d["strong_scaling"]["value"] > 0
    assert d["value_fp32_pipe"] is None         # --no-extra-stages: no fp32-pipe window
    assert sc["maps_equal_append_order_kernel"] is True and sc["side_list"] == 0 and sc["group_form"]["frac"] > 0
    # round 6: the single rollout's step as ONE launch (the filing un-projection in front of it), the two-launch form beside it
    one = sc["one_launch_form"]
    assert one["maps_equal_two_launch_build"] is True and one["store_in_step_after_40_filed_frames"] is True
    assert one["ms_build"] > 0 and sc["two_launch_form"]["ms"] > 0 and abs(sc["ms"] - (one["ms_build"] + one["filing_and_clear_ms"])) < 2e-4
    assert d["scatter_frac"] == sc["frac"] and d["scatter_frac_group_form"] == sc["group_form"]["frac"]
    assert d["tuning"] == {"active": False, "non_default_knobs": {}, "numerics_affecting": []}
    assert cpu["kind"] == "port" and cpu["value"] > 0 and set(cpu["legs_ms"]) == {"nbp_forward", "raster", "unproject",
                                                                                 "map_accumulate", "coverage"}


def test_bench_live_traffic_pass_finds_the_dominant_kernel(hip):
    """the rocprofv3 PMC passes bench.py runs itself must find the dominant kernel by the symbol the LIBRARY
    reports (nbp_tile_kernel_symbol) -- a name table in bench.py went stale when the kernel grew template parameters and the line
    silently carried a committed figure of an older round."""
    import shutil
    if not (shutil.which("rocprofv3") or os.path.exists("/opt/rocm/bin/rocprofv3")):
        pytest.skip("rocprofv3 not installed")
    d = _run(["--no-cpu-baseline", "--no-strong"], live=True)
    rf, sc = d["roofline"], d["roofline_scatter"]
    if "timed out" in rf["traffic_source"]:
        pytest.skip("the rocprofv3 pass timed out on this box (a slow host, not a lookup failure): " + rf["traffic_source"][:120])
    assert rf["kernel_symbol"].startswith("conv3x3_halo_h2_kernel<") and rf["kernel_symbol"].endswith(">")
    assert rf["traffic_is_live"] is True and rf["traffic_source"].startswith("rocprofv3"), rf["traffic_source"]
    assert rf["traffic"] > 0 and 0.5 < rf["traffic_over_algorithmic"] < 4.0
    assert sc["traffic_is_live"] is True and sc["traffic"] > 0
    assert all(k.startswith(("conv3x3_halo_h2_kernel<", "gate1x1_h2_kernel<", "tile ")) for k in rf["by_kernel"]), list(rf["by_kernel"])
    for key in ("train_maps_per_s", "bf16_512_b8_frac", "fwd_b1_ms", "single_rollout_steps_per_s", "lockstep_forward_share",
                "value_fp32_pipe", "all_conv_frac_executed", "roofline_traffic_is_live"):
        assert key in d                                      # top-level scalars (None for the stages --no-extra-stages skips)
    assert d["fwd_b1_ms"] > 0 and 0 < d["lockstep_forward_share"] < 2 and d["roofline_traffic_is_live"] is True


def test_bench_gpus_flag_launches_the_ranks(hip):
    d = _run(["--gpus", "2", "--no-cpu-baseline"], env={"NBP_DIST_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    assert d["value"] > 0 and abs(d["value"] - 3 * 2 * 2 / (d["ms_per_step"] * 3e-3)) < 1e-3 * d["value"]
    st = d["strong_scaling"]                # 3 fixed hard scenes over 2 ranks: 2 + 1, the job's time is the slower rank's
    assert st["scaling"] == "strong" and st["scenes_per_rank"] == [2, 1] and len(st["per_rank_s"]) == 2
    assert abs(st["value"] - 3 * 3 / (st["ms_per_step"] * 3e-3)) < 1e-3 * st["value"] and st["imbalance_max_over_mean"] >= 1.0
    assert st["ms_per_step"] * 3e-3 >= max(st["per_rank_s"]) - 1e-6            # the job's time is the slowest rank's (max over ranks)
    assert d["distributed"]["backend"] == "gloo" and d["distributed"]["world"] == 2
    di = d["distributed"]                   # what a reader needs to believe an N-GPU line: the ranks, their devices, their own seconds
    assert di["world_size_reported_by_backend"] == 2 and [r["rank"] for r in di["ranks"]] == [0, 1]
    assert all(r["device_uuid"] and r["timed_window_s"] > 0 for r in di["ranks"]) and len({r["pid"] for r in di["ranks"]}) == 2
    assert di["distinct_device_uuids"] == 1                 # (this test: two ranks sharing the box's one GPU over gloo)
    assert d["ms_per_step"] * 3e-3 >= max(r["timed_window_s"] for r in di["ranks"]) - 1e-4


def test_bench_plain_run_is_the_headline_and_dumps_its_outputs(hip, tmp_path):
    """Without --full: the headline alone (the other stages' fields are null), exactly --steps timed steps; --dump-outputs writes
    what the last timed step left the rollouts with, as float32 / float64 .npy files, and the same arguments write the same files."""
    import numpy as np
    runs = []
    for tag in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--advance", "2",
                            "--rollouts-per-gpu", "2", "--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        runs.append(json.loads(lines[0]))
    d = runs[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["config"]["window_steps"] == [3, 6] and abs(d["value"] - 3 * 2 / (d["ms_per_step"] * 3e-3)) < 1e-3 * d["value"]
    assert d["roofline"] is None and d["roofline_scatter"] is None and d["cpu_baseline"] is None and d["strong_scaling"] is None
    assert d["full_rollout"] is None and d["value_fp32_pipe"] is None and d["nbp_maps_per_s"] is None
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == ["cloud_count.npy", "cloud_sample.npy", "coverage.npy", "maps6_sample.npy",
                                                           "maps6_sample_rollouts.npy", "v_cam_history.npy", "x_cam_history.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    out = {n[:-len(".npy")]: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert out["coverage"].shape == (2, 6) and out["cloud_count"].shape == (2,) and (out["cloud_count"] > 0).all()
    assert out["maps6_sample"].shape == (2, 6, 256, 256) and out["maps6_sample"].sum() > 0
    assert out["x_cam_history"].shape[0] == 2 and out["x_cam_history"].shape[2] == 3
    for n in names:                                      # same arguments, same inputs: the same outputs, bit for bit
        assert np.array_equal(out[n[:-len(".npy")]], np.load(tmp_path / "b" / n), equal_nan=True), n


def test_bench_full_rollout_stage_runs_the_entry_point(hip):
    """VERDICT r05 Next 4: configs[1] as BASELINE.json words it, end to end -- bench.full_rollout writes a small synthetic simple set,
    runs `python test_nbp_planning.py -c <config>` as a child process and reports the wall clock with its setup / stepping / JSON
    breakdown (here 2 scenes x 6 poses)."""
    sys.path.insert(0, ROOT)
    import bench
    fr = bench.full_rollout(n_scenes=2, n_poses=6)
    assert "error" not in fr, fr
    assert fr["scenes"] == 2 and fr["poses"] == 6 and fr["runs"] == 2 and fr["steps"] == 12
    assert fr["wall_s"] > fr["in_process_s"] > fr["stepping_s"] > 0 and fr["setup_s"] > 0 and fr["gather_and_json_s"] >= 0
    assert abs(fr["steps_per_s_wall"] - 12 / fr["wall_s"]) < 0.01 * fr["steps_per_s_wall"] + 0.01
    assert 0.0 < fr["final_coverage_mean"] <= 1.0
    assert not os.path.exists(os.path.join(ROOT, "configs", "test", "_bench_full_rollout.json"))
