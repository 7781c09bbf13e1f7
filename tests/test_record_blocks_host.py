"""The tail of a test run on the host (testers/nbp_planning.py::collect_records): synthetic per-run results go through the coverage
gather and one float64 gather per block that is on, in a single process and as world 2 over gloo, and come out as the records of
the result JSON.  Rank 0 forms every block from the gathered float64 row; the other ranks keep none."""
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from nextbestpath_amd.utility import recon_metrics as rm
from nextbestpath_amd.utility import surface_metrics as sm
from nextbestpath_amd.utility import tsdf
from nextbestpath_amd.utility import view_metrics as vm

N_POSES, VIEWS, THRESHOLDS = 3, 3, [0.5, 1.0]
RUNS = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]          # five runs: under world 2, rank 1 has a pad row
SCENES = ["maze_a", "maze_b", "maze_c"]
PARAMS = dict(image_height=24, image_width=40, zfar=50.0, sensor_range=70.0)
ORDER = ["coverage", "auc", "reconstruction", "reconstruction_curve", "policy", "depth_noise", "depth_filter", "views", "fusion",
         "surface", "X_cam_history", "V_cam_history"]
BLOCKS = ["reconstruction", "reconstruction_curve", "views", "fusion", "surface"]
GATHERS = ["gather_reconstruction", "gather_reconstruction_curve", "gather_views", "gather_fusion", "gather_surface"]
ALL_ON = dict(recon_metrics={"thresholds": THRESHOLDS, "cap": 4.0, "curve": True}, view_metrics={"views": VIEWS}, fusion=True,
              surface_metrics={"thresholds": [0.05, 0.5, 1.0]}, policy="frontier", depth_noise={"sigma_base": 0.01},
              depth_filter={"range_base": 0.5})


def _options(**on):
    """resolve_options with every option given (None = off), so that no configuration file read earlier in the process speaks."""
    from nextbestpath_amd.testers import nbp_planning as tp
    return tp.resolve_options(**{**dict.fromkeys(tp._test_config), **on})


def _recon_raw(rng, n_thresholds, rid):
    """recon_metrics.pack_raw's vector with counts above 2^24 and sums that fp32 would not carry."""
    n_rec, n_gt = 20_000_000 + rid, 30_000_001 + 7 * rid
    return rm.pack_raw(rng.uniform(0, 1e6, 2) + 1e-9, rng.integers(0, n_rec, n_thresholds), n_rec, rng.uniform(0, 1e6, 2) + 1e-9,
                       rng.integers(0, n_gt, n_thresholds), n_gt)


def _raw(key, rid, opts):
    """Run rid's raw float64 numbers of the block `key`, as the modules' own pack functions lay them out."""
    rng = np.random.default_rng(100 * rid + BLOCKS.index(key))
    recon = opts.recon_metrics or rm.option_spec(True)
    T = len(recon["thresholds"])
    if key == "reconstruction":
        return _recon_raw(rng, T, rid)
    if key == "reconstruction_curve":
        return np.stack([_recon_raw(rng, T, rid + s) for s in range(N_POSES)])
    if key == "views":
        n = VIEWS - 1 if rid == 3 else VIEWS                     # one run reached fewer poses than the option asks for
        counts = np.zeros((n, len(vm.RAW_COUNTS)), np.int64)
        counts[:, 0] = 20_000_000 + rng.integers(0, 1000, n)     # n_gt
        counts[:, 2] = rng.integers(1, 10_000_000, n)            # n_hit
        counts[:, 1] = counts[:, 2] + rng.integers(0, 1000, n)   # n_c
        counts[:, 3:] = rng.integers(0, 1000, (n, 3))
        return vm.pack_raw(counts, rng.uniform(0, 1e6, (n, len(vm.RAW_SUMS))) + 1e-9)
    if key == "fusion":
        return tsdf.pack_raw(_recon_raw(rng, T, rid), 2 ** 27 + rid, 2 ** 25 + 3 * rid, 505 - rid)
    Ts = len(opts.surface_metrics["thresholds"])
    n = 20_000_000 + rid
    cloud = sm.pack_raw(rng.uniform(0, 1e6, 2) + 1e-9, rng.integers(0, n, Ts), n)
    fused = sm.pack_raw(rng.uniform(0, 1e4, 2) + 1e-9, rng.integers(0, 70_000, Ts), 70_001 + rid) if opts.fusion is not None else None
    return sm.pack_record(cloud, fused, {"faces": 2 ** 25 + rid, "faces_used": 2 ** 25 - rid, "entries": 2 ** 30 + 3 * rid})


def _view_options(opts):
    return vm.resolved_options(opts.view_metrics, PARAMS["image_height"], PARAMS["image_width"], PARAMS["zfar"])


def _want(key, rid, opts):
    """The block that the module's own summariser forms from run rid's raw numbers."""
    raw = _raw(key, rid, opts)
    recon = opts.recon_metrics or rm.option_spec(True)
    if key == "reconstruction":
        return rm.summarise_raw(raw, recon["thresholds"], recon["cap"])
    if key == "reconstruction_curve":
        return rm.summarise_curve(raw, recon["thresholds"], recon["cap"])
    if key == "views":
        return vm.summarise_raw(raw, _view_options(opts))
    if key == "fusion":
        return tsdf.summarise_raw(raw, recon["thresholds"], recon["cap"], tsdf.resolved_options(opts.fusion, PARAMS["sensor_range"]))
    return sm.summarise_record(raw, opts.surface_metrics)


def _blocks_on(opts):
    on = {"reconstruction": opts.recon_metrics is not None,
          "reconstruction_curve": opts.recon_metrics is not None and bool(opts.recon_metrics.get("curve")),
          "views": opts.view_metrics is not None, "fusion": opts.fusion is not None, "surface": opts.surface_metrics is not None}
    return [key for key in BLOCKS if on[key]]


def _result(run, opts):
    """What run_many returns for one run, with a wrong, locally formed block under every record key that is on."""
    from nextbestpath_amd.testers import nbp_planning as tp
    rid = RUNS.index(run)
    res = {"scene": SCENES[run[0]], "start": run[1], "coverage": [0.125 * (s + 1) + rid / 64 for s in range(N_POSES)],
           "X_cam_history": [[float(rid), 0.0, 1.0]], "V_cam_history": [[0.0, float(rid)]], "n_points": 1000 + rid}
    res.update(tp.run_tags(opts.policy_spec, opts.depth_noise, opts.depth_filter))
    for key in _blocks_on(opts):
        res[key] = {"formed_locally": rid}
        res[key + "_raw"] = _raw(key, rid, opts).tolist()
    if "views" in res:
        res["views"]["options"] = _view_options(opts)            # (what the driver checks on every rank)
    return res


def _collect(rank, world, on):
    from nextbestpath_amd import parallel_rollout as pr
    from nextbestpath_amd.testers import nbp_planning as tp
    opts = _options(**on)
    mine = pr.shard(RUNS, rank, world)
    results = [_result(run, opts) for run in mine]
    return tp.collect_records(results, RUNS, mine, rank, world, torch.device("cpu"), opts, SimpleNamespace(**PARAMS), N_POSES, SCENES)


def _check_rank0(gathered, out, on):
    opts = _options(**on)
    blocks = _blocks_on(opts)
    tags = [k for k in ("policy", "depth_noise", "depth_filter") if on.get(k) is not None]
    assert [r["run_id"] for r in gathered] == list(range(len(RUNS)))
    assert sorted(out) == SCENES and sum(len(v) for v in out.values()) == len(RUNS)
    for r in gathered:
        rid = r["run_id"]
        assert not [k for k in r if k.endswith("_raw")]
        rec = out[SCENES[RUNS[rid][0]]][str(RUNS[rid][1])]
        histories = [k for k in ("X_cam_history", "V_cam_history") if k in r]         # (this rank's own runs carry them)
        assert list(rec) == [k for k in ORDER if k in ["coverage", "auc"] + blocks + tags + histories]
        for key in BLOCKS:
            assert (key in r) == (key in rec) == (key in blocks)
        for key in blocks:
            assert r[key] == rec[key] == _want(key, rid, opts), (key, rid)            # float64 all the way: equal, not close
        assert rec["coverage"] == r["coverage"] and rec["auc"] == r["auc"] and len(rec["coverage"]) == N_POSES
    return opts


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from nextbestpath_amd import parallel_rollout as pr
    r, w, _ = pr.init_distributed()
    q.put((r, _collect(r, w, ALL_ON)))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_all_blocks_on_world2():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    opts = _check_rank0(*got[0], ALL_ON)
    assert _blocks_on(opts) == BLOCKS
    out = got[0][1]
    assert "X_cam_history" in out["maze_a"]["0"] and "X_cam_history" not in out["maze_a"]["1"]     # rank 1's histories stay there
    assert out["maze_b"]["1"]["views"]["n_views"] == VIEWS - 1 and out["maze_a"]["0"]["views"]["n_views"] == VIEWS
    assert out["maze_c"]["0"]["fusion"]["n_points"] == 20_000_004 and "fused" in out["maze_c"]["0"]["surface"]
    gathered, none = got[1]
    assert none is None and [r["run_id"] for r in gathered] == list(range(len(RUNS)))
    for r in gathered:                                           # the other ranks lose the blocks and their raw keys
        assert not [k for k in r if k in BLOCKS or k.endswith("_raw")]


def test_all_blocks_on_single_process(monkeypatch):
    from nextbestpath_amd import parallel_rollout as pr
    calls = []
    for name in GATHERS:
        monkeypatch.setattr(pr, name, lambda *a, _name=name, _real=getattr(pr, name), **k: calls.append(_name) or _real(*a, **k))
    gathered, out = _collect(0, 1, ALL_ON)
    _check_rank0(gathered, out, ALL_ON)
    assert calls == GATHERS                                      # one gather per block, in the record's order
    assert all("X_cam_history" in rec for scene in out.values() for rec in scene.values())
    rec = out["maze_a"]["0"]
    assert list(rec) == ORDER and rec["policy"]["name"] == "frontier" and rec["depth_noise"]["sigma_base"] == 0.01
    assert rec["reconstruction"]["cap"] == 4.0 and [t["threshold"] for t in rec["fusion"]["thresholds"]] == THRESHOLDS
    assert len(rec["reconstruction_curve"]["chamfer"]) == N_POSES and rec["views"]["options"]["height"] == PARAMS["image_height"]


def test_only_fusion_on_borrows_the_reconstruction_defaults(monkeypatch):
    from nextbestpath_amd import parallel_rollout as pr
    calls = []
    for name in GATHERS:
        monkeypatch.setattr(pr, name, lambda *a, _name=name, _real=getattr(pr, name), **k: calls.append(_name) or _real(*a, **k))
    on = dict(fusion={"voxel": 0.5})
    gathered, out = _collect(0, 1, on)
    opts = _check_rank0(gathered, out, on)
    assert calls == ["gather_fusion"] and opts.recon_metrics is None
    for r in gathered:
        want = tsdf.summarise_raw(_raw("fusion", r["run_id"], opts), rm.DEFAULT_THRESHOLDS, rm.DEFAULT_CAP,
                                  {"voxel": 0.5, "trunc": 1.0, "min_weight": 1, "max_depth": PARAMS["sensor_range"]})
        assert r["fusion"] == want and r["fusion"]["cap"] == rm.DEFAULT_CAP and len(r["fusion"]["thresholds"]) == 1


def test_everything_off_enters_no_float64_gather(monkeypatch):
    from nextbestpath_amd import parallel_rollout as pr
    calls = []
    for name in GATHERS:
        monkeypatch.setattr(pr, name, lambda *a, _name=name, **k: calls.append(_name) or {})
    gathered, out = _collect(0, 1, {})
    _check_rank0(gathered, out, {})
    assert calls == []
    assert all(list(rec) == ["coverage", "auc", "X_cam_history", "V_cam_history"] for scene in out.values() for rec in scene.values())


def test_views_made_with_other_options_are_refused():
    from nextbestpath_amd import parallel_rollout as pr
    from nextbestpath_amd.testers import nbp_planning as tp
    opts = _options(view_metrics={"views": VIEWS})
    mine = pr.shard(RUNS, 0, 1)
    results = [_result(run, opts) for run in mine]
    results[2]["views"]["options"] = dict(results[2]["views"]["options"], height=PARAMS["image_height"] + 1)
    with pytest.raises(RuntimeError, match="view_metrics: run 2"):
        tp.collect_records(results, RUNS, mine, 0, 1, torch.device("cpu"), opts, SimpleNamespace(**PARAMS), N_POSES, SCENES)


# ---------------------------------------------------------------------------------------------------------------- the table itself
class _StubRollout:
    """A finished rollout as _result reads it, with every observer on; records which methods are called, and with what."""

    def __init__(self, opts):
        self.calls = []
        self.scene_name, self.start, self.nbp, self.params = "maze_a", 0, object(), SimpleNamespace(**PARAMS)
        self.camera = SimpleNamespace(X_cam_history=torch.zeros(2, 3), V_cam_history=torch.zeros(2, 2), depth_noise=None,
                                      depth_filter=None, image_height=PARAMS["image_height"], image_width=PARAMS["image_width"])
        self.st = SimpleNamespace(cloud_count=torch.tensor([1234]))
        self.recon_spec, self.view_spec = opts.recon_metrics, opts.view_metrics
        self.fusion_spec, self.surface_spec = opts.fusion, opts.surface_metrics
        self.fusion = None if opts.fusion is None else object()
        self._opts = opts

    def coverage_evolution(self, n):
        return [0.25] * n

    def fused_cloud(self):
        self.calls.append("fused_cloud")
        return "points", 7

    def _measured(self, name, key, fused="absent"):
        self.calls.append(name)
        if self.fusion is not None and fused != "absent":
            assert fused == ("points", 7), (name, fused)         # the caller's extraction is handed on, never repeated
        return _raw(key, 0, self._opts)

    def reconstruction_metrics(self, raw=False):
        return self._measured("reconstruction_metrics", "reconstruction")

    def reconstruction_curve(self, n, raw=False):
        assert n == N_POSES
        return self._measured("reconstruction_curve", "reconstruction_curve")

    def view_metrics(self, raw=False):
        return self._measured("view_metrics", "views")

    def fusion_metrics(self, raw=False, fused=None):
        return self._measured("fusion_metrics", "fusion", fused)

    def surface_metrics(self, raw=False, fused=None):
        return self._measured("surface_metrics", "surface", fused)


def test_table_options_keys_and_one_fused_cloud_per_record():
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.testers import record_blocks as rb
    assert [b.key for b in rb.BLOCKS] == BLOCKS and len({b.key for b in rb.BLOCKS}) == len(rb.BLOCKS)
    assert {b.option for b in rb.BLOCKS} <= set(tp._test_config) and set(tp.OBSERVER_OPTIONS) == {b.option for b in rb.BLOCKS}
    assert [b.gather for b in rb.BLOCKS] == GATHERS
    opts = _options(**ALL_ON)
    assert rb.blocks_on(opts) == rb.BLOCKS and rb.blocks_on(_options()) == ()
    assert [b.key for b in rb.blocks_on(_options(recon_metrics=True, surface_metrics=True))] == ["reconstruction", "surface"]
    for block in rb.BLOCKS:                                      # a block alone, handed the record's extraction: asks for none
        ro = _StubRollout(opts)
        raw = block.measure(ro, N_POSES, ro.fused_cloud())
        assert ro.calls.count("fused_cloud") == 1 and len(ro.calls) == 2
        assert block.summarise(raw, *block.context(opts, SimpleNamespace(**PARAMS), N_POSES)) == _want(block.key, 0, opts)
    ro = _StubRollout(opts)                                      # a whole record: one extraction, every block measured once, in order
    res = tp._result(ro, N_POSES)
    assert ro.calls == ["fused_cloud", "reconstruction_metrics", "reconstruction_curve", "view_metrics", "fusion_metrics",
                        "surface_metrics"]
    keys = [k for key in BLOCKS for k in (key, key + "_raw")]
    assert [k for k in res if k in keys] == keys
    for key in BLOCKS:
        assert res[key] == _want(key, 0, opts) and res[key + "_raw"] == _raw(key, 0, opts).tolist()
    off = _StubRollout(_options(view_metrics={"views": VIEWS}))  # without `fusion` nothing is extracted
    assert [k for k in tp._result(off, N_POSES) if k in keys] == ["views", "views_raw"] and off.calls == ["view_metrics"]
