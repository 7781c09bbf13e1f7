"""The entry driver with every end-of-rollout block on (reconstruction and its curve, views, fusion, surface): the records it writes
hold the blocks in the record's order, and each block is the one run_many forms for the same runs, seeds and options."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ["coverage", "auc", "reconstruction", "reconstruction_curve", "views", "fusion", "surface", "X_cam_history", "V_cam_history"]
BLOCKS = ORDER[2:7]
OPTIONS = dict(recon_metrics={"curve": True}, view_metrics={"views": 2}, fusion=True, surface_metrics=True)
N_POSES, SEED, TORCH_SEED = 3, 8, 9
GRID = 128                             # (tests/test_gpu_frontier.py's, and its two scenes)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    d = tmp_path_factory.mktemp("record_blocks")
    for i in range(2):
        make_maze_scene(str(d / f"maze_{i:02d}"), seed=31 + i, cells=4, size=2.4, height=1.2, tess=0.3)
    return str(d)


def test_driver_writes_every_block(hip, dataset, tmp_path):
    """The JSON's records hold exactly the record's key order; each of the five blocks, in the JSON and in the list the driver
    returns, equals the block of the per-run result that run_many forms for the same runs, seeds and options (exactly: the driver
    calls just that, the cloud's rows are assigned by an ordered compaction, the splat breaks depth ties by row, and every
    reduction behind a block has a fixed order); and each block is valid JSON without NaN.  Every block is compared before the
    verdict, which names the (scene, start, block) that differ."""
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    with open(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json")) as fh:
        cfg = json.load(fh)
    cfg["_camera_management"]["gathering_factor"] = 0.002        # the thinned cloud of test_gpu_frontier's driver test
    os.makedirs(tmp_path / "cfg")
    with open(tmp_path / "cfg" / "thin.json", "w") as fh:
        json.dump(cfg, fh)
    got = tp.test_nbp_planning(params_file="thin.json", model_file="none.pth", results_json_file="blocks.json", numGPU=0, test_scenes=[],
                               configs_dir=str(tmp_path / "cfg"), dataset_path=dataset, nbp_weights=None, results_dir=str(tmp_path),
                               n_poses=N_POSES, seed=SEED, torch_seed=TORCH_SEED, rollouts_per_gpu=2, grid_size=GRID, **OPTIONS)
    with open(tmp_path / "blocks.json") as fh:
        out = json.load(fh)
    assert sorted(out) == ["maze_00", "maze_01"] and len(got) == 2
    for scene in out.values():
        for rec in scene.values():
            assert list(rec) == ORDER                            # no policy, noise or filter here: their place is behind the curve
    # the same runs, seeds and options through run_many, as the driver calls it
    device = torch.device("cuda", 0)
    params = tp.load_params(str(tmp_path / "cfg" / "thin.json"))
    params.test_scenes = []
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(TORCH_SEED))
    net.to(device).eval()
    opts = tp.resolve_options(policy=None, symmetry_ensemble=None, depth_noise=None, depth_filter=None, **OPTIONS)
    net.symmetry_ensemble = params.symmetry_ensemble = opts.symmetry_ensemble
    ds = sc.SceneDataset(dataset, [])
    runs = tp.list_runs(ds, params)
    assert len(runs) == 2
    with torch.no_grad():
        results = tp.run_many(params, net, ds, runs, device, [SEED + 1000 * r[0] + r[1] for r in runs], 0.05, N_POSES, 2, GRID,
                              **opts.rollout)
    differ = []
    for (si, k), res, g in zip(runs, results, got):
        rec = out[ds[si]["scene_name"]][str(k)]
        assert g["run_id"] == runs.index((si, k)) and not [key for key in g if key.endswith("_raw")]
        for key in BLOCKS:
            print(key, res[key], rec[key])
            block = json.loads(json.dumps(res[key], allow_nan=False))
            # fixed-order reductions: the same bits, run to run (every block is looked at before the verdict)
            differ += [(si, k, key)] * (rec[key] != block or json.loads(json.dumps(g[key], allow_nan=False)) != block)
        assert rec["reconstruction"]["n_points"] == res["n_points"] > 0 and rec["views"]["n_views"] == 2
        assert rec["fusion"]["frames"] > 0 and "fused" in rec["surface"] and len(rec["reconstruction_curve"]["chamfer"]) == N_POSES
    assert not differ, differ
