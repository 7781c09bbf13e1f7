"""GPU: trajectory collection in lock-step groups (trajectory_collection(..., rollouts_per_gpu=K)) -- the three group-form entry
points against the single-rollout path they replace (bit for bit), and the group driver's records against the serial collector's
(byte for byte, same order)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL_POSES = [(0.0, 3.3, 0.0), (7.3, 5.0, -11.9), (-30.0, 1.0, 25.0), (100.0, 3.0, 0.0)]     # test_gpu_training_data's


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    d = tmp_path_factory.mktemp("synth_lockstep")
    for i in range(4):
        make_maze_scene(str(d / f"maze_{i:02d}"), seed=10 + i, cells=6, size=4.8, height=1.2, tess=0.4, hull="shell")
    return str(d)


def _meshes(dataset, n):
    from nextbestpath_amd.simulator import scene as sc
    ds = sc.SceneDataset(dataset)
    return [sc.load_scene(os.path.join(ds.data_path, ds[i]["scene_name"], ds[i]["obj_name"]), 10.0, torch.device("cuda"))
            for i in range(n)]


def _net():
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(9))
    return net.cuda().eval()


def test_label_batch_equals_single_calls(hip, dataset):
    from nextbestpath_amd.utility import hipops
    meshes = _meshes(dataset, 3)
    items = [(m.verts, m.faces, p[1], p[0], p[2]) for m in meshes for p in LABEL_POSES]
    got = hipops.slice_obstacle_fig_batch(items).cpu().numpy()
    for k, (v, f, y0, cx, cz) in enumerate(items):
        ref = hipops.slice_obstacle_fig(v, f, y0, cx, cz).cpu().numpy()
        assert np.array_equal(got[k], ref), k
        assert (ref.sum() == 0) if cx > 50 else (ref.sum() > 50)
    # more than 16 poses go in chunks; the 512 grid too
    big = hipops.slice_obstacle_fig_batch(items + items[:6], 512, 160.0).cpu().numpy()
    for k, (v, f, y0, cx, cz) in enumerate(items + items[:6]):
        assert np.array_equal(big[k], hipops.slice_obstacle_fig(v, f, y0, cx, cz, 512, 160.0).cpu().numpy()), k
    # n = 0 and n = 17 are refused
    out = torch.zeros(17, 256, 256, device="cuda")
    VP, I = C.c_void_p, C.c_int
    ve, fa, nf = (VP * 17)(*[meshes[0].verts.data_ptr()] * 17), (VP * 17)(*[meshes[0].faces.data_ptr()] * 17), \
        (I * 17)(*[meshes[0].faces.shape[0]] * 17)
    pose = np.zeros((17, 3), np.float32)
    geo = hipops.reference_figure_geometry(256, 80.0)
    for n in (0, 17):
        rc = hip.nbp_slice_obstacle_fig_batch_f32(n, ve, fa, nf, pose.ctypes.data, 256, *geo, out.data_ptr(), None)
        assert rc == -1, (n, rc)


def _torch_goal_values(pos, pose, o1, V, gr):
    """CollectionRollout._replan's expression."""
    from nextbestpath_amd.utility import utils as hu
    p2d = hu.transform_points_to_n_pieces(pos, pose)
    cells = hu.get_point_position_in_the_img(p2d.squeeze(0), (V, V), gr).reshape(2, -1)
    ok = (cells[0] >= 0) & (cells[0] < V) & (cells[1] >= 0) & (cells[1] < V)
    vals = o1.amax(0)[cells[0].clamp(0, V - 1), cells[1].clamp(0, V - 1)]
    return cells.cpu().numpy(), ok.cpu().numpy(), vals.cpu().numpy()


def test_goal_values_batch_equals_replan_expression(hip):
    from nextbestpath_amd.utility import hipops
    V, gr = 64, (-40, 40)
    net = _net()
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(3, 5, 256, 256, generator=g) > 0.97).float().cuda()
    with torch.no_grad():
        out1, _ = net(x)
    rng = np.random.default_rng(5)
    poses = [(1.7, 2.0, -3.1, 0.0, 0.0), (-12.25, 1.0, 7.5, 0.0, 0.0), (0.0, 3.0, 0.0, 0.0, 0.0)]
    # nodes on half-cell edges ((v + 40) * 0.8 = k + 0.5), exactly on the window's edges, and far outside it
    k = np.arange(-3, 68, dtype=np.float64)
    edge = 40.0 - (k + 0.5) / 0.8
    lat = []
    for j, (cx, cy, cz, _, _) in enumerate(poses):
        e_z = np.stack([np.full_like(edge, cx), np.full_like(edge, 1.0), cz + edge], 1)
        e_x = np.stack([cx + edge, np.full_like(edge, 1.0), np.full_like(edge, cz + 0.3)], 1)
        rnd = np.stack([rng.uniform(-70, 70, 300), rng.uniform(0, 3, 300), rng.uniform(-70, 70, 300)], 1)
        lat.append(torch.from_numpy(np.concatenate([e_z, e_x, rnd])[: 400 + 37 * j].astype(np.float32)).cuda())
    items, outs = [], []
    for j, pos in enumerate(lat):
        P = pos.shape[0]
        cell, val = torch.empty(P, dtype=torch.int32, device="cuda"), torch.empty(P, dtype=torch.float32, device="cuda")
        items.append((pos, (poses[j][0], poses[j][2]), out1[j].reshape(8, V, V).contiguous(), cell, val))
        outs.append((cell, val))
    hipops.goal_values_batch(items, V, gr)
    n_out = n_edge = 0
    for j, pos in enumerate(lat):
        cells, ok, vals = _torch_goal_values(pos, poses[j], out1[j], V, gr)
        cell, val = outs[j][0].cpu().numpy(), outs[j][1].cpu().numpy()
        assert np.array_equal(cell >= 0, ok)
        assert np.array_equal(cell[ok], (cells[0] * V + cells[1])[ok])
        assert np.array_equal(val.view(np.int32), vals.view(np.int32))
        n_out += int((~ok).sum())
        n_edge += int(ok[:71].sum())
    assert n_out > 100 and n_edge > 100


def test_hindsight_cells_batch_equals_per_experience_path(hip):
    from nextbestpath_amd.utility import hipops
    from nextbestpath_amd.utility import utils as hu
    V, gr = 64, (-40, 40)
    rng = np.random.default_rng(11)
    segs = []
    # poses 1.25 units apart along x and z: every difference is a multiple of 1.25 = one cell (0.625 = half a cell edge)
    segs.append(np.stack([np.arange(20) * 0.625 - 3.0, np.ones(20), -np.arange(20) * 1.875 + 2.0], 1))
    segs.append(np.stack([rng.uniform(-60, 60, 33), rng.uniform(0, 3, 33), rng.uniform(-60, 60, 33)], 1))     # many outside
    segs.append(np.array([[5.0, 1.0, 5.0]]))
    segs.append(np.stack([np.full(7, 10.0), np.ones(7), 10.0 + 40.0 * np.array([0, 0.5, 0.99, 1.0, 1.0 - 0.625 / 40, 1.2, -1.0])], 1))
    items, outs = [], []
    for s in segs:
        xz = torch.from_numpy(s[:, [0, 2]].astype(np.float32)).cuda().contiguous()
        c = torch.empty(len(s), len(s), dtype=torch.int32, device="cuda")
        items.append((xz, c))
        outs.append(c)
    hipops.hindsight_cells_batch(items, V, gr)
    n_in = n_out = 0
    for s, c in zip(segs, outs):
        got = c.cpu().numpy()
        m = len(s)
        for a in range(m):
            assert (got[a, :a + 1] == -1).all()
            later = s[a + 1:]
            if not len(later):
                continue
            pts = torch.tensor([list(p) for p in later.tolist()], dtype=torch.float32, device="cuda")
            p2d = hu.transform_points_to_n_pieces(pts, list(s[a]))
            rc = hu.get_point_position_in_the_img(p2d.squeeze(0), (V, V), gr).reshape(2, -1).cpu().numpy()
            ok = (rc[0] >= 0) & (rc[0] < V) & (rc[1] >= 0) & (rc[1] < V)
            want = np.where(ok, rc[0] * V + rc[1], -1)
            assert np.array_equal(got[a, a + 1:], want), (a, got[a, a + 1:], want)
            n_in += int(ok.sum())
            n_out += int((~ok).sum())
    assert n_in > 100 and n_out > 100


class _Subset:
    def __init__(self, ds, n):
        self.ds, self.n, self.data_path = ds, n, ds.data_path

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.ds[i]


def _collect_subset(dataset, tmp_path, name, n_scenes, K, n_poses=40):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility import nbp_utils as nu
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    params.n_poses_in_trajectory = 30
    ds = _Subset(sc.SceneDataset(dataset), n_scenes)
    env = nu.LogEnv(str(tmp_path / name))
    cov = []
    n = nu.trajectory_collection(params, 1, ds, env, (256, 256), (64, 64), (-40, 40), _net(), cov, None, torch.device("cuda"),
                                 n_poses=n_poses, n_gt_points=8000, rollouts_per_gpu=K)
    return n, cov, [v for _, v in env.items()]


@pytest.mark.parametrize("n_scenes,K", [(4, 3), (3, 16)])
def test_lockstep_collection_equals_serial(hip, dataset, tmp_path, n_scenes, K):
    """K = 3 over 4 scenes (a slot is refilled) and K = 16 over 3: the same records, byte for byte, in the same order."""
    n1, cov1, v1 = _collect_subset(dataset, tmp_path, "serial", n_scenes, 1)
    nk, covk, vk = _collect_subset(dataset, tmp_path, f"k{K}", n_scenes, K)
    assert n1 > 0 and nk == n1 == len(v1) == len(vk)
    assert cov1 == covk and len(cov1) > 0
    for i, (a, b) in enumerate(zip(v1, vk)):
        assert a == b, f"record {i} differs"


def test_train_entry_point_with_lockstep_collection(hip, dataset, tmp_path):
    cfg = json.load(open(os.path.join(ROOT, "configs/nbp/nbp_default_training_config.json")))
    cfg["_data"]["data_path"] = dataset
    cfg["_scene_management"]["n_gt_surface_points"] = 8000
    cfg["_nbp"].update({"nbp_model_name": "nbp_t", "nbp_batch_size": 4, "epochs": 1, "inner_epochs": 1, "n_validation": 4,
                        "n_collect_poses": 40, "output_dir": str(tmp_path / "w"), "collect": True, "collect_rollouts_per_gpu": 2})
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from nextbestpath_amd.testers.nbp_planning import load_params\n"
            "from nextbestpath_amd.trainers.train_nbp_model import run_training_nbp\n"
            "p = load_params(%r); assert p.collect_rollouts_per_gpu == 2\n"
            "h = run_training_nbp(p); print('HIST', h)\n") % (ROOT, str(path))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2500:]
    hist = json.load(open(tmp_path / "w" / "loss.json"))
    assert "1" in hist and np.isfinite(hist["1"]["training_loss"]) and np.isfinite(hist["1"]["validation_loss"])
    assert os.path.exists(tmp_path / "w" / "nbp_t_best_val.pth")
