"""GPU: the information-gain policy (csrc/nbp_infogain.hip) against its numpy definition (nextbestpath_amd/utility/infogain.py), bit
for bit, and as a drop-in for the network in Rollout, MultiRollout and the test driver."""
import json
import os

import numpy as np
import pytest
import torch

import infogain_cases as ic
from nextbestpath_amd.utility import infogain as ig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _policy(maps, R, d, unknown, penalty):
    """The device policy into NaN-filled buffers: every element must be written."""
    from nextbestpath_amd.utility import hipops
    B, S = maps.shape[0], maps.shape[-1]
    out = (torch.full((B, 8, S // 4, S // 4), float("nan"), device="cuda"), torch.full((B, 1, S, S), float("nan"), device="cuda"))
    o1, o2 = hipops.infogain_policy(torch.from_numpy(maps).cuda(), R, d, unknown, penalty, out=out)
    assert o1 is out[0] and o2 is out[1]
    return o1.cpu().numpy(), o2.cpu().numpy()


def _visible(maps, R, d, cells):
    """hipops.infogain_visible, unpacked -> bool [n, 2R+1, 2R+1]."""
    from nextbestpath_amd.utility import hipops
    words = hipops.infogain_visible(torch.from_numpy(maps).cuda(), R, d, cells).cpu().numpy().view(np.uint64)
    assert words.shape == (len(cells), 2 * R + 1)
    assert not (words >> np.uint64(2 * R + 1)).any()                                     # nothing beyond the window
    return ((words[:, :, None] >> np.arange(2 * R + 1, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)


@pytest.mark.parametrize("name,R,d,unknown,penalty", ic.POLICY_CASES)
def test_policy_against_the_definition(hip, name, R, d, unknown, penalty):
    o1, o2 = _policy(ic.case(name), R, d, unknown, penalty)
    w1, w2 = ic.reference(name, R, d, unknown, penalty)
    assert o1.dtype == np.float32 and o1.shape == w1.shape and o2.shape == w2.shape
    assert np.array_equal(o2, w2)
    assert np.array_equal(o1, w1), np.argwhere(o1 != w1)[:5]


@pytest.mark.parametrize("name,R,d", [("one_word", 31, 0), ("seam", 31, 0), ("seam", 24, 2), ("seam", 1, 0), ("s256", 31, 2),
                                      ("bands", 2, 8), ("rooms", 24, 0)])
def test_visible_masks_against_the_definition(hip, name, R, d):
    maps = ic.case(name)
    B, V = maps.shape[0], maps.shape[-1] // 4
    cells = ic.edge_cells(B, V)
    if name == "seam":                       # beside the seam, in the corridor, and under the diagonal wall
        cells = np.concatenate([cells, np.asarray([(0, 16, 15), (0, 16, 16), (0, 16, 17), (0, 20, 15), (0, 22, 18)], np.int32)])
    got = _visible(maps, R, d, cells)
    seen_any = False
    for b in range(B):
        pick = np.nonzero(cells[:, 0] == b)[0]
        want = ig.visible(maps[b], dilate=d, radius=R, cells=cells[pick, 1:])
        assert np.array_equal(got[pick], want), (b, [i for i in range(len(pick)) if not np.array_equal(got[pick][i], want[i])])
        seen_any |= bool(want.any())
    assert seen_any
    # more cells than one launch carries (128): the same masks again, in order
    many = np.concatenate([cells] * (300 // len(cells) + 1))[:300]
    again = _visible(maps, R, d, many)
    assert np.array_equal(again, got[np.arange(300) % len(cells)])


def test_the_masks_explain_the_gain(hip):
    """gain = popcount(visible & unknown & sector): the diagnostic call and the policy agree on the device."""
    from nextbestpath_amd.utility import frontier as fr
    maps, R, d = ic.case("seam"), 31, 0
    cells = ic.edge_cells(3, 32)
    vis = _visible(maps, R, d, cells)
    o1, _ = _policy(maps, R, d, "free", 0)
    table = fr.sector_table(R)
    for (b, g0, g1), v in zip(cells, vis):
        pad = np.zeros((128 + 2 * R, 128 + 2 * R), bool)
        pad[R:R + 128, R:R + 128] = fr.cell_classes(maps[b], d)["unknown"]
        win = pad[4 * g0:4 * g0 + 2 * R + 1, 4 * g1:4 * g1 + 2 * R + 1]
        assert np.array_equal(o1[b, :, g0, g1], (table & (v & win)[None]).sum((1, 2)).astype(np.float32)), (b, g0, g1)


def test_a_batch_is_its_items_and_two_runs_agree(hip):
    maps = ic.case("bands")
    o1, o2 = _policy(maps, 31, 2, "obstacle", 1)
    again = _policy(maps, 31, 2, "obstacle", 1)
    assert np.array_equal(o1, again[0]) and np.array_equal(o2, again[1])                  # determinism
    assert o1.max() > 0 and o2.max() == 1.0
    for i in range(len(maps)):
        s1, s2 = _policy(maps[i:i + 1], 31, 2, "obstacle", 1)
        assert np.array_equal(s1[0], o1[i]) and np.array_equal(s2[0], o2[i]), i


def test_refusals_by_return_code(hip):
    B, S, R = 2, 128, 24
    V, W = S // 4, S // 64
    maps = torch.zeros(B, 6, S, S, device="cuda")
    out1 = torch.full((B, 8, V, V), 7.0, device="cuda")
    out2 = torch.full((B, 1, S, S), 7.0, device="cuda")
    masks = torch.full((3, 2 * R + 1), 7, dtype=torch.int64, device="cuda")
    need = hip.nbp_infogain_workspace_bytes(B, S)
    assert need == 4 * B * S * W * 8
    assert hip.nbp_infogain_workspace_bytes(0, S) == 0 and hip.nbp_infogain_workspace_bytes(B, 96) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    E_ARG, E_WS, E_SHAPE = -1, -2, -3
    good = np.asarray([(0, 0, 0), (1, V - 1, V - 1), (1, V // 2, V // 2)], np.int32)

    def policy(maps6=p(maps), B=B, S=S, R=R, d=2, pen=0, o1=p(out1), o2=p(out2), w=p(ws), nbytes=need):
        return hip.nbp_infogain_policy_f32(maps6, B, S, R, d, 1, pen, o1, o2, w, nbytes, st)

    def visible(maps6=p(maps), B=B, S=S, R=R, d=2, cells=good, n=3, o=p(masks), w=p(ws), nbytes=need):
        return hip.nbp_infogain_visible_u64(maps6, B, S, R, d, None if cells is None else cells.ctypes.data, n, o, w, nbytes, st)

    assert policy(S=96) == E_SHAPE and policy(S=100) == E_SHAPE and visible(S=96) == E_SHAPE
    assert policy(B=0) == E_ARG and policy(B=-1) == E_ARG and visible(B=0) == E_ARG
    assert policy(R=0) == E_ARG and policy(R=32) == E_ARG and visible(R=0) == E_ARG and visible(R=32) == E_ARG
    assert policy(d=-1) == E_ARG and policy(d=9) == E_ARG and visible(d=-1) == E_ARG and visible(d=9) == E_ARG
    assert policy(pen=-1) == E_ARG
    assert policy(maps6=None) == E_ARG and policy(o1=None) == E_ARG and policy(o2=None) == E_ARG and policy(w=None) == E_ARG
    assert visible(maps6=None) == E_ARG and visible(cells=None) == E_ARG and visible(o=None) == E_ARG and visible(w=None) == E_ARG
    assert visible(n=0) == E_ARG and visible(n=-1) == E_ARG
    for bad in ((B, 0, 0), (-1, 0, 0), (0, V, 0), (0, -1, 0), (0, 0, V), (0, 0, -1)):
        cells = good.copy()
        cells[2] = bad
        assert visible(cells=cells) == E_ARG, bad
    assert policy(nbytes=need - 1) == E_WS and visible(nbytes=need - 1) == E_WS
    torch.cuda.synchronize()
    assert (out1 == 7).all() and (out2 == 7).all() and (masks == 7).all() and not ws.any()      # nothing was launched
    assert policy() == 0 and visible() == 0
    torch.cuda.synchronize()
    # nothing seen, nothing occupied: every cell of the domain counts its whole punctured disc, cut by the grid's edge
    assert (out1[:, :, 0] == 0).all() and (out1[:, :, :, 0] == 0).all() and (out2[:, :, 1:, 1:] == 1).all()
    n_disc = sum(1 for y in range(-R, R + 1) for x in range(-R, R + 1) if (y or x) and y * y + x * x <= R * R)
    assert out1[:, :, V // 2, V // 2].sum(1).tolist() == [n_disc] * B
    m = masks.cpu().numpy().view(np.uint64)
    assert not m[0].any() and (m[2] == np.uint64(2 ** (2 * R + 1) - 1)).sum() == 2 * R and m[2][R] == np.uint64((2 ** (2 * R + 1) - 1) ^ (1 << R))


# ---------------------------------------------------------------------------------------------------------------- drop-in
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    d = tmp_path_factory.mktemp("infogain")
    for i in range(2):
        make_maze_scene(str(d / f"maze_{i:02d}"), seed=31 + i, cells=4, size=2.4, height=1.2, tess=0.3)
    return str(d)


def _small_params():
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    params.n_gt_surface_points = 3000
    return params


GRID, STEPS = 128, 8
OPTIONS = {"name": "infogain", "radius": 24, "dilate": 2, "unknown": "obstacle", "distance_penalty": 1}


def _host_policy(options):
    """The policy through the numpy definition: copies the maps back every step, runs utility/infogain.py::policy_batch and
    uploads its outputs.  The reference of the drop-in test."""
    from nextbestpath_amd.testers.frontier_policy import InfoGainPolicy

    class HostInfoGainPolicy(InfoGainPolicy):
        def forward_maps(self, maps6):
            self.calls += 1
            o1, o2 = ig.policy_batch(maps6.cpu().numpy(), **self._kernel_options())
            return (torch.from_numpy(np.ascontiguousarray(o1)).to(maps6.device),
                    torch.from_numpy(np.ascontiguousarray(o2)).to(maps6.device))
    return HostInfoGainPolicy(options)


def _trace(ro, n):
    return ([tuple(p) for p in ro.camera.cam_idx_history], [tuple(p) for p in ro.path], ro.n_replans, ro.coverage_evolution(n))


def _build(policy, ds, params, k):
    from nextbestpath_amd.testers import nbp_planning as tp
    return tp.build_rollout(params, policy, ds, (k % 2, 0), torch.device("cuda"), seed=70 + k, grid=GRID)


@pytest.fixture(scope="module")
def singles(hip, dataset):
    """Three rollouts of 8 steps under the device policy, each alone: (their traces, the policy's call count)."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers.frontier_policy import InfoGainPolicy
    params, ds = _small_params(), sc.SceneDataset(dataset)
    policy = InfoGainPolicy(OPTIONS)
    traces = []
    for k in range(3):
        ro = _build(policy, ds, params, k)
        for _ in range(STEPS):
            ro.step()
        ro.finish()
        traces.append(_trace(ro, STEPS))
    return traces, policy.calls


def test_single_rollout_under_the_device_policy_is_the_one_under_the_definition(hip, dataset, singles):
    from nextbestpath_amd.simulator import scene as sc
    params, ds = _small_params(), sc.SceneDataset(dataset)
    host = _host_policy(OPTIONS)
    ro = _build(host, ds, params, 0)
    for _ in range(STEPS):
        ro.step()
    ro.finish()
    want = _trace(ro, STEPS)
    got = singles[0][0]
    assert host.calls == STEPS and singles[1] == 3 * STEPS
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and got[3] == want[3]
    assert want[2] >= 1 and want[3][-1] > 0 and len(set(want[0])) > 2                    # it replans, covers and travels
    o1, _ = ig.policy(ro.st.maps6.cpu().numpy(), **{k: v for k, v in OPTIONS.items() if k != "name"})
    assert o1.max() > 0                                                                  # the planner was given values to rank


def test_lock_step_rollouts_equal_the_rollouts_alone(hip, dataset, singles):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.testers.frontier_policy import InfoGainPolicy
    params, ds = _small_params(), sc.SceneDataset(dataset)
    policy = InfoGainPolicy(OPTIONS)
    ros = [_build(policy, ds, params, k) for k in range(3)]
    m = tp.MultiRollout(ros, policy, torch.device("cuda"))
    assert len(m.groups) == 2
    for _ in range(STEPS):
        m.step()
    m.flush()
    assert policy.calls == 2 * STEPS
    for ro, want in zip(ros, singles[0]):
        assert _trace(ro, STEPS) == want
    with pytest.raises(ValueError):
        tp.MultiRollout(ros, policy, torch.device("cuda"), symmetry_ensemble="c2")
    with pytest.raises(ValueError):
        tp.Rollout(params, policy, ros[0].camera, ros[0].gt, ros[0].mesh, ros[0].mesh, ros[0].y_bins, torch.device("cuda"),
                   grid=GRID, symmetry_ensemble="d4")


def test_driver_writes_the_policy_into_every_record(hip, dataset, tmp_path):
    """The driver under `policy="infogain"`: as tests/test_gpu_frontier.py's, with the cloud thinned (gathering_factor 0.002) so that
    the coverage figure stays exact and the curve must be non-decreasing."""
    from nextbestpath_amd.testers import nbp_planning as tp
    with open(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json")) as fh:
        cfg = json.load(fh)
    assert cfg["_camera_management"]["gathering_factor"] == 0.05
    cfg["_camera_management"]["gathering_factor"] = 0.002
    os.makedirs(tmp_path / "cfg")
    with open(tmp_path / "cfg" / "thin.json", "w") as fh:
        json.dump(cfg, fh)
    common = dict(params_file="thin.json", model_file="none.pth", numGPU=0, test_scenes=[], configs_dir=str(tmp_path / "cfg"),
                  dataset_path=dataset, nbp_weights=None, results_dir=str(tmp_path), n_poses=5, rollouts_per_gpu=2, grid_size=GRID)
    default = {"name": "infogain", "radius": 24, "dilate": 2, "unknown": "free", "distance_penalty": 0}
    got = tp.test_nbp_planning(results_json_file="infogain.json", policy="infogain", **common)
    assert len(got) == 2
    with open(tmp_path / "infogain.json") as fh:
        out = json.load(fh)
    assert sorted(out) == ["maze_00", "maze_01"]
    for scene in out.values():
        for rec in scene.values():
            assert rec["policy"] == default
            cov = rec["coverage"]
            assert len(cov) == 5 and all(b >= a for a, b in zip(cov, cov[1:])) and cov[-1] > 0
    for r in got:
        assert r["policy"] == default and 0 < r["n_points"] < 8000
    custom = tp.test_nbp_planning(results_json_file="infogain2.json", policy={"name": "infogain", "radius": 12, "distance_penalty": 2},
                                  **dict(common, n_poses=2))
    assert custom[0]["policy"] == dict(default, radius=12, distance_penalty=2)
    for bad in ("macarons", {"name": "infogain", "radius": 40}, {"name": "infogain", "colour": 1}, {"name": "infogain", "dilate": 9}):
        with pytest.raises(ValueError):
            tp.test_nbp_planning(results_json_file="bad.json", policy=bad, **common)
    with pytest.raises(ValueError):
        tp.test_nbp_planning(results_json_file="bad.json", policy="infogain", symmetry_ensemble="c2", **common)

