"""GPU: the frontier policy (csrc/nbp_frontier.hip) against its numpy definition (nextbestpath_amd/utility/frontier.py), bit for bit,
and as a drop-in for the network in Rollout, MultiRollout and the test driver."""
import json
import os

import numpy as np
import pytest
import torch

import frontier_cases as fc
from nextbestpath_amd.utility import frontier as fr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _policy(maps, R, d, unknown, penalty):
    """The device policy into NaN-filled buffers: every element must be written."""
    from nextbestpath_amd.utility import hipops
    B, S = maps.shape[0], maps.shape[-1]
    out = (torch.full((B, 8, S // 4, S // 4), float("nan"), device="cuda"), torch.full((B, 1, S, S), float("nan"), device="cuda"))
    o1, o2 = hipops.frontier_policy(torch.from_numpy(maps).cuda(), R, d, unknown, penalty, out=out)
    assert o1 is out[0] and o2 is out[1]
    return o1.cpu().numpy(), o2.cpu().numpy()


@pytest.mark.parametrize("name,d", sorted({(c[0], c[2]) for c in fc.POLICY_CASES}))
def test_mask_against_the_definition(hip, name, d):
    from nextbestpath_amd.utility import hipops
    maps = fc.case(name)
    bits, unknown = hipops.frontier_mask(torch.from_numpy(maps).cuda(), d, want_unknown=True)
    only = hipops.frontier_mask(torch.from_numpy(maps).cuda(), d)
    f, u = fc.classes(name, d)
    assert np.array_equal(_u64(bits), fr.pack_bits(f))
    assert np.array_equal(_u64(unknown), fr.pack_bits(u))
    assert torch.equal(only, bits)


@pytest.mark.parametrize("name,R,d,unknown,penalty", fc.POLICY_CASES)
def test_policy_against_the_definition(hip, name, R, d, unknown, penalty):
    o1, o2 = _policy(fc.case(name), R, d, unknown, penalty)
    w1, w2 = fc.reference(name, R, d, unknown, penalty)
    assert o1.dtype == np.float32 and o1.shape == w1.shape and o2.shape == w2.shape
    assert np.array_equal(o2, w2)
    assert np.array_equal(o1, w1), np.argwhere(o1 != w1)[:5]


def test_a_batch_is_its_items_and_two_runs_agree(hip):
    maps = np.stack([fc.random_item(128, 40 + i, (0.02, 0.2, 0.5, 0.8, 0.97)[i]) for i in range(5)])
    o1, o2 = _policy(maps, 31, 2, "obstacle", 1)
    again = _policy(maps, 31, 2, "obstacle", 1)
    assert np.array_equal(o1, again[0]) and np.array_equal(o2, again[1])                  # determinism
    assert o1.max() > 0 and o2.max() == 1.0
    for i in range(5):
        s1, s2 = _policy(maps[i:i + 1], 31, 2, "obstacle", 1)
        assert np.array_equal(s1[0], o1[i]) and np.array_equal(s2[0], o2[i]), i


def test_refusals_by_return_code(hip):
    B, S = 2, 128
    V, W = S // 4, S // 64
    maps = torch.zeros(B, 6, S, S, device="cuda")
    out1 = torch.full((B, 8, V, V), 7.0, device="cuda")
    out2 = torch.full((B, 1, S, S), 7.0, device="cuda")
    bits = torch.full((B, S, W), 7, dtype=torch.int64, device="cuda")
    need = hip.nbp_frontier_workspace_bytes(B, S)
    assert need == 5 * B * S * W * 8
    assert hip.nbp_frontier_workspace_bytes(0, S) == 0 and hip.nbp_frontier_workspace_bytes(B, 96) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    E_ARG, E_WS, E_SHAPE = -1, -2, -3

    def policy(maps6=p(maps), B=B, S=S, R=24, d=2, pen=0, o1=p(out1), o2=p(out2), w=p(ws), nbytes=need):
        return hip.nbp_frontier_policy_f32(maps6, B, S, R, d, 1, pen, o1, o2, w, nbytes, st)

    def mask(maps6=p(maps), B=B, S=S, d=2, f=p(bits), u=None, w=p(ws), nbytes=need):
        return hip.nbp_frontier_mask_u64(maps6, B, S, d, f, u, w, nbytes, st)

    assert policy(S=96) == E_SHAPE and policy(S=100) == E_SHAPE and mask(S=96) == E_SHAPE
    assert policy(B=0) == E_ARG and policy(B=-1) == E_ARG and mask(B=0) == E_ARG
    assert policy(R=0) == E_ARG and policy(R=32) == E_ARG
    assert policy(d=-1) == E_ARG and policy(d=9) == E_ARG and mask(d=-1) == E_ARG and mask(d=9) == E_ARG
    assert policy(pen=-1) == E_ARG
    assert policy(maps6=None) == E_ARG and policy(o1=None) == E_ARG and policy(o2=None) == E_ARG and policy(w=None) == E_ARG
    assert mask(maps6=None) == E_ARG and mask(f=None) == E_ARG and mask(w=None) == E_ARG
    assert policy(nbytes=need - 1) == E_WS and mask(nbytes=4 * need // 5 - 1) == E_WS
    torch.cuda.synchronize()
    assert (out1 == 7).all() and (out2 == 7).all() and (bits == 7).all() and not ws.any()      # nothing was launched
    assert policy() == 0 and mask(nbytes=4 * need // 5) == 0
    torch.cuda.synchronize()
    assert (out1 == 0).all() and (out2[:, :, 1:, 1:] == 1).all() and (bits == 0).all()


# ---------------------------------------------------------------------------------------------------------------- drop-in
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    d = tmp_path_factory.mktemp("frontier")
    for i in range(2):
        make_maze_scene(str(d / f"maze_{i:02d}"), seed=31 + i, cells=4, size=2.4, height=1.2, tess=0.3)
    return str(d)


def _small_params():
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    params.n_gt_surface_points = 3000
    return params


GRID, STEPS = 128, 8


def _host_policy(options):
    """The policy through the numpy definition: copies the maps back every step, runs utility/frontier.py::policy_batch and
    uploads its outputs.  The reference of the drop-in test."""
    from nextbestpath_amd.testers.frontier_policy import FrontierPolicy

    class HostFrontierPolicy(FrontierPolicy):
        def forward_maps(self, maps6):
            self.calls += 1
            o1, o2 = fr.policy_batch(maps6.cpu().numpy(), **self._kernel_options())
            return (torch.from_numpy(np.ascontiguousarray(o1)).to(maps6.device),
                    torch.from_numpy(np.ascontiguousarray(o2)).to(maps6.device))
    return HostFrontierPolicy(options)
OPTIONS = {"name": "frontier", "radius": 24, "dilate": 2, "unknown": "obstacle", "distance_penalty": 1}


def _trace(ro, n):
    return ([tuple(p) for p in ro.camera.cam_idx_history], [tuple(p) for p in ro.path], ro.n_replans, ro.coverage_evolution(n))


def _build(policy, ds, params, k):
    from nextbestpath_amd.testers import nbp_planning as tp
    return tp.build_rollout(params, policy, ds, (k % 2, 0), torch.device("cuda"), seed=70 + k, grid=GRID)


@pytest.fixture(scope="module")
def singles(hip, dataset):
    """Three rollouts of 8 steps under the device policy, each alone: (their traces, the policy's call count)."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers.frontier_policy import FrontierPolicy
    params, ds = _small_params(), sc.SceneDataset(dataset)
    policy = FrontierPolicy(OPTIONS)
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
    o1, _ = fr.policy(ro.st.maps6.cpu().numpy(), **{k: v for k, v in OPTIONS.items() if k != "name"})
    assert o1.max() > 0                                                                  # the planner was given values to rank


def test_lock_step_rollouts_equal_the_rollouts_alone(hip, dataset, singles):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.testers.frontier_policy import FrontierPolicy
    params, ds = _small_params(), sc.SceneDataset(dataset)
    policy = FrontierPolicy(OPTIONS)
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


def test_a_network_never_takes_the_policy_branch(hip, dataset, monkeypatch):
    """With a network in place of the policy the rollout runs the parent's code path: the policy branch is never entered, in a
    single rollout (both forms of its step) or in a lock-step group."""
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict

    def never(*a, **k):
        raise AssertionError("the policy branch was taken with a network")
    monkeypatch.setattr(tp, "_policy_forward", never)
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(9))
    net = net.cuda().eval()
    assert not tp._wants_maps(net)
    params, ds = _small_params(), sc.SceneDataset(dataset)
    traces = {}
    for overlap in (True, False):
        monkeypatch.setattr(tp, "_STEP_OVERLAP", overlap)
        ro = _build(net, ds, params, 0)
        for _ in range(4):
            ro.step()
        ro.finish()
        traces[overlap] = _trace(ro, 4)
    assert traces[True] == traces[False]
    ros = [_build(net, ds, params, 0), _build(net, ds, params, 1)]
    m = tp.MultiRollout(ros, net, torch.device("cuda"))
    for _ in range(4):
        m.step()
    m.flush()
    assert _trace(ros[0], 4) == traces[True]


def test_driver_writes_the_policy_into_every_record(hip, dataset, tmp_path):
    """The coverage figure is exact while the cloud holds fewer than twice the GT points, and a seeded sub-sample of the cloud
    beyond (nbp_coverage_count_f32), which is not monotone: the parameters here thin the cloud (gathering_factor 0.002: 21 frames of at
    most 234 points, under 5000 in all, against tens of thousands of GT points) so that five steps stay far below that, and the curve must then be non-decreasing."""
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
    got = tp.test_nbp_planning(results_json_file="frontier.json", policy="frontier", **common)
    assert len(got) == 2
    with open(tmp_path / "frontier.json") as fh:
        out = json.load(fh)
    assert sorted(out) == ["maze_00", "maze_01"]
    for scene in out.values():
        for rec in scene.values():
            assert rec["policy"] == {"name": "frontier", "radius": 24, "dilate": 2, "unknown": "free", "distance_penalty": 0}
            cov = rec["coverage"]
            assert len(cov) == 5 and all(b >= a for a, b in zip(cov, cov[1:])) and cov[-1] > 0
    for r in got:
        assert r["policy"]["name"] == "frontier" and 0 < r["n_points"] < 8000
    custom = tp.test_nbp_planning(results_json_file="frontier2.json", policy={"name": "frontier", "radius": 12, "distance_penalty": 2},
                                  **dict(common, n_poses=2))
    assert custom[0]["policy"] == {"name": "frontier", "radius": 12, "dilate": 2, "unknown": "free", "distance_penalty": 2}
    plain = tp.test_nbp_planning(results_json_file="plain.json", **dict(common, n_poses=2))
    with open(tmp_path / "plain.json") as fh:
        out = json.load(fh)
    assert all("policy" not in rec for scene in out.values() for rec in scene.values()) and all("policy" not in r for r in plain)
    for bad in ("macarons", {"name": "frontier", "radius": 40}, {"name": "frontier", "colour": 1}):
        with pytest.raises(ValueError):
            tp.test_nbp_planning(results_json_file="bad.json", policy=bad, **common)
    with pytest.raises(ValueError):
        tp.test_nbp_planning(results_json_file="bad.json", policy="frontier", symmetry_ensemble="c2", **common)
