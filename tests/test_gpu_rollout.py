"""GPU: end-to-end exploration rollout on a procedural maze (short), invariants + determinism."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    d = tmp_path_factory.mktemp("synth")
    for i in range(2):
        make_maze_scene(str(d / f"maze_{i:02d}"), seed=i, cells=8, size=4.8, height=1.2, tess=0.3)
    return str(d)


def _net(nbp_weights):
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    net = NBP()
    net.load_state_dict(make_explorer_state_dict(9))
    return net.cuda().eval()


def test_short_rollout_invariants_and_determinism(hip, dataset, nbp_weights):
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    ds = sc.SceneDataset(dataset)
    net = _net(nbp_weights)
    runs = tp.list_runs(ds, params)
    assert len(runs) == 2
    n_poses = 12
    with torch.no_grad():
        a = tp.run_one(params, net, ds, runs[0], torch.device("cuda"), n_poses=n_poses, seed=5)
        b = tp.run_one(params, net, ds, runs[0], torch.device("cuda"), n_poses=n_poses, seed=5)
    cov = a["coverage"]
    assert len(cov) == n_poses and cov[0] == 0.0                       # empty cloud at step 0 (ref :457-460)
    assert all(0.0 <= c <= 1.0 for c in cov) and cov[-1] > 0.0
    X = np.asarray(a["X_cam_history"])
    assert X.shape == (1 + 4 + 4 * n_poses, 3)                          # 1 init + 4 first move + 4 per step
    step = np.linalg.norm(np.diff(X[4::4], axis=0), axis=1)            # lattice moves: 0 (turn) or 3 units
    assert np.all((np.abs(step) < 1e-4) | (np.abs(step - 3.0) < 1e-4))
    assert a["n_points"] > 1000
    assert np.abs(step - 3.0).min() < 1e-4                               # the agent actually travels
    assert a["coverage"] == b["coverage"] and a["X_cam_history"] == b["X_cam_history"]     # seeded => bit identical


def test_step_with_the_forward_on_its_own_stream_is_the_step_in_stream_order(hip, dataset, nbp_weights, monkeypatch, tmp_path):
    """Rollout.step runs the step's forward on a side stream (two input buffers used alternately; only a replanning step waits for
    it): the same trajectory, coverage, cloud and -- at the last step -- network input and outputs as with everything in stream
    order, and a RolloutState taken over by the next rollout starts clean."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    make_maze_scene(str(tmp_path / "m"), seed=115, cells=10, size=6.0, height=1.2, tess=0.25)      # bench.py's kind of scene
    ds0, ds1 = sc.SceneDataset(dataset), sc.SceneDataset(str(tmp_path), ["m"])
    net = _net(nbp_weights)
    dev = torch.device("cuda")
    got = {}
    for overlap in (False, True):
        monkeypatch.setattr(tp, "_STEP_OVERLAP", overlap)
        state = tp.RolloutState(dev)
        for ds, n_steps, seed in ((ds0, 9, 5), (ds1, 70, 23)):            # the second rollout reuses the first one's state
            ro = tp.build_rollout(params, net, ds, tp.list_runs(ds, params)[0], dev, state=state, seed=seed)
            replans = []
            for _ in range(n_steps):
                ro.step()
                replans.append(ro.need_replan)
            ro.finish()
            torch.cuda.synchronize()
        n = int(ro.st.cloud_count.item())
        with torch.no_grad():
            o1, o2 = net(ro.st.net_in)
        got[overlap] = (replans, ro.coverage_evolution(70), ro.camera.X_cam_history.tolist(), ro.st.cloud[:n].clone(),
                        ro.st.net_in.clone(), o1.clone(), o2.clone())
        assert (state._overlap is not None) == overlap
    a, b = got[False], got[True]
    assert a[0] == b[0], (a[0], b[0])
    assert any(a[0]) and sum(not r for r in a[0]) >= 10, a[0]        # steps of both kinds in the window
    assert a[1] == b[1] and a[2] == b[2]
    for x, y in zip(a[3:], b[3:]):
        assert torch.equal(x, y)


def test_entry_point_json_schema(hip, dataset, tmp_path):
    cfg = {"numGPU": 0, "dataset_path": dataset, "test_scenes": [], "params_name":
           "macarons_default_training_config.json", "model_name": "x.pth", "results_json_name": "out_test_entry.json",
           "test_resolution": 0.05, "use_perfect_depth_map": True, "compute_collision": False, "load_json": False,
           "random_seed": 8, "torch_seed": 9, "nbp_weights": "./weights/none.pth"}
    cfg_path = os.path.join(ROOT, "configs/test/_pytest_entry.json")
    with open(cfg_path, "w") as fh:
        json.dump(cfg, fh)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "test_nbp_planning.py"), "-c", "_pytest_entry.json",
                            "--n-poses", "3"], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = json.load(open(os.path.join(ROOT, "data", "out_test_entry.json")))
        assert sorted(out) == ["maze_00", "maze_01"]
        rec = out["maze_00"]["0"]
        assert set(rec) >= {"coverage", "X_cam_history", "V_cam_history"} and len(rec["coverage"]) == 3
    finally:
        os.remove(cfg_path)


def test_multi_rollout_matches_single(hip, dataset, nbp_weights):
    """Lock-step batched rollouts (B = 2 forward, shared sync) walk the same trajectories as separate runs."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    ds = sc.SceneDataset(dataset)
    net = _net(nbp_weights)
    dev = torch.device("cuda")

    def build(si, seed):
        sd = ds[si]
        settings = sc.Settings(sd["settings"], params.scene_scale_factor)
        mesh = sc.load_scene(os.path.join(ds.data_path, sd["scene_name"], sd["obj_name"]), params.scene_scale_factor, dev)
        _, gt = sc.setup_gt_scene(params, settings, mesh, dev, 0.05, seed=1, n_points=20000)
        cam = tp.setup_test_camera(params, mesh, settings.camera.start_positions[0], settings, dev, seed=seed)
        return tp.Rollout(params, net, cam, gt, mesh, mesh, sc.y_bins_for(mesh.verts_host, 4), dev, seed=seed)

    n = 10
    singles = [build(0, 3), build(1, 4)]
    for r in singles:
        for _ in range(n):
            r.step()
    multi_r = [build(0, 3), build(1, 4)]
    m = tp.MultiRollout(multi_r, net, dev)
    for _ in range(n):
        m.step()
    m.flush()
    for a, b in zip(singles, multi_r):
        assert a.camera.cam_idx_history == b.camera.cam_idx_history          # same goals, same paths, same headings
        assert np.array_equal(a.camera.X_cam_history, b.camera.X_cam_history)
        ca, cb = a.coverage_evolution(n), b.coverage_evolution(n)
        assert ca == cb


def test_multi_rollout_on_a_non_square_lattice(hip, nbp_weights, tmp_path):
    """the rollouts of a group keep their replanning results as ROWS of one buffer; a row holds float64 scores,
    so the row pitch must be a multiple of 8 whatever the lattice -- E = 2 W (2 L H - L - H) directed edges is a multiple of 8 on
    square lattices only (13 x 15 gives 724).  Four rollouts in two groups of two walk the single rollouts' trajectories."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    for i in range(2):
        make_maze_scene(str(tmp_path / f"rect_{i}"), seed=20 + i, cells=8, size=4.8, height=1.2, tess=0.3)
        path = tmp_path / f"rect_{i}" / "settings.json"
        st = json.loads(path.read_text())
        assert st["camera"]["pose_l"] == 15
        st["camera"]["pose_l"] = 13                              # 13 x 15 positions over the same extent
        st["camera"]["start_positions"] = [[min(p[0], 11)] + p[1:] for p in st["camera"]["start_positions"]]
        path.write_text(json.dumps(st))
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    ds = sc.SceneDataset(str(tmp_path))
    net = _net(nbp_weights)
    dev = torch.device("cuda")
    n = 8
    singles = [tp.build_rollout(params, net, ds, (k % 2, 0), dev, seed=3 + k) for k in range(4)]
    E = len(singles[0].planner.edges)
    assert E % 8 != 0 and singles[0].planner.result_bytes() % 8 == 0
    for r in singles:
        for _ in range(n):
            r.step()
    multi_r = [tp.build_rollout(params, net, ds, (k % 2, 0), dev, seed=3 + k) for k in range(4)]
    m = tp.MultiRollout(multi_r, net, dev)
    assert all(len(g) == 2 for g in m.groups) and all(res is not None for res in m._res)
    for _ in range(n):
        m.step()
    m.flush()
    assert sum(r.n_replans for r in multi_r) > 0
    for a, b in zip(singles, multi_r):
        assert a.camera.cam_idx_history == b.camera.cam_idx_history
        assert a.coverage_evolution(n) == b.coverage_evolution(n)


def test_dead_forward_elision_changes_nothing(hip, dataset, nbp_weights):
    """MultiRollout(elide_dead_forward=True) forwards only the maps of the rollouts that replan (the reference discards the
    network's output on the other steps, nbp_planning.py:252): trajectories, clouds and coverage are those of the default mode,
    which forwards every map at every step as the reference does (bench.py reports the elided rate beside the headline only)."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    ds = sc.SceneDataset(dataset)
    net = _net(nbp_weights)
    dev = torch.device("cuda")
    n = 14
    runs = {}
    for elide in (False, True):
        ros = [tp.build_rollout(params, net, ds, (i % 2, 0), dev, seed=60 + i) for i in range(6)]
        m = tp.MultiRollout(ros, net, dev, elide_dead_forward=elide)
        seen = []
        for _ in range(n):
            m.step()
            seen.append(sum(r.need_replan for r in ros))
        m.flush()
        runs[elide] = (ros, seen)
    assert 0 < sum(runs[True][1]) < 6 * n                       # some steps replanned, some did not: both branches were exercised
    for a, b in zip(runs[False][0], runs[True][0]):
        assert a.camera.cam_idx_history == b.camera.cam_idx_history and a.n_replans == b.n_replans
        assert np.array_equal(a.camera.X_cam_history, b.camera.X_cam_history)
        assert a.coverage_evolution(n) == b.coverage_evolution(n)
        na = int(a.st.cloud_count.item())
        assert na == int(b.st.cloud_count.item()) and torch.equal(a.st.cloud[:na], b.st.cloud[:na])


def test_group_streams_run_side_by_side_even_after_a_graph_capture(hip, nbp_weights):
    """The lock-step's groups overlap only if their streams sit on different hardware queues.  HIP assigns queues at first use;
    after a hipGraph capture in the process (NBP.forward_static) two fresh pool streams were measured on ONE queue (6 % of the
    48-rollout lock-step, profiles/r04/stream_queue_collision.txt).  _concurrent_streams keeps only streams that it has seen
    overlap: checked here after a capture, for two and for three groups."""
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility.synthetic import make_count_maps
    dev = torch.device("cuda")
    m = NBP()
    m.load_state_dict(nbp_weights, strict=True)
    m = m.cuda().eval()
    x = make_count_maps(1, 64, seed=1).cuda()
    with torch.no_grad():
        m.forward_static(x)                                   # a capture: the condition under which the collision was seen
    for n in (2, 3):
        streams, check = tp._concurrent_streams(dev, n)
        assert len(streams) == n and check["concurrent"] and check["streams_tested"] >= n
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        torch.cuda.synchronize()
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                if i == 0:
                    ev[0].record()
                torch.cuda._sleep(400_000)
                ev[i + 1].record()
        torch.cuda.synchronize()
        one = ev[0].elapsed_time(ev[1])
        assert max(ev[0].elapsed_time(e) for e in ev[1:]) < 1.6 * one, "the spin kernels ran one after the other"


def test_four_streams_match_single_rollouts(hip, dataset, nbp_weights):
    """Four groups = four HIP streams stepping concurrently (scratch buffers are per stream): every rollout still walks
    exactly the trajectory it walks alone."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    ds = sc.SceneDataset(dataset)
    net = _net(nbp_weights)
    dev = torch.device("cuda")
    n = 8
    singles = [tp.build_rollout(params, net, ds, (i % 2, 0), dev, seed=40 + i) for i in range(4)]
    for r in singles:
        for _ in range(n):
            r.step()
    multi_r = [tp.build_rollout(params, net, ds, (i % 2, 0), dev, seed=40 + i) for i in range(4)]
    m = tp.MultiRollout(multi_r, net, dev, n_groups=4)
    assert len(m.groups) == 4 and len({s.cuda_stream for s in m.streams}) == 4
    for _ in range(n):
        m.step()
    m.flush()
    torch.cuda.synchronize()
    for a, b in zip(singles, multi_r):
        assert a.camera.cam_idx_history == b.camera.cam_idx_history
        assert a.coverage_evolution(n) == b.coverage_evolution(n)
        assert int(a.st.cloud_count.item()) == int(b.st.cloud_count.item())
        k = int(a.st.cloud_count.item())
        assert torch.equal(a.st.cloud[:k], b.st.cloud[:k])


def test_group_larger_than_the_batched_kernels_hold(hip, dataset, nbp_weights):
    """A lock-step group of 18 rollouts (the strong-scaling stage on one GPU has groups of 20): the batched stages take 12 / 16
    rollouts per launch, larger groups go in chunks -- same trajectories, clouds and coverage as one launch per rollout."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    ds = sc.SceneDataset(dataset)
    net = _net(nbp_weights)
    dev = torch.device("cuda")
    n, R = 5, 18
    runs = []
    for batched in (True, False):
        ros = [tp.build_rollout(params, net, ds, (i % 2, 0), dev, seed=70 + i) for i in range(R)]
        m = tp.MultiRollout(ros, net, dev, n_groups=1)
        assert len(m.groups) == 1 and len(m.groups[0]) == R
        m.batched = batched
        for _ in range(n):
            m.step()
        m.flush()
        torch.cuda.synchronize()
        runs.append(ros)
    for a, b in zip(*runs):
        assert a.camera.cam_idx_history == b.camera.cam_idx_history
        assert a.coverage_evolution(n) == b.coverage_evolution(n)
        k = int(a.st.cloud_count.item())
        assert k == int(b.st.cloud_count.item()) and torch.equal(a.st.cloud[:k], b.st.cloud[:k])
        assert torch.equal(a.st.maps6, b.st.maps6)


def test_group_with_an_eager_colour_camera_matches_single_rollouts(hip, nbp_weights, tmp_path):
    """The per-rollout fallback inside the group stages (simulator/lockstep.py): a camera with contrast_factor != 1 renders its
    colours eagerly, so a group that holds one cannot take the batched rasteriser / un-projection calls and goes one call per
    rollout.  Two rollouts in ONE group, the first deferring its colours and the second eager, over step 0's replan, a move and the
    supervision frames: each walks the trajectory, sees the coverage and builds the cloud AND its colours of the same rollout
    stepped alone, bit for bit."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    for i in range(2):
        make_maze_scene(str(tmp_path / f"maze_{i}"), seed=30 + i, cells=8, size=4.8, height=1.2, tess=0.3)
    path = tmp_path / "maze_1" / "settings.json"
    st = json.loads(path.read_text())
    st["camera"]["contrast_factor"] = 1.4
    path.write_text(json.dumps(st))
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    ds = sc.SceneDataset(str(tmp_path))
    net = _net(nbp_weights)
    dev = torch.device("cuda")
    n = 3
    singles = [tp.build_rollout(params, net, ds, (i, 0), dev, seed=50 + i) for i in range(2)]
    for r in singles:
        for _ in range(n):
            r.step()
    multi_r = [tp.build_rollout(params, net, ds, (i, 0), dev, seed=50 + i) for i in range(2)]
    m = tp.MultiRollout(multi_r, net, dev, n_groups=1)
    assert len(m.groups) == 1 and len(m.groups[0]) == 2
    for _ in range(n):
        m.step()
    m.flush()
    torch.cuda.synchronize()
    for a, b in zip(singles, multi_r):
        assert a.camera.cam_idx_history == b.camera.cam_idx_history
        assert a.coverage_evolution(n) == b.coverage_evolution(n)
        k = int(a.st.cloud_count.item())
        assert k > 0 and k == int(b.st.cloud_count.item())
        assert torch.equal(a.st.cloud[:k], b.st.cloud[:k])
        assert torch.equal(a.st.cloud_rgb[:k], b.st.cloud_rgb[:k])
        assert float(b.st.cloud_rgb[:k].abs().sum()) > 0
    # the group really was mixed: the first camera defers its colours, the second renders them eagerly
    assert multi_r[0].camera._zface_ring is not None and multi_r[0].camera._rgb_ring is None
    assert multi_r[1].camera._rgb_ring is not None and multi_r[1].camera._zface_ring is None


def test_rollout_on_512_grid(hip, dataset, nbp_weights):
    """BASELINE configs[4] geometry: 512x512 grid, +-80 window (same 0.3125 units / pixel), value map 128x128."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    ds = sc.SceneDataset(dataset)
    net = _net(nbp_weights)
    ro = tp.build_rollout(params, net, ds, (0, 0), torch.device("cuda"), seed=2, grid=512)
    for _ in range(4):
        ro.step()
    assert ro.st.maps6.shape == (6, 512, 512) and ro.S == 512 and ro.V == 128 and ro.grid_range == (-80, 80)
    cov = ro.coverage_evolution(4)
    assert cov[0] == 0.0 and cov[-1] > 0.0
    # the 256-grid map is the centre crop of the 512-grid map's geometry: same points, same pitch
    assert float(ro.st.maps6[:5].sum()) > 0


def test_config5_bf16_multi_rollout_512(hip, dataset, nbp_weights):
    """BASELINE configs[4] in miniature: 8 concurrent rollouts on a 512 grid, forwards batched through the bf16
    network.  bf16 cannot promise the fp32 path's decisions, so the check is behavioural: every rollout explores
    (coverage grows, no NaN) and the first steps -- where the agent only follows its initial path -- coincide."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    ds = sc.SceneDataset(dataset)
    dev = torch.device("cuda")
    net16 = _net(nbp_weights)
    net16.conv_precision = "bf16"
    net32 = _net(nbp_weights)
    n = 6
    out = {}
    for tag, net in (("bf16", net16), ("fp32", net32)):
        ros = [tp.build_rollout(params, net, ds, (i % 2, 0), dev, seed=10 + i, grid=512) for i in range(8)]
        m = tp.MultiRollout(ros, net, dev)
        for _ in range(n):
            m.step()
        m.flush()
        out[tag] = ros
    for a, b in zip(out["bf16"], out["fp32"]):
        ca, cb = a.coverage_evolution(n), b.coverage_evolution(n)
        assert all(np.isfinite(ca)) and ca[-1] > 0.0 and max(ca) >= ca[1] - 1e-9, (ca, cb)
        assert a.camera.cam_idx_history[:2] == b.camera.cam_idx_history[:2], (a.camera.cam_idx_history, b.camera.cam_idx_history)
        assert abs(ca[1] - cb[1]) < 1e-6, (ca, cb)      # same first frames -> same first coverage value


def test_scene_parallel_entry_point_two_ranks(hip, dataset):
    """torchrun with 2 ranks (sharing this box's single GPU, gloo for the one all_gather): each rank runs its
    shard of the (scene, start) runs; rank 0 writes the merged coverage JSON == the single-process result."""
    cfg = {"numGPU": 0, "dataset_path": dataset, "test_scenes": [], "params_name":
           "macarons_default_training_config.json", "model_name": "x.pth", "results_json_name": "out_test_2rank.json",
           "test_resolution": 0.05, "use_perfect_depth_map": True, "compute_collision": False, "load_json": False,
           "random_seed": 8, "torch_seed": 9, "nbp_weights": "./weights/none.pth"}
    cfg_path = os.path.join(ROOT, "configs/test/_pytest_2rank.json")
    with open(cfg_path, "w") as fh:
        json.dump(cfg, fh)
    env = dict(os.environ, NBP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    try:
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", "29611",
                            os.path.join(ROOT, "test_nbp_planning.py"), "-c", "_pytest_2rank.json", "--n-poses", "4"],
                           capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        two = json.load(open(os.path.join(ROOT, "data", "out_test_2rank.json")))
        cfg["results_json_name"] = "out_test_1rank.json"
        with open(cfg_path, "w") as fh:
            json.dump(cfg, fh)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "test_nbp_planning.py"), "-c", "_pytest_2rank.json",
                            "--n-poses", "4"], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        one = json.load(open(os.path.join(ROOT, "data", "out_test_1rank.json")))
        assert sorted(two) == sorted(one) == ["maze_00", "maze_01"]
        for scene in one:
            assert np.allclose(two[scene]["0"]["coverage"], one[scene]["0"]["coverage"], atol=1e-7)
    finally:
        os.remove(cfg_path)


@pytest.mark.parametrize("cells,size", [(1, 1.2), (2, 1.5), (3, 1.8)])
def test_rollout_on_tiny_scenes(hip, nbp_weights, tmp_path, cells, size):
    """Degenerate scenes: a single room with a 3 x 3 / 4 x 4 / 5 x 5 pose lattice.  The agent quickly runs out of valid
    goals (every position visited / no candidate passes the density test) and must keep stepping without an exception
    (the reference would hit its unbound `next_idx`, nbp_planning.py:255-258)."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    make_maze_scene(str(tmp_path / "tiny"), seed=cells, cells=cells, size=size, height=1.2, tess=0.3)
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    ds = sc.SceneDataset(str(tmp_path))
    net = _net(nbp_weights)
    ro = tp.build_rollout(params, net, ds, (0, 0), torch.device("cuda"), seed=3)
    for _ in range(25):
        ro.step()
    torch.cuda.synchronize()
    cov = ro.coverage_evolution(25)
    assert all(np.isfinite(cov)) and cov[-1] > 0.2          # a single room is mostly seen within a few steps
    assert len(ro.camera.cam_idx_history) >= 25


def test_split_path_and_fp32_pipe_take_the_same_trajectory(hip, dataset, nbp_weights):
    """The default eval path (3x3 convolutions as three fp16 MFMAs per product on two-piece operands) and the fp32 MFMA pipe drive
    the same exploration: identical lattice path, coverage curve and cloud size over 40 steps (value maps differ at the 1e-6
    level, goal cells do not)."""
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.testers import nbp_planning as tp
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    ds = sc.SceneDataset(dataset)
    runs = tp.list_runs(ds, params)
    res = {}
    for prec in ("fp32_split", "fp32"):
        net = _net(nbp_weights)
        net.conv_precision = prec
        with torch.no_grad():
            res[prec] = tp.run_one(params, net, ds, runs[1], torch.device("cuda"), n_poses=40, seed=11)
    a, b = res["fp32_split"], res["fp32"]
    assert a["X_cam_history"] == b["X_cam_history"] and a["coverage"] == b["coverage"] and a["n_points"] == b["n_points"]
    assert a["coverage"][-1] > 0.02
