"""GPU: the four lock-step group entry points that only ran inside the collection test -- replan_batch, coverage_count_batch,
unproject_append_batch and raster_zface_batch -- on deliberately RAGGED groups.  A group form is n single calls in one launch: the
launch takes the largest item's grid, every item reads its OWN arguments and sizes through blockIdx.y / .z, leaves its surplus
workgroups, and the slots behind the last item copy item 0.  Every test runs the group once, the single-call form per item into
fresh outputs, and requires equal bits for every output of every item; the small items are compared with the float64 / numpy
oracle too, so that two equal wrong answers cannot pass.  Every device tensor of a call stays referenced until the test's last
read (the allocator reuses no block).

What a ragged group can and cannot show, kernel by kernel (from the kernels' code; each line was tried once as a mutation):
  * coverage_tally: the body strides by the item's own grid -- a 1-workgroup stride under 16 workgroups counts stamps many times.
  * raster_tile: gx_tile carries the item's own segment count -- a lost segment or block is seen (dense17000 needs its second).
  * the un-projection: frame f is read through ITS pointer -- frame 0's pointer for every frame is seen by every item of 4 frames.
  * score_edges: the cut [0, g_score) / [g_score, g_score + g_edges) is seen where it moves an edge workgroup (an edge body that
    starts at blockIdx.x instead of blockIdx.x - g_score leaves edges unwritten).  The bodies compute ONE candidate or edge per
    thread from bx and never use their gx argument, so which grid is passed as gx changes nothing, and a workgroup past the item's
    last one would only find i >= P / e >= E: neither the stride nor the upper end of the cut is observable, here or anywhere.
  * coverage_mark: gx_mark covers every sampled point in the first pass of the stride loop (or sits at the 2048 cap, which is then
    gridDim.x too), and a surplus workgroup starts past M: neither the stride nor the early exit is observable.  What is seen is a
    LOST workgroup (an exit at gx_mark / 2) and the item's own cloud, size, seed, plan and epoch."""
import ctypes as C

import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import hipops as ho
from oracle import camera as ocam
from oracle import csim
from oracle import planner as opl

pytestmark = pytest.mark.gpu
D = "cuda"
E_ARG, E_WS, E_SHAPE = -1, -2, -3


class _Owner:
    """Stands in for the rollout object that owns an item's scratch (hipops._item_ws)."""


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(D)


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).reshape(-1).view(np.uint8)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ replan
REPLAN_P = (1, 3, 4, 260, 700)          # g_score = 1, 1, 1, 65, 175 (one wave per candidate, four per workgroup)
REPLAN_E = (700, 1, 257, 256, 5)        # g_edges = 3, 1, 2, 1, 1: the item with the most score workgroups has the fewest edge ones
REPLAN_NOSKIP = (1, 3)
REPLAN_S, REPLAN_V = 64, 16


def _replan_spec(j, P, E, skip_none, S=REPLAN_S, V=REPLAN_V):
    """Host inputs of one replanning rollout.  The lattice has max(P, 48) nodes; the first P are the candidates and the edges join
    any two nodes, so that an item of one candidate still has blocked and free edges.  Node 0 sits on the pose (a valid candidate:
    its map cell is occupied), node 1 far outside the window (an invalid candidate, and a blocked edge 0 -> 1)."""
    rng = np.random.default_rng(100 + j)
    cx, cz = float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5))
    pose = np.array([cx, 3.3, cz, 0, 0], np.float32)
    maps6 = ((rng.random((6, S, S)) < 0.0008) * rng.integers(1, 4, (6, S, S))).astype(np.float32)
    maps6[0, S // 2, S // 2] = 1.0
    out2 = (rng.random((S, S)) * 0.14).astype(np.float32)                # ~7 % of the cells reach the 0.13 threshold
    traj = (rng.random((S, S)) < 0.02).astype(np.float32)
    out1 = rng.normal(0, 1, (8, V, V)).astype(np.float32)
    N = max(P, 48)
    nodes = np.stack([cx + rng.uniform(-48, 48, N), np.full(N, 3.3), cz + rng.uniform(-48, 48, N)], 1).astype(np.float32)
    nodes[0] = (pose[0], 3.3, pose[2])
    nodes[1] = (pose[0] + np.float32(60.0), 3.3, pose[2])
    edges = rng.integers(0, N, (E, 2)).astype(np.int32)
    edges[0] = (0, 1)
    if E > 1:
        edges[1] = (0, 0)
    skip = None
    if not skip_none:
        skip = (rng.random(P) < 0.1).astype(np.uint8)
        skip[0] = 0
    return dict(pose=pose, maps6=maps6, out2=out2, traj=traj, out1=out1, nodes=nodes, P=P, edges=edges, skip=skip)


def _replan_dev(s):
    d = {k: _dev(s[k]) for k in ("maps6", "out2", "traj", "out1", "nodes", "edges")}
    d["skip"] = None if s["skip"] is None else _dev(s["skip"])
    d["pos"] = d["nodes"][:s["P"]]                # the candidates: a prefix view of the lattice (same base pointer)
    return d


def _replan_outputs(s, S=REPLAN_S):
    P, E = s["P"], len(s["edges"])
    return dict(obst=torch.full((S, S), -5.0, device=D), fullproj=torch.full((S, S), -5.0, device=D),
                valid=torch.full((P,), 0xCC, dtype=torch.uint8, device=D), cell=torch.full((P, 2), -7, dtype=torch.int32, device=D),
                score=torch.full((P,), float("nan"), dtype=torch.float64, device=D),
                blocked=torch.full((E,), 0xCC, dtype=torch.uint8, device=D))


def _replan_item(s, d, o):
    return (d["out2"], d["maps6"], d["traj"], o["obst"], o["fullproj"], d["pos"], (float(s["pose"][0]), float(s["pose"][2])), d["out1"],
            d["skip"], o["valid"], o["cell"], o["score"], d["edges"], o["blocked"])


def _replan_single(s, d):
    obst, fullproj = ho.fuse_obstacle(d["out2"], d["maps6"], d["traj"])
    valid, cell, score = ho.score_candidates(d["pos"], s["pose"], d["out1"], fullproj, d["skip"])
    blocked = ho.edges_blocked(obst, s["pose"], d["nodes"], d["edges"])
    return dict(obst=obst, fullproj=fullproj, valid=valid, cell=cell, score=score, blocked=blocked)


REPLAN_OUT = ("obst", "fullproj", "valid", "cell", "score", "blocked")


def test_replan_batch_ragged_equals_single_calls_and_oracle(hip):
    S, V = REPLAN_S, REPLAN_V
    specs = [_replan_spec(j, P, E, j in REPLAN_NOSKIP) for j, (P, E) in enumerate(zip(REPLAN_P, REPLAN_E))]
    devs = [_replan_dev(s) for s in specs]
    outs = [_replan_outputs(s) for s in specs]
    ho.replan_batch([_replan_item(s, d, o) for s, d, o in zip(specs, devs, outs)], S, V)
    refs = [_replan_single(s, d) for s, d in zip(specs, devs)]
    for j, (s, o, r) in enumerate(zip(specs, outs, refs)):
        for k in REPLAN_OUT:
            assert _same(o[k], r[k]), f"item {j} (P = {s['P']}, E = {len(s['edges'])}): {k} differs from the single call"
    for j, (s, o) in enumerate(zip(specs, outs)):
        P, E = s["P"], len(s["edges"])
        obst_o, full_o = opl.fuse_obstacle(s["out2"], s["maps6"], s["traj"])
        assert np.array_equal(o["obst"].cpu().numpy(), obst_o) and np.array_equal(o["fullproj"].cpu().numpy(), full_o), j
        v_o, c_o, s_o = opl.score_candidates(s["nodes"][:P], s["pose"], s["out1"], full_o, s["skip"], V=V)
        assert np.array_equal(o["valid"].cpu().numpy().astype(bool), v_o), j
        assert np.array_equal(o["cell"].cpu().numpy()[v_o], c_o[v_o]) and np.array_equal(o["score"].cpu().numpy()[v_o], s_o[v_o]), j
        want = np.array([opl.edge_blocked(s["nodes"][a], s["nodes"][b], s["pose"], obst_o) for a, b in s["edges"]])
        assert np.array_equal(o["blocked"].cpu().numpy().astype(bool), want), j
        # the group is not degenerate: candidate 0 valid and 1 invalid, edge 0 blocked and 1 free by construction (all that an item
        # of P = 3 or 4, E = 5 is asked for); from 100 candidates or edges on, more than 10 of either kind among the random ones
        assert v_o[0] and (P < 2 or not v_o[1]) and (P < 100 or 10 < v_o.sum() < P - 10), (j, v_o.sum())
        assert want[0] and (E < 2 or not want[1]) and (E < 100 or 10 < want.sum() < E - 10), (j, want.sum())
    # 17 copies in rotated order: 16 + 1 chunking, the 17th is a chunk of n = 1
    order = [(k + 2) % 5 for k in range(17)]
    outs17 = [_replan_outputs(specs[j]) for j in order]
    ho.replan_batch([_replan_item(specs[j], devs[j], o) for j, o in zip(order, outs17)], S, V)
    for k, (j, o) in enumerate(zip(order, outs17)):
        for name in REPLAN_OUT:
            assert _same(o[name], refs[j][name]), f"copy {k} of item {j}: {name} differs from the single call"


def test_replan_batch_every_group_size(hip):
    """n = 1 .. 16 on tiny items: every blockIdx.y, and the padding slots (copies of item 0 with no workgroups) for every n."""
    S, V = REPLAN_S, REPLAN_V
    shapes = [(1, 300), (3, 1), (4, 257), (5, 5)]                  # g_score 1 1 1 2, g_edges 2 1 2 1
    specs = [_replan_spec(20 + j, P, E, j % 2 == 1) for j, (P, E) in enumerate(shapes)]
    devs = [_replan_dev(s) for s in specs]
    refs = [_replan_single(s, d) for s, d in zip(specs, devs)]
    keep = []
    for n in range(1, 17):
        order = [(n + k) % len(specs) for k in range(n)]
        outs = [_replan_outputs(specs[j]) for j in order]
        ho.replan_batch([_replan_item(specs[j], devs[j], o) for j, o in zip(order, outs)], S, V)
        keep.append(outs)
        for k, (j, o) in enumerate(zip(order, outs)):
            for name in REPLAN_OUT:
                assert _same(o[name], refs[j][name]), f"n = {n}, slot {k} (item {j}): {name} differs from the single call"


# ------------------------------------------------------------------ coverage
def _cov_plan_data(j, G, side):
    """GT points in a box of its own and the box; `side` sets the density that leaves the coverage partial."""
    rng = np.random.default_rng(200 + j)
    lo = np.array([-10.0 * j, 3.0 * j, 5.0 - 7.0 * j], np.float32)
    hi = lo + np.float32(side)
    gt = rng.uniform(lo, hi, (G, 3)).astype(np.float32)
    return gt, (lo.tolist(), hi.tolist())


def _cov_cloud(seed, box, n):
    """n points around the box, a part of them outside the plan's grid (the box grown by the threshold)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(box[0], np.float32), np.array(box[1], np.float32)
    pad = np.float32(2.5)
    return rng.uniform(lo - pad, hi + pad, (n, 3)).astype(np.float32)


def _cov_case(pc, seed, n_dev=None, n=None, preset=None):
    """One item's cloud: n_dev = a device-side size, n = a host-side size below the buffer's, preset = a count the tally adds to."""
    return dict(pc=pc, seed=seed, n_dev=n_dev, n=n, preset=preset)


def _cov_run_group(plans, cases):
    """-> the out tensors of the items after ONE group call."""
    outs, items = [], []
    for plan, c in zip(plans, cases):
        out = torch.tensor([123456 if c["preset"] is None else c["preset"], -9], dtype=torch.int32, device=D)
        outs.append(out)
        items.append((plan, c["pc"], out, c["n_dev"], c["n"], c["seed"], c["preset"] is not None))
    ho.coverage_count_batch(items)
    return outs


def _cov_run_single(plans, cases):
    outs = []
    for plan, c in zip(plans, cases):
        out = torch.tensor([654321 if c["preset"] is None else c["preset"], -9], dtype=torch.int32, device=D)
        plan.count(c["pc"], out, n_dev=c["n_dev"], n=c["n"], seed=c["seed"], out_is_zero=c["preset"] is not None)
        outs.append(out)
    return outs


COV_G = (200, 3000, 16383, 16384)          # the last two straddle the tally's switch from 1 workgroup to 16
COV_SIDE = (9.0, 24.0, 44.0, 52.0)


def test_coverage_count_batch_ragged_equals_single_calls_and_oracle(hip):
    data = [_cov_plan_data(j, G, side) for j, (G, side) in enumerate(zip(COV_G, COV_SIDE))]
    gts = [_dev(gt) for gt, _ in data]
    plans = [ho.CoveragePlan(g, 1.0, 2, bbox=box) for g, (_, box) in zip(gts, data)]
    twins = [ho.CoveragePlan(g, 1.0, 2, bbox=box) for g, (_, box) in zip(gts, data)]      # the single-call side's own plans
    boxes = [box for _, box in data]
    half = torch.tensor([2500], dtype=torch.int64, device=D)
    half2 = torch.tensor([16000], dtype=torch.int64, device=D)
    none = torch.zeros(8, 3, device=D)                                     # "no points": a buffer of which n = 0 are in use
    # first assignment: G = 200 a cloud below 2 G (3 mark workgroups), G = 3000 a device-side size of half the buffer and a count
    # that is ADDED to a preset one, G = 16383 no points, G = 16384 a cloud above 2 G (sub-sampled to 32768: 512 mark workgroups)
    host_a = [_cov_cloud(301, boxes[0], 150), _cov_cloud(302, boxes[1], 5000), None, _cov_cloud(304, boxes[3], 40000)]
    # second assignment: the sub-sampled cloud on G = 16383 (its tally is the 1-workgroup form over 64 strides), a device-side
    # size on G = 16384, no points on G = 200, a sub-sampled cloud on G = 3000
    host_b = [None, _cov_cloud(312, boxes[1], 9000), _cov_cloud(313, boxes[2], 40000), _cov_cloud(314, boxes[3], 32000)]
    dev_a = [none if h is None else _dev(h) for h in host_a]
    dev_b = [none if h is None else _dev(h) for h in host_b]
    cases_a = [_cov_case(dev_a[0], 21), _cov_case(dev_a[1], 22, n_dev=half, preset=1000), _cov_case(dev_a[2], 23, n=0), _cov_case(dev_a[3], 24)]
    cases_b = [_cov_case(dev_b[0], 31, n=0), _cov_case(dev_b[1], 32), _cov_case(dev_b[2], 33, preset=77), _cov_case(dev_b[3], 34, n_dev=half2)]
    eff_a = [host_a[0], host_a[1][:2500], None, host_a[3]]                 # what the oracle sees (it sub-samples above 2 G itself)
    eff_b = [None, host_b[1], host_b[2], host_b[3][:16000]]
    keep = []
    for cases, eff, m_want in ((cases_a, eff_a, [150, 2500, 0, 32768]), (cases_b, eff_b, [0, 6000, 32766, 16000])):
        first = _cov_run_group(plans, cases)
        second = _cov_run_group(plans, cases)                              # bumped epochs, the same counts
        single = _cov_run_single(twins, cases)
        keep += [first, second, single]
        for j, (a, b, c) in enumerate(zip(first, second, single)):
            got, preset = a.cpu().tolist(), cases[j]["preset"] or 0
            assert got == c.cpu().tolist(), f"G = {COV_G[j]}: group {got} != single call {c.cpu().tolist()}"
            assert got == b.cpu().tolist(), f"G = {COV_G[j]}: second group call {b.cpu().tolist()} != first {got}"
            assert got[1] == m_want[j], (j, got)
            if eff[j] is None:
                assert got[0] == preset, (j, got)
            else:
                assert 0 < got[0] - preset < COV_G[j], (j, got)
            if COV_G[j] <= 3000 and eff[j] is not None:                    # the larger items are pinned by the single form
                assert got[0] - preset == opl.coverage(data[j][0], eff[j], seed=cases[j]["seed"])[1], (j, got)


def test_coverage_count_batch_every_group_size(hip):
    """n = 1 .. 16 on tiny plans (each item its own plan: a plan's stamps belong to one item of a launch)."""
    Gs = (50, 200, 120, 77)
    data = [_cov_plan_data(j, Gs[j % 4] + j, 6.0 + j % 3) for j in range(16)]
    gts = [_dev(gt) for gt, _ in data]
    plans = [ho.CoveragePlan(g, 1.0, 2, bbox=box) for g, (_, box) in zip(gts, data)]
    twins = [ho.CoveragePlan(g, 1.0, 2, bbox=box) for g, (_, box) in zip(gts, data)]
    nd = torch.tensor([40], dtype=torch.int64, device=D)
    none = torch.zeros(8, 3, device=D)
    cases, want = [], []
    for j, (gt, box) in enumerate(data):
        kind = j % 4
        host = None if kind == 0 else _cov_cloud(400 + j, box, (0, 30, 500, 90)[kind])     # none, below 2 G, above 2 G, device-side size
        cases.append(_cov_case(none if host is None else _dev(host), 50 + j, n_dev=nd if kind == 3 else None, n=0 if host is None else None,
                               preset=9 if j % 5 == 2 else None))
        eff = None if host is None else (host[:40] if kind == 3 else host)
        want.append((cases[j]["preset"] or 0) + (0 if eff is None else opl.coverage(gt, eff, seed=50 + j)[1]))
    single = [o.cpu().tolist() for o in _cov_run_single(twins, cases)]
    assert [s[0] for s in single] == want and sum(1 for j, s in enumerate(single) if s[0] > (cases[j]["preset"] or 0)) >= 10
    keep = []
    for n in range(1, 17):
        order = [(n + k) % 16 for k in range(n)]
        outs = _cov_run_group([plans[j] for j in order], [cases[j] for j in order])
        keep.append(outs)
        for k, (j, o) in enumerate(zip(order, outs)):
            assert o.cpu().tolist() == single[j], f"n = {n}, slot {k} (plan {j}): {o.cpu().tolist()} != single call {single[j]}"


# ------------------------------------------------------------------ meshes and cameras of the simulator tests
def _box_mesh(h=4.0):
    """The closed room of test_raster_closed_form_box_full_res: 12 faces."""
    v = np.array([[x, y, zz] for x in (-h, h) for y in (-h, h) for zz in (-h, h)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def _soup_mesh(seed, n):
    """The triangle soup of test_raster_random_triangle_soup_vs_oracle: clip-plane crossers, degenerate and flat faces."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-6, 6, (n, 1, 3))
    size = rng.choice([0.05, 0.5, 3.0, 30.0], (n, 1, 1), p=[0.2, 0.4, 0.3, 0.1])
    tri = (c + rng.normal(0, 1, (n, 3, 3)) * size).astype(np.float32)
    tri[:5, 2] = tri[:5, 1]
    tri[5:10, :, 1] = tri[5:10, :1, 1]
    return tri.reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def _cams(poses):
    RT = [ocam.camera_RT(x, v) for x, v in poses]
    return RT, ho.cams12(np.stack([r for r, _ in RT]), np.stack([t for _, t in RT]), D)


def _dense_mesh(n, R, T, H, W):
    """n small triangles that ALL project into the first 64 image columns of the camera (R, T): one coarse tile of 64 x 64 pixels
    whose face list is longer than a 16384-entry segment."""
    rng = np.random.default_rng(77)
    s = min(H, W)
    t = float(ocam.TAN_HALF_FOV)
    z = rng.uniform(3.0, 10.0, n)
    ndc_x = rng.uniform((W - 2 * 56 - 1) / s, (W - 2 * 4 - 1) / s, n)            # centres in columns 4 .. 56
    ndc_y = rng.uniform(-0.8 * H / s, 0.8 * H / s, n)
    centre = np.stack([ndc_x * z * t, ndc_y * z * t, z], 1)
    view = centre[:, None, :] + rng.normal(0, 0.06, (n, 3, 3))
    world = (view.reshape(-1, 3) - np.asarray(T, np.float64)) @ np.asarray(R, np.float64).T       # X_view = X_world R + T
    return world.astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def _colors(seed, n_verts):
    return np.random.default_rng(seed).uniform(0.05, 1.0, (n_verts, 3)).astype(np.float32)


# ------------------------------------------------------------------ un-projection
UNPROJ_POSES = [([1.0, 3.3, -2.0], [0.0, 45.0]), ([4.0, 3.3, -2.0], [30.0, 90.0]), ([4.0, 3.3, 1.0], [-30.0, 200.0]),
                ([7.0, 3.3, 1.0], [0.0, 315.0])]
BOX_POSES = [([0.0, 0.0, 0.0], [0.0, 0.0]), ([1.5, -1.0, 2.0], [25.0, 140.0]), ([-2.0, 2.0, -1.0], [-40.0, 250.0]),
             ([2.5, 0.5, 2.0], [10.0, 30.0])]
SOUP_POSES = [([0.5, -1.0, 2.0], [10.0, 20.0]), ([-2.0, 1.0, 0.0], [-35.0, 130.0]), ([2.5, 2.0, -1.5], [50.0, 220.0]),
              ([0.0, 0.0, 0.0], [-10.0, 300.0])]
RING_ORDER = (3, 0, 1, 2)               # a camera's ring of 5 frames that wraps: the four frames of a call are not adjacent


def _random_depth(seed, F_, H, W):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.6, 120, (F_, H, W)).astype(np.float32)            # a part beyond the 70-unit sensor range
    d[rng.random((F_, H, W)) < 0.25] = -1
    return d


def _into_ring(frames, fill):
    """frames [F,H,W] -> (ring [5,H,W] that holds frame f in slot RING_ORDER[f], the F views in call order)."""
    ring = torch.full((5,) + tuple(frames.shape[1:]), fill, dtype=frames.dtype, device=D)
    for f in range(frames.shape[0]):
        ring[RING_ORDER[f]].copy_(frames[f])
    return ring, [ring[RING_ORDER[f]] for f in range(frames.shape[0])]


def _render(mesh, poses, F_, H, W, color_seed):
    """A coloured item's inputs: depth and (depth, face) images of the single-call renderer, the mesh and its vertex colours."""
    v, f = mesh
    RT, cams = _cams(poses[:F_])
    vd, fd, cd = _dev(v), _dev(f), _dev(_colors(color_seed, len(v)))
    z, zf = ho.raster_zface(vd, fd, cams, H, W)
    return RT, cams, z, zf, (vd, fd, cd)


def _unproj_specs(H, W, F_):
    """Five items: 0 depth only, frames in a wrapped ring; 1 coloured (the box); 2 depth only, its last frame sees nothing; 3 coloured
    (a soup) with a capacity that clamps; 4 coloured (the box, other colours), depth AND face images in wrapped rings."""
    specs = []
    RT0, cams0 = _cams(UNPROJ_POSES[:F_])
    d0 = _random_depth(5, F_, H, W)
    ring0, frames0 = _into_ring(_dev(d0), -1.0)
    specs.append(dict(host=d0, RT=RT0, cams=cams0, ring=ring0, frames=frames0, seed=11, start=17, cap=4000, shade=None))
    RT1, cams1, z1, zf1, m1 = _render(_box_mesh(), BOX_POSES, F_, H, W, 1)
    specs.append(dict(RT=RT1, cams=cams1, frames=[z1[f] for f in range(F_)], z=z1, seed=12, start=3, cap=4000,
                      shade=([zf1[f] for f in range(F_)], zf1) + m1))
    RT2, cams2 = _cams(UNPROJ_POSES[::-1][:F_])
    d2 = _random_depth(6, F_, H, W)
    d2[F_ - 1] = -1
    z2 = _dev(d2)
    specs.append(dict(host=d2, RT=RT2, cams=cams2, frames=[z2[f] for f in range(F_)], z=z2, seed=13, start=250, cap=4000, shade=None))
    RT3, cams3, z3, zf3, m3 = _render(_soup_mesh(2, 300), SOUP_POSES, F_, H, W, 3)
    specs.append(dict(RT=RT3, cams=cams3, frames=[z3[f] for f in range(F_)], z=z3, seed=14, start=40, cap=40 + 9 * F_,
                      shade=([zf3[f] for f in range(F_)], zf3) + m3))
    RT4, cams4, z4, zf4, m4 = _render(_box_mesh(3.0), BOX_POSES[::-1], F_, H, W, 4)
    ring4, frames4 = _into_ring(z4, -1.0)
    zring4, zframes4 = _into_ring(zf4, -1)
    specs.append(dict(RT=RT4, cams=cams4, ring=(ring4, zring4), frames=frames4, seed=15, start=1, cap=4000, shade=(zframes4, zf4) + m4))
    for s in specs:
        s["stacked"] = torch.stack(s["frames"]).contiguous()             # the single call's [F,H,W]
    return specs


def _unproj_state(s):
    cloud = torch.zeros(s["cap"], 3, device=D)
    cloud[:s["start"]] = 7.0
    rgb = None
    if s["shade"] is not None:
        rgb = torch.zeros(s["cap"], 3, device=D)
        rgb[:s["start"]] = 0.25
    return dict(owner=_Owner(), cloud=cloud, rgb=rgb, count=torch.tensor([s["start"]], dtype=torch.int64, device=D))


def _unproj_item(s, st, ambient=0.85):
    shade = None if s["shade"] is None else (s["shade"][0], s["shade"][2], s["shade"][3], s["shade"][4], ambient)
    return (st["owner"], s["frames"], s["cams"], st["cloud"], st["count"], s["seed"], st["rgb"], shade)


def _unproj_single(s):
    st = _unproj_state(s)
    shade = None if s["shade"] is None else (s["shade"][1].contiguous(), s["shade"][2], s["shade"][3], s["shade"][4], 0.85)
    ho.unproject_append(s["stacked"], None, s["cams"], st["cloud"], st["count"], 0.05, 70.0, seed=s["seed"], cloud_rgb=st["rgb"], shade=shade)
    return st


def _unproj_same(st, ref, what):
    n, n_ref = int(st["count"].item()), int(ref["count"].item())
    assert n == n_ref, f"{what}: cloud_count {n} != single call {n_ref}"
    assert _same(st["cloud"], ref["cloud"]), f"{what}: cloud differs from the single call"         # the appended points, the prefix
    if ref["rgb"] is not None:                                                                     # and the untouched tail
        assert _same(st["rgb"], ref["rgb"]), f"{what}: cloud_rgb differs from the single call"
    return n


@pytest.mark.parametrize("F_", [1, 4])
@pytest.mark.parametrize("H,W", [(32, 56), (48, 172)])
def test_unproject_append_batch_ragged_equals_single_calls_and_oracle(hip, H, W, F_):
    """H W = 1792 is below one 2048-pixel chunk; 8256 is 5 compact chunks and 3 fast ones, neither a whole multiple."""
    specs = _unproj_specs(H, W, F_)
    states = [_unproj_state(s) for s in specs]
    ho.unproject_append_batch([_unproj_item(s, st) for s, st in zip(specs, states)], H, W, F_)
    refs = [_unproj_single(s) for s in specs]
    for j, (s, st, ref) in enumerate(zip(specs, states, refs)):
        n = _unproj_same(st, ref, f"item {j}")
        assert float((st["cloud"][:s["start"]] - 7.0).abs().sum()) == 0.0, j
        if s["shade"] is None:                                       # the oracle: frame f is sampled with the seed of frame index f
            want = [ocam.partial_point_cloud(s["host"][f], None, s["RT"][f][0], s["RT"][f][1], 0.05, 70.0, seed=s["seed"], frame_index=f)[0]
                    for f in range(F_)]
            want = np.concatenate(want, 0)
            assert n == s["start"] + len(want) and (len(want) > 20 or F_ == 1 and j == 2), (j, n)
            assert np.array_equal(st["cloud"][s["start"]:n].cpu().numpy(), want), j
        else:
            assert n > s["start"] + 8 and float((st["rgb"][:s["start"]] - 0.25).abs().sum()) == 0.0, (j, n)
            c = st["rgb"][s["start"]:n].cpu().numpy()
            assert (c > 0).all() and (c <= 1).all() and len(np.unique(c, axis=0)) > 4, j        # shaded, not one constant colour
    assert int(states[3]["count"].item()) == specs[3]["cap"]         # the capacity clamped
    assert int(states[2]["count"].item()) == int(refs[2]["count"].item()) > (250 if F_ > 1 else 249)


def test_unproject_append_batch_13_items_go_in_two_chunks(hip):
    H, W, F_ = 32, 56, 4
    specs = _unproj_specs(H, W, F_)
    refs = [_unproj_single(s) for s in specs]
    order = [(k + 3) % 5 for k in range(13)]
    states = [_unproj_state(specs[j]) for j in order]
    ho.unproject_append_batch([_unproj_item(specs[j], st) for j, st in zip(order, states)], H, W, F_)
    for k, (j, st) in enumerate(zip(order, states)):
        _unproj_same(st, refs[j], f"copy {k} of item {j}")


def test_unproject_append_batch_every_group_size(hip):
    H, W, F_ = 32, 56, 4
    specs = _unproj_specs(H, W, F_)
    refs = [_unproj_single(s) for s in specs]
    keep = []
    for n in range(1, 13):
        order = [(n + k) % 5 for k in range(n)]
        states = [_unproj_state(specs[j]) for j in order]
        ho.unproject_append_batch([_unproj_item(specs[j], st) for j, st in zip(order, states)], H, W, F_)
        keep.append(states)
        for k, (j, st) in enumerate(zip(order, states)):
            _unproj_same(st, refs[j], f"n = {n}, slot {k} (item {j})")


def test_unproject_append_batch_refuses_mixed_ambient(hip):
    """One ambient reaches the kernel: coloured items that carry different values must be refused, not shaded with the last one."""
    H, W, F_ = 32, 56, 1
    specs = _unproj_specs(H, W, F_)
    states = [_unproj_state(s) for s in specs]
    items = [_unproj_item(s, st, ambient=0.85 if j != 3 else 0.5) for j, (s, st) in enumerate(zip(specs, states))]
    with pytest.raises(ValueError):
        ho.unproject_append_batch(items, H, W, F_)
    # 13 items whose odd one is the 13th, a chunk of its own: the whole list is checked before the first chunk is launched
    order = [1, 3, 4] * 4 + [3]
    states13 = [_unproj_state(specs[j]) for j in order]
    items13 = [_unproj_item(specs[j], st, ambient=0.85 if k < 12 else 0.5) for k, (j, st) in enumerate(zip(order, states13))]
    with pytest.raises(ValueError):
        ho.unproject_append_batch(items13, H, W, F_)
    torch.cuda.synchronize()
    for s, st in list(zip(specs, states)) + [(specs[j], st) for j, st in zip(order, states13)]:     # refused before any launch
        assert int(st["count"].item()) == s["start"] and float(st["cloud"][s["start"]:].abs().sum()) == 0.0
    # one shared value other than the default is passed on: the single call with the same value gives the same colours
    ho.unproject_append_batch([_unproj_item(s, st, ambient=0.5) for s, st in zip(specs, states)], H, W, F_)
    s, ref = specs[1], _unproj_state(specs[1])
    ho.unproject_append(s["stacked"], None, s["cams"], ref["cloud"], ref["count"], 0.05, 70.0, seed=s["seed"], cloud_rgb=ref["rgb"],
                        shade=(s["shade"][1], s["shade"][2], s["shade"][3], s["shade"][4], 0.5))
    _unproj_same(states[1], ref, "ambient 0.5")
    assert not _same(states[1]["rgb"], _unproj_single(s)["rgb"])


# ------------------------------------------------------------------ rasteriser
RASTER_H, RASTER_W = 48, 80
BIG_POSES = [([0.0, 1.0, 0.0], [0.0, 0.0]), ([2.0, 1.0, 6.0], [5.0, 200.0]), ([-3.0, 2.0, 5.0], [-20.0, 120.0]), ([0.5, 0.0, 2.0], [15.0, 10.0])]
NOTHING = ([500.0, 3.0, 500.0], [0.0, 45.0])          # far outside every mesh, looking away from them


def _raster_specs(H, W):
    """Four items, the largest neither first nor last: a 300-face soup (its frame 1 sees nothing), 17000 small faces that fill one
    coarse tile's list past a 16384-entry segment in frame 0, the 12-face box, a 257-face soup (a second setup workgroup of one
    lane).  pick = the frame an n_frames = 1 call renders."""
    soup_poses = [SOUP_POSES[0], NOTHING, SOUP_POSES[2], SOUP_POSES[3]]
    R0, T0 = ocam.camera_RT(*BIG_POSES[0])
    specs = [dict(name="soup300", mesh=_soup_mesh(2, 300), poses=soup_poses, pick=1, oracle=True),
             dict(name="dense17000", mesh=_dense_mesh(17000, R0, T0, H, W), poses=BIG_POSES, pick=0, oracle=False),
             dict(name="box12", mesh=_box_mesh(), poses=BOX_POSES, pick=0, oracle=True),
             dict(name="soup257", mesh=_soup_mesh(3, 257), poses=SOUP_POSES[::-1], pick=0, oracle=True)]
    for s in specs:
        s["verts"], s["faces"] = _dev(s["mesh"][0]), _dev(s["mesh"][1])
    return specs


def _raster_cams(s, F_):
    poses = s["poses"] if F_ == 4 else s["poses"][s["pick"]:s["pick"] + 1]
    return _cams(poses)


def _raster_out(F_, H, W):
    return dict(owner=_Owner(), z=torch.full((F_, H, W), -77.0, device=D), zf=torch.full((F_, H, W), 5, dtype=torch.int64, device=D))


def _raster_check_image(s, o, what):
    z, zf = o["z"].cpu().numpy(), o["zf"].cpu().numpy()
    hit = zf != -1
    assert np.array_equal(z[~hit], np.full((~hit).sum(), -1.0, np.float32)), what
    assert np.array_equal(z[hit].view(np.uint32), (zf[hit] >> 32).astype(np.uint32)), what
    face = zf[hit] & 0xFFFFFFFF
    assert (face < len(s["mesh"][1])).all(), what
    return z, hit


@pytest.mark.parametrize("F_", [4, 1])
def test_raster_zface_batch_ragged_equals_single_calls_and_oracle(hip, F_):
    H, W = RASTER_H, RASTER_W
    specs = _raster_specs(H, W)
    cams = [_raster_cams(s, F_) for s in specs]
    outs = [_raster_out(F_, H, W) for _ in specs]
    ho.raster_zface_batch([(o["owner"], s["verts"], s["faces"], c[1], o["z"], o["zf"]) for s, c, o in zip(specs, cams, outs)], H, W, F_)
    refs = [ho.raster_zface(s["verts"], s["faces"], c[1], H, W) for s, c in zip(specs, cams)]
    for s, o, (z_ref, zf_ref) in zip(specs, outs, refs):
        assert _same(o["zf"], zf_ref), f"{s['name']}: the (depth, face) image differs from the single call"
        assert _same(o["z"], z_ref), f"{s['name']}: the depth image differs from the single call"
    for s, (RT, _), o in zip(specs, cams, outs):
        z, hit = _raster_check_image(s, o, s["name"])
        if s["name"] == "dense17000":                # the first 64 columns hold every face in frame 0, the last 16 none
            assert hit[0, :, :64].mean() > 0.4 and not hit[0, :, 64:].any(), hit[0].mean()
            # ... and the image NEEDS the list's second segment.  That segment holds 17000 - 16384 = 616 entries; which faces they
            # are is up to the order of the setup's atomics (67 workgroups run at once), late ones first of all.  With w distinct
            # winning faces a random 616 of the 17000 hold none with probability (1 - w / 17000)^616: below 1e-6 from w = 400
            face = o["zf"][0].cpu().numpy()[hit[0]] & 0xFFFFFFFF
            print(f"dense17000: {hit[0].sum()} hit pixels, {len(np.unique(face))} distinct winners, {(face >= 16384).sum()} pixels of faces >= 16384")
            assert len(np.unique(face)) >= 400 and (face >= 16384).any(), (len(np.unique(face)), (face >= 16384).sum())
        if not s["oracle"]:
            continue
        for i, (R, T) in enumerate(RT):
            want = csim.raster_zbuf(s["mesh"][0], s["mesh"][1], R, T, H, W, ocam.TAN_HALF_FOV)
            if s["poses"][i if F_ == 4 else s["pick"]] is NOTHING:
                assert not hit[i].any() and (want == -1).all(), s["name"]
            elif s["name"] == "box12":
                assert np.array_equal(z[i], want) and (z[i] > 0).all(), (s["name"], i)
            else:                                    # the soups: test_raster_random_triangle_soup_vs_oracle's criterion
                same = np.isclose(z[i], want, rtol=1e-5, atol=1e-5)
                assert same.mean() > 0.995, (s["name"], i, same.mean())
                assert ((z[i] > 0) == (want > 0)).mean() > 0.995, (s["name"], i)
                assert 0.02 < (z[i] > 0).mean(), (s["name"], i)


def test_raster_zface_batch_feeds_unproject_append_batch(hip):
    """The step loop's pairing: the group render's depth and (depth, face) images go straight into the group un-projection with
    colours; the single-call chain raster_zface -> unproject_append(shade=) gives the same clouds."""
    H, W, F_ = RASTER_H, RASTER_W, 4
    specs = [s for s in _raster_specs(H, W) if s["name"] in ("soup300", "box12")]
    cams = [_raster_cams(s, F_) for s in specs]
    outs = [_raster_out(F_, H, W) for _ in specs]
    ho.raster_zface_batch([(o["owner"], s["verts"], s["faces"], c[1], o["z"], o["zf"]) for s, c, o in zip(specs, cams, outs)], H, W, F_)
    cols = [_dev(_colors(8 + j, len(s["mesh"][0]))) for j, s in enumerate(specs)]
    us = []
    for j, (s, c, o) in enumerate(zip(specs, cams, outs)):
        us.append(dict(cams=c[1], frames=[o["z"][f] for f in range(F_)], seed=70 + j, start=5 + j, cap=3000,
                       shade=([o["zf"][f] for f in range(F_)], o["zf"], s["verts"], s["faces"], cols[j])))
    states = [_unproj_state(u) for u in us]
    ho.unproject_append_batch([_unproj_item(u, st) for u, st in zip(us, states)], H, W, F_)
    for j, (s, c, u, st) in enumerate(zip(specs, cams, us, states)):
        z, zf = ho.raster_zface(s["verts"], s["faces"], c[1], H, W)
        ref = _unproj_state(u)
        ho.unproject_append(z, None, c[1], ref["cloud"], ref["count"], 0.05, 70.0, seed=u["seed"], cloud_rgb=ref["rgb"],
                            shade=(zf, s["verts"], s["faces"], cols[j], 0.85))
        n = _unproj_same(st, ref, s["name"])
        assert n > u["start"] + 50, (s["name"], n)


def test_raster_zface_batch_every_group_size(hip):
    H, W, F_ = 16, 24, 4
    meshes = [("box12", _box_mesh(), BOX_POSES), ("soup257", _soup_mesh(3, 257), SOUP_POSES), ("soup30", _soup_mesh(4, 30), SOUP_POSES[::-1]),
              ("soup300", _soup_mesh(2, 300), [SOUP_POSES[0], NOTHING, SOUP_POSES[2], SOUP_POSES[3]])]
    specs = [dict(name=n, verts=_dev(m[0]), faces=_dev(m[1]), cams=_cams(p)[1]) for n, m, p in meshes]
    refs = [ho.raster_zface(s["verts"], s["faces"], s["cams"], H, W) for s in specs]
    assert all(int((zf != -1).sum()) > 30 for _, zf in refs)
    keep = []
    for n in range(1, 13):
        order = [(n + k) % len(specs) for k in range(n)]
        outs = [_raster_out(F_, H, W) for _ in order]
        ho.raster_zface_batch([(o["owner"], specs[j]["verts"], specs[j]["faces"], specs[j]["cams"], o["z"], o["zf"])
                               for j, o in zip(order, outs)], H, W, F_)
        keep.append(outs)
        for k, (j, o) in enumerate(zip(order, outs)):
            assert _same(o["zf"], refs[j][1]) and _same(o["z"], refs[j][0]), f"n = {n}, slot {k} ({specs[j]['name']}) differs from the single call"


# ------------------------------------------------------------------ refusals (return codes only: nothing is launched)
VP, I, LL, U, SZ = C.c_void_p, C.c_int, C.c_longlong, C.c_uint, C.c_size_t


def _arr(ctype, values):
    return (ctype * len(values))(*values)


def test_group_forms_refuse_bad_arguments(hip):
    # ---- replan: cap 16
    S, V, m = REPLAN_S, REPLAN_V, 17
    s = _replan_spec(0, 4, 5, False)
    d, o = _replan_dev(s), _replan_outputs(s)

    def replan(n, null=None):
        t = dict(out2=d["out2"], maps6=d["maps6"], traj=d["traj"], obst=o["obst"], fullproj=o["fullproj"], pos=d["pos"], out1=d["out1"],
                 skip=d["skip"], valid=o["valid"], cell=o["cell"], score=o["score"], edges=d["edges"], blocked=o["blocked"])
        a = {k: _arr(VP, [v.data_ptr()] * m) for k, v in t.items()}
        if null:
            a[null][1] = None
        xz = np.zeros((m, 2), np.float32)
        return hip.nbp_replan_batch_f32(n, a["out2"], a["maps6"], a["traj"], 0.13, S, a["obst"], a["fullproj"], a["pos"], _arr(I, [4] * m),
                                        xz.ctypes.data, a["out1"], V, -40.0, 40.0, a["skip"], a["valid"], a["cell"], a["score"], a["edges"],
                                        _arr(I, [5] * m), a["blocked"], None)
    assert replan(0) == E_ARG and replan(17) == E_ARG
    assert replan(2, "maps6") == E_ARG and replan(2, "blocked") == E_ARG

    # ---- coverage: cap 16
    gt, box = _cov_plan_data(0, 50, 6.0)
    plan = ho.CoveragePlan(_dev(gt), 1.0, 2, bbox=box)
    pc, out = _dev(_cov_cloud(1, box, 30)), torch.zeros(2, dtype=torch.int32, device=D)
    lo, hi = np.tile(np.array(box[0], np.float32), (m, 1)), np.tile(np.array(box[1], np.float32), (m, 1))

    def coverage(n, null=None, epoch=1):
        a = dict(plans=_arr(VP, [plan.plan.data_ptr()] * m), pc=_arr(VP, [pc.data_ptr()] * m), cnt=_arr(VP, [out.data_ptr()] * m),
                 mout=_arr(VP, [out[1:].data_ptr()] * m))
        if null:
            a[null][1] = None
        return hip.nbp_coverage_count_planned_batch_f32(n, a["plans"], _arr(I, [50] * m), 1.0, lo.ctypes.data, hi.ctypes.data, a["pc"],
                                                        _arr(LL, [30] * m), _arr(VP, [None] * m), _arr(LL, [100] * m), _arr(U, [0] * m),
                                                        _arr(U, [1, epoch] + [1] * (m - 2)), a["cnt"], a["mout"], None)
    assert coverage(0) == E_ARG and coverage(17) == E_ARG
    assert coverage(2, "plans") == E_ARG and coverage(2, "pc") == E_ARG
    assert coverage(2, epoch=0) == E_ARG

    # ---- un-projection: cap 12
    m = 13
    cams = np.zeros((m, 1, 12), np.float32)

    def unproject(n, H=32, W=56, null=None, shift=0, short=0):
        depth = torch.full((H * W + 8,), -1.0, device=D)
        cloud, count = torch.zeros(64, 3, device=D), torch.zeros(1, dtype=torch.int64, device=D)
        need = int(hip.nbp_unproject_workspace_bytes(1, H, W))
        ws = torch.empty(need + 512, dtype=torch.uint8, device=D)
        a = dict(depth=_arr(VP, [depth.data_ptr()] * m), cnts=_arr(VP, [ws.data_ptr() + need + 256] * m), cloud=_arr(VP, [cloud.data_ptr()] * m),
                 count=_arr(VP, [count.data_ptr()] * m), ws=_arr(VP, [ws.data_ptr()] * m))
        a["depth"][1] = depth.data_ptr() + shift
        if null:
            a[null][1] = None
        nul = _arr(VP, [None] * m)
        rc = hip.nbp_unproject_append_shaded_batch_f32(n, a["depth"], nul, nul, nul, nul, cams.ctypes.data, 1, H, W, ho.TAN_HALF_FOV, 70.0,
                                                       0.05, _arr(U, [0] * m), 0.85, a["cnts"], a["cloud"], nul, a["count"], _arr(LL, [64] * m),
                                                       a["ws"], need - short, None)
        torch.cuda.synchronize()
        assert int(count.item()) == 0
        return rc
    assert unproject(0) == E_ARG and unproject(13) == E_ARG
    assert unproject(2, null="cloud") == E_ARG and unproject(2, null="depth") == E_ARG
    assert unproject(2, H=3, W=5) == E_SHAPE                                    # H W % 4 != 0
    assert unproject(2, shift=4) == E_ARG                                       # a frame misaligned by 4 bytes
    assert unproject(2, short=1) == E_WS

    # ---- rasteriser: cap 12
    v, f = _box_mesh()
    vd, fd = _dev(v), _dev(f)
    H, W = 16, 24
    z, zf = torch.zeros(1, H, W, device=D), torch.zeros(1, H, W, dtype=torch.int64, device=D)
    need = int(hip.nbp_raster_workspace_bytes(12, 1, H, W, 0))
    ws = torch.empty(need, dtype=torch.uint8, device=D)

    def raster(n, null=None, short=0):
        a = dict(verts=_arr(VP, [vd.data_ptr()] * m), faces=_arr(VP, [fd.data_ptr()] * m), z=_arr(VP, [z.data_ptr()] * m),
                 zf=_arr(VP, [zf.data_ptr()] * m), ws=_arr(VP, [ws.data_ptr()] * m))
        if null:
            a[null][1] = None
        return hip.nbp_raster_zface_batch_f32(n, a["verts"], _arr(I, [8] * m), a["faces"], _arr(I, [12] * m), cams.ctypes.data, 1, H, W,
                                              ho.TAN_HALF_FOV, ho.Z_CLIP, a["z"], a["zf"], a["ws"], _arr(SZ, [need, need - short] + [need] * (m - 2)),
                                              None)
    assert raster(0) == E_ARG and raster(13) == E_ARG
    assert raster(2, null="verts") == E_ARG and raster(2, null="zf") == E_ARG
    assert raster(2, short=1) == E_WS
    torch.cuda.synchronize()
    assert float(z.abs().sum()) == 0.0
