"""Host side of the information-gain policy (nextbestpath_amd/utility/infogain.py, the numpy definition): the ray fan, exact D4
equivariance, the bound by the frontier count, known answers behind walls, and the option parsing.  No GPU."""
import os

import numpy as np
import pytest

import infogain_cases as ic
from nextbestpath_amd.utility import augment
from nextbestpath_amd.utility import frontier as fr
from nextbestpath_amd.utility import infogain as ig


def sparse_maps(S, seed, band):
    """Seen blobs in unknown space with the band on `band` of all pixels (sparse: rays travel); row 0 and column 0 zero."""
    rng = np.random.default_rng(seed)
    m = np.zeros((6, S, S), np.float32)
    for _ in range(5):
        r0, c0 = rng.integers(1, S - 8, 2)
        h, w = rng.integers(6, S // 2, 2)
        m[int(rng.integers(0, 5)), r0:r0 + h, c0:c0 + w] = 1.0
    m[:5, rng.random((S, S)) < 0.05] = 0                       # pin-holes
    m[5][rng.random((S, S)) < band] = 1.0
    m[:, 0, :] = 0
    m[:, :, 0] = 0
    return m


def _planes(m, d):
    cls = fr.cell_classes(m, d)
    S = m.shape[1]
    blocked = cls["occupied"].copy()
    blocked[0, :] = blocked[:, 0] = True
    assert np.array_equal(blocked, ig._blocked_unknown(m, d)[0])
    return blocked, cls["unknown"]


@pytest.mark.parametrize("R", range(1, 32))
def test_the_fan_covers_the_square_and_is_d4_symmetric(R):
    t = ig.ray_table(R)
    assert t.shape == (8 * R, R, 2) and t.dtype == np.int64
    assert len({tuple(p) for p in t[:, -1]}) == 8 * R and (np.abs(t[:, -1]).max(1) == R).all()         # one ray per rim pixel
    k = np.arange(1, R + 1)
    assert (np.abs(t).max(2) == k[None]).all()                 # the major axis advances by one per point
    want = np.sign(t[:, -1:, :]) * np.floor(k[None, :, None] * np.abs(t[:, -1:, :]) / R + 0.5).astype(np.int64)
    assert np.array_equal(t, want)                             # k m / R, halves away from zero (k |m| / R + 1/2 is exact in doubles)
    cover = np.zeros((2 * R + 1, 2 * R + 1), bool)
    cover[t[..., 0] + R, t[..., 1] + R] = True
    cover[R, R] = True
    assert cover.all()
    rays = {tuple(map(tuple, ray)) for ray in t}
    for move in (lambda p: (p[1], p[0]), lambda p: (-p[0], p[1]), lambda p: (p[0], -p[1])):              # the three generators
        assert {tuple(move(p) for p in ray) for ray in rays} == rays


@pytest.mark.parametrize("S,combos", [(64, ((5, 0), (12, 1), (31, 0), (24, 2))), (128, ((31, 0), (12, 2)))])
@pytest.mark.parametrize("unknown", ["free", "obstacle"])
def test_exact_d4_equivariance(S, combos, unknown):
    n_valued = n_cut = 0
    for i, band in enumerate((0.005, 0.03)):
        m = sparse_maps(S, 3 + S + i, band)
        assert 0.004 < (m[5, 1:, 1:] > 0).mean() < 0.035
        for R, d in combos:
            kw = dict(radius=R, dilate=d, unknown=unknown, distance_penalty=1)
            o1, o2 = ig.policy(m, **kw)
            n_valued += int((o1 > 0).sum())
            n_cut += int((o1 < np.maximum(fr.gain(fr.cell_classes(m, d)["unknown"], R) - ig_ring(S), 0)).sum())
            for op in range(1, 8):
                p1, p2 = ig.policy(augment.transform_maps(m, op), **kw)
                w1, w2 = augment.transform_value_map(o1, op), augment.transform_maps(o2, op)
                assert np.array_equal(p1[:, 1:, 1:], w1[:, 1:, 1:]), (R, d, op)
                assert np.array_equal(p2[:, 1:, 1:], w2[:, 1:, 1:]), (R, d, op)
    assert n_valued > 100 and n_cut > 100                      # values to move, and walls that took some away
    if unknown == "obstacle":
        assert o2.sum() > 0


def ig_ring(S):
    g = np.arange(S // 4)
    return np.maximum(np.abs(g - S // 8)[:, None], np.abs(g - S // 8)[None, :])[None]


@pytest.mark.parametrize("R,d", [(1, 0), (7, 2), (24, 0), (31, 1)])
def test_without_walls_it_is_the_count_of_unknown_pixels(R, d):
    m = sparse_maps(64, 9, 0.0)
    blocked, unknown = _planes(m, d)
    assert not blocked[1:, 1:].any() and unknown.any()
    g, want = ig.gain(blocked, unknown, R), fr.gain(unknown, R)
    assert np.array_equal(g[:, 1:, 1:], want[:, 1:, 1:]) and want[:, 1:, 1:].sum() > 0
    assert not g[:, 0].any() and not g[:, :, 0].any()          # value row 0 and value column 0 stand outside the domain
    assert want[:, 0].any() and want[:, :, 0].any()


def test_never_more_than_the_count_of_unknown_pixels():
    checked = 0
    for name, R, d, unknown, penalty in ic.POLICY_CASES:
        o1 = ic.reference(name, R, d, unknown, penalty)[0]
        for m, got in zip(ic.case(name), o1):
            bound = np.maximum(fr.gain(fr.cell_classes(m, d)["unknown"], R) - penalty * ig_ring(m.shape[1]), 0)
            assert (got <= bound).all(), (name, R, d)
            checked += 1
    assert checked > 40


def test_a_closed_room_and_a_door():
    R = 20
    closed = ig.gain(*_planes(ic.room(False), 0), R)
    assert not closed[:, 7:10, 7:10].any()                     # the cells inside (pixels 28..36) see no unknown space
    assert fr.gain(_planes(ic.room(False), 0)[1], R)[:, 8, 8].min() > 0          # ... which lies within reach in every heading
    door = ig.gain(*_planes(ic.room(True), 0), R)
    assert door[0, 8, 8] == 33 and not door[1:, 8, 8].any()    # through the door in the north wall: heading 0 only
    inside = door[:, 7:10, 7:10]
    assert inside[0, :, 1].all() and not inside[1:, :, 1].any()                  # so for the cells straight below the door
    vis = ig.visible(ic.room(True), dilate=0, radius=R, cells=[(8, 8)])[0]
    assert vis.shape == (2 * R + 1, 2 * R + 1) and not vis[R, R]
    assert vis[R - 7:R + 8, R - 7:R + 8].sum() == 15 * 15 - 1 and vis[R - 8, R]          # the room but the cell's own pixel; the door
    assert not vis[R + 8:].any() and not vis[:, R + 8:].any() and not vis[:, :R - 7].any()
    assert (vis & fr.sector_table(R)[0])[:R - 7].sum() == 33   # the door and what lies beyond it, all unknown: the gain
    assert not ig.visible(ic.room(True), dilate=0, radius=R, cells=[(6, 7), (0, 3)]).any()             # on the wall; outside the domain


def test_a_staircase_wall_is_not_slipped_through():
    R = 31
    g0, g1 = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    near = 4 * g0 + 4 * g1 < 70
    blocked, unknown = _planes(ic.stairs(False), 0)
    wall = blocked[1:, 1:]
    assert not (wall[1:, :] & wall[:-1, :]).any() and not (wall[:, 1:] & wall[:, :-1]).any()           # 8-connected only
    assert not ig.gain(blocked, unknown, R)[:, near].any()
    assert fr.gain(unknown, R)[:, near].sum() > 10000
    assert sum(ic.corner_cuts(blocked, R, a, b) for a, b in ((8, 8), (4, 12), (12, 3))) > 50           # the corner rule did it
    gap = ig.gain(*_planes(ic.stairs(True), 0), R)
    assert gap[5, 8, 8] == 221 and not gap[[0, 1, 2, 3, 4, 6, 7], 8, 8].any()
    assert gap[:, near].sum() == 1923


def test_option_parsing():
    default = {"name": "infogain", "radius": 24, "dilate": 2, "unknown": "free", "distance_penalty": 0}
    assert ig.option_spec(None) is None and ig.option_spec("nbp") is None and ig.option_spec({"name": "nbp"}) is None
    assert ig.option_spec("infogain") == default and ig.option_spec({"name": "infogain"}) == default
    assert list(ig.option_spec("infogain")) == list(default)
    got = ig.option_spec({"name": "infogain", "radius": 31, "dilate": 0, "unknown": "obstacle", "distance_penalty": 3})
    assert got == {"name": "infogain", "radius": 31, "dilate": 0, "unknown": "obstacle", "distance_penalty": 3}
    assert ig.option_spec({"name": "infogain", "radius": np.int64(5)})["radius"] == 5
    for bad in (True, 3, "macarons", "frontier", {"radius": 5}, {"name": "other"}, {"name": "frontier"}, {"name": "infogain", "radios": 5},
                {"name": "infogain", "radius": 0}, {"name": "infogain", "radius": 32}, {"name": "infogain", "radius": 2.0},
                {"name": "infogain", "radius": True}, {"name": "infogain", "dilate": -1}, {"name": "infogain", "dilate": 9},
                {"name": "infogain", "unknown": "wall"}, {"name": "infogain", "unknown": None},
                {"name": "infogain", "distance_penalty": -1}, {"name": "infogain", "distance_penalty": 0.5},
                {"name": "nbp", "radius": 5}, ["infogain"]):
        with pytest.raises(ValueError):
            ig.option_spec(bad)
    for bad in ("infogain", {"name": "infogain"}, {"name": "infogain", "radius": 5}):
        with pytest.raises(ValueError):
            fr.option_spec(bad)                                # the frontier policy's parser keeps refusing every name but its own
    with pytest.raises(ValueError):
        ig.policy(np.zeros((6, 96, 96), np.float32))           # S is not a multiple of 64
    with pytest.raises(ValueError):
        ig.policy(np.zeros((6, 64, 64), np.float32), radius=32)
    with pytest.raises(ValueError):
        ig.visible(np.zeros((6, 64, 64), np.float32), cells=[(16, 0)])
    with pytest.raises(ValueError):
        ig.ray_table(0)


def test_make_policy_dispatches_on_the_name():
    from nextbestpath_amd.testers.frontier_policy import FrontierPolicy, InfoGainPolicy, make_policy
    assert make_policy(None) is None and make_policy("nbp") is None and make_policy({"name": "nbp"}) is None
    p = make_policy({"name": "infogain", "radius": 12})
    assert type(p) is InfoGainPolicy and p.wants_maps6 and p.options == dict(ig.option_spec("infogain"), radius=12)
    assert type(make_policy("frontier")) is FrontierPolicy and make_policy("frontier").options == fr.option_spec("frontier")
    with pytest.raises(ValueError, match="'frontier'.*'infogain'"):
        make_policy("macarons")                                # the error lists both names
    for bad in ({"name": "infogain", "radius": 40}, {"name": "infogain", "colour": 1}, {"name": "nbp", "radius": 1}, 3, ["infogain"]):
        with pytest.raises(ValueError):
            make_policy(bad)
    with pytest.raises(ValueError):
        p.symmetry_ensemble = "d4"
    p.symmetry_ensemble = None
    with pytest.raises(ValueError):
        InfoGainPolicy("frontier")


def test_the_cases_reach_what_they_are_for():
    """The cases of tests/test_gpu_infogain.py: a ray cut by the corner rule, a ray across the word seam, gain in every heading of one
    cell, windows over every edge, every band density, and items of a batch that differ."""
    for name in ("seam", "s256", "bands", "rooms"):
        m = ic.case(name)
        assert not any(np.array_equal(m[0], m[i]) for i in range(1, len(m)))
    seam = ic.case("seam")
    blocked = ig._blocked_unknown(seam[0], 0)[0]
    assert sum(ic.corner_cuts(blocked, 31, g0, g1) for g0 in range(18, 26) for g1 in (13, 15, 16, 18)) > 0      # at the diagonal wall
    assert sum(ic.corner_cuts(ig._blocked_unknown(ic.case("bands")[3], 0)[0], 31, 16, g1) for g1 in range(1, 32)) > 0
    vis = ig.visible(seam[0], dilate=0, radius=31, cells=[(16, 15), (16, 17)])        # pixels (64, 60) and (64, 68) in the corridor
    assert vis[0][:, 31 + 4:].any() and vis[1][:, :31 - 5].any()                       # seen across the seam, from either side
    o1 = ic.reference("seam", 31, 0, "obstacle", 3)[0]
    assert (o1 > 0).all(1).any() and (ic.reference("bands", 31, 0, "obstacle", 3)[0] > 0).all(1).any()
    V = o1.shape[-1]
    g = ic.reference("seam", 24, 2, "free", 0)[0]
    for e in (1, V - 1):                                       # windows that hang over each edge and corner hold gain
        for k in (1, V // 2, V - 1):
            assert g[:, :, e, k].sum() > 0 and g[:, :, k, e].sum() > 0, (e, k)
    dens = [(m[5, 1:, 1:] > 0).mean() for m in ic.case("bands")]
    assert dens[0] == 0 and 0.003 < dens[1] < 0.007 and 0.02 < dens[2] < 0.04 and 0.13 < dens[3] < 0.17 and dens[4] == 1
    b = ic.reference("bands", 31, 0, "obstacle", 3)[0]
    assert b[0].sum() > b[1].sum() > b[2].sum() > b[3].sum() > 0 and b[4].sum() == 0
    assert ic.reference("empty", 31, 0, "obstacle", 0)[0][:, :, 1:, 1:].min() > 0 and ic.reference("empty", 31, 0, "obstacle", 0)[1].sum() == 2 * 63 * 63
    cells = ic.edge_cells(3, 32)
    assert cells[:, 1].min() == 0 and cells[:, 1].max() == 31 and cells[:, 2].min() == 0 and cells[:, 2].max() == 31 and set(cells[:, 0]) == {0, 1, 2}


def test_the_committed_config_names_the_policy():
    from nextbestpath_amd.testers import nbp_planning as tp
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = tp.load_params(os.path.join(root, "configs/test/test_via_infogain.json"))
    assert ig.option_spec(p.policy) == ig.option_spec("infogain") and p.results_json_name == "synth_simple_infogain.json"
