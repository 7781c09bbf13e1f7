"""Host side of the frontier policy (nextbestpath_amd/utility/frontier.py, the numpy definition): the sector partition, the heading
directions from the camera code, exact D4 equivariance, known answers, the domain, and the option parsing.  No GPU."""
import numpy as np
import pytest

import frontier_cases as fc
from nextbestpath_amd.utility import augment
from nextbestpath_amd.utility import frontier as fr


def random_maps(S, seed, density=0.3, band=0.2):
    """A map stack [6,S,S] with row 0 and column 0 zero: seen pixels at `density` spread over the five height channels, the
    camera-height band on `band` of them."""
    rng = np.random.default_rng(seed)
    m = np.zeros((6, S, S), np.float32)
    seen = rng.random((S, S)) < density
    ch = rng.integers(0, 5, (S, S))
    for k in range(5):
        m[k][seen & (ch == k)] = rng.integers(1, 9, int((seen & (ch == k)).sum()))
    m[5][seen & (rng.random((S, S)) < band)] = 2.0
    m[:, 0, :] = 0
    m[:, :, 0] = 0
    return m


def blob_maps(S, seed):
    """Seen regions with real boundaries: a few free rectangles with holes, so that frontiers are lines and not dust."""
    rng = np.random.default_rng(seed)
    m = np.zeros((6, S, S), np.float32)
    for _ in range(6):
        r0, c0 = rng.integers(1, S - 8, 2)
        h, w = rng.integers(4, S // 3, 2)
        m[int(rng.integers(0, 5)), r0:r0 + h, c0:c0 + w] = 1.0
    m[:5, rng.random((S, S)) < 0.05] = 0                       # pin-holes
    m[5][rng.random((S, S)) < 0.03] = 1.0
    m[:, 0, :] = 0
    m[:, :, 0] = 0
    return m


def test_sector_partition():
    R = 31
    d = np.arange(-R, R + 1)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    inside = np.stack([fr.in_sector(h, dy, dx) for h in range(8)])
    nonzero = (dy != 0) | (dx != 0)
    assert np.array_equal(inside.sum(0), nonzero.astype(np.int64))             # exactly one sector, none for the origin
    table = fr.sector_table(R)
    disc = nonzero & (dy * dy + dx * dx <= R * R)
    assert table.shape == (8, 2 * R + 1, 2 * R + 1) and np.array_equal(table.sum(0), disc.astype(np.int64))
    # a sector's pixels in a row are contiguous (a cone cut with a disc is convex): the kernel's table is one interval per row
    for r in (1, 2, 5, 24, 31):
        t = fr.sector_table(r)
        for h in range(8):
            for row in t[h]:
                cols = np.nonzero(row)[0]
                assert len(cols) == 0 or cols[-1] - cols[0] + 1 == len(cols)
    # the sum over the headings is the number of frontier pixels in the punctured disc
    S = 64
    f = np.zeros((S, S), bool)
    f[1:, 1:] = np.random.default_rng(0).random((S - 1, S - 1)) < 0.2
    for r in (1, 7, 31):
        g = fr.gain(f, r).sum(0)
        rr = np.arange(-r, r + 1)
        oy, ox = np.meshgrid(rr, rr, indexing="ij")
        keep = ((oy != 0) | (ox != 0)) & (oy * oy + ox * ox <= r * r)
        for g0, g1 in ((0, 0), (3, 15), (8, 8), (15, 0), (15, 15), (7, 2)):
            want = sum(bool(f[4 * g0 + y, 4 * g1 + x]) for y, x in zip(oy[keep], ox[keep])
                       if 0 <= 4 * g0 + y < S and 0 <= 4 * g1 + x < S)
            assert g[g0, g1] == want


def _heading_dir(h):
    """(d_row, d_col) of heading h from the camera code, as tests/test_augment_host.py derives it."""
    from nextbestpath_amd.simulator.camera import _look_rotation
    look = _look_rotation((0.0, 45.0 * h))[:, 2]
    return np.array([-look[2], -look[0]])


def test_directions_from_the_camera_code():
    S, V = 64, 16
    g0 = g1 = V // 2
    for h in range(8):
        d = _heading_dir(h)
        assert np.abs(d * np.abs(fr.DIRECTIONS[h]).sum() ** 0.5 - np.array(fr.DIRECTIONS[h])).max() < 1e-12
        f = np.zeros((S, S), bool)
        r, c = np.rint(np.array([4 * g0, 4 * g1]) + 10.0 * d).astype(int)
        f[r - 1:r + 2, c - 1:c + 2] = True                     # a 3 x 3 blob 10 pixels ahead of the cell
        g = fr.gain(f, 24)[:, g0, g1]
        assert g[h] == 9 and g.sum() == 9, (h, g)


def _moved_policy(m, op, **kw):
    return fr.policy(augment.transform_maps(m, op), **kw)


@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("unknown", ["free", "obstacle"])
def test_exact_d4_equivariance(S, unknown):
    maps = [random_maps(S, 11 + S, density=0.04), blob_maps(S, 12 + S)]
    n_front = n_valued = 0
    for m in maps:
        for d in (0, 2):
            for R in (5, 31):
                kw = dict(radius=R, dilate=d, unknown=unknown, distance_penalty=2)
                o1, o2 = fr.policy(m, **kw)
                n_front += int(fr.cell_classes(m, d)["frontier"].sum())
                n_valued += int((o1 > 0).sum())
                for op in range(8):
                    p1, p2 = _moved_policy(m, op, **kw)
                    w1, w2 = augment.transform_value_map(o1, op), augment.transform_maps(o2, op)
                    assert np.array_equal(p1[:, 1:, 1:], w1[:, 1:, 1:]), (d, R, op)
                    assert np.array_equal(p2[:, 1:, 1:], w2[:, 1:, 1:]), (d, R, op)
    assert n_front > 100 and n_valued > 100
    if unknown == "obstacle":
        assert o2.sum() > 0


def _square(S=64, r0=20, c0=30, n=7):
    m = np.zeros((6, S, S), np.float32)
    m[2, r0:r0 + n, c0:c0 + n] = 3.0
    return m


def _perimeter(S, r0, c0, n):
    f = np.zeros((S, S), bool)
    f[r0:r0 + n, c0:c0 + n] = True
    f[r0 + 1:r0 + n - 1, c0 + 1:c0 + n - 1] = False
    return f


def test_known_answer_square_and_pin_hole():
    S, r0, c0, n = 64, 20, 30, 7
    m = _square(S, r0, c0, n)
    for d in (0, 1):
        f = fr.cell_classes(m, d)["frontier"]
        assert f.sum() == 24 and np.array_equal(f, _perimeter(S, r0, c0, n))
    m[:, r0 + 3, c0 + 3] = 0                                   # one unseen pin-hole in the middle
    f0 = fr.cell_classes(m, 0)["frontier"]
    hole = np.zeros((S, S), bool)
    for dr, dc in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        hole[r0 + 3 + dr, c0 + 3 + dc] = True
    assert np.array_equal(f0, _perimeter(S, r0, c0, n) | hole) and f0.sum() == 28
    assert np.array_equal(fr.cell_classes(m, 1)["frontier"], _perimeter(S, r0, c0, n))
    # the band takes a pixel out of free space, and so out of the frontier
    m = _square(S, r0, c0, n)
    m[5, r0, c0 + 2] = 1.0
    f = fr.cell_classes(m, 0)["frontier"]
    assert f.sum() == 23 and not f[r0, c0 + 2]
    # out2: the unknown pixels of the domain, or nothing
    o1, o2 = fr.policy(_square(), unknown="obstacle", dilate=0)
    assert o2.shape == (1, S, S) and o2.sum() == (S - 1) ** 2 - n * n and o2[0, 0].sum() == 0 and o2[0, :, 0].sum() == 0
    assert fr.policy(_square(), unknown="free")[1].sum() == 0
    assert o1.dtype == np.float32 and o1.shape == (8, 16, 16)
    # the penalty: gain minus penalty times the Chebyshev ring, clamped at zero
    g = fr.gain(fr.cell_classes(_square(), 0)["frontier"], 24)
    p1 = fr.policy(_square(), dilate=0, distance_penalty=3)[0]
    for g0, g1 in ((5, 8), (6, 9), (0, 0), (8, 8), (4, 12)):
        assert np.array_equal(p1[:, g0, g1], np.maximum(g[:, g0, g1] - 3 * max(abs(g0 - 8), abs(g1 - 8)), 0).astype(np.float32))
    assert (g - p1).max() > 0 and p1.max() > 0


def test_domain_row_and_column_zero_change_nothing():
    S = 64
    m = random_maps(S, 5)
    m[2, 1:6, 1:6] = 1.0                                       # seen free space right beside the excluded row and column
    m[5, 1:6, 1:6] = 0.0
    want = [fr.policy(m, unknown=u, dilate=d) for u in ("free", "obstacle") for d in (0, 2)]
    rng = np.random.default_rng(6)
    m2 = m.copy()
    m2[:, 0, :] = rng.integers(0, 3, (6, S))
    m2[:, :, 0] = rng.integers(0, 3, (6, S))
    assert (m2[:, 0, :] > 0).any() and (m2[:, :, 0] > 0).any()
    got = [fr.policy(m2, unknown=u, dilate=d) for u in ("free", "obstacle") for d in (0, 2)]
    for (a1, a2), (b1, b2) in zip(want, got):
        assert np.array_equal(a1, b1) and np.array_equal(a2, b2)
    cls = fr.cell_classes(m2, 2)
    for k in ("seen", "occupied", "free", "unknown", "frontier"):
        assert not cls[k][0].any() and not cls[k][:, 0].any(), k


def test_pack_bits_round_trip():
    rng = np.random.default_rng(2)
    p = rng.random((3, 128, 128)) < 0.5
    w = fr.pack_bits(p)
    assert w.shape == (3, 128, 2) and w.dtype == np.uint64
    assert int(w[1, 5, 1]) == sum(1 << i for i in range(64) if p[1, 5, 64 + i])
    assert np.array_equal(fr.unpack_bits(w, 128), p)


def test_option_parsing():
    default = {"name": "frontier", "radius": 24, "dilate": 2, "unknown": "free", "distance_penalty": 0}
    assert fr.option_spec(None) is None and fr.option_spec("nbp") is None and fr.option_spec({"name": "nbp"}) is None
    assert fr.option_spec("frontier") == default and fr.option_spec({"name": "frontier"}) == default
    assert list(fr.option_spec("frontier")) == list(default)
    got = fr.option_spec({"name": "frontier", "radius": 31, "dilate": 0, "unknown": "obstacle", "distance_penalty": 3})
    assert got == {"name": "frontier", "radius": 31, "dilate": 0, "unknown": "obstacle", "distance_penalty": 3}
    assert fr.option_spec({"name": "frontier", "radius": np.int64(5)})["radius"] == 5
    for bad in (True, 3, "macarons", {"radius": 5}, {"name": "other"}, {"name": "frontier", "radios": 5},
                {"name": "frontier", "radius": 0}, {"name": "frontier", "radius": 32}, {"name": "frontier", "radius": 2.0},
                {"name": "frontier", "radius": True}, {"name": "frontier", "dilate": -1}, {"name": "frontier", "dilate": 9},
                {"name": "frontier", "unknown": "wall"}, {"name": "frontier", "unknown": None},
                {"name": "frontier", "distance_penalty": -1}, {"name": "frontier", "distance_penalty": 0.5},
                {"name": "nbp", "radius": 5}, ["frontier"]):
        with pytest.raises(ValueError):
            fr.option_spec(bad)
    with pytest.raises(ValueError):
        fr.policy(np.zeros((6, 96, 96), np.float32))           # S is not a multiple of 64
    with pytest.raises(ValueError):
        fr.policy(np.zeros((5, 64, 64), np.float32))
    with pytest.raises(ValueError):
        fr.policy(np.zeros((6, 64, 64), np.float32), radius=32)


def test_the_cases_reach_what_they_are_for():
    """The cases of tests/test_gpu_frontier.py hold frontier pixels whose windows hang over each edge and corner, and differ per batch item."""
    for name in ("seam", "s256", "density01", "density50"):
        m = fc.case(name)
        assert not any(np.array_equal(m[0], m[i]) for i in range(1, len(m)))
        g = fc.reference(name, 31, 0, "obstacle", 0)[0] if name != "s256" else fc.reference(name, 31, 1, "obstacle", 0)[0]
        V = g.shape[-1]
        for g0 in (0, V - 1):
            for g1 in (0, V // 2, V - 1):
                assert g[:, :, g0, g1].sum() > 0 and g[:, :, g1, g0].sum() > 0, (name, g0, g1)
    assert fc.reference("empty", 31, 0, "obstacle", 0)[0].sum() == 0 and fc.reference("empty", 31, 0, "obstacle", 0)[1].sum() == 2 * 63 * 63
    assert fc.reference("full", 31, 8, "obstacle", 3)[1].sum() == 0
    assert fc.reference("one_word", 24, 2, "free", 3)[0].max() > 0
    # 99 % seen: a few unknown pixels are left at d = 0 and give frontier; the closing at d = 8 leaves none
    assert fc.reference("density99", 31, 0, "obstacle", 0)[0].sum() > 0 and fc.reference("density99", 31, 8, "obstacle", 3)[0].sum() == 0
