"""The depth-frame filter's definition (nextbestpath_amd/utility/depth_filter.py), pinned without a GPU: the option's accept / refuse
rules, known answers worked by hand (constant frame, flying pixel, the gate's boundary, the lower-median rule, border windows, hole
filling), a pixel-by-pixel transcription of the definition with sorted lists, the exact equivariance under the image's symmetries,
and the statistics the filter must have on a noisy frame to be worth running."""
import os

import numpy as np
import pytest

from nextbestpath_amd.utility import depth_filter as df
from nextbestpath_amd.utility import depth_noise as dn

f32, u32 = np.float32, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def same(a, b):
    return a.dtype == b.dtype == f32 and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------- the option
def test_option_none_and_defaults():
    assert df.option_spec(None) is None
    assert df.option_spec({"range_base": 0.03}) == {"radius": 1, "range_base": 0.03, "range_quad": 0.0, "smooth": True,
                                                    "min_support": 0, "fill_support": 0}
    full = {"radius": 2, "range_base": 0, "range_quad": 0.003, "smooth": False, "min_support": 24, "fill_support": 18}
    got = df.option_spec(full)
    assert got == full and list(got) == ["radius", "range_base", "range_quad", "smooth", "min_support", "fill_support"]
    assert isinstance(got["range_base"], float) and isinstance(got["min_support"], int) and got["smooth"] is False
    assert df.option_spec(got) == got                               # a normalised spec is a fixed point
    assert df.option_spec({"range_quad": np.float32(0.5), "min_support": np.int64(8), "radius": np.int32(1)})["min_support"] == 8


@pytest.mark.parametrize("bad", [
    True, False, 1, "on", [], ("range_base", 1.0),                                   # another type: no preset
    {}, {"radius": 1}, {"range_base": 0.0, "range_quad": 0.0}, {"range_base": 0},    # both ranges 0
    {"range_base": 1.0, "sigma": 2.0}, {"range_base": 1.0, 3: 4},                    # unknown keys
    {"range_base": True}, {"range_base": 1.0, "range_quad": False}, {"range_base": "1"}, {"range_base": None},
    {"range_base": -0.1}, {"range_base": 1.0, "range_quad": -1e-9}, {"range_base": float("nan")}, {"range_base": float("inf")},
    {"range_base": 1.0, "radius": 0}, {"range_base": 1.0, "radius": 3}, {"range_base": 1.0, "radius": True},
    {"range_base": 1.0, "radius": 1.0}, {"range_base": 1.0, "radius": None},
    {"range_base": 1.0, "smooth": 1}, {"range_base": 1.0, "smooth": None}, {"range_base": 1.0, "smooth": "yes"},
    {"range_base": 1.0, "min_support": -1}, {"range_base": 1.0, "min_support": 9}, {"range_base": 1.0, "min_support": 2.0},
    {"range_base": 1.0, "min_support": True}, {"range_base": 1.0, "radius": 2, "min_support": 25},
    {"range_base": 1.0, "fill_support": -1}, {"range_base": 1.0, "fill_support": 9}, {"range_base": 1.0, "fill_support": False},
    {"range_base": 1.0, "radius": 2, "fill_support": 25}, {"range_base": 1.0, "fill_support": None},
])
def test_option_refuses(bad):
    with pytest.raises(ValueError):
        df.option_spec(bad)


def test_option_accepts_the_maxima():
    assert df.option_spec({"range_base": 1.0, "min_support": 8, "fill_support": 8})["fill_support"] == 8
    assert df.option_spec({"range_base": 1.0, "radius": 2, "min_support": 24, "fill_support": 24})["min_support"] == 24


def test_apply_refuses():
    z = np.zeros((3, 3), f32)
    for spec in (None, {}, {"range_base": 1.0, "radius": 3}):
        with pytest.raises(ValueError):
            df.apply(z, spec)
    for frame in (np.zeros((2, 3, 3), f32), np.zeros(5, f32), np.zeros((0, 4), f32)):
        with pytest.raises(ValueError):
            df.apply(frame, {"range_base": 1.0})


# ---------------------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("radius", [1, 2])
def test_constant_frame_comes_back(radius):
    """Every neighbour is inside the gate; the smallest window is the corner's: 3 neighbours at radius 1, 8 at radius 2."""
    z = np.full((6, 7), 7.5, f32)
    corner = 3 if radius == 1 else 8
    for smooth in (True, False):
        for support in range(corner + 1):
            out = df.apply(z, {"radius": radius, "range_base": 0.1, "smooth": smooth, "min_support": support, "fill_support": support})
            assert same(out, z), (smooth, support)
    out = df.apply(z, {"radius": radius, "range_base": 0.1, "min_support": corner + 1})
    lost = np.argwhere(out == -1).tolist()
    assert lost == [[0, 0], [0, 6], [5, 0], [5, 6]]                  # one more than the corner's window holds: the corners go


def test_flying_pixel_is_rejected_and_nothing_else_changes():
    z = np.empty((9, 9), f32)
    z[:, :5], z[:, 5:] = 10.0, 20.0
    z[4, 4] = 15.0                                                  # between the two surfaces: no neighbour within 0.5 of it
    out = df.apply(z, {"radius": 1, "range_base": 0.5, "min_support": 2})
    want = z.copy()
    want[4, 4] = -1.0
    assert same(out, want)
    assert same(df.apply(z, {"radius": 1, "range_base": 0.5}), z)   # without the support test it stays: its own median


def _window(centre, neighbours):
    z = np.full((3, 3), -1.0, f32)
    z[1, 1] = centre
    for (r, c), v in zip([(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)], neighbours):
        z[r, c] = v
    return z


@pytest.mark.parametrize("side", [+1, -1])
def test_gate_boundary(side):
    """range_quad 0, range_base T = 0.5, centre 10: a neighbour at exactly 10 +- T is in (|difference| = T exactly, <=), the next
    float beyond it is out (10.5 + 2^-20 - 10 and 10 - (9.5 - 2^-20) are 0.5 + 2^-20 exactly).  Two such neighbours: in, the set is
    {10, b, b}, whose rank-1 element is b; out, the set is {10}: the median flips, and so does the support count (2 -> 0)."""
    T = f32(0.5)
    at = f32(10.0) + f32(side) * T
    beyond = np.nextafter(at, f32(side * 100.0), dtype=f32)
    assert abs(float(at) - 10.0) == 0.5 and abs(float(beyond) - 10.0) == 0.5 + 2.0 ** -20
    spec = {"radius": 1, "range_base": 0.5, "range_quad": 0.0}
    for places in ((0, 7), (1, 3), (4, 6)):
        nb = [-1.0] * 8
        nb[places[0]] = nb[places[1]] = at
        assert bits(df.apply(_window(10.0, nb), spec))[1, 1] == bits(at)
        assert df.apply(_window(10.0, nb), dict(spec, min_support=2))[1, 1] == at
        assert df.apply(_window(10.0, nb), dict(spec, min_support=3))[1, 1] == -1.0
        nb[places[0]] = nb[places[1]] = beyond
        assert df.apply(_window(10.0, nb), spec)[1, 1] == f32(10.0)
        assert df.apply(_window(10.0, nb), dict(spec, min_support=1))[1, 1] == -1.0
        nb[places[0]] = at                                          # one in, one out: {10, at}, rank 0
        lower = min(f32(10.0), at)
        assert df.apply(_window(10.0, nb), dict(spec, min_support=1))[1, 1] == lower
        assert df.apply(_window(10.0, nb), dict(spec, min_support=2))[1, 1] == -1.0


def test_gate_quadratic_term():
    """gate(4) with range_base 0.25 and range_quad 0.0625 is 0.25 + 0.0625 * 16 = 1.25 exactly: 5.25 is in, the next float is out."""
    spec = {"radius": 1, "range_base": 0.25, "range_quad": 0.0625, "smooth": False, "min_support": 1}
    at = f32(5.25)
    assert df.apply(_window(4.0, [at] + [-1.0] * 7), spec)[1, 1] == f32(4.0)
    assert df.apply(_window(4.0, [np.nextafter(at, f32(9), dtype=f32)] + [-1.0] * 7), spec)[1, 1] == -1.0
    assert df.apply(_window(4.0, [-1.0] * 7 + [f32(2.75)]), spec)[1, 1] == f32(4.0)
    assert df.apply(_window(4.0, [-1.0] * 7 + [np.nextafter(f32(2.75), f32(0), dtype=f32)]), spec)[1, 1] == -1.0


def test_lower_median_of_an_even_set():
    """Centre 12 and gated neighbours 9, 10, 11: four values, rank 3 // 2 = 1 -> 10 (the upper median would be 11)."""
    spec = {"radius": 1, "range_base": 5.0}
    assert df.apply(_window(12.0, [11.0, -1.0, 9.0, -1.0, -1.0, 10.0, -1.0, -1.0]), spec)[1, 1] == f32(10.0)
    # an odd set: 9, 10, 11, 12, 13 -> 11; and a neighbour outside the gate (30) is not in the set
    assert df.apply(_window(12.0, [11.0, 13.0, 9.0, 30.0, -1.0, 10.0, -1.0, -1.0]), spec)[1, 1] == f32(11.0)
    assert df.apply(_window(12.0, [11.0, 13.0, 9.0, 30.0, -1.0, 10.0, -1.0, -1.0]), dict(spec, smooth=False))[1, 1] == f32(12.0)


def test_border_windows():
    one = np.full((1, 1), 3.0, f32)
    for radius in (1, 2):
        assert same(df.apply(one, {"radius": radius, "range_base": 1.0}), one)                      # S is empty: the median of {z}
        assert df.apply(one, {"radius": radius, "range_base": 1.0, "min_support": 1})[0, 0] == -1.0
        hole = np.full((1, 1), -1.0, f32)
        assert df.apply(hole, {"radius": radius, "range_base": 1.0, "fill_support": 1})[0, 0] == -1.0
    z = np.full((5, 5), 3.0, f32)
    # radius 1: a corner has 3 neighbours, an edge pixel 5, an interior pixel 8
    for support, survivors in ((3, 25), (4, 21), (5, 21), (6, 9), (8, 9)):
        out = df.apply(z, {"radius": 1, "range_base": 1.0, "min_support": support})
        assert int((out == 3.0).sum()) == survivors and int((out == -1.0).sum()) == 25 - survivors, support
    # radius 2 on 5 x 5: corner 8, next to the corner on the edge 11, edge middle 14, (1,1) 15, (1,2) 19, centre 24
    counts = {8: 25, 9: 21, 11: 21, 12: 13, 14: 13, 15: 9, 16: 5, 19: 5, 20: 1, 24: 1}
    for support, survivors in counts.items():
        out = df.apply(z, {"radius": 2, "range_base": 1.0, "min_support": support})
        assert int((out == 3.0).sum()) == survivors, support
    # a 1 x 5 row at radius 2: the ends have 2 neighbours, the middle 4
    row = np.full((1, 5), 3.0, f32)
    assert df.apply(row, {"radius": 2, "range_base": 1.0, "min_support": 3}).tolist() == [[-1.0, 3.0, 3.0, 3.0, -1.0]]


def test_fill():
    nb = [f32(10.0) + f32(0.01) * f32(k) for k in (3, 8, 1, 6, 5, 2, 7, 4)]           # 10.01 .. 10.08, shuffled
    lower, upper = sorted(nb)[3], sorted(nb)[4]
    spec = {"radius": 1, "range_base": 0.5, "smooth": False, "fill_support": 8}
    z = _window(-1.0, nb)
    out = df.apply(z, spec)
    assert bits(out)[1, 1] == bits(lower) and lower != upper       # rank (8 - 1) // 2 = 3: the lower median
    want = z.copy()
    want[1, 1] = lower
    assert same(out, want)                                          # smooth off: nothing else moves
    assert df.apply(z, dict(spec, fill_support=0))[1, 1] == -1.0
    # the same hole on a depth edge: one side of the window is 20
    edge = _window(-1.0, nb[:5] + [20.0, 20.0, 20.0])
    assert df.apply(edge, dict(spec, fill_support=1))[1, 1] == -1.0
    assert df.apply(edge, dict(spec, fill_support=1, range_base=10.0))[1, 1] == sorted(nb[:5] + [f32(20.0)] * 3)[3]
    # |V| = fill_support - 1 stays a hole; |V| = fill_support is filled with the rank (7 - 1) // 2 = 3 element
    seven = _window(-1.0, nb[:7] + [-1.0])
    assert df.apply(seven, spec)[1, 1] == -1.0
    assert df.apply(seven, dict(spec, fill_support=7))[1, 1] == sorted(nb[:7])[3]
    # NaN is invalid: as a neighbour it does not count, as a centre it is a hole
    nan7 = _window(-1.0, nb[:7] + [np.nan])
    assert df.apply(nan7, spec)[1, 1] == -1.0
    assert df.apply(nan7, dict(spec, fill_support=7))[1, 1] == sorted(nb[:7])[3]
    nanc = _window(np.nan, nb)
    assert bits(df.apply(nanc, spec))[1, 1] == bits(lower)
    assert df.apply(nanc, dict(spec, fill_support=0))[1, 1] == -1.0
    got = df.apply(_window(10.0, nb[:7] + [np.nan]), {"radius": 1, "range_base": 0.5, "min_support": 8})
    assert got[1, 1] == -1.0 and got[2, 2] == -1.0                  # 7 gated neighbours, not 8; the NaN pixel comes out as a hole


def _random_frame(H, W, holes, seed):
    rng = np.random.default_rng(seed)
    z = (rng.uniform(5.0, 6.0, (H, W)) + np.where(rng.random((H, W)) < 0.1, 3.0, 0.0)).astype(f32)
    z[rng.random((H, W)) < holes] = -1.0
    return z


def _by_the_book(z, spec):
    """The definition pixel by pixel, with Python lists and sorted()."""
    spec = df.option_spec(spec)
    H, W = z.shape
    r, rb, rq = spec["radius"], f32(spec["range_base"]), f32(spec["range_quad"])

    def gate(c):
        t = f32(c * c)
        t = f32(rq * t)
        return f32(rb + t)
    out = np.full((H, W), -1.0, f32)
    for y in range(H):
        for x in range(W):
            nb = [z[j, i] for j in range(max(0, y - r), min(H, y + r + 1)) for i in range(max(0, x - r), min(W, x + r + 1))
                  if (j, i) != (y, x) and z[j, i] > -1]
            c = z[y, x]
            if c > -1:
                S = [v for v in nb if f32(abs(f32(v - c))) <= gate(c)]
                if len(S) >= spec["min_support"]:
                    out[y, x] = sorted(S + [c])[len(S) // 2] if spec["smooth"] else c
            elif spec["fill_support"] > 0 and len(nb) >= spec["fill_support"]:
                m = sorted(nb)[(len(nb) - 1) // 2]
                if all(f32(abs(f32(v - m))) <= gate(m) for v in nb):
                    out[y, x] = m
    return out


ALL_ON = {1: {"radius": 1, "range_base": 0.2, "range_quad": 0.01, "min_support": 2, "fill_support": 5},
          2: {"radius": 2, "range_base": 0.2, "range_quad": 0.01, "min_support": 5, "fill_support": 14}}


@pytest.mark.parametrize("radius", [1, 2])
def test_apply_equals_the_definition_pixel_by_pixel(radius):
    z = _random_frame(14, 19, 0.2, 5 + radius)
    for spec in (ALL_ON[radius], dict(ALL_ON[radius], smooth=False), {"radius": radius, "range_quad": 0.02},
                 {"radius": radius, "range_base": 0.3, "fill_support": 1}):
        got, want = df.apply(z, spec), _by_the_book(z, spec)
        assert same(got, want), spec
    got = df.apply(z, ALL_ON[radius])
    assert ((got == -1) & (z > -1)).any() and ((got > -1) & (z == -1)).any() and ((got != z) & (got > -1) & (z > -1)).any()
    assert np.isin(got[got > -1], z).all()                          # every output value is an element of the input, or -1


@pytest.mark.parametrize("radius", [1, 2])
def test_exact_d4_equivariance(radius):
    """apply(op(z)) == op(apply(z)) bit for bit: the two flips, the transpose, a quarter turn (they generate the eight)."""
    z = _random_frame(33, 50, 0.2, 77)
    spec = ALL_ON[radius]
    base = df.apply(z, spec)
    assert ((base == -1) & (z > -1)).any() and ((base > -1) & (z == -1)).any() and ((base != z) & (base > -1) & (z > -1)).any()
    for name, op in (("flipud", np.flipud), ("fliplr", np.fliplr), ("transpose", np.transpose), ("rot90", np.rot90)):
        assert same(df.apply(np.ascontiguousarray(op(z)), spec), np.ascontiguousarray(op(base))), name


# ---------------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("radius,fill_support,rmse_bound", [(1, 6, 0.6), (2, 18, 0.4)])
def test_statistics_on_a_noisy_scene(radius, fill_support, rmse_bound):
    """A slanted plane with a box in front of it and a background patch, through the noise model (4 frames), then the filter.
    Measured with this definition: radius 1: RMSE ratio 0.459, holes 9174 -> 775, 0 background pixels filled, 244 valid raw pixels
    lost; radius 2: 0.288, 9174 -> 1051, 0, 11.  A filter that does nothing scores 1.0; a plain 3 x 3 median on i.i.d. Gaussian noise
    about 0.43."""
    H, W = 256, 456
    col, row = np.arange(W, dtype=f32)[None, :], np.arange(H, dtype=f32)[:, None]
    clean = (f32(8) + f32(12) * col / f32(W) + f32(0.01) * row).astype(f32)
    clean[60:160, 100:220] = 5.0
    clean[200:230, 300:380] = -1.0
    noise = {"sigma_base": 0.01, "sigma_quad": 0.001, "dropout": 0.02, "seed": 1}
    spec = {"radius": radius, "range_base": 0.03, "range_quad": 0.003, "min_support": 2, "fill_support": fill_support}
    se_f = se_r = 0.0
    holes_raw = holes_f = background = lost = valid_raw = 0
    for frame in range(4):
        raw = dn.apply(clean, 5, frame, noise)
        out = df.apply(raw, spec)
        cv, rv, fv = clean > -1, raw > -1, out > -1
        m = cv & rv & fv
        se_f += float(((out[m].astype(np.float64) - clean[m]) ** 2).sum())
        se_r += float(((raw[m].astype(np.float64) - clean[m]) ** 2).sum())
        holes_raw += int((cv & ~rv).sum())
        holes_f += int((cv & ~fv).sum())
        background += int((~cv & fv).sum())
        lost += int((rv & ~fv).sum())
        valid_raw += int(rv.sum())
    ratio = (se_f / se_r) ** 0.5
    print(f"radius {radius}: RMSE ratio {ratio:.3f}, holes {holes_raw} -> {holes_f}, background filled {background}, "
          f"valid raw pixels lost {lost} of {valid_raw}")
    assert ratio <= rmse_bound
    assert holes_raw > 0 and holes_f <= holes_raw / 4
    assert background == 0
    assert lost <= 0.005 * valid_raw


# ---------------------------------------------------------------------------------------------------------------- the wiring
def test_option_reaches_every_driver():
    import inspect
    import json

    from nextbestpath_amd.simulator import lockstep
    from nextbestpath_amd.simulator.camera import Camera
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.testers import random_walk_planning as rw
    from nextbestpath_amd.trainers import train_nbp_model
    from nextbestpath_amd.utility import hipops
    from nextbestpath_amd.utility import nbp_utils as nu
    cfg = json.load(open(os.path.join(ROOT, "configs/nbp/nbp_default_training_config.json")))["_nbp"]
    assert "collect_depth_filter" in cfg and cfg["collect_depth_filter"] is None
    assert 'depth_filter=getattr(params, "collect_depth_filter", None)' in inspect.getsource(train_nbp_model)
    for fn in (nu.trajectory_collection, Camera.__init__, lockstep.setup_test_camera, rw.test_random_walk_planning):
        assert inspect.signature(fn).parameters["depth_filter"].default is None, fn
    # the planning drivers take their options as **options, checked against the known names: the camera's are handed to the camera
    for fn in (tp.build_rollout, tp.run_one, tp.run_many, tp.test_nbp_planning):
        assert inspect.signature(fn).parameters["options"].kind is inspect.Parameter.VAR_KEYWORD, fn
    assert "depth_filter" in tp.CAMERA_OPTIONS and "depth_filter" in tp._test_config
    spec = {"range_base": 0.5}
    assert tp._known_options("run_one", {"depth_filter": spec}) is None
    for fn in (tp.build_rollout, tp.run_one, tp.run_many):
        with pytest.raises(TypeError, match="depth_blur"):        # (before anything is built: the other arguments are never read)
            fn(*[None] * 6, depth_filter=spec, depth_blur={})
    assert inspect.signature(Camera.frames_batch).parameters["raw"].default is False
    assert callable(hipops.depth_filter) and callable(hipops.depth_filter_batch) and callable(Camera.filter_item)


def test_test_config_key_resolves_like_depth_noise(tmp_path):
    import json

    from nextbestpath_amd.testers import nbp_planning as tp
    spec = {"range_base": 0.03, "min_support": 2}
    path = tmp_path / "cfg.json"
    try:
        path.write_text(json.dumps({"nbp_weights": "none", "depth_filter": spec}))
        tp.load_params(str(path))
        assert tp._test_config["depth_filter"] == spec
        path.write_text(json.dumps({"nbp_weights": "none"}))
        tp.load_params(str(path))
        assert tp._test_config["depth_filter"] is tp._UNSET
    finally:
        tp._test_config["depth_filter"] = tp._UNSET
