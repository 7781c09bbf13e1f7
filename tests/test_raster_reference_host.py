"""CPU: oracle/raster.py (the fp32 restatement every rasteriser GPU test is bit-compared with) against the float64 arbiter of
tests/raster_reference.py, on every seam scene and on the four triangle soups of test_gpu_sim_planner.py.  Pins, per frame and in
this order: the ambiguous share stays under its cap (a condition on the scene, not a measurement), hit / background agree on every
non-ambiguous pixel, the depth obeys the accuracy statement of raster_reference's docstring, and the winning face is one of the
arbiter's sure winners.  It also proves, with the device's face boxes restated in numpy, that each seam scene reaches the path of
nbp_sim.hip it is named after."""
import functools
import os

import numpy as np
import pytest

import raster_reference as rr
from oracle import camera as ocam
from oracle import raster as orast

HAVE_C_TWIN = os.path.isdir(os.path.join(os.path.dirname(os.path.abspath(orast.__file__)), "_build"))
TAGS = [t for t, _ in rr.seam_scenes()] + [f"soup{s}" for s in (1, 2, 3, 4)]


@functools.lru_cache(maxsize=None)
def scene(tag):
    if tag.startswith("soup"):
        sc = rr.soup(int(tag[4:]))
        sc["cams"] = [ocam.camera_RT(x, v) for x, v in sc["poses"]]
        return sc
    return dict(rr.seam_scenes())[tag]()


def test_constants_are_the_projects():
    from nextbestpath_amd.utility import hipops
    assert rr.TAN_HALF_FOV == ocam.TAN_HALF_FOV and float(rr.TAN_HALF_FOV) == hipops.TAN_HALF_FOV and rr.Z_CLIP == hipops.Z_CLIP
    assert rr.K_DEPTH >= 4 * rr.MEASURED_DEPTH_CONSTANT and rr.K_DEPTH == 2.0 ** np.ceil(np.log2(4 * rr.MEASURED_DEPTH_CONSTANT))


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_against_float64(tag):
    sc = scene(tag)
    v, f, H, W = sc["verts"], sc["faces"], sc["H"], sc["W"]
    colors = rr.id_colors(len(f))
    worst = 0.0
    for i, (R, T) in enumerate(sc["cams"]):
        arb = rr.depth64(v, f, R, T, H, W)
        z = orast.raster_zbuf(v, f, R, T, H, W, rr.TAN_HALF_FOV)
        if HAVE_C_TWIN:
            from oracle import csim
            assert np.array_equal(z.view(np.int32), csim.raster_zbuf(v, f, R, T, H, W, rr.TAN_HALF_FOV).view(np.int32)), (tag, i)
            zc, rgb = csim.raster_rgbz(v, f, colors, R, T, H, W, rr.TAN_HALF_FOV, ambient=1.0)
        else:
            zc, rgb = orast.raster_rgbz(v, f, colors, R, T, H, W, rr.TAN_HALF_FOV, ambient=1.0)
        assert np.array_equal(z.view(np.int32), zc.view(np.int32)), (tag, i)
        share = arb.ambiguous.mean()
        assert share <= rr.AMBIGUOUS_SHARE_CAP, (tag, i, share)
        ok = ~arb.ambiguous
        wrong = ok & ((z > 0) != arb.hit)
        assert not wrong.any(), (tag, i, int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
        ratio = np.where(ok, rr.depth_error_ratio(arb, v, f, R, T, z), 0.0)
        worst = max(worst, float(ratio.max()))
        print(f"{tag}[{i}]: ambiguous {100 * share:.3f} %, max err / (cond 2^-24) = {ratio.max():.3f}")
        assert ratio.max() <= rr.K_DEPTH, (tag, i, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
        ids = rr.decode_ids(rgb, z > 0)
        assert ids.max() < len(f)
        sure = arb.sure_winner(ids)
        bad = ok & (z > 0) & ~sure
        assert not bad.any(), (tag, i, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        if tag == "ties":
            assert (z > 0).all(), "crack in the tessellated plane"
            assert ids.max() < rr.TIES_BASE, "a copy under a higher id won a pixel"
            assert len(np.unique(ids)) > rr.TIES_BASE // 2
    assert worst <= rr.MEASURED_DEPTH_CONSTANT, (tag, worst)        # the documented measurement stays true


def _coarse_index(sc, k, frame=0):
    """Set of coarse tiles (row-major index) the box of face k touches in `frame`."""
    R, T = sc["cams"][frame]
    have, tx0, tx1, ty0, ty1 = rr.face_boxes32(sc["verts"], sc["faces"], R, T, sc["H"], sc["W"])
    ncx = -(-(-(-sc["W"] // 8)) // 8)
    if not have[k]:
        return set()
    return {cy * ncx + cx for cy in range(ty0[k] // 8, ty1[k] // 8 + 1) for cx in range(tx0[k] // 8, tx1[k] // 8 + 1)}


def test_coarse65_reaches_the_second_pass():
    sc = scene("coarse65")
    R, T = sc["cams"][0]
    counts = rr.coarse_list_counts(sc["verts"], sc["faces"], R, T, sc["H"], sc["W"])
    assert counts.shape == (3, 23) and counts.size > 64 and (counts > 0).all()
    for k in sc["only_late"]:
        tiles = _coarse_index(sc, k)
        assert tiles and min(tiles) >= 64, (k, tiles)
    assert {63, 64} <= _coarse_index(sc, sc["spanning"])
    assert _coarse_index(sc, sc["covering"]) == set(range(69))


@pytest.mark.parametrize("tag", ["wide2048", "tall2048"])
def test_strips_file_fine_tile_255(tag):
    sc = scene(tag)
    R, T = sc["cams"][0]
    have, tx0, tx1, ty0, ty1 = rr.face_boxes32(sc["verts"], sc["faces"], R, T, sc["H"], sc["W"])
    lo, hi = (tx0, tx1) if tag == "wide2048" else (ty0, ty1)
    for k in sc["last_tile"]:
        assert have[k] and lo[k] == 255 and hi[k] == 255, (k, lo[k], hi[k])
    assert have[sc["covering"]] and lo[sc["covering"]] == 0 and hi[sc["covering"]] == 255


def test_seg2_fills_a_second_segment_of_one_list_only():
    sc = scene("seg2")
    R, T = sc["cams"][0]
    counts = rr.coarse_list_counts(sc["verts"], sc["faces"], R, T, sc["H"], sc["W"])
    assert counts.shape == (2, 2) and rr.SEG < counts[0, 0] < 2 * rr.SEG
    rest = np.delete(counts.reshape(-1), 0)
    assert (rest > 0).all() and (rest < rr.SEG).all(), counts
    assert len(sc["faces"]) > rr.SEG                                  # the launch has two segments per block
    small = scene("small12")
    assert len(small["faces"]) == 12 and (small["H"], small["W"]) == (sc["H"], sc["W"])


@pytest.mark.parametrize("n", rr.PIECE_COUNTS)
def test_pieces_count_exactly_n(n):
    for place in rr.PIECE_PLACES:
        sc = scene(f"pieces{n}-{place}")
        R, T = sc["cams"][0]
        have, tx0, tx1, ty0, ty1 = rr.face_boxes32(sc["verts"], sc["faces"], R, T, 16, 16)
        assert len(have) == n and have.all() and (tx0 == 0).all() and (tx1 == 1).all() and (ty0 == 0).all() and (ty1 == 1).all()
        arb = rr.depth64(sc["verts"], sc["faces"], R, T, 16, 16)
        assert (arb.face == sc["nearest"]).all()


def test_clip_scene_culls_and_clamps():
    sc = scene("clip")
    R, T = sc["cams"][0]
    have, *_ = rr.face_boxes32(sc["verts"], sc["faces"], R, T, sc["H"], sc["W"])
    assert not have[sc["culled"]] and have[1:].all()
    view = (sc["verts"].astype(np.float64) @ R + T).reshape(-1, 3, 3)
    assert (view[0, :, 2] == 0.5).all() and view[1, 0, 2] == 0.5 and (view[4, :, 2] < 0).any()
    col = (sc["W"] - min(sc["H"], sc["W"]) * view[7, 0, 0] / (view[7, 0, 2] * float(rr.TAN_HALF_FOV)) - 1) / 2
    assert abs(col) > 1e8                                              # the +-1e8 clamp of the screen box is what keeps it an int
    arb = rr.depth64(sc["verts"], sc["faces"], R, T, sc["H"], sc["W"])
    for k in (5, 6, 7):                                                # each needle is seen (its pixels are arbiter-ambiguous)
        assert (arb.ambiguous & arb.possible_winner(np.full((sc["H"], sc["W"]), k))).any(), k


def test_segments_hit64_margins():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    f = np.array([[0, 1, 2]])
    p0 = np.array([[0.25, 0.25, -1], [0.25, 0.25, -1], [0.25, 0.25, 0.0], [0.5, 0.5, -1], [2, 2, -1]], np.float64)
    p1 = np.array([[0.25, 0.25, 1], [0.25, 0.25, 0.0], [0.25, 0.25, 1], [0.5, 0.5, 1], [2, 2, 1]], np.float64)
    hit, unsure = rr.segments_hit64(p0, p1, v, f)
    assert hit.tolist() == [True, False, False, False, False]
    assert unsure.tolist() == [False, True, True, True, False]       # ends on the face, starts on it, through an edge
