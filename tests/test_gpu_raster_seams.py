"""GPU: the two-level binned rasteriser of csrc/nbp_sim.hip at its seams (tests/raster_reference.py builds the scenes and says
which path each one reaches).  Every entry point must give the oracle's depth bit for bit and the oracle's winning face; a pixel
may differ only where the float64 arbiter calls it ambiguous, and then only towards one of the arbiter's possible winners (or the
background).  The oracle here is its C twin (oracle/csim.py): tests/test_raster_reference_host.py holds the twin to
oracle/raster.py bit for bit and both to the float64 arbiter."""
import numpy as np
import pytest
import torch

import raster_reference as rr
from nextbestpath_amd import _lib
from nextbestpath_amd.utility import hipops as ho
from oracle import csim

pytestmark = pytest.mark.gpu
D = "cuda"
_cache = {}


def _scene(tag):
    """Scene, its device tensors and the oracle's (depth, face id) images: computed once, shared, never written to."""
    if tag not in _cache:
        sc = dict(rr.seam_scenes())[tag]()
        v, f, H, W = sc["verts"], sc["faces"], sc["H"], sc["W"]
        colors = rr.id_colors(len(f))
        zs, ids = [], []
        for R, T in sc["cams"]:
            z, rgb = csim.raster_rgbz(v, f, colors, R, T, H, W, rr.TAN_HALF_FOV, ambient=1.0)
            zs.append(z)
            ids.append(rr.decode_ids(rgb, z > 0))
        sc["z_oracle"], sc["id_oracle"] = np.stack(zs), np.stack(ids)
        sc["cams12"] = ho.cams12(np.stack([r for r, _ in sc["cams"]]), np.stack([t for _, t in sc["cams"]]))
        sc["vd"], sc["fd"] = torch.from_numpy(v).to(D), torch.from_numpy(f).to(D)
        _cache[tag] = sc
    return _cache[tag]


def check_against_oracle(sc, z_dev, zface_dev, what):
    """z_dev [F,H,W] fp32, zface_dev [F,H,W] int64 from the device -> the number of pixels that differ from the oracle."""
    v, f, H, W = sc["verts"], sc["faces"], sc["H"], sc["W"]
    total = 0
    for i, (R, T) in enumerate(sc["cams"]):
        z, zo = np.ascontiguousarray(z_dev[i]), sc["z_oracle"][i]
        assert np.isfinite(z).all()
        mism = z.view(np.int32) != zo.view(np.int32)
        n_mism = int(mism.sum())
        total += n_mism
        zf = zface_dev[i]
        face = np.where(zf == -1, -1, zf & 0xFFFFFFFF)
        assert np.array_equal((zf >> 32).astype(np.int32).view(np.float32)[face >= 0], z[face >= 0]), (what, i)
        assert np.array_equal(face >= 0, z > 0), (what, i)
        wrong_id = ~mism & (z > 0) & (face != sc["id_oracle"][i])
        assert not wrong_id.any(), (what, i, f"{int(wrong_id.sum())} pixels with the oracle's depth and another face",
                                    np.argwhere(wrong_id)[:4].tolist())
        if n_mism == 0:
            continue
        arb = rr.depth64(v, f, R, T, H, W)                             # only when something differs: the usual cost is the oracle's
        stray = mism & ~arb.ambiguous
        assert not stray.any(), (what, i, f"{n_mism} pixels differ from the oracle, {int(stray.sum())} of them not ambiguous",
                                 np.argwhere(stray)[:4].tolist())
        assert n_mism <= rr.AMBIGUOUS_SHARE_CAP * H * W, (what, i, f"{n_mism} pixels differ from the oracle")
        hit = mism & (z > 0)
        if hit.any():                             # a differing hit: a possible winner's depth, within the bound
            fimg = np.where(hit, face, -1)
            z64, _, _, _ = arb.evaluate(fimg)
            cond = rr.cond64(v, f, R, T, H, W, rr.TAN_HALF_FOV, fimg)
            okw = arb.possible_winner(fimg)
            with np.errstate(invalid="ignore", divide="ignore"):
                okz = np.abs(z.astype(np.float64) - z64) / z64 <= rr.K_DEPTH * cond * 2.0 ** -24
            bad = hit & ~(okw & okz)
            assert not bad.any(), (what, i, f"{n_mism} pixels differ from the oracle, {int(bad.sum())} are no possible winner's depth",
                                   np.argwhere(bad)[:4].tolist())
    return total


def _render_both(sc, **kw):
    z, _ = ho.raster_zbuf(sc["vd"], sc["fd"], sc["cams12"], sc["H"], sc["W"], **kw)
    z2, zf = ho.raster_zface(sc["vd"], sc["fd"], sc["cams12"], sc["H"], sc["W"], **kw)
    torch.cuda.synchronize()
    assert torch.equal(z.view(torch.int32), z2.view(torch.int32)), "raster_zbuf and raster_zface disagree on the depth"
    return z.cpu().numpy(), zf.cpu().numpy()


SCENES = ["coarse65", "wide2048", "tall2048", "seg2", "small12", "ties", "clip", "frames"]


@pytest.mark.parametrize("tag", SCENES)
def test_seam_scene_vs_oracle(hip, tag):
    sc = _scene(tag)
    z, zf = _render_both(sc)
    n = check_against_oracle(sc, z, zf, tag)
    print(f"{tag}: {n} pixels differ from the oracle")
    assert (z > 0).any()
    if tag == "ties":
        face = zf & 0xFFFFFFFF
        assert (z > 0).all(), "crack in the tessellated plane"
        assert int(face.max()) < rr.TIES_BASE, "a copy under a higher id won a pixel"


@pytest.mark.parametrize("n", rr.PIECE_COUNTS)
def test_piece_boundaries_vs_oracle(hip, n):
    for place in rr.PIECE_PLACES:
        sc = _scene(f"pieces{n}-{place}")
        z, zf = _render_both(sc)
        k = check_against_oracle(sc, z, zf, (n, place))
        print(f"pieces{n}-{place}: {k} pixels differ from the oracle")
        assert ((zf & 0xFFFFFFFF) == sc["nearest"]).all(), (n, place)


class _Owner:
    pass


def test_batch_with_and_without_a_second_segment(hip):
    """raster_zface_batch with one item that has a second list segment and one that has not: the launch's grid is the larger item's,
    the 12-face item's workgroups beyond its own a.gx_tile must leave its images alone.  Both orders; each equals its single call."""
    big, small = _scene("seg2"), _scene("small12")
    H, W = big["H"], big["W"]
    singles = [ho.raster_zface(s["vd"], s["fd"], s["cams12"], H, W) for s in (big, small)]
    singles = [(a.clone(), b.clone()) for a, b in singles]
    for order in ((big, small), (small, big)):
        outs = [(torch.full((1, H, W), 7.0, device=D), torch.full((1, H, W), 7, dtype=torch.int64, device=D)) for _ in order]
        ho.raster_zface_batch([(_Owner(), s["vd"], s["fd"], s["cams12"], oz, ozf) for s, (oz, ozf) in zip(order, outs)], H, W, 1)
        torch.cuda.synchronize()
        for s, (oz, ozf) in zip(order, outs):
            ref = singles[0] if s is big else singles[1]
            assert torch.equal(oz.view(torch.int32), ref[0].view(torch.int32)) and torch.equal(ozf, ref[1])
            check_against_oracle(s, oz.cpu().numpy(), ozf.cpu().numpy(), "batch")


def _refused(code, fn, *outs):
    """fn must raise the library's error `code` and leave the sentinel-filled outputs alone (nothing was launched)."""
    keep = [o.clone() for o in outs]
    with pytest.raises(_lib.NbpHipError, match=code):
        fn()
    torch.cuda.synchronize()
    for o, k in zip(outs, keep):
        assert torch.equal(o, k)


def test_refusals_launch_nothing(hip):
    sc = _scene("small12")
    vd, fd, cam = sc["vd"], sc["fd"], sc["cams12"]
    for H, W in ((8, 2049), (2049, 8)):
        oz = torch.full((1, H, W), 7.0, device=D)
        ozf = torch.full((1, H, W), 7, dtype=torch.int64, device=D)
        _refused("NBP_E_SHAPE", lambda: ho.raster_zbuf(vd, fd, cam, H, W, out=oz), oz)
        _refused("NBP_E_SHAPE", lambda: ho.raster_zface(vd, fd, cam, H, W, out_z=oz, out_zface=ozf), oz, ozf)
        _refused("NBP_E_SHAPE", lambda: ho.raster_zface_batch([(_Owner(), vd, fd, cam, oz, ozf)], H, W, 1), oz, ozf)
    fr = rr.scene_frames(9)
    c9 = ho.cams12(np.stack([r for r, _ in fr["cams"]]), np.stack([t for _, t in fr["cams"]]))
    v9, f9 = torch.from_numpy(fr["verts"]).to(D), torch.from_numpy(fr["faces"]).to(D)
    oz = torch.full((9, fr["H"], fr["W"]), 7.0, device=D)
    ozf = torch.full((9, fr["H"], fr["W"]), 7, dtype=torch.int64, device=D)
    _refused("NBP_E_ARG", lambda: ho.raster_zbuf(v9, f9, c9, fr["H"], fr["W"], out=oz), oz)
    _refused("NBP_E_ARG", lambda: ho.raster_zface(v9, f9, c9, fr["H"], fr["W"], out_z=oz, out_zface=ozf), oz, ozf)


@pytest.mark.parametrize("z_clip", [0.0, -0.5, float("nan")])
def test_z_clip_must_be_positive(hip, z_clip):
    """atomicMin on float bit patterns orders positive depths only: every rasteriser entry point refuses z_clip <= 0."""
    sc = _scene("small12")
    vd, fd, cam, H, W = sc["vd"], sc["fd"], sc["cams12"], sc["H"], sc["W"]
    oz = torch.full((1, H, W), 7.0, device=D)
    ozf = torch.full((1, H, W), 7, dtype=torch.int64, device=D)
    orgb = torch.full((1, H, W, 3), 7.0, device=D)
    col = torch.from_numpy(rr.id_colors(len(sc["faces"]))).to(D)
    _refused("NBP_E_ARG", lambda: ho.raster_zbuf(vd, fd, cam, H, W, z_clip=z_clip, out=oz), oz)
    _refused("NBP_E_ARG", lambda: ho.raster_zface(vd, fd, cam, H, W, z_clip=z_clip, out_z=oz, out_zface=ozf), oz, ozf)
    _refused("NBP_E_ARG", lambda: ho.raster_rgbz(vd, fd, col, cam, H, W, z_clip=z_clip, out_z=oz, out_rgb=orgb), oz, orgb)
    _refused("NBP_E_ARG", lambda: ho.raster_zface_batch([(_Owner(), vd, fd, cam, oz, ozf)], H, W, 1, z_clip=z_clip), oz, ozf)
    z, _ = ho.raster_zbuf(vd, fd, cam, H, W, z_clip=1e-3, out=oz)      # a small positive one is served
    torch.cuda.synchronize()
    assert (z > 0).any() and not (z == 7.0).any()
