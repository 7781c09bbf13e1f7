"""The depth-sensor noise model's definition (nextbestpath_amd/utility/depth_noise.py), pinned without a GPU: known answers of the
counter-based words and of the Gaussian stand-in, a worked 7 x 13 frame, the option's accept / refuse rules, the identity when every
effect is zero, and the statistics the words must have for the model to be usable as noise."""
import os

import numpy as np
import pytest

from nextbestpath_amd.utility import depth_noise as dn

f32, u32 = np.float32, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _px(*p):
    return np.asarray(p, u32)


def test_known_words():
    key = dn.frame_key(3, 2)
    assert key == 0x6d47486c
    got = [int(dn.words(_px(0), k, key)[0]) for k in range(4)]
    assert got == [0x637c6fc6, 0x3e765104, 0xdea95fd7, 0xa1642b5b]
    assert sum(int(b) for w in got for b in w.to_bytes(4, "little")) == 1893
    assert int(dn.words(_px(5), 4, key)[0]) == 0xaabd9897
    assert int(dn.words(_px(0), 0, dn.frame_key(0, 0))[0]) == 0x6648b050


def test_known_gaussians():
    g = dn.gaussian(_px(0, 5, 90), dn.frame_key(3, 2))
    assert g.dtype == f32
    assert [float(v).hex() for v in g] == [float.fromhex(h).hex() for h in ("-0x1.fd3a10p-2", "-0x1.013626p+0", "0x1.ad8d48p-2")]
    assert float(dn.G_SCALE) == float(f32(1.0 / np.sqrt(16 * (256.0 ** 2 - 1) / 12)))
    # 4081 levels, bounded: the extreme byte sums
    lo, hi = (f32(0) - dn.G_MEAN) * dn.G_SCALE, (f32(4080) - dn.G_MEAN) * dn.G_SCALE
    assert -6.91 < lo < -6.9 and 6.9 < hi < 6.91


def test_seed_and_frame_wrap():
    assert dn.frame_key(3 + (1 << 32), 2) == dn.frame_key(3, 2)
    assert dn.frame_key(3, 2 + (1 << 32)) == dn.frame_key(3, 2)
    assert dn.word_seed({"seed": 4294967295}, 2) == (4294967295 + 2 * 7919) % (1 << 32)
    assert dn.dropout_threshold(0.0) == 0 and dn.dropout_threshold(0.5) == 1 << 31
    assert dn.dropout_threshold(np.nextafter(1.0, 0.0)) <= (1 << 32) - 1


WORKED = dict(sigma_base=0.01, sigma_quad=0.002, dropout=0.1, edge_threshold=5.0, z_min=0.5)


def worked_frame():
    z = np.full((7, 13), 10.0, f32)
    z[:2] = 30.0
    z[3, 5] = -1.0
    return z


def test_worked_frame():
    out = dn.apply(worked_frame(), 3, 2, WORKED)
    assert out.dtype == f32 and out.shape == (7, 13)
    gone = {tuple(int(v) for v in rc) for rc in np.argwhere(out == -1.0)}
    want = {(r, c) for r in (1, 2) for c in range(13)} | {(0, 6), (5, 7), (3, 5)}
    assert gone == want and len(gone) == 29
    assert float(out[0, 0]).hex() == float.fromhex("0x1.d19932p+4").hex()
    assert float(out[3, 0]).hex() == float.fromhex("0x1.46faa8p+3").hex()
    assert float(out[6, 12]).hex() == float.fromhex("0x1.42d1a6p+3").hex()
    # the spec's own seed plays no part in apply (the caller mixes it into the word seed)
    assert np.array_equal(out, dn.apply(worked_frame(), 3, 2, dict(WORKED, seed=99)))


def test_edge_rules():
    """Neighbours outside the image and background neighbours do not count; the comparison is strict and in fp32."""
    spec = dict(edge_threshold=5.0)
    z = np.full((3, 4), 10.0, f32)
    z[1, 1] = -1.0                                  # a hole: its neighbours are NOT flying pixels
    assert np.array_equal(dn.apply(z, 0, 0, spec), z)
    z = np.full((1, 3), 10.0, f32)
    z[0, 2] = 15.0                                  # a step of exactly the threshold stays
    assert np.array_equal(dn.apply(z, 0, 0, spec), z)
    z[0, 2] = np.nextafter(f32(15.0), f32(16.0))
    assert dn.apply(z, 0, 0, spec).tolist() == [[10.0, -1.0, -1.0]]
    assert dn.apply(np.full((1, 1), 3.0, f32), 0, 0, spec).tolist() == [[3.0]]


def test_option_spec_accepts():
    assert dn.option_spec(None) is None
    assert dn.option_spec({}) == {"sigma_base": 0.0, "sigma_quad": 0.0, "dropout": 0.0, "edge_threshold": 0.0, "z_min": 0.5, "seed": 0}
    s = dn.option_spec({"sigma_base": 1, "sigma_quad": 0.25, "dropout": 0.5, "edge_threshold": None, "z_min": 2, "seed": 7})
    assert s == {"sigma_base": 1.0, "sigma_quad": 0.25, "dropout": 0.5, "edge_threshold": 0.0, "z_min": 2.0, "seed": 7}
    assert isinstance(s["sigma_base"], float) and isinstance(s["seed"], int)
    assert dn.option_spec(s) == s                   # a normalised spec is its own normal form
    assert dn.option_spec({"edge_threshold": 0})["edge_threshold"] == 0.0
    import json
    assert json.loads(json.dumps(s)) == s


@pytest.mark.parametrize("bad", [True, False, "typical", 1.0, [0.1], {"sigma": 0.1}, {"sigma_base": -0.1}, {"sigma_quad": -1e-9},
                                 {"dropout": 1.0}, {"dropout": 1.5}, {"dropout": -0.1}, {"z_min": 0}, {"z_min": -1.0},
                                 {"edge_threshold": -5.0}, {"seed": -1}, {"seed": 1.5}, {"sigma_base": float("nan")},
                                 {"sigma_base": float("inf")}, {"sigma_base": "0.1"}, {"sigma_base": None}, {"seed": None}])
def test_option_spec_refuses(bad):
    with pytest.raises(ValueError):
        dn.option_spec(bad)


def test_apply_refuses():
    with pytest.raises(ValueError):
        dn.apply(np.zeros((4, 4), f32), 0, 0, None)
    with pytest.raises(ValueError):
        dn.apply(np.zeros((2, 4, 4), f32), 0, 0, {})
    with pytest.raises(ValueError):
        dn.apply(np.zeros((0, 4), f32), 0, 0, {})


def test_identity_when_every_effect_is_zero():
    rng = np.random.default_rng(5)
    z = rng.uniform(0.5, 80.0, (33, 100)).astype(f32)
    z[0, 0] = f32(0.5)
    z[rng.random((33, 100)) < 0.2] = -1.0
    for seed, frame in ((0, 0), (3, 2), (12345, 4294967295)):
        out = dn.apply(z, seed, frame, {})
        assert out.tobytes() == z.tobytes()
    # below z_min the clamp shows, and only there
    z2 = z.copy()
    z2[5, 5] = f32(0.25)
    out = dn.apply(z2, 1, 1, {})
    assert out[5, 5] == f32(0.5)
    out[5, 5] = z2[5, 5]
    assert out.tobytes() == z2.tobytes()


H, W = 256, 456
N = H * W


def _corr(a, b):
    a = a.astype(np.float64).ravel() - a.mean(dtype=np.float64)
    b = b.astype(np.float64).ravel() - b.mean(dtype=np.float64)
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("seed", [0, 1, 12345])
@pytest.mark.parametrize("frame", [0, 1, 407])
def test_statistics(seed, frame):
    """mean, standard deviation, dropout fraction at 4 sigma of their sampling error; correlations of g between neighbouring pixels
    and consecutive frames below 0.012 (sampling error 1 / sqrt(N) = 0.003)."""
    p = np.arange(N, dtype=u32).reshape(H, W)
    key = dn.frame_key(seed, frame)
    g = dn.gaussian(p, key).astype(np.float64)
    mean, sd = g.mean(), g.std()
    frac = float((dn.words(p, 4, key) < u32(dn.dropout_threshold(0.1))).mean())
    g_next = dn.gaussian(p, dn.frame_key(seed, frame + 1))
    ch, cv, cf = _corr(g[:, 1:], g[:, :-1]), _corr(g[1:], g[:-1]), _corr(g, g_next)
    print(f"seed {seed} frame {frame}: mean {mean:+.4f} sd-1 {sd - 1:+.4f} dropout-0.1 {frac - 0.1:+.4f} corr h {ch:+.4f} v {cv:+.4f} "
          f"frames {cf:+.4f}")
    assert abs(mean) <= 4 / np.sqrt(N)
    assert abs(sd - 1) <= 4 / np.sqrt(2 * N)
    assert abs(frac - 0.1) <= 4 * np.sqrt(0.09 / N)
    assert max(abs(ch), abs(cv), abs(cf)) < 0.012
    assert np.abs(g).max() <= 6.91


def test_trainer_option_reaches_the_collector():
    import inspect
    import json

    from nextbestpath_amd.trainers import train_nbp_model
    from nextbestpath_amd.utility import nbp_utils as nu
    cfg = json.load(open(os.path.join(ROOT, "configs/nbp/nbp_default_training_config.json")))["_nbp"]
    assert "collect_depth_noise" in cfg and cfg["collect_depth_noise"] is None
    assert inspect.signature(nu.trajectory_collection).parameters["depth_noise"].default is None
    assert 'depth_noise=getattr(params, "collect_depth_noise", None)' in inspect.getsource(train_nbp_model)
