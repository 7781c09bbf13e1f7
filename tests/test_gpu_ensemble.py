"""GPU: the D4 symmetry ensemble of the eval forward -- nbp_ensemble_expand_f32 against transform_maps (bit for bit),
nbp_ensemble_reduce_f32 against the float64 definition (augment.ensemble_reference) within the rounding of its n fp32 additions and
one division, argument errors, NBP.symmetry_ensemble through every eval forward path (eager, captured graph, sliced inner batch,
the lock-step planner's two packed calls) and the equivariance the ensemble buys."""
import os

import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import augment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.device("cuda")

SHAPES = [(3, 16), (2, 80), (1, 144)]      # a tile smaller than the block; 64 + 16; two full tiles and a remainder (V = 4, 20, 36)
SPECS = ["c2", "flips", "d4", (0, 3, 5)]   # (0, 3, 5): the pair that is not self-inverse


def _ops(spec):
    from nextbestpath_amd.utility import hipops
    ops = augment.check_ensemble(spec)
    return ops, hipops.symmetry_ops(ops, D)


@pytest.mark.parametrize("spec", SPECS, ids=str)
@pytest.mark.parametrize("B,S", SHAPES)
def test_expand_equals_transform_maps_bit_for_bit(hip, B, S, spec):
    from nextbestpath_amd.utility import hipops
    ops, ops_dev = _ops(spec)
    x = (np.random.default_rng(S).standard_normal((B, 5, S, S)) + 3.0).astype(np.float32)      # row 0 / col 0 non-zero
    xd = torch.from_numpy(x).to(D)
    out = hipops.symmetry_expand(xd, ops_dev)
    own = torch.full((len(ops), B, 5, S, S), -7.0, device=D)
    assert hipops.symmetry_expand(xd, ops_dev, out=own) is own
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), torch.from_numpy(x))                                           # out of place
    assert out.shape == (len(ops), B, 5, S, S) and torch.equal(out, own)
    out = out.cpu().numpy()
    for k, op in enumerate(ops):
        assert np.array_equal(out[k].view(np.uint32), augment.transform_maps(x, op).view(np.uint32)), (k, op)


@pytest.mark.parametrize("spec", SPECS, ids=str)
@pytest.mark.parametrize("B,S", SHAPES)
def test_reduce_equals_the_float64_definition(hip, B, S, spec):
    """The kernel adds n <= 8 fp32 terms in the order k = 0 .. n-1 and divides once: n - 1 additions whose partial sums are at most
    sum_k |term_k| in magnitude, and one division, each correctly rounded (relative error 2^-24).  Allowed deviation per cell from
    the float64 reference: (n + 1) 2^-24 (sum_k |term_k|) / count."""
    from nextbestpath_amd.utility import hipops
    ops, ops_dev = _ops(spec)
    n, V = len(ops), S // 4
    rng = np.random.default_rng(1000 + S + n)
    raw1 = rng.standard_normal((n, B, 8, V, V)).astype(np.float32)
    raw2 = rng.standard_normal((n, B, 1, S, S)).astype(np.float32)
    r1d, r2d = torch.from_numpy(raw1).to(D), torch.from_numpy(raw2).to(D)
    o1, o2 = hipops.symmetry_reduce(r1d, r2d, ops_dev)
    p1, p2 = hipops.symmetry_reduce(r1d, r2d, ops_dev, out=(torch.full_like(o1, -7.0), torch.full_like(o2, -7.0)))
    torch.cuda.synchronize()
    assert torch.equal(r1d.cpu(), torch.from_numpy(raw1)) and torch.equal(r2d.cpu(), torch.from_numpy(raw2))
    assert torch.equal(o1, p1) and torch.equal(o2, p2)                                          # deterministic, caller-owned outputs
    e1, e2 = augment.ensemble_reference(raw1, raw2, ops)
    a1, a2 = augment.ensemble_reference(np.abs(raw1), np.abs(raw2), ops)                        # (sum_k |term_k|) / count
    for name, got, want, mag in (("out1", o1, e1, a1), ("out2", o2, e2, a2)):
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == want.shape and np.isfinite(got).all()
        excess = np.abs(got - want) - (n + 1) * 2.0 ** -24 * mag
        regions = {"row 0": excess[..., 0, 1:], "column 0": excess[..., 1:, 0], "corner": excess[..., 0, 0],
                   "interior": excess[..., 1:, 1:]}
        for where, e in regions.items():
            print(f"{name} {where}: max |got - ref| - bound = {e.max():.3e}")
            assert e.max() <= 0.0, (name, where, float(e.max()))


def test_bad_arguments_launch_nothing(hip):
    from nextbestpath_amd import _lib
    from nextbestpath_amd.utility import hipops
    B, S, n = 2, 32, 4
    V = S // 4
    ops = _ops("flips")[1]
    x = torch.rand(B, 5, S, S, device=D)
    xo = torch.full((8, B, 5, S, S), -7.0, device=D)
    r1, r2 = torch.rand(8, B, 8, V, V, device=D), torch.rand(8, B, 1, S, S, device=D)
    o1, o2 = torch.full((B, 8, V, V), -7.0, device=D), torch.full((B, 1, S, S), -7.0, device=D)
    st, p = _lib.current_stream(), _lib.ptr
    ex, rd = hip.nbp_ensemble_expand_f32, hip.nbp_ensemble_reduce_f32
    assert ex(p(x), B, S, p(ops), 0, p(xo), st) == -1                      # n = 0
    assert ex(p(x), B, S, p(ops), 9, p(xo), st) == -1                      # n = 9
    assert ex(p(x), B, 24, p(ops), n, p(xo), st) == -3                     # S % 16
    assert ex(p(x), B, S, p(ops), n, p(x), st) == -1                       # in place
    assert ex(p(x), B, S, p(ops), n, p(xo) + 4, st) == -3                  # off the 16-byte grid
    assert ex(p(x), 0, S, p(ops), n, p(xo), st) == -1 and ex(0, B, S, p(ops), n, p(xo), st) == -1
    assert ex(p(x), B, S, 0, n, p(xo), st) == -1 and ex(p(x), B, S, p(ops), n, 0, st) == -1
    assert rd(p(r1), p(r2), B, S, p(ops), 0, p(o1), p(o2), st) == -1
    assert rd(p(r1), p(r2), B, S, p(ops), 9, p(o1), p(o2), st) == -1
    assert rd(p(r1), p(r2), B, 24, p(ops), n, p(o1), p(o2), st) == -3
    assert rd(p(r1), p(r2), B, S, p(ops), n, p(r1), p(o2), st) == -1       # in place
    assert rd(p(r1), p(r2), B, S, p(ops), n, p(o1), p(r2), st) == -1
    assert rd(p(r1), p(r2), B, S, p(ops), n, p(o1) + 4, p(o2), st) == -3   # off the 16-byte grid
    assert rd(p(r1) + 8, p(r2), B, S, p(ops), n, p(o1), p(o2), st) == -3
    assert rd(0, p(r2), B, S, p(ops), n, p(o1), p(o2), st) == -1 and rd(p(r1), p(r2), B, S, 0, n, p(o1), p(o2), st) == -1
    assert rd(p(r1), p(r2), 7282, S, p(ops), n, p(o1), p(o2), st) == -3    # 9 B planes > 65535: checked before anything is read
    torch.cuda.synchronize()
    assert bool((xo == -7.0).all()) and bool((o1 == -7.0).all()) and bool((o2 == -7.0).all())
    # the wrappers: device tensors only, dtypes and shapes as ValueError
    with pytest.raises(RuntimeError):
        hipops.symmetry_expand(x.cpu(), ops)
    with pytest.raises(RuntimeError):
        hipops.symmetry_reduce(r1[:4].contiguous(), r2[:4].contiguous(), ops.cpu())
    with pytest.raises(ValueError):
        hipops.symmetry_expand(x, ops.long())
    with pytest.raises(ValueError):
        hipops.symmetry_expand(x.double(), ops)
    with pytest.raises(ValueError):
        hipops.symmetry_expand(x[:, :4].contiguous(), ops)
    with pytest.raises(ValueError):
        hipops.symmetry_expand(x, ops, out=xo)                             # 8 members' room for a 4-member ensemble
    with pytest.raises(ValueError):
        hipops.symmetry_reduce(r1, r2, ops)                                # n = 8 planes, 4 op codes
    with pytest.raises(ValueError):
        hipops.symmetry_reduce(r1[:4].contiguous(), r2[:4, :, :, :16, :16].contiguous(), ops)
    with pytest.raises(ValueError):
        hipops.symmetry_ops((1, 0), D)


@pytest.fixture(scope="module")
def net(nbp_weights):
    from nextbestpath_amd.networks.nbp_model import NBP
    m = NBP()
    m.load_state_dict(nbp_weights, strict=True)
    m.conv_precision = "fp32"
    return m.cuda().eval()


def _maps(B, S, seed, zero_border=False):
    from nextbestpath_amd.utility.synthetic import make_count_maps
    x = make_count_maps(B, S, seed=seed)
    if zero_border:
        x[..., 0, :] = 0
        x[..., :, 0] = 0
    return x.contiguous()


def test_forward_paths_return_the_ensemble(hip, net):
    from nextbestpath_amd.utility import hipops
    B, S = 2, 32
    x = _maps(B, S, 3).cuda()
    ops, ops_dev = _ops("d4")
    try:
        with torch.no_grad():
            assert net.symmetry_ensemble is None
            plain = [t.clone() for t in net(x)]
            xe = hipops.symmetry_expand(x, ops_dev)
            r1, r2 = net(xe.view(8 * B, 5, S, S))                                  # the plain forward on the 16-map batch
            want = hipops.symmetry_reduce(r1.view(8, B, 8, S // 4, S // 4), r2.view(8, B, 1, S, S), ops_dev)
            net.symmetry_ensemble = "d4"
            got = [t.clone() for t in net(x)]
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            assert not torch.equal(got[0], plain[0])
            g = net.forward_static(x)
            assert torch.equal(g[0], got[0]) and torch.equal(g[1], got[1])
            x.copy_(_maps(B, S, 4).cuda())                                         # new content, same tensor: the replay reads it
            g = [t.clone() for t in net.forward_static(x)]
            e = net(x)
            assert torch.equal(g[0], e[0]) and torch.equal(g[1], e[1]) and not torch.equal(g[0], got[0])
            x.copy_(_maps(B, S, 3).cuda())
            net.symmetry_ensemble = None
            back = net(x)
            assert torch.equal(back[0], plain[0]) and torch.equal(back[1], plain[1])
            s = net.forward_static(x)
            assert torch.equal(s[0], plain[0]) and torch.equal(s[1], plain[1])
    finally:
        net.eval()
        net.symmetry_ensemble = None


def test_sliced_inner_batch(hip, net, monkeypatch):
    """16 moved maps through the plain forward in slices of 5, 5, 5 and 1 against one batch of 16.  The project allows a sample's
    outputs to differ between batch sizes (tests/test_gpu_network.py::test_forward_batch_consistency_and_determinism asserts 1e-5 at
    other sizes, not bit identity), so the comparison is the 1e-4 parity bar; the difference is printed."""
    from nextbestpath_amd.networks import packing
    B, S = 2, 32
    x = _maps(B, S, 5).cuda()
    try:
        net.symmetry_ensemble = "d4"
        with torch.no_grad():
            whole = [t.clone() for t in net(x)]
            monkeypatch.setattr(packing, "ENSEMBLE_MAX_INNER_BATCH", 5)
            assert packing._ensemble_layout(net.symmetry_ensemble, B, S, "fp32")[0] == 5
            sliced = [t.clone() for t in net(x)]
            again = net(x)
            assert torch.equal(again[0], sliced[0]) and torch.equal(again[1], sliced[1])
        d1, d2 = float((sliced[0] - whole[0]).abs().max()), float((sliced[1] - whole[1]).abs().max())
        print(f"sliced (5, 5, 5, 1) against one batch of 16: max |d out1| = {d1:.3e}, max |d out2| = {d2:.3e}")
        assert d1 < 1e-4 and d2 < 1e-4
    finally:
        net.symmetry_ensemble = None


def test_the_ensemble_is_equivariant_on_the_device(hip, net):
    """E(h x) against h E(x) on the interior cells, h the three generators, on an input with a zero border (there the transforms
    are an exact group action and the two sides are equal in exact arithmetic: tests/test_ensemble_host.py).  Each side is a mean of
    forwards that each meet the 1e-4 parity bar against exact arithmetic: 2e-4."""
    from nextbestpath_amd.networks import packing
    S = 32
    x = _maps(1, S, 7, zero_border=True).numpy()
    try:
        net.symmetry_ensemble = "d4"
        with torch.no_grad():
            e1, e2 = (t.cpu().numpy() for t in net(torch.from_numpy(x).cuda()))
            for h in (augment.TRANSPOSE, augment.REFLECT_ROWS, augment.REFLECT_COLS):
                h1, h2 = (t.cpu().numpy() for t in net(torch.from_numpy(augment.transform_maps(x, h)).cuda()))
                d1 = np.abs(h1 - augment.transform_value_map(e1, h))[..., 1:, 1:].max()
                d2 = np.abs(h2 - augment.transform_maps(e2, h))[..., 1:, 1:].max()
                print(f"h = {h}: max |E(h x) - h E(x)| = {d1:.3e} (out1), {d2:.3e} (out2)")
                assert d1 < 2e-4 and d2 < 2e-4, (h, d1, d2)
            # the diagnostic: the plain network (random weights) is far from equivariant, and the attribute comes back
            q1, q2 = packing.equivariance_error(net, torch.from_numpy(x).cuda(), "d4")
            print(f"equivariance_error of the plain network: {q1:.3e} (out1), {q2:.3e} (out2)")
            assert q1 > 1e-2 and np.isfinite(q1) and np.isfinite(q2) and q2 >= 0.0
            assert net.symmetry_ensemble == tuple(range(8)) and not net.training
    finally:
        net.symmetry_ensemble = None


def test_lockstep_planner_follows_the_attribute(hip, tmp_path):
    """One lock-step group of two rollouts with symmetry_ensemble = "c2": the group's batched forward (MultiRollout._forward) and the
    forward over the replanning subset with its caller-sized workspace both return what nbp(net_in) returns with the same attribute."""
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.simulator import scene as sc
    from nextbestpath_amd.simulator.mesh import make_maze_scene
    from nextbestpath_amd.testers import nbp_planning as tp
    from nextbestpath_amd.utility.synthetic import make_explorer_state_dict
    make_maze_scene(str(tmp_path / "maze_00"), seed=0, cells=8, size=4.8, height=1.2, tess=0.3)
    params = tp.load_params(os.path.join(ROOT, "configs/macarons/macarons_default_training_config.json"))
    ds = sc.SceneDataset(str(tmp_path))
    nbp = NBP()
    nbp.load_state_dict(make_explorer_state_dict(9))
    nbp = nbp.cuda().eval()
    with torch.no_grad():
        ros = [tp.build_rollout(params, nbp, ds, (0, 0), D, seed=60 + i) for i in range(2)]
        m = tp.MultiRollout(ros, nbp, D, n_groups=1, elide_dead_forward=True, symmetry_ensemble="c2")
        assert nbp.symmetry_ensemble == (0, 6) and len(m.groups) == 1
        seen, inner = [], m._forward

        def recording_forward(net_in):
            out1, out2 = inner(net_in)
            if not seen:
                seen.append((net_in.clone(), out1.clone(), out2.clone()))
            return out1, out2

        m._forward = recording_forward
        m.step()
        assert all(r.n_replans == 1 for r in ros) and len(seen) == 1          # the first step replans: the whole group's forward
        for _ in range(4):
            m.step()
        m.flush()
        torch.cuda.synchronize()
        assert m._packed is not None and m._packed.ensemble == (0, 6)
        net_in, out1, out2 = seen[0]
        d1, d2 = nbp(net_in)
        assert torch.equal(out1, d1) and torch.equal(out2, d2)
        nbp.symmetry_ensemble = None
        assert not torch.equal(nbp(net_in)[0], out1)                           # and it was the ensemble, not the plain forward
        nbp.symmetry_ensemble = "c2"
        # the subset forward: rollout 1 alone replans
        m._packed = nbp._ensure_packed(D)
        ros[0].need_replan, ros[1].need_replan = False, True
        s1, s2, rows = m._forward_replanning_only(0)
        assert rows == {1: 0} and s1.shape[0] == 1
        d1, d2 = nbp(m.net_in[0][1:2])
        assert torch.equal(s1, d1) and torch.equal(s2, d2)
        torch.cuda.synchronize()
    assert all(0.0 <= c <= 1.0 for r in ros for c in r.coverage_evolution(5))
