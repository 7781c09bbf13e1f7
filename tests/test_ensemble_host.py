"""Host: the definitions behind the D4 symmetry ensemble of the eval forward (utility/augment.py) -- the inverse elements found by
brute force, the action on dense value maps against the action on sparse targets, the named ensembles, the float64 definition
(ensemble_reference) on constant maps, and the equivariance of the definition itself with the float64 oracle network."""
import os

import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import augment
from nextbestpath_amd.utility.augment import (ENSEMBLES, check_ensemble, ensemble_reference, inverse_op, transform_maps,
                                               transform_value_map)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _zero_bordered_indices(n):
    a = np.arange(n * n, dtype=np.int64).reshape(n, n) + 1
    a[0, :] = 0
    a[:, 0] = 0
    return a


def _brute_force_inverse(g, n=6):
    """The one element h with h(g(a)) == a on an index array whose row 0 and column 0 are zero."""
    a = _zero_bordered_indices(n)
    found = [h for h in range(8) if np.array_equal(transform_maps(transform_maps(a, g), h), a)]
    assert len(found) == 1, (g, found)
    return found[0]


def test_inverse_op_is_the_brute_force_inverse():
    for g in range(8):
        a = _zero_bordered_indices(8)
        assert np.array_equal(transform_maps(transform_maps(a, g), inverse_op(g)), a), g
        assert inverse_op(g) == _brute_force_inverse(g), g
        assert inverse_op(inverse_op(g)) == g
    with pytest.raises(ValueError):
        inverse_op(8)


def test_named_ensembles_hold_the_identity_first_and_are_closed_under_inverse():
    assert set(ENSEMBLES) == {"c2", "flips", "d4"}
    assert ENSEMBLES["c2"] == (0, 6) and ENSEMBLES["flips"] == (0, 2, 4, 6) and ENSEMBLES["d4"] == tuple(range(8))
    for name, ops in ENSEMBLES.items():
        assert ops[0] == 0 and len(set(ops)) == len(ops)
        assert {_brute_force_inverse(g) for g in ops} == set(ops), name
        assert check_ensemble(name) == ops and check_ensemble(list(ops)) == ops


@pytest.mark.parametrize("V", [4, 8])
def test_value_maps_move_as_the_sparse_targets_do(V):
    for op in range(8):
        for h in range(8):
            for r in range(1, V):
                for c in range(1, V):
                    y = np.zeros((8, V, V))
                    y[h, r, c] = 1.0 + h + 10 * r + 100 * c
                    moved = transform_value_map(y, op)
                    px, gains = augment.transform_targets([[h, r, c]], [y[h, r, c]], op, V)
                    assert len(px) == 1                         # r, c >= 1: the target stays on the grid
                    where = np.argwhere(moved != 0)
                    assert where.tolist() == px.tolist(), (op, h, r, c)
                    assert moved[tuple(px[0])] == gains[0]
    y = np.random.default_rng(V).standard_normal((2, 3, 8, V, V))                    # leading axes ride along
    for op in range(8):
        m = transform_value_map(y, op)
        for h in range(8):
            assert np.array_equal(m[..., augment.heading_map(op)[h], :, :], transform_maps(y[..., h, :, :], op))


@pytest.mark.parametrize("name", ["c2", "flips", "d4"])
def test_ensemble_of_a_constant_map_is_that_constant_everywhere(name):
    n = len(ENSEMBLES[name])
    B, V, S = 2, 4, 16
    o1, o2 = ensemble_reference(np.full((n, B, 8, V, V), 1.75), np.full((n, B, 1, S, S), 0.375), name)
    assert o1.shape == (B, 8, V, V) and o2.shape == (B, 1, S, S) and o1.dtype == np.float64
    assert np.all(o1 == 1.75) and np.all(o2 == 0.375)                              # row 0, column 0 and the corner included
    assert np.all(o1[..., 0, :] == 1.75) and np.all(o1[..., :, 0] == 1.75) and np.all(o2[..., 0, 0] == 0.375)


def test_ensemble_reference_moves_each_member_back():
    """raw[k] = g_k y for one y with a zero border: every member moved back is y, so the ensemble is y."""
    rng = np.random.default_rng(0)
    V, S = 4, 16
    y1, y2 = rng.standard_normal((1, 8, V, V)), rng.standard_normal((1, 1, S, S))
    for y in (y1, y2):
        y[..., 0, :] = 0
        y[..., :, 0] = 0
    ops = (0, 3, 5, 1, 6)
    raw1 = np.stack([transform_value_map(y1, g) for g in ops])
    raw2 = np.stack([transform_maps(y2, g) for g in ops])
    o1, o2 = ensemble_reference(raw1, raw2, ops)
    assert np.abs(o1 - y1).max() < 1e-15 and np.abs(o2 - y2).max() < 1e-15


def test_check_ensemble():
    assert check_ensemble(None) is None
    assert check_ensemble("d4") == tuple(range(8))
    assert check_ensemble([0, 3, 5]) == (0, 3, 5) and check_ensemble(np.array([0, 6])) == (0, 6) and check_ensemble((0,)) == (0,)
    for bad in ((1, 0), (2,), (0, 2, 2), (0, 0), (0, 8), (0, -1), "d8", "", (), 3, (0, 1.5), (0, "1")):
        with pytest.raises(ValueError):
            check_ensemble(bad)


def test_module_attribute_goes_through_check_ensemble():
    from nextbestpath_amd.networks.nbp_model import NBP
    with torch.device("meta"):
        net = NBP()
    assert net.symmetry_ensemble is None
    net.symmetry_ensemble = "flips"
    assert net.symmetry_ensemble == (0, 2, 4, 6)
    net.symmetry_ensemble = [0, 5, 3]
    assert net.symmetry_ensemble == (0, 5, 3)
    with pytest.raises(ValueError):
        net.symmetry_ensemble = (3, 5)
    assert net.symmetry_ensemble == (0, 5, 3)
    net.symmetry_ensemble = None
    assert net.symmetry_ensemble is None


def test_the_definition_is_equivariant_in_float64():
    """E = the d4 ensemble of the float64 oracle network (oracle.nbp_net.nbp_forward, the weights of tests/golden/nbp_fwd_S32.npz),
    S = 32, B = 1.  On inputs whose row 0 and column 0 are zero the transforms are an exact group action, so E(h x) = h E(x) on the
    cells with row, col >= 1 for every h in D4, whatever the network is; the two sides differ by the order of float64 sums only:
    1e-12 relative to the largest magnitude."""
    from oracle import nbp_net
    from nextbestpath_amd.utility.synthetic import make_nbp_state_dict
    g = np.load(os.path.join(ROOT, "tests", "golden", "nbp_fwd_S32.npz"))
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in make_nbp_state_dict(int(g["weight_seed"])).items()}
    x = g["x"].astype(np.float64)
    assert x.shape == (1, 5, 32, 32)
    x[..., 0, :] = 0
    x[..., :, 0] = 0
    ops = ENSEMBLES["d4"]

    def E(y):
        raws = []
        with torch.no_grad():
            for k in ops:
                r1, r2 = nbp_net.nbp_forward(sd, torch.from_numpy(transform_maps(y, k)))
                raws.append((r1.numpy(), r2.numpy()))
        return ensemble_reference(np.stack([r[0] for r in raws]), np.stack([r[1] for r in raws]), ops)

    e1, e2 = E(x)
    assert np.abs(e1).max() > 0.1 and np.abs(e2).max() > 0.1
    for h in range(1, 8):
        h1, h2 = E(transform_maps(x, h))
        d1 = np.abs(h1 - transform_value_map(e1, h))[..., 1:, 1:].max()
        d2 = np.abs(h2 - transform_maps(e2, h))[..., 1:, 1:].max()
        assert d1 <= 1e-12 * np.abs(e1).max() and d2 <= 1e-12 * np.abs(e2).max(), (h, d1, d2)
    # and the plain network is NOT equivariant (random weights): the ensemble is what makes it so
    with torch.no_grad():
        p1, _ = nbp_net.nbp_forward(sd, torch.from_numpy(x))
        q1, _ = nbp_net.nbp_forward(sd, torch.from_numpy(transform_maps(x, 1)))
    assert np.abs(q1.numpy() - transform_value_map(p1.numpy(), 1))[..., 1:, 1:].max() > 1e-3


def test_the_test_config_key_reaches_the_driver(tmp_path):
    """The entry script hands test_nbp_planning the options it knows by keyword; `symmetry_ensemble` of a configs/test/ file (one
    with the NBP options) is kept by load_params for it, and a test config without the key clears it."""
    import json
    from nextbestpath_amd.testers import nbp_planning as tp
    with_key, without, other = tmp_path / "a.json", tmp_path / "b.json", tmp_path / "c.json"
    with_key.write_text(json.dumps({"_network": {"nbp_weights": "w.pth", "symmetry_ensemble": [0, 6]}}))
    without.write_text(json.dumps({"_network": {"nbp_weights": "w.pth"}}))
    other.write_text(json.dumps({"_rollout": {"image_height": 4}}))
    assert tp.load_params(str(with_key)).symmetry_ensemble == [0, 6] and tp._test_config["symmetry_ensemble"] == [0, 6]
    tp.load_params(str(other))                                   # not a test config: the record stays
    assert tp._test_config["symmetry_ensemble"] == [0, 6]
    assert not hasattr(tp.load_params(str(without)), "symmetry_ensemble") and tp._test_config["symmetry_ensemble"] is tp._UNSET
