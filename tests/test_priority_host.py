"""nextbestpath_amd/utility/priority.py on the host: the draws and weights of ReplayPriorities, the option checks, and
objective_reference against torch's mse_loss / binary_cross_entropy and their autograd gradients (CPU tensors, float64)."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nextbestpath_amd.utility import priority as P


def test_alpha_zero_is_uniform_with_unit_weights():
    pr = P.ReplayPriorities(alpha=0.0, beta=0.7)
    keys = list(range(7))
    pr.update(keys[:4], [0.1, 5.0, 0.0, 2.5])
    assert np.array_equal(pr.probabilities(keys), np.full(7, 1 / 7))
    assert np.array_equal(pr.weights(keys), np.ones(7))
    pr.begin(keys)
    idx, w = pr.draw(np.random.default_rng(0), 50)
    assert np.array_equal(w, np.ones(50)) and idx.min() >= 0 and idx.max() < 7
    assert pr.stats()["effective_sample_size"] == pytest.approx(1.0, rel=1e-15)


def test_draw_frequencies_follow_the_probabilities():
    eps = 1e-3
    pr = P.ReplayPriorities(alpha=1.0, beta=0.4, eps=eps)
    keys = ["a", "b", "c", "d"]
    pr.update(keys, np.array([1.0, 2.0, 3.0, 4.0]) - eps)
    prob = pr.probabilities(keys)
    assert np.allclose(prob, np.array([0.1, 0.2, 0.3, 0.4]), rtol=1e-14, atol=0)
    pr.begin(keys)
    n = 40000
    idx, _ = pr.draw(np.random.default_rng(12345), n)
    freq = np.bincount(idx, minlength=4) / n
    bound = 5 * np.sqrt(prob * (1 - prob) / n)
    print("frequencies", freq, "bound", bound)
    assert np.all(np.abs(freq - prob) <= bound)
    st = pr.stats()
    assert st["draws"] == n and st["distinct_fraction"] == 1.0


def test_weights_equal_the_closed_form():
    pr = P.ReplayPriorities(alpha=0.6, beta=0.4, eps=1e-3)
    keys = list(range(5))
    l = np.array([0.2, 1.5, 0.01, 3.0, 0.7])
    pr.update(keys, l)
    q = (l + 1e-3) ** 0.6
    prob = q / q.sum()
    w = (5 * prob) ** -0.4
    w /= w.max()
    assert np.allclose(pr.probabilities(keys), prob, rtol=1e-14, atol=0)
    assert np.allclose(pr.weights(keys), w, rtol=1e-14, atol=0)
    assert pr.weights(keys).max() == 1.0 and np.argmax(pr.weights(keys)) == 2          # the least likely record
    pr.begin(keys)
    idx, got = pr.draw(np.random.default_rng(3), 64)
    assert np.allclose(got, w[idx], rtol=1e-14, atol=0) and got.max() <= 1.0
    st = pr.stats()
    assert st["min_weight"] == got.min() and st["loss_max"] == 3.0 and st["loss_min"] == 0.01
    assert st["loss_mean"] == pytest.approx(l.mean(), rel=1e-15)
    assert st["effective_sample_size"] == pytest.approx(q.sum() ** 2 / (5 * (q * q).sum()), rel=1e-14)
    assert st["distinct_fraction"] == len(set(idx.tolist())) / 5


def test_an_unseen_record_gets_the_largest_loss_seen():
    pr = P.ReplayPriorities(alpha=0.6)
    assert np.array_equal(pr.losses(["x", "y"]), [1.0, 1.0])                          # before any has been seen
    pr.update(["x"], [0.25])
    assert np.array_equal(pr.losses(["x", "y"]), [0.25, 0.25])
    pr.update(["z", "x"], [7.5, 0.125])
    assert np.array_equal(pr.losses(["x", "y", "z"]), [0.125, 7.5, 7.5])              # the largest ever seen, not the largest kept
    pr.update(["z"], [0.5])
    assert np.array_equal(pr.losses(["x", "y", "z"]), [0.125, 7.5, 0.5])


def test_update_then_probabilities_round_trips():
    pr = P.ReplayPriorities(alpha=0.5, eps=0.01)
    keys = [b"k0", b"k1", 2]
    l = np.array([0.3, 0.0, 2.0])
    pr.update(keys, l)
    assert np.array_equal(pr.losses(keys), l)
    q = np.sqrt(l + 0.01)
    assert np.allclose(pr.probabilities(keys), q / q.sum(), rtol=1e-15, atol=0)
    assert np.allclose(pr.probabilities(keys, alpha=1.0, eps=1.0), (l + 1) / (l + 1).sum(), rtol=1e-15, atol=0)
    pr.update([b"k1", b"k1"], [4.0, 5.0])                                             # a key named twice keeps the last
    assert pr.table[b"k1"] == 5.0


def test_the_same_seed_gives_the_same_draws():
    def run(seed):
        pr = P.ReplayPriorities(alpha=0.6)
        keys = list(range(100))
        pr.update(keys, np.linspace(0.0, 3.0, 100))
        pr.begin(keys)
        rng = np.random.default_rng(seed)
        return [pr.draw(rng, 16) for _ in range(4)]
    a, b, c = run(9), run(9), run(10)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    assert any(not np.array_equal(x[0], y[0]) for x, y in zip(a, c))


def test_options_are_validated():
    assert P.check_options(None, beta="nonsense") is None                              # off: nothing else is looked at
    assert P.check_options(0.6) == {"alpha": 0.6, "beta": 0.4, "eps": 1e-3, "seed": None}
    assert P.check_options(0, 1, 0.5, 7) == {"alpha": 0.0, "beta": 1.0, "eps": 0.5, "seed": 7}
    for bad in (dict(alpha=-0.1), dict(alpha="0.6"), dict(alpha=True), dict(alpha=float("nan")), dict(alpha=0.6, beta=1.5),
                dict(alpha=0.6, beta=-0.1), dict(alpha=0.6, beta=None), dict(alpha=0.6, eps=0), dict(alpha=0.6, eps=-1),
                dict(alpha=0.6, eps=float("inf")), dict(alpha=0.6, seed=-1), dict(alpha=0.6, seed=1.5)):
        with pytest.raises(ValueError):
            P.check_options(**bad)
    with pytest.raises(ValueError):
        P.ReplayPriorities(alpha=None)
    from nextbestpath_amd.trainers import train_nbp_model as T
    assert T.replay_priority_options(types.SimpleNamespace()) is None
    assert T.replay_priority_options(types.SimpleNamespace(replay_priority_alpha=None)) is None
    assert T.make_replay_priorities(types.SimpleNamespace()) is None
    got = T.replay_priority_options(types.SimpleNamespace(replay_priority_alpha=0.6, replay_priority_seed=3))
    assert got == {"alpha": 0.6, "beta": 0.4, "eps": 1e-3, "seed": 3}
    with pytest.raises(ValueError):
        T.replay_priority_options(types.SimpleNamespace(replay_priority_alpha=0.6, replay_priority_beta=2))
    with pytest.raises(ValueError):        # before any work: no device, no optimizer, no network is touched
        T.train_experience_data([], types.SimpleNamespace(replay_priority_alpha=-1, nbp_batch_size=4), None, None, "cpu", 2)


def test_default_config_has_the_options_off():
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = json.load(open(os.path.join(root, "configs/nbp/nbp_default_training_config.json")))["_nbp"]
    assert cfg["replay_priority_alpha"] is None and cfg["replay_priority_beta"] == 0.4
    assert cfg["replay_priority_eps"] == 1e-3 and cfg["replay_priority_seed"] is None


def _batch(seed, B=3, S=8, C=8, K=17):
    rng = np.random.default_rng(seed)
    V = S // 4
    out1 = rng.normal(size=(B, C, V, V)).astype(np.float32)
    out2 = rng.uniform(0.02, 0.98, size=(B, 1, S, S)).astype(np.float32)
    gt = (rng.random((B, 1, S, S)) < 0.3).astype(np.float32)
    coords = np.stack([rng.integers(0, B, K), rng.integers(0, C, K), rng.integers(0, V, K), rng.integers(0, V, K)], 1)
    coords[1] = coords[0]                                                              # a cell named twice
    gains = rng.uniform(0, 5, K).astype(np.float32)
    return out1, coords.astype(np.int64), gains, out2, gt


def test_objective_reference_is_torch_mse_and_bce():
    out1, coords, gains, out2, gt = _batch(4)
    coef = (0.37, 1.9)
    ref = P.objective_reference(out1, coords, gains, out2, gt, None, coef)
    o1 = torch.from_numpy(out1).double().requires_grad_(True)
    o2 = torch.from_numpy(out2).double().requires_grad_(True)
    c = torch.from_numpy(coords)
    mse = F.mse_loss(o1[c[:, 0], c[:, 1], c[:, 2], c[:, 3]], torch.from_numpy(gains).double())
    bce = F.binary_cross_entropy(o2, torch.from_numpy(gt).double())
    (coef[0] * mse + coef[1] * bce).backward()
    assert ref["mse"] == pytest.approx(mse.item(), rel=1e-12)
    assert ref["bce"] == pytest.approx(bce.item(), rel=1e-12)
    assert np.allclose(ref["d_out1"], o1.grad.numpy(), rtol=1e-12, atol=0)
    assert np.allclose(ref["d_out2"], o2.grad.numpy(), rtol=1e-12, atol=0)
    assert ref["per_sample"][:, 1].sum() == len(gains)
    assert ref["totals"][0] == pytest.approx(ref["per_sample"][:, 0].sum(), rel=1e-15)


def test_objective_reference_weights_clamps_and_bad_rows():
    out1, coords, gains, out2, gt = _batch(5)
    B = out1.shape[0]
    w = np.array([0.0, 0.5, 1.0])
    plain = P.objective_reference(out1, coords, gains, out2, gt)
    ref = P.objective_reference(out1, coords, gains, out2, gt, w)
    assert np.array_equal(ref["per_sample"], plain["per_sample"])                      # the weights enter the totals only
    assert ref["totals"][1] == pytest.approx((w * plain["per_sample"][:, 2]).sum(), rel=1e-15)
    for b in range(B):
        assert np.allclose(ref["d_out2"][b], w[b] * plain["d_out2"][b], rtol=1e-15, atol=0)
        assert np.allclose(ref["d_out1"][b], w[b] * plain["d_out1"][b], rtol=1e-15, atol=0)
    # a row out of range contributes nothing, but K stays the number of rows
    bad = coords.copy()
    bad[3, 2] = out1.shape[2]
    r2 = P.objective_reference(out1, bad, gains, out2, gt)
    keep = np.arange(len(gains)) != 3
    r3 = P.objective_reference(out1, coords[keep], gains[keep], out2, gt)
    assert np.allclose(r2["per_sample"], r3["per_sample"], rtol=1e-15, atol=0)
    assert r2["mse"] == pytest.approx(r3["mse"] * (len(gains) - 1) / len(gains), rel=1e-14)
    # exact 0 and 1 in out2: log clamped at -100, the gradient's denominator floored at 1e-12
    p = np.array([[[[0.0, 1.0], [0.0, 1.0]]]], np.float32)
    t = np.array([[[[0.0, 1.0], [1.0, 0.0]]]], np.float32)
    r = P.objective_reference(np.zeros((1, 1, 1, 1), np.float32), np.zeros((0, 4), np.int64), np.zeros(0, np.float32), p, t)
    assert r["per_sample"].tolist() == [[0.0, 0.0, 200.0]] and r["mse"] == 0.0 and r["bce"] == 50.0
    assert np.array_equal(r["d_out2"], np.array([[[[0.0, 0.0], [-1e12 / 4, 1e12 / 4]]]]))
    bce = F.binary_cross_entropy(torch.from_numpy(p).double(), torch.from_numpy(t).double())
    assert r["bce"] == bce.item()


def test_sample_loss_is_the_samples_share_of_the_loss():
    out1, coords, gains, out2, gt = _batch(6, B=1, K=9)
    coords[:, 0] = 0
    ref = P.objective_reference(out1, coords, gains, out2, gt)
    s = np.array([0.3, -0.2])
    l = P.sample_loss(ref["per_sample"], out2.shape[-1], s)
    want = ref["mse"] / (2 * np.exp(2 * s[0])) + ref["bce"] / np.exp(2 * s[1])       # B = 1: the batch's loss without s0 + s1
    assert l.shape == (1,) and l[0] == pytest.approx(want, rel=1e-14)
    assert P.sample_loss(np.array([[0.0, 0.0, 32.0]]), 4, (0.0, 0.0))[0] == 2.0      # no targets: max(n, 1)


def test_read_combined_data_with_keys(tmp_path):
    """with_keys=True: the same records in the same order, each with its store key; the default leaves the records as they are."""
    import random
    from nextbestpath_amd.utility import nbp_utils as nu
    env = nu.LogEnv(str(tmp_path / "db"))
    rng = np.random.default_rng(0)
    for i in range(12):
        nu.store_experience(env, {"current_model_input": torch.from_numpy(rng.random((1, 5, 8, 8)).astype(np.float32)),
                                  "current_gt_2d_layout": torch.from_numpy((rng.random((1, 1, 8, 8)) < 0.2).astype(np.float32)),
                                  "target_value_map_pixel": np.array([[1, 0, 1]]), "actual_coverage_gain": np.ones(1, np.float32),
                                  "pose_i": i})
    keys = env.keys()
    for kw in (dict(sample_m=None), dict(sample_m=4, sample_size=3)):
        random.seed(0)
        plain = nu.read_combined_data(env, **kw)
        random.seed(0)
        keyed = nu.read_combined_data(env, with_keys=True, **kw)
        assert all("_key" not in d for d in plain)
        assert [d["pose_i"] for d in keyed] == [d["pose_i"] for d in plain]
        assert [d["_key"] for d in keyed] == [keys[d["pose_i"]] for d in keyed] and all(isinstance(d["_key"], bytes) for d in keyed)
        assert all(set(k) - {"_key"} == set(p) for k, p in zip(keyed, plain))
    # the keys are what the table files a record's loss under
    pr = P.ReplayPriorities(0.6)
    pr.update([d["_key"] for d in keyed[:2]], [0.5, 2.0])
    assert pr.losses([keyed[1]["_key"], keyed[0]["_key"], b"other"]).tolist() == [2.0, 0.5, 2.0]
