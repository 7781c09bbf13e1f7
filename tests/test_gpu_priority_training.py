"""Loss-prioritised replay in the trainer (train_experience_data with replay_priority_alpha; utility/priority.py) on 24 synthetic
records at S = 32 with batches of 4: off means the trainer as it was, on means seeded draws, weights on the device, the fused
objective and a table updated from the optimizer step's read-back."""
import json
import os
import random
import types

import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import priority as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RECORDS, BS, S = 24, 4, 32
EARLY = (0, 5, 11)                                     # records of pose_i <= 10: not part of epoch 1


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _db():
    from nextbestpath_amd.trainers import train_nbp_model as T
    db = T.make_synthetic_experiences(N_RECORDS, S=S, seed=5)
    for i, d in enumerate(db):
        d["pose_i"] = 3 if i in EARLY else 20 + i
    return db


_RUNS = {}


def _train_run(tag, epoch=2, calls=1, spy=False, **opts):
    """`calls` inner epochs of train_experience_data from fixed seeds -> losses per call, the final state_dict, and with the option
    on the ReplayPriorities, its stats after every call and (spy) what every batch's objective saw."""
    if tag in _RUNS:
        return _RUNS[tag]
    from nextbestpath_amd.networks import training as tr
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.trainers import train_nbp_model as T
    D = _dev()
    params = types.SimpleNamespace(nbp_batch_size=BS, random_seed=8, **opts)
    db = _db()
    torch.manual_seed(3); random.seed(3); np.random.seed(3)
    net = NBP().to(D)
    _, opt, _, _ = T.initialize_nbp(params, net)
    net.train()
    pr = T.make_replay_priorities(params)
    kw = {} if pr is None else {"priorities": pr}
    seen = []
    real = tr.loss_weighted

    def spying(nbp, out1, bidx, coords, gains, out2, gt, weights=None):
        loss, per_sample = real(nbp, out1, bidx, coords, gains, out2, gt, weights)
        with torch.no_grad():
            plain = nbp.loss(tr.gather_values(out1.detach(), bidx, coords), gains, out2.detach(), gt)
        seen.append((weights.detach().clone(), loss.detach().clone(), plain.detach().clone()))
        return loss, per_sample

    losses, stats = [], []
    try:
        if spy:
            tr.loss_weighted = spying
        for _ in range(calls):
            losses.append(T.train_experience_data(list(db), params, opt, net, D, current_epoch=epoch, **kw))
            if pr is not None:
                stats.append((pr.stats(), pr.counts.copy(), list(pr.keys)))
    finally:
        tr.loss_weighted = real
    torch.cuda.synchronize()
    res = dict(losses=losses, state={k: t.detach().clone() for k, t in net.state_dict().items()}, priorities=pr, stats=stats,
               seen=[tuple(t.cpu() for t in s) for s in seen])
    _RUNS[tag] = res
    return res


def test_option_absent_and_null_are_the_same_run(hip):
    a = _train_run("absent")
    b = _train_run("null", replay_priority_alpha=None, replay_priority_beta=0.9, replay_priority_eps=0.5)
    assert a["priorities"] is None and b["priorities"] is None
    assert len(a["losses"][0]) == 1 and np.isfinite(a["losses"][0]).all()             # 6 batches: one optimizer step
    assert a["losses"] == b["losses"]
    assert all(torch.equal(a["state"][k], b["state"][k]) for k in a["state"])


def test_same_seeds_same_run(hip):
    a = _train_run("p06_a", epoch=1, calls=2, replay_priority_alpha=0.6)
    b = _train_run("p06_b", epoch=1, calls=2, replay_priority_alpha=0.6)
    assert a["losses"] == b["losses"] and len(a["losses"]) == 2 and np.isfinite(a["losses"]).all()
    assert a["priorities"].table == b["priorities"].table and a["priorities"].table
    assert all(torch.equal(a["state"][k], b["state"][k]) for k in a["state"])
    assert all(np.array_equal(x[1], y[1]) for x, y in zip(a["stats"], b["stats"]))
    c = _train_run("p06_c", epoch=1, calls=2, replay_priority_alpha=0.6, replay_priority_seed=1234)
    assert any(not np.array_equal(x[1], y[1]) for x, y in zip(a["stats"], c["stats"]))   # the seed option reaches the draws


def test_draws_table_and_stats(hip):
    r = _train_run("p06_a", epoch=1, calls=2, replay_priority_alpha=0.6)
    pr = r["priorities"]
    N = N_RECORDS - len(EARLY)
    drawn = set()
    for st, counts, keys in r["stats"]:
        # epoch 1: the early poses are not in the population; without store keys a record's key is its position in the list
        assert keys == [i for i in range(N_RECORDS) if i not in EARLY]
        assert counts.sum() == N == st["draws"] == st["n"]                            # an inner epoch still trains on N samples
        assert set(st) == {"n", "effective_sample_size", "loss_min", "loss_mean", "loss_max", "min_weight", "draws",
                           "distinct_fraction"}
        assert 0.0 < st["effective_sample_size"] <= 1.0 and 0.0 < st["min_weight"] <= 1.0
        assert st["distinct_fraction"] == (counts > 0).sum() / N
        assert 0.0 < st["loss_min"] <= st["loss_mean"] <= st["loss_max"]
        drawn |= {k for k, c in zip(keys, counts) if c}
    assert drawn and drawn == set(pr.table)                                           # exactly the records drawn have an entry,
    assert all(np.isfinite(v) and v > 0.0 and v != 1.0 for v in pr.table.values())    # and none keeps the initial 1.0
    assert not set(pr.table) & set(EARLY)
    assert pr.max_seen == max(pr.table.values()) or pr.max_seen > max(pr.table.values())
    json.dumps(r["stats"][-1][0])                                                     # what loss.json receives


def test_alpha_zero_is_the_unweighted_objective(hip):
    r = _train_run("p0", spy=True, replay_priority_alpha=0.0, replay_priority_beta=1.0)
    assert len(r["seen"]) == N_RECORDS // BS
    worst = 0.0
    for w, fused, plain in r["seen"]:
        assert w.dtype == torch.float32 and w.shape == (BS,) and bool((w == 1.0).all())
        worst = max(worst, abs(fused.item() - plain.item()) / abs(plain.item()))
    print("fused against nbp.loss, worst relative difference:", worst)
    assert worst <= 1e-6
    assert r["losses"][0] == [sum(f.item() for _, f, _ in r["seen"]) / 8]             # the loss list: the window's sum over 8, as ever
    assert r["stats"][0][0]["effective_sample_size"] == pytest.approx(1.0, rel=1e-12)


def test_weights_below_one_reach_the_device(hip):
    """Second inner epoch at alpha 0.6: the table holds different losses, so some weight is below 1 and the loss is the weighted one."""
    r = _train_run("p06_spy", calls=2, spy=True, replay_priority_alpha=0.6, replay_priority_beta=1.0)
    first, second = r["seen"][:6], r["seen"][6:]
    assert all(bool((w == 1.0).all()) for w, _, _ in first)                           # nothing trained on yet: all priorities equal
    assert any(bool((w < 1.0).any()) for w, _, _ in second) and all(bool(((w > 0) & (w <= 1)).all()) for w, _, _ in second)
    assert any(abs(f.item() - p.item()) > 1e-4 * abs(p.item()) for w, f, p in second if bool((w < 1.0).any()))


def test_backward_of_the_objective_does_not_wait_for_the_host(hip):
    from nextbestpath_amd.networks import training as tr
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.trainers import train_nbp_model as T
    D = _dev()
    torch.manual_seed(3)
    net = NBP().to(D).train()
    xs, gt, coords, gains, bidx = T._collate(_db()[:2], D)
    w = torch.tensor([1.0, 0.5], device=D)

    def step(guard):
        out1, out2 = net(xs)
        loss, _ = tr.loss_weighted(net, out1, bidx, coords, gains, out2, gt, w)
        torch.cuda.synchronize()
        if guard:
            torch.cuda.set_sync_debug_mode("error")
        try:
            loss.backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        net.zero_grad()

    step(False)                                        # warm: every workspace and cached pack exists
    # the mode is live in this build: a read-back raises under it
    probe = torch.ones(1, device=D)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    step(True)
    torch.cuda.synchronize()


def _train(tmp_path, name, extra):
    from nextbestpath_amd.testers.nbp_planning import load_params
    from nextbestpath_amd.trainers import train_nbp_model as T
    cfg = json.load(open(os.path.join(ROOT, "configs/nbp/nbp_default_training_config.json")))
    out = tmp_path / name
    cfg["_nbp"].update({"nbp_model_name": "nbp_p", "nbp_batch_size": 2, "grid_size": S, "epochs": 1, "inner_epochs": 2,
                        "samples_per_epoch": 6, "n_validation_synthetic": 2, "output_dir": str(out), "collect": False})
    for k in [k for k in cfg["_nbp"] if k.startswith("replay_priority_")]:
        cfg["_nbp"].pop(k)
    cfg["_nbp"].update(extra)
    path = tmp_path / f"{name}.json"
    path.write_text(json.dumps(cfg))
    T.run_training_nbp(load_params(str(path)))
    return json.load(open(out / "loss.json"))


def test_loss_json_gains_the_key_only_with_the_option_on(hip, tmp_path):
    off = _train(tmp_path, "off", {})
    assert set(off["1"]) == {"training_loss", "validation_loss"}
    null = _train(tmp_path, "null", {"replay_priority_alpha": None})
    assert null == off
    on = _train(tmp_path, "on", {"replay_priority_alpha": 0.6, "replay_priority_beta": 0.5})
    assert set(on["1"]) == {"training_loss", "validation_loss", "replay_priority"}
    rp = on["1"]["replay_priority"]
    assert rp["alpha"] == 0.6 and rp["beta"] == 0.5 and rp["draws"] == rp["n"] and 0.0 < rp["effective_sample_size"] <= 1.0
    assert {"loss_min", "loss_mean", "loss_max", "min_weight", "distinct_fraction"} <= set(rp)
    with pytest.raises(ValueError):
        _train(tmp_path, "bad", {"replay_priority_alpha": 0.6, "replay_priority_eps": 0})
    assert not (tmp_path / "bad").exists()             # refused before any work
