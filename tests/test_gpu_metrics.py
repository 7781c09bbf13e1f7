"""hipops.validation_metrics (csrc/nbp_metrics.hip) against the numpy definition (nextbestpath_amd/utility/metrics.py), and the
trainer's wiring of it.

Equality: obst, rank and val[:, 2:] exactly; val[:, :2] within 1e-12 relative -- float64 sums of at most a few hundred terms (2100
in the one case that leaves LDS) in another order, so the difference is at most a few thousand x 2^-53 = a few 1e-13."""
import json
import os

import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import hipops
from nextbestpath_amd.utility import metrics as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY_KEYS = {"n_samples", "n_targets", "n_bad_targets", "value_mae", "value_rmse", "rank_accuracy", "top1_hit_rate", "mean_regret",
                "obstacle"}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _case(seed, B, S, counts, bad=0, nan1=0, nan2=0):
    """A batch as validation_model has it: bidx shuffled, duplicate cells, gains with ties and zeros (d * 100 if d > 0 else 0)."""
    rng = np.random.default_rng(seed)
    V = S // 4
    out1 = rng.choice(np.linspace(-1, 3, 33), size=(B, 8, V, V)).astype(np.float32)          # few distinct values: ties in p
    out2 = rng.random((B, 1, S, S)).astype(np.float32)
    gt = (rng.random((B, 1, S, S)) < 0.3).astype(np.float32)
    K = int(sum(counts))
    bidx = np.repeat(np.arange(B), counts).astype(np.int64)
    coords = np.stack([rng.integers(0, 8, K), rng.integers(0, V, K), rng.integers(0, V, K)], 1).astype(np.int64)
    d = rng.integers(-2, 6, K)
    gains = np.where(d > 0, d * 100, 0).astype(np.float32)
    for k in range(0, K - 1, 7):
        coords[k + 1] = coords[k]                                                            # duplicate cells
    for k in rng.choice(K, size=min(bad, K), replace=False):
        coords[k, rng.integers(0, 3)] = rng.choice([-1, 8 if V <= 8 else V, -2 ** 40, 2 ** 40, 2 ** 31])
    for _ in range(nan1):
        out1[rng.integers(0, B), rng.integers(0, 8), rng.integers(0, V), rng.integers(0, V)] = np.nan
    for _ in range(nan2):
        out2[rng.integers(0, B), 0, rng.integers(0, S), rng.integers(0, S)] = np.nan
    perm = rng.permutation(K)
    return out1, out2, gt, coords[perm], gains[perm], bidx[perm]


def _gpu(case, thresholds):
    dev = _dev()
    got = hipops.validation_metrics(*(torch.from_numpy(a).to(dev) for a in case), thresholds)
    assert [t.dtype for t in got] == [torch.int64, torch.int64, torch.float64] and all(t.is_cuda for t in got)
    return tuple(t.cpu().numpy() for t in got)


def _check(got, want):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[2].shape == want[2].shape
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(got[2][:, 2:], want[2][:, 2:])
    a, b = got[2][:, :2], want[2][:, :2]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    rel = float((np.abs(a[ok] - b[ok]) / np.where(b[ok] != 0, np.abs(b[ok]), 1.0)).max()) if ok.any() else 0.0
    print(f"val[:, :2]: worst relative difference {rel:.2e}")
    assert rel <= 1e-12, rel


def _thresholds(T, out2):
    """0.0 and 1.0 and a value present in out2 among them once T allows."""
    return ([0.13], [0.13, float(out2[0, 0, 3, 5])], None, None, None, None, None,
            [0.13, 0.0, 1.0, float(out2[0, 0, 3, 5]), 0.5, 0.25, 0.75, -1.0])[T - 1]


# (B, S, T, per-sample target counts): less than one workgroup of pixels; odd batch with the full threshold list; two workgroups'
# worth of pixels per sample.  The counts straddle the wave (64) and the workgroup (256) sizes.
SHAPES = [(1, 16, 1, [65]), (1, 16, 1, [0]), (3, 32, 8, [300, 0, 1]), (3, 32, 8, [2, 63, 64]), (2, 64, 2, [65, 300]), (2, 64, 2, [1, 2])]


@pytest.mark.parametrize("B,S,T,counts", SHAPES)
def test_kernel_matches_the_definition(hip, B, S, T, counts):
    case = _case(100 + B + S + sum(counts), B, S, counts)
    ts = _thresholds(T, case[1])
    if T > 1:
        assert np.any(case[1] == np.float32(ts[1 if T == 2 else 3]))
    _check(_gpu(case, ts), M.validation_metrics_reference(*case, ts))


def test_more_targets_than_the_kernel_holds_in_lds(hip):
    """2100 good targets in one sample (the kernel keeps up to 2048 pairs (p, g) in LDS and reads the raw lists beyond that),
    beside a sample that stays inside."""
    case = _case(7, 2, 32, [2100, 40], bad=5)
    _check(_gpu(case, [0.13]), M.validation_metrics_reference(*case, [0.13]))


def test_bad_coordinates_are_rejected_by_the_range_test(hip):
    """Indices outside the value map (valid memory, wrong numbers): counted, never dereferenced."""
    case = _case(8, 3, 32, [64, 65, 2], bad=40)
    want = M.validation_metrics_reference(*case, [0.13, 0.5])
    assert want[1][:, 1].sum() >= 30
    _check(_gpu(case, [0.13, 0.5]), want)


def test_nans_in_the_outputs(hip):
    case = _case(9, 2, 32, [63, 300], nan1=600, nan2=500)
    want = M.validation_metrics_reference(*case, [0.13, 0.0])
    assert np.isnan(want[2][:, 0]).all() and np.isnan(case[1]).sum() > 400
    _check(_gpu(case, [0.13, 0.0]), want)
    # a sample whose every value is NaN: pred_best is its first good target
    case[0][1] = np.nan
    want = M.validation_metrics_reference(*case, [0.13])
    assert want[1][1, 3] == 0 and want[1][1, 4] == 0 and want[1][1, 2] > 0
    _check(_gpu(case, [0.13]), want)


def test_no_targets_at_all(hip):
    out1, out2, gt, coords, gains, bidx = _case(10, 2, 16, [0, 0])
    assert coords.shape == (0, 3)
    got = _gpu((out1, out2, gt, coords, gains, bidx), [0.13])
    _check(got, M.validation_metrics_reference(out1, out2, gt, coords, gains, bidx, [0.13]))
    assert not got[1].any() and not got[2].any() and got[0].sum() == 2 * 16 * 16


def test_two_runs_give_the_same_bits(hip):
    case = _case(11, 3, 64, [300, 65, 1], bad=3)
    dev = _dev()
    args = [torch.from_numpy(a).to(dev) for a in case]
    a = hipops.validation_metrics(*args, [0.13, 0.5])
    b = hipops.validation_metrics(*args, [0.13, 0.5])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int64), b[2].view(torch.int64))


def test_the_call_does_not_synchronise(hip):
    dev = _dev()
    args = [torch.from_numpy(a).to(dev) for a in _case(12, 2, 32, [5, 9])]
    hipops.validation_metrics(*args)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = hipops.validation_metrics(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(got[1][:, 0].sum()) == 14


def test_argument_checking(hip):
    dev = _dev()
    case = _case(13, 2, 16, [3, 4])
    out1, out2, gt, coords, gains, bidx = (torch.from_numpy(a).to(dev) for a in case)
    with pytest.raises(RuntimeError):
        hipops.validation_metrics(out1.cpu(), out2, gt, coords, gains, bidx)
    with pytest.raises(RuntimeError):
        hipops.validation_metrics(out1, out2, gt, coords, gains, bidx.cpu())
    with pytest.raises(ValueError):
        hipops.validation_metrics(out1, out2.double(), gt, coords, gains, bidx)
    with pytest.raises(ValueError):
        hipops.validation_metrics(out1, out2, gt, coords.int(), gains, bidx)
    with pytest.raises(ValueError):
        hipops.validation_metrics(out1, out2, gt, coords, gains, bidx.int())
    with pytest.raises(ValueError):
        hipops.validation_metrics(out1[:, :7], out2, gt, coords, gains, bidx)
    with pytest.raises(ValueError):
        hipops.validation_metrics(out1, out2, gt[:1], coords, gains, bidx)
    with pytest.raises(ValueError):
        hipops.validation_metrics(out1, out2, gt, coords[:, :2], gains, bidx)
    with pytest.raises(ValueError):
        hipops.validation_metrics(out1, out2, gt, coords, gains[:-1], bidx)
    with pytest.raises(ValueError):
        hipops.validation_metrics(out1, out2, gt, coords, gains, bidx, thresholds=[0.1] * 9)
    with pytest.raises(ValueError):
        hipops.validation_metrics(out1, out2, gt, coords, gains, bidx, thresholds=[])


# ---- the trainer
@pytest.fixture(scope="module")
def net(nbp_weights):
    from nextbestpath_amd.networks.nbp_model import NBP
    nbp = NBP()
    nbp.load_state_dict(nbp_weights, strict=True)
    return nbp.to(_dev()).eval()


def test_validation_model_with_metrics(hip, net):
    """Three synthetic validation records at S = 64 in batches of two: the same loss float with and without the accumulator, one
    read-back, and the summary of the definition applied to nbp(xs) of the same batches."""
    import types
    from nextbestpath_amd.trainers import train_nbp_model as T
    dev = _dev()
    db = T.make_synthetic_experiences(3, 64, seed=5)
    params = types.SimpleNamespace(nbp_batch_size=2)
    ts = (0.13, 0.5)
    with torch.no_grad():
        plain = T.validation_model(db, params, net, dev)
        acc = T.ValidationMetrics(ts)
        with_metrics = T.validation_model(db, params, net, dev, metrics=acc)
        assert isinstance(plain, float) and plain == with_metrics
        assert not acc._pending and acc.totals[0] == 3
        tot = np.zeros(M.totals_size(2))
        for i in (0, 2):
            xs, gt, coords, gains, bidx = T._collate(db[i:i + 2], dev)
            out1, out2 = net(xs)
            tot += M.totals(*M.validation_metrics_reference(*(t.cpu().numpy() for t in (out1, out2, gt, coords, gains, bidx)), ts))
    got, want = acc.summary(dev), M.summarize_totals(tot, ts)
    assert set(got) == SUMMARY_KEYS and got["n_samples"] == 3 and got["n_targets"] == sum(len(d["actual_coverage_gain"]) for d in db)
    for k in ("value_mae", "value_rmse", "mean_regret"):
        assert got.pop(k) == pytest.approx(want.pop(k), rel=1e-12)
    assert got == want
    assert T.metric_thresholds(types.SimpleNamespace()) is None
    assert T.metric_thresholds(types.SimpleNamespace(validation_metrics=True)) == (0.13,)
    assert T.metric_thresholds(types.SimpleNamespace(validation_metrics=True, metric_thresholds=[0.2, 0.4])) == (0.2, 0.4)


def _train(tmp_path, name, extra):
    from nextbestpath_amd.testers.nbp_planning import load_params
    from nextbestpath_amd.trainers import train_nbp_model as T
    cfg = json.load(open(os.path.join(ROOT, "configs/nbp/nbp_default_training_config.json")))
    out = tmp_path / name
    cfg["_nbp"].update({"nbp_model_name": "nbp_m", "nbp_batch_size": 2, "grid_size": 64, "epochs": 1, "inner_epochs": 2,
                        "samples_per_epoch": 8, "n_validation_synthetic": 3, "output_dir": str(out), "collect": False})
    for k in ("validation_metrics", "metric_thresholds"):
        cfg["_nbp"].pop(k)
    cfg["_nbp"].update(extra)
    path = tmp_path / f"{name}.json"
    path.write_text(json.dumps(cfg))
    T.run_training_nbp(load_params(str(path)))
    return out, json.load(open(out / "loss.json")), torch.load(out / "nbp_m_best_val.pth", map_location="cpu")


def _is_summary(m, n_samples, thresholds):
    assert set(m) == SUMMARY_KEYS and m["n_samples"] == n_samples and m["n_targets"] > 0 and m["n_bad_targets"] == 0
    assert [e["threshold"] for e in m["obstacle"]] == list(thresholds)
    assert all(set(e) == {"threshold", "precision", "recall", "iou", "f1"} for e in m["obstacle"])
    assert 0.0 <= m["rank_accuracy"] <= 1.0 and 0.0 <= m["top1_hit_rate"] <= 1.0 and m["mean_regret"] >= 0.0
    assert m["value_rmse"] >= m["value_mae"] > 0.0


def test_trainer_writes_the_metrics_only_when_asked(hip, tmp_path):
    _, loss0, ck0 = _train(tmp_path, "absent", {})
    assert set(loss0["1"]) == {"training_loss", "validation_loss"}
    assert set(ck0) == {"epoch", "model_state_dict", "optimizer_state_dict"}
    _, loss1, ck1 = _train(tmp_path, "on", {"validation_metrics": True, "metric_thresholds": [0.13, 0.5]})
    assert set(loss1["1"]) == {"training_loss", "validation_loss", "validation_metrics"}
    _is_summary(loss1["1"]["validation_metrics"], 3, (0.13, 0.5))
    assert ck1["validation_metrics"] == loss1["1"]["validation_metrics"]
    # an observer: the run itself does not change by a bit
    assert loss1["1"]["training_loss"] == loss0["1"]["training_loss"] and loss1["1"]["validation_loss"] == loss0["1"]["validation_loss"]
    assert all(torch.equal(ck1["model_state_dict"][k], ck0["model_state_dict"][k]) for k in ck0["model_state_dict"])


def test_trainer_with_ema_writes_both(hip, tmp_path):
    out, loss, ck = _train(tmp_path, "ema", {"validation_metrics": True, "ema_decay": 0.9})
    assert set(loss["1"]) == {"training_loss", "validation_loss", "validation_loss_ema", "validation_metrics", "validation_metrics_ema"}
    _is_summary(loss["1"]["validation_metrics"], 3, (0.13,))
    _is_summary(loss["1"]["validation_metrics_ema"], 3, (0.13,))
    assert loss["1"]["validation_metrics_ema"] != loss["1"]["validation_metrics"]
    assert ck["validation_metrics"] == loss["1"]["validation_metrics"]
    best = torch.load(out / "nbp_m_best_val_ema.pth", map_location="cpu")
    assert best["validation_metrics"] == loss["1"]["validation_metrics_ema"]
