"""GPU: the D4 augmentation of training batches -- nbp_augment_batch_f32 against the numpy restatement of its index rule (bit for
bit), against the device map build on a mirrored cloud, the equivariance of the gathered loss inputs, and the trainer option
`augment_probability` (off: the trainer as it was, bit for bit; on: deterministic, finite, the replay records untouched)."""
import json
import os
import random
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import augment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.device("cuda")


def restate(a, op):
    """The index rule as one numpy gather: out[r][c] = A[fr ? n - r : r][fc ? n - c : c], A = in^T when bit 0 is set, 0 where the
    source index is n (bit 1 = fr, bit 2 = fc)."""
    a = np.asarray(a)
    n = a.shape[-1]
    R, C = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    rp = n - R if op & 2 else R
    cp = n - C if op & 4 else C
    ok = (rp < n) & (cp < n)
    rp, cp = np.minimum(rp, n - 1), np.minimum(cp, n - 1)
    sr, sc = (cp, rp) if op & 1 else (rp, cp)
    return np.where(ok, a[..., sr, sc], 0).astype(a.dtype)


def _ops_dev(ops):
    return torch.tensor(list(ops), dtype=torch.int32, device=D)


@pytest.mark.parametrize("S", [32, 48, 256])
@pytest.mark.parametrize("ops", [tuple(range(8)), (5, 0, 5, 3, 0, 0, 7, 1, 2, 2, 6), (0,), (4,)])
def test_kernel_equals_the_numpy_restatement(hip, S, ops):
    from nextbestpath_amd.utility import hipops
    B = len(ops)
    rng = np.random.default_rng(S + B)
    x = (rng.standard_normal((B, 5, S, S)) + 3.0).astype(np.float32)          # row 0 / col 0 non-zero: the zeroing is seen
    gt = (rng.random((B, 1, S, S)) + 0.5).astype(np.float32)
    xd, gd = torch.from_numpy(x).to(D), torch.from_numpy(gt).to(D)
    xo, go = hipops.augment_batch(xd, gd, _ops_dev(ops))
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), torch.from_numpy(x)) and torch.equal(gd.cpu(), torch.from_numpy(gt))      # out of place
    xo, go = xo.cpu().numpy(), go.cpu().numpy()
    for b, op in enumerate(ops):
        assert np.array_equal(xo[b].view(np.uint32), restate(x[b], op).view(np.uint32)), (b, op)
        assert np.array_equal(go[b].view(np.uint32), restate(gt[b], op).view(np.uint32)), (b, op)
        assert np.array_equal(xo[b], augment.transform_maps(x[b], op))
        if op == 0:
            assert np.array_equal(xo[b], x[b]) and np.array_equal(go[b], gt[b])
        if op & 2:
            assert not xo[b][:, 0, :].any() and not go[b][:, 0, :].any()
        if op & 4:
            assert not xo[b][:, :, 0].any() and not go[b][:, :, 0].any()


def test_bad_arguments_write_nothing(hip):
    from nextbestpath_amd import _lib
    from nextbestpath_amd.utility import hipops
    B, S = 2, 32
    x = torch.rand(B, 5, S, S, device=D)
    gt = torch.rand(B, 1, S, S, device=D)
    ops = _ops_dev([3, 5])
    xo = torch.full_like(x, -7.0)
    go = torch.full_like(gt, -7.0)
    st = _lib.current_stream()
    p = _lib.ptr
    call = hip.nbp_augment_batch_f32
    assert call(p(x), p(gt), p(ops), B, 24, p(xo), p(go), st) < 0           # S % 16
    assert call(p(x), p(gt), p(ops), 0, S, p(xo), p(go), st) < 0            # B < 1
    assert call(0, p(gt), p(ops), B, S, p(xo), p(go), st) < 0
    assert call(p(x), 0, p(ops), B, S, p(xo), p(go), st) < 0
    assert call(p(x), p(gt), 0, B, S, p(xo), p(go), st) < 0
    assert call(p(x), p(gt), p(ops), B, S, 0, p(go), st) < 0
    assert call(p(x), p(gt), p(ops), B, S, p(xo), 0, st) < 0
    assert call(p(x), p(gt), p(ops), B, S, p(x), p(go), st) < 0             # in place
    assert call(p(x), p(gt), p(ops), B, S, p(xo) + 4, p(go), st) < 0        # off the 16-byte grid
    torch.cuda.synchronize()
    assert bool((xo == -7.0).all()) and bool((go == -7.0).all())
    assert call(p(x), p(gt), p(ops), B, S, p(xo), p(go), st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(xo[1].cpu().numpy(), restate(x[1].cpu().numpy(), 5))
    # the wrapper takes device tensors only
    with pytest.raises(RuntimeError):
        hipops.augment_batch(x.cpu(), gt, ops)
    with pytest.raises(RuntimeError):
        hipops.augment_batch(x, gt, ops.cpu())
    with pytest.raises(ValueError):
        hipops.augment_batch(x, gt, ops.long())


def _move(v, op):
    """(row, col) camera-frame coordinates of a cloud under `op` (v = -(offset): mirrored offsets are mirrored coordinates)."""
    vr, vc = v[..., 0], v[..., 1]
    if op & 1:
        vr, vc = vc, vr
    if op & 2:
        vr = -vr
    if op & 4:
        vc = -vc
    return np.stack([vr, vc], -1)


def test_device_map_build_of_the_mirrored_cloud_equals_augment_batch(hip):
    """20 000 seeded points (6 planes' worth) within +-45 units of the camera, on a 2^-14 grid so that every mirrored coordinate is
    exact in fp32: utils.map_points_to_n_imgs of the moved cloud == augment_batch of the maps of the cloud, on rows / cols 1..S-1.
    Cells that a point within 1e-4 cells of a half-cell tie of rint can reach are counted and excluded (the fp32 rounding of
    (v + 40) * scale is not mirror-symmetric to the last bit, 3e-5 cells at most); fewer than 1 in 10 000 may be."""
    from nextbestpath_amd.utility import hipops, utils
    S, m = 256, 20000
    rng = np.random.default_rng(7)
    v = np.round(rng.uniform(-45.0, 45.0, (6, m, 2)) * 2.0 ** 14) / 2.0 ** 14
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    first = utils.map_points_to_n_imgs(torch.from_numpy(v.astype(np.float32)).to(D), (S, S), (-40, 40))          # [6,S,S]
    assert float(first.sum()) > 6 * 15000
    ops = list(range(8))
    x = first[:5].unsqueeze(0).repeat(8, 1, 1, 1).contiguous()
    gt = first[5:].unsqueeze(0).repeat(8, 1, 1, 1).contiguous()
    xo, go = hipops.augment_batch(x, gt, _ops_dev(ops))
    moved = torch.cat([xo, go], 1).cpu().numpy()                                                                     # [8,6,S,S]
    excluded = 0
    for op in ops:
        v2 = _move(v, op)
        second = utils.map_points_to_n_imgs(torch.from_numpy(v2.astype(np.float32)).to(D), (S, S), (-40, 40)).cpu().numpy()
        diff = (moved[op] != second)[:, 1:, 1:]
        u = (v2 + 40.0) * S / 80.0
        ties = np.zeros((6, S, S), dtype=bool)
        for k, ur, uc in ((k, ur, uc) for k in range(6)
                          for ur, uc in u[k][(np.abs(u[k] - np.floor(u[k]) - 0.5) < 1e-4).any(1)]):
            for r in (int(np.floor(ur)), int(np.ceil(ur))):
                for c in (int(np.floor(uc)), int(np.ceil(uc))):
                    if 0 <= r < S and 0 <= c < S:
                        ties[k, r, c] = True
        bad = diff & ~ties[:, 1:, 1:]
        print(f"op {op}: {int(diff.sum())} tie cells excluded of {diff.size}")
        assert not bad.any(), f"op {op}: {int(bad.sum())} cells differ away from rint ties"
        if op == 0:
            assert not diff.any()
        excluded += int(diff.sum())
    assert excluded * 10000 < 8 * 6 * (S - 1) ** 2


def test_gathered_values_are_equivariant(hip):
    from nextbestpath_amd.networks import training as tr
    B, V = 8, 64
    rng = np.random.default_rng(1)
    out1 = rng.standard_normal((B, 8, V, V)).astype(np.float32)
    twin = np.empty_like(out1)
    pix, bidx, pix2, bidx2, kept = [], [], [], [], []
    for b in range(B):
        op = b
        hm = augment.heading_map(op)
        for c in range(8):
            twin[b, hm[c]] = restate(out1[b, c], op)
        k = 30
        p = np.stack([rng.integers(0, 8, k), rng.integers(1, V, k), rng.integers(1, V, k)], 1).astype(np.int64)
        p[:4, 1] = 0
        p[2:6, 2] = 0                                           # targets on row 0 / col 0: dropped by the reflections
        ident = np.arange(k, dtype=np.float32)                  # the gains carry the targets' identity through the drop
        p2, g2 = augment.transform_targets(p, ident, op, V)
        pix.append(p); bidx.append(np.full(k, b))
        pix2.append(p2); bidx2.append(np.full(len(p2), b)); kept.append(g2.astype(np.int64) + b * k)
        assert len(p2) == k - (4 if op in (2, 3, 4, 5) else 6 if op in (6, 7) else 0)
    with torch.no_grad():
        a = tr.gather_values(torch.from_numpy(out1).to(D), torch.from_numpy(np.concatenate(bidx)).to(D),
                             torch.from_numpy(np.concatenate(pix)).to(D)).cpu().numpy()
        t = tr.gather_values(torch.from_numpy(twin).to(D), torch.from_numpy(np.concatenate(bidx2)).to(D),
                             torch.from_numpy(np.concatenate(pix2)).to(D)).cpu().numpy()
    assert np.array_equal(t.view(np.uint32), a[np.concatenate(kept)].view(np.uint32))


# ---- the trainer

def _db_bytes(db):
    return [{k: (v.tobytes(), v.dtype.str, v.shape) if isinstance(v, np.ndarray) else v for k, v in d.items()} for d in db]


_RUNS = {}


def _train_run(tag, **opts):
    """One epoch of train_experience_data on 64 synthetic records (S = 64, 16 batches, 2 optimizer steps) from fixed seeds."""
    if tag in _RUNS:
        return _RUNS[tag]
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.trainers import train_nbp_model as T
    params = types.SimpleNamespace(nbp_batch_size=4, random_seed=8, **opts)
    db = T.make_synthetic_experiences(64, S=64, seed=5)
    for d in db[:8]:
        d["target_value_map_pixel"][0, 1:] = 0                 # targets on row 0 / col 0: some are dropped when augmented
    before = _db_bytes(db)
    order = list(db)
    where = {id(d): i for i, d in enumerate(db)}
    torch.manual_seed(3); random.seed(3); np.random.seed(3)
    net = NBP().to(D)
    _, opt, _, _ = T.initialize_nbp(params, net)
    net.train()
    losses = T.train_experience_data(order, params, opt, net, D, current_epoch=2)
    torch.cuda.synchronize()
    res = dict(losses=losses, state={k: t.detach().clone() for k, t in net.state_dict().items()}, global_rng=random.getstate(),
               untouched=_db_bytes(db) == before, order=[where[id(d)] for d in order])
    _RUNS[tag] = res
    return res


def test_default_is_untouched(hip):
    a = _train_run("absent")
    b = _train_run("zero", augment_probability=0.0)
    assert len(a["losses"]) == 2 and a["losses"] == b["losses"]
    for k in a["state"]:
        assert torch.equal(a["state"][k], b["state"][k]), k
    assert a["global_rng"] == b["global_rng"] and a["order"] == b["order"]


def test_augmented_epoch_is_deterministic_finite_and_leaves_the_records_alone(hip):
    z = _train_run("zero", augment_probability=0.0)
    a = _train_run("one_a", augment_probability=1.0)
    b = _train_run("one_b", augment_probability=1.0)
    assert len(a["losses"]) == 2 and a["losses"] == b["losses"]
    for k in a["state"]:
        assert torch.equal(a["state"][k], b["state"][k]), k
    assert a["losses"] != z["losses"]
    assert all(np.isfinite(v) for v in a["losses"])
    assert a["untouched"] and b["untouched"] and z["untouched"]
    # the option draws from the trainer's own generator: the replay set is shuffled as without it
    assert a["global_rng"] == z["global_rng"] and a["order"] == z["order"]
    c = _train_run("one_seeded", augment_probability=1.0, augment_seed=12345)
    assert c["losses"] != a["losses"] and all(np.isfinite(v) for v in c["losses"])


def test_augmented_epoch_with_synchronous_copies_equals_the_staged_one(hip, monkeypatch):
    from nextbestpath_amd.trainers import train_nbp_model as T
    a = _train_run("one_a", augment_probability=1.0)
    monkeypatch.setattr(T, "_STAGE_BATCHES", False)
    s = _train_run("one_sync", augment_probability=1.0)
    assert a["losses"] == s["losses"]
    for k in a["state"]:
        assert torch.equal(a["state"][k], s["state"][k]), k


def test_train_entry_point_with_augmentation(hip, tmp_path):
    cfg = json.load(open(os.path.join(ROOT, "configs/nbp/nbp_default_training_config.json")))
    assert cfg["_nbp"]["augment_probability"] == 0.0
    cfg["_data"]["data_path"] = str(tmp_path / "no_dataset_here")          # offline mode: synthetic records
    cfg["_nbp"].update({"nbp_model_name": "nbp_aug", "nbp_batch_size": 4, "grid_size": 64, "epochs": 1, "inner_epochs": 1,
                        "samples_per_epoch": 16, "n_validation_synthetic": 4, "output_dir": str(tmp_path / "w"),
                        "augment_probability": 0.5})
    path = tmp_path / "cfg_aug.json"
    path.write_text(json.dumps(cfg))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_nbp.py"), "-c", str(path)], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2500:]
    hist = json.load(open(tmp_path / "w" / "loss.json"))
    assert "1" in hist and np.isfinite(hist["1"]["training_loss"]) and np.isfinite(hist["1"]["validation_loss"])
