"""WeightEMA / TensorEMA (nextbestpath_amd/optim.py, csrc/nbp_ema.hip) on the GPU against the float64 restatement of tests/ema_reference.py.

Inputs: magnitudes are exact zeros or in [1e-4, 1e2]: no subnormal appears.  Error bound: ema_reference.bound (a count of roundings,
never a measured value).  Every numeric check prints its worst error / bound ratio before it asserts."""
import copy
import json
import os
import types

import numpy as np
import pytest
import torch

import ema_reference as R
from nextbestpath_amd.optim import HipAdamW, TensorEMA, WeightEMA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMELS = [1, 3, 8, 64, 4099, 16385, 65537]        # below a quad, ragged tails, one element past a chunk, several chunks
# (numel, live tensor one element into its storage, shadow one element into its storage): the 4-byte path
VIEWS = [(4099, True, False), (16385, False, True), (4099, True, True), (2, True, True)]
UPDATES = 12


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _draw(rng, n):
    x = 10.0 ** rng.uniform(-4, 2, size=n) * rng.choice([-1.0, 1.0], size=n)
    return np.where(rng.random(n) < 0.1, 0.0, x).astype(np.float32)


def _place(host, misaligned):
    """A device tensor holding `host`; misaligned: a view that starts one element into its storage (address = 4 mod 16)."""
    if not misaligned:
        t = torch.from_numpy(host.copy()).to(_dev())
        assert t.data_ptr() % 16 == 0
        return t
    base = torch.empty(host.size + 1, dtype=torch.float32, device=_dev())
    t = base[1:]
    t.copy_(torch.from_numpy(host))
    assert t.data_ptr() % 16 == 4
    return t


def _bits_equal(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def _layout(force=None):
    """[(numel, live misaligned, shadow misaligned)]; force: every tensor aligned (False) or every tensor misaligned (True)."""
    lay = [(n, False, False) for n in NUMELS] + VIEWS
    return lay if force is None else [(n, force, force) for n, _, _ in lay]


def _twelve_updates(decay, warmup, check, force=None, seed=7):
    """-> (final shadows, num_updates).  p is redrawn between updates; before update 6 one live tensor moves to a new allocation."""
    rng = np.random.default_rng(seed)
    lay = _layout(force)
    live = [_place(_draw(rng, n), mp) for n, mp, _ in lay]
    shadow = [_place(_draw(rng, n), me) for n, _, me in lay]
    ema = TensorEMA(live, shadow)
    worst = 0.0
    for step in range(UPDATES):
        p_host = [_draw(rng, n) for n, _, _ in lay]
        for t, h in zip(live, p_host):
            t.copy_(torch.from_numpy(h))
        if step == 6:
            old = live[4].data_ptr()
            live[4].data = live[4].detach().clone()
            assert live[4].data_ptr() != old
        before = [e.cpu().numpy().copy() for e in shadow] if check else None
        ema.update(decay, warmup)
        if check:
            for e0, p, e in zip(before, p_host, shadow):
                got = e.cpu().numpy()
                ref = R.ema_step(e0, p, decay, step, warmup)
                err = np.abs(got.astype(np.float64) - ref)
                b = R.bound(e0, p, ref)
                assert np.all(np.isfinite(got))
                worst = max(worst, float(np.where(err == 0, 0.0, err / np.where(b > 0, b, 1e-300)).max()))
    if check:
        print(f"decay {decay} warm-up {warmup}: worst error / bound over {UPDATES} updates {worst:.3f}")
        assert worst <= 1.0, worst
    return [e.clone() for e in shadow], int(ema.num_updates)


# ---- 1. twelve consecutive updates against the float64 restatement
@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_twelve_updates_match_float64_restatement(hip, decay, warmup):
    _, n = _twelve_updates(decay, warmup, check=True)
    assert n == UPDATES


def test_the_check_sees_the_schedule(hip):
    """The bound has the power to tell one update's decay from the next one's: the restatement at n + 1 does not pass at n."""
    rng = np.random.default_rng(5)
    p, e0 = _draw(rng, 4099), _draw(rng, 4099)
    live, shadow = [_place(p, False)], [_place(e0, False)]
    ema = TensorEMA(live, shadow)
    ema.set_num_updates(3)
    ema.update(0.999, True)
    got = shadow[0].cpu().numpy().astype(np.float64)
    right, wrong = R.ema_step(e0, p, 0.999, 3), R.ema_step(e0, p, 0.999, 4)
    assert np.all(np.abs(got - right) <= R.bound(e0, p, right))
    assert np.any(np.abs(got - wrong) > R.bound(e0, p, wrong))
    assert int(ema.num_updates) == 4


# ---- 2. determinism; alignment does not change a bit
def test_two_runs_and_both_alignments_are_bit_identical(hip):
    a, _ = _twelve_updates(0.999, True, check=False, force=False)
    b, _ = _twelve_updates(0.999, True, check=False, force=False)
    c, _ = _twelve_updates(0.999, True, check=False, force=True)
    m, _ = _twelve_updates(0.999, True, check=False)
    assert _bits_equal(a, b), "two runs differ"
    assert _bits_equal(a, c) and _bits_equal(a, m), "the 4-byte path differs from the 16-byte path"


# ---- 3. the gate
class _Bag(torch.nn.Module):
    def __init__(self, hosts):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(h.copy())) for h in hosts])


def _set_grads(ps, hosts):
    for p, g in zip(ps, hosts):
        p.grad = torch.from_numpy(g.copy()).to(p.device)


def _check_against(what, before, ps, shadow, decay, n, warmup=True):
    worst = 0.0
    for e0, p, e in zip(before, ps, shadow):
        ph = p.detach().cpu().numpy()
        ref = R.ema_step(e0, ph, decay, n, warmup)
        err = np.abs(e.cpu().numpy().astype(np.float64) - ref)
        b = R.bound(e0, ph, ref)
        worst = max(worst, float(np.where(err == 0, 0.0, err / np.where(b > 0, b, 1e-300)).max()))
    print(f"{what}: worst error / bound {worst:.3f}")
    return worst


def test_a_dropped_optimizer_step_drops_the_update(hip):
    rng = np.random.default_rng(31)
    bag = _Bag([_draw(rng, n) for n in NUMELS]).to(_dev())
    ps = list(bag.parameters())
    opt = HipAdamW(ps, lr=1e-2, skip_nonfinite=True)
    ema = WeightEMA(bag, 0.999)
    shadow = list(ema.module.parameters())
    assert all(not e.requires_grad for e in shadow) and not ema.module.training
    _set_grads(ps, [_draw(rng, n) for n in NUMELS])
    opt.step()
    ema.update(opt)                                              # update 1 (n = 0)
    assert int(ema.num_updates) == 1
    held = [e.clone() for e in shadow]
    bad = [_draw(rng, n) for n in NUMELS]
    bad[5][9000] = float("inf")
    _set_grads(ps, bad)
    opt.step()                                                   # dropped on the device
    ema.update(opt)
    assert int(opt.skipped_steps) == 1
    assert _bits_equal(held, shadow) and int(ema.num_updates) == 1
    _set_grads(ps, [_draw(rng, n) for n in NUMELS])
    before = [e.cpu().numpy().copy() for e in shadow]
    opt.step()
    ema.update(opt)                                              # applies with the d of the unchanged n = 1
    assert _check_against("first update after a dropped one", before, ps, shadow, 0.999, 1) <= 1.0
    assert _check_against("  (the same against n = 2: must fail)", before, ps, shadow, 0.999, 2) > 1.0
    assert int(ema.num_updates) == 2 and int(opt.skipped_steps) == 1


def test_with_a_torch_optimizer_every_update_applies(hip):
    rng = np.random.default_rng(33)
    bag = _Bag([_draw(rng, n) for n in NUMELS]).to(_dev())
    ps = list(bag.parameters())
    opt = torch.optim.AdamW(ps, lr=1e-2, fused=True)
    ema = WeightEMA(bag, 0.5, warmup=False)
    shadow = list(ema.module.parameters())
    for n, arg in enumerate((opt, None, opt)):
        _set_grads(ps, [_draw(rng, k) for k in NUMELS])
        opt.step()
        before = [e.cpu().numpy().copy() for e in shadow]
        ema.update(arg)
        assert _check_against(f"torch optimizer, update {n + 1}", before, ps, shadow, 0.5, n, warmup=False) <= 1.0
    assert int(ema.num_updates) == 3


def test_update_does_not_synchronise(hip):
    rng = np.random.default_rng(35)
    bag = _Bag([_draw(rng, n) for n in NUMELS]).to(_dev())
    ps = list(bag.parameters())
    opt = HipAdamW(ps, skip_nonfinite=True)
    ema = WeightEMA(bag, 0.999)
    grads = [[torch.from_numpy(_draw(rng, n)).to(_dev()) for n in NUMELS] for _ in range(3)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for gs in grads:
            for p, g in zip(ps, gs):
                p.grad = g
            opt.step()
            ema.update(opt)
            opt.zero_grad(set_to_none=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(ema.num_updates) == 3


# ---- 4. the stale-pack trap on the real network
def _perturb(nbp, seed):
    gen = torch.Generator(device=_dev()).manual_seed(seed)
    with torch.no_grad():
        for p in nbp.parameters():
            p.mul_(1.0 + 0.05 * torch.randn(p.shape, generator=gen, device=p.device))
        for name, b in nbp.named_buffers():
            if name.endswith("running_mean"):
                b.add_(0.01 * torch.randn(b.shape, generator=gen, device=b.device))
            elif name.endswith("running_var"):
                b.mul_(1.0 + 0.05 * torch.rand(b.shape, generator=gen, device=b.device))
            else:
                b.add_(3)


def test_the_shadow_network_repacks_after_an_update(hip, nbp_weights):
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.utility.synthetic import make_count_maps
    nbp = NBP()
    nbp.load_state_dict(nbp_weights, strict=True)
    nbp = nbp.to(_dev())
    nbp.conv_precision = "fp32"
    x = make_count_maps(1, 32, seed=2).to(_dev())
    ema = WeightEMA(nbp, 0.0, warmup=False)
    assert ema.module.conv_precision == "fp32" and not ema.module.training and nbp.training
    assert all(not p.requires_grad for p in ema.module.parameters())
    with torch.no_grad():
        first = [o.clone() for o in ema.module(x)]
    # control: the kernel's writes alone leave the packed weights of a network stale (what WeightEMA.update has to undo)
    twin = copy.deepcopy(ema.module)
    with torch.no_grad():
        twin_first = [o.clone() for o in twin(x)]
    _perturb(nbp, 1)
    floats = lambda m: list(m.parameters()) + [b for b in m.buffers() if b.dtype.is_floating_point]
    TensorEMA(floats(nbp), floats(twin)).update(0.0, False)
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(twin_first, twin(x))), "the control no longer shows the trap"
    ema.update()                                                 # decay 0: e' = p exactly
    with torch.no_grad():
        second = [o.clone() for o in ema.module(x)]
        live = nbp.eval()(x)
    nbp.train()
    assert not torch.equal(first[0], second[0]) and not torch.equal(first[1], second[1])
    assert _bits_equal(second, live)
    assert _bits_equal(floats(nbp), floats(ema.module))
    # decay 0.9: a running statistic is the average, not a copy; the integer buffers are the live ones
    key = "Conv3.conv.1.running_var"
    e0 = ema.module.state_dict()[key].cpu().numpy().copy()
    _perturb(nbp, 2)
    ema.decay = 0.9
    ema.update()
    sd, live_sd = ema.module.state_dict(), nbp.state_dict()
    p = live_sd[key].cpu().numpy()
    ref = R.ema_step(e0, p, 0.9, 1, warmup=False)
    got = sd[key].cpu().numpy()
    assert np.all(np.abs(got.astype(np.float64) - ref) <= R.bound(e0, p, ref)) and not np.array_equal(got, p)
    tracked = [k for k in sd if k.endswith("num_batches_tracked")]
    assert tracked and all(int(sd[k]) == int(live_sd[k]) == int(nbp_weights[k]) + 6 for k in tracked)
    with torch.no_grad():
        third = ema.module(x)
    assert not torch.equal(third[0], second[0])


# ---- 5. state round trip
def test_state_dict_round_trip_continues_bit_for_bit(hip, nbp_weights):
    from nextbestpath_amd.networks.nbp_model import NBP
    nbp = NBP()
    nbp.load_state_dict(nbp_weights, strict=True)
    nbp = nbp.to(_dev())
    a = WeightEMA(nbp, 0.999)
    for s in (1, 2):
        _perturb(nbp, s)
        a.update()
    state = copy.deepcopy(a.state_dict())
    assert set(state) == {"decay", "warmup", "num_updates", "shadow"}
    assert (state["decay"], state["warmup"], state["num_updates"]) == (0.999, True, 2)
    _perturb(nbp, 3)                                             # b starts from other weights and other options
    b = WeightEMA(nbp, 0.5, warmup=False)
    b.load_state_dict(state)
    assert (b.decay, b.warmup, int(b.num_updates)) == (0.999, True, 2)
    for s in (4, 5, 6):
        _perturb(nbp, s)
        a.update()
        b.update()
    sa, sb = a.module.state_dict(), b.module.state_dict()
    assert int(a.num_updates) == int(b.num_updates) == 5
    assert len(sa) == 327 and list(sa) == list(nbp.state_dict())
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not torch.equal(sa["Conv1.conv.0.weight"], state["shadow"]["Conv1.conv.0.weight"])
    with torch.device("meta"):
        fresh = NBP()
    fresh.load_state_dict(sa, strict=True, assign=True)


# ---- 6. the trainer, synthetic mode
def _train(tmp_path, name, extra):
    from nextbestpath_amd.testers.nbp_planning import load_params
    from nextbestpath_amd.trainers import train_nbp_model as T
    cfg = json.load(open(os.path.join(ROOT, "configs/nbp/nbp_default_training_config.json")))
    out = tmp_path / name
    cfg["_nbp"].update({"nbp_model_name": "nbp_ema", "nbp_batch_size": 4, "grid_size": 64, "epochs": 1, "inner_epochs": 1,
                        "samples_per_epoch": 16, "n_validation_synthetic": 4, "output_dir": str(out), "collect": False})
    cfg["_nbp"].update(extra)
    path = tmp_path / f"{name}.json"
    path.write_text(json.dumps(cfg))
    T.run_training_nbp(load_params(str(path)))
    return out, json.load(open(out / "loss.json")), torch.load(out / "nbp_ema_best_val.pth", map_location="cpu")


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_trainer_with_ema_is_an_observer(hip, tmp_path, optimizer):
    from nextbestpath_amd.networks.nbp_model import NBP
    opts = {"optimizer": optimizer, "skip_nonfinite_steps": optimizer == "hip"}
    out0, loss0, ck0 = _train(tmp_path, "off", dict(opts, ema_decay=None))
    out1, loss1, ck1 = _train(tmp_path, "on", dict(opts, ema_decay=0.9))
    # off: today's outputs
    assert "validation_loss_ema" not in loss0["1"] and "ema_state_dict" not in ck0
    assert not (out0 / "nbp_ema_best_val_ema.pth").exists()
    # the live run does not change by a bit
    assert loss1["1"]["training_loss"] == loss0["1"]["training_loss"] and loss1["1"]["validation_loss"] == loss0["1"]["validation_loss"]
    assert list(ck1["model_state_dict"]) == list(ck0["model_state_dict"])
    assert all(torch.equal(ck1["model_state_dict"][k], ck0["model_state_dict"][k]) for k in ck0["model_state_dict"])
    assert {k: v for k, v in loss1["1"].items() if k != "validation_loss_ema"} == loss0["1"]
    # on: the averaged network is validated and checkpointed
    assert np.isfinite(loss1["1"]["validation_loss_ema"])
    es = ck1["ema_state_dict"]
    assert es["decay"] == 0.9 and es["warmup"] is True and es["num_updates"] >= 1 and len(es["shadow"]) == 327
    best = torch.load(out1 / "nbp_ema_best_val_ema.pth", map_location="cpu")
    assert best["validation_loss_ema"] == loss1["1"]["validation_loss_ema"]
    with torch.device("meta"):
        fresh = NBP()
    fresh.load_state_dict(best["model_state_dict"], strict=True, assign=True)
    assert all(torch.equal(best["model_state_dict"][k], es["shadow"][k]) for k in es["shadow"])
    # the average moved off the initial weights and is not the live network
    k = "Conv1.conv.0.weight"
    assert not torch.equal(es["shadow"][k], ck1["model_state_dict"][k])


def test_collection_model_is_the_shadow_only_under_ema_collect(hip):
    from nextbestpath_amd.trainers import train_nbp_model as T
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 1), torch.nn.BatchNorm2d(3)).to(_dev())
    ema = T.make_ema(types.SimpleNamespace(ema_decay=0.9, ema_warmup=False), net)
    assert isinstance(ema, WeightEMA) and ema.decay == 0.9 and ema.warmup is False
    assert T.collection_model(types.SimpleNamespace(ema_collect=True), net, ema) is ema.module
    assert T.collection_model(types.SimpleNamespace(ema_collect=False), net, ema) is net
    assert T.collection_model(types.SimpleNamespace(), net, ema) is net
    assert T.collection_model(types.SimpleNamespace(ema_collect=True), net, None) is net
