"""HipAdamW (nextbestpath_amd/optim.py, csrc/nbp_optim.hip) on the GPU against the float64 restatement of tests/optim_reference.py.

Inputs: gradient magnitudes are exact zeros or in [1e-6, 1e2]; state is zero or |m| in [1e-6, 1e2], v in [1e-12, 1e4]: no subnormal
appears in v or in a product.  Error bounds: optim_reference.bounds (counts of fp32 roundings, never measured values).  Every check
prints its worst error / bound ratio before it asserts."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import optim_reference as R
from nextbestpath_amd.optim import HipAdamW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (3,), (8,), (64,), (4099,), (65537,), (512, 512, 3, 3)]        # numel 1, 3, 8, 64, 4099, 65 537, 2 359 296
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _log_uniform(rng, shape, lo, hi, zeros=0.0, signed=True):
    x = 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), size=shape)
    if signed:
        x = x * rng.choice([-1.0, 1.0], size=shape)
    if zeros:
        x = np.where(rng.random(shape) < zeros, 0.0, x)
    return x.astype(np.float32)


def _grads(rng, shapes):
    return [_log_uniform(rng, s, 1e-6, 1e2, zeros=0.1) for s in shapes]


def _params(rng, shapes):
    return [_log_uniform(rng, s, 1e-4, 1.0) for s in shapes]


def _nbp_params():
    from nextbestpath_amd.networks.nbp_model import NBP
    torch.manual_seed(9)
    return [p.detach().numpy().copy() for p in NBP().parameters()]


def _state(rng, shapes, step):
    return {"step": float(step), "m": [_log_uniform(rng, s, 1e-6, 1e2) for s in shapes],
            "v": [_log_uniform(rng, s, 1e-12, 1e4, signed=False) for s in shapes]}


def _make(kind, p_host, state=None, **extra):
    """-> (optimizer, device parameters); state: {"step", "m", "v"} loaded through load_state_dict (both classes take the same dict)."""
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(_dev())) for p in p_host]
    opt = HipAdamW(ps, **HYPER, **extra) if kind == "hip" else torch.optim.AdamW(ps, fused=True, **HYPER)
    if state is not None:
        sd = {"state": {i: {"step": torch.tensor(state["step"], dtype=torch.float32), "exp_avg": torch.from_numpy(state["m"][i].copy()),
                            "exp_avg_sq": torch.from_numpy(state["v"][i].copy())} for i in range(len(ps))},
              "param_groups": opt.state_dict()["param_groups"]}
        opt.load_state_dict(sd)
    return opt, ps


def _set_grads(ps, g_host):
    for p, g in zip(ps, g_host):
        p.grad = torch.from_numpy(g.copy()).to(p.device)


def _snapshot(opt, ps):
    """Host copies (p, m, v, step) of the optimizer's current state; zeros before the first step."""
    out = {"p": [p.detach().cpu().numpy().copy() for p in ps], "m": [], "v": [], "step": []}
    for p in ps:
        st = opt.state.get(p, {})
        out["m"].append(st["exp_avg"].cpu().numpy().copy() if st else np.zeros(tuple(p.shape), np.float32))
        out["v"].append(st["exp_avg_sq"].cpu().numpy().copy() if st else np.zeros(tuple(p.shape), np.float32))
        out["step"].append(float(st["step"]) if st else 0.0)
    return out


def _violations(before, after, g_host, step, lr, coef=1.0, clipped=False):
    """Worst error / bound ratio of (m, v, p) over all tensors, stepping the restatement from `before`."""
    worst = [0.0, 0.0, 0.0]
    for i in range(len(g_host)):
        r = R.adamw_step(before["p"][i], g_host[i], before["m"][i], before["v"][i], step, lr, *HYPER["betas"], HYPER["eps"],
                         HYPER["weight_decay"], coef)
        bm, bv, bp = R.bounds(before["p"][i], r, lr, *HYPER["betas"], clipped=clipped)
        for k, (got, want, b) in enumerate(((after["m"][i], r["m"], bm), (after["v"][i], r["v"], bv), (after["p"][i], r["p"], bp))):
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(np.isfinite(got))
            ratio = np.where(err == 0, 0.0, err / np.where(b > 0, b, 1e-300))
            worst[k] = max(worst[k], float(ratio.max()))
    return worst


def _check(what, before, after, g_host, step, lr, coef=1.0, clipped=False):
    worst = _violations(before, after, g_host, step, lr, coef, clipped)
    print(f"{what}: worst error / bound  m {worst[0]:.3f}  v {worst[1]:.3f}  p {worst[2]:.3f}")
    assert max(worst) <= 1.0, (what, worst)
    assert all(s == float(step) for s in after["step"]), (what, after["step"][:4], step)


def _bits_equal(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def _device_state(opt, ps):
    return ([p.detach().clone() for p in ps], [opt.state[p]["exp_avg"].clone() for p in ps],
            [opt.state[p]["exp_avg_sq"].clone() for p in ps], [opt.state[p]["step"].clone() for p in ps])


# ---- 1. one step against the float64 restatement; torch's fused kernel goes through the same bounds
@pytest.mark.parametrize("kind", ["hip", "torch"])
@pytest.mark.parametrize("case", ["zero_state", "random_state", "nbp"])
def test_one_step_matches_float64_restatement(hip, kind, case):
    rng = np.random.default_rng({"zero_state": 1, "random_state": 2, "nbp": 3}[case])
    p_host = _nbp_params() if case == "nbp" else _params(rng, SHAPES)
    shapes = [p.shape for p in p_host]
    state = _state(rng, shapes, 7) if case == "random_state" else None
    opt, ps = _make(kind, p_host, state)
    g = _grads(rng, shapes)
    _set_grads(ps, g)
    before = _snapshot(opt, ps)
    opt.step()
    _check(f"{kind}/{case}", before, _snapshot(opt, ps), g, (8 if state else 1), HYPER["lr"])


# ---- 2. twenty consecutive steps, each checked from the device's own state; ReduceLROnPlateau lowers lr between steps 10 and 11
def _twenty_steps(check):
    rng = np.random.default_rng(11)
    opt, ps = _make("hip", _params(rng, SHAPES))
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.1, patience=0)
    for step in range(1, 21):
        if step == 11:
            sched.step(1.0)
            sched.step(2.0)
            assert opt.param_groups[0]["lr"] == pytest.approx(1e-4)
        g = _grads(rng, SHAPES)
        _set_grads(ps, g)
        before = _snapshot(opt, ps) if check else None
        opt.step()
        opt.zero_grad(set_to_none=True)
        if check:
            after = _snapshot(opt, ps)
            _check(f"step {step}", before, after, g, step, opt.param_groups[0]["lr"])
            if step == 11:      # the check has the power to see the learning rate: the old one does not pass
                assert max(_violations(before, after, g, step, 1e-3)) > 1.0
    return _device_state(opt, ps)


def test_twenty_steps_with_lr_drop(hip):
    _twenty_steps(check=True)


# ---- 3. the norm and the clip coefficient
def _clip_case(factor, check):
    """One clipped step with max_grad_norm = factor x the true norm, from a random state at step 4.  -> device results."""
    rng = np.random.default_rng(21)
    p_host = _params(rng, SHAPES)
    state = _state(rng, SHAPES, 4)
    g = _grads(rng, SHAPES)
    norm64 = R.total_norm(g)
    opt, ps = _make("hip", p_host, state, max_grad_norm=factor * norm64)
    _set_grads(ps, g)
    g_dev = [p.grad.clone() for p in ps]
    before = _snapshot(opt, ps)
    opt.step()
    assert _bits_equal(g_dev, [p.grad for p in ps]), "p.grad was modified"
    got = float(opt.last_grad_norm)
    if check:
        print(f"grad norm: device {got!r}, float64 {norm64!r}, relative error {abs(got - norm64) / norm64:.2e}")
        assert abs(got - norm64) <= 1e-5 * norm64
        coef = R.clip_coef(g, factor * norm64)
        assert (coef < 1.0) == (factor < 1.0)
        _check(f"clip x{factor}", before, _snapshot(opt, ps), g, 5, HYPER["lr"], coef, clipped=coef < 1.0)
    if factor > 1.0:            # the coefficient is exactly 1.0f: the same bits as a step without the norm pass
        plain, qs = _make("hip", p_host, state)
        _set_grads(qs, g)
        plain.step()
        assert all(_bits_equal(a, b) for a, b in zip(_device_state(opt, ps), _device_state(plain, qs)))
    return _device_state(opt, ps) + ([opt.last_grad_norm.clone()],)


@pytest.mark.parametrize("factor", [0.5, 2.0])
def test_norm_and_clipping(hip, factor):
    _clip_case(factor, check=True)


def test_norm_of_the_nbp_gradient_list(hip):
    rng = np.random.default_rng(23)
    p_host = _nbp_params()
    g = _grads(rng, [p.shape for p in p_host])
    opt, ps = _make("hip", p_host, skip_nonfinite=True)
    _set_grads(ps, g)
    opt.step()
    got, want = float(opt.last_grad_norm), R.total_norm(g)
    print(f"NBP list ({sum(x.size for x in g)} elements): device norm {got!r}, float64 {want!r}")
    assert abs(got - want) <= 1e-5 * want and int(opt.skipped_steps) == 0


# ---- 4. a non-finite gradient element (planted data; nothing here faults the device)
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_step_is_skipped(hip, bad):
    rng = np.random.default_rng(31)
    p_host = _params(rng, SHAPES)
    opt, ps = _make("hip", p_host, max_grad_norm=1.0, skip_nonfinite=True)
    g = _grads(rng, SHAPES)
    _set_grads(ps, g)
    opt.step()                                   # step 1: finite
    held = _device_state(opt, ps)
    g2 = _grads(rng, SHAPES)
    g2[5][40000] = bad
    _set_grads(ps, g2)
    opt.step()                                   # dropped
    assert all(_bits_equal(a, b) for a, b in zip(held, _device_state(opt, ps)))
    assert int(opt.skipped_steps) == 1 and not np.isfinite(float(opt.last_grad_norm))
    # from a fresh optimizer: the dropped step leaves step = 0, the next finite one is step 1
    opt, ps = _make("hip", p_host, skip_nonfinite=True)
    _set_grads(ps, g2)
    opt.step()
    assert int(opt.skipped_steps) == 1 and all(float(opt.state[p]["step"]) == 0.0 for p in ps)
    assert _bits_equal([torch.from_numpy(p) for p in p_host], [p.detach().cpu() for p in ps])
    _set_grads(ps, g)
    before = _snapshot(opt, ps)
    opt.step()
    _check("first finite step after a dropped one", before, _snapshot(opt, ps), g, 1, HYPER["lr"])
    assert int(opt.skipped_steps) == 1


# ---- 5. determinism
def test_two_runs_are_bit_identical(hip):
    for run in (lambda: _twenty_steps(check=False), lambda: _clip_case(0.5, check=False), lambda: _clip_case(2.0, check=False)):
        a, b = run(), run()
        assert all(_bits_equal(x, y) for x, y in zip(a, b))


# ---- 6. state_dict exchange with torch.optim.AdamW(fused=True), both directions
@pytest.mark.parametrize("first", ["hip", "torch"])
def test_state_dict_exchange(hip, first):
    second = "torch" if first == "hip" else "hip"
    rng = np.random.default_rng(41)
    a, ps = _make(first, _params(rng, SHAPES))
    for _ in range(3):
        _set_grads(ps, _grads(rng, SHAPES))
        a.step()
    sd = copy.deepcopy(a.state_dict())
    b, qs = _make(second, [p.detach().cpu().numpy() for p in ps])
    b.load_state_dict(sd)
    g = _grads(rng, SHAPES)
    _set_grads(qs, g)
    before = _snapshot(b, qs)
    assert before["step"] == [3.0] * len(qs)
    assert _bits_equal([torch.from_numpy(m) for m in before["m"]], [a.state[p]["exp_avg"].cpu() for p in ps])
    b.step()
    _check(f"{first} -> {second}, step 4", before, _snapshot(b, qs), g, 4, HYPER["lr"])


# ---- 7. no host synchronisation in step()
def test_step_does_not_synchronise(hip):
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    rng = np.random.default_rng(51)
    opt, ps = _make("hip", _params(rng, SHAPES), max_grad_norm=1.0, skip_nonfinite=True)
    grads = [[torch.from_numpy(x).to(_dev()) for x in _grads(rng, SHAPES)] for _ in range(3)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for gs in grads:                         # the first step builds the tables, the later ones refresh the gradient addresses
            for p, g in zip(ps, gs):
                p.grad = g
            opt.step()
            opt.zero_grad(set_to_none=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(opt.state[ps[0]]["step"]) == 3.0


# ---- refusals that need a device tensor
def test_noncontiguous_tensors_are_refused(hip):
    w = torch.nn.Parameter(torch.zeros(8, 6, device=_dev()).t())
    with pytest.raises(ValueError):
        HipAdamW([w])
    p = torch.nn.Parameter(torch.zeros(6, 8, device=_dev()))
    opt = HipAdamW([p])
    p.grad = torch.ones(8, 6, device=_dev()).t()
    with pytest.raises(ValueError):
        opt.step()
    with pytest.raises(ValueError):
        opt.step(closure=lambda: 0.0)


# ---- 8. the trainer
def _train(tmp_path, name, extra):
    from nextbestpath_amd.testers.nbp_planning import load_params
    from nextbestpath_amd.trainers import train_nbp_model as T
    cfg = json.load(open(os.path.join(ROOT, "configs/nbp/nbp_default_training_config.json")))
    for k in ("optimizer", "grad_clip_norm", "skip_nonfinite_steps"):
        del cfg["_nbp"][k]
    out = tmp_path / name
    cfg["_nbp"].update({"nbp_model_name": "nbp_opt", "nbp_batch_size": 4, "grid_size": 64, "epochs": 1, "inner_epochs": 1,
                        "samples_per_epoch": 16, "n_validation_synthetic": 4, "output_dir": str(out), "collect": False})
    cfg["_nbp"].update(extra)
    path = tmp_path / f"{name}.json"
    path.write_text(json.dumps(cfg))
    hist = T.run_training_nbp(load_params(str(path)))
    ck = torch.load(out / "nbp_opt_best_val.pth", map_location="cpu")
    return hist, json.load(open(out / "loss.json")), ck


def test_trainer_with_hip_optimizer(hip, tmp_path, monkeypatch):
    calls = []
    real = HipAdamW.step
    monkeypatch.setattr(HipAdamW, "step", lambda self, closure=None: (calls.append(1), real(self, closure))[1])
    opts = {"optimizer": "hip", "grad_clip_norm": 1.0, "skip_nonfinite_steps": True}
    hist, loss, ck = _train(tmp_path, "a", opts)
    n_steps = len(calls)
    assert n_steps >= 1
    e = loss["1"]
    assert set(e) == {"training_loss", "validation_loss", "grad_norm", "skipped_steps"}
    assert np.isfinite(e["training_loss"]) and np.isfinite(e["validation_loss"])
    assert len(e["grad_norm"]) == n_steps and all(np.isfinite(v) and v > 0 for v in e["grad_norm"]) and e["skipped_steps"] == 0
    assert {"step", "exp_avg", "exp_avg_sq"} == set(ck["optimizer_state_dict"]["state"][0])
    # the same run again: the same bits
    hist2, loss2, ck2 = _train(tmp_path, "b", opts)
    assert loss2 == loss
    assert all(torch.equal(ck["model_state_dict"][k], ck2["model_state_dict"][k]) for k in ck["model_state_dict"])
    # without the three keys: today's loss.json
    _, loss3, _ = _train(tmp_path, "c", {})
    assert set(loss3["1"]) == {"training_loss", "validation_loss"}
    assert len(calls) == 2 * n_steps
