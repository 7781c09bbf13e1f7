"""The optimizer's host side without a GPU: the float64 restatement against torch.optim.AdamW, the trainer's options, the config."""
import json
import os

import numpy as np
import pytest
import torch

import optim_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("max_norm", [None, 0.75, 1e6])
def test_restatement_matches_torch_adamw_float64(max_norm):
    """5 steps of torch.optim.AdamW on CPU float64 tensors (behind clip_grad_norm_ when clipping) against the numpy restatement,
    to 1e-12 relative: pins tests/optim_reference.py to the rule the GPU tests hold the kernels to."""
    rng = np.random.default_rng(4)
    shapes = [(1,), (3,), (7, 5), (64,), (2, 3, 4, 5)]
    lr, b1, b2, eps, wd = 3e-3, 0.9, 0.999, 1e-8, 0.01
    ps = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s))) for s in shapes]
    opt = torch.optim.AdamW(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p = [t.detach().numpy().copy() for t in ps]
    m = [np.zeros(s) for s in shapes]
    v = [np.zeros(s) for s in shapes]
    for step in range(1, 6):
        gs = [rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 1) for s in shapes]
        for t, g in zip(ps, gs):
            t.grad = torch.from_numpy(g.copy())
        if max_norm is not None:
            tn = torch.nn.utils.clip_grad_norm_(ps, max_norm)
            assert abs(float(tn) - R.total_norm(gs)) <= 1e-12 * R.total_norm(gs)
        opt.step()
        coef = R.clip_coef(gs, max_norm)
        assert (coef < 1.0) == (max_norm == 0.75)
        for i in range(len(shapes)):
            r = R.adamw_step(p[i], gs[i], m[i], v[i], step, lr, b1, b2, eps, wd, coef)
            p[i], m[i], v[i] = r["p"], r["m"], r["v"]
            st = opt.state[ps[i]]
            for got, want in ((ps[i].detach().numpy(), p[i]), (st["exp_avg"].numpy(), m[i]), (st["exp_avg_sq"].numpy(), v[i])):
                assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want) + 1e-300), (step, i, np.abs(got - want).max())


def test_default_config_holds_the_optimizer_keys_switched_off():
    cfg = json.load(open(os.path.join(ROOT, "configs/nbp/nbp_default_training_config.json")))["_nbp"]
    assert cfg["optimizer"] == "torch" and cfg["grad_clip_norm"] is None and cfg["skip_nonfinite_steps"] is False


def _tiny():
    return torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 1))


def test_make_optimizer_default_is_torch_adamw():
    from nextbestpath_amd.trainers import train_nbp_model as T
    net = _tiny()
    for opt in (T.make_optimizer(net), T.initialize_nbp(None, net)[1]):
        assert type(opt) is torch.optim.AdamW
        g = opt.param_groups[0]
        assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (0.001, (0.9, 0.999), 1e-8, 0.01)


def test_make_optimizer_refuses_bad_options():
    from nextbestpath_amd.trainers import train_nbp_model as T
    net = _tiny()
    with pytest.raises(ValueError):
        T.make_optimizer(net, impl="sgd")
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            T.make_optimizer(net, impl="hip", grad_clip_norm=bad)
    with pytest.raises(ValueError, match="hip"):
        T.make_optimizer(net, impl="torch", grad_clip_norm=1.0)
    with pytest.raises(ValueError, match="hip"):
        T.make_optimizer(net, skip_nonfinite_steps=True)

    class P:
        optimizer = "torch"
        grad_clip_norm = 1.0
    with pytest.raises(ValueError):
        T.initialize_nbp(P(), net)


def test_hip_adamw_refuses_cpu_parameters_and_unsupported_forms():
    from nextbestpath_amd.optim import HipAdamW
    from nextbestpath_amd.trainers import train_nbp_model as T
    net = _tiny()
    with pytest.raises(RuntimeError):
        HipAdamW(net.parameters())
    with pytest.raises(RuntimeError):
        T.make_optimizer(net, impl="hip", grad_clip_norm=1.0)
    for kw in ({"amsgrad": True}, {"maximize": True}, {"differentiable": True}, {"max_grad_norm": 0.0}, {"max_grad_norm": -2.0}):
        with pytest.raises(ValueError):
            HipAdamW(net.parameters(), **kw)
