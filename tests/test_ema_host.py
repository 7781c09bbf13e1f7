"""The weight average's host side without a GPU: the decay schedule of tests/ema_reference.py, option validation, the refusals, the config."""
import copy
import json
import os
import types

import numpy as np
import pytest
import torch

import ema_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_warmup_schedule_reaches_the_decay_at_the_right_update():
    assert R.decay_at(0.999, 0) == 0.1 and R.decay_at(0.999, 1) == 2.0 / 11.0
    # (1 + n) / (10 + n) >= 0.999  <=>  n >= 8990, where the quotient 8991 / 9000 is the double nearest to 0.999: the literal itself
    assert R.decay_at(0.999, 8989) == 8990.0 / 8999.0 < 0.999
    assert R.decay_at(0.999, 8990) == 0.999 and R.decay_at(0.999, 10 ** 6) == 0.999
    # decay 0.5: 8 / 17 at n = 7, 9 / 18 = 0.5 at n = 8 (both arguments of the min agree), the decay from there on
    assert [R.decay_at(0.5, n) for n in (6, 7, 8, 9, 100)] == [7.0 / 16.0, 8.0 / 17.0, 0.5, 0.5, 0.5]
    assert all(R.decay_at(d, n, warmup=False) == d for d in (0.0, 0.5, 0.999) for n in (0, 3, 10 ** 4))
    assert R.decay_at(0.0, 5) == 0.0


def test_restatement_is_the_lerp_and_its_bound_covers_the_other_association():
    rng = np.random.default_rng(3)
    e = (10.0 ** rng.uniform(-4, 2, 1000) * rng.choice([-1.0, 1.0], 1000)).astype(np.float32)
    p = (10.0 ** rng.uniform(-4, 2, 1000) * rng.choice([-1.0, 1.0], 1000)).astype(np.float32)
    for decay, n in ((0.999, 0), (0.999, 10 ** 4), (0.5, 3)):
        d = R.decay_at(decay, n)
        ref = R.ema_step(e, p, decay, n)
        other = d * e.astype(np.float64) + (1.0 - d) * p.astype(np.float64)
        assert np.all(np.abs(other.astype(np.float32).astype(np.float64) - ref) <= R.bound(e, p, ref))
        torch_lerp = torch.lerp(torch.from_numpy(e).double(), torch.from_numpy(p).double(), 1.0 - d).numpy()
        assert np.all(np.abs(torch_lerp - ref) <= 2.0 ** -45 * (np.abs(e) + np.abs(p)))
    assert np.array_equal(R.ema_step(e, p, 0.0, 0, warmup=False), p.astype(np.float64))


def test_decay_validation():
    from nextbestpath_amd.optim import check_ema_decay
    for good in (0, 0.0, 0.5, 0.999, np.float32(0.25)):
        assert check_ema_decay(good) == float(good)
    for bad in (-0.1, 1, 1.0, 1.5, float("nan"), float("inf"), "0.9", True, None, [0.9]):
        with pytest.raises(ValueError):
            check_ema_decay(bad)


def test_weight_ema_refuses_cpu_modules_and_bad_options():
    from nextbestpath_amd.optim import TensorEMA, WeightEMA
    net = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    with pytest.raises(RuntimeError):
        WeightEMA(net, 0.999)
    with pytest.raises(ValueError):
        WeightEMA(net, 1.0)
    with pytest.raises(ValueError):
        WeightEMA(net, -0.5, warmup=False)
    with pytest.raises(RuntimeError):
        TensorEMA([torch.zeros(4)], [torch.zeros(4)])
    with pytest.raises(ValueError):
        TensorEMA([], [])


def test_trainer_options():
    from nextbestpath_amd.trainers import train_nbp_model as T
    net = torch.nn.Linear(3, 2)
    assert T.make_ema(types.SimpleNamespace(), net) is None
    assert T.make_ema(types.SimpleNamespace(ema_decay=None, ema_warmup=True, ema_collect=True), net) is None
    for bad in (1.0, -0.1, 2, "0.9", True):
        with pytest.raises(ValueError):
            T.make_ema(types.SimpleNamespace(ema_decay=bad), net)
    with pytest.raises(RuntimeError):                    # a valid decay on a CPU module: no CPU path
        T.make_ema(types.SimpleNamespace(ema_decay=0.9), net)
    assert T.collection_model(types.SimpleNamespace(ema_collect=True), net, None) is net


def test_default_config_holds_the_ema_keys_switched_off():
    cfg = json.load(open(os.path.join(ROOT, "configs/nbp/nbp_default_training_config.json")))["_nbp"]
    assert cfg["ema_decay"] is None and cfg["ema_warmup"] is True and cfg["ema_collect"] is False


def test_a_copied_network_does_not_share_the_pack():
    from nextbestpath_amd.networks.nbp_model import NBP
    with torch.device("meta"):
        net = NBP()
    net.conv_precision = "fp32"
    net._packed_key, net._tensors, net._graphs = ("key",), [1], {"k": 2}        # what a packed network carries (the handle aside)
    twin = copy.deepcopy(net)
    assert twin._packed is None and twin._packed_key is None and twin._tensors is None and twin._graphs == {}
    assert twin.conv_precision == "fp32" and list(twin.state_dict()) == list(net.state_dict())
    assert net._packed_key == ("key",) and net._graphs == {"k": 2}
