"""The fused per-sample objective (csrc/nbp_objective.hip: hipops.objective_forward / objective_backward, tr.ObjectiveFn,
tr.loss_weighted) against the float64 definition (nextbestpath_amd/utility/priority.py::objective_reference) on random tensors.

Bounds: per_sample and totals within 1e-5 relative (the bound NBP.loss is held to; every term is non-negative, so the sums do not
cancel), n_b exactly; d_out1 and d_out2 elementwise within 1e-5 relative plus 1e-5 of the tensor's largest magnitude.  Each test
prints the worst ratio error / bound it met (a ratio of 1 is the bound)."""
import functools
import types

import numpy as np
import pytest
import torch

from nextbestpath_amd import _lib
from nextbestpath_amd.networks import training as tr
from nextbestpath_amd.utility import hipops
from nextbestpath_amd.utility import priority as P

pytestmark = pytest.mark.gpu

REL = 1e-5
SHAPES = [(1, 16, 8), (3, 32, 8), (4, 48, 8)]        # S^2 = 2304 is not a multiple of 1024: several workgroups per plane and a ragged last pass
COUNTS = {1: [70], 2: [3, 9], 3: [0, 70, 5], 4: [0, 70, 5, 40]}      # a sample without rows, one with more rows than a wave has lanes


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def _case(B, S, C, extremes=True, seed=0, V=None):
    """(out1, coords_bcxy, gains, out2, gt): per sample distinct cells but for ONE cell named twice (in the sample with the most
    rows), one row out of range, the rows shuffled across the samples; with `extremes` out2 holds exact 0.0 and 1.0 against labels
    of both values."""
    rng = np.random.default_rng(1000 * B + S + seed)
    V = S // 4 if V is None else V
    out1 = rng.normal(size=(B, C, V, V)).astype(np.float32)
    out2 = rng.uniform(1e-4, 1 - 1e-4, size=(B, 1, S, S)).astype(np.float32)
    gt = (rng.random((B, 1, S, S)) < 0.3).astype(np.float32)
    if extremes:
        out2[0, 0, 0, :4] = [0.0, 0.0, 1.0, 1.0]
        gt[0, 0, 0, :4] = [0.0, 1.0, 0.0, 1.0]
        out2[B - 1, 0, S - 1, S - 4:] = [1.0, 0.0, 1.0, 0.0]
        gt[B - 1, 0, S - 1, S - 4:] = [0.0, 0.0, 1.0, 1.0]
    rows = []
    for b, n in enumerate(COUNTS[B]):
        cells = rng.permutation(C * V * V)[:n]
        if n >= 70:
            cells[1] = cells[0]                                   # a cell named twice
        rows += [(b, c // (V * V), (c // V) % V, c % V) for c in cells]
    rows.append((B - 1, 0, V, 0))                                 # one row out of range
    coords = np.array(rows, dtype=np.int64)
    gains = rng.uniform(0, 5, len(rows)).astype(np.float32)
    perm = rng.permutation(len(rows))
    out = (out1, coords[perm], gains[perm], out2, gt)
    for a in out:
        a.setflags(write=False)
    return out


def _weights(kind, B):
    if kind == "none":
        return None
    w = np.linspace(1.0, 0.25, B).astype(np.float32)              # weights in (0, 1]
    if kind == "zero":
        w[B // 2] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def _reference(B, S, C, extremes, kind, coef):
    return P.objective_reference(*_case(B, S, C, extremes), _weights(kind, B), coef)


def _to(dev, *arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def _rel_ratio(got, want):
    """max |got - want| / (REL |want|); equal values (0 against 0 among them) count as 0"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / (REL * np.abs(want)))
    return float(r.max()) if r.size else 0.0


def _grad_ratio(got, want):
    """max |got - want| / (REL |want| + REL max |want|)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = REL * np.abs(want) + REL * np.abs(want).max()
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


def _run(case, w, coef):
    dev = _dev()
    out1, coords, gains, out2, gt, w_d = _to(dev, *case, w)
    per_sample, totals = hipops.objective_forward(out1, coords, gains, out2, gt, w_d)
    assert per_sample.dtype == torch.float64 and totals.dtype == torch.float64 and per_sample.is_cuda
    d1, d2 = hipops.objective_backward(out1, coords, gains, out2, gt, w_d, torch.tensor(coef, dtype=torch.float32, device=dev))
    assert d1.shape == out1.shape and d2.shape == out2.shape
    return tuple(t.cpu().numpy() for t in (per_sample, totals, d1, d2))


@pytest.mark.parametrize("kind", ["none", "unit", "zero"])
@pytest.mark.parametrize("extremes", [True, False])
@pytest.mark.parametrize("B,S,C", SHAPES)
def test_kernels_match_the_reference(hip, B, S, C, extremes, kind):
    coef = (0.37, 1.9)
    ref = _reference(B, S, C, extremes, kind, coef)
    per_sample, totals, d1, d2 = _run(_case(B, S, C, extremes), _weights(kind, B), coef)
    assert np.array_equal(per_sample[:, 1], ref["per_sample"][:, 1]) and per_sample[:, 1].sum() == sum(COUNTS[B])
    ratios = {"v": _rel_ratio(per_sample[:, 0], ref["per_sample"][:, 0]), "o": _rel_ratio(per_sample[:, 2], ref["per_sample"][:, 2]),
              "totals": _rel_ratio(totals, ref["totals"]), "d_out1": _grad_ratio(d1, ref["d_out1"]),
              "d_out2": _grad_ratio(d2, ref["d_out2"])}
    print("worst error / bound:", (B, S, C), extremes, kind, {k: f"{v:.3g}" for k, v in ratios.items()})
    assert all(np.isfinite(a).all() for a in (per_sample, totals, d1, d2))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    if kind == "zero":                                            # a weight of 0: the sample's planes of both gradients are zero
        b = B // 2
        assert not d1[b].any() and not d2[b].any()
    if extremes and kind == "none":                               # the -100 clamp and the 1e-12 floor were met
        assert abs(ref["d_out2"]).max() >= 1e12 * 1.9 / (B * S * S) * 0.99 and ref["per_sample"][0, 2] >= 200.0


@pytest.mark.parametrize("B,S,V", [(2, 5, 3), (2, 6, 2)])
def test_planes_that_are_no_whole_number_of_quads(hip, B, S, V):
    """S^2 = 25: every access is 4 bytes wide; S^2 = 36: whole quads, one ragged pass."""
    case = _case(B, S, 8, True, 0, V)
    w = _weights("unit", B)
    ref = P.objective_reference(*case, w, (1.0, 1.0))
    per_sample, totals, d1, d2 = _run(case, w, (1.0, 1.0))
    assert np.array_equal(per_sample[:, 1], ref["per_sample"][:, 1])
    ratios = [_rel_ratio(per_sample, ref["per_sample"]), _rel_ratio(totals, ref["totals"]), _grad_ratio(d1, ref["d_out1"]),
              _grad_ratio(d2, ref["d_out2"])]
    print("worst error / bound:", (B, S), ratios)
    assert max(ratios) <= 1.0


def test_planes_off_the_sixteen_byte_grid(hip):
    """out2 and gt four bytes past a 16-byte boundary: 4-byte accesses, same bound; the backward gives the same bits."""
    dev = _dev()
    B, S, C = 3, 32, 8
    case = _case(B, S, C)
    out1, coords, gains, out2, gt = _to(dev, *case)
    n = out2.numel()
    o2 = torch.empty(n + 4, dtype=torch.float32, device=dev)[1:n + 1].view(out2.shape).copy_(out2)
    g2 = torch.empty(n + 4, dtype=torch.float32, device=dev)[1:n + 1].view(gt.shape).copy_(gt)
    assert o2.data_ptr() % 16 == 4 and o2.is_contiguous()
    ref = _reference(B, S, C, True, "none", (1.0, 1.0))
    ps, tot = hipops.objective_forward(out1, coords, gains, o2, g2)
    assert _rel_ratio(ps.cpu().numpy(), ref["per_sample"]) <= 1.0 and _rel_ratio(tot.cpu().numpy(), ref["totals"]) <= 1.0
    coef = torch.ones(2, dtype=torch.float32, device=dev)
    a = hipops.objective_backward(out1, coords, gains, out2, gt, None, coef)
    b = hipops.objective_backward(out1, coords, gains, o2, g2, None, coef)
    assert torch.equal(a[1], b[1]) and _grad_ratio(a[0].cpu().numpy(), ref["d_out1"]) <= 1.0


def test_no_rows_at_all(hip):
    dev = _dev()
    B, S, C = 3, 32, 8
    out1, _, _, out2, gt = _case(B, S, C)
    none = (np.zeros((0, 4), np.int64), np.zeros(0, np.float32))
    ref = P.objective_reference(out1, *none, out2, gt)
    per_sample, totals, d1, d2 = _run((out1, *none, out2, gt), None, (1.0, 1.0))
    assert not per_sample[:, :2].any() and totals[0] == 0.0 and not d1.any()
    assert _rel_ratio(per_sample[:, 2], ref["per_sample"][:, 2]) <= 1.0 and _grad_ratio(d2, ref["d_out2"]) <= 1.0
    o1, o2, g = _to(dev, out1, out2, gt)
    mse, bce, _ = tr.ObjectiveFn.apply(o1, o2, torch.zeros(0, 4, dtype=torch.int64, device=dev), torch.zeros(0, device=dev), g, None)
    assert mse.item() == 0.0 and bce.item() == pytest.approx(ref["bce"], rel=REL)


def _net(dev):
    return types.SimpleNamespace(log_vars=torch.nn.Parameter(torch.tensor([0.3, -0.2], device=dev)))


@pytest.mark.parametrize("B,S,C", SHAPES)
def test_objective_fn_is_the_existing_path_without_weights(hip, B, S, C):
    """tr.loss_weighted(weights=None) against gather_values + tr.loss on the same tensors: the loss within 1e-5 relative, the three
    gradients within the gradient bound; the outputs have the documented types."""
    dev = _dev()
    out1, coords, gains, out2, gt = _to(dev, *_case(B, S, C, False))
    bidx, cxy = coords[:, 0].contiguous(), coords[:, 1:].contiguous()
    V = out1.shape[-1]
    ok = (cxy[:, 1] < V)                                          # (the existing path's caller range-checks the rows: _collate)
    bidx, cxy, gains = bidx[ok], cxy[ok].contiguous(), gains[ok]
    res = []
    for fused in (False, True):
        net = _net(dev)
        o1, o2 = out1.clone().requires_grad_(True), out2.clone().requires_grad_(True)
        if fused:
            loss, per_sample = tr.loss_weighted(net, o1, bidx, cxy, gains, o2, gt)
            assert per_sample.shape == (B, 3) and per_sample.dtype == torch.float64 and not per_sample.requires_grad
        else:
            loss = tr.loss(net, tr.gather_values(o1, bidx, cxy), gains, o2, gt)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        loss.backward()
        res.append([t.detach().cpu().numpy() for t in (loss, o1.grad, o2.grad, net.log_vars.grad)])
    old, new = res
    ratios = [_rel_ratio(new[0], old[0])] + [_grad_ratio(n, o) for n, o in zip(new[1:], old[1:])]
    print("worst error / bound against the existing path:", (B, S, C), ratios)
    assert max(ratios) <= 1.0
    ref = P.objective_reference(*(t.cpu().numpy() for t in (out1, torch.cat([bidx.view(-1, 1), cxy], 1), gains, out2, gt)))
    want = ref["mse"] / (2 * np.exp(0.6)) + 0.3 + ref["bce"] / np.exp(-0.4) - 0.2
    assert _rel_ratio(new[0], want) <= 1.0
    mse, bce, _ = tr.ObjectiveFn.apply(out1, out2, torch.cat([bidx.view(-1, 1), cxy], 1), gains, gt, None)
    assert mse.dim() == 0 and bce.dim() == 0 and mse.dtype == torch.float32 and bce.dtype == torch.float32


def test_weighted_objective_fn_gradients(hip):
    """With weights the autograd path (ObjectiveFn through loss_weighted) gives the reference's weighted loss and gradients."""
    dev = _dev()
    B, S, C = 4, 48, 8
    case = _case(B, S, C, False)
    w = _weights("zero", B)
    out1, coords, gains, out2, gt, w_d = _to(dev, *case, w)
    net = _net(dev)
    o1, o2 = out1.clone().requires_grad_(True), out2.clone().requires_grad_(True)
    loss, _ = tr.loss_weighted(net, o1, coords[:, 0].contiguous(), coords[:, 1:].contiguous(), gains, o2, gt, w_d)
    loss.backward()
    c0, c1 = 1 / (2 * np.exp(0.6)), 1 / np.exp(-0.4)
    ref = P.objective_reference(*case, w, (c0, c1))
    assert _rel_ratio(loss.item(), c0 * ref["mse"] + 0.3 + c1 * ref["bce"] - 0.2) <= 1.0
    assert _grad_ratio(o1.grad.cpu().numpy(), ref["d_out1"]) <= 1.0 and _grad_ratio(o2.grad.cpu().numpy(), ref["d_out2"]) <= 1.0
    want_s = np.array([1 - 2 * c0 * ref["mse"], 1 - 2 * c1 * ref["bce"]])
    assert _grad_ratio(net.log_vars.grad.cpu().numpy(), want_s) <= 1.0


def test_two_runs_give_the_same_bits(hip):
    B, S, C = 4, 48, 8
    case, w = _case(B, S, C), _weights("unit", B)
    a, b = _run(case, w, (0.37, 1.9)), _run(case, w, (0.37, 1.9))
    for x, y in zip(a, b):                                        # d_out1 too: no cell is named more than twice, and a + b = b + a
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_a_samples_terms_do_not_depend_on_its_slot_or_on_the_batch(hip):
    dev = _dev()
    B, S, C = 4, 48, 8
    out1, coords, gains, out2, gt = _case(B, S, C)
    base = hipops.objective_forward(*_to(dev, out1, coords, gains, out2, gt))[0].cpu().numpy()
    # the samples in another order: sample b sits in slot perm[b]; the rows stay where they are
    perm = np.array([2, 3, 1, 0])
    inv = np.argsort(perm)
    c2 = coords.copy()
    inside = (c2[:, 0] >= 0) & (c2[:, 0] < B)
    c2[inside, 0] = perm[c2[inside, 0]]
    moved = hipops.objective_forward(*_to(dev, out1[inv], c2, gains, out2[inv], gt[inv]))[0].cpu().numpy()
    assert np.array_equal(moved[perm].view(np.uint8), base.view(np.uint8))
    # the other samples' rows elsewhere among the sample's own (which keep their order)
    b = 1
    mine = np.nonzero(coords[:, 0] == b)[0]
    others = np.nonzero(coords[:, 0] != b)[0]
    order = np.concatenate([others[::-1][:5], mine[:30], others[::-1][5:], mine[30:]])
    mixed = hipops.objective_forward(*_to(dev, out1, coords[order], gains[order], out2, gt))[0].cpu().numpy()
    assert np.array_equal(mixed[b].view(np.uint8), base[b].view(np.uint8))
    # every sample alone (B = 1), with its own rows only
    for b in range(B):
        rows = coords[:, 0] == b
        c1 = coords[rows].copy()
        c1[:, 0] = 0
        alone = hipops.objective_forward(*_to(dev, out1[b:b + 1], c1, gains[rows], out2[b:b + 1], gt[b:b + 1]))[0].cpu().numpy()
        assert np.array_equal(alone[0].view(np.uint8), base[b].view(np.uint8)), b


def test_error_codes_and_nothing_written(hip):
    dev = _dev()
    L = hip
    B, S, C = 3, 32, 8
    V = S // 4
    out1, coords, gains, out2, gt = _to(dev, *_case(B, S, C))
    K = coords.shape[0]
    assert L.nbp_objective_workspace_bytes(0, S) == 0 and L.nbp_objective_workspace_bytes(B, 0) == 0
    need = L.nbp_objective_workspace_bytes(B, S)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    per_sample = torch.full((B, 3), -7.0, dtype=torch.float64, device=dev)
    totals = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    d1, d2 = torch.full_like(out1, -7.0), torch.full_like(out2, -7.0)
    coef = torch.ones(2, dtype=torch.float32, device=dev)
    p = _lib.ptr
    st = _lib.current_stream()

    def fwd(**kw):
        a = dict(out1=p(out1), coords=p(coords), gains=p(gains), K=K, C=C, H=V, W=V, out2=p(out2), gt=p(gt), B=B, S=S, w=None,
                 ps=p(per_sample), tot=p(totals), ws=p(ws), n=need)
        a.update(kw)
        return L.nbp_objective_forward_f32(a["out1"], a["coords"], a["gains"], a["K"], a["C"], a["H"], a["W"], a["out2"], a["gt"], a["B"],
                                           a["S"], a["w"], a["ps"], a["tot"], a["ws"], a["n"], st)

    def bwd(**kw):
        a = dict(out1=p(out1), coords=p(coords), gains=p(gains), K=K, C=C, H=V, W=V, out2=p(out2), gt=p(gt), B=B, S=S, w=None,
                 coef=p(coef), d1=p(d1), d2=p(d2), ws=p(ws), n=need)
        a.update(kw)
        return L.nbp_objective_backward_f32(a["out1"], a["coords"], a["gains"], a["K"], a["C"], a["H"], a["W"], a["out2"], a["gt"],
                                            a["B"], a["S"], a["w"], a["coef"], a["d1"], a["d2"], a["ws"], a["n"], st)

    E_ARG, E_WS = -1, -2
    for f, names in ((fwd, ("out1", "coords", "gains", "out2", "gt", "ps", "tot", "ws")),
                     (bwd, ("out1", "coords", "gains", "out2", "gt", "coef", "d1", "d2", "ws"))):
        for name in names:
            assert f(**{name: None}) == E_ARG, name
        assert f(B=0) == E_ARG and f(K=-1) == E_ARG and f(S=0) == E_ARG
        assert f(n=need - 1) == E_WS and f(n=0) == E_WS
    torch.cuda.synchronize()
    for t in (per_sample, totals, d1, d2):
        assert bool((t == -7.0).all())
    # K = 0 needs neither coords nor gains
    assert fwd(K=0, coords=None, gains=None) == 0 and bwd(K=0, coords=None, gains=None) == 0
    torch.cuda.synchronize()
    assert not bool((per_sample == -7.0).any()) and not bool(d1.any()) and not bool((d2 == -7.0).any())
    # the Python layers refuse what the kernels cannot take
    with pytest.raises(RuntimeError):
        hipops.objective_forward(out1.cpu(), coords, gains, out2, gt)
    with pytest.raises(ValueError):
        hipops.objective_forward(out1, coords[:, :3].contiguous(), gains, out2, gt)
    with pytest.raises(ValueError):
        hipops.objective_backward(out1, coords, gains, out2, gt, None, coef.double())
