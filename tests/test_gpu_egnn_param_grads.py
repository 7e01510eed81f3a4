"""Parameter gradients of the EGNN velocity on the kernels (csrc/egnn_param_grad.hip, ``EGNNDynamics.vjp_parameters``, the
opt-in ``kernel_backward`` autograd route) against the float64 oracle's ``autograd.grad`` on the cases of
``egnn_cases.py``: every feature tile, padded ``F != G``, ragged last blocks, pruning cutoffs, 1 / 2 / 3 layers, B = 1, 2, 3.

Bound per parameter tensor: relative L2 ``max(1e-5, 4 x the float32 oracle's own distance from the float64 one)``
(``egnn_param_grad_cases.bound``; the host test states the condition).  Every figure is printed before it is asserted.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import egnn_cases as ec
import egnn_param_grad_cases as pc

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize('name', ec.NAMES)
SPLIT = pytest.mark.parametrize('split', [True, False], ids=['split-f16', 'exact-fp32'])


def _dynamics(name, split):
    dyn = ec.dynamics(name).cuda()
    dyn.split_gemm = split
    return dyn


@functools.lru_cache(maxsize=None)
def _run(name, split, max_workgroups=0):
    """``vjp_parameters`` of a case with ``g = v``, once per (case, arithmetic, cap); host copies, left unchanged."""
    c = ec.case(name)
    vel, gx, grads = _dynamics(name, split).vjp_parameters(c['t'], c['x'].cuda(), c['v'].cuda(), max_workgroups=max_workgroups)
    torch.cuda.synchronize()
    return vel.cpu(), gx.cpu(), {k: v.cpu() for k, v in grads.items()}


def _check_against_oracle(name, grads, what):
    ref = pc.oracle_param_grads(name)
    unused = pc.unused_names(name)
    assert set(grads) == set(pc.parameter_names(name))
    failures = []
    for k in pc.parameter_names(name):
        got = grads[k].numpy().astype(np.float64)
        if k in unused:
            assert ref[k] is None and not got.any(), k            # exact zeros
            continue
        assert got.shape == ref[k].shape and np.isfinite(got).all(), k
        bound, e32 = pc.bound(name, k)
        e = ec.rel_l2(got, ref[k])
        print(f'{name} {what} {k}: rel L2 {e:.2e} (float32 oracle {e32:.2e}, bound {bound:.1e})')
        if not e <= bound:
            failures.append((k, e, bound))
    assert not failures, failures


# ------------------------------------------------------------------ 1. every case against the float64 oracle
@CASES
@SPLIT
def test_gradients_match_the_float64_oracle(name, split):
    _check_against_oracle(name, _run(name, split)[2], 'split-f16' if split else 'exact-fp32')


# ------------------------------------------------------------------ 2. items per workgroup
@pytest.mark.parametrize('name', ['n41_t2', 'n260_l1'])
def test_items_per_workgroup(name):
    """``max_workgroups`` = 1, 2, 3 and the default: within the oracle bound, bit-reproducible, and within 1e-6 of each other
    (``n260_l1`` with one workgroup is the case that needs the edge pass's second summation level: one fp32 running sum
    over its 34 items was 1.3e-6 from the default grid)."""
    c = ec.case(name)
    dyn = _dynamics(name, False)
    x, v = c['x'].cuda(), c['v'].cuda()
    runs = {}
    for cap in (1, 2, 3, 0):
        first = dyn.vjp_parameters(c['t'], x, v, max_workgroups=cap)[2]
        again = dyn.vjp_parameters(c['t'], x, v, max_workgroups=cap)[2]
        for k in first:
            assert torch.equal(first[k], again[k]), (cap, k)          # no atomics: bit-reproducible
        runs[cap] = {k: t.cpu() for k, t in first.items()}
        _check_against_oracle(name, runs[cap], f'max_workgroups={cap}')
    for cap in (1, 2, 3):
        for k in pc.parameter_names(name):
            if k in pc.unused_names(name):
                continue
            e = ec.rel_l2(runs[cap][k].numpy(), runs[0][k].numpy())
            print(f'{name} max_workgroups={cap} against the default, {k}: rel L2 {e:.2e}')
            assert e <= 1e-6, (cap, k)                                # only the grouping of the fp32 sums differs


# ------------------------------------------------------------------ 3. consistency with what exists
@SPLIT
def test_velocity_and_position_cotangent_are_those_of_the_existing_routes(split):
    name = 'n41_t2'
    c = ec.case(name)
    dyn = _dynamics(name, split)
    x, v = c['x'].cuda(), c['v'].cuda()
    vel, gx, _ = dyn.vjp_parameters(c['t'], x, v)
    with torch.no_grad():
        assert torch.equal(vel, dyn(c['t'], x))
    assert torch.equal(gx, dyn.vjp(c['t'], x, v)[1])


def test_linear_in_the_cotangent():
    name = 'n33_t2full'
    c = ec.case(name)
    dyn = _dynamics(name, False)
    x, g1 = c['x'].cuda(), c['v'].cuda()
    g2 = torch.randn(g1.shape, generator=torch.Generator().manual_seed(5)).cuda()
    a, b, ab = (dyn.vjp_parameters(c['t'], x, g)[2] for g in (g1, g2, g1 + g2))
    for k in pc.parameter_names(name):
        if k in pc.unused_names(name):
            continue
        e = ec.rel_l2(ab[k].cpu().numpy(), (a[k].double() + b[k].double()).cpu().numpy())
        print(f'{name} {k}: grads(g1 + g2) against grads(g1) + grads(g2): rel L2 {e:.2e}')
        assert e <= 1e-5, k


# ------------------------------------------------------------------ 4. finite differences, no autograd anywhere
def test_central_differences_of_the_float64_oracle():
    """One entry each of a weight matrix, a bias and a ``_log_gammas`` tensor, tensor and entry drawn by seed among the
    entries whose reference gradient is at least the tensor's RMS (a relative tolerance says nothing at an entry whose
    gradient is zero to rounding)."""
    name, h = 'n17_t1', 1e-6
    c = ec.case(name)
    grads = _run(name, False)[2]
    ref = pc.oracle_param_grads(name)
    rng = np.random.default_rng(7)
    live = [k for k in pc.parameter_names(name) if k not in pc.unused_names(name)]
    groups = ([k for k in live if k.endswith('.weight')], [k for k in live if k.endswith('.bias')],
              [k for k in live if k.endswith('_log_gammas')])
    for group in groups:
        k = group[rng.integers(len(group))]
        r = ref[k]
        big = np.argwhere(np.abs(r) >= np.sqrt((r ** 2).mean()))
        idx = tuple(big[rng.integers(len(big))])
        vals = []
        for sign in (1.0, -1.0):
            sd = {kk: p.clone() for kk, p in c['sd64'].items()}
            sd[k][idx] += sign * h
            vals.append(float(pc.oracle_value(name, sd, c['v'])))
        fd = (vals[0] - vals[1]) / (2 * h)
        got = float(grads[k][idx])
        print(f'{name} {k}{idx}: kernels {got:.8e}, central difference {fd:.8e}, autograd reference {r[idx]:.8e}')
        assert abs(got - fd) <= 1e-4 * abs(fd), (k, idx)


# ------------------------------------------------------------------ 5. the autograd route
SECOND_ORDER = 'kernel_backward = False'


def test_kernel_backward_route():
    name = 'n33_t2full'
    c = ec.case(name)
    dyn = _dynamics(name, False)
    dyn.kernel_backward = True
    x, g = c['x'].cuda().requires_grad_(True), c['v'].cuda()
    _, gx, grads = dyn.vjp_parameters(c['t'], x.detach(), g)
    (dyn(c['t'], x) * g).sum().backward()
    unused = pc.unused_names(name)
    for k, p in dyn.named_parameters():
        if k in unused:
            assert p.grad is None, k
        else:
            assert torch.equal(p.grad, grads[k]), k
    assert torch.equal(x.grad, gx)
    # second order: refused, with the way out
    vel = dyn(c['t'], x)
    first = torch.autograd.grad((vel * vel).sum(), [p for k, p in dyn.named_parameters() if k not in unused], create_graph=True)
    with pytest.raises(RuntimeError, match=SECOND_ORDER):
        sum((f * f).sum() for f in first).backward()


def test_default_route_is_torch_forward_and_agrees(monkeypatch):
    name = 'n33_t2full'
    c = ec.case(name)
    dyn = _dynamics(name, False)
    assert dyn.kernel_backward is False
    calls = []
    original = dyn.torch_forward
    monkeypatch.setattr(dyn, 'torch_forward', lambda t, x: (calls.append(1), original(t, x))[1])
    (dyn(c['t'], c['x'].cuda()) * c['v'].cuda()).sum().backward()
    assert len(calls) == 1
    unused = pc.unused_names(name)
    assert all(p.grad is None for k, p in dyn.named_parameters() if k in unused)
    _check_against_oracle(name, {k: (torch.zeros_like(p) if k in unused else p.grad).detach().cpu()
                                 for k, p in dyn.named_parameters()}, 'torch_forward')
    _check_against_oracle(name, _run(name, False)[2], 'kernels')


# ------------------------------------------------------------------ 6. training
def test_training_smoke():
    name = 'n17_t1'
    c = ec.case(name)
    x = c['x'].cuda()
    u = 0.1 * torch.randn(x.shape, generator=torch.Generator().manual_seed(11)).cuda()
    start = _dynamics(name, False)
    final = {}
    for flag in (True, False):
        dyn = copy.deepcopy(start)
        dyn.kernel_backward = flag
        opt = torch.optim.AdamW(dyn.parameters(), lr=1e-3)
        losses = []
        for _ in range(10):
            opt.zero_grad()
            loss = (dyn(c['t'], x) - u).square().sum()
            loss.backward()
            opt.step()
            losses.append(float(loss))
        print(f'kernel_backward={flag}: loss {losses[0]:.6e} -> {losses[-1]:.6e}')
        assert losses[-1] < losses[0]
        final[flag] = losses[-1]
    assert abs(final[True] - final[False]) <= 1e-3 * abs(final[False])


def test_continuous_flow_over_a_flagged_module_stays_on_torch_forward(monkeypatch):
    from tfep_amd.nn.flows import ContinuousFlow
    name = 'n17_t1'
    c = ec.case(name)
    dyn = _dynamics(name, False)
    dyn.kernel_backward = True
    calls = []
    original = dyn.torch_forward
    monkeypatch.setattr(dyn, 'torch_forward', lambda t, x: (calls.append(1), original(t, x))[1])
    flow = ContinuousFlow(dyn, trace_estimator='hutchinson', solver='euler', solver_options={'step_size': 0.5},
                          regularization=False)
    opt = torch.optim.AdamW(flow.parameters(), lr=1e-3)
    y, trace = flow(c['x'].cuda())
    (y.square().sum() - trace.sum()).backward()              # differentiates the trace: second derivatives of the dynamics
    opt.step()
    assert len(calls) == 2
    live = [p for k, p in dyn.named_parameters() if k not in pc.unused_names(name)]
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in live)


# ------------------------------------------------------------------ 7. empty batch and errors
def test_empty_batch_and_errors():
    name = 'n17_t1'
    c = ec.case(name)
    dyn = _dynamics(name, None)
    x, v = c['x'].cuda(), c['v'].cuda()
    vel, gx, grads = dyn.vjp_parameters(c['t'], x[:0], v[:0])
    assert vel.shape == gx.shape == (0, x.shape[1])
    assert set(grads) == set(pc.parameter_names(name))
    assert all(g.shape == p.shape and g.dtype == torch.float32 and not g.any() for g, p in
               ((grads[k], p) for k, p in dyn.named_parameters()))
    with pytest.raises(ValueError, match='shape'):
        dyn.vjp_parameters(c['t'], x, v[:, :-3])
    with pytest.raises(TypeError, match='float32'):
        dyn.vjp_parameters(c['t'], x.double(), v)
    wide = ec.dynamics(name)
    wide._dims = (wide._dims[0], 80, wide._dims[2])
    assert not wide.kernels_supported()
    with pytest.raises(NotImplementedError, match='<= 64'):
        wide.vjp_parameters(c['t'], x, v)
