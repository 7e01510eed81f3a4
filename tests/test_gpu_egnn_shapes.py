"""The EGNN kernels (csrc/egnn.hip) at every feature tile and at ragged atom counts, against the float64 oracle
(oracle/egnn.py) on the cases of ``egnn_cases.py``: tile 1, tile 2 with and without feature padding, the 3 -> 4 promotion;
two to seventeen destination blocks with a short last one; grids of 2, 4, 6, 9 and 34 workgroups for the XCD remap; three
layers and the single-layer route; forward, J v and v^T J (both reverse edge passes) on the split-f16 and the exact-fp32
chain.  The conditions the cases rest on are asserted on the host (``test_egnn_cases_host.py``).

Bounds, those of ``test_gpu_continuous.py``: relative L2 <= 1e-5 for the velocity, J v and v^T J, over the whole tensor and
over the atoms of the short last block alone; ``1e-5 max(sum |terms|, 1)`` for the traces; ``rtol = 1e-4, atol = 1e-7`` for
the squared norms.  Every figure is printed before it is asserted, with the float32 oracle's own distance from the
float64 one beside it.
"""
import functools

import numpy as np
import pytest
import torch

import egnn_cases as ec

pytestmark = pytest.mark.gpu

REL = 1e-5
SCALE = 0.5                 # of the terms added to the accumulators
FILL = 1.25                 # what trace and velocity_squared_norm hold before the call (frobenius: see _fills)

CASES = pytest.mark.parametrize('name', ec.NAMES)
SPLIT = pytest.mark.parametrize('split', [True, False], ids=['split-f16', 'exact-fp32'])


def _dynamics(name, split):
    dyn = ec.dynamics(name).cuda()
    dyn.split_gemm = split
    return dyn


def _fills(name):
    """The constants ``(trace, frobenius, velocity_squared_norm)`` hold before the call.  ``frobenius += SCALE |J v|^2`` is
    checked to ``rtol = 1e-4`` of the sum, so what was there has the size of what is added (the power of two nearest to it):
    neither is then lost in the other's tolerance."""
    added = SCALE * float((ec.reference(name)['jv'] ** 2).sum(1).mean())
    return FILL, float(2.0 ** round(np.log2(added))), FILL


def _products(dyn, name, t, x, v):
    """Everything one case needs from the kernels: the three velocities, J v, v^T J and both sets of accumulators."""
    B = x.shape[0]
    acc_f, acc_r = ([torch.full((B,), f, device='cuda') for f in _fills(name)] for _ in range(2))
    with torch.no_grad():
        vel = dyn(t, x)
        vel_f, jv = dyn.jvp(t, x, v, trace=acc_f[0], frobenius=acc_f[1], scale=SCALE, velocity_squared_norm=acc_f[2])
        vel_r, vj = dyn.vjp(t, x, v, trace=acc_r[0], frobenius=acc_r[1], scale=SCALE, velocity_squared_norm=acc_r[2])
    return dict(vel=vel, vel_f=vel_f, jv=jv, vel_r=vel_r, vj=vj, acc_f=acc_f, acc_r=acc_r)


@functools.lru_cache(maxsize=None)
def _run(name, split):
    """The kernels on the whole batch of a case, once per (case, arithmetic chain); host copies, left unchanged."""
    c = ec.case(name)
    out = _products(_dynamics(name, split), name, c['t'], c['x'].cuda(), c['v'].cuda())
    torch.cuda.synchronize()
    return {k: ([a.cpu() for a in o] if isinstance(o, list) else o.cpu()) for k, o in out.items()}


def _last_block(c):
    return slice(3 * 16 * (c['n_blk'] - 1), 3 * c['n'])


def _check_rel(name, split, what, got, key):
    """Relative L2 of ``got`` against the float64 oracle, whole tensor and the atoms of the short last block."""
    c = ec.case(name)
    r64, r32 = ec.reference(name)[key], ec.reference(name, torch.float32)[key]
    got = got.numpy().astype(np.float64)
    lb = _last_block(c)
    e, e32 = ec.rel_l2(got, r64), ec.rel_l2(r32, r64)
    e_lb, e32_lb = ec.rel_l2(got[:, lb], r64[:, lb]), ec.rel_l2(r32[:, lb], r64[:, lb])
    chain = 'split-f16' if split else 'exact-fp32'
    print(f'{name} {chain} {what}: rel L2 {e:.2e} (float32 oracle {e32:.2e}); atoms {16 * (c["n_blk"] - 1)}..{c["n"] - 1} of '
          f'the last block {e_lb:.2e} (float32 oracle {e32_lb:.2e})')
    assert np.isfinite(got).all()
    assert e <= REL
    assert e_lb <= REL


@CASES
def test_case_lands_on_its_tile(name):
    c = ec.case(name)
    assert _dynamics(name, None)._tile() == ec.TILES[name][1] == ec.tile(c['F'], c['G'])     # as asserted on the host
    assert _dynamics(name, None).kernels_supported()


@SPLIT
@CASES
def test_velocity(name, split):
    out = _run(name, split)
    _check_rel(name, split, 'velocity', out['vel'], 'vel')
    assert torch.equal(out['vel_f'], out['vel'])                          # the tangent does not perturb the primal
    assert torch.equal(out['vel_r'], out['vel'])                          # nor does keeping every layer's inputs
    c = ec.case(name)
    assert float(out['vel'].reshape(c['B'], c['n'], 3).sum(1).abs().max()) < 1e-5      # centre of geometry preserved


def _check_accumulators(name, split, what, acc, key):
    """``trace = fill + SCALE v . prod``, ``frobenius = fill + SCALE |prod|^2`` (added to what was there),
    ``velocity_squared_norm = |vel|^2`` (overwritten)."""
    c = ec.case(name)
    ref = ec.reference(name)
    v = c['v'].double().numpy()
    fill_t, fill_f, fill_v = _fills(name)
    trace, frob, vsq = (a.numpy().astype(np.float64) for a in acc)
    terms = SCALE * ref[key] * v
    tr_ref, bound = fill_t + terms.sum(1), 1e-5 * np.maximum(np.abs(terms).sum(1), 1.0)
    fr_add = SCALE * (ref[key] ** 2).sum(1)
    fr_ref = fill_f + fr_add
    vs_ref = (ref['vel'] ** 2).sum(1)
    # the reference tells "scale x the term added" and "overwritten" from their neighbours: leaving the fill out, adding it
    # where it is overwritten, or a scale of 1 would each miss the bounds below
    assert np.all(fill_t > 2 * bound) and np.any(np.abs(terms.sum(1)) > 2 * bound)
    assert np.all(fill_f > 1e-3 * fr_ref) and np.all(fr_add > 1e-3 * fr_ref) and np.all(fill_v > 1e-3 * vs_ref)
    chain = 'split-f16' if split else 'exact-fp32'
    print(f'{name} {chain} {what}: trace error / bound {np.abs(trace - tr_ref).max():.2e} / {bound.min():.2e}, '
          f'frobenius rel {np.abs(frob / fr_ref - 1).max():.2e}, |vel|^2 rel {np.abs(vsq / vs_ref - 1).max():.2e}; '
          f'traces {tr_ref}, frobenius {fr_ref}, |vel|^2 {vs_ref}')
    assert np.all(np.abs(trace - tr_ref) <= bound)
    np.testing.assert_allclose(frob, fr_ref, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(vsq, vs_ref, rtol=1e-4, atol=1e-7)
    return trace


@SPLIT
@CASES
def test_jvp_and_its_accumulators(name, split):
    out = _run(name, split)
    _check_rel(name, split, 'J v', out['jv'], 'jv')
    _check_accumulators(name, split, 'jvp', out['acc_f'], 'jv')


@SPLIT
@CASES
def test_vjp_and_its_accumulators(name, split):
    out = _run(name, split)
    _check_rel(name, split, 'v^T J', out['vj'], 'vj')
    tr_r = _check_accumulators(name, split, 'vjp', out['acc_r'], 'vj')
    # the forward-mode and the reverse-mode trace are the same number: v . (J v) == (v^T J) . v
    c = ec.case(name)
    tr_f = out['acc_f'][0].numpy().astype(np.float64)
    terms = np.abs(SCALE * ec.reference(name)['vj'] * c['v'].double().numpy()).sum(1)
    atol = 1e-4 * np.maximum(terms, 1.0)
    print(f'{name}: forward trace {tr_f}, reverse trace {tr_r}, atol {atol}')
    assert np.all(np.abs(tr_f - tr_r) <= atol + 1e-4 * np.abs(tr_r))


@SPLIT
@CASES
def test_last_row_alone_reproduces_its_row_of_the_batch(name, split):
    """Rows are independent and the reductions have a fixed order: which sample a workgroup reads (``blk / n_blk`` after the
    XCD remap) changes with the grid, the numbers must not."""
    c = ec.case(name)
    out = _run(name, split)
    alone = _products(_dynamics(name, split), name, c['t'], c['x'][-1:].clone().cuda(), c['v'][-1:].clone().cuda())
    for k in ('vel', 'vel_f', 'jv', 'vel_r', 'vj'):
        assert torch.equal(alone[k].cpu(), out[k][-1:]), k                # (B = 1: the same call twice)
    for k in ('acc_f', 'acc_r'):
        for a, b in zip(alone[k], out[k]):
            assert torch.equal(a.cpu(), b[-1:]), k


@SPLIT
def test_swapping_two_atoms_across_destination_blocks_swaps_their_velocities(split):
    """Two atoms of one type, one in the first destination block and one in the short last one, trade places: every
    workgroup must read the 16 Q rows and positions of ITS block for the velocities to trade places with them."""
    name = 'n41_t2'
    c = ec.case(name)
    n, B = c['n'], c['B']
    i, j = 1, 40
    types = c['kwargs']['node_types']
    assert types[i] == types[j] and i < 16 and j >= 16 * (c['n_blk'] - 1)
    perm = list(range(n))
    perm[i], perm[j] = j, i
    xp = c['x'].reshape(B, n, 3)[:, perm].reshape(B, -1).contiguous()
    with torch.no_grad():
        vel_p = _dynamics(name, split)(c['t'], xp.cuda()).cpu()
    vel = _run(name, split)['vel']
    want = vel.reshape(B, n, 3)[:, perm].reshape(B, -1)
    print(f'{name}: max |vel(P x) - P vel(x)| = {float((vel_p - want).abs().max()):.2e}; the two atoms move by '
          f'{float((vel.reshape(B, n, 3)[:, i] - vel.reshape(B, n, 3)[:, j]).abs().max()):.2e}')
    assert torch.allclose(vel_p, want, rtol=0, atol=2e-5)
    assert float((vel.reshape(B, n, 3)[:, i] - vel.reshape(B, n, 3)[:, j]).abs().max()) > 1e-2    # the swap is visible
