"""The Z-matrix placement kernels (csrc/zmatrix.hip) against the plain float64 reference of tests/zmatrix_ref.py on its
three cases (one level of two lane passes, a 40-level chain, a shuffled tree whose fixed atoms are no prefix), in float32
and float64: values, log-det and gradients, the round trip through ``cartesian_to_zmatrix``, independence of the batch bit
for bit, a strided input, opcheck, and ``ZMatrixFlow``.

Bounds, those of tests/test_gpu_geometry.py.  float64: relative L2 <= 1e-10.  float32: nothing fixed in advance -- the
bound of a quantity is 4 x the relative L2 error of the REFERENCE run in float32 on the same (rounded) inputs against its
float64 run.  Dihedrals are compared as (sin, cos).  Every figure is printed before it is asserted.
"""
import os
import sys

import numpy as np
import pytest
import torch

import geometry_ref as gr
import zmatrix_ref as zr
from tfep_amd import ops
from tfep_amd.utils import geometry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32, F64 = torch.float32, torch.float64
TOL64 = 1e-10
dtypes = pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
cases = pytest.mark.parametrize('name', zr.CASES)
KEYS = ('x', 'log_det_J', 'g_d', 'g_a', 'g_t', 'g_x_fixed')


def _dev(a, dtype, grad=False):
    return torch.as_tensor(a).to('cuda', dtype).requires_grad_(grad)


def _tables(name):
    c = zr.case(name)
    return c['z_matrix'], c['fixed_atoms']


def _run(name, dtype, rows=slice(None), x_fixed=None):
    """The kernels on the rows ``rows`` of a case with the case's cotangents: a dict like ``zr.reference``, of tensors."""
    c = zr.case(name)
    args = [_dev(c[k][rows], dtype, grad=True) for k in zr.INPUTS]
    if x_fixed is not None:
        args[3] = x_fixed
    x, ldj = geometry.zmatrix_to_cartesian(*args, *_tables(name))
    grads = torch.autograd.grad([x, ldj], args, [_dev(c['cx'][rows], dtype).reshape(x.shape), _dev(c['cl'][rows], dtype)])
    return dict(zip(KEYS, (x, ldj, *grads)))


def _np(t):
    return t.detach().cpu().numpy()


def _assert_close(what, got, ref, ref32, dtype, wrap=np.asarray):
    """``got`` against the float64 reference ``ref``: 1e-10 in float64, 4 x the reference's own float32 error in float32."""
    got = _np(got)
    rel = zr.rel_l2(wrap(got), wrap(ref))
    bound = TOL64 if dtype == F64 else 4.0 * zr.rel_l2(wrap(ref32), wrap(ref))
    print(f'{what} {dtype}: rel L2 {rel:.3e} (bound {bound:.3e})')
    assert got.dtype == (np.float64 if dtype == F64 else np.float32)
    assert rel <= bound, (what, rel, bound)


def _references(name, dtype):
    """The float64 reference on the inputs a run in ``dtype`` sees, and the float32 reference on the same inputs."""
    rounded = dtype == F32
    return zr.reference(name, rounded=rounded), zr.reference(name, rounded=True, dtype=F32)


@dtypes
@cases
def test_values_and_log_det_match_the_reference(name, dtype):
    got, (ref, ref32) = _run(name, dtype), _references(name, dtype)
    assert got['x'].shape == ref['x'].shape and got['log_det_J'].shape == (zr.B,)
    for k in ('x', 'log_det_J'):
        _assert_close(f'{name} {k}', got[k], ref[k], ref32[k], dtype)


@dtypes
@cases
def test_gradients_match_the_reference(name, dtype):
    got, (ref, ref32) = _run(name, dtype), _references(name, dtype)
    for k in ('g_d', 'g_a', 'g_t', 'g_x_fixed'):
        _assert_close(f'{name} {k}', got[k], ref[k], ref32[k], dtype)


def _reference_round_trip(name, dtype):
    """The reference's own round trip in ``dtype`` on the rounded inputs: place, then the reference internal coordinates."""
    c = zr.case(name)
    z = c['z_matrix']
    d, a, t, x_fixed = (v.to(dtype) for v in zr.inputs(name, rounded=True))
    x, ldj = zr.place(d, a, t, x_fixed, z, c['fixed_atoms'])
    d2, a2, t2 = gr.internal_coordinates(x, z[:, :2].t(), z[:, :3].t(), z.t())
    ldj2 = -(2.0 * torch.log(d2) + torch.log(torch.abs(torch.sin(a2)))).sum(1)
    return {'d': d2, 'a': a2, 't': t2, 'x_fixed': x[:, c['fixed_atoms']], 'log_det_J': ldj, 'minus_back': -ldj2}


@dtypes
@cases
def test_round_trip(name, dtype):
    c = zr.case(name)
    start = dict(zip(zr.INPUTS, zr.inputs(name, rounded=dtype == F32)))
    x, ldj = geometry.zmatrix_to_cartesian(*(_dev(start[k], dtype) for k in zr.INPUTS), *_tables(name))
    d, a, t, x_fixed, ldj_back = geometry.cartesian_to_zmatrix(x, *_tables(name))
    assert x_fixed.shape == (zr.B, len(c['fixed_atoms']), 3) and d.shape == a.shape == t.shape == start['d'].shape
    ref32 = {k: v.to(F64).numpy() for k, v in _reference_round_trip(name, F32).items()}
    for k, got in (('d', d), ('a', a), ('t', t), ('x_fixed', x_fixed)):
        _assert_close(f'{name} round trip {k}', got, start[k].numpy(), ref32[k], dtype, zr.circ if k == 't' else np.asarray)
    # the two log-dets cancel
    diff = float((ldj + ldj_back).abs().max())
    print(f'{name} {dtype}: max |log_det_J + log_det_J back| = {diff:.3e}')
    if dtype == F64:
        assert diff <= 1e-9
    else:
        _assert_close(f'{name} minus the log-det back', -ldj_back, _np(ldj).astype(np.float64),
                      ref32['minus_back'] - ref32['log_det_J'] + _np(ldj), dtype)
    # the flat layout gives the same bits
    flat = geometry.zmatrix_to_cartesian(*(_dev(start[k], dtype) for k in zr.INPUTS[:3]),
                                         _dev(start['x_fixed'], dtype).reshape(zr.B, -1), *_tables(name))
    assert flat[0].shape == (zr.B, x.shape[1] * 3) and torch.equal(flat[0].reshape(x.shape), x) and torch.equal(flat[1], ldj)
    again = geometry.cartesian_to_zmatrix(flat[0], *_tables(name))
    assert again[3].shape == (zr.B, 3 * len(c['fixed_atoms'])) and torch.equal(again[0], d) and torch.equal(again[4], ldj_back)


@dtypes
@cases
def test_bits_do_not_depend_on_the_batch_and_are_reproducible(name, dtype):
    """Row 4 of the batch of 6 (the first wave of the second workgroup when four rows share one, with two idle waves
    beside it) against the same row run alone, values and gradients; and the same call twice."""
    first, again, alone = _run(name, dtype), _run(name, dtype), _run(name, dtype, rows=slice(4, 5))
    for k in KEYS:
        assert torch.equal(first[k], again[k]), k
        assert alone[k].shape[0] == 1 and torch.equal(first[k][4:5], alone[k]), k


@dtypes
def test_strided_input_is_read_in_place(dtype):
    name = 'tree'
    c = zr.case(name)
    wide = torch.zeros(zr.B, 24, device='cuda', dtype=dtype)
    wide[:, 5:20] = _dev(c['x_fixed'].reshape(zr.B, -1), dtype)
    x_fixed = wide[:, 5:20].requires_grad_(True)
    assert x_fixed.stride(0) == 24 and not x_fixed.is_contiguous()
    plain, strided = _run(name, dtype), _run(name, dtype, x_fixed=x_fixed)
    for k in KEYS:
        assert torch.equal(plain[k].reshape(strided[k].shape), strided[k]), k
    # (d, a, t) as column slices of one tensor, as a flow hands them over
    mixed = torch.cat([_dev(c[k], dtype) for k in ('d', 'a', 't')], dim=1)
    d, a, t = torch.split(mixed, 60, dim=1)
    assert not a.is_contiguous()
    x, ldj = geometry.zmatrix_to_cartesian(d, a, t, _dev(c['x_fixed'], dtype), *_tables(name))
    assert torch.equal(x, plain['x']) and torch.equal(ldj, plain['log_det_J'])


@dtypes
def test_opcheck_and_dtype_contract(dtype):
    name = 'tree'
    c = zr.case(name)
    tables = ops.zmatrix_tables(*_tables(name), 65, 'cuda')
    args = lambda grad: [_dev(c[k].reshape(zr.B, -1), dtype, grad=grad) for k in zr.INPUTS]
    t = torch.ops.tfep
    torch.library.opcheck(t.zmatrix_place.default, (*args(True), *tables))
    d, a, tt, x_fixed = args(False)
    x, _ = t.zmatrix_place(d, a, tt, x_fixed, *tables)
    torch.library.opcheck(t.zmatrix_place_backward.default,
                          (x, d, a, tt, *tables, _dev(c['cx'].reshape(zr.B, -1), dtype), _dev(c['cl'], dtype)))
    other = F64 if dtype == F32 else F32
    with pytest.raises(TypeError):
        geometry.zmatrix_to_cartesian(d, a.to(other), tt, x_fixed, *_tables(name))
    with pytest.raises(TypeError):
        t.zmatrix_place_backward(x, d, a, tt, *tables, _dev(c['cx'].reshape(zr.B, -1), other), _dev(c['cl'], dtype))
    from tfep_amd._lib import TfepHipError
    with pytest.raises(TfepHipError, match='no CPU fallback'):
        geometry.zmatrix_to_cartesian(d, a, tt.cpu(), x_fixed, *_tables(name))
    with pytest.raises(TfepHipError, match='no CPU fallback'):
        geometry.cartesian_to_zmatrix(x.cpu(), *_tables(name))


# ------------------------------------------------------------------ the flow

def _flow():
    """``ZMatrixFlow`` around the 2-layer affine MAF of tools/check_flow_log_det.py on the 195 mixed coordinates of ``tree``,
    its parameters scaled down so that the inner flow stays near the identity and the angles inside (0, pi)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        from check_flow_log_det import small_maf
    finally:
        sys.path.pop(0)
    from tfep_amd.nn.flows import ZMatrixFlow
    flow = ZMatrixFlow(small_maf(D=3 * 65, seed=7), *_tables('tree')).to('cuda')
    with torch.no_grad():
        for p in flow.parameters():
            p.mul_(0.1)
    return flow


def test_zmatrix_flow_inverts_and_its_log_det_is_the_autograd_one():
    from tfep_amd.utils.math import batch_autograd_log_abs_det_J
    flow = _flow()
    x = _dev(zr.reference('tree')['x'][:3].reshape(3, -1), F64, grad=True)
    # the setup: what the inner flow makes of the internal coordinates is still a valid set of them
    d, a, t, x_fixed, _ = geometry.cartesian_to_zmatrix(x.detach(), *_tables('tree'))
    mixed = flow.flow(torch.cat([d, a, t, x_fixed], dim=1))[0].detach()
    print(f'inner flow: d in [{float(mixed[:, :60].min()):.3f}, {float(mixed[:, :60].max()):.3f}], '
          f'a in [{float(mixed[:, 60:120].min()):.3f}, {float(mixed[:, 60:120].max()):.3f}]')
    assert float(mixed[:, :60].min()) > 0.5 and 0.3 < float(mixed[:, 60:120].min()) and float(mixed[:, 60:120].max()) < 2.8
    y, ldj = flow(x)
    assert y.shape == x.shape and ldj.shape == (3,)
    print(f'max |y - x| = {float((y - x).detach().abs().max()):.3e}')
    assert float((y - x).detach().abs().max()) > 1e-4                      # the inner flow does move the atoms
    ref = batch_autograd_log_abs_det_J(x, y, retain_graph=True)
    err = float((ldj - ref).abs().max())
    print(f'max |log_det_J - autograd| = {err:.3e}')
    assert err <= 1e-8
    x_back, ldj_back = flow.inverse(y.detach())
    err_x, err_l = float((x_back - x).abs().max()), float((ldj_back + ldj).abs().max())
    print(f'inverse(forward(x)): max |dx| = {err_x:.3e}, max |log-det sum| = {err_l:.3e}')
    assert err_x <= 1e-9 and err_l <= 1e-8
    (y.square().sum() - ldj.sum()).backward()
    grads = [p.grad for p in flow.flow.parameters()]
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads) and x.grad is not None
