"""The Z-matrix placement kernels (csrc/zmatrix.hip) against the plain float64 reference of tests/zmatrix_ref.py on its
three cases (one level of two lane passes, a 40-level chain, a shuffled tree whose fixed atoms are no prefix), in float32
and float64: values, log-det and gradients, the round trip through ``cartesian_to_zmatrix``, independence of the batch bit
for bit, a strided input, opcheck, and ``ZMatrixFlow``.

Bounds, those of tests/test_gpu_geometry.py.  float64: relative L2 <= 1e-10.  float32: nothing fixed in advance -- the
bound of a quantity is 4 x the relative L2 error of the REFERENCE run in float32 on the same (rounded) inputs against its
float64 run.  Dihedrals are compared as (sin, cos).  Every figure is printed before it is asserted.
"""
import pytest
import torch

import zmatrix_ref as zr
from tfep_amd import ops
from tfep_amd.utils import geometry

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
dtypes = pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
cases = pytest.mark.parametrize('name', zr.CASES)
# the runs of the kernels and the comparison at the bounds above: shared with tests/test_gpu_zmatrix_tiers.py
KEYS, _dev, _tables, _run, _references, _assert_close = zr.KEYS, zr.dev, zr.tables, zr.run, zr.references, zr.assert_close


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


@dtypes
@cases
def test_round_trip(name, dtype):
    zr.check_round_trip(name, dtype)


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

def test_zmatrix_flow_inverts_and_its_log_det_is_the_autograd_one():
    from tfep_amd.utils.math import batch_autograd_log_abs_det_J
    flow = zr.flow('tree')
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
