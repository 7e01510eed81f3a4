"""The relative-frame kernels (csrc/relframe.hip) and ``CartesianToMixedFlow`` against the plain reference of
tests/relframe_ref.py on its cases (no other atom, two lane passes, the 9 + 60 atom mixed system), under all 8 settings of
``remove_ref_rototranslation``, in float32 and float64: values, ``origin``, ``R``, log-det and every gradient, kept and
removed DOFs, the rotation by pi, the round trip, independence of the batch bit for bit, strided inputs, opcheck and the
error contract, and the flow around an identity, a fixed element-wise flow and a spline MAF.

Bounds, those of tests/test_gpu_zmatrix.py.  float64: relative L2 <= 1e-10.  float32: nothing fixed in advance -- the
bound of a quantity is 4 x the relative L2 error of the REFERENCE run in float32 on the same (rounded) inputs against its
float64 run.  Every figure is printed before it is asserted.
"""
import math

import numpy as np
import pytest
import torch

import relframe_ref as rr
from tfep_amd.nn.flows import CartesianToMixedFlow
from tfep_amd.utils import geometry

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
TOL64 = 1e-10
dtypes = pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
cases = pytest.mark.parametrize('name', rr.CASES)
removes = pytest.mark.parametrize('remove', rr.REMOVES, ids=lambda r: ''.join('TF'[not f] for f in r))
ENCODE_KEYS = ('coords', 'origin', 'R', 'ldj', 'g_x')
DECODE_KEYS = ('x', 'ldj_back', 'g_coords', 'g_origin', 'g_R')


def _dev(a, dtype, grad=False):
    return torch.as_tensor(a).to('cuda', dtype).requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


def _assert_close(what, got, ref, ref32, dtype):
    """``got`` against the float64 reference ``ref``: 1e-10 in float64, 4 x the reference's own float32 error in float32."""
    got = _np(got)
    rel = rr.rel_l2(got.reshape(ref.shape), ref)
    bound = TOL64 if dtype == F64 else 4.0 * rr.rel_l2(ref32, ref)
    print(f'{what} {dtype}: rel L2 {rel:.3e} (bound {bound:.3e})')
    assert got.dtype == (np.float64 if dtype == F64 else np.float32)
    assert rel <= bound, (what, rel, bound)


def _references(name, remove, dtype):
    """The float64 reference on the inputs a run in ``dtype`` sees, and the float32 reference on the same inputs."""
    return rr.reference(name, remove, rounded=dtype == F32), rr.reference(name, remove, rounded=True, dtype=F32)


def _run_encode(name, remove, dtype, rows=slice(None), x=None):
    cot = rr.cotangents(name, remove)
    if x is None:
        x = _dev(rr.case(name)['x_cart'][rows], dtype, grad=True)
    outs = geometry.cartesian_to_relative_frame(x, remove)
    (g_x,) = torch.autograd.grad(outs, x, [_dev(cot[k][rows], dtype) for k in ('coords', 'origin', 'R', 'ldj')])
    return dict(zip(ENCODE_KEYS, (*outs, g_x)))


def _run_decode(name, remove, dtype, rows=slice(None), coords=None):
    cot = rr.cotangents(name, remove)
    args = [_dev(t[rows], dtype, grad=True) for t in rr.decode_inputs(name, remove, rounded=False)]
    if coords is not None:
        args[0] = coords
    outs = geometry.relative_frame_to_cartesian(*args, remove)
    grads = torch.autograd.grad(outs, args, [_dev(cot[k][rows], dtype) for k in ('x', 'ldj_back')])
    return dict(zip(DECODE_KEYS, (*outs, *grads)))


# ------------------------------------------------------------------ the two maps

@dtypes
@removes
@cases
def test_encode_matches_the_reference(name, remove, dtype):
    got, (ref, ref32) = _run_encode(name, remove, dtype), _references(name, remove, dtype)
    n_c = rr.case(name)['x_cart'].shape[1]
    assert got['coords'].shape == (rr.B, rr.width(n_c, remove)) and got['R'].shape == (rr.B, 3, 3)
    assert got['origin'].shape == (rr.B, 3) and got['ldj'].shape == (rr.B,) and got['g_x'].shape == (rr.B, n_c, 3)
    for k in ENCODE_KEYS:
        _assert_close(f'{name} encode {k}', got[k], ref[k], ref32[k], dtype)
    # the kept reference DOFs are zero up to round-off; the origin's exactly
    kept = _np(got['coords'])[:, rr.width(n_c, remove) - rr.n_kept(remove):]
    scale = float(rr.case(name)['x_cart'].abs().max())
    print(f'{name} kept DOFs {dtype}: max abs {np.abs(kept).max() if kept.size else 0.0:.3e} (|x| {scale:.3f})')
    if dtype == F64 and kept.size:
        assert np.abs(kept).max() <= 1e-12 * scale
    if not remove[0]:
        assert np.all(kept[:, :3] == 0.0)


@dtypes
@removes
@cases
def test_decode_matches_the_reference(name, remove, dtype):
    got, (ref, ref32) = _run_decode(name, remove, dtype), _references(name, remove, dtype)
    n_c = rr.case(name)['x_cart'].shape[1]
    assert got['x'].shape == (rr.B, n_c, 3) and got['g_R'].shape == (rr.B, 3, 3) and got['g_origin'].shape == (rr.B, 3)
    for k in DECODE_KEYS:
        _assert_close(f'{name} decode {k}', got[k], ref[k], ref32[k], dtype)


@dtypes
@removes
def test_removed_dofs_are_exact_zeros_after_decode(remove, dtype):
    """With the identity for ``R`` and a zero origin the positions are the frame coordinates themselves."""
    coords, _, _ = (_dev(t, dtype) for t in rr.decode_inputs('mixed', remove, rounded=False))
    eye = torch.eye(3, device='cuda', dtype=dtype).expand(rr.B, 3, 3).contiguous()
    x, _ = geometry.relative_frame_to_cartesian(coords, torch.zeros(rr.B, 3, device='cuda', dtype=dtype), eye, remove)
    origin, axis, plane = x[:, -3], x[:, -2], x[:, -1]
    assert torch.equal(axis[:, 0], coords[:, 0])
    for removed, values in zip(remove, (origin, axis[:, 1:], plane[:, 2:])):
        assert bool((values == 0).all()) == removed, (remove, values)


@dtypes
def test_the_rotation_by_pi(dtype):
    x = rr.pi_case()
    remove = (False, False, False)
    ref = [t.numpy() for t in rr.encode(x, remove)]
    ref32 = [t.to(F64).numpy() for t in rr.encode(x.to(F32), remove)]
    got = geometry.cartesian_to_relative_frame(_dev(x, dtype), remove)
    for k, g, r, r32 in zip(('coords', 'origin', 'R', 'ldj'), got, ref, ref32):
        _assert_close(f'pi {k}', g, r, r32, dtype)
    R = _np(got[2]).astype(np.float64)
    print(f'R of the row with the axis vector (-2, 0, 0):\n{R[1]}')
    assert np.abs(R[1, 0] - np.array([-1.0, 0.0, 0.0])).max() <= 4e-16 and abs(float(got[0][1, 0]) - 2.0) <= 1e-15
    if dtype == F64:
        ortho = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max()
        det = np.abs(np.linalg.det(R) - 1.0).max()
        print(f'max |R R^T - I| = {ortho:.3e}, max |det R - 1| = {det:.3e}')
        assert ortho <= 1e-14 and det <= 1e-14
    # the gradient exists on that row: nothing reaches the axis atom through R1, the rest is finite
    xg = _dev(x, dtype, grad=True)
    outs = geometry.cartesian_to_relative_frame(xg, remove)
    (g,) = torch.autograd.grad(sum(o.sum() for o in outs), xg)
    assert bool(torch.isfinite(g).all())


@dtypes
@removes
@cases
def test_round_trip_on_the_device(name, remove, dtype):
    x = rr.case(name)['x_cart']
    x = x.to(F32).to(F64) if dtype == F32 else x
    coords, origin, R, ldj = geometry.cartesian_to_relative_frame(_dev(x, dtype), remove)
    x_back, ldj_back = geometry.relative_frame_to_cartesian(coords, origin, R, remove)
    x32 = x.to(F32)
    ref32 = rr.decode(*rr.encode(x32, remove)[:3], remove)[0].to(F64).numpy()
    _assert_close(f'{name} decode(encode(x))', x_back, x.numpy(), ref32, dtype)
    total = float((ldj + ldj_back).abs().max())
    bound = 1e-10 * max(1.0, float(ldj.abs().max()))
    print(f'{name} {dtype}: max |log-det sum| = {total:.3e} (float64 bound {bound:.3e})')
    if dtype == F64:
        assert total <= bound
    else:
        enc32 = rr.encode(x32, remove)
        ref_total = float((enc32[3] + rr.decode(*enc32[:3], remove)[1]).abs().max())
        print(f'  reference in float32: {ref_total:.3e}')
        assert total <= 4.0 * max(ref_total, 2.0 ** -23 * float(ldj.abs().max()))


@dtypes
def test_many_rows(dtype):
    """4099 rows: past one pass of any grid the launch could be folded into; values only."""
    x = rr.many_case()
    x = x.to(F32).to(F64) if dtype == F32 else x
    remove = (True, False, True)
    ref, ref32 = rr.encode(x, remove), rr.encode(x.to(F32), remove)
    got = geometry.cartesian_to_relative_frame(_dev(x, dtype), remove)
    for k, g, r, r32 in zip(('coords', 'origin', 'R', 'ldj'), got, ref, ref32):
        # (the normalised angle of a row may sit at the cut of atan2: compare it on the circle)
        if k == 'coords':
            wrap = lambda c: np.concatenate([np.cos(2 * np.pi * c[:, 2:3]), np.sin(2 * np.pi * c[:, 2:3]), c[:, :2], c[:, 3:]], 1)
            rel = rr.rel_l2(wrap(_np(g).astype(np.float64)), wrap(r.numpy()))
            bound = TOL64 if dtype == F64 else 4.0 * rr.rel_l2(wrap(r32.to(F64).numpy()), wrap(r.numpy()))
            print(f'many coords {dtype}: rel L2 {rel:.3e} (bound {bound:.3e})')
            assert rel <= bound
        else:
            _assert_close(f'many {k}', g, r.numpy(), r32.to(F64).numpy(), dtype)
    back, ldj_back = geometry.relative_frame_to_cartesian(*got[:3], remove)
    _assert_close('many decode(encode(x))', back, x.numpy(),
                  rr.decode(*ref32[:3], remove)[0].to(F64).numpy(), dtype)


@dtypes
@cases
def test_bits_do_not_depend_on_the_batch_and_are_reproducible(name, dtype):
    remove = (False, True, False)
    for run, keys in ((_run_encode, ENCODE_KEYS), (_run_decode, DECODE_KEYS)):
        first, again, alone = run(name, remove, dtype), run(name, remove, dtype), run(name, remove, dtype, rows=slice(0, 3))
        for k in keys:
            assert torch.equal(first[k], again[k]), k
            assert alone[k].shape[0] == 3 and torch.equal(first[k][:3], alone[k]), k


@dtypes
def test_strided_inputs_are_read_in_place(dtype):
    name, remove = 'wide', (True, False, False)
    x = rr.case(name)['x_cart'].reshape(rr.B, -1)
    wide = torch.zeros(rr.B, x.shape[1] + 11, device='cuda', dtype=dtype)
    wide[:, 4:4 + x.shape[1]] = _dev(x, dtype)
    x_slice = wide[:, 4:4 + x.shape[1]].requires_grad_(True)
    assert x_slice.stride(0) == x.shape[1] + 11 and not x_slice.is_contiguous()
    plain, strided = _run_encode(name, remove, dtype), _run_encode(name, remove, dtype, x=x_slice)
    for k in ENCODE_KEYS:
        assert torch.equal(plain[k].reshape(strided[k].shape), strided[k]), k
    coords = rr.decode_inputs(name, remove, rounded=False)[0]
    mixed = torch.cat([torch.zeros(rr.B, 7, dtype=F64), coords, torch.zeros(rr.B, 2, dtype=F64)], 1)
    c_slice = _dev(mixed, dtype)[:, 7:7 + coords.shape[1]].requires_grad_(True)
    assert not c_slice.is_contiguous()
    plain, strided = _run_decode(name, remove, dtype), _run_decode(name, remove, dtype, coords=c_slice)
    for k in DECODE_KEYS:
        assert torch.equal(plain[k], strided[k]), k


@dtypes
def test_opcheck_and_the_error_contract(dtype):
    name, remove = 'mixed', (False, True, False)
    t = torch.ops.tfep
    cot = rr.cotangents(name, remove)
    x = _dev(rr.case(name)['x_cart'].reshape(rr.B, -1), dtype)
    torch.library.opcheck(t.relative_frame_encode.default, (x.clone().requires_grad_(True), *remove))
    coords, origin, R, ldj = t.relative_frame_encode(x, *remove)
    g = [_dev(cot[k].reshape(rr.B, -1) if cot[k].dim() > 1 else cot[k], dtype) for k in ('coords', 'origin', 'R', 'ldj')]
    torch.library.opcheck(t.relative_frame_encode_backward.default, (x, *remove, *g))
    torch.library.opcheck(t.relative_frame_decode.default,
                          (*(v.clone().requires_grad_(True) for v in (coords, origin, R)), *remove))
    gx, gl = _dev(cot['x'].reshape(rr.B, -1), dtype), _dev(cot['ldj_back'], dtype)
    torch.library.opcheck(t.relative_frame_decode_backward.default, (coords, origin, R, *remove, gx, gl))
    other = F64 if dtype == F32 else F32
    with pytest.raises(TypeError):
        t.relative_frame_decode(coords, origin.to(other), R, *remove)
    with pytest.raises(TypeError):
        geometry.relative_frame_to_cartesian(coords, origin, R.to(other), remove)
    with pytest.raises(TypeError):
        t.relative_frame_encode_backward(x, *remove, g[0], g[1].to(other), g[2], g[3])
    with pytest.raises(TypeError):
        t.relative_frame_decode_backward(coords, origin, R, *remove, gx.to(other), gl)
    with pytest.raises(ValueError, match='n_c >= 3'):
        t.relative_frame_encode(x[:, :6].contiguous(), *remove)
    with pytest.raises(ValueError, match='coords has'):
        t.relative_frame_decode(coords, origin, R, True, True, True)              # 4 kept columns too many: no 3 n
    with pytest.raises(ValueError, match='coords has'):
        t.relative_frame_decode(coords[:, :2].contiguous(), origin, R, *remove)
    with pytest.raises(ValueError, match='grad_coords'):
        t.relative_frame_encode_backward(x, *remove, g[0][:, :-1].contiguous(), g[1], g[2], g[3])
    from tfep_amd._lib import TfepHipError
    with pytest.raises(TfepHipError, match='no CPU fallback'):
        geometry.relative_frame_to_cartesian(coords, origin.cpu(), R, remove)


# ------------------------------------------------------------------ the flow

class _Identity(torch.nn.Module):
    def forward(self, x):
        return x, torch.zeros(len(x), dtype=x.dtype, device=x.device)

    inverse = forward


class _Fixed(torch.nn.Module):
    """The fixed element-wise flow of relframe_ref: distance-type columns times 1.02, plain Cartesian columns plus 0.05."""

    def __init__(self, by_type):
        super().__init__()
        self.by_type = {k: by_type[k].tolist() for k in ('distances', 'cartesians')}

    def forward(self, y):
        return rr.fixed_inner(y, self.by_type)

    def inverse(self, y):
        scale, shift = torch.ones(y.shape[1], dtype=y.dtype), torch.zeros(y.shape[1], dtype=y.dtype)
        scale[self.by_type['distances']] = 1.02
        shift[self.by_type['cartesians']] = 0.05
        log_det = torch.full((len(y),), -len(self.by_type['distances']) * math.log(1.02), dtype=y.dtype, device=y.device)
        return (y - shift.to(y.device)) / scale.to(y.device), log_det


def _mixed_flow(inner, remove):
    c = rr.case('mixed')
    return CartesianToMixedFlow(inner, c['cartesian'], c['z_matrix'], c['reference'], list(remove)).to('cuda')


def _round_trip_bound(x, remove, dtype):
    """The reference's own float32 round trip through the whole change, as (float64 values, max |log-det sum|)."""
    c = rr.case('mixed')
    y, ldj = rr.mixed_flow(x.to(F32), c['z_matrix'], c['ordered'], remove, lambda m: (m, torch.zeros(len(m))))
    return y.to(F64).numpy(), float(ldj.abs().max())


@dtypes
@removes
def test_flow_around_the_identity(remove, dtype):
    c = rr.case('mixed')
    flow = _mixed_flow(_Identity(), remove)
    assert flow.cartesian_atom_indices.tolist() == c['ordered'].tolist() and flow.n_dofs_out == 3 * 69 - 6 + rr.n_kept(remove)
    x = c['x'].to(F32).to(F64) if dtype == F32 else c['x']
    y, ldj = flow(_dev(x.reshape(rr.B, -1), dtype))
    assert y.shape == (rr.B, 3 * 69) and ldj.shape == (rr.B,)
    ref32, ref32_ldj = _round_trip_bound(x, remove, dtype)
    _assert_close('identity flow y', y, x.reshape(rr.B, -1).numpy(), ref32.reshape(rr.B, -1), dtype)
    parts = flow.cartesian_to_mixed(_dev(x.reshape(rr.B, -1), dtype))
    total, scale = float(ldj.abs().max()), max(1.0, float(parts[1].abs().max()))
    print(f'identity flow {dtype}: max |log_det_J| = {total:.3e} (log-det of the way in {scale:.3f}; reference in float32 '
          f'{ref32_ldj:.3e})')
    assert total <= (1e-10 * scale if dtype == F64 else 4.0 * max(ref32_ldj, 2.0 ** -23 * scale))
    # the mixed coordinates themselves: the normalised angles and torsions are in [0, 1], the layout is the reference's
    mixed = parts[0]
    assert mixed.shape == (rr.B, flow.n_dofs_out)
    assert float(mixed[:, 60:180].min()) >= 0.0 and float(mixed[:, 60:180].max()) <= 1.0
    ref_mixed = rr.to_mixed(x, c['z_matrix'], c['ordered'], remove)[0]
    ref32_mixed = rr.to_mixed(x.to(F32), c['z_matrix'], c['ordered'], remove)[0].to(F64)
    _assert_close('mixed coordinates', mixed, ref_mixed.numpy(), ref32_mixed.numpy(), dtype)
    # the 3-D layout gives the same bits
    y3, ldj3 = flow(_dev(x, dtype))
    assert y3.shape == (rr.B, 69, 3) and torch.equal(y3.reshape(rr.B, -1), y) and torch.equal(ldj3, ldj)


@dtypes
@removes
def test_flow_around_a_fixed_elementwise_flow(remove, dtype):
    c, cot = rr.case('mixed'), rr.cotangents('mixed', remove)
    flow = _mixed_flow(_Identity(), remove)
    flow.flow = _Fixed(flow.get_dof_indices_by_type())
    assert {k: v for k, v in flow.flow.by_type.items()} == rr.columns_by_type(60, 9, remove)
    ref, ref32 = rr.flow_reference(remove, rounded=dtype == F32), rr.flow_reference(remove, rounded=True, dtype=F32)
    x = _dev((c['x'].to(F32).to(F64) if dtype == F32 else c['x']).reshape(rr.B, -1), dtype, grad=True)
    y, ldj = flow(x)
    (g_x,) = torch.autograd.grad([y, ldj], x, [_dev(cot['flow_x'].reshape(rr.B, -1), dtype), _dev(cot['flow_ldj'], dtype)])
    for k, got in (('y', y), ('log_det_J', ldj), ('g_x', g_x)):
        _assert_close(f'fixed flow {k}', got, ref[k], ref32[k], dtype)
    assert float((y - x).detach().abs().max()) > 1e-3                       # the wrapped flow does move the atoms
    x_back, ldj_back = flow.inverse(y.detach())
    x32 = c['x'].to(F32)
    by_type = rr.columns_by_type(60, 9, remove)
    fwd32 = rr.mixed_flow(x32, c['z_matrix'], c['ordered'], remove, lambda m: rr.fixed_inner(m, by_type))[0]
    back32 = rr.mixed_flow(fwd32, c['z_matrix'], c['ordered'], remove, lambda m: _Fixed.inverse(flow.flow, m))[0]
    _assert_close('inverse(forward(x))', x_back, _np(x).astype(np.float64), back32.to(F64).reshape(rr.B, -1).numpy(), dtype)
    total = float((ldj.detach() + ldj_back).abs().max())
    print(f'max |log-det sum| = {total:.3e}')
    if dtype == F64:
        assert total <= 1e-10 * max(1.0, float(ldj.detach().abs().max()))


@dtypes
def test_flow_around_a_spline_maf_round_trips_and_trains(dtype):
    """A 2-layer MAF with a neural spline over [0, 1] on the normalised angles and torsions (a102n among them)."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF, PartialFlow, SequentialFlow
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    remove = (True, True, True)
    c = rr.case('mixed')
    flow = _mixed_flow(_Identity(), remove)
    by_type = flow.get_dof_indices_by_type()
    mapped = sorted(by_type['angles'].tolist() + by_type['torsions'].tolist())
    fixed = [i for i in range(flow.n_dofs_out) if i not in set(mapped)]
    D = len(mapped)
    assert D == 121
    torch.manual_seed(3)
    maf = SequentialFlow(*[MAF(generate_degrees(D, order), transformer=NeuralSplineTransformer(torch.zeros(D), torch.ones(D), 5),
                               initialize_identity=False) for order in ('ascending', 'descending')])
    flow.flow = PartialFlow(maf.to(dtype), fixed_indices=fixed).to('cuda')
    x = _dev(c['x'].reshape(rr.B, -1), dtype, grad=True)
    y, ldj = flow(x)
    assert float((y - x).detach().abs().max()) > 1e-3
    x_back, ldj_back = flow.inverse(y.detach())
    err_x, err_l = float((x_back - x).detach().abs().max()), float((ldj_back + ldj).detach().abs().max())
    print(f'spline MAF {dtype}: inverse(forward(x)) max |dx| = {err_x:.3e}, max |log-det sum| = {err_l:.3e}')
    assert err_x <= (1e-9 if dtype == F64 else 1e-5)
    loss = y.square().sum() - ldj.sum()
    loss.backward()
    grads = [p.grad for p in flow.parameters()]
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads) and bool(torch.isfinite(x.grad).all())
