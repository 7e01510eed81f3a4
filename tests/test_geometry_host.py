"""CPU tests of the geometry layer (reference ``tfep/utils/geometry.py``, ``tfep/utils/math.py``): the public names and
their signatures, the C ABI symbols, the host-side validation of the index tables, the golden fixture, and the functions
that are plain torch expressions against the reference's float64 results.  No kernel is launched."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import golden_util as gu
from tfep_amd import _lib, ops
from tfep_amd.utils import geometry, math as tmath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reference's signatures (tfep/utils/geometry.py, tfep/utils/math.py); internal_coordinates is this package's own
SIGNATURES = {
    geometry: {
        'pdist': '(x, pairs=None, return_diff=False)',
        'vector_vector_angle': '(x1, x2)',
        'vector_plane_angle': '(x, plane)',
        'proper_dihedral_angle': '(x1, x2, x3)',
        'rotation_matrix_3d': '(angles, directions)',
        'batchwise_rotate': '(x, rotation_matrices, inverse=False)',
        'cartesian_to_polar': '(x, y, return_log_det_J=False)',
        'polar_to_cartesian': '(r, angle, return_log_det_J=False)',
        'internal_coordinates': '(x, pairs=None, triples=None, quads=None)',
    },
    tmath: {
        'batchwise_dot': '(x1, x2, keepdim=False)',
        'batchwise_outer': '(x1, x2)',
        'cov': '(x, ddof=1, dim_sample=0, inplace=False, return_mean=False)',
        'batch_autograd_jacobian': '(x, y, **grad_kwargs)',
        'batch_autograd_log_abs_det_J': '(x, y, **grad_kwargs)',
    },
}
SYMBOLS = [f'tfep_{name}{sfx}' for name in ('internal_coordinates', 'internal_coordinates_backward', 'polar', 'polar_backward')
           for sfx in ('', '_f64')]


def _plain(signature):
    """The signature without annotations."""
    return '(' + ', '.join(str(p.replace(annotation=inspect.Parameter.empty)) for p in signature.parameters.values()) + ')'


@pytest.mark.parametrize('module', list(SIGNATURES), ids=lambda m: m.__name__)
def test_public_names_have_the_reference_signatures(module):
    for name, expected in SIGNATURES[module].items():
        assert _plain(inspect.signature(getattr(module, name))) == expected, name


def test_symbols_are_bound_and_declared():
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    declared = set(re.findall(r'\b(tfep_[a-z0-9_]+)\s*\(', header))
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert name in declared, name
    f32, f64 = (_lib._SIGNATURES['tfep_internal_coordinates_backward' + s] for s in ('', '_f64'))
    assert f32 == f64


def test_ops_are_registered():
    from tfep_amd import torch_ops
    assert torch_ops.GEOMETRY_OPS == ('internal_coordinates', 'internal_coordinates_backward', 'polar_forward',
                                      'polar_backward')
    for name in torch_ops.GEOMETRY_OPS:
        assert hasattr(torch.ops.tfep, name)


@pytest.mark.parametrize('kind, n_rows', [('pairs', 2), ('triples', 3), ('quads', 4)])
def test_index_validation(kind, n_rows):
    n = 7
    good = torch.arange(n_rows).unsqueeze(1).repeat(1, 3)
    for bad_value in (-1, n):
        bad = good.clone()
        bad[n_rows - 1, 1] = bad_value
        with pytest.raises(ValueError, match='outside'):
            ops.index_tables(**{kind: bad}, **_others(kind), n_atoms=n, device='cpu')
        # the public entry point validates before anything touches a device
        with pytest.raises(ValueError, match='outside'):
            geometry.internal_coordinates(torch.zeros(2, n, 3), **{kind: bad})
    with pytest.raises(ValueError, match='shape'):
        ops.index_tables(**{kind: torch.zeros(n_rows + 1, 3, dtype=torch.int64)}, **_others(kind), n_atoms=n, device='cpu')
    with pytest.raises(ValueError, match='shape'):
        ops.index_tables(**{kind: torch.zeros(3, dtype=torch.int64)}, **_others(kind), n_atoms=n, device='cpu')
    with pytest.raises(ValueError, match='integer'):
        ops.index_tables(**{kind: good.double()}, **_others(kind), n_atoms=n, device='cpu')
    with pytest.raises(ValueError, match='outside'):
        geometry.pdist(torch.zeros(2, n, 3), pairs=torch.tensor([[0], [n]]))


def _others(kind):
    return {k: None for k in ('pairs', 'triples', 'quads') if k != kind}


def test_incidence_list_is_in_table_order():
    """Every atom's items: the entries it appears in, pairs then triples then quads, each as 4 * entry + slot."""
    g = gu.load('geometry.npz')
    tables = [torch.from_numpy(g[f'hub/{k}']) for k in ('pairs', 'triples', 'quads')]
    pairs, triples, quads, start, items = ops.index_tables(*tables, n_atoms=7, device='cpu')
    assert all(t.dtype == torch.int32 for t in (pairs, triples, quads, start, items))
    flat = [(int(t[s, e]), 4 * (off + e) + s) for t, off in zip(tables, (0, 6, 11)) for e in range(t.shape[1])
            for s in range(t.shape[0])]
    for atom in range(7):
        expected = sorted(item for a, item in flat if a == atom)
        assert items[start[atom]:start[atom + 1]].tolist() == expected
    assert int(start[-1]) == len(flat) == items.numel()
    assert int(start[4]) - int(start[3]) == 6 + 5 + 5          # atom 3 is in every entry
    # the same tensor objects again: the prepared tables come from the cache
    assert ops.index_tables(*tables, n_atoms=7, device='cpu')[3] is start
    empty = ops.index_tables(None, None, None, n_atoms=7, device='cpu')
    assert [tuple(t.shape) for t in empty] == [(2, 0), (3, 0), (4, 0), (8,), (0,)]


def test_golden_loads_with_the_expected_keys():
    g = gu.load('geometry.npz')
    assert g['x'].shape == (11, 7, 3) and g['x'].dtype == np.float64
    for case in ('main', 'hub'):
        for k in ('pairs', 'triples', 'quads', 'd', 'a', 't', 'gd', 'ga', 'gt', 'gx', 'f32/d', 'f32/a', 'f32/t', 'f32/gx'):
            assert f'{case}/{k}' in g.files, (case, k)
        assert g[f'{case}/gx'].shape == (11, 7, 3) and g[f'{case}/f32/gx'].dtype == np.float32
        # the condition the generator asserts: no angle near 0 or pi
        assert np.abs(np.sin(g[f'{case}/a'])).min() >= 0.1
    assert (g['hub/pairs'] == 3).any(0).all() and (g['hub/triples'] == 3).any(0).all() and (g['hub/quads'] == 3).any(0).all()
    for name in ('cartesian_to_polar', 'polar_to_cartesian'):
        assert {f'{name}/{k}' for k in ('in0', 'in1', 'out0', 'out1', 'out2', 'cot0', 'cot1', 'cot2', 'g0', 'g1')} <= set(g.files)
    assert os.path.getsize(os.path.join(gu.GOLDEN, 'geometry.npz')) < 256 * 1024


# ------------------------------------------------------------------ the torch expressions, float64 on the CPU

def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).requires_grad_(grad)


def _close(got, ref, tol=1e-12):
    rel, _ = gu.err_stats(got.detach().numpy(), ref)
    assert rel <= tol, rel


@pytest.mark.parametrize('name', ['vector_vector_angle', 'vector_plane_angle', 'proper_dihedral_angle'])
def test_vector_functions_match_the_reference(name):
    g = gu.load('geometry.npz')
    inputs = [_t(g[f'{name}/in{i}'], grad=True) for i in range(3 if name == 'proper_dihedral_angle' else 2)]
    out = getattr(geometry, name)(*inputs)
    _close(out, g[f'{name}/out'])
    grads = torch.autograd.grad((out * _t(g[f'{name}/cot'])).sum(), inputs)
    for i, gr in enumerate(grads):
        _close(gr, g[f'{name}/g{i}'], 1e-11)


def test_pdist_with_diff_matches_the_reference():
    g = gu.load('geometry.npz')
    d, diff = geometry.pdist(_t(g['x']), pairs=_t(g['main/pairs']), return_diff=True)
    _close(d, g['pdist_diff/d'])
    _close(diff, g['pdist_diff/diff'])
    _close(geometry.pdist(_t(g['x']), return_diff=True)[0], g['pdist_all/d'])


@pytest.mark.parametrize('name', ['rotation_batch', 'rotation_single'])
def test_rotation_matrix_3d_matches_the_reference(name):
    g = gu.load('geometry.npz')
    angles, directions = _t(g[f'{name}/angles'], grad=True), _t(g[f'{name}/directions'], grad=True)
    R = geometry.rotation_matrix_3d(angles, directions)
    _close(R, g[f'{name}/out'])
    ga, gd = torch.autograd.grad((R * _t(g[f'{name}/cot'])).sum(), (angles, directions))
    _close(ga, g[f'{name}/g_angles'], 1e-11)
    _close(gd, g[f'{name}/g_directions'], 1e-11)


def test_math_matches_the_reference():
    g = gu.load('geometry.npz')
    a, b = _t(g['math/in0']), _t(g['math/in1'])
    _close(tmath.batchwise_dot(a, b), g['math/dot'])
    assert tmath.batchwise_dot(a, b, keepdim=True).shape == g['math/dot_keepdim'].shape
    _close(tmath.batchwise_outer(a, b), g['math/outer'])
    c0, m0 = tmath.cov(a, return_mean=True)
    c1, m1 = tmath.cov(a, ddof=0, dim_sample=1, return_mean=True)
    for got, key in ((c0, 'cov0'), (m0, 'mean0'), (c1, 'cov1'), (m1, 'mean1')):
        assert got.shape == g[f'math/{key}'].shape
        _close(got, g[f'math/{key}'])
    _close(tmath.cov(a), g['math/cov0'])
    centred = a.clone()
    tmath.cov(centred, inplace=True)
    _close(centred, (a - a.mean(0)).numpy())
    with pytest.raises(ValueError):
        tmath.cov(a[0])
    with pytest.raises(ValueError):
        tmath.cov(a, dim_sample=2)
    z = a.clone().requires_grad_(True)
    y = torch.tanh(z @ _t(g['math/w'])) + 2.0 * z
    _close(tmath.batch_autograd_jacobian(z, y, retain_graph=True), g['math/jacobian'])
    _close(tmath.batch_autograd_log_abs_det_J(z, y), g['math/log_abs_det_J'])
