"""CPU tests of the geometry layer (reference ``tfep/utils/geometry.py``, ``tfep/utils/math.py``): the public names and
their signatures, the C ABI symbols, the host-side validation of the index tables, the golden fixture, and the functions
that are plain torch expressions against the reference's float64 results; the plain float64 restatement of the kernels
that the GPU tests compare with (tests/geometry_ref.py) against the same results; the table cache; and the per-entry
arithmetic of csrc/geometry.h, compiled for the host.  No kernel is launched."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import geometry_ref as gr
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


# ------------------------------------------------------------------ the restatement the GPU tests compare with

def _rel(got, ref, wrap=np.asarray):
    return gr.rel_l2(wrap(got), wrap(ref))


@pytest.mark.parametrize('case', ['main', 'hub'])
def test_plain_reference_matches_the_golden_internal_coordinates(case):
    """tests/geometry_ref.py is written from the header of csrc/geometry.h; here it meets the reference's own results."""
    g = gu.load('geometry.npz')
    tables = [g[f'{case}/{k}'] for k in ('pairs', 'triples', 'quads')]
    got = gr.coordinates_and_gradient(g['x'], tables, [g[f'{case}/{k}'] for k in ('gd', 'ga', 'gt')])
    for k, v, wrap in zip(('d', 'a', 't', 'gx'), got, (np.asarray, gr.circ, gr.circ, np.asarray)):
        rel = _rel(v, g[f'{case}/{k}'], wrap)
        print(f'{case} {k}: rel L2 {rel:.3e}')
        assert v.shape == g[f'{case}/{k}'].shape and rel <= 1e-12, (case, k, rel)


def test_plain_reference_matches_the_golden_distances_of_all_pairs():
    g = gu.load('geometry.npz')
    d, a, t = gr.internal_coordinates(_t(g['x']), pairs=torch.triu_indices(7, 7, offset=1))
    rel = _rel(d.numpy(), g['pdist_all/d'])
    print(f'pdist_all d: rel L2 {rel:.3e}')
    assert rel <= 1e-12 and a.shape == t.shape == (11, 0)


@pytest.mark.parametrize('name', ['cartesian_to_polar', 'polar_to_cartesian'])
def test_plain_reference_matches_the_golden_polar_maps(name):
    g = gu.load('geometry.npz')
    got = gr.polar_and_gradient(g[f'{name}/in0'], g[f'{name}/in1'], name == 'polar_to_cartesian',
                                [g[f'{name}/cot{i}'] for i in range(3)])
    for k, v in zip(('out0', 'out1', 'out2', 'g0', 'g1'), got):
        rel = _rel(v, g[f'{name}/{k}'], gr.circ if (name, k) == ('cartesian_to_polar', 'out1') else np.asarray)
        print(f'{name} {k}: rel L2 {rel:.3e}')
        assert rel <= 1e-12, (name, k, rel)


def test_wide_tables_have_the_layout_the_gpu_tests_rely_on():
    pairs, triples, quads = gr.wide_tables()
    assert [tuple(t.shape) for t in (pairs, triples, quads)] == [(2, 70), (3, 67), (4, 65)]
    for t in (pairs, triples, quads):
        assert all(len(set(col)) == t.shape[0] for col in t.t().tolist())          # distinct atoms in every entry
        assert int(t.min()) >= 0 and int(t.max()) < 125 and bool((t == 3).any())
    assert pairs[0, 0::2].eq(64).all() and pairs[1, 1::2].eq(64).all()
    assert bool(((pairs == 64).any(0) & (pairs == 11).any(0)).any())
    x, _, cots = gr.wide_case()
    assert x.shape == (6, 130, 3) and [tuple(c.shape) for c in cots] == [(6, 70), (6, 67), (6, 65)]
    min_d, min_sin, min_rejection = gr.conditioning(x, pairs, triples, quads)
    print(f'seed {gr.WIDE_SEED}: min d {min_d:.4f}, min sin(a) {min_sin:.4f}, min(|v|, |w|) {min_rejection:.4f}')
    assert min_d >= gr.MIN_D and min_sin >= gr.MIN_SIN and min_rejection >= gr.MIN_REJECTION


# ------------------------------------------------------------------ the table cache

def test_table_cache_sees_an_in_place_write():
    """The cache keys on the identity, version and shape of the tensors given: a table changed in place is prepared
    again, and validated again."""
    n = 9
    pairs = torch.tensor([[0, 1, 2], [3, 4, 5]])
    triples = torch.tensor([[0, 1], [2, 3], [4, 5]])
    first = ops.index_tables(pairs, triples, None, n_atoms=n, device='cpu')
    assert ops.index_tables(pairs, triples, None, n_atoms=n, device='cpu') is first
    pairs[1, 2] = 8
    triples[0, 1] = 7
    second = ops.index_tables(pairs, triples, None, n_atoms=n, device='cpu')
    fresh = ops.index_tables(pairs.clone(), triples.clone(), None, n_atoms=n, device='cpu')
    assert second is not first
    for got, new, old in zip(second, fresh, first):
        assert torch.equal(got, new)
    assert second[0].tolist() == [[0, 1, 2], [3, 4, 8]] and second[1][0].tolist() == [0, 7]
    start, items = second[3], second[4]
    assert items[start[8]:start[9]].tolist() == [4 * 2 + 1]                       # atom 8: pair 2, slot 1
    assert items[start[7]:start[8]].tolist() == [4 * (3 + 1) + 0]                 # atom 7: triple 1, slot 0
    assert items[start[5]:start[6]].tolist() == [4 * (3 + 1) + 2]                 # atom 5 has left pair 2
    assert not torch.equal(first[4], items)
    for bad in (n, -1):
        pairs[0, 0] = bad
        with pytest.raises(ValueError, match='outside'):
            ops.index_tables(pairs, triples, None, n_atoms=n, device='cpu')
    pairs[0, 0] = 0
    assert torch.equal(ops.index_tables(pairs, triples, None, n_atoms=n, device='cpu')[4], items)


def test_long_incidence_lists_are_in_table_order():
    """The wide tables: atom 64 has 70 items, five atoms have none, the offsets never decrease."""
    tables = gr.wide_tables()
    P, A, T = (t.shape[1] for t in tables)
    *_, start, items = ops.index_tables(*tables, n_atoms=gr.WIDE_N, device='cpu')
    assert start.shape == (gr.WIDE_N + 1,) and int(start[0]) == 0
    assert bool((start[1:] >= start[:-1]).all())
    assert int(start[-1]) == 2 * P + 3 * A + 4 * T == items.numel()
    assert start[125:].tolist() == [int(start[-1])] * 6                           # atoms 125..129 are empty
    flat = [(int(t[s, e]), 4 * (off + e) + s) for t, off in zip(tables, (0, P, P + A)) for e in range(t.shape[1])
            for s in range(t.shape[0])]
    for atom in range(gr.WIDE_N):
        assert items[start[atom]:start[atom + 1]].tolist() == sorted(item for a, item in flat if a == atom), atom
    hub = items[start[64]:start[65]].tolist()
    assert hub[:P] == [4 * e + e % 2 for e in range(P)] and all(item >= 4 * P for item in hub[P:])


# ------------------------------------------------------------------ csrc/geometry.h on the host

def test_entry_arithmetic_and_its_vjps_on_the_host(tmp_path):
    """csrc/geometry.h is __host__ __device__: tools/geometry_host_check.cpp, built for the host alone, checks the four VJPs
    against central differences in long double and the translation invariance of the point cotangents."""
    import subprocess
    from tfep_amd.build import _hipcc
    exe = str(tmp_path / 'geometry_host_check')
    subprocess.run([_hipcc(), '-std=c++17', '--cuda-host-only', '-x', 'hip', os.path.join(ROOT, 'tools', 'geometry_host_check.cpp'),
                    '-o', exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    print(done.stdout)
    assert done.returncode == 0, done.stdout + done.stderr
