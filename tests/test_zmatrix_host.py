"""CPU tests of the Z-matrix placement layer: the C ABI symbols and the torch ops, the host-side validation of a Z-matrix,
its level schedule and incidence list against ones built by brute force, the table cache, the conditioning of the cases
the GPU tests use, the plain reference of tests/zmatrix_ref.py against the reference formulas of tests/geometry_ref.py, and
the per-atom arithmetic of csrc/zmatrix.h compiled for the host.  No kernel is launched."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import geometry_ref as gr
import zmatrix_ref as zr
from tfep_amd import _lib, ops
from tfep_amd.utils import geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = [f'tfep_{name}{sfx}' for name in ('zmatrix_place', 'zmatrix_place_backward') for sfx in ('', '_f64')]


def test_symbols_are_bound_and_declared():
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    declared = set(re.findall(r'\b(tfep_[a-z0-9_]+)\s*\(', header))
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert name in declared, name
    for name in ('tfep_zmatrix_place', 'tfep_zmatrix_place_backward'):
        assert _lib._SIGNATURES[name] == _lib._SIGNATURES[name + '_f64']
    assert _lib.ABI_VERSION == 8 and re.search(r'#define\s+TFEP_HIP_ABI_VERSION\s+8\b', header)


def test_ops_and_public_names():
    from tfep_amd import torch_ops
    from tfep_amd.nn import flows
    assert torch_ops.ZMATRIX_OPS == ('zmatrix_place', 'zmatrix_place_backward')
    assert not set(torch_ops.ZMATRIX_OPS) & set(torch_ops.GEOMETRY_OPS)
    for name in torch_ops.ZMATRIX_OPS:
        assert hasattr(torch.ops.tfep, name)
    assert str(inspect.signature(geometry.zmatrix_to_cartesian)) == '(d, a, t, x_fixed, z_matrix, fixed_atoms)'
    assert str(inspect.signature(geometry.cartesian_to_zmatrix)) == '(x, z_matrix, fixed_atoms)'
    assert str(inspect.signature(ops.zmatrix_tables)) == '(z_matrix, fixed_atoms, n_atoms, device)'
    assert issubclass(flows.ZMatrixFlow, torch.nn.Module)
    flow = flows.ZMatrixFlow(torch.nn.Identity(), zr.case('tree')['z_matrix'], zr.case('tree')['fixed_atoms'])
    assert {'_z_matrix', '_fixed_atoms'} <= set(dict(flow.named_buffers()))
    from tfep_amd.build import SOURCES
    assert 'zmatrix.hip' in SOURCES


# ------------------------------------------------------------------ validation

GOOD_Z = [[3, 0, 1, 2], [4, 3, 0, 1], [5, 4, 3, 0]]
GOOD_FIXED = [0, 1, 2]


def _tables(z, fixed=GOOD_FIXED, n_atoms=6):
    return ops.zmatrix_tables(torch.as_tensor(z), torch.as_tensor(fixed), n_atoms, 'cpu')


def _with(row, col, value):
    z = [list(r) for r in GOOD_Z]
    z[row][col] = value
    return z


@pytest.mark.parametrize('z, fixed, n_atoms, match', [
    (torch.tensor(GOOD_Z).double(), GOOD_FIXED, 6, 'integer'),
    (GOOD_Z, torch.tensor(GOOD_FIXED).float(), 6, 'integer'),
    (torch.tensor(GOOD_Z) > 1, GOOD_FIXED, 6, 'integer'),
    (torch.tensor(GOOD_Z)[:, :3], GOOD_FIXED, 6, 'shape'),
    (torch.tensor(GOOD_Z).t(), GOOD_FIXED, 6, 'shape'),
    (torch.tensor(GOOD_Z).reshape(-1), GOOD_FIXED, 6, 'shape'),
    (GOOD_Z, [GOOD_FIXED], 6, 'shape'),
    (_with(2, 3, 6), GOOD_FIXED, 6, 'outside'),
    (GOOD_Z, [0, 1, 6], 6, 'outside'),
    (_with(1, 3, -1), GOOD_FIXED, 6, 'negative'),
    (_with(0, 0, -1), GOOD_FIXED, 6, 'negative'),
    (GOOD_Z, [0, 1, -2], 6, 'negative'),
    (_with(1, 2, 3), GOOD_FIXED, 6, 'distinct'),
    (_with(2, 1, 5), GOOD_FIXED, 6, 'distinct'),
    (GOOD_Z[:2] + [[4, 3, 1, 0]], GOOD_FIXED, 6, 'placed twice'),
    (GOOD_Z, [0, 1, 2, 2], 6, 'fixed twice'),
    (_with(2, 0, 2), GOOD_FIXED, 6, 'both fixed and placed'),
    (GOOD_Z, GOOD_FIXED, 7, 'neither'),
    (GOOD_Z[:2], GOOD_FIXED, 6, 'neither'),
    ([[2, 0, 1, 3], [3, 2, 0, 1]], [0, 1], 4, 'at least 3'),
    ([[3, 4, 0, 1], [4, 3, 1, 2]], GOOD_FIXED, 5, 'cycle'),
    ([[3, 0, 1, 2], [4, 5, 3, 0], [5, 6, 4, 3], [6, 4, 0, 1]], GOOD_FIXED, 7, 'cycle'),
], ids=lambda v: v if isinstance(v, str) else None)
def test_validation(z, fixed, n_atoms, match):
    with pytest.raises(ValueError, match=match):
        ops.zmatrix_tables(torch.as_tensor(z), torch.as_tensor(fixed), n_atoms, 'cpu')


def test_validation_names_the_lds_limit_and_reaches_the_public_functions():
    """A row that one workgroup's LDS cannot hold is refused on the host, naming the limit, before anything is launched;
    the public functions validate before anything touches a device."""
    n = ops.ZMATRIX_MAX_PLACED + 1
    chain = torch.stack([torch.arange(3, n + 3) - s for s in range(4)], dim=1)
    with pytest.raises(ValueError, match=f'{ops.ZMATRIX_LDS_LIMIT} bytes of LDS.*{ops.ZMATRIX_MAX_PLACED} placed'):
        ops.zmatrix_tables(chain, torch.arange(3), n + 3, 'cpu')
    assert (ops.ZMATRIX_LDS_LIMIT, ops.ZMATRIX_MAX_ATOMS, ops.ZMATRIX_MAX_PLACED) == (160 * 1024, 6826, 2275)
    ops.zmatrix_tables(chain[:-1], torch.arange(3), n + 2, 'cpu')              # the largest chain there is room for
    v = torch.zeros(2, 3)
    with pytest.raises(ValueError, match='cycle'):
        geometry.zmatrix_to_cartesian(v[:, :2], v[:, :2], v[:, :2], torch.zeros(2, 3, 3), torch.tensor([[3, 4, 0, 1], [4, 3, 1, 2]]),
                                      torch.arange(3))
    with pytest.raises(ValueError, match='distinct'):
        geometry.cartesian_to_zmatrix(torch.zeros(2, 6, 3), torch.tensor(_with(1, 2, 3)), torch.arange(3))
    with pytest.raises(ValueError, match='x_fixed'):
        geometry.zmatrix_to_cartesian(v, v, v, torch.zeros(2, 4, 3), torch.tensor(GOOD_Z), torch.arange(3))
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        geometry.zmatrix_to_cartesian(v, v, v, torch.zeros(2, 3, 3), torch.tensor(GOOD_Z), torch.arange(3))


# ------------------------------------------------------------------ the schedule

def _brute_force_levels(z, fixed):
    level = {int(i): 0 for i in fixed}
    left = {int(r[0]): [int(v) for v in r[1:]] for r in z}
    while left:
        for atom, refs in list(left.items()):
            if all(v in level for v in refs):
                level[atom] = 1 + max(level[v] for v in refs)
                del left[atom]
    return level


@pytest.mark.parametrize('name', zr.CASES)
def test_level_schedule_and_incidence_list_against_brute_force(name):
    c = zr.case(name)
    z, fixed = c['z_matrix'], c['fixed_atoms']
    n_ic, n_atoms = len(z), len(z) + len(fixed)
    tb = ops.zmatrix_tables(z, fixed, n_atoms, 'cpu')
    assert all(t.dtype == torch.int32 and t.is_contiguous() for t in tb)
    rows, level_start, fixed_t, start, items = (t.tolist() for t in tb)
    level = _brute_force_levels(z.tolist(), fixed.tolist())
    # the sorted rows: by level, the caller's order within a level; the fifth row is the caller's row
    expected = sorted(range(n_ic), key=lambda r: (level[int(z[r, 0])], r))
    assert rows[4] == expected
    assert [[rows[c_][s] for c_ in range(4)] for s in range(n_ic)] == [z[r].tolist() for r in expected]
    n_levels = max(level.values())
    assert level_start == [sum(1 for r in range(n_ic) if level[int(z[r, 0])] <= lv) for lv in range(n_levels + 1)]
    assert level_start[0] == 0 and level_start[-1] == n_ic and fixed_t == fixed.tolist()
    for lv in range(n_levels):                                  # no atom of a level references an atom of the same level
        here = {rows[0][s] for s in range(level_start[lv], level_start[lv + 1])}
        assert all(rows[c_][s] not in here for s in range(level_start[lv], level_start[lv + 1]) for c_ in (1, 2, 3))
    # the incidence list: for every atom the sorted rows that reference it, ascending, as 4 * sorted row + slot
    assert len(start) == n_atoms + 1 and start[0] == 0 and start[-1] == 3 * n_ic == len(items)
    for atom in range(n_atoms):
        assert items[start[atom]:start[atom + 1]] == [4 * s + slot for s in range(n_ic) for slot in range(3)
                                                      if rows[1 + slot][s] == atom], atom
    shape = {'wide': (1, 70), 'chain': (40, 1), 'tree': (7, 16)}[name]
    widths = [b - a for a, b in zip(level_start, level_start[1:])]
    print(f'{name}: {n_levels} levels, widths {widths}')
    assert (n_levels, max(widths)) == shape
    if name == 'wide':
        assert [start[i + 1] - start[i] for i in range(3)] == [70, 70, 70]
    if name == 'tree':
        assert fixed.tolist() != sorted(fixed.tolist()) or fixed.tolist() != list(range(5))
        assert rows[4] != list(range(n_ic))                      # the caller's rows are not in level order


def test_table_cache_sees_an_in_place_write():
    z, fixed = torch.tensor(GOOD_Z), torch.tensor(GOOD_FIXED)
    first = ops.zmatrix_tables(z, fixed, 6, 'cpu')
    assert ops.zmatrix_tables(z, fixed, 6, 'cpu') is first
    assert ops.zmatrix_index_tables(z, fixed, 6, 'cpu')[0][2].t().tolist() == GOOD_Z
    z[2, 1:] = torch.tensor([0, 1, 2])                           # atom 5 now hangs on the fixed atoms: level 1
    second = ops.zmatrix_tables(z, fixed, 6, 'cpu')
    assert second is not first
    assert first.level_start.tolist() == [0, 1, 2, 3] and second.level_start.tolist() == [0, 2, 3]
    assert second.rows[4].tolist() == [0, 2, 1]
    for got, fresh in zip(second, ops.zmatrix_tables(z.clone(), fixed.clone(), 6, 'cpu')):
        assert torch.equal(got, fresh)
    z[2, 1] = 5
    with pytest.raises(ValueError, match='distinct'):
        ops.zmatrix_tables(z, fixed, 6, 'cpu')
    fixed[0] = 3
    z[2, 1] = 0
    with pytest.raises(ValueError, match='both fixed and placed'):
        ops.zmatrix_tables(z, fixed, 6, 'cpu')


# ------------------------------------------------------------------ the cases and the reference

@pytest.mark.parametrize('name', zr.CASES)
def test_cases_are_well_conditioned(name):
    c = zr.case(name)
    assert c['d'].shape == (zr.B, len(c['z_matrix'])) and zr.B == 6
    assert 0.9 <= float(c['d'].min()) and float(c['d'].max()) <= 1.6
    assert 0.6 <= float(c['a'].min()) and float(c['a'].max()) <= 2.5
    assert -np.pi < float(c['t'].min()) and float(c['t'].max()) < np.pi
    low = zr.min_reference_sine(zr.reference(name)['x'], c['z_matrix'])
    print(f"{name}: seed {c['seed']}, min sin(x_j, x_k, x_l) = {low:.4f}")
    assert low >= zr.MIN_SINE == 0.3


@pytest.mark.parametrize('name', zr.CASES)
def test_reference_round_trips_through_the_reference_internal_coordinates(name):
    """The placement of tests/zmatrix_ref.py against the formulas of tests/geometry_ref.py (which test_geometry_host.py
    ties to the reference's results): the internal coordinates of the placed atoms are the ones they were placed with."""
    c = zr.case(name)
    z = c['z_matrix']
    x = torch.from_numpy(zr.reference(name)['x'])
    d, a, t = gr.internal_coordinates(x, z[:, :2].t(), z[:, :3].t(), z.t())
    for k, got in (('d', d), ('a', a)):
        err = float((got - c[k]).abs().max())
        print(f'{name} {k}: max abs {err:.3e}')
        assert err <= 1e-12
    err = float(np.abs(gr.wrapped(t.numpy() - c['t'].numpy())).max())
    print(f'{name} t: max abs {err:.3e}')
    assert err <= 1e-12
    assert torch.equal(x[:, c['fixed_atoms']], c['x_fixed'])


def test_reference_runs_in_float32():
    ref32, ref = zr.reference('chain', rounded=True, dtype=zr.F32), zr.reference('chain', rounded=True)
    rel = zr.rel_l2(ref32['x'], ref['x'])
    assert 0.0 < rel < 1e-4, rel


# ------------------------------------------------------------------ csrc/zmatrix.h on the host

def test_atom_arithmetic_and_its_vjp_on_the_host(tmp_path):
    """csrc/zmatrix.h is __host__ __device__: tools/zmatrix_host_check.cpp, built for the host alone, checks place_atom
    against ic_distance / ic_angle / ic_dihedral and place_atom_vjp against central differences in long double."""
    from tfep_amd.build import _hipcc
    exe = str(tmp_path / 'zmatrix_host_check')
    subprocess.run([_hipcc(), '-std=c++17', '--cuda-host-only', '-x', 'hip', os.path.join(ROOT, 'tools', 'zmatrix_host_check.cpp'),
                    '-o', exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    print(done.stdout)
    assert done.returncode == 0, done.stdout + done.stderr
