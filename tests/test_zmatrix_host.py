"""CPU tests of the Z-matrix placement layer: the C ABI symbols and the torch ops, the host-side validation of a Z-matrix,
its level schedule and incidence list against ones built by brute force, the table cache, the launch shape the library
chooses at every tier of workgroup rows and LDS size and its limits at the C entry points, the conditioning of the cases
the GPU tests use and the stability of their reference, the plain reference of tests/zmatrix_ref.py against the reference
formulas of tests/geometry_ref.py, and the per-atom arithmetic of csrc/zmatrix.h compiled for the host.  No kernel is
launched."""
import ctypes
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
SYMBOLS.append('tfep_zmatrix_launch_shape')


def test_symbols_are_bound_and_declared():
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    declared = set(re.findall(r'\b(tfep_[a-z0-9_]+)\s*\(', header))
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert name in declared, name
    for name in ('tfep_zmatrix_place', 'tfep_zmatrix_place_backward'):
        assert _lib._SIGNATURES[name] == _lib._SIGNATURES[name + '_f64']
    assert len([name for name in _lib.EXPORTED_SYMBOLS if name.startswith('tfep_zmatrix_')]) == len(SYMBOLS) == 5
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


# (levels, widest level) of every case.  The tier cases above 700 placed atoms are left out: the brute force is quadratic
# in the atoms and takes more than a few seconds there, and they are the tree of t200 .. t600 again.
SCHEDULES = {'wide': (1, 70), 'chain': (40, 1), 'tree': (7, 16), 't200': (10, 62), 't260': (10, 54), 'c300': (300, 1),
             't400': (10, 87), 't600': (11, 118), 'w700': (1, 700)}


@pytest.mark.parametrize('name', SCHEDULES)
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
    widths = [b - a for a, b in zip(level_start, level_start[1:])]
    print(f'{name}: {n_levels} levels, widths {widths}')
    assert (n_levels, max(widths)) == SCHEDULES[name]
    if name in ('wide', 'w700'):
        assert [start[i + 1] - start[i] for i in range(3)] == [n_ic] * 3
    if name == 'w700':
        assert -(-n_ic // 64) == 11                              # the one level takes 11 passes of the 64 lanes
    if name == 'tree' or name in zr.TIERS and zr.TIERS[name].kind == 'tree':
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

def _launch_shape(n_atoms, n_ic, backward):
    """``(return code, rows of a workgroup, LDS bytes)`` of the library's own query; (-7, -7) is what it never wrote."""
    rows, lds = ctypes.c_int(-7), ctypes.c_int64(-7)
    rc = _lib.load().tfep_zmatrix_launch_shape(n_atoms, n_ic, int(backward), ctypes.byref(rows), ctypes.byref(lds))
    return rc, rows.value, lds.value


# LDS bytes of the tier cases (forward, backward), worked out by hand: 4 x 24 x 205, 4 x 72 x 200 and so on
TIER_BYTES = {'t200': (19680, 57600), 't260': (25440, 56160), 'c300': (29088, 64800), 't400': (38880, 57600),
              't600': (58080, 43200), 'w700': (50616, 50400), 't1200': (57840, 86400), 't2275': (54720, 163800),
              'f6826': (163824, 163800)}


@pytest.mark.parametrize('name', zr.TIER_CASES)
def test_launch_shape_of_every_tier_case(name):
    """The library lands a tier case in the tier it is recorded for in tests/zmatrix_ref.py: the rows of a workgroup, its
    LDS bytes, and whether that is above the 48 KiB past which the launcher raises the kernel's LDS attribute."""
    tier, c = zr.TIERS[name], zr.case(name)
    assert (len(c['fixed_atoms']), len(c['z_matrix'])) == (tier.n_fixed, tier.n_ic) and c['d'].shape[0] == zr.TIER_B == 7
    for backward, recorded, ruled, nbytes in zip((False, True), (tier.forward, tier.backward), zr.tier_shapes(name),
                                                 TIER_BYTES[name]):
        rc, rows, lds = _launch_shape(tier.n_fixed + tier.n_ic, tier.n_ic, backward)
        print(f"{name} {'backward' if backward else 'forward'}: {rows} rows, {lds} bytes of LDS")
        assert rc == 0
        assert (rows, lds > 48 * 1024) == recorded == (ruled.rows, ruled.attribute)
        assert lds == ruled.lds_bytes == nbytes <= ops.ZMATRIX_LDS_LIMIT
        assert rows * 64 <= 256                                  # (the kernels' launch bounds)


# size, rows, LDS attribute raised, one row above 64 KiB: both sides of every boundary of the table of tiers
FORWARD_TIERS = [(512, 4, False, False), (513, 4, True, False), (682, 4, True, False), (683, 3, True, False),
                 (910, 3, True, False), (911, 2, False, False), (1365, 2, True, False), (1366, 1, False, False),
                 (2048, 1, False, False), (2049, 1, True, False), (2730, 1, True, False), (2731, 1, True, True),
                 (6826, 1, True, True)]
BACKWARD_TIERS = [(170, 4, False, False), (171, 4, True, False), (227, 4, True, False), (228, 3, True, False),
                  (303, 3, True, False), (304, 2, False, False), (455, 2, True, False), (456, 1, False, False),
                  (682, 1, False, False), (683, 1, True, False), (910, 1, True, False), (911, 1, True, True),
                  (2275, 1, True, True)]


@pytest.mark.parametrize('backward', [False, True], ids=['forward', 'backward'])
def test_launch_shape_on_both_sides_of_every_tier_boundary(backward):
    for size, rows, attribute, beyond_shared in BACKWARD_TIERS if backward else FORWARD_TIERS:
        n_atoms, n_ic = (size + 3, size) if backward else (size, size - 3)
        rc, got_rows, lds = _launch_shape(n_atoms, n_ic, backward)
        assert rc == 0 and got_rows == rows, (size, got_rows)
        assert lds == rows * size * (72 if backward else 24), (size, lds)
        assert (lds > 48 * 1024, lds > 64 * 1024) == (attribute, beyond_shared), (size, lds)
        assert (got_rows, lds, attribute) == tuple(zr.launch_shape(n_atoms, n_ic, backward)), size
    # the other size does not enter: the forward keeps every atom, the backward the placed ones
    assert _launch_shape(6826, 3, False) == _launch_shape(6826, 6000, False) == (0, 1, 163824)
    assert _launch_shape(2500, 200, True) == _launch_shape(203, 200, True) == (0, 4, 57600)
    assert _launch_shape(0, 0, backward) == (0, 4, 0)


def test_limits_at_the_c_entry_points():
    """One row of 6826 atoms forward and of 2275 placed atoms backward is what the launchers accept; one more is an invalid
    argument that names the limit, from the query and from the four launchers alike, before anything is launched (the
    pointers are never dereferenced); and no rows at the limit sizes is nothing to do."""
    lib = _lib.load()
    message = lambda: lib.tfep_last_error().decode()
    assert (ops.ZMATRIX_MAX_ATOMS, ops.ZMATRIX_MAX_PLACED, ops.ZMATRIX_LDS_LIMIT) == (6826, 2275, 163840)
    assert _launch_shape(6826, 2275, False) == (0, 1, 163824) and _launch_shape(6826, 2275, True) == (0, 1, 163800)
    for n_atoms, n_ic, backward in ((6827, 2275, False), (2279, 2276, True), (6827, 2276, True)):
        assert _launch_shape(n_atoms, n_ic, backward) == (-1, -7, -7)
        assert '163840' in message() and '6826 atoms' in message() and '2275 placed' in message(), message()
    assert _launch_shape(6827, 2276 - 1, True)[0] == 0             # (2275 placed atoms among 6827: the backward holds them)
    assert _launch_shape(-1, 0, False)[0] == -1 and 'negative' in message()
    assert lib.tfep_zmatrix_launch_shape(10, 7, 0, None, None) == -1 and 'non-NULL' in message()
    fake = 1 << 12                     # a non-NULL pointer that is never dereferenced: every call returns before a launch
    for sfx in ('', '_f64'):
        place = getattr(lib, 'tfep_zmatrix_place' + sfx)
        back = getattr(lib, 'tfep_zmatrix_place_backward' + sfx)

        def forward(n_fixed, n_ic, B):
            n = n_fixed + n_ic
            return place(fake, n_ic, fake, n_ic, fake, n_ic, fake, 3 * n_fixed, fake, n_ic, fake, 1, fake, n_fixed, fake, 3 * n,
                         fake, n, B, None)

        def backward(n_fixed, n_ic, B):
            n = n_fixed + n_ic
            return back(fake, 3 * n, fake, n_ic, fake, n_ic, fake, n_ic, fake, n_ic, fake, 1, fake, n_fixed, fake, fake, 3 * n_ic,
                        fake, 3 * n, fake, fake, fake, fake, fake, n, B, None)

        assert forward(3, 6824, 4) == -1
        assert 'zmatrix_place' + sfx + ':' in message() and '163848 bytes' in message() and '6826 atoms' in message(), message()
        assert backward(3, 2276, 4) == -1
        assert 'zmatrix_place_backward' + sfx + ':' in message() and '163872 bytes' in message(), message()
        assert '163840' in message() and '2275 placed' in message(), message()
        assert forward(4551, 2275, 0) == 0 and backward(4551, 2275, 0) == 0
        assert forward(3, 6824, 0) == -1 and backward(3, 2276, 0) == -1       # (the size is refused whatever the batch)


@pytest.mark.parametrize('name', zr.ALL_CASES)
def test_cases_are_well_conditioned(name):
    c = zr.case(name)
    assert zr.B == 6 and zr.TIER_B == 7
    assert c['d'].shape == (7 if name in zr.TIER_CASES else 6, len(c['z_matrix'])) and c['d'].shape[0] == zr.batch(name)
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


@pytest.mark.parametrize('name', zr.ALL_CASES)
def test_float64_reference_is_stable_under_one_ulp_of_its_inputs(name):
    """The float64 reference on inputs each moved to the next float64, up or down: every quantity stays within 1e-11
    relative L2 of the unperturbed run -- a tenth of the 1e-10 the float64 kernels are held to, so that what a GPU test
    measures there is the kernel and never the conditioning of the case.  (A case that fails this is to be replaced by a
    shallower one of the same tiers; the bound of the GPU tests does not move.)"""
    ref, off = zr.reference(name), zr.reference(name, one_ulp_off=True)
    moved = [float((a != b).double().mean()) for a, b in zip(zr.inputs(name, False), zr.inputs(name, False, one_ulp_off=True))]
    assert min(moved) == 1.0, moved                               # every element of every input did move
    for k in zr.KEYS:
        rel = zr.rel_l2(off[k], ref[k])
        print(f'{name} {k}: rel L2 {rel:.3e} under one ulp of the inputs (bound 1e-11)')
        assert rel <= 1e-11, (name, k, rel)


@pytest.mark.parametrize('name', zr.ALL_CASES)
def test_float32_reference_has_an_error_to_measure_the_kernels_by(name):
    """The float32 kernels are held to 4 x the error of the reference run in float32: that error is not zero for any
    quantity of any case (a zero would ask the kernel for the float64 result to the bit), nor anything but rounding."""
    ref32, ref = zr.reference(name, rounded=True, dtype=zr.F32), zr.reference(name, rounded=True)
    for k in zr.KEYS:
        rel = zr.rel_l2(ref32[k], ref[k])
        print(f'{name} {k}: float32 reference rel L2 {rel:.3e}')
        assert 0.0 < rel < 1e-4, (name, k, rel)


@pytest.mark.parametrize('name', zr.ROUND_TRIP_TIER_CASES)
def test_float32_reference_round_trip_has_an_error_to_measure_the_kernels_by(name):
    """The same for what the round trip of the tier cases is held to: the internal coordinates the float32 reference gets
    back against the ones it started from, and the log-det of its way back (a float32 sum) against the float64 reference
    log-det.  (The fixed atoms are copied, there and in the kernels: no error on either side.)"""
    ref32 = {k: v.to(zr.F64).numpy() for k, v in zr.reference_round_trip(name, zr.F32).items()}
    start = dict(zip(zr.INPUTS, zr.inputs(name, rounded=True)))
    ldj = zr.reference(name, rounded=True)['log_det_J']
    for k, got, ref in (('d', ref32['d'], start['d'].numpy()), ('a', ref32['a'], start['a'].numpy()),
                        ('t', zr.circ(ref32['t']), zr.circ(start['t'].numpy())), ('log_det_J', ref32['log_det_J'], ldj),
                        ('minus the log-det back', ref32['minus_back'], ldj)):
        rel = zr.rel_l2(got, ref)
        print(f'{name} round trip {k}: float32 reference rel L2 {rel:.3e}')
        assert 0.0 < rel < 1e-4, (name, k, rel)
    assert np.array_equal(ref32['x_fixed'], start['x_fixed'].numpy())


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
