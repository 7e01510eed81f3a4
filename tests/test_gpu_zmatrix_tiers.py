"""The Z-matrix placement kernels (csrc/zmatrix.hip) at every shape their launchers choose: the tier cases of
tests/zmatrix_ref.py (``TIERS``; 7 rows) put the forward and the backward kernel at least once into each of 4, 3, 2 and 1
rows a workgroup, under and over the 48 KiB past which the kernel's LDS attribute is raised, over the 64 KiB the rows of a
workgroup share, and at the 160 KiB limit of one row (6826 atoms forward, 2275 placed atoms backward).  The cases of
tests/test_gpu_zmatrix.py (at most 73 atoms) all run 4 rows a workgroup under 48 KiB.  tests/test_zmatrix_host.py holds
the tier of every case against the library's own answer (``tfep_zmatrix_launch_shape``).

What a wrong launch shape would break, and the test that sees it:
    a row a workgroup of 3 waves (192 threads) or a ragged last workgroup skips    every output element is written
    LDS slices of two waves that overlap (a wrong stride per wave)                  values, gradients; bits of a middle row
    the attribute not raised, raised too late or lost by a later launch             order of first use; every case over 48 KiB
    a launch at the CU's whole LDS that the runtime refuses                         t2275, f6826: an error, not a wrong value

Bounds, those of tests/test_gpu_zmatrix.py and not re-tuned for the sizes here.  float64: relative L2 <= 1e-10 against
the float64 reference (which moves by less than 1e-11 under one ulp of its inputs: tests/test_zmatrix_host.py).  float32:
4 x the relative L2 error of the REFERENCE run in float32 on the same (rounded) inputs against its float64 run.  Dihedrals
are compared as (sin, cos).  Every figure is printed before it is asserted.  The references are computed once a session
(``zr.reference`` is cached) and shared by the tests.
"""
import math

import pytest
import torch

import zmatrix_ref as zr
from tfep_amd import ops
from tfep_amd.utils import geometry

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
dtypes = pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
cases = pytest.mark.parametrize('name', zr.TIER_CASES)
LAST = zr.TIER_B - 1            # the lone wave of the ragged last workgroup at 4, 3 and 2 rows a workgroup


def _forward(name, dtype):
    """``(x, log_det_J)`` of a case by the forward kernel alone."""
    return geometry.zmatrix_to_cartesian(*(zr.dev(zr.case(name)[k], dtype) for k in zr.INPUTS), *zr.tables(name))


def _assert_all_close(name, got, dtype, keys=zr.KEYS):
    ref, ref32 = zr.references(name, dtype)
    for k in keys:
        assert got[k].shape == ref[k].shape, (k, got[k].shape)
        zr.assert_close(f'{name} {k}', got[k], ref[k], ref32[k], dtype)


# ------------------------------------------------------------------ the attribute (first in the file, see below)

@dtypes
def test_order_of_first_use(dtype):
    """The launcher raises the kernel's LDS attribute at the first launch that needs more than 48 KiB, once for a kernel
    and a device.  A launch that needs none, one that sets it for the largest row there is, the first again, one in
    between: the small case gives the same bits before and after, the others are right; then the same for the backward
    kernel.  This file runs after
    tests/test_gpu_zmatrix.py, whose cases need no attribute, and this test is the first of the file: in a run of the
    whole suite, and when the file is run alone, these are the first launches of either kernel above 48 KiB."""
    first = _forward('t200', dtype)                                    # 19 680 B: no attribute
    large = _forward('t2275', dtype)                                   # 54 720 B: sets it
    again = _forward('t200', dtype)
    between = _forward('t600', dtype)                                  # 58 080 B
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    for name, got in (('t200', first), ('t2275', large), ('t600', between)):
        _assert_all_close(name, dict(zip(zr.KEYS, got)), dtype, zr.KEYS[:2])
    # the backward: t600 is its one tier under 48 KiB (1 row of 43 200 B); t260 (3 rows, 56 160 B) raises the attribute
    # itself, t2275 takes the whole 163 800 B
    small = zr.run('t600', dtype)
    first = zr.run('t260', dtype)
    large = zr.run('t2275', dtype)
    again = zr.run('t260', dtype)
    small_again = zr.run('t600', dtype)
    for k in zr.KEYS:
        assert torch.equal(first[k], again[k]) and torch.equal(small[k], small_again[k]), k
    _assert_all_close('t600', small, dtype)
    _assert_all_close('t260', first, dtype)
    _assert_all_close('t2275', large, dtype)


# ------------------------------------------------------------------ against the reference

@dtypes
@cases
def test_values_and_log_det_match_the_reference(name, dtype):
    x, ldj = _forward(name, dtype)
    tier = zr.TIERS[name]
    assert x.shape == (zr.TIER_B, tier.n_fixed + tier.n_ic, 3) and ldj.shape == (zr.TIER_B,)
    _assert_all_close(name, {'x': x, 'log_det_J': ldj}, dtype, ('x', 'log_det_J'))


@dtypes
@cases
def test_gradients_match_the_reference(name, dtype):
    _assert_all_close(name, zr.run(name, dtype), dtype, ('g_d', 'g_a', 'g_t', 'g_x_fixed'))


def _poisoned(call, outputs, dtype):
    """``call()`` after blocks of the sizes of its ``outputs`` were filled with NaN and freed: the caching allocator is
    likely to hand them to the ``torch.empty`` of the op, so that an element the kernel does not write is a NaN and not the
    right value an earlier call left in the same block.  Likely, not certain -- least so for the few bytes of
    ``log_det_J``, which share a size class with many other free blocks.  The finiteness check is therefore an extra; what
    catches a row left out is the comparison with the reference, which only a block that still holds an earlier call's
    right values could get past, and the poisoning is there to make that unlikely."""
    torch.cuda.synchronize()
    poison = [torch.full(shape, math.nan, device='cuda', dtype=dtype) for shape in outputs]
    del poison
    return call()


@dtypes
@cases
def test_every_output_element_is_written(name, dtype):
    """The raw ops, which allocate their outputs with ``torch.empty``: every element of every output is finite and within
    the bounds, and two calls agree bit for bit.  This is what sees a row that a workgroup of three waves, or the ragged
    last workgroup, leaves out (how surely: ``_poisoned``)."""
    c, n_rows, tier = zr.case(name), zr.TIER_B, zr.TIERS[name]
    n = tier.n_fixed + tier.n_ic
    tables = ops.zmatrix_tables(*zr.tables(name), n, 'cuda')
    d, a, t, x_fixed = (zr.dev(c[k].reshape(n_rows, -1), dtype) for k in zr.INPUTS)
    gx, gl = zr.dev(c['cx'].reshape(n_rows, -1), dtype), zr.dev(c['cl'], dtype)
    op = torch.ops.tfep
    place = lambda: op.zmatrix_place(d, a, t, x_fixed, *tables)
    x, ldj = _poisoned(place, [(n_rows, 3 * n), (n_rows,)], dtype)
    assert x.shape == (n_rows, 3 * n) and ldj.shape == (n_rows,)
    back = lambda: op.zmatrix_place_backward(x, d, a, t, *tables, gx, gl)
    grads = _poisoned(back, [(n_rows, tier.n_ic)] * 3 + [(n_rows, 3 * tier.n_fixed)], dtype)
    assert [tuple(g.shape) for g in grads] == [(n_rows, tier.n_ic)] * 3 + [(n_rows, 3 * tier.n_fixed)]
    got = dict(zip(zr.KEYS, (x.reshape(n_rows, n, 3), ldj, *grads[:3], grads[3].reshape(n_rows, tier.n_fixed, 3))))
    for k, v in got.items():
        unwritten = int((~torch.isfinite(v)).sum())
        print(f'{name} {k} {dtype}: {unwritten} of {v.numel()} elements not finite')
        assert unwritten == 0, k
    _assert_all_close(name, got, dtype)
    x2, ldj2 = _poisoned(place, [(n_rows, 3 * n), (n_rows,)], dtype)
    grads2 = _poisoned(back, [(n_rows, tier.n_ic)] * 3 + [(n_rows, 3 * tier.n_fixed)], dtype)
    assert torch.equal(x, x2) and torch.equal(ldj, ldj2)
    assert all(torch.equal(g, g2) for g, g2 in zip(grads, grads2))


# ------------------------------------------------------------------ bit for bit

@dtypes
@cases
def test_bits_do_not_depend_on_the_workgroup(name, dtype):
    """The last of the 7 rows run alone (the only wave of a workgroup, at the start of its LDS) against the same row in
    the batch, where it is the lone wave of the ragged last workgroup at 4, 3 and 2 rows a workgroup; and for t260 and
    t400 row 1, a middle wave (the last at 2 rows) whose LDS slice lies behind another's: values and gradients."""
    full = zr.run(name, dtype)
    for row in (LAST, 1) if name in ('t260', 't400') else (LAST,):
        alone = zr.run(name, dtype, rows=slice(row, row + 1))
        for k in zr.KEYS:
            assert alone[k].shape[0] == 1 and torch.equal(full[k][row:row + 1], alone[k]), (k, row)


@dtypes
@pytest.mark.parametrize('name', zr.ROUND_TRIP_TIER_CASES)
def test_round_trip(name, dtype):
    """Through ``cartesian_to_zmatrix``: the internal-coordinate kernel on 260, 1200 and 2275 quads.  The two log-dets
    are each held to the float64 reference log-det (``zr.check_round_trip``), at the bounds of every other quantity."""
    zr.check_round_trip(name, dtype, log_dets_against_reference=True)


# ------------------------------------------------------------------ the flow

def test_zmatrix_flow_on_a_few_hundred_atoms():
    """``ZMatrixFlow`` on the 265 atoms of t260 (the backward runs 3 rows a workgroup) around the small MAF of
    tests/test_gpu_zmatrix.py, float64: ``inverse(forward(x))`` and the two log-dets, at the bounds of that test.

    The way in returns a dihedral in (-pi, pi], so a row in which the inner flow moves a dihedral across +-pi is placed
    correctly but not inverted by ``inverse`` (as with an angle moved out of (0, pi): the docstring of ``ZMatrixFlow``).
    Of the 7 x 260 dihedrals of t260, uniform in (-pi, pi), this MAF moves 3 across, in rows 1, 2 and 5.  All 7 rows go
    through ``forward`` and its backward, and the internal coordinates of what it places are what the inner flow made,
    dihedrals as (sin, cos); ``inverse(forward(x))`` and the two log-dets are compared on the 4 rows that stay inside
    the cut, and that they are these 4 is asserted."""
    name, n_ic = 't260', zr.TIERS['t260'].n_ic
    flow = zr.flow(name)
    x = zr.dev(zr.reference(name)['x'].reshape(zr.TIER_B, -1), F64, grad=True)
    # the setup: what the inner flow makes of the internal coordinates is still a valid set of them, the inner flow is
    # inverted by its own inverse, and the rows whose dihedrals all stay inside the cut
    d, a, t, x_fixed, _ = geometry.cartesian_to_zmatrix(x.detach(), *zr.tables(name))
    before = torch.cat([d, a, t, x_fixed], dim=1)
    mixed = flow.flow(before)[0].detach()
    d1, a1, t1 = mixed[:, :n_ic], mixed[:, n_ic:2 * n_ic], mixed[:, 2 * n_ic:3 * n_ic]
    print(f'inner flow: d in [{float(d1.min()):.3f}, {float(d1.max()):.3f}], a in [{float(a1.min()):.3f}, '
          f'{float(a1.max()):.3f}], t in [{float(t1.min()):.4f}, {float(t1.max()):.4f}]')
    assert float(d1.min()) > 0.5 and 0.3 < float(a1.min()) and float(a1.max()) < 2.8
    err_inner = float((flow.flow.inverse(mixed)[0] - before).abs().max())
    print(f'inner flow alone: inverse(forward) max |d| = {err_inner:.3e}')
    assert err_inner <= 1e-9
    across = (t1.abs() > math.pi).sum(1)
    margin = float((t1.abs() - math.pi).abs().min())
    print(f'dihedrals moved across the cut, row by row: {across.tolist()}; the closest to it is {margin:.2e} away')
    assert across.tolist() == [0, 1, 1, 0, 0, 1, 0] and margin > 1e-6
    inside = across == 0
    y, ldj = flow(x)
    assert y.shape == x.shape and ldj.shape == (zr.TIER_B,)
    print(f'max |y - x| = {float((y - x).detach().abs().max()):.3e}')
    assert float((y - x).detach().abs().max()) > 1e-4                      # the inner flow does move the atoms
    # every row is placed where the inner flow says
    d2, a2, t2, x_fixed2, _ = geometry.cartesian_to_zmatrix(y.detach(), *zr.tables(name))
    err_y = max(float((d2 - d1).abs().max()), float((a2 - a1).abs().max()), float((t2.sin() - t1.sin()).abs().max()),
                float((t2.cos() - t1.cos()).abs().max()), float((x_fixed2 - mixed[:, 3 * n_ic:]).abs().max()))
    print(f'internal coordinates of forward(x) against the inner flow, all rows: max |d| = {err_y:.3e}')
    assert err_y <= 1e-9
    x_back, ldj_back = flow.inverse(y.detach())
    err_x = float((x_back - x)[inside].abs().max())
    err_l = float((ldj_back + ldj)[inside].abs().max())
    print(f'inverse(forward(x)), {int(inside.sum())} rows: max |dx| = {err_x:.3e}, max |log-det sum| = {err_l:.3e}')
    assert err_x <= 1e-9 and err_l <= 1e-8
    (y.square().sum() - ldj.sum()).backward()
    grads = [p.grad for p in flow.flow.parameters()]
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads) and x.grad is not None and bool(torch.isfinite(x.grad).all())
