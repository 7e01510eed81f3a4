"""The internal-coordinate and polar kernels (csrc/geometry.hip) past one wave pass and past one block, against the plain
float64 restatement of tests/geometry_ref.py (tied to the reference's results in tests/test_geometry_host.py).

The wide case (``geometry_ref.wide_case``): 130 atoms, 70 + 67 + 65 table entries, 6 rows.  The atom loop of the backward
takes three trips, the last with two lanes; the entry loop of the forward takes four, with the pair / triple boundary
inside the second, the triple / quad boundary inside the third and ten lanes in the last; the second workgroup is half
empty; atom 64 sums 70 pair terms, atoms 125..129 none.  The polar arrays have 1031 elements: in float32 257 packs of 16
bytes and 3 tail elements over 2 blocks, in float64 515 and 1 over 3.

Bounds.  float64: relative L2 <= 1e-10 per quantity (the bound of tests/test_gpu_geometry.py), and per element
``1e-10 max(1, |ref|)``.  float32: csrc/geometry.h promises fp64 arithmetic on the widened inputs and ONE rounding on
store, so against the float64 reference on the float32-rounded inputs and cotangents every element obeys
``|got - ref| <= 2^-23 |ref| + 1e-10 max|ref|`` (``geometry_ref.f32_contract_ratio``): twice one float32 rounding, plus
the float64 bound on the row's largest element.  Under the conditions asserted on the wide case (distances >= 0.1,
sin(angle) >= 0.01, rejections >= 0.02) the fp64 round-off times the conditioning (<= 100 / 0.02) stays below 1e-11
relative, so the bound is derived, not measured; a kernel computing in float32 misses it by orders of magnitude.  Angles
and dihedrals are compared as (sin, cos) in L2 and by the wrapped difference per element.  Every figure is printed before
it is asserted.
"""
import itertools

import numpy as np
import pytest
import torch

import geometry_ref as gr
import golden_util as gu
from tfep_amd import ops
from tfep_amd.utils import geometry

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
TOL64 = 1e-10
N, B = gr.WIDE_N, gr.WIDE_B
NAMES = ('d', 'a', 't', 'gx')
IS_ANGLE = dict(d=False, a=True, t=True, gx=False)


def _dev(a, dtype, grad=False):
    return torch.as_tensor(a).detach().to(device='cuda', dtype=dtype, copy=True).requires_grad_(grad)


def _rounded(a, dtype):
    """The float64 array a tensor of ``dtype`` holds after the conversion: what the reference of a float32 run starts from."""
    return torch.as_tensor(a).to(dtype).to(F64)


def _kernels(x, tables, cots):
    """``(d, a, t, gx)`` as numpy arrays: the kernels on the device rows ``x`` with the device cotangents; a cotangent that
    is None is left to autograd."""
    d, a, t = geometry.internal_coordinates(x, *tables)
    used = [(o, c) for o, c in zip((d, a, t), cots) if c is not None]
    (gx,) = torch.autograd.grad([o for o, _ in used], x, [c for _, c in used])
    assert gx.shape == x.shape and gx.dtype == x.dtype
    return [v.detach().cpu().numpy() for v in (d, a, t, gx)]


def _run(case, dtype, tables=None, cots=None, rows=slice(None)):
    x, all_tables, all_cots = case
    tables = all_tables if tables is None else tables
    cots = all_cots if cots is None else cots
    return _kernels(_dev(x[rows].reshape(-1, 3 * N), dtype, grad=True), tables,
                    [None if c is None else _dev(c[rows], dtype) for c in cots])


@pytest.fixture(scope='module')
def wide():
    """The wide case with the conditions the bounds rest on, checked on the CPU reference before anything is compared."""
    x, tables, cots = gr.wide_case()
    min_d, min_sin, min_rejection = gr.conditioning(x, *tables)
    print(f'wide case, seed {gr.WIDE_SEED}: min d {min_d:.4f}, min sin(a) {min_sin:.4f}, min(|v|, |w|) {min_rejection:.4f}')
    assert min_d >= gr.MIN_D and min_sin >= gr.MIN_SIN and min_rejection >= gr.MIN_REJECTION
    return x, tables, cots


@pytest.fixture(scope='module')
def wide_ref(wide):
    """The float64 reference of the wide case on the inputs as each dtype holds them; computed once."""
    x, tables, cots = wide
    return {dt: gr.coordinates_and_gradient(_rounded(x, dt), tables, [_rounded(c, dt) for c in cots]) for dt in (F32, F64)}


def _assert_matches(what, got, ref, dtype):
    """float64: relative L2 <= 1e-10 per quantity; float32: the one-rounding contract on every element."""
    for k, v, r in zip(NAMES, got, ref):
        r = r.reshape(v.shape)
        assert v.dtype == (np.float64 if dtype == F64 else np.float32) and np.isfinite(v).all(), (what, k)
        if dtype == F64:
            rel = gr.rel_l2(gr.circ(v), gr.circ(r)) if IS_ANGLE[k] else gr.rel_l2(v, r)
            print(f'{what} f64 {k}: rel L2 {rel:.3e} = {rel / TOL64:.3e} of the bound {TOL64:.0e}')
            assert rel <= TOL64, (what, k, rel)
        else:
            ratio = gr.f32_contract_ratio(v, r, angle=IS_ANGLE[k])
            print(f'{what} f32 {k}: largest |got - ref| / (2^-23 |ref| + 1e-10 max|ref|) = {ratio:.3f}')
            assert ratio <= 1.0, (what, k, ratio)


# ------------------------------------------------------------------ (a) values and gradients at the wide size

@DTYPES
def test_wide_values_and_gradients_match_the_float64_reference(wide, wide_ref, dtype):
    got = _run(wide, dtype)
    assert [v.shape for v in got] == [(B, gr.WIDE_P), (B, gr.WIDE_A), (B, gr.WIDE_T), (B, 3 * N)]
    _assert_matches('wide', got, wide_ref[dtype], dtype)
    # atoms 125..129 are in no entry: their cotangent is written, as +0.0
    unused = got[3].reshape(B, N, 3)[:, gr.WIDE_USED:]
    assert (unused == 0.0).all() and not np.signbit(unused).any()
    assert (got[3].reshape(B, N, 3)[:, :gr.WIDE_USED] != 0.0).any(axis=2).sum() > B * 100
    # the (batch, n_particles, 3) form: the cotangent has the shape and dtype of x
    x = _dev(wide[0], dtype, grad=True)
    d, a, t = geometry.internal_coordinates(x, *wide[1])
    (gx,) = torch.autograd.grad([d, a, t], x, [_dev(c, dtype) for c in wide[2]])
    assert gx.shape == x.shape == (B, N, 3) and gx.dtype == dtype
    assert np.array_equal(gx.cpu().numpy().reshape(B, 3 * N), got[3])


# ------------------------------------------------------------------ (b) kind boundaries, element by element

def test_every_entry_matches_and_a_missing_table_moves_no_column(wide, wide_ref):
    x, tables, cots = wide
    full = _run(wide, F64)
    for k, v, r in zip(NAMES[:3], full, wide_ref[F64]):
        ratio = gr.f64_element_ratio(v, r, angle=k == 't')
        print(f'wide f64 {k}: largest |got - ref| / (1e-10 max(1, |ref|)) = {ratio:.3e}')
        assert ratio <= 1.0, (k, ratio)
    for keep in itertools.chain(itertools.combinations(range(3), 1), itertools.combinations(range(3), 2)):
        some_tables = [t if i in keep else None for i, t in enumerate(tables)]
        some_cots = [c if i in keep else None for i, c in enumerate(cots)]
        got = _run(wide, F64, tables=some_tables, cots=some_cots)
        for i in range(3):
            if i in keep:
                assert np.array_equal(got[i], full[i]), (keep, NAMES[i])
            else:
                assert got[i].shape == (B, 0), (keep, NAMES[i])
        ref_gx = gr.coordinates_and_gradient(x, some_tables, some_cots)[3].reshape(B, 3 * N)
        rel = gr.rel_l2(got[3], ref_gx)
        print(f'tables {[NAMES[i] for i in keep]} alone: gx rel L2 {rel:.3e}')
        assert rel <= TOL64, (keep, rel)
    # the gradient of d.sum() alone, in the three-table run: the triples and quads contribute nothing
    xd = _dev(x, F64, grad=True)
    d, _, _ = geometry.internal_coordinates(xd, *tables)
    (gx,) = torch.autograd.grad(d.sum(), xd)
    ones = [torch.ones(B, gr.WIDE_P, dtype=F64), None, None]
    ref_gx = gr.coordinates_and_gradient(x, tables, ones)[3]
    rel, ratio = gr.rel_l2(gx.cpu().numpy(), ref_gx), gr.f64_element_ratio(gx.cpu().numpy(), ref_gx)
    print(f'gradient of d.sum(): rel L2 {rel:.3e}, largest element ratio {ratio:.3e}')
    assert rel <= TOL64 and ratio <= 1.0


# ------------------------------------------------------------------ (c) bits

@DTYPES
def test_wide_bits_do_not_depend_on_the_batch_or_the_layout(wide, dtype):
    x, tables, cots = wide
    first, again, three = _run(wide, dtype), _run(wide, dtype), _run(wide, dtype, rows=slice(0, 3))
    # the same rows as a column slice of a wider tensor: row stride 3 N + 5, from column 1, not 16-byte aligned
    buf = torch.zeros(B, 3 * N + 5, device='cuda', dtype=dtype)
    buf[:, 1:1 + 3 * N] = _dev(x.reshape(B, 3 * N), dtype)
    xs = buf[:, 1:1 + 3 * N].requires_grad_(True)
    assert xs.stride(0) == 3 * N + 5 and xs.data_ptr() % 16 != 0
    sliced = _kernels(xs, tables, [_dev(c, dtype) for c in cots])
    for k, a, b, c, s in zip(NAMES, first, again, three, sliced):
        assert np.array_equal(a, b, equal_nan=True), k
        assert np.array_equal(a[:3], c, equal_nan=True), k
        assert np.array_equal(a, s, equal_nan=True), k


# ------------------------------------------------------------------ (d) the float32 contract on the golden rows

@pytest.mark.parametrize('case', ['main', 'hub'])
def test_float32_is_float64_arithmetic_rounded_once_on_the_golden_rows(case):
    """The 7-atom rows of tests/golden/geometry.npz (sin(angle) >= 0.1, rejections >= 0.1: better conditioned than the wide
    case, so the same bound holds); the wide rows are in test_wide_values_and_gradients_match_the_float64_reference."""
    g = gu.load('geometry.npz')
    tables = [torch.from_numpy(g[f'{case}/{k}']) for k in ('pairs', 'triples', 'quads')]
    cots = [g[f'{case}/{k}'] for k in ('gd', 'ga', 'gt')]
    x = _dev(g['x'].reshape(11, 21), F32, grad=True)
    got = _kernels(x, tables, [_dev(c, F32) for c in cots])
    ref = gr.coordinates_and_gradient(_rounded(g['x'], F32), tables, [_rounded(c, F32) for c in cots])
    _assert_matches(f'golden {case}', got, ref, F32)


# ------------------------------------------------------------------ (e) a NaN stays where it belongs

def test_degenerate_row_leaves_every_other_row_and_atom_alone(wide):
    """Row 2 gets a coincident pair and a collinear triple.  Atom 64 is in every pair, so the pair that is made coincident
    is the one of atoms 64 and 11: atom 11 is put on atom 64 (which does not move).  The triple is the first one that
    holds neither atom; its three atoms are put on (0, 0, 0), (1, 0, 0), (2, 0, 0), where the cosine is -1 exactly."""
    x, tables, cots = wide
    pairs, triples, quads = tables
    pair = int(((pairs == 64).any(0) & (pairs == 11).any(0)).nonzero()[0])
    triple = int((~((triples == 64) | (triples == 11)).any(0)).nonzero()[0])
    moved = {11, *triples[:, triple].tolist()}
    x2 = x.clone()
    x2[2, 11] = x2[2, 64]
    for step, atom in enumerate(triples[:, triple].tolist()):
        x2[2, atom] = torch.tensor([float(step), 0.0, 0.0], dtype=F64)
    # what the moved atoms can reach: the entries that hold one, and the atoms of those entries
    touched_entries = [torch.isin(t, torch.tensor(sorted(moved))).any(0).numpy() for t in tables]
    touched_atoms = set().union(*(t[:, torch.from_numpy(m)].reshape(-1).tolist() for t, m in zip(tables, touched_entries)))
    free_atoms = np.array([i not in touched_atoms for i in range(N)])
    print(f'row 2: {[int(m.sum()) for m in touched_entries]} entries and {len(touched_atoms)} atoms touch the moved atoms '
          f'{sorted(moved)}; {int(free_atoms.sum())} atoms are free')
    assert touched_entries[0][pair] and touched_entries[1][triple] and free_atoms.sum() >= 40 and not free_atoms[64]

    clean = _run(wide, F64)
    bad = _run((x2, tables, cots), F64)
    others = np.arange(B) != 2
    for k, c, b in zip(NAMES, clean, bad):
        assert np.isfinite(c).all(), k
        assert np.array_equal(c[others], b[others]), k                       # no other row notices
    for k, c, b, m in zip(NAMES[:3], clean, bad, touched_entries):
        assert np.isfinite(b[2][~m]).all() and np.array_equal(c[2][~m], b[2][~m]), k
    c_gx, b_gx = (v[3].reshape(B, N, 3)[2] for v in (clean, bad))
    assert np.isfinite(b_gx[free_atoms]).all() and np.array_equal(c_gx[free_atoms], b_gx[free_atoms])
    print(f'row 2: {int((~np.isfinite(b_gx)).any(1).sum())} atoms have a non-finite cotangent')
    assert bad[0][2, pair] == 0.0


# ------------------------------------------------------------------ (f) polar: several blocks, mixed alignment

N_POLAR = 1031
POLAR_NAMES = ('out0', 'out1', 'log_det_J', 'g0', 'g1')


@pytest.fixture(scope='module')
def polar_case():
    """Radii in [0.5, 3], angles in (-3, 3), three cotangents; the Cartesian inputs are the points of those."""
    g = torch.Generator().manual_seed(5)
    r = 0.5 + 2.5 * torch.rand(N_POLAR, dtype=F64, generator=g)
    angle = 5.99 * (torch.rand(N_POLAR, dtype=F64, generator=g) - 0.5)
    cots = [torch.randn(N_POLAR, dtype=F64, generator=g) for _ in range(3)]
    return {'polar_to_cartesian': (r, angle), 'cartesian_to_polar': (r * angle.cos(), r * angle.sin()), 'cots': cots}


def _shifted(v, dtype, offset, grad=True):
    buf = torch.zeros(len(v) + offset, device='cuda', dtype=dtype)
    buf[offset:] = _dev(v, dtype)
    return buf[offset:].requires_grad_(grad)


def _polar_kernels(name, a, b, cots):
    """``(o0, o1, ldj, ga, gb)`` with the log-det and its cotangent, then ``(o0, o1, ga, gb)`` without, as numpy arrays."""
    fn = getattr(geometry, name)
    outs = fn(a, b, return_log_det_J=True)
    grads = torch.autograd.grad(outs, (a, b), cots)
    plain = fn(a, b)
    plain_grads = torch.autograd.grad(plain, (a, b), cots[:2])
    assert len(plain) == 2 and all(o.shape == a.shape and o.dtype == a.dtype for o in (*outs, *grads, *plain, *plain_grads))
    return [v.detach().cpu().numpy() for v in (*outs, *grads)], [v.detach().cpu().numpy() for v in (*plain, *plain_grads)]


@DTYPES
@pytest.mark.parametrize('name', ['cartesian_to_polar', 'polar_to_cartesian'])
def test_polar_over_several_blocks_and_mixed_alignment(polar_case, name, dtype):
    a64, b64 = polar_case[name]
    cots64 = polar_case['cots']
    size = torch.empty(0, dtype=dtype).element_size()
    pack = 16 // size
    cots = [_dev(c, dtype) for c in cots64]

    a, b = _shifted(a64, dtype, 0), _shifted(b64, dtype, 0)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    with_ldj, without = _polar_kernels(name, a, b, cots)

    # against the float64 reference on the inputs as this dtype holds them
    inputs = [_rounded(v, dtype) for v in (a64, b64)]
    ref_cots = [_rounded(c, dtype) for c in cots64]
    to_cartesian = name == 'polar_to_cartesian'
    ref_with = gr.polar_and_gradient(*inputs, to_cartesian, ref_cots)
    ref_without = gr.polar_and_gradient(*inputs, to_cartesian, ref_cots[:2])
    ref_without = (*ref_without[:2], *ref_without[3:])
    for tag, got, ref, names in (('', with_ldj, ref_with, POLAR_NAMES),
                                 (' (no log-det)', without, ref_without, POLAR_NAMES[:2] + POLAR_NAMES[3:])):
        for k, v, r in zip(names, got, ref):
            is_angle = (name, k) == ('cartesian_to_polar', 'out1')
            if dtype == F64:
                rel = gr.rel_l2(gr.circ(v), gr.circ(r)) if is_angle else gr.rel_l2(v, r)
                print(f'{name} f64 {k}{tag}: rel L2 {rel:.3e} = {rel / TOL64:.3e} of the bound {TOL64:.0e}')
                assert rel <= TOL64, (k, rel)
            else:
                ratio = gr.f32_contract_ratio(v, r, angle=is_angle)
                print(f'{name} f32 {k}{tag}: largest |got - ref| / (2^-23 |ref| + 1e-10 max|ref|) = {ratio:.3f}')
                assert ratio <= 1.0, (k, ratio)

    # only b one element off: everything on the scalar path; both 16 bytes off: still the pack path
    for what, off_a, off_b in (('b shifted by one element', 0, 1), ('both shifted by 16 bytes', pack, pack)):
        a, b = _shifted(a64, dtype, off_a), _shifted(b64, dtype, off_b)
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == (off_b * size) % 16
        for got, ref in zip(_polar_kernels(name, a, b, cots), (with_ldj, without)):
            for k, v, r in zip(POLAR_NAMES, got, ref):
                assert np.array_equal(v, r), (what, k)

    # (1031, 3) as the transpose of a (3, 1031) tensor: read through its strides, the output shape kept
    def columns(v):
        return torch.stack([v, v.flip(0), v.roll(7)])
    a, b = (columns(_dev(v, dtype)).t().requires_grad_(True) for v in (a64, b64))
    assert a.shape == (N_POLAR, 3) and not a.is_contiguous()
    got_with, got_without = _polar_kernels(name, a, b, [columns(c).t() for c in cots])
    for got, ref in ((got_with, with_ldj), (got_without, without)):
        for k, v, r in zip(POLAR_NAMES, got, ref):
            assert v.shape == (N_POLAR, 3), k
            assert np.array_equal(v, columns(torch.from_numpy(r)).t().numpy()), ('transposed', k)


@pytest.mark.parametrize('offset', [0, 1], ids=['packs', 'scalar'])
def test_polar_angle_on_the_axes_and_in_every_quadrant(offset):
    """(+-1, +-0), (+-0, +-1), (+-1, +-1): the angle has the value and the sign of atan2, atan2(-0.0, -1) = -pi included."""
    x = torch.tensor([1, 1, -1, -1, 0.0, -0.0, 0.0, -0.0, 1, 1, -1, -1], dtype=F64)
    y = torch.tensor([0.0, -0.0, 0.0, -0.0, 1, 1, -1, -1, 1, -1, 1, -1], dtype=F64)
    r, angle = geometry.cartesian_to_polar(_shifted(x, F64, offset, grad=False), _shifted(y, F64, offset, grad=False))
    r, angle, ref = r.cpu().numpy(), angle.cpu().numpy(), torch.atan2(y, x).numpy()
    for xi, yi, got, want in zip(x.tolist(), y.tolist(), angle, ref):
        print(f'atan2({yi:+.1f}, {xi:+.1f}) = {got:+.17f} (CPU {want:+.17f})')
    assert np.abs(angle - ref).max() <= 1e-15
    assert np.array_equal(np.signbit(angle), np.signbit(ref))
    assert np.abs(r - torch.sqrt(x * x + y * y).numpy()).max() <= 1e-15


# ------------------------------------------------------------------ (g) the raw ops refuse before any launch

def test_raw_ops_refuse_bad_arguments_before_any_launch(wide, monkeypatch):
    x, tables, cots = wide
    xd = _dev(x.reshape(B, 3 * N), F64)
    prepared = ops.index_tables(*tables, n_atoms=N, device='cuda')
    pairs, triples, quads, start, items = prepared
    gd, ga, gt = (_dev(c, F64) for c in cots)

    def no_launch(name, *args):
        raise AssertionError(f'{name} was called')
    monkeypatch.setattr(ops, 'call', no_launch)

    def refused(fn, *args):
        with pytest.raises(ValueError):
            fn(*args)
    for bad_start in (start[:-1], torch.cat([start, start[-1:]])):
        refused(ops.internal_coordinates, xd, pairs, triples, quads, bad_start, items)
        refused(ops.internal_coordinates_backward, xd, pairs, triples, quads, bad_start, items, gd, ga, gt)
    strided = torch.zeros(3, 2 * gr.WIDE_A, dtype=torch.int32, device='cuda')[:, ::2]
    strided.copy_(triples)
    assert strided.shape == triples.shape and not strided.is_contiguous()
    refused(ops.internal_coordinates, xd, pairs, strided, quads, start, items)
    refused(ops.internal_coordinates_backward, xd, pairs, strided, quads, start, items, gd, ga, gt)
    for i, g in enumerate((gd, ga, gt)):
        for bad in (g[:, :-1], torch.cat([g, g[:, :1]], dim=1)):
            grads = [gd, ga, gt]
            grads[i] = bad
            refused(ops.internal_coordinates_backward, xd, *prepared, *grads)
    a = torch.ones(8, device='cuda', dtype=F64)
    refused(ops.polar, a, a[:7], False, True)
    refused(ops.polar, a.reshape(2, 4), a, True, False)
    refused(ops.polar_backward, a, a, False, a, a[:7], None)
