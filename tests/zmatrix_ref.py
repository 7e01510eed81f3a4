"""A plain torch-CPU placement of atoms from a Z-matrix, for the tests of csrc/zmatrix.hip: a loop over the rows in
topological order, vectorised over the batch, in the dtype of its inputs, gradients by ``torch.autograd.grad``.  Written
from the formulas of the header comment of csrc/zmatrix.h; it shares no code with ``tfep_amd``.

    b1 = unit(x_k - x_j)
    w  = unit((x_l - x_k) - ((x_l - x_k) . b1) b1)
    x_i = x_j + d (cos a  b1 + sin a (cos t  w - sin t (b1 x w)))
    log_det_J = sum over the placed atoms of 2 log d + log|sin a|

And the three cases of the tests, from fixed seeds (B = 6 rows, which is no multiple of the rows of a workgroup):
    wide   3 fixed atoms and 70 atoms that all reference them: one level that takes two passes of the 64 lanes, and a
           70-item incidence list on each fixed atom
    chain  3 fixed atoms and 40 atoms, each placed from the previous three: 40 levels of one atom
    tree   5 fixed atoms and 60 placed ones, each bonded to a random atom placed before it (7 levels); the atom labels
           are a random permutation (the fixed atoms are no prefix of the range) and the rows are shuffled
Values: d in [0.9, 1.6], a in [0.6, 2.5], t uniform in (-pi, pi).

And the TIER cases (``TIERS``, TIER_B = 7 rows): the same three constructions at the sizes at which the launchers of
csrc/zmatrix.hip change the shape of the launch -- the rows of a workgroup, the LDS it takes, whether the kernel needs
its LDS attribute raised -- one case at least for each kernel in each tier.  ``launch_shape`` restates the launchers' rule
from the header comment of csrc/zmatrix.hip; tests/test_zmatrix_host.py holds the library's own answer against it.

The last section holds what the two GPU test files share: the runs of the kernels and the comparison at the project's
bounds.  Only those functions call ``tfep_amd`` (they import it when called); the reference above them does not.
"""
import collections
import functools
import heapq
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
B = 6
# seeds for which the reference atoms of every row are far from collinear: ``min_reference_sine`` >= MIN_SINE, asserted
# in tests/test_zmatrix_host.py (a condition on the cases, not a tolerance)
SEEDS = {'wide': 1, 'chain': 1, 'tree': 15}
MIN_SINE = 0.3
CASES = tuple(SEEDS)

# ----------------------------------------------------------------------------- the launch tiers

LDS_SHARED, LDS_ATTRIBUTE, MAX_ROWS = 64 * 1024, 48 * 1024, 4
Shape = collections.namedtuple('Shape', 'rows lds_bytes attribute')


def launch_shape(n_atoms, n_ic, backward):
    """The launch of a placement kernel by the rule of the header comment of csrc/zmatrix.hip: a row keeps 24 bytes per
    atom forward and 72 bytes per placed atom backward; a workgroup holds as many rows as fit 64 KiB, four at the most,
    and one when a row alone needs more; above 48 KiB the kernel's LDS attribute has to be raised first."""
    row = 72 * n_ic if backward else 24 * n_atoms
    rows = max(1, min(MAX_ROWS, LDS_SHARED // row)) if row else MAX_ROWS
    return Shape(rows, rows * row, rows * row > LDS_ATTRIBUTE)


# name: the construction, n_fixed, n_ic, and the tier the case is MEANT to land in -- (rows of a workgroup, attribute
# raised) forward and backward --, written down by hand from the table of tiers and held against ``launch_shape`` and the
# library in tests/test_zmatrix_host.py.  The smallest set with every kernel in every tier:
#   forward   4 rows (t200 .. t400), 4 rows + attribute (t600), 3 rows (w700), 2 rows (t1200), 1 row + attribute (t2275),
#             1 row of the CU's whole LDS (f6826: 6826 atoms, 163 824 B); a single row under 48 KiB (1366 .. 2048 atoms)
#             differs from t2275 in nothing but the attribute, which t600 and w700 raise
#   backward  4 rows + attribute (t200), 3 rows (t260, c300), 2 rows (t400), 1 row under 48 KiB (t600), 1 row + attribute
#             (w700), 1 row above 64 KiB (t1200), 1 row of the whole LDS (t2275, f6826: 2275 placed atoms, 163 800 B)
Tier = collections.namedtuple('Tier', 'kind n_fixed n_ic forward backward')
TIERS = {
    't200': Tier('tree', 5, 200, (4, False), (4, True)),
    't260': Tier('tree', 5, 260, (4, False), (3, True)),
    'c300': Tier('chain', 3, 300, (4, False), (3, True)),      # 300 levels of one atom
    't400': Tier('tree', 5, 400, (4, False), (2, True)),
    't600': Tier('tree', 5, 600, (4, True), (1, False)),
    'w700': Tier('wide', 3, 700, (3, True), (1, True)),        # one level of 11 lane passes, 700 items per fixed atom
    't1200': Tier('tree', 5, 1200, (2, True), (1, True)),
    't2275': Tier('tree', 5, 2275, (1, True), (1, True)),
    'f6826': Tier('tree', 4551, 2275, (1, True), (1, True)),
}
TIER_B = 7                  # ragged at 4, 3 and 2 rows a workgroup: 4 + 3, 3 + 3 + 1, 2 + 2 + 2 + 1
# seeds as SEEDS, the lowest that meets MIN_SINE: only the triangles among the fixed atoms depend on them (see ``_tree``)
TIER_SEEDS = {'t200': 12, 't260': 4, 'c300': 1, 't400': 46, 't600': 1, 'w700': 1, 't1200': 24, 't2275': 18, 'f6826': 3}
TIER_CASES = tuple(TIERS)
ALL_CASES = CASES + TIER_CASES


def batch(name):
    """The rows of a case."""
    return TIER_B if name in TIERS else B


def tier_shapes(name):
    """``(forward, backward)`` ``Shape`` of a tier case, from its sizes alone."""
    t = TIERS[name]
    return launch_shape(t.n_fixed + t.n_ic, t.n_ic, False), launch_shape(t.n_fixed + t.n_ic, t.n_ic, True)


def _dot(a, b):
    return (a * b).sum(-1, keepdim=True)


def _unit(a):
    return a / _dot(a, a).sqrt()


def topological_order(z_matrix, fixed_atoms):
    """The rows of ``z_matrix`` in an order in which every reference is in place: repeatedly the first row that can be
    placed."""
    z = [[int(v) for v in row] for row in z_matrix]
    placed = set(int(i) for i in fixed_atoms)
    waiting = collections.defaultdict(list)                    # atom -> the rows that wait for it
    missing = []
    for r, row in enumerate(z):
        refs = [v for v in row[1:] if v not in placed]
        missing.append(len(refs))
        for v in refs:
            waiting[v].append(r)
    ready = [r for r, m in enumerate(missing) if m == 0]       # (ascending: a heap already)
    order = []
    while ready:
        row = heapq.heappop(ready)                             # the first row that can be placed
        order.append(row)
        for r in waiting.pop(z[row][0], ()):
            missing[r] -= 1
            if missing[r] == 0:
                heapq.heappush(ready, r)
    assert len(order) == len(z), 'the Z-matrix has a cycle or a reference that is never placed'
    return order


def place(d, a, t, x_fixed, z_matrix, fixed_atoms):
    """``(x, log_det_J)``: positions (B, n_atoms, 3) and the log-det (B,) from ``d, a, t`` (B, n_ic; column c for row c of
    ``z_matrix``) and ``x_fixed`` (B, n_fixed, 3)."""
    z = [[int(v) for v in row] for row in z_matrix]
    pos = {int(i): x_fixed[:, f] for f, i in enumerate(fixed_atoms)}
    for r in topological_order(z, fixed_atoms):
        i, j, k, l = z[r]
        b1 = _unit(pos[k] - pos[j])
        r_ = pos[l] - pos[k]
        w = _unit(r_ - _dot(r_, b1) * b1)
        n = torch.linalg.cross(b1, w, dim=-1)
        dr, ar, tr = d[:, r:r + 1], a[:, r:r + 1], t[:, r:r + 1]
        pos[i] = pos[j] + dr * (torch.cos(ar) * b1 + torch.sin(ar) * (torch.cos(tr) * w - torch.sin(tr) * n))
    x = torch.stack([pos[i] for i in range(len(pos))], dim=1)
    return x, (2.0 * torch.log(d) + torch.log(torch.abs(torch.sin(a)))).sum(1)


def min_reference_sine(x, z_matrix):
    """The smallest sine of the angle (x_j, x_k, x_l) at x_k over the rows of ``z_matrix`` and the batch: what the
    placement and its derivative divide by."""
    x = torch.as_tensor(x).detach().to(F64)
    z = torch.as_tensor(z_matrix).long()
    u, v = x[:, z[:, 1]] - x[:, z[:, 2]], x[:, z[:, 3]] - x[:, z[:, 2]]
    cos = _dot(u, v) / (_dot(u, u).sqrt() * _dot(v, v).sqrt())
    return float((1.0 - cos * cos).clamp_min(0.0).sqrt().min())


# ----------------------------------------------------------------------------- the cases

def _wide(n_ic, g):
    return torch.tensor([[3 + m] + torch.randperm(3, generator=g).tolist() for m in range(n_ic)]), torch.arange(3)


def _chain(n_ic):
    return torch.tensor([[i, i - 1, i - 2, i - 3] for i in range(3, 3 + n_ic)]), torch.arange(3)


def _tree(n_fixed, n_ic, g):
    """Atom m (before relabelling) is bonded to a random earlier atom j and takes j's own first two references as k and
    l, so the angle (j, k, l) is the angle j was placed with, in [0.6, 2.5] whatever the size of the tree; a fixed j takes
    the next two fixed atoms, and only those triangles depend on the seed."""
    n = n_fixed + n_ic
    label = torch.randperm(n, generator=g)
    refs = {f: [(f + 1) % n_fixed, (f + 2) % n_fixed] for f in range(n_fixed)}
    rows = []
    for m in range(n_fixed, n):
        j = int(torch.randint(m, (1,), generator=g))
        refs[m] = [j, refs[j][0]]
        rows.append(label[[m, j] + refs[j]].tolist())
    rows = [rows[r] for r in torch.randperm(n_ic, generator=g).tolist()]
    return torch.tensor(rows), label[:n_fixed].clone()


def _z_matrix(name, g):
    """``(z_matrix (n_ic, 4), fixed_atoms (n_fixed,))`` int64."""
    kind, n_fixed, n_ic = TIERS[name][:3] if name in TIERS else {'wide': ('wide', 3, 70), 'chain': ('chain', 3, 40),
                                                                  'tree': ('tree', 5, 60)}[name]
    return _wide(n_ic, g) if kind == 'wide' else _chain(n_ic) if kind == 'chain' else _tree(n_fixed, n_ic, g)


def _fixed_positions(n_rows, n_fixed, g):
    """``x_fixed`` (n_rows, n_fixed, 3).  A handful of fixed atoms are random points.  Thousands of them (f6826) are a
    random chain instead, placed with values from the ranges of the cases: the tree hangs an atom on the triangle (f, f +
    1, f + 2) of fixed atoms, and among thousands of random triangles some are always close to collinear, while the angle
    of three consecutive atoms of a chain is the angle the third was placed with.  Only the two triangles that wrap around
    the end of the chain are left to the seed."""
    x = 1.5 * torch.randn(n_rows, min(n_fixed, 5), 3, dtype=F64, generator=g)
    if n_fixed <= 5:
        return x
    uniform = lambda lo, hi: lo + (hi - lo) * torch.rand(n_rows, n_fixed - 3, dtype=F64, generator=g)
    d, a, t = uniform(0.9, 1.6), uniform(0.6, 2.5), -uniform(-math.pi, math.pi)
    return place(d, a, t, x[:, :3], *_chain(n_fixed - 3))[0]


@functools.lru_cache(maxsize=None)
def case(name, seed=None):
    """The float64 inputs of a case: a dict with ``z_matrix``, ``fixed_atoms``, ``d``, ``a``, ``t`` (B, n_ic), ``x_fixed``
    (B, n_fixed, 3) and the cotangents ``cx`` (B, n_atoms, 3) and ``cl`` (B,) of the loss the gradient tests use, B =
    ``batch(name)``.  The tensors are shared between the tests: do not write to them."""
    if name in TIERS:
        seed = TIER_SEEDS[name] if seed is None else seed
        g = torch.Generator().manual_seed(1000 * (11 + TIER_CASES.index(name)) + seed)
    else:
        seed = SEEDS[name] if seed is None else seed
        g = torch.Generator().manual_seed(1000 * (1 + CASES.index(name)) + seed)
    n_rows = batch(name)
    z, fixed = _z_matrix(name, g)
    n_ic, n_fixed = len(z), len(fixed)
    uniform = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, dtype=F64, generator=g)
    return {
        'seed': seed, 'z_matrix': z, 'fixed_atoms': fixed,
        'd': uniform(0.9, 1.6, n_rows, n_ic), 'a': uniform(0.6, 2.5, n_rows, n_ic),
        't': -uniform(-math.pi, math.pi, n_rows, n_ic),             # (rand is in [0, 1): the sign flip leaves out -pi)
        'x_fixed': _fixed_positions(n_rows, n_fixed, g),
        'cx': torch.randn(n_rows, n_ic + n_fixed, 3, dtype=F64, generator=g),
        'cl': torch.randn(n_rows, dtype=F64, generator=g),
    }


INPUTS = ('d', 'a', 't', 'x_fixed')


def inputs(name, rounded, one_ulp_off=False):
    """The four float64 inputs of a case; ``rounded``: rounded to float32 and widened again (what a float32 run sees);
    ``one_ulp_off``: every element moved to the next float64, up or down by a fixed random sign."""
    c = case(name)
    values = [c[k].to(F32).to(F64) if rounded else c[k] for k in INPUTS]
    if one_ulp_off:
        g = torch.Generator().manual_seed(77)
        toward = lambda v: torch.where(torch.rand(v.shape, generator=g) < 0.5, -math.inf, math.inf).to(F64)
        values = [torch.nextafter(v, toward(v)) for v in values]
    return values


@functools.lru_cache(maxsize=None)
def reference(name, rounded=False, dtype=F64, one_ulp_off=False):
    """``{'x', 'log_det_J', 'g_d', 'g_a', 'g_t', 'g_x_fixed'}`` of a case as float64 numpy arrays: the placement run in
    ``dtype`` on the (``rounded``, ``one_ulp_off``) inputs, and the gradient of ``sum(cx * x) + sum(cl * log_det_J)``.
    Computed once."""
    c = case(name)
    args = [v.to(dtype).clone().requires_grad_(True) for v in inputs(name, rounded, one_ulp_off)]
    x, ldj = place(*args, c['z_matrix'], c['fixed_atoms'])
    loss = (c['cx'].to(dtype) * x).sum() + (c['cl'].to(dtype) * ldj).sum()
    grads = torch.autograd.grad(loss, args)
    out = {'x': x, 'log_det_J': ldj, **{'g_' + k: g for k, g in zip(INPUTS, grads)}}
    return {k: v.detach().to(F64).numpy() for k, v in out.items()}


# ----------------------------------------------------------------------------- comparisons

def circ(a):
    """(sin, cos) of angles: a branch flip at +-pi is no error."""
    a = np.asarray(a, dtype=np.float64)
    return np.stack([np.sin(a), np.cos(a)])


def rel_l2(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


# ----------------------------------------------------------------------------- what the GPU tests share

TOL64 = 1e-10
KEYS = ('x', 'log_det_J', 'g_d', 'g_a', 'g_t', 'g_x_fixed')


def dev(a, dtype, grad=False):
    return torch.as_tensor(a).to('cuda', dtype).requires_grad_(grad)


def to_numpy(t):
    return t.detach().cpu().numpy()


def tables(name):
    c = case(name)
    return c['z_matrix'], c['fixed_atoms']


def run(name, dtype, rows=slice(None), x_fixed=None):
    """The kernels on the rows ``rows`` of a case with the case's cotangents: a dict like ``reference``, of tensors."""
    from tfep_amd.utils import geometry
    c = case(name)
    args = [dev(c[k][rows], dtype, grad=True) for k in INPUTS]
    if x_fixed is not None:
        args[3] = x_fixed
    x, ldj = geometry.zmatrix_to_cartesian(*args, *tables(name))
    grads = torch.autograd.grad([x, ldj], args, [dev(c['cx'][rows], dtype).reshape(x.shape), dev(c['cl'][rows], dtype)])
    return dict(zip(KEYS, (x, ldj, *grads)))


def references(name, dtype):
    """The float64 reference on the inputs a run in ``dtype`` sees, and the float32 reference on the same inputs."""
    return reference(name, rounded=dtype == F32), reference(name, rounded=True, dtype=F32)


def assert_close(what, got, ref, ref32, dtype, wrap=np.asarray):
    """``got`` against the float64 reference ``ref``: 1e-10 in float64, 4 x the reference's own float32 error in float32."""
    got = to_numpy(got)
    rel = rel_l2(wrap(got), wrap(ref))
    bound = TOL64 if dtype == F64 else 4.0 * rel_l2(wrap(ref32), wrap(ref))
    print(f'{what} {dtype}: rel L2 {rel:.3e} (bound {bound:.3e})')
    assert got.dtype == (np.float64 if dtype == F64 else np.float32)
    assert rel <= bound, (what, rel, bound)


@functools.lru_cache(maxsize=None)
def reference_round_trip(name, dtype):
    """The reference's own round trip in ``dtype`` on the rounded inputs: place, then the reference internal coordinates."""
    import geometry_ref as gr
    c = case(name)
    z = c['z_matrix']
    d, a, t, x_fixed = (v.to(dtype) for v in inputs(name, rounded=True))
    x, ldj = place(d, a, t, x_fixed, z, c['fixed_atoms'])
    d2, a2, t2 = gr.internal_coordinates(x, z[:, :2].t(), z[:, :3].t(), z.t())
    ldj2 = -(2.0 * torch.log(d2) + torch.log(torch.abs(torch.sin(a2)))).sum(1)
    return {'d': d2, 'a': a2, 't': t2, 'x_fixed': x[:, c['fixed_atoms']], 'log_det_J': ldj, 'minus_back': -ldj2}


ROUND_TRIP_TIER_CASES = ('t260', 't1200', 'f6826')


def check_round_trip(name, dtype, log_dets_against_reference=False):
    """``cartesian_to_zmatrix(zmatrix_to_cartesian(...))`` gives the internal coordinates back, the two log-dets cancel,
    and the flat layout gives the same bits.

    The two log-dets in float32: by default ``-log_det_J back`` against the kernels' own ``log_det_J`` at 4 x the
    mismatch of the reference's two float32 log-dets.  ``log_dets_against_reference``: instead each of the two against
    the float64 reference log-det, the one at 4 x the error of the float32 reference's log-det, the other at 4 x the
    error of the log-det of the float32 reference's own round trip -- errors of float32 sums against a float64 sum, which
    tests/test_zmatrix_host.py asserts to be non-zero; and in float64 each within 1e-10 of the reference."""
    from tfep_amd.utils import geometry
    c, n_rows = case(name), batch(name)
    start = dict(zip(INPUTS, inputs(name, rounded=dtype == F32)))
    x, ldj = geometry.zmatrix_to_cartesian(*(dev(start[k], dtype) for k in INPUTS), *tables(name))
    d, a, t, x_fixed, ldj_back = geometry.cartesian_to_zmatrix(x, *tables(name))
    assert x_fixed.shape == (n_rows, len(c['fixed_atoms']), 3) and d.shape == a.shape == t.shape == start['d'].shape
    ref32 = {k: v.to(F64).numpy() for k, v in reference_round_trip(name, F32).items()}
    for k, got in (('d', d), ('a', a), ('t', t), ('x_fixed', x_fixed)):
        assert_close(f'{name} round trip {k}', got, start[k].numpy(), ref32[k], dtype, circ if k == 't' else np.asarray)
    # the two log-dets cancel
    diff = float((ldj + ldj_back).abs().max())
    print(f'{name} {dtype}: max |log_det_J + log_det_J back| = {diff:.3e}')
    if dtype == F64:
        assert diff <= 1e-9
    if log_dets_against_reference:
        ref = reference(name, rounded=dtype == F32)['log_det_J']
        assert_close(f'{name} log-det', ldj, ref, ref32['log_det_J'], dtype)
        assert_close(f'{name} minus the log-det back', -ldj_back, ref, ref32['minus_back'], dtype)
    elif dtype == F32:
        assert_close(f'{name} minus the log-det back', -ldj_back, to_numpy(ldj).astype(np.float64),
                     ref32['minus_back'] - ref32['log_det_J'] + to_numpy(ldj), dtype)
    # the flat layout gives the same bits
    flat = geometry.zmatrix_to_cartesian(*(dev(start[k], dtype) for k in INPUTS[:3]),
                                         dev(start['x_fixed'], dtype).reshape(n_rows, -1), *tables(name))
    assert flat[0].shape == (n_rows, x.shape[1] * 3) and torch.equal(flat[0].reshape(x.shape), x) and torch.equal(flat[1], ldj)
    again = geometry.cartesian_to_zmatrix(flat[0], *tables(name))
    assert again[3].shape == (n_rows, 3 * len(c['fixed_atoms'])) and torch.equal(again[0], d) and torch.equal(again[4], ldj_back)


def flow(name='tree'):
    """``ZMatrixFlow`` around the 2-layer affine MAF of tools/check_flow_log_det.py on the mixed coordinates of a case, its
    parameters scaled down so that the inner flow stays near the identity and the angles inside (0, pi)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    try:
        from check_flow_log_det import small_maf
    finally:
        sys.path.pop(0)
    from tfep_amd.nn.flows import ZMatrixFlow
    z, fixed = tables(name)
    made = ZMatrixFlow(small_maf(D=3 * (len(z) + len(fixed)), seed=7), z, fixed).to('cuda')
    with torch.no_grad():
        for p in made.parameters():
            p.mul_(0.1)
    return made
