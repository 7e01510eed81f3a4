"""A plain float64 restatement of the geometry kernels (csrc/geometry.hip), for the tests: torch expressions on CPU
tensors written from the formulations in the header comment of csrc/geometry.h, gradients by ``torch.autograd.grad``;
the wide index tables that take the kernels past one wave pass; and the comparisons the tests share.

    distance  |p1 - p0|
    angle     acos(clamp(u . v / (|u| |v|), -1, 1)),  u = p0 - p1, v = p2 - p1
    dihedral  b0 = p0 - p1, b1 = (p2 - p1) / |p2 - p1|, b2 = p3 - p2; v = b0 - (b0 . b1) b1, w = b2 - (b2 . b1) b1;
              atan2((b1 x v) . w, v . w)
    polar     (x, y) -> (sqrt(x^2 + y^2), atan2(y, x), -log r);  (r, angle) -> (r cos, r sin, +log r)

``tests/test_geometry_host.py`` ties these expressions to the reference's results in ``tests/golden/geometry.npz``.
"""
import math

import numpy as np
import torch

F64 = torch.float64

# the wide case: three trips of the 64-lane atom loop with a ragged last one; four passes of the entry loop, the kind
# boundaries (entries 70 and 137) inside the second and the third pass, the last pass of 10 lanes; one full workgroup of
# four rows and one half-empty one
WIDE_N, WIDE_P, WIDE_A, WIDE_T, WIDE_B = 130, 70, 67, 65, 6
WIDE_USED = 125                       # atoms 125..129 are in no entry
WIDE_HUB = 64                         # in every pair, alternately in slot 0 and slot 1
WIDE_SEED = 0
# conditions of the wide case, asserted on this reference before anything is compared (not tolerances)
MIN_D, MIN_SIN, MIN_REJECTION = 0.1, 0.01, 0.02


def _dot(a, b):
    return (a * b).sum(-1)


def _norm(a):
    return _dot(a, a).sqrt()


def _points(x):
    x = torch.as_tensor(x)
    return x.reshape(x.shape[0], -1, 3)


def _table(table, n_rows):
    return torch.empty(n_rows, 0, dtype=torch.int64) if table is None else torch.as_tensor(table).long()


def _rejections(x, quads):
    q = [x[:, quads[i]] for i in range(4)]
    b0, e, b2 = q[0] - q[1], q[2] - q[1], q[3] - q[2]
    b1 = e / _norm(e).unsqueeze(-1)
    v = b0 - _dot(b0, b1).unsqueeze(-1) * b1
    w = b2 - _dot(b2, b1).unsqueeze(-1) * b1
    return b1, v, w


def internal_coordinates(x, pairs=None, triples=None, quads=None):
    """``(d, a, t)`` of the positions ``x`` (B, n, 3) or (B, 3 n): (B, P), (B, A), (B, T); a table not given is empty."""
    x = _points(x)
    pairs, triples, quads = _table(pairs, 2), _table(triples, 3), _table(quads, 4)
    d = _norm(x[:, pairs[1]] - x[:, pairs[0]])
    u, v = x[:, triples[0]] - x[:, triples[1]], x[:, triples[2]] - x[:, triples[1]]
    a = torch.acos(torch.clamp(_dot(u, v) / (_norm(u) * _norm(v)), -1.0, 1.0))
    b1, v, w = _rejections(x, quads)
    t = torch.atan2(_dot(torch.linalg.cross(b1, v, dim=-1), w), _dot(v, w))
    return d, a, t


def conditioning(x, pairs=None, triples=None, quads=None):
    """What the derivatives divide by: ``(min d, min sin(a), min over the dihedrals of min(|v|, |w|))``; ``inf`` for an
    empty table."""
    x = _points(torch.as_tensor(x).detach().to(F64))
    d, a, _ = internal_coordinates(x, pairs, triples, quads)
    _, v, w = _rejections(x, _table(quads, 4))
    low = lambda t: float(t.min()) if t.numel() else math.inf
    return low(d), low(a.sin()), min(low(_norm(v)), low(_norm(w)))


def polar(a, b, to_cartesian):
    """``(o0, o1, log_det_J)`` of the element-wise polar map, as csrc/geometry.h states it."""
    if to_cartesian:
        return a * torch.cos(b), a * torch.sin(b), torch.log(a)
    r = (a * a + b * b).sqrt()
    return r, torch.atan2(b, a), -torch.log(r)


def _f64(a):
    """A float64 CPU copy, detached (a float32 array is widened exactly)."""
    return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a.detach().cpu()).to(F64).clone()


def coordinates_and_gradient(x, tables, cotangents):
    """``(d, a, t, gx)`` as float64 numpy arrays: the values at ``x`` and the gradient of ``sum(cotangent * output)``;
    a cotangent that is ``None`` counts as zero.  ``gx`` has the shape of ``x``."""
    x = _f64(x).requires_grad_(True)
    outs = internal_coordinates(x, *tables)
    total = sum((_f64(c) * o).sum() for c, o in zip(cotangents, outs) if c is not None and o.numel())
    gx = torch.autograd.grad(total, x)[0] if isinstance(total, torch.Tensor) else torch.zeros_like(x)
    return tuple(v.detach().numpy() for v in (*outs, gx))


def polar_and_gradient(a, b, to_cartesian, cotangents):
    """``(o0, o1, log_det_J, ga, gb)`` as float64 numpy arrays; two cotangents leave the log-det out of the gradient."""
    a, b = _f64(a).requires_grad_(True), _f64(b).requires_grad_(True)
    outs = polar(a, b, to_cartesian)
    ga, gb = torch.autograd.grad(sum((_f64(c) * o).sum() for c, o in zip(cotangents, outs)), (a, b))
    return tuple(v.detach().numpy() for v in (*outs, ga, gb))


# ----------------------------------------------------------------------------- the wide case

def wide_tables(seed=WIDE_SEED):
    """``(pairs, triples, quads)`` int64 of 70 + 67 + 65 entries over 130 atoms.  Every entry holds distinct atoms; atoms
    125..129 are in none; atom 64 is in every pair, in slot 0 of the even ones and slot 1 of the odd ones; atom 3 and
    atom 11 are in the first two pairs, atom 3 in the first triple and the first quad."""
    g = torch.Generator().manual_seed(seed)
    others = torch.tensor([i for i in range(WIDE_USED) if i != WIDE_HUB])
    others = others[torch.randperm(len(others), generator=g)[:WIDE_P]]
    others[0], others[1] = 3, 11
    hub = torch.full((WIDE_P,), WIDE_HUB)
    even = torch.arange(WIDE_P) % 2 == 0
    pairs = torch.stack([torch.where(even, hub, others), torch.where(even, others, hub)])

    def distinct(n_rows, count):
        table = torch.stack([torch.randperm(WIDE_USED, generator=g)[:n_rows] for _ in range(count)], dim=1)
        if not bool((table[:, 0] == 3).any()):
            table[1, 0] = 3
        return table
    return pairs, distinct(3, WIDE_A), distinct(4, WIDE_T)


def wide_case(seed=WIDE_SEED):
    """``(x, tables, cotangents)``: float64 positions (6, 130, 3) from ``randn``, the wide tables, and one ``randn``
    cotangent per output."""
    tables = wide_tables(seed)
    g = torch.Generator().manual_seed(seed + 1000)
    x = torch.randn(WIDE_B, WIDE_N, 3, dtype=F64, generator=g)
    cots = tuple(torch.randn(WIDE_B, c, dtype=F64, generator=g) for c in (WIDE_P, WIDE_A, WIDE_T))
    return x, tables, cots


# ----------------------------------------------------------------------------- comparisons

def wrapped(diff):
    """An angle difference brought to [-pi, pi)."""
    return (np.asarray(diff, dtype=np.float64) + np.pi) % (2.0 * np.pi) - np.pi


def circ(a):
    """(sin, cos) of angles: a branch flip at +-pi is no error."""
    a = np.asarray(a, dtype=np.float64)
    return np.stack([np.sin(a), np.cos(a)])


def rel_l2(got, ref):
    d = np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(d) / max(np.linalg.norm(ref), 1e-300))


def _rows(a):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(1, -1)


def f32_contract_ratio(got, ref, angle=False):
    """The float32 contract of csrc/geometry.h -- fp64 arithmetic on the widened inputs, one rounding on store -- as a
    bound on every element: ``|got - ref| <= 2^-23 |ref| + 1e-10 max|ref|`` with ``ref`` the float64 reference on the
    float32-rounded inputs.  One float32 rounding is 2^-24 relative, the first term is twice that; the floor is the
    project's float64 bound on the largest element of the row (a 1-D array is one row) and covers cancellation in a long
    sum.  ``angle``: the difference is wrapped.  Returns the largest ratio of an error to its bound; not finite if an
    element is."""
    got, ref = _rows(got), _rows(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    diff = wrapped(got - ref) if angle else got - ref
    bound = 2.0 ** -23 * np.abs(ref) + 1e-10 * np.abs(ref).max(axis=1, keepdims=True)
    ratio = np.abs(diff) / bound
    return float(ratio.max()) if np.isfinite(ratio).all() else math.inf


def f64_element_ratio(got, ref, angle=False):
    """The largest ``|got - ref| / (1e-10 max(1, |ref|))`` over the elements (the difference wrapped for an ``angle``)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    diff = wrapped(got - ref) if angle else got - ref
    ratio = np.abs(diff) / (1e-10 * np.maximum(1.0, np.abs(ref)))
    return float(ratio.max()) if np.isfinite(ratio).all() else math.inf
