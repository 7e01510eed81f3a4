"""Float32 inputs at which the float32 symmetrized Moebius kernels (``symmoebius_kernel<float, DIM, INVERSE>``,
``symmoebius_backward_kernel<float, DIM, INVERSE>``) take every path, with the float64 reference of
``tests/symmoebius_ref.py`` evaluated on those very float32 numbers cast up: the rounding of the inputs is no part of any
error measured against it.  CPU only; shared by ``test_symmoebius_cases_host.py`` (the conditions the cases rest on) and
``test_gpu_symmoebius_f32.py`` (the kernels).  Conventions as ``tests/moebius_cases.py``.

Random cases ``r_d{dim}_b{B}_n{vectors}``: dim 2, 3, 4 are the compile-time instantiations, 5 and 8 the run-time-dimension
kernel and its largest d; 65 vectors give lane 0 a second pass, 5 rows are one more than a workgroup holds.  ``x`` of scale
2, ``w`` of scale 3.  ``e_r07_d{dim}``: random numbers (5 rows of 3 vectors) with ``max_radius = 0.7``.

Edge cases for dim 2, 3, 4 and 5, written out and not drawn (two vectors per row of ``e_wbig``):

* ``e_wzero_*``  rows of random numbers with ``w = 0`` for the whole of row 1 and for the first vector of row 2 (the
                 identity, log-det 0, the zero sub-gradient of ``|w|``, the ``wn > 0`` branch of the VJP);
* ``e_wbig_*``   ``|w| = WBIG = 1e4`` (``r2 = 0.98``, ``H = (1 - r2)^2 = 4e-4`` at the poles): row 0 ``x`` parallel to ``w``,
                 row 1 antiparallel, row 2 orthogonal;
* ``e_xscale_*`` ``|x| = 1e-6`` (row 0) and ``|x| = 1e4`` (row 1), ``w`` of scale 3.

``x = 0`` is left out: the reference is 0 / 0 there.

The poles of ``e_wbig``.  The forward map expands the angle between ``x`` and ``w`` by ``(1 + r2) / (1 - r2) = 100`` there, so
a ``w`` that is parallel to ``x`` only up to float32 rounding (an angle of 6e-8) is no fixed point to 2^-22.  ``x`` and ``w``
are therefore exact float32 multiples of one integer vector of integer norm (``_DIRS``: Pythagorean tuples, ``x = n 2^-k``,
``w = m n`` with ``m`` = WBIG / |n| rounded to 20 bits, so that every product is exact in float32): the float32 numbers the
kernel reads ARE parallel, ``x_i w_j - x_j w_i = 0`` exactly, and orthogonal rows have ``x . w = 0`` exactly.  ``|w|`` is
WBIG to 2^-20 relative.

``WBIG``: 1e4 was kept, no smaller value was needed.  Measured (``reference_stability``; tests/test_symmoebius_cases_host.py
prints it): under one float64 ulp the reference's gradients move by at most 5.3e-7 x 2^-22 (``e_wbig_d2``; the other ``e_wbig``
cases 1.3e-7 to 5.1e-7, everything else below 4e-8), against the 1e-2 x 2^-22 at which a case would be dropped:
``GRAD_DROPPED`` is empty.
"""
import functools
import math

import torch

import symmoebius_ref as ref

F32, F64 = torch.float32, torch.float64
MAX_RADIUS = 0.99
WBIG = 1e4
DIMS = (2, 3, 4, 5, 8)
EDGE_DIMS = (2, 3, 4, 5)
SHAPES = ((1, 1), (5, 1), (1, 65), (5, 65))

RANDOM = tuple(f'r_d{d}_b{B}_n{n}' for d in DIMS for B, n in SHAPES)
EDGE = tuple(f'e_{kind}_d{d}' for d in EDGE_DIMS for kind in ('wzero', 'wbig', 'xscale')) + tuple(f'e_r07_d{d}' for d in DIMS)
NAMES = RANDOM + EDGE

#: Cases left out of the gradient comparison because the float64 reference gradient itself moves by more than 1 % of the
#: 2^-22 bound under a one-ulp (float64) change of its inputs (``reference_stability``; at most two may stand here;
#: tests/test_symmoebius_cases_host.py holds this list to the measurement).
GRAD_DROPPED = ()

#: (integer vector n, an integer vector orthogonal to it, k) per vector slot of an ``e_wbig`` row; both of integer norm;
#: ``x = n 2^-k``: |x| = 0.625 and 3.25 (dim 2), 0.875 and 2.25 (dim 3), 0.5 and 2.25 (dim 4), 0.5 and 3 (dim 5)
_DIRS = {2: (((3, 4), (-4, 3), 3), ((-5, 12), (12, 5), 2)),
         3: (((2, 3, 6), (3, -6, 2), 3), ((1, 4, 8), (4, 7, -4), 2)),
         4: (((1, 1, 1, 1), (1, -1, 1, -1), 2), ((2, 4, 5, 6), (4, -2, 6, -5), 2)),
         5: (((1, 1, 1, 2, 3), (1, 1, 1, 0, -1), 3), ((1, 1, 3, 3, 4), (2, -2, 2, -2, 0), 1))}


def _parse(name):
    p = name.split('_')
    kind = p[0] if p[0] == 'r' else p[1]
    fields = {s[0]: int(s[1:]) for s in p[1:] if s[0] in 'dbn' and s[1:].isdigit()}
    return kind, fields


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _round20(v):
    """``v`` rounded to 20 significant bits."""
    mant, exp = math.frexp(v)
    return math.ldexp(round(mant * 2 ** 20), exp - 20)


def wbig_rows(dim, wbig=WBIG):
    """``(x, w)`` of ``e_wbig``: rows parallel, antiparallel, orthogonal; float64 tensors whose entries are float32 numbers."""
    rows_x, rows_w = [], []
    for relation in ('parallel', 'antiparallel', 'orthogonal'):
        xs, ws = [], []
        for n, perp, k in _DIRS[dim]:
            n, perp = torch.tensor(n, dtype=F64), torch.tensor(perp, dtype=F64)
            xs.append(n * 2.0 ** -k)
            ws.append({'parallel': _round20(wbig / float(n.norm())) * n, 'antiparallel': -_round20(wbig / float(n.norm())) * n,
                       'orthogonal': _round20(wbig / float(perp.norm())) * perp}[relation])
        rows_x.append(torch.cat(xs))
        rows_w.append(torch.cat(ws))
    return torch.stack(rows_x), torch.stack(rows_w)


def _inputs(name):
    """``x, w, gy, gl`` in float64 (rounded to float32 by ``case``), the dimension and ``max_radius``."""
    kind, f = _parse(name)
    dim = f['d']
    gen = torch.Generator().manual_seed(_seed(name))
    max_radius = 0.7 if kind == 'r07' else MAX_RADIUS
    if kind == 'wbig':
        x, w = wbig_rows(dim)
    else:
        B, nvec = (f['b'], f['n']) if kind == 'r' else {'wzero': (3, 3), 'xscale': (2, 2), 'r07': (5, 3)}[kind]
        D = nvec * dim
        x = 2 * torch.randn(B, D, dtype=F64, generator=gen)
        w = 3 * torch.randn(B, D, dtype=F64, generator=gen)
        if kind == 'wzero':
            w[1] = 0.0
            w[2, :dim] = 0.0
        if kind == 'xscale':
            v = x.reshape(B, -1, dim)
            x = (v / v.norm(dim=-1, keepdim=True)).reshape(B, -1)
            x[0] *= 1e-6
            x[1] *= 1e4
    B, D = x.shape
    gy, gl = torch.randn(B, D, dtype=F64, generator=gen), torch.randn(B, dtype=F64, generator=gen)
    return x, w, gy, gl, dim, max_radius


def reference(x, w, gy, gl, dim, max_radius):
    """``{'fwd': (y, log_det_J, grad_x, grad_w), 'inv': ...}`` of ``symmoebius_ref`` in float64 at float32 or float64 inputs;
    the gradients are those of ``(y * gy).sum() + (log_det_J * gl).sum()`` -- autograd, and at the degenerate vectors of the
    inverse the inverse-function theorem on the forward restatement (``symmoebius_ref.inverse_gradients``)."""
    x, w, gy, gl = (t.to(F64) for t in (x, w, gy, gl))
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y, l = ref.symmetrized_moebius(xr, wr, dim, max_radius)
    ((y * gy).sum() + (l * gl).sum()).backward()
    return {'fwd': (y.detach(), l.detach(), xr.grad, wr.grad), 'inv': ref.inverse_gradients(x, w, gy, gl, dim, max_radius)}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: ``x, w, gy, gl`` float32 CPU tensors, ``dim``, ``max_radius``, ``B``, ``nvec``, ``wzero`` (the ``(B, nvec)`` bool of
    vectors with ``w = 0``) and the float64 reference ``fwd`` / ``inv`` = ``(y, log_det_J, grad_x, grad_w)`` at those float32
    numbers.  Computed once per name: treat it as read-only."""
    x, w, gy, gl, dim, max_radius = _inputs(name)
    x, w, gy, gl = (t.to(F32) for t in (x, w, gy, gl))
    B, nvec = x.shape[0], x.shape[1] // dim
    out = dict(name=name, x=x, w=w, gy=gy, gl=gl, dim=dim, max_radius=max_radius, B=B, nvec=nvec,
               wzero=(w.reshape(B, nvec, dim) == 0).all(-1))
    out.update(reference(x, w, gy, gl, dim, max_radius))
    return out


def cotangent_norm(c):
    return float(torch.cat([c['gy'].double().flatten(), c['gl'].double()]).norm())


def rel_l2(got, ref_):
    got, ref_ = got.detach().cpu().to(F64), ref_.detach().cpu().to(F64)
    return float((got - ref_).norm() / ref_.norm().clamp(min=1e-300))


def wzero_gradient_error(c, key, gw):
    """At the vectors with ``w = 0`` the parameter gradient is exactly zero in the reference (the map is even in ``w``), a
    relative error against it is undefined, and both sides hold round-off only: the larger of the two norms there, in units
    of the cotangents' norm (as ``moebius_cases.grad_errors`` for the identity map).  0.0 for a case without such vectors."""
    if not bool(c['wzero'].any()):
        return 0.0
    B, nvec, dim = c['B'], c['nvec'], c['dim']
    at = lambda g: g.detach().cpu().to(F64).reshape(B, nvec, dim)[c['wzero']]                   # noqa: E731
    return max(float(at(gw).norm()), float(at(c[key][3]).norm())) / cotangent_norm(c)


def grad_errors(c, key, gx, gw):
    """(relative L2 of grad x, relative L2 of grad w, ``wzero_gradient_error``) against the reference's."""
    return rel_l2(gx, c[key][2]), rel_l2(gw, c[key][3]), wzero_gradient_error(c, key, gw)


@functools.lru_cache(maxsize=None)
def reference_stability(name):
    """How far the reference's own gradients move when every input is moved by one float64 ulp (a factor ``1 +- 2^-52``,
    signs drawn; zeros stay zeros): the largest of the ``grad_errors`` of the perturbed run against the unperturbed one,
    forward and inverse, as a multiple of the 2^-22 bound of the kernel comparison.  A pole moved by an ulp leaves the pole
    by an angle of 1e-16, far below ``symmoebius_ref.DEGENERATE_B``: it is a degenerate vector of the inverse after the
    move as before it, and the forward direction takes the moved numbers as they are."""
    c = case(name)
    gen = torch.Generator().manual_seed(_seed(name) + 1)
    ulp = lambda t: t.to(F64) * (1.0 + (2.0 * torch.randint(0, 2, t.shape, generator=gen).to(F64) - 1.0) * 2.0 ** -52)  # noqa: E731
    x, w = ulp(c['x']), ulp(c['w'])
    moved = reference(x, w, c['gy'], c['gl'], c['dim'], c['max_radius'])
    return max(max(grad_errors(c, key, moved[key][2], moved[key][3])) for key in ('fwd', 'inv')) / 2.0 ** -22
