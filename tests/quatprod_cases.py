"""Float32 inputs at which the float32 quaternion product kernels (``quatprod_kernel<float, INVERSE>``,
``quatprod_backward_kernel<float, INVERSE>``) take every path, with the float64 reference of ``tests/quatprod_ref.py``
evaluated on those very float32 numbers cast up: the rounding of the inputs is no part of any error measured against it.
CPU only; shared by ``test_quatprod_cases_host.py`` (the conditions the cases rest on) and ``test_gpu_quatprod_f32.py`` (the
kernels).  Conventions as ``tests/moebius_cases.py``.

Random cases ``r_d4_b{B}_n{quaternions}``: 65 quaternions give lane 0 a second pass, 5 rows are one more than a workgroup
holds.  ``x`` of scale 2, ``p`` of scale 3.

Edge cases, written out and not drawn (scalar LAST: ``(x, y, z, w)``); 2 rows of 3 quaternions unless stated:

* ``e_pscale``  ``|p| = 1e-6`` (row 0) and ``|p| = 1e4`` (row 1): the normalisation ``p / |p|`` and the ``1 / |p|`` of the
                parameter gradient at both ends;
* ``e_pscalar`` ``p = (0, 0, 0, s)``, a pure scalar: ``s`` = 1, -1, 2.5 (row 0: the identity, minus the identity, the
                identity again) and 1e-6, -1e4, 0.75 (row 1);
* ``e_pvector`` a pure vector quaternion, scalar part zero: ``(s, 0, 0, 0)``, ``(0, s, 0, 0)``, ``(0, 0, s, 0)`` (row 0: the
                three units i, j, k, scaled) and three with rational components (row 1);
* ``e_xaxis``   ``x`` with one non-zero component: 4 rows (the component) of 3 quaternions, random ``p``.

``p = 0`` is left out of the compared cases: the reference is 0 / 0 there.
"""
import functools

import torch

from quatprod_ref import quat_torch

F32, F64 = torch.float32, torch.float64
SHAPES = ((1, 1), (5, 1), (1, 65), (5, 65))

RANDOM = tuple(f'r_d4_b{B}_n{n}' for B, n in SHAPES)
EDGE = ('e_pscale', 'e_pscalar', 'e_pvector', 'e_xaxis')
NAMES = RANDOM + EDGE

#: Cases left out of the gradient comparison because the float64 reference gradient itself moves by more than 1 % of the
#: 2^-22 bound under a one-ulp (float64) change of its inputs (``reference_stability``; at most two may stand here;
#: tests/test_quatprod_cases_host.py holds this list to the measurement).
GRAD_DROPPED = ()

PSCALAR = ((1.0, -1.0, 2.5), (1e-6, -1e4, 0.75))
PVECTOR = (((3.0, 0.0, 0.0, 0.0), (0.0, -0.5, 0.0, 0.0), (0.0, 0.0, 1e3, 0.0)),
           ((2 / 7, 3 / 7, 6 / 7, 0.0), (-1.0, 4.0, -8.0, 0.0), (0.6, 0.0, -0.8, 0.0)))


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _inputs(name):
    """``x, p, gy`` in float64 (rounded to float32 by ``case``)."""
    gen = torch.Generator().manual_seed(_seed(name))
    if name.startswith('r_'):
        f = {s[0]: int(s[1:]) for s in name.split('_')[1:]}
        B, n = f['b'], f['n']
    else:
        B, n = (4, 3) if name == 'e_xaxis' else (2, 3)
    x = 2 * torch.randn(B, 4 * n, dtype=F64, generator=gen)
    p = 3 * torch.randn(B, 4 * n, dtype=F64, generator=gen)
    if name == 'e_pscale':
        pv = p.reshape(B, n, 4)
        p = (pv / pv.norm(dim=-1, keepdim=True)).reshape(B, -1)
        p[0] *= 1e-6
        p[1] *= 1e4
    elif name == 'e_pscalar':
        p = torch.zeros(B, n, 4, dtype=F64)
        p[:, :, 3] = torch.tensor(PSCALAR, dtype=F64)
        p = p.reshape(B, -1)
    elif name == 'e_pvector':
        p = torch.tensor(PVECTOR, dtype=F64).reshape(B, -1)
    elif name == 'e_xaxis':
        keep = torch.zeros(B, n, 4, dtype=F64)
        for b in range(B):
            keep[b, :, b] = 1.0
        x = x * keep.reshape(B, -1)
    gy = torch.randn(B, 4 * n, dtype=F64, generator=gen)
    return x, p, gy


def reference(x, p, gy):
    """``{'fwd': (y, grad_x, grad_p), 'inv': ...}`` of ``quat_torch`` in float64 at float32 or float64 inputs; the gradients
    are those of ``(y * gy).sum()`` by autograd (the log-det is the constant zero)."""
    out = {}
    for key, inverse in (('fwd', False), ('inv', True)):
        xr, pr = x.to(F64).clone().requires_grad_(True), p.to(F64).clone().requires_grad_(True)
        y = quat_torch(xr, pr, inverse)
        (y * gy.to(F64)).sum().backward()
        out[key] = (y.detach(), xr.grad, pr.grad)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: ``x, p, gy`` float32 CPU tensors, ``B``, ``nq`` and the float64 reference ``fwd`` / ``inv`` = ``(y, grad_x, grad_p)``
    at those float32 numbers.  Computed once per name: treat it as read-only."""
    x, p, gy = (t.to(F32) for t in _inputs(name))
    out = dict(name=name, x=x, p=p, gy=gy, B=x.shape[0], nq=x.shape[1] // 4)
    out.update(reference(x, p, gy))
    return out


def rel_l2(got, ref):
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    return float((got - ref).norm() / ref.norm().clamp(min=1e-300))


def grad_errors(c, key, gx, gp):
    """Relative L2 of the two gradients against the reference's."""
    return rel_l2(gx, c[key][1]), rel_l2(gp, c[key][2])


@functools.lru_cache(maxsize=None)
def reference_stability(name):
    """How far the reference's own gradients move when every input is moved by one float64 ulp (a factor ``1 +- 2^-52``,
    signs drawn; zeros stay zeros): the larger of the ``grad_errors`` of the perturbed run against the unperturbed one,
    forward and inverse, as a multiple of the 2^-22 bound of the kernel comparison."""
    c = case(name)
    gen = torch.Generator().manual_seed(_seed(name) + 1)
    ulp = lambda t: t.to(F64) * (1.0 + (2.0 * torch.randint(0, 2, t.shape, generator=gen).to(F64) - 1.0) * 2.0 ** -52)  # noqa: E731
    moved = reference(ulp(c['x']), ulp(c['p']), c['gy'])
    return max(max(grad_errors(c, key, moved[key][1], moved[key][2])) for key in ('fwd', 'inv')) / 2.0 ** -22
