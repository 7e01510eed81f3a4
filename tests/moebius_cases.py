"""Float32 inputs at which the float32 Moebius kernels (``moebius_kernel<float, DIM>``, ``moebius_backward_kernel<float>``,
the split-f16 side output) take every path, with the float64 reference of ``tests/moebius_ref.py`` evaluated on those very
float32 numbers cast up: the rounding of the inputs is no part of any error measured against it.  CPU only; shared by
``test_moebius_cases_host.py`` (the conditions the cases rest on) and ``test_gpu_moebius_f32.py`` (the kernels).

Random cases ``r_d{dim}_u{0|1}_b{B}_n{vectors}``: dim 2, 3 are the compile-time instantiations, 1, 5, 8 the
runtime-dimension kernel; 65 vectors give lane 0 a second pass, 5 rows are one more than a workgroup holds.  On the unit
sphere ``x`` is normalised in float64 and rounded to float32: both sides see the rounded numbers (``|x| = 1`` to a float32
ulp, which the map's formula with ``|x|^2 := 1`` takes as it is).

Edge cases, for dim 2 and 3 and both sphere settings, written out and not drawn (two vectors per row; directions with
rational components, radii 0.5 and 3 off the sphere):

* ``e_wzero_*``  rows of random numbers with ``w = 0`` for the whole of row 1 and for the first vector of row 2
                 (c = 1, log c = 0, the zero sub-gradient of ``|w|``);
* ``e_wbig_*``   ``|w| = 1e4``, so that ``|u| = 0.99 |x| 1e4 / (1 + 1e4)``: row 0 ``x`` parallel to ``w`` (the smallest
                 ``|d|^2``, c = 197), row 1 antiparallel (the largest, c = 1 / 197), row 2 orthogonal;
* ``e_xscale_*`` off the sphere only: ``|x| = 1e-6`` (row 0) and ``|x| = 1e4`` (row 1), ``w`` of order one;
* ``e_r07_d3_u0`` random numbers with ``max_radius = 0.7``.

``x = 0`` off the sphere is left out: the reference is 0 / 0 there.
"""
import functools

import torch

import moebius_ref

F32, F64 = torch.float32, torch.float64
MAX_RADIUS = 0.99
DIMS = (1, 2, 3, 5, 8)
SHAPES = ((1, 1), (5, 1), (1, 65), (5, 65))

RANDOM = tuple(f'r_d{d}_u{u}_b{B}_n{n}' for d in DIMS for u in (0, 1) for B, n in SHAPES)
EDGE = tuple(f'e_{kind}_d{d}_u{u}' for d in (2, 3) for u in (0, 1) for kind in ('wzero', 'wbig', 'xscale')
             if not (kind == 'xscale' and u == 1)) + ('e_r07_d3_u0',)
NAMES = RANDOM + EDGE

#: Cases left out of the gradient comparison because the float64 reference gradient itself moves by more than 1 % of the
#: 2^-22 bound under a one-ulp (float64) change of its inputs (``reference_stability``; at most two may stand here;
#: tests/test_moebius_cases_host.py holds this list to the measurement).
GRAD_DROPPED = ()

#: (direction, a direction orthogonal to it) per vector slot of an edge row: unit vectors with rational components
_DIRS = {2: (((0.6, 0.8), (-0.8, 0.6)), ((-5 / 13, 12 / 13), (12 / 13, 5 / 13))),
         3: (((2 / 7, 3 / 7, 6 / 7), (3 / 7, -6 / 7, 2 / 7)), ((1 / 9, 4 / 9, 8 / 9), (4 / 9, 7 / 9, -4 / 9)))}
_RADII = (0.5, 3.0)


def _parse(name):
    p = name.split('_')
    kind = p[0] if p[0] == 'r' else p[1]
    fields = {s[0]: int(s[1:]) for s in p[1:] if s[0] in 'dubn' and s[1:].isdigit()}
    return kind, fields


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _on_sphere(x, dim):
    B = x.shape[0]
    v = x.reshape(B, -1, dim)
    return (v / v.norm(dim=-1, keepdim=True)).reshape(B, -1)


def _inputs(name):
    """``x, w, gy, gl`` in float64 (rounded to float32 by ``case``), the dimension, the sphere flag and ``max_radius``."""
    kind, f = _parse(name)
    dim, unit = f['d'], bool(f['u'])
    gen = torch.Generator().manual_seed(_seed(name))
    max_radius = 0.7 if kind == 'r07' else MAX_RADIUS
    if kind == 'wbig':
        rows_x, rows_w = [], []
        for relation in ('parallel', 'antiparallel', 'orthogonal'):
            xs, ws = [], []
            for (e, perp), radius in zip(_DIRS[dim], _RADII):
                e, perp = torch.tensor(e, dtype=F64), torch.tensor(perp, dtype=F64)
                # (the direction as float32 holds it: w is a multiple of the very x the kernel reads, to the rounding of
                # the product)
                xe = (e if unit else radius * e).to(F32).to(F64)
                xs.append(xe)
                ws.append({'parallel': 1e4 * xe / xe.norm(), 'antiparallel': -1e4 * xe / xe.norm(), 'orthogonal': 1e4 * perp}[relation])
            rows_x.append(torch.cat(xs))
            rows_w.append(torch.cat(ws))
        x, w = torch.stack(rows_x), torch.stack(rows_w)
    else:
        B, nvec = (f['b'], f['n']) if kind == 'r' else {'wzero': (3, 3), 'xscale': (2, 2), 'r07': (5, 3)}[kind]
        D = nvec * dim
        x = torch.randn(B, D, dtype=F64, generator=gen)
        if unit:
            x = _on_sphere(x, dim)
        w = torch.randn(B, D, dtype=F64, generator=gen)
        if kind == 'wzero':
            w[1] = 0.0
            w[2, :dim] = 0.0
        if kind == 'xscale':
            x = _on_sphere(x, dim)
            x[0] *= 1e-6
            x[1] *= 1e4
    B, D = x.shape
    gy, gl = torch.randn(B, D, dtype=F64, generator=gen), torch.randn(B, dtype=F64, generator=gen)
    return x, w, gy, gl, dim, unit, max_radius


def reference(x, w, gy, gl, dim, max_radius, unit_sphere):
    """``{'fwd': (y, log_det_J, grad_x, grad_w), 'inv': ...}`` of ``moebius_ref`` in float64 at float32 or float64 inputs;
    the gradients are those of ``(y * gy).sum() + (log_det_J * gl).sum()``."""
    out = {}
    for key, fn in (('fwd', moebius_ref.moebius), ('inv', moebius_ref.moebius_inverse)):
        xr, wr = x.to(F64).clone().requires_grad_(True), w.to(F64).clone().requires_grad_(True)
        y, l = fn(xr, wr, dim, max_radius, unit_sphere)
        ((y * gy.to(F64)).sum() + (l * gl.to(F64)).sum()).backward()
        out[key] = (y.detach(), l.detach(), xr.grad, wr.grad)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: ``x, w, gy, gl`` float32 CPU tensors, ``dim``, ``unit_sphere``, ``max_radius``, ``B``, ``nvec`` and the float64
    reference ``fwd`` / ``inv`` = ``(y, log_det_J, grad_x, grad_w)`` at those float32 numbers.  Computed once per name:
    treat it as read-only."""
    x, w, gy, gl, dim, unit, max_radius = _inputs(name)
    x, w, gy, gl = (t.to(F32) for t in (x, w, gy, gl))
    out = dict(name=name, x=x, w=w, gy=gy, gl=gl, dim=dim, unit_sphere=unit, max_radius=max_radius, B=x.shape[0],
               nvec=x.shape[1] // dim)
    out.update(reference(x, w, gy, gl, dim, max_radius, unit))
    return out


def identity_parameter_gradient(c):
    """dim = 1 off the sphere: ``(|x|^2 - u^2) / (x - u) - u = x`` for every ``w``, the parameter gradient is exactly zero."""
    return c['dim'] == 1 and not c['unit_sphere']


def cotangent_norm(c):
    return float(torch.cat([c['gy'].double().flatten(), c['gl'].double()]).norm())


def rel_l2(got, ref):
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    return float((got - ref).norm() / ref.norm().clamp(min=1e-300))


def grad_errors(c, key, gx, gw):
    """Relative L2 of the two gradients against the reference's; the parameter gradient of the identity map (dim = 1 off the
    sphere) is exactly zero, a relative error against it is undefined, and both sides hold round-off only -- there the
    larger of the two norms, in units of the cotangents' norm, is returned in its place."""
    ex, ew = rel_l2(gx, c[key][2]), rel_l2(gw, c[key][3])
    if identity_parameter_gradient(c):
        ew = max(float(gw.detach().cpu().double().norm()), float(c[key][3].norm())) / cotangent_norm(c)
    return ex, ew


@functools.lru_cache(maxsize=None)
def reference_stability(name):
    """How far the reference's own gradients move when every input is moved by one float64 ulp (a factor ``1 +- 2^-52``,
    signs drawn): the larger of the ``grad_errors`` of the perturbed run against the unperturbed one, forward and
    inverse, as a multiple of the 2^-22 bound of the kernel comparison."""
    c = case(name)
    gen = torch.Generator().manual_seed(_seed(name) + 1)
    ulp = lambda t: t.to(F64) * (1.0 + (2.0 * torch.randint(0, 2, t.shape, generator=gen).to(F64) - 1.0) * 2.0 ** -52)  # noqa: E731
    moved = reference(ulp(c['x']), ulp(c['w']), c['gy'], c['gl'], c['dim'], c['max_radius'], c['unit_sphere'])
    return max(max(grad_errors(c, key, moved[key][2], moved[key][3])) for key in ('fwd', 'inv')) / 2.0 ** -22


# ------------------------------------------------------------------ the split-f16 side output, restated

SPLIT_SCALE = 16384.0           # 2^14: |y| <= 1 on the unit sphere


def split_halves(y):
    """``(hi, lo)`` float16 of a float32 tensor with ``|y| <= 1``: ``t = 2^14 y`` (exact), ``hi`` = t rounded to float16,
    ``lo`` = the residual (exact in float32) rounded to float16."""
    t = y * SPLIT_SCALE
    hi = t.half()
    lo = (t - hi.float()).half()
    return hi, lo


def split_decode(y_split, D):
    """``(hi, lo, padding)`` of a ``(B, cols_padded)`` float32 buffer of split rows: group g (16 halves = 8 words) holds the
    8 hi halves of features 8 g ... 8 g + 7 and then their 8 lo halves; ``padding``: the words past the D / 8 groups."""
    B = y_split.shape[0]
    halves = y_split.contiguous().view(torch.float16).reshape(B, -1)
    grp = halves[:, :2 * D].reshape(B, D // 8, 2, 8)
    return grp[:, :, 0].reshape(B, D), grp[:, :, 1].reshape(B, D), y_split[:, D:]


def split_reconstruct(hi, lo):
    return (hi.double() + lo.double()) / SPLIT_SCALE


def split_bound(y):
    """``|(hi + lo) / 2^14 - y| <= 2^-22 |y| + 2^-39``: hi leaves a residual of at most 2^-11 |t| (11 significant bits), lo
    rounds that to 11 bits again -- 2^-22 |t| -- unless lo is a float16 subnormal, whose spacing is 2^-24: half of it is
    2^-25 in units of t, 2^-39 in units of y."""
    return 2.0 ** -22 * y.double().abs() + 2.0 ** -39
