"""A plain torch-CPU restatement of the relative-frame maps of csrc/relframe.hip and of the whole mixed coordinate change
of ``CartesianToMixedFlow``, for the tests: torch expressions in the dtype of their inputs, gradients by
``torch.autograd.grad``.  Written from the formulas of the header comment of csrc/relframe.h; it shares no code with
``tfep_amd``.  The whole change composes with tests/geometry_ref.py (internal coordinates) and tests/zmatrix_ref.py
(placement).

    the last three atoms of x (B, n_c, 3) are the origin o, the axis atom a, the plane atom p
    u = (a - o) / |a - o|,  c = u_x,  w = u x e_x,  R1 = I + [w]x + [w]x^2 / (1 + c);  R1 = diag(-1, -1, 1) when 1 + c <= 1e-12
    q = R1 (p - o),  R2 = cos I + sin [e_x]x + (1 - cos) e_x e_x^T,  cos = |q_y| / |(q_y, q_z)|,  sin = -sign(q_y) q_z / |(q_y, q_z)|,
        R2 = I when q_y == 0;  R = R2 R1
    v_i = R (x_i - o);  d01 = (v_a)_x,  d02 = hypot((v_p)_x, (v_p)_y),  a102n = (atan2((v_p)_y, (v_p)_x) + pi) / (2 pi)
    coords = [d01, d02, a102n | v_i of the other atoms | kept: v_o (3), (v_a)_y,z (2), (v_p)_z (1)]
    log_det_J = -log d02 - log 2 pi;  the way back: x_i = R^T v_i + o, log_det_J = log 2 pi + log d02

The cases, from fixed seeds, B = 6 rows (no multiple of the 4 rows of a workgroup), positions 1.5 * randn:
    refs_only  n_c = 3: no other atom
    wide       n_c = 70: two passes of the 64 lanes
    mixed      9 Cartesian atoms and the 60 placed atoms of the shuffled ``tree`` Z-matrix of tests/zmatrix_ref.py, the 69
               atom labels permuted again, the three reference atoms neither a prefix of the Cartesian atoms nor in order
    many       B = 4099, n_c = 5, values only
    pi         3 rows of n_c = 4; the axis vector of row 1 is exactly (-2, 0, 0): the rotation by pi
Each of the first three runs under all 8 settings of ``remove``; the conditions their seeds meet are asserted in
tests/test_relframe_host.py.
"""
import functools
import itertools
import math

import numpy as np
import torch

import geometry_ref as gr
import zmatrix_ref as zr

F32, F64 = torch.float32, torch.float64
B = 6
SEEDS = {'refs_only': 2, 'wide': 0, 'mixed': 4}
CASES = tuple(SEEDS)
REMOVES = tuple(itertools.product((False, True), repeat=3))
# conditions on the inputs of the cases (not tolerances)
MIN_ONE_PLUS_C, MIN_LENGTH, MAX_ABS_A102, SOME_C_BELOW = 0.05, 0.5, math.pi - 0.1, -0.2
MANY_B, MANY_N_C = 4099, 5
LOG_TWO_PI = math.log(2.0 * math.pi)


# ----------------------------------------------------------------------------- the two maps

def _skew(w):
    z = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], 1), torch.stack([w[:, 2], z, -w[:, 0]], 1),
                        torch.stack([-w[:, 1], w[:, 0], z], 1)], 1)


def rotation(da, dp):
    """R (B, 3, 3) from the axis vector ``da`` and the plane vector ``dp`` (B, 3)."""
    eye = torch.eye(3, dtype=da.dtype)
    ex = eye[0]
    u = da / (da * da).sum(1, keepdim=True).sqrt()
    c = u[:, 0]
    K = _skew(torch.linalg.cross(u, ex.expand_as(u), dim=1))
    safe = (1.0 + c) > 1e-12
    r1 = eye + K + K @ K / torch.where(safe, 1.0 + c, torch.ones_like(c))[:, None, None]
    r1 = torch.where(safe[:, None, None], r1, torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=da.dtype)))
    q = (r1 @ dp.unsqueeze(2)).squeeze(2)
    qy, qz = q[:, 1], q[:, 2]
    norm, sgn = (qy * qy + qz * qz).sqrt(), torch.sign(qy)
    cos = torch.where(sgn == 0, torch.ones_like(qy), qy.abs() / norm)[:, None, None]
    sin = torch.where(sgn == 0, torch.zeros_like(qy), -sgn * qz / norm)[:, None, None]
    r2 = cos * eye + sin * _skew(ex.unsqueeze(0))[0] + (1.0 - cos) * torch.outer(ex, ex)
    return r2 @ r1


def n_kept(remove):
    return sum(n for n, r in zip((3, 2, 1), remove) if not r)


def width(n_c, remove):
    return 3 + 3 * (n_c - 3) + n_kept(remove)


def encode(x, remove):
    """``(coords (B, W), origin (B, 3), R (B, 3, 3), log_det_J (B,))`` of ``x`` (B, n_c, 3)."""
    o = x[:, -3]
    R = rotation(x[:, -2] - o, x[:, -1] - o)
    v = (x - o.unsqueeze(1)) @ R.transpose(1, 2)
    va, vp = v[:, -2], v[:, -1]
    d02 = torch.hypot(vp[:, 0], vp[:, 1])
    a102n = (torch.atan2(vp[:, 1], vp[:, 0]) + math.pi) / (2.0 * math.pi)
    kept = ([] if remove[0] else [v[:, -3]]) + ([] if remove[1] else [va[:, 1:]]) + ([] if remove[2] else [vp[:, 2:]])
    coords = torch.cat([torch.stack([va[:, 0], d02, a102n], 1), v[:, :-3].reshape(len(x), -1), *kept], 1)
    return coords, o, R, -torch.log(d02) - LOG_TWO_PI


def decode(coords, origin, R, remove):
    """``(x (B, n_c, 3), log_det_J (B,))``: the inverse of ``encode``."""
    n_o = (coords.shape[1] - 3 - n_kept(remove)) // 3
    assert coords.shape[1] == width(n_o + 3, remove), (coords.shape, remove)
    d01, d02, a102 = coords[:, 0], coords[:, 1], 2.0 * math.pi * coords[:, 2] - math.pi
    kept = list(torch.split(coords[:, 3 + 3 * n_o:], [n for n, r in zip((3, 2, 1), remove) if not r], dim=1))
    zeros = lambda n: torch.zeros(len(coords), n, dtype=coords.dtype)
    vo = zeros(3) if remove[0] else kept.pop(0)
    va = torch.cat([d01.unsqueeze(1), zeros(2) if remove[1] else kept.pop(0)], 1)
    vp = torch.cat([torch.stack([d02 * torch.cos(a102), d02 * torch.sin(a102)], 1), zeros(1) if remove[2] else kept.pop(0)], 1)
    v = torch.cat([coords[:, 3:3 + 3 * n_o].reshape(len(coords), n_o, 3), vo.unsqueeze(1), va.unsqueeze(1), vp.unsqueeze(1)], 1)
    return v @ R + origin.unsqueeze(1), LOG_TWO_PI + torch.log(d02)


# ----------------------------------------------------------------------------- the whole mixed coordinate change

def to_mixed(x, z_matrix, cartesian, remove):
    """``(y, log_det_J, origin, R)``: ``x`` (B, n_atoms, 3) as ``[d | a / pi | (t + pi) / 2 pi | encode(x[cartesian])]``."""
    z = torch.as_tensor(z_matrix).long()
    d, a, t = gr.internal_coordinates(x, z[:, :2].t(), z[:, :3].t(), z.t())
    log_det = -(2.0 * torch.log(d) + torch.log(torch.abs(torch.sin(a)))).sum(1)
    log_det = log_det - len(z) * math.log(math.pi) - len(z) * LOG_TWO_PI
    coords, origin, R, log_det_frame = encode(x[:, torch.as_tensor(cartesian).long()], remove)
    return torch.cat([d, a / math.pi, (t + math.pi) / (2.0 * math.pi), coords], 1), log_det + log_det_frame, origin, R


def from_mixed(y, origin, R, z_matrix, cartesian, remove):
    """``(x (B, n_atoms, 3), log_det_J)``: the inverse of ``to_mixed``."""
    n = len(z_matrix)
    d, a, t, coords = torch.split(y, [n, n, n, y.shape[1] - 3 * n], dim=1)
    x_cart, log_det_frame = decode(coords, origin, R, remove)
    x, log_det = zr.place(d, a * math.pi, 2.0 * math.pi * t - math.pi, x_cart, z_matrix, cartesian)
    return x, log_det + n * math.log(math.pi) + n * LOG_TWO_PI + log_det_frame


def mixed_flow(x, z_matrix, cartesian, remove, inner):
    """``(y, log_det_J)`` of the whole flow around ``inner`` (mixed coordinates -> (mixed coordinates, log_det_J))."""
    y, log_det_in, origin, R = to_mixed(x, z_matrix, cartesian, remove)
    y, log_det_flow = inner(y)
    x_out, log_det_out = from_mixed(y, origin, R, z_matrix, cartesian, remove)
    return x_out, log_det_in + log_det_flow + log_det_out


# ----------------------------------------------------------------------------- the cases

def _mixed_topology():
    """The ``tree`` Z-matrix of zmatrix_ref with four more Cartesian atoms, relabelled: ``(z_matrix (60, 4), the sorted
    Cartesian atoms (9,), the reference atoms (3,), the Cartesian atoms with the reference atoms last (9,))``."""
    tree = zr.case('tree')
    label = torch.randperm(69, generator=torch.Generator().manual_seed(77))
    z = label[tree['z_matrix']]
    cartesian = torch.cat([label[tree['fixed_atoms']], label[65:]]).sort().values
    reference = cartesian[[6, 1, 4]]
    ordered = torch.cat([cartesian[[0, 2, 3, 5, 7, 8]], reference])
    return z, cartesian, reference, ordered


@functools.lru_cache(maxsize=None)
def case(name, seed=None):
    """The float64 inputs of a case: ``x_cart`` (B, n_c, 3), the reference atoms last.  ``mixed`` also has ``x`` (B, 69, 3),
    ``z_matrix``, ``cartesian`` (sorted), ``reference`` and ``ordered`` (the fixed atoms of the Z-matrix, reference atoms
    last).  The tensors are shared between the tests: do not write to them."""
    seed = SEEDS[name] if seed is None else seed
    g = torch.Generator().manual_seed(5000 * (1 + CASES.index(name)) + seed)
    n_c = {'refs_only': 3, 'wide': 70, 'mixed': 9}[name]
    out = {'seed': seed, 'x_cart': 1.5 * torch.randn(B, n_c, 3, dtype=F64, generator=g)}
    if name == 'mixed':
        z, cartesian, reference, ordered = _mixed_topology()
        tree = zr.case('tree')
        x, _ = zr.place(tree['d'], tree['a'], tree['t'], out['x_cart'], z, ordered)
        out.update(x=x, z_matrix=z, cartesian=cartesian, reference=reference, ordered=ordered)
    return out


@functools.lru_cache(maxsize=None)
def cotangents(name, remove):
    """Random float64 cotangents of a case under ``remove``: of encode's outputs (``coords``, ``origin``, ``R``, ``ldj``),
    of decode's (``x``, ``ldj_back``), the values ``kept`` that decode reads in the kept columns, and for ``mixed`` of the
    flow's outputs (``flow_x``, ``flow_ldj``)."""
    c = case(name)
    n_c = c['x_cart'].shape[1]
    g = torch.Generator().manual_seed(9000 + 100 * CASES.index(name) + REMOVES.index(remove))
    r = lambda *shape: torch.randn(*shape, dtype=F64, generator=g)
    out = {'coords': r(B, width(n_c, remove)), 'origin': r(B, 3), 'R': r(B, 3, 3), 'ldj': r(B), 'x': r(B, n_c, 3),
           'ldj_back': r(B), 'kept': 0.3 * r(B, n_kept(remove))}
    if name == 'mixed':
        out.update(flow_x=r(B, 69, 3), flow_ldj=r(B))
    return out


def _round(t, rounded):
    return t.to(F32).to(F64) if rounded else t


def decode_inputs(name, remove, rounded):
    """``(coords, origin, R)`` float64 for decode: the reference's encode of the case with the kept columns replaced by
    the case's ``kept`` values (the wrapped flow may move them); ``rounded``: as a float32 run sees them."""
    coords, origin, R, _ = encode(case(name)['x_cart'], remove)
    coords = coords.clone()
    if n_kept(remove):
        coords[:, -n_kept(remove):] = cotangents(name, remove)['kept']
    return [_round(t, rounded) for t in (coords, origin, R)]


@functools.lru_cache(maxsize=None)
def reference(name, remove, rounded=False, dtype=F64):
    """Float64 numpy arrays of a case under ``remove``, the maps run in ``dtype`` on the (``rounded``) inputs: encode's
    ``coords, origin, R, ldj`` and ``g_x`` (the gradient of the sum of all four outputs times their cotangents); decode's
    ``x, ldj_back`` and ``g_coords, g_origin, g_R``.  Computed once."""
    cot = {k: v.to(dtype) for k, v in cotangents(name, remove).items()}
    x = _round(case(name)['x_cart'], rounded).to(dtype).clone().requires_grad_(True)
    outs = encode(x, remove)
    (g_x,) = torch.autograd.grad(sum((cot[k] * o).sum() for k, o in zip(('coords', 'origin', 'R', 'ldj'), outs)), x)
    args = [t.to(dtype).clone().requires_grad_(True) for t in decode_inputs(name, remove, rounded)]
    x_back, ldj_back = decode(*args, remove)
    grads = torch.autograd.grad((cot['x'] * x_back).sum() + (cot['ldj_back'] * ldj_back).sum(), args)
    out = dict(zip(('coords', 'origin', 'R', 'ldj', 'g_x', 'x', 'ldj_back', 'g_coords', 'g_origin', 'g_R'),
                   (*outs, g_x, x_back, ldj_back, *grads)))
    return {k: v.detach().to(F64).numpy() for k, v in out.items()}


def fixed_inner(y, by_type):
    """The fixed element-wise wrapped flow of the tests: the distance-type columns times 1.02, the plain Cartesian columns
    plus 0.05; ``log_det_J = n log 1.02``.  ``by_type``: the column lists ``'distances'`` and ``'cartesians'``."""
    scale, shift = torch.ones(y.shape[1], dtype=y.dtype), torch.zeros(y.shape[1], dtype=y.dtype)
    scale[by_type['distances']] = 1.02
    shift[by_type['cartesians']] = 0.05
    log_det = torch.full((len(y),), len(by_type['distances']) * math.log(1.02), dtype=y.dtype)
    return y * scale.to(y.device) + shift.to(y.device), log_det.to(y.device)



def columns_by_type(n_ic, n_c, remove):
    """The ``'distances'`` and ``'cartesians'`` columns of the mixed layout, written from the layout itself."""
    return {'distances': list(range(n_ic)) + [3 * n_ic, 3 * n_ic + 1],
            'cartesians': list(range(3 * n_ic + 3, 3 * n_ic + 3 + 3 * (n_c - 3)))}


@functools.lru_cache(maxsize=None)
def flow_reference(remove, rounded=False, dtype=F64):
    """``{'y', 'log_det_J', 'g_x'}`` of the whole flow on ``mixed`` around ``fixed_inner``, as float64 numpy arrays."""
    c, cot = case('mixed'), cotangents('mixed', remove)
    by_type = columns_by_type(60, 9, remove)
    x = _round(c['x'], rounded).to(dtype).clone().requires_grad_(True)
    y, ldj = mixed_flow(x, c['z_matrix'], c['ordered'], remove, lambda m: fixed_inner(m, by_type))
    (g_x,) = torch.autograd.grad((cot['flow_x'].to(dtype) * y).sum() + (cot['flow_ldj'].to(dtype) * ldj).sum(), x)
    return {k: v.detach().to(F64).numpy() for k, v in (('y', y), ('log_det_J', ldj), ('g_x', g_x))}


@functools.lru_cache(maxsize=None)
def many_case():
    g = torch.Generator().manual_seed(4099)
    return 1.5 * torch.randn(MANY_B, MANY_N_C, 3, dtype=F64, generator=g)


def pi_case():
    """(3, 4, 3) float64, exact in float32: the axis vector of row 1 is exactly (-2, 0, 0)."""
    x = torch.tensor([[[0.5, 1.25, -0.75], [0.25, -0.5, 1.0], [1.5, 0.75, 0.5], [-0.25, 1.0, 2.0]],
                      [[1.0, -0.5, 0.25], [0.5, -0.25, 1.0], [-1.5, -0.25, 1.0], [1.25, 0.5, -0.5]],
                      [[-0.5, 0.75, 1.5], [0.0, 0.5, -1.0], [-1.0, -1.5, 0.25], [0.75, 1.0, 0.5]]], dtype=F64)
    assert (x[1, 2] - x[1, 1]).tolist() == [-2.0, 0.0, 0.0]
    return x


def conditions(x_cart):
    """``(min 1 + c, min |a - o|, min d02, max |a102|, min c)`` over the rows of ``x_cart`` (B, n_c, 3), float64."""
    x = torch.as_tensor(x_cart).to(F64)
    da = x[:, -2] - x[:, -3]
    length = (da * da).sum(1).sqrt()
    c = da[:, 0] / length
    coords = encode(x, (True, True, True))[0]
    a102 = 2.0 * math.pi * coords[:, 2] - math.pi
    return float((1.0 + c).min()), float(length.min()), float(coords[:, 1].min()), float(a102.abs().max()), float(c.min())


rel_l2 = zr.rel_l2
