#!/usr/bin/env python
"""Timings of ``CartesianToMixedFlow`` for DESIGN section 4j: the flow around an identity flow on its kernel route
(``internal_coordinates``, the relative-frame kernels, ``zmatrix_place``) against a composition of the package's torch
functions written here (index gathers with ``vector_vector_angle`` / ``proper_dihedral_angle``,
``reference_frame_rotation_matrix(..., project_on_positive_axis=True)``, ``batchwise_rotate``, the polar map and the masks
in torch, the placement level by level), in one process, forward and forward + backward, float32 and float64.
B = 65 536 rows of 1000 atoms, 500 of them Cartesian, the other 500 on a tree of 31 levels.  One JSON line per measurement;
HIP events, one warm-up, the median of 5 runs.  Run on an MI355X:

    python tools/measure_relframe.py
"""
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfep_amd import ops  # noqa: E402
from tfep_amd.nn.flows import CartesianToMixedFlow  # noqa: E402
from tfep_amd.utils import geometry  # noqa: E402

dev = torch.device('cuda')
B, N_ATOMS, N_CART = 65536, 1000, 500
LEVELS = [16] * 30 + [20]                      # 31 levels, 500 placed atoms
REFERENCE = [250, 10, 400]                     # origin, axis, plane
REMOVE = (True, True, True)
REPS = 5


class Identity(torch.nn.Module):
    def forward(self, x):
        return x, torch.zeros(len(x), dtype=x.dtype, device=x.device)

    inverse = forward


def tree_z_matrix(seed=0):
    """The Cartesian atoms 0..499 are the roots; an atom is bonded to a random atom j of the level below and takes j's own j
    and k as k, l."""
    g = torch.Generator().manual_seed(seed)
    refs = {f: [(f + 1) % N_CART, (f + 2) % N_CART] for f in range(N_CART)}
    rows, below, atom = [], list(range(N_CART)), N_CART
    for width in LEVELS:
        level = list(range(atom, atom + width))
        for i in level:
            j = below[int(torch.randint(len(below), (1,), generator=g))]
            rows.append([i, j] + refs[j])
            refs[i] = [j, refs[j][0]]
        below, atom = level, atom + width
    return torch.tensor(rows)


def composition(x, z, cartesian, tables):
    """The whole flow around the identity in torch ops: way in, way back, the summed log-det."""
    n, n_ic = len(x), len(z)
    p = x.reshape(n, -1, 3)
    i, j, k, l = (z[:, c].to(x.device) for c in range(4))
    d = torch.linalg.vector_norm(p[:, i] - p[:, j], dim=-1)
    a = geometry.vector_vector_angle(p[:, i] - p[:, j], p[:, k] - p[:, j])
    t = geometry.proper_dihedral_angle(p[:, j] - p[:, i], p[:, k] - p[:, j], p[:, l] - p[:, k])
    log_det = -(2.0 * torch.log(d) + torch.log(torch.abs(torch.sin(a)))).sum(1)
    (a, la), (t, lt) = geometry.normalize_angles(a), geometry.normalize_torsions(t)
    xc = p[:, cartesian.to(x.device)]
    origin = xc[:, -3]
    xc = xc - origin.unsqueeze(1)
    R = geometry.reference_frame_rotation_matrix(xc[:, -2], xc[:, -1], geometry.get_axis_from_name('x'),
                                                 geometry.get_axis_from_name('y'), project_on_positive_axis=True)
    v = geometry.batchwise_rotate(xc, R)
    d01, d02 = v[:, -2, 0], torch.hypot(v[:, -1, 0], v[:, -1, 1])
    a102n = (torch.atan2(v[:, -1, 1], v[:, -1, 0]) + math.pi) / (2.0 * math.pi)
    log_det = log_det + la + lt - torch.log(d02) - math.log(2.0 * math.pi)
    y = torch.cat([d, a, t, d01[:, None], d02[:, None], a102n[:, None], v[:, :-3].reshape(n, -1)], 1)
    # ... the identity flow ...
    d, a, t, d01, d02, a102n, others = torch.split(y, [n_ic, n_ic, n_ic, 1, 1, 1, y.shape[1] - 3 * n_ic - 3], 1)
    a102 = 2.0 * math.pi * a102n - math.pi
    zero = torch.zeros_like(d01)
    refs = torch.cat([zero, zero, zero, d01, zero, zero, d02 * torch.cos(a102), d02 * torch.sin(a102), zero], 1)
    v = torch.cat([others, refs], 1).reshape(n, -1, 3)
    log_det = log_det + torch.log(d02[:, 0]) + math.log(2.0 * math.pi)
    xc = geometry.batchwise_rotate(v, R, inverse=True) + origin.unsqueeze(1)
    (a, la), (t, lt) = geometry.unnormalize_angles(a), geometry.unnormalize_torsions(t)
    # the placement, level by level
    rows, level_start, fixed = tables.rows.long(), tables.level_start.tolist(), tables.fixed.long()
    out = torch.zeros(n, N_ATOMS, 3, dtype=x.dtype, device=x.device)
    out[:, fixed] = xc
    for s0, s1 in zip(level_start, level_start[1:]):
        i, j, k, l, col = (rows[r, s0:s1] for r in range(5))
        xj, xk, xl = out[:, j], out[:, k], out[:, l]
        b1 = torch.nn.functional.normalize(xk - xj, dim=-1)
        r = xl - xk
        w = torch.nn.functional.normalize(r - (r * b1).sum(-1, keepdim=True) * b1, dim=-1)
        nrm = torch.linalg.cross(b1, w, dim=-1)
        dl, al, tl = d[:, col, None], a[:, col, None], t[:, col, None]
        out[:, i] = xj + dl * (torch.cos(al) * b1 + torch.sin(al) * (torch.cos(tl) * w - torch.sin(tl) * nrm))
    log_det = log_det + la + lt + (2.0 * torch.log(d) + torch.log(torch.abs(torch.sin(a)))).sum(1)
    return out.reshape(n, -1), log_det


def median_ms(fn, reps=REPS, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), times


def main():
    z = tree_z_matrix()
    flow = CartesianToMixedFlow(Identity(), torch.arange(N_CART), z, REFERENCE, REMOVE).to(dev)
    cartesian = flow.cartesian_atom_indices.cpu()
    tables = ops.zmatrix_tables(z, cartesian, N_ATOMS, dev)
    for dtype in (torch.float32, torch.float64):
        # positions the Z-matrix is well conditioned on: placed from random internal coordinates
        g = torch.Generator(device=dev).manual_seed(1)
        rand = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, device=dev, dtype=dtype, generator=g)
        x, _ = geometry.zmatrix_to_cartesian(rand(0.9, 1.6, B, len(z)), rand(0.6, 2.5, B, len(z)), rand(-3.1, 3.1, B, len(z)),
                                             5.0 * torch.randn(B, 3 * N_CART, device=dev, dtype=dtype, generator=g), z, cartesian)
        routes = {'kernel': flow, 'torch': lambda v: composition(v, z, cartesian, tables)}

        def forward_backward(route):
            leaf = x.detach().requires_grad_(True)
            y, ldj = route(leaf)
            (y.sum() + ldj.sum()).backward()

        with torch.no_grad():
            (yk, lk), (yt, lt) = routes['kernel'](x), routes['torch'](x)
            diff = dict(max_abs_dy_kernel=float((yk - x).abs().max()), max_abs_dy_torch=float((yt - x).abs().max()),
                        max_abs_log_det_kernel=float(lk.abs().max()), max_abs_log_det_torch=float(lt.abs().max()))
            del yk, lk, yt, lt
            fwd = {name: median_ms(lambda: route(x)) for name, route in routes.items()}
        bwd = {name: median_ms(lambda: forward_backward(route)) for name, route in routes.items()}
        for what, res in (('forward', fwd), ('forward + backward', bwd)):
            print(json.dumps(dict(what=what, dtype=str(dtype), batch=B, atoms=N_ATOMS, cartesian=N_CART, levels=len(LEVELS),
                                  kernel_ms=round(res['kernel'][0], 3), torch_ms=round(res['torch'][0], 3),
                                  ratio=round(res['torch'][0] / res['kernel'][0], 2), **diff,
                                  kernel_all_ms=res['kernel'][1], torch_all_ms=res['torch'][1])), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
