#!/usr/bin/env python
"""Timings of the Z-matrix placement kernels for DESIGN section 4i: ``utils.geometry.zmatrix_to_cartesian`` against a
level-by-level torch composition of the same placement (written here: per level a gather of the three references, the
frame, the new positions, an indexed write), in one process, forward and forward + backward, float32 and float64.
B = 65 536 rows of 1000 atoms, two Z-matrices: a tree of 31 levels (33 atoms a level, each bonded to a random atom of the
level below) and a chain (997 levels of one atom).  One JSON line per measurement with the time and the bytes per second
the kernels achieve on the tensors they must read and write; HIP events, warm-up, the median of the repetitions.  Run on
an MI355X:

    python tools/measure_zmatrix.py
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfep_amd import ops  # noqa: E402
from tfep_amd.utils import geometry  # noqa: E402

dev = torch.device('cuda')
B, N_ATOMS, N_FIXED, WIDTH = 65536, 1000, 3, 33
N_IC = N_ATOMS - N_FIXED
FIXED = torch.arange(N_FIXED)


def tree_z_matrix(seed=0):
    """Levels of WIDTH atoms; an atom is bonded to a random atom j of the level below and takes j's own j and k as k, l."""
    g = torch.Generator().manual_seed(seed)
    refs = {f: [(f + 1) % 3, (f + 2) % 3] for f in range(3)}
    rows, below, atom = [], [0, 1, 2], N_FIXED
    while atom < N_ATOMS:
        level = list(range(atom, min(atom + WIDTH, N_ATOMS)))
        for i in level:
            j = below[int(torch.randint(len(below), (1,), generator=g))]
            rows.append([i, j] + refs[j])
            refs[i] = [j, refs[j][0]]
        below, atom = level, level[-1] + 1
    return torch.tensor(rows)


def chain_z_matrix():
    return torch.tensor([[i, i - 1, i - 2, i - 3] for i in range(N_FIXED, N_ATOMS)])


def composition(d, a, t, x_fixed, tables):
    """The placement level by level in torch ops, on the level-sorted tables of ``ops.zmatrix_tables``."""
    rows, level_start, fixed = tables.rows.long(), tables.level_start.tolist(), tables.fixed.long()
    x = torch.zeros(len(d), N_ATOMS, 3, dtype=d.dtype, device=d.device)
    x[:, fixed] = x_fixed.reshape(len(d), -1, 3)
    for s0, s1 in zip(level_start, level_start[1:]):
        i, j, k, l, col = (rows[r, s0:s1] for r in range(5))
        xj, xk, xl = x[:, j], x[:, k], x[:, l]
        b1 = torch.nn.functional.normalize(xk - xj, dim=-1)
        r = xl - xk
        w = torch.nn.functional.normalize(r - (r * b1).sum(-1, keepdim=True) * b1, dim=-1)
        n = torch.linalg.cross(b1, w, dim=-1)
        dl, al, tl = d[:, col, None], a[:, col, None], t[:, col, None]
        x[:, i] = xj + dl * (torch.cos(al) * b1 + torch.sin(al) * (torch.cos(tl) * w - torch.sin(tl) * n))
    return x.reshape(len(d), -1), (2.0 * torch.log(d) + torch.log(torch.abs(torch.sin(a)))).sum(1)


def median_ms(fn, reps, warmup=1):
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


for graph, z in (('tree', tree_z_matrix()), ('chain', chain_z_matrix())):
    tables = ops.zmatrix_tables(z, FIXED, N_ATOMS, dev)
    for dtype in (torch.float32, torch.float64):
        g = torch.Generator(device=dev).manual_seed(1)
        rand = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, device=dev, dtype=dtype, generator=g)
        inputs = [rand(0.9, 1.6, B, N_IC), rand(0.6, 2.5, B, N_IC), rand(-3.14, 3.14, B, N_IC),
                  torch.randn(B, 3 * N_FIXED, device=dev, dtype=dtype, generator=g)]
        routes = {'kernel': lambda *v: geometry.zmatrix_to_cartesian(*v, z, FIXED),
                  'torch': lambda *v: composition(*v, tables)}

        def forward_backward(route):
            leaves = [v.detach().requires_grad_(True) for v in inputs]
            x, ldj = route(*leaves)
            (x.sum() + ldj.sum()).backward()

        with torch.no_grad():
            diff = max(float((k - c).abs().max()) for k, c in zip(routes['kernel'](*inputs), routes['torch'](*inputs)))
            fwd = {name: median_ms(lambda: route(*inputs), 5 if name == 'kernel' else 2) for name, route in routes.items()}
        bwd = {name: median_ms(lambda: forward_backward(route), 5 if name == 'kernel' else 2) for name, route in routes.items()}
        # what a pass must move: forward d, a, t, x_fixed in and x, log_det_J out; backward x, d, a, t and the two
        # cotangents in, four cotangents out
        size = torch.finfo(dtype).bits // 8
        moved_fwd = B * size * (3 * N_IC + 3 * N_FIXED + 3 * N_ATOMS + 1)
        moved_bwd = B * size * (3 * N_ATOMS + 3 * N_IC + 3 * N_ATOMS + 1 + 3 * N_IC + 3 * N_FIXED)
        for what, res, moved in (('forward', fwd, moved_fwd), ('forward + backward', bwd, moved_fwd + moved_bwd)):
            print(json.dumps(dict(graph=graph, levels=tables.level_start.numel() - 1, what=what, dtype=str(dtype), batch=B,
                                  atoms=N_ATOMS, kernel_ms=round(res['kernel'][0], 4), torch_ms=round(res['torch'][0], 4),
                                  ratio=round(res['torch'][0] / res['kernel'][0], 2),
                                  kernel_GB_per_s=round(moved / res['kernel'][0] / 1e6, 1), max_abs_diff=diff,
                                  kernel_all_ms=res['kernel'][1], torch_all_ms=res['torch'][1])), flush=True)
        del inputs
        torch.cuda.empty_cache()
