#!/usr/bin/env python
"""Timings of the internal-coordinate kernels for README / DESIGN section 4h: ``utils.geometry.internal_coordinates``
against the torch composition of the same quantities (gather, subtract, norm, cross, dot, atan2 through
``pdist(return_diff=True)``, ``vector_vector_angle`` and ``proper_dihedral_angle``) in one process, forward and forward +
backward, float32 and float64.  One shape: B = 65 536 rows of 1000 atoms, the 999 bonds, 998 angles and 997 torsions of
a chain.  One JSON line per measurement; HIP events, warm-up, the median of the repetitions.  Run on an MI355X:

    python tools/measure_geometry.py
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfep_amd.utils import geometry  # noqa: E402

dev = torch.device('cuda')
B, N_ATOMS = 65536, 1000
i = torch.arange(N_ATOMS)
PAIRS = torch.stack([i[:-1], i[1:]])
TRIPLES = torch.stack([i[:-2], i[1:-1], i[2:]])
QUADS = torch.stack([i[:-3], i[1:-2], i[2:-1], i[3:]])


def composition(x, pairs, triples, quads):
    x = x.reshape(len(x), -1, 3)
    p = [x[:, triples[k]] for k in range(3)]
    q = [x[:, quads[k]] for k in range(4)]
    return (geometry.pdist(x, pairs, return_diff=True)[0], geometry.vector_vector_angle(p[0] - p[1], p[2] - p[1]),
            geometry.proper_dihedral_angle(q[1] - q[0], q[2] - q[1], q[3] - q[2]))


def median_ms(fn, reps, warmup=2):
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


for dtype in (torch.float32, torch.float64):
    x = torch.randn(B, 3 * N_ATOMS, device=dev, dtype=dtype, generator=torch.Generator(device=dev).manual_seed(1))
    dev_tables = [t.to(dev) for t in (PAIRS, TRIPLES, QUADS)]
    routes = {'kernel': lambda z: geometry.internal_coordinates(z, PAIRS, TRIPLES, QUADS),
              'torch': lambda z: composition(z, *dev_tables)}

    def forward_backward(route):
        xg = x.detach().requires_grad_(True)
        d, a, t = route(xg)
        (d.sum() + a.sum() + t.sum()).backward()

    with torch.no_grad():
        diff = max(float((k - t).abs().max()) for k, t in zip(routes['kernel'](x), routes['torch'](x)))
        fwd = {name: median_ms(lambda: route(x), 10 if name == 'kernel' else 5) for name, route in routes.items()}
    bwd = {name: median_ms(lambda: forward_backward(route), 5 if name == 'kernel' else 3) for name, route in routes.items()}
    for what, res in (('forward', fwd), ('forward + backward', bwd)):
        print(json.dumps(dict(what=what, dtype=str(dtype), batch=B, atoms=N_ATOMS, kernel_ms=round(res['kernel'][0], 4),
                              torch_ms=round(res['torch'][0], 4), ratio=round(res['torch'][0] / res['kernel'][0], 2),
                              max_abs_diff=diff, kernel_all_ms=res['kernel'][1], torch_all_ms=res['torch'][1])), flush=True)
    del x
    torch.cuda.empty_cache()
