#!/usr/bin/env python
"""Timings of the edge geometry and pruning ops for README / DESIGN section 4l: ``compute_edge_distances(differentiable=True)``
and ``prune_long_edges(kernel=True)`` against their default torch routes (unchanged since before the ops existed), in one
process: B = 4096 samples x 64 nodes, all ordered pairs (4032 edges each, 1.65e7 edges), unit directions; then the cutoff at
the median distance over ``(edges, distances, directions)``.  Forward and forward + backward, float32 and float64.  One JSON
line per measurement: HIP events, warm-up, the median of the repetitions, the ratio torch / kernel, and the GB/s of the kernel
route on the bytes the algorithm has to move (``*_bytes`` below: every input read once, every output written once).  Run on an
MI355X:

    python tools/measure_edge_ops.py
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfep_amd.nn import graph  # noqa: E402

dev = torch.device('cuda')
B, N_NODES = 4096, 64


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


def geometry_bytes(n, e, s, backward):
    forward = 16 * e + 3 * s * n + 4 * s * e                       # edges, x; distances and directions
    # the backward reads x, the edges, the incidence list and both cotangents, and writes gx
    return forward + (3 * s * n + 16 * e + 16 * e + 8 * (n + 1) + 4 * s * e + 3 * s * n if backward else 0)


def prune_bytes(e, kept, s, backward):
    # the distances twice, the tile offsets, keep_index written and read per tensor, the kept rows read and written
    forward = 2 * s * e + 2 * 8 * (e // 256 + 1) + 8 * kept + 3 * 8 * kept + 2 * (16 + 4 * s) * kept
    # the VJP of each gather: zero the (E, w) cotangent, read the kept rows and ids, add them
    return forward + (4 * s * e + 2 * 8 * kept + 2 * 4 * s * kept if backward else 0)


def report(what, which, dtype, res, n_bytes, extra):
    kernel, torch_ = res['kernel'], res['torch']
    print(json.dumps(dict(what=what, which=which, dtype=str(dtype), kernel_ms=round(kernel[0], 4), torch_ms=round(torch_[0], 4),
                          ratio=round(torch_[0] / kernel[0], 2), kernel_gb_per_s=round(n_bytes / kernel[0] / 1e6, 1),
                          algorithmic_bytes=n_bytes, **extra, kernel_all_ms=kernel[1], torch_all_ms=torch_[1])), flush=True)


edges = graph.get_all_edges(B, N_NODES).to(dev)
E, N = edges.shape[1], B * N_NODES
for dtype in (torch.float32, torch.float64):
    s = 4 if dtype == torch.float32 else 8
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(N, 3, device=dev, dtype=dtype, generator=gen)
    g_r = torch.randn(E, device=dev, dtype=dtype, generator=gen)
    g_d = torch.randn(E, 3, device=dev, dtype=dtype, generator=gen)
    routes = {'kernel': lambda z: graph.compute_edge_distances(z, edges, normalize_directions=True, differentiable=True),
              'torch': lambda z: graph.compute_edge_distances(z, edges, normalize_directions=True)}

    def geometry_forward_backward(route):
        xg = x.detach().requires_grad_(True)
        torch.autograd.grad(route(xg), xg, (g_r, g_d))

    with torch.no_grad():
        (r_k, d_k), (r_t, d_t) = routes['kernel'](x), routes['torch'](x)
        diff = max(float((r_k - r_t).abs().max()), float((d_k - d_t).abs().max()))
        fwd = {name: median_ms(lambda: route(x), 10) for name, route in routes.items()}
    bwd = {name: median_ms(lambda: geometry_forward_backward(route), 5) for name, route in routes.items()}
    extra = dict(n_edges=E, n_nodes=N, max_abs_diff=diff)
    report('edge_geometry', 'forward', dtype, fwd, geometry_bytes(N, E, s, False), extra)
    report('edge_geometry', 'forward + backward', dtype, bwd, geometry_bytes(N, E, s, True), extra)

    cutoff = float(r_t.median())
    routes = {'kernel': lambda r, d: graph.prune_long_edges(cutoff, edges, r, d, kernel=True),
              'torch': lambda r, d: graph.prune_long_edges(cutoff, edges, r, d)}
    with torch.no_grad():
        got, want = routes['kernel'](r_t, d_t), routes['torch'](r_t, d_t)
        same = all(torch.equal(a, b) for a, b in zip(got, want))
        kept = int(want[1].shape[0])
        fwd = {name: median_ms(lambda: route(r_t, d_t), 10) for name, route in routes.items()}
    c_r, c_d = g_r[:kept].contiguous(), g_d[:kept].contiguous()
    del got, want, r_k, d_k

    def prune_forward_backward(route):
        rg, dg = r_t.detach().requires_grad_(True), d_t.detach().requires_grad_(True)
        torch.autograd.grad(route(rg, dg)[1:], (rg, dg), (c_r, c_d))

    bwd = {name: median_ms(lambda: prune_forward_backward(route), 5) for name, route in routes.items()}
    extra = dict(n_edges=E, n_kept=kept, equal_to_torch=same)
    report('prune_long_edges', 'forward', dtype, fwd, prune_bytes(E, kept, s, False), extra)
    report('prune_long_edges', 'forward + backward', dtype, bwd, prune_bytes(E, kept, s, True), extra)
    del x, g_r, g_d, r_t, d_t, c_r, c_d, routes
    torch.cuda.empty_cache()
