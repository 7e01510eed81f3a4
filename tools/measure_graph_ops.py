#!/usr/bin/env python
"""Timings of the differentiable radial expansion and segment sum for README / DESIGN section 4k:
``torch.ops.tfep.radial_expansion`` (Behler-Parrinello, zero beyond the cutoff, trainable means and widths) against the torch
composition of the same quantities (the expressions of ``tfep/nn/embeddings/radial.py``) at n = 2^22 distances x 64
functions, and ``torch.ops.tfep.segment_sum`` against ``index_add_`` at 2^22 x 64 rows into 2^16 segments; forward and
forward + backward, float32 and float64, in one process.  One JSON line per measurement; HIP events, warm-up, the median of
the repetitions.  Run on an MI355X:

    python tools/measure_graph_ops.py
"""
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfep_amd.torch_ops  # noqa: E402,F401  (registers torch.ops.tfep.*)

dev = torch.device('cuda')
N, K, N_SEGMENTS, R_CUTOFF = 2 ** 22, 64, 2 ** 16, 1.25


def composition(r, means, log_gammas):
    encoding = torch.exp(-log_gammas.exp() * (r.unsqueeze(-1) - means).pow(2))
    s = 0.5 * torch.cos(math.pi / R_CUTOFF * r) + 0.5
    s = torch.where(r > R_CUTOFF, torch.zeros_like(s), s)
    return encoding * s.unsqueeze(-1)


def index_add(data, ids):
    return data.new_zeros(N_SEGMENTS, data.shape[1]).index_add_(0, ids, data)


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


def report(what, dtype, fwd, bwd, diff):
    for which, res in (('forward', fwd), ('forward + backward', bwd)):
        print(json.dumps(dict(what=what, which=which, dtype=str(dtype), kernel_ms=round(res['kernel'][0], 4),
                              torch_ms=round(res['torch'][0], 4), ratio=round(res['torch'][0] / res['kernel'][0], 2),
                              max_abs_diff=diff, kernel_all_ms=res['kernel'][1], torch_all_ms=res['torch'][1])), flush=True)


for dtype in (torch.float32, torch.float64):
    gen = torch.Generator(device=dev).manual_seed(1)
    r = 1.5 * R_CUTOFF * torch.rand(N, device=dev, dtype=dtype, generator=gen)
    means = torch.linspace(0.0, R_CUTOFF, K, device=dev, dtype=dtype).requires_grad_(True)
    log_gammas = torch.full((K,), math.log(1.0 / (3.0 * R_CUTOFF / (K - 1)) ** 2), device=dev, dtype=dtype).requires_grad_(True)
    cot = torch.randn(N, K, device=dev, dtype=dtype, generator=gen)
    routes = {'kernel': lambda z: torch.ops.tfep.radial_expansion(z, means, log_gammas, R_CUTOFF, True, True),
              'torch': lambda z: composition(z, means, log_gammas)}

    def forward_backward(route):
        rg = r.detach().requires_grad_(True)
        torch.autograd.grad(route(rg), (rg, means, log_gammas), cot)

    with torch.no_grad():
        diff = float((routes['kernel'](r) - routes['torch'](r)).abs().max())
        fwd = {name: median_ms(lambda: route(r), 10) for name, route in routes.items()}
    bwd = {name: median_ms(lambda: forward_backward(route), 5) for name, route in routes.items()}
    report('radial_expansion', dtype, fwd, bwd, diff)
    del r, routes
    torch.cuda.empty_cache()

    data = cot                                                         # (2^22, 64)
    ids = torch.randint(0, N_SEGMENTS, (N,), device=dev, generator=gen)
    seg_cot = torch.randn(N_SEGMENTS, K, device=dev, dtype=dtype, generator=gen)
    routes = {'kernel': lambda z: torch.ops.tfep.segment_sum(z, ids, N_SEGMENTS), 'torch': lambda z: index_add(z, ids)}

    def segment_forward_backward(route):
        dg = data.detach().requires_grad_(True)
        torch.autograd.grad(route(dg), dg, seg_cot)

    with torch.no_grad():
        diff = float((routes['kernel'](data) - routes['torch'](data)).abs().max())
        fwd = {name: median_ms(lambda: route(data), 10) for name, route in routes.items()}
    bwd = {name: median_ms(lambda: segment_forward_backward(route), 5) for name, route in routes.items()}
    report('segment_sum', dtype, fwd, bwd, diff)
    del data, cot, ids, seg_cot, routes
    torch.cuda.empty_cache()
