#!/usr/bin/env python
"""Timings of the frame arithmetic of CenteredCentroidFlow and OrientedFlow for README / DESIGN section 4g: the frame
kernels (``frame_kernels=True``) against the torch ops (``frame_kernels=False``) in one process, forward and forward +
backward, float32 and float64.  One shape: B = 131 072 rows of 1000 atoms, each wrapper around an identity flow, so that
the frame arithmetic (and PartialFlow's column gather / scatter, common to both routes) is all that runs.  One JSON line per
measurement; HIP events, warm-up, the median of the repetitions.  ``kernel_tb_per_s`` counts the bytes the kernel route has
to move: the row read and written once by each of the two launches of the forward, and the cotangent read and written once
by each of the two launches of the backward (the orient backward reads the row as well).  Run on an MI355X:

    python tools/measure_frames.py
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfep_amd.nn.flows import CenteredCentroidFlow, OrientedFlow  # noqa: E402

dev = torch.device('cuda')
B, N_ATOMS = 131072, 1000
D = 3 * N_ATOMS


class Identity(torch.nn.Module):
    def forward(self, x):
        return x, torch.zeros(len(x), device=x.device, dtype=x.dtype)

    inverse = forward

    def n_parameters(self):
        return 0


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


def report(**kw):
    print(json.dumps(kw), flush=True)


FLOWS = {'CenteredCentroidFlow': lambda: CenteredCentroidFlow(Identity(), space_dimension=3),
         'OrientedFlow': lambda: OrientedFlow(Identity())}

for dtype in (torch.float32, torch.float64):
    x = torch.randn(B, D, device=dev, dtype=dtype, generator=torch.Generator(device=dev).manual_seed(1))
    gout = torch.randn(B, D, device=dev, dtype=dtype, generator=torch.Generator(device=dev).manual_seed(2))
    size = x.element_size()
    fwd_bytes = 2 * 2 * B * D * size
    for name, make in FLOWS.items():
        kernels, torch_ops = make().to(dtype).to(dev), make().to(dtype).to(dev)
        kernels.frame_kernels, torch_ops.frame_kernels = True, False
        bwd_bytes = (2 * 2 + (1 if name == 'OrientedFlow' else 0)) * B * D * size

        def forward_backward(flow):
            xg = x.detach().requires_grad_(True)
            flow(xg)[0].backward(gout)

        with torch.no_grad():
            y_k, y_t = kernels(x)[0], torch_ops(x)[0]
            assert kernels.last_route == 'kernels' and torch_ops.last_route == 'torch'
            diff = float((y_k - y_t).abs().max())
            del y_k, y_t
            t_k, all_k = median_ms(lambda: kernels(x), 10)
            t_t, all_t = median_ms(lambda: torch_ops(x), 5)
        report(what='forward', flow=name, dtype=str(dtype), batch=B, atoms=N_ATOMS, kernel_ms=round(t_k, 4),
               torch_ms=round(t_t, 4), ratio=round(t_t / t_k, 2), kernel_tb_per_s=round(fwd_bytes / t_k / 1e9, 3),
               max_abs_diff=diff, kernel_all_ms=all_k, torch_all_ms=all_t)
        tb_k, allb_k = median_ms(lambda: forward_backward(kernels), 5)
        tb_t, allb_t = median_ms(lambda: forward_backward(torch_ops), 3)
        report(what='forward + backward', flow=name, dtype=str(dtype), batch=B, atoms=N_ATOMS, kernel_ms=round(tb_k, 4),
               torch_ms=round(tb_t, 4), ratio=round(tb_t / tb_k, 2),
               kernel_tb_per_s=round((fwd_bytes + bwd_bytes) / tb_k / 1e9, 3), kernel_all_ms=allb_k, torch_all_ms=allb_t)
        del kernels, torch_ops
        torch.cuda.empty_cache()
    del x, gout
    torch.cuda.empty_cache()
