#!/usr/bin/env python
"""Timings and peak memory of ``bootstrap(work, fep_estimator, n_resamples=10000)`` on 65 536 samples, the README's example,
for README / DESIGN section 4m: ``resampler='torch'`` (indices from ``torch.randint``, Dirichlet weights from torch's gamma
sampler, then ``tfep_bootstrap_fep``: the route from before the in-kernel resampler existed, unchanged) against
``resampler='kernel'`` (``tfep_bootstrap_table`` + ``tfep_bootstrap_fep_resampled``), in one process.  Standard, biased and
Bayesian bootstrap; float32 and float64 data; ``batch=None`` and ``batch=1000``.  One JSON line per measurement: HIP events
around the whole call after warm-up, the median of the repetitions, the ratio torch / kernel, and
``torch.cuda.max_memory_allocated`` above what was allocated before the call.  Run on an MI355X:

    python tools/measure_bootstrap.py
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfep_amd.analysis import bootstrap, fep_estimator  # noqa: E402

dev = torch.device('cuda')
N, N_RESAMPLES = 65536, 10000


def measure(fn, reps, warmup=1):
    """(median ms, all ms, peak bytes above the starting allocation) of ``fn``."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), times, torch.cuda.max_memory_allocated() - base


gen = torch.Generator(device=dev).manual_seed(1)
for dtype in (torch.float32, torch.float64):
    work = torch.randn(N, device=dev, dtype=dtype, generator=gen) * 2.0
    biased = torch.stack([work, torch.randn(N, device=dev, dtype=dtype, generator=gen)], dim=1)
    for mode, data, bayesian in (('standard', work, False), ('biased', biased, False), ('bayesian', work, True)):
        for batch in (None, 1000):
            res, means = {}, {}
            for resampler in ('torch', 'kernel'):
                def run():
                    out = bootstrap(data, fep_estimator, n_resamples=N_RESAMPLES, batch=batch, bayesian=bayesian,
                                    generator=None if bayesian else 7, resampler=resampler)
                    means[resampler] = float(out['mean']), float(out['standard_deviation'])
                res[resampler] = measure(run, reps=5 if resampler == 'kernel' else 3)
            print(json.dumps(dict(
                what='bootstrap(fep_estimator)', mode=mode, dtype=str(dtype), n=N, n_resamples=N_RESAMPLES, batch=batch,
                torch_ms=round(res['torch'][0], 3), kernel_ms=round(res['kernel'][0], 3),
                ratio=round(res['torch'][0] / res['kernel'][0], 2),
                torch_peak_mib=round(res['torch'][2] / 2 ** 20, 1), kernel_peak_mib=round(res['kernel'][2] / 2 ** 20, 3),
                torch_mean_std=means['torch'], kernel_mean_std=means['kernel'],
                torch_all_ms=res['torch'][1], kernel_all_ms=res['kernel'][1])), flush=True)
    del work, biased, data
    torch.cuda.empty_cache()
