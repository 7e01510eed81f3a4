#!/usr/bin/env python
"""Timings of the blocked float64 backward through the MAF inverse (``layer.blocked_inverse_backward``) for README /
DESIGN section 4b.  One JSON line per measurement; HIP events, one warm-up round, medians of alternating rounds, peak
memory per route.  Run on an MI355X:

    python tools/measure_inverse_backward_f64.py d300      # D = 300, B = 1024: inverse + backward, flag on against off
    python tools/measure_inverse_backward_f64.py d3000     # D = 3000, B = 8192: flag on only, beside forward + backward
    python tools/measure_inverse_backward_f64.py quat256   # 256 features of quaternions, 64 degrees, B = 1024:
    python tools/measure_inverse_backward_f64.py sym2_256  # 256 features of symmetrized Moebius 2-vectors, 128 degrees:
                                                           #   ``blocked_inverse_backward_vectors`` on against off

One shape per process (a fresh process per shape keeps one shape's kept conditioner passes out of the next one's peak), each
under a time limit of its own, e.g. ``timeout -k 10 600 python tools/measure_inverse_backward_f64.py quat256``; ``D=128``
in the environment halves the vector shapes.
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfep_amd.nn.conditioners import generate_degrees  # noqa: E402
from tfep_amd.nn.flows import MAF  # noqa: E402
from tfep_amd.nn.transformers import (NeuralSplineTransformer, QuaternionProductTransformer,  # noqa: E402
                                      SymmetrizedMoebiusTransformer)

dev = torch.device('cuda')
F64 = torch.float64


def report(**kw):
    print(json.dumps(kw), flush=True)


def layer_rq8(D):
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        with torch.device(dev):
            torch.manual_seed(0)
            layer = MAF(generate_degrees(D), transformer=NeuralSplineTransformer(torch.full((D,), -5.0), torch.full((D,), 5.0), 8),
                        initialize_identity=False)
    finally:
        torch.set_default_dtype(old)
    assert layer.is_float64
    return layer


def layer_vectors(D, transformer, repeats):
    """One float64 layer of vector-valued members, default width, every vector inside one degree; all opt-ins on."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        with torch.device(dev):
            torch.manual_seed(0)
            layer = MAF(generate_degrees(D, repeats=repeats), transformer=transformer, initialize_identity=False)
    finally:
        torch.set_default_dtype(old)
    assert layer.is_float64
    layer.blocked_inverse_f64_vectors = True
    layer.blocked_inverse_backward = True
    return layer


def inverse_backward_vectors(layer, y0, flag):
    def run():
        layer.blocked_inverse_backward_vectors = flag
        layer.zero_grad(set_to_none=True)
        y = y0.clone().requires_grad_(True)
        x, ldj = layer.inverse(y)
        (x.square().sum() + ldj.sum()).backward()
        assert layer.last_inverse_backward_route == ('blocked_f64' if flag else 'per_degree')
    return run


def timed(fn):
    """``(ms, peak bytes above what was allocated before the call)`` of one call."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base


def inverse_backward(layer, y0, flag):
    def run():
        layer.blocked_inverse_backward = flag
        layer.zero_grad(set_to_none=True)
        y = y0.clone().requires_grad_(True)
        x, ldj = layer.inverse(y)
        (x.square().sum() + ldj.sum()).backward()
    return run


def forward_backward(layer, x0):
    def run():
        layer.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y, ldj = layer(x)
        (y.square().sum() + ldj.sum()).backward()
    return run


def alternate(runs, rounds):
    """Medians of ``rounds`` alternating rounds over the named callables (one warm-up round first)."""
    for fn in runs.values():
        fn()
    ms = {k: [] for k in runs}
    peak = {k: 0 for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            t, p = timed(fn)
            ms[k].append(t)
            peak[k] = max(peak[k], p)
    return {k: statistics.median(v) for k, v in ms.items()}, ms, peak


which = set(sys.argv[1:]) or {'d300'}
gen = torch.Generator(device=dev).manual_seed(1)

if 'd300' in which:
    D, B = 300, 1024
    layer = layer_rq8(D)
    y0 = 4.0 * (2.0 * torch.rand(B, D, device=dev, dtype=F64, generator=gen) - 1.0)
    med, all_ms, peak = alternate({'on': inverse_backward(layer, y0, True), 'off': inverse_backward(layer, y0, False),
                                   'forward_backward': forward_backward(layer, y0)}, rounds=int(os.environ.get('ROUNDS', 5)))
    assert layer.last_inverse_route == 'blocked_f64'
    report(what='float64 inverse + backward of one RQ-8 layer, default width', D=D, batch=B,
           block=layer._blocked_f64_backward_plan()['block'], n_blocks=len(layer._blocked_f64_backward_plan()['blocks']),
           flag_on_ms=round(med['on'], 3), flag_off_ms=round(med['off'], 3), ratio=round(med['off'] / med['on'], 2),
           forward_backward_ms=round(med['forward_backward'], 3),
           flag_on_peak_mib=round(peak['on'] / 2 ** 20, 1), flag_off_peak_mib=round(peak['off'] / 2 ** 20, 1), all_ms=all_ms)

if 'd3000' in which:
    D, B = 3000, 8192
    layer = layer_rq8(D)
    y0 = 4.0 * (2.0 * torch.rand(B, D, device=dev, dtype=F64, generator=gen) - 1.0)
    med, all_ms, peak = alternate({'on': inverse_backward(layer, y0, True), 'forward_backward': forward_backward(layer, y0)},
                                  rounds=int(os.environ.get('ROUNDS', 3)))
    assert layer.last_inverse_backward_route == 'blocked_f64'
    report(what='float64 inverse + backward of one RQ-8 layer, default width, flag on only', D=D, batch=B,
           block=layer._blocked_f64_backward_plan()['block'], n_blocks=len(layer._blocked_f64_backward_plan()['blocks']),
           flag_on_ms=round(med['on'], 2), forward_backward_ms=round(med['forward_backward'], 2),
           multiple_of_forward_backward=round(med['on'] / med['forward_backward'], 2),
           flag_on_peak_gib=round(peak['on'] / 2 ** 30, 2), forward_backward_peak_gib=round(peak['forward_backward'] / 2 ** 30, 2),
           all_ms=all_ms)

for name, make, repeats in (('quat256', QuaternionProductTransformer, 4), ('sym2_256', lambda: SymmetrizedMoebiusTransformer(2), 2)):
    if name not in which:
        continue
    D, B = int(os.environ.get('D', 256)), 1024
    layer = layer_vectors(D, make(), repeats)
    with torch.no_grad():                                   # images of random points: no zero vector
        y0 = layer(torch.randn(B, D, device=dev, dtype=F64, generator=gen))[0]
    med, all_ms, peak = alternate({'on': inverse_backward_vectors(layer, y0, True), 'off': inverse_backward_vectors(layer, y0, False)},
                                  rounds=int(os.environ.get('ROUNDS', 5)))
    assert layer.last_inverse_route == 'blocked_f64'
    layer.blocked_inverse_backward_vectors = True
    plan = layer._blocked_f64_backward_plan()
    report(what=f'float64 inverse + backward of one {type(layer._transformer).__name__} layer, default width, '
                'blocked_inverse_backward_vectors on against off', shape=name, D=D, n_degrees=D // repeats, batch=B,
           block=plan['block'], n_blocks=len(plan['blocks']), flag_on_ms=round(med['on'], 3), flag_off_ms=round(med['off'], 3),
           ratio=round(med['off'] / med['on'], 2), flag_on_peak_mib=round(peak['on'] / 2 ** 20, 1),
           flag_off_peak_mib=round(peak['off'] / 2 ** 20, 1), all_ms=all_ms)
