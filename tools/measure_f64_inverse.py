#!/usr/bin/env python
"""Timings of the float64 blocked inverse for README / DESIGN section 4b.  One JSON line per measurement; HIP events, one
warm-up, the median of the repetitions.  Run on an MI355X:

    python tools/measure_f64_inverse.py d300            # D = 300: blocked against the pass per degree, in one process
    python tools/measure_f64_inverse.py d3000           # D = 3000: forward, blocked inverse, block-size sweep, and ONE
                                                        # conditioner pass + transformer inverse of the pass per degree
    python tools/measure_f64_inverse.py small           # small layers: where (if anywhere) the pass per degree is faster
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfep_amd.nn.conditioners import generate_degrees  # noqa: E402
from tfep_amd.nn.flows import MAF  # noqa: E402
from tfep_amd.nn.transformers import NeuralSplineTransformer  # noqa: E402

dev = torch.device('cuda')
F64 = torch.float64


def median_ms(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
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


def mask_flops(layer, B):
    return 2.0 * B * sum(float(torch.count_nonzero(lin.mask)) for lin in layer._conditioner.layers[::2])


which = set(sys.argv[1:]) or {'d300'}
gen = torch.Generator(device=dev).manual_seed(1)

with torch.no_grad():
    if 'd300' in which or 'small' in which:
        sizes = [(300, 8192, 5, 2)] if 'd300' in which else []
        if 'small' in which:
            sizes += [(6, 64, 20, 20), (16, 256, 20, 20), (66, 1024, 10, 5)]
        for D, B, reps_b, reps_p in sizes:
            layer = layer_rq8(D)
            y = 4.0 * (2.0 * torch.rand(B, D, device=dev, dtype=F64, generator=gen) - 1.0)
            layer.blocked_inverse = True
            tb, all_b = median_ms(lambda: layer.inverse(y), reps_b)
            assert layer.last_inverse_route == 'blocked_f64'
            xb = layer.inverse(y)[0]
            layer.blocked_inverse = False
            tp, all_p = median_ms(lambda: layer.inverse(y), reps_p)
            assert layer.last_inverse_route == 'per_degree'
            xp = layer.inverse(y)[0]
            report(what='float64 inverse of one RQ-8 layer, default width', D=D, batch=B,
                   hidden=int(layer._conditioner.dimensions_hidden[0]), block=layer._blocked_f64_host_plan()['block'],
                   blocked_ms=round(tb, 3), per_degree_ms=round(tp, 3), ratio=round(tp / tb, 2), blocked_all_ms=all_b,
                   per_degree_all_ms=all_p, max_abs_diff=float((xb - xp).abs().max()))
            del layer

    if 'd3000' in which:
        D, B = 3000, 8192
        layer = layer_rq8(D)
        x = 4.0 * (2.0 * torch.rand(B, D, device=dev, dtype=F64, generator=gen) - 1.0)
        tf, all_f = median_ms(lambda: layer(x), 3)
        y = layer(x)[0]
        fl = mask_flops(layer, B)
        report(what='float64 forward', D=D, batch=B, ms=round(tf, 2), all_ms=all_f, tflops=round(fl / tf / 1e9, 2))
        blocks = [int(b) for b in os.environ.get('SWEEP', '16,8,4').split(',')]
        for G in blocks:
            layer.inverse_block_f64 = G
            layer._dev = {k: v for k, v in layer._dev.items() if not (isinstance(k, tuple) and k[0] == 'blocked_f64_host')}
            torch.cuda.empty_cache()
            tb, all_b = median_ms(lambda: layer.inverse(y), 3)
            xi = layer.inverse(y)[0]
            report(what='float64 blocked inverse', D=D, batch=B, block_requested=G,
                   block=layer._blocked_f64_host_plan()['block'], n_blocks=len(layer._blocked_f64_host_plan()['blocks']),
                   ms=round(tb, 2), all_ms=all_b, forwards=round(tb / tf, 2), tflops_on_mask_flops=round(fl / tb / 1e9, 2),
                   roundtrip_max_abs=float((xi - x).abs().max()))
        layer._dev = {k: v for k, v in layer._dev.items() if not (isinstance(k, tuple) and k[0] == 'blocked_f64_host')}
        torch.cuda.empty_cache()
        # one pass of the pass per degree: conditioner forward + transformer inverse (the algorithm runs 3000 of them)
        with layer._conditioner.frozen_weights():
            def one_pass():
                par = layer.get_transformer_parameters(x)
                return layer._transformer.inverse(y, par)
            t1, all_1 = median_ms(one_pass, 3)
        report(what='float64 pass per degree: ONE conditioner pass + transformer inverse (weights packed once)', D=D, batch=B,
               ms=round(t1, 2), all_ms=all_1, extrapolated_inverse_s=round(t1 * D / 1e3, 1),
               note='extrapolation: one pass x 3000 degrees, not a measurement of the whole inverse')
