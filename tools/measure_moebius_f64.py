#!/usr/bin/env python
"""Timings of the opt-in float64 Moebius transformer (``MoebiusTransformer.float64_kernels``) for README / DESIGN section 4b.
Run on an MI355X:

    python tools/measure_moebius_f64.py              # both cases, one after the other
    python tools/measure_moebius_f64.py map          # B = 131 072, D = 1024, d = 2 on the unit sphere (the cfg4-ii shape):
                                                     #   float32 against float64, forward and VJP, with the symmetrized
                                                     #   float64 forward in the same process as the yardstick
    python tools/measure_moebius_f64.py inverse      # B = 8192, D = 1024, repeats=2: the inverse of one float64 MAF layer,
                                                     #   blocked (both switches on) against the pass per degree

The driver starts one fresh worker process per case under ``timeout -k 10 <LIMIT>`` (environment ``LIMIT``, default 300 s) and
stops at the first worker that does not end cleanly: nothing more is started on a device after a failure.  A worker warms up
every variant once, then times ``ROUNDS`` (default 5) alternating rounds with HIP events around each call and prints one JSON
line with the medians and every sample.  No device setting is touched."""
import json
import os
import statistics
import subprocess
import sys

CASES = ('map', 'inverse')


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def _medians(samples):
    return {k + '_ms': round(statistics.median(v), 4) for k, v in samples.items()}


def worker_map():
    import torch
    from tfep_amd import ops
    B, D, dim = 131072, 1024, 2
    dev = torch.device('cuda')
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, D, device=dev, dtype=torch.float64, generator=gen)
    x = (x.reshape(B, -1, dim) / x.reshape(B, -1, dim).norm(dim=-1, keepdim=True)).reshape(B, D)
    w = torch.randn(B, D, device=dev, dtype=torch.float64, generator=gen)
    gy = torch.randn(B, D, device=dev, dtype=torch.float64, generator=gen)
    gl = torch.randn(B, device=dev, dtype=torch.float64, generator=gen)
    data = {'f64': (x, w, gy, gl), 'f32': tuple(t.float() for t in (x, w, gy, gl))}
    variants = {}
    for k, (x_, w_, gy_, gl_) in data.items():
        variants[f'moebius_forward_{k}'] = lambda x_=x_, w_=w_: ops.moebius(x_, w_, dim, 0.99, True)
        variants[f'moebius_vjp_{k}'] = lambda x_=x_, w_=w_, gy_=gy_, gl_=gl_: ops.moebius_backward(x_, w_, dim, 0.99, True, gy_, gl_)
    variants['symmetrized_forward_f64'] = lambda: ops.symmetrized_moebius(x, w, dim, 0.99)
    samples = {k: [] for k in variants}
    for k, fn in variants.items():                                          # warm-up
        _timed(fn)
    for _ in range(int(os.environ.get('ROUNDS', '5'))):
        for k, fn in variants.items():
            samples[k].append(_timed(fn)[0])
    y64, y32 = ops.moebius(x, w, dim, 0.99, True)[0], ops.moebius(*data['f32'][:2], dim, 0.99, True)[0]
    print(json.dumps(dict(what='Moebius map d = 2 on the unit sphere, float32 against float64 (forward, VJP); symmetrized float64 '
                               'forward as the yardstick', batch=B, D=D, **_medians(samples), all_ms=samples,
                          max_abs_diff_f32_f64=float((y64 - y32.double()).abs().max()))), flush=True)


def worker_inverse():
    import torch
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import MoebiusTransformer
    B, D = 8192, 1024
    dev, F64 = torch.device('cuda'), torch.float64
    torch.manual_seed(0)
    torch.set_default_dtype(F64)
    with torch.device(dev):
        tr = MoebiusTransformer(2, unit_sphere=True)
        tr.float64_kernels = True
        layer = MAF(generate_degrees(D, repeats=2), transformer=tr, initialize_identity=False)
    torch.set_default_dtype(torch.float32)
    assert layer.is_float64
    gen = torch.Generator(device=dev).manual_seed(1)
    y = torch.randn(B, D, device=dev, dtype=F64, generator=gen)
    y = (y.reshape(B, -1, 2) / y.reshape(B, -1, 2).norm(dim=-1, keepdim=True)).reshape(B, D)

    def run(flag):
        layer.blocked_inverse_f64_vectors = flag
        ms, out = _timed(lambda: layer.inverse(y))
        assert layer.last_inverse_route == ('blocked_f64' if flag else 'per_degree')
        return ms, out

    with torch.no_grad():
        (_, (xb, lb)), (_, (xp, lp)) = run(True), run(False)           # warm-up of both routes, and the outputs to compare
        samples = dict(blocked=[], per_degree=[])
        for _ in range(int(os.environ.get('ROUNDS', '5'))):
            samples['blocked'].append(run(True)[0])
            samples['per_degree'].append(run(False)[0])
    med = _medians(samples)
    layer.blocked_inverse_f64_vectors = True                            # (the plan of the blocked route: for its block size)
    print(json.dumps(dict(what='float64 inverse of one Moebius MAF layer (d = 2, unit sphere): blocked against the pass per degree',
                          batch=B, D=D, repeats=2, n_degrees=int(layer._inverse_masks.shape[0]),
                          hidden=int(layer._conditioner.dimensions_hidden[0]), block=layer._blocked_f64_host_plan()['block'],
                          **med, ratio=round(med['per_degree_ms'] / med['blocked_ms'], 2), all_ms=samples,
                          max_abs_diff_x=float((xb - xp).abs().max()), max_abs_diff_ldj=float((lb - lp).abs().max()))), flush=True)


def main(argv):
    if argv[:1] == ['--worker']:
        import torch
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert torch.cuda.is_available(), 'this measurement needs an MI355X'
        return {'map': worker_map, 'inverse': worker_inverse}[argv[1]]()
    limit = os.environ.get('LIMIT', '300')
    for case in argv or list(CASES):
        if case not in CASES:
            raise SystemExit(f'unknown case {case!r}: one of {sorted(CASES)}')
        rc = subprocess.run(['timeout', '-k', '10', limit, sys.executable, os.path.abspath(__file__), '--worker', case]).returncode
        if rc != 0:
            raise SystemExit(f'{case}: the worker ended with status {rc}; nothing more is started')


if __name__ == '__main__':
    main(sys.argv[1:])
