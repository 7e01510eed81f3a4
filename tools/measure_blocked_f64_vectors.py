#!/usr/bin/env python
"""Timings of the opt-in float64 blocked inverse for vector-valued transformers (``blocked_inverse_f64_vectors``) for README /
DESIGN section 4b: one float64 MAF layer at B = 8192, the flag on against the flag off (the pass per degree: the default
route) in the same process on the same input, alternating.  Run on an MI355X:

    python tools/measure_blocked_f64_vectors.py              # both cases, one after the other
    python tools/measure_blocked_f64_vectors.py quat         # D = 1024 of quaternions, generate_degrees(..., repeats=4)
    python tools/measure_blocked_f64_vectors.py sym2         # D = 1024 of symmetrized Moebius d = 2, repeats=2

The driver starts one fresh worker process per case under ``timeout -k 10 <LIMIT>`` (environment ``LIMIT``, default 300 s) and
stops at the first worker that does not end cleanly: nothing more is started on a device after a failure.  A worker warms up
both routes, then times ``ROUNDS`` (default 5) alternating pairs with HIP events around the whole ``layer.inverse`` call and
prints one JSON line: the medians, every sample, the ratio, and the largest difference between the two routes' results.
No device setting is touched."""
import json
import os
import statistics
import subprocess
import sys

CASES = {'quat': dict(D=1024, repeats=4), 'sym2': dict(D=1024, repeats=2)}
B = 8192


def worker(case):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import QuaternionProductTransformer, SymmetrizedMoebiusTransformer
    assert torch.cuda.is_available(), 'this measurement needs an MI355X'
    dev, F64 = torch.device('cuda'), torch.float64
    cfg = CASES[case]
    D = cfg['D']
    torch.manual_seed(0)
    torch.set_default_dtype(F64)
    with torch.device(dev):
        tr = QuaternionProductTransformer() if case == 'quat' else SymmetrizedMoebiusTransformer(2)
        layer = MAF(generate_degrees(D, repeats=cfg['repeats']), transformer=tr, initialize_identity=False)
    torch.set_default_dtype(torch.float32)
    assert layer.is_float64
    gen = torch.Generator(device=dev).manual_seed(1)
    y = torch.randn(B, D, device=dev, dtype=F64, generator=gen)

    def run(flag):
        layer.blocked_inverse_f64_vectors = flag
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = layer.inverse(y)
        e1.record()
        torch.cuda.synchronize()
        assert layer.last_inverse_route == ('blocked_f64' if flag else 'per_degree')
        return e0.elapsed_time(e1), out

    with torch.no_grad():
        (_, (xb, lb)), (_, (xp, lp)) = run(True), run(False)           # warm-up of both routes, and the outputs to compare
        on, off = [], []
        for _ in range(int(os.environ.get('ROUNDS', '5'))):
            on.append(run(True)[0])
            off.append(run(False)[0])
    print(json.dumps(dict(
        what='float64 inverse of one MAF layer: blocked_inverse_f64_vectors on against off (pass per degree)', case=case, D=D,
        batch=B, repeats=cfg['repeats'], n_degrees=int(layer._inverse_masks.shape[0]),
        hidden=int(layer._conditioner.dimensions_hidden[0]), block=layer._blocked_f64_host_plan()['block'],
        blocked_ms=round(statistics.median(on), 3), per_degree_ms=round(statistics.median(off), 3),
        ratio=round(statistics.median(off) / statistics.median(on), 2), blocked_all_ms=on, per_degree_all_ms=off,
        max_abs_diff_x=float((xb - xp).abs().max()), max_abs_diff_ldj=float((lb - lp).abs().max()))), flush=True)


def main(argv):
    if argv[:1] == ['--worker']:
        return worker(argv[1])
    limit = os.environ.get('LIMIT', '300')
    for case in argv or list(CASES):
        if case not in CASES:
            raise SystemExit(f'unknown case {case!r}: one of {sorted(CASES)}')
        rc = subprocess.run(['timeout', '-k', '10', limit, sys.executable, os.path.abspath(__file__), '--worker', case]).returncode
        if rc != 0:
            raise SystemExit(f'{case}: the worker ended with status {rc}; nothing more is started')


if __name__ == '__main__':
    main(sys.argv[1:])
