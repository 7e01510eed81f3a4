#!/usr/bin/env python
"""Time the stand-alone quaternion product kernels at B = 131 072 rows, D = 1024 features (256 quaternions per row), float32
and float64: forward, inverse and the VJP of both directions (``tfep_quaternion_product[_backward][_f64]``), and in the same
process the symmetrized Moebius forward at d = 4 (``tfep_symmetrized_moebius``), the kernel with the same memory traffic.

Per kernel: the median of ``--reps`` HIP-event timings after ``--warmup`` calls, each window ``--inner`` launches long; the
rate on the bytes the kernel must move -- 3 B D sizeof(T) for a forward / inverse (x and p read, y written: 12 / 24 bytes
per feature; the (B,) log-det is left out), 5 B D sizeof(T) for a VJP (x, p, gy read, gx, gp written) -- and the ratio of
the forward to the symmetrized Moebius d = 4 forward of the same dtype.

    python tools/probe/quatprod_layer.py [--batch 131072] [--features 1024] [--reps 9]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402


def timed(fn, warmup, reps, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=131072)
    ap.add_argument('--features', type=int, default=1024)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=10)
    args = ap.parse_args()
    from tfep_amd import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.tfep.*)
    B, D = args.batch, args.features
    bwd = torch.ops.tfep.quaternion_product_backward
    if not torch.cuda.is_available():
        sys.exit('quatprod_layer.py needs a GPU')
    for dt in (torch.float32, torch.float64):
        size = torch.empty(0, dtype=dt).element_size()
        gen = torch.Generator(device='cuda').manual_seed(0)
        x = torch.randn(B, D, device='cuda', dtype=dt, generator=gen)
        p = 2 * torch.randn(B, D, device='cuda', dtype=dt, generator=gen)
        gy = torch.randn(B, D, device='cuda', dtype=dt, generator=gen)
        out = dict(dtype=str(dt).replace('torch.', ''), batch=B, features=D)
        runs = [('forward', 3, lambda: ops.quaternion_product(x, p)),
                ('inverse', 3, lambda: ops.quaternion_product(x, p, inverse=True)),
                ('vjp_forward', 5, lambda: bwd(x, p, gy, False)),
                ('vjp_inverse', 5, lambda: bwd(x, p, gy, True)),
                ('symmoebius_d4_forward', 3, lambda: ops.symmetrized_moebius(x, p, 4, 0.99))]
        with torch.no_grad():
            for name, n_arrays, fn in runs:
                med, lo, hi = timed(fn, args.warmup, args.reps, args.inner)
                nbytes = n_arrays * B * D * size
                out[name] = dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), GBps=round(nbytes / med / 1e6, 1))
        out['forward_over_symmoebius_d4'] = round(out['forward']['ms'] / out['symmoebius_d4_forward']['ms'], 3)
        print(json.dumps(out), flush=True)
        del x, p, gy
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
