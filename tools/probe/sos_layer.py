#!/usr/bin/env python
"""Time one cfg2-sized MAF layer with the SOS polynomial transformer: D = 3000 features, K = 2 polynomials (5 parameters
per feature), the cfg2 hidden width (two hidden layers of 14 998 units, what the default rule gives the 25 parameters
per feature of cfg2's 8-bin spline), B = 8192 and 65 536 rows.  Per batch size:

  * the layer forward (no grad) on the fused split-f16 and exact-fp32 paths and on the generic path (``fused = False``: three
    GEMMs, the (B, 5 D) parameters through HBM, the element-wise SOS kernel) with split-f16 and with exact-fp32 GEMMs;
  * the element-wise kernel alone (``tfep_sos_forward`` on a (B, 5 D) parameter tensor), with the bytes it must move and
    the rate that gives;
  * an affine layer of the same shape (2 parameters per feature) on the fused split-f16 path, for comparison.

Times are HIP-event means over ``--reps`` calls after one warm-up call.  Kernel times: run the same script under
``rocprofv3 --kernel-trace --stats -- python tools/probe/sos_layer.py``.

    python tools/probe/sos_layer.py [--batches 8192 65536] [--reps 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[8192, 65536])
    ap.add_argument('--features', type=int, default=3000)
    ap.add_argument('--polynomials', type=int, default=2)
    ap.add_argument('--hidden', type=int, default=14998)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    from tfep_amd import ops
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import AffineTransformer, SOSPolynomialTransformer
    D, K = args.features, args.polynomials
    P = 2 * K + 1
    torch.manual_seed(0)
    hl = [args.hidden] * 2
    layer = MAF(generate_degrees(D), transformer=SOSPolynomialTransformer(K), hidden_layers=hl, initialize_identity=False).cuda()
    affine = MAF(generate_degrees(D), transformer=AffineTransformer(), hidden_layers=hl, initialize_identity=False).cuda()
    hidden = [lin.out_features for lin in layer._conditioner._linears()[:-1]]
    for B in args.batches:
        x = torch.randn(B, D, device='cuda')
        out = dict(features=D, polynomials=K, batch=B, hidden=hidden)
        with torch.no_grad():
            for name, fused, split in (('fused_split', True, True), ('fused_exact', True, False), ('generic_split', False, True),
                                       ('generic', False, False)):
                layer.fused, layer.split_gemm = fused, split
                out[f'{name}_ms'] = timed(lambda: layer(x), args.reps)
            layer.fused, layer.split_gemm = None, None
            out['default_ms'] = timed(lambda: layer(x), args.reps)
            affine.fused, affine.split_gemm = True, True
            out['affine_fused_split_ms'] = timed(lambda: affine(x), args.reps)
            affine.fused, affine.split_gemm = False, False
            out['affine_generic_ms'] = timed(lambda: affine(x), args.reps)
            theta = torch.randn(B, P * D, device='cuda') * 0.5
            out['sos_kernel_ms'] = timed(lambda: ops.sos(x, theta, K), args.reps * 4)
            nbytes = (P + 2) * B * D * 4 + B * 4             # parameters + x read, y written, log-det written
            out['sos_kernel_bytes'] = nbytes
            out['sos_kernel_TBps'] = nbytes / out['sos_kernel_ms'] / 1e9
            del theta
        print(json.dumps(out), flush=True)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
