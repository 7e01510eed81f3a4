#!/usr/bin/env python
"""Time one cfg2-sized MAF layer in float64: D = 3000 features, an 8-bin RQ spline (25 parameters per feature), two
hidden layers of 14 998 units, B = 8192 rows.  Four figures, each timed on its own:

  * the conditioner (MADE: three fp64-MFMA GEMMs, the weights re-packed on every call);
  * the spline kernel on the (B, 25 D) float64 parameter tensor (``tfep_spline_forward_f64``), with the bytes it has to
    stream and the rate that gives;
  * the layer forward (no grad);
  * forward plus backward of ``y.sum() + ldj.sum()`` with respect to every parameter (the generic training path).

    python tools/probe/f64_flow.py [--batch 8192] [--reps 3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

F64 = torch.float64


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
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--features', type=int, default=3000)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    D, B = args.features, args.batch
    torch.manual_seed(0)
    layer = MAF(generate_degrees(D), transformer=NeuralSplineTransformer(torch.full((D,), -5.0), torch.full((D,), 5.0), 8),
                initialize_identity=False).cuda().double()
    made, tr = layer._conditioner, layer._transformer
    hidden = [lin.out_features for lin in made._linears()[:-1]]
    x = torch.randn(B, D, device='cuda', dtype=F64)
    out = dict(features=D, batch=B, hidden=hidden, n_params_per_feature=tr.n_parameters_per_feature)
    with torch.no_grad():
        out['conditioner_ms'] = timed(lambda: made(x), args.reps)
        theta = made(x)
        out['spline_ms'] = timed(lambda: tr(x, theta), args.reps * 4)
        nbytes = theta.numel() * 8 + 2 * x.numel() * 8 + 4 * D * 8 + B * 8
        out['spline_bytes'] = nbytes
        out['spline_TBps'] = nbytes / out['spline_ms'] / 1e9
        del theta
        out['forward_ms'] = timed(lambda: layer(x), args.reps)

    def train():
        for p in layer.parameters():
            p.grad = None
        y, ldj = layer(x)
        (y.sum() + ldj.sum()).backward()
    out['forward_backward_ms'] = timed(train, args.reps)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
