"""Time and peak memory of ``EGNNDynamics.vjp_parameters`` in one process on one GPU:

  1. against ``vjp`` at BASELINE cfg5's shape (B = 16 384, 256 atoms, F = G = 64, 4 layers);
  2. against ``torch_forward`` + ``autograd.grad`` at the largest batch (a power of two) whose ``dense_route_bytes`` fits.

Run it under a time limit of its own (``timeout -k 10 600 python tools/measure_egnn_param_grads.py``); it exits at the
first failure and prints one JSON line per measurement.
"""
import argparse
import json
import sys
import time

import torch

from tfep_amd.nn.dynamics import EGNNDynamics


def _time(fn, repeats):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / repeats * 1e3, torch.cuda.max_memory_allocated() / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16384)
    ap.add_argument('--atoms', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('needs a GPU')
    n = args.atoms
    torch.manual_seed(0)
    dyn = EGNNDynamics(node_types=[i % 3 for i in range(n)], r_cutoff=1.0, initialize_identity=False).cuda()
    gen = torch.Generator().manual_seed(1)
    side = round(n ** (1 / 3) + 0.5)
    grid = torch.stack(torch.meshgrid(*[torch.arange(side, dtype=torch.float32)] * 3, indexing='ij'), -1).reshape(-1, 3)[:n]

    def batch(B):
        x = (grid[None] * 0.3 + 0.05 * torch.randn(B, n, 3, generator=gen)).reshape(B, 3 * n).cuda()
        return x, torch.randn(B, 3 * n, generator=gen).cuda()

    x, g = batch(args.batch)
    with torch.no_grad():
        ms_vjp, mib_vjp = _time(lambda: dyn.vjp(0.4, x, g), args.repeats)
        ms_pg, mib_pg = _time(lambda: dyn.vjp_parameters(0.4, x, g), args.repeats)
    print(json.dumps(dict(what='vjp_parameters against vjp', batch=args.batch, atoms=n, vjp_ms=ms_vjp, vjp_parameters_ms=ms_pg,
                          ratio=ms_pg / ms_vjp, vjp_peak_mib=mib_vjp, vjp_parameters_peak_mib=mib_pg)), flush=True)
    del x, g
    torch.cuda.empty_cache()

    free = torch.cuda.mem_get_info()[0]
    B = 1
    while dyn.dense_route_bytes(2 * B) * 2 < free:       # (autograd keeps about twice the lower bound)
        B *= 2
    x, g = batch(B)
    params = [p for k, p in dyn.named_parameters() if f'graph_layer_{dyn._n_layers - 1}.update_h_mlp' not in k]

    def dense():
        return torch.autograd.grad(dyn.torch_forward(0.4, x), params, g)

    ms_dense, mib_dense = _time(dense, args.repeats)
    with torch.no_grad():
        ms_pg, mib_pg = _time(lambda: dyn.vjp_parameters(0.4, x, g), args.repeats)
    print(json.dumps(dict(what='vjp_parameters against torch_forward + autograd.grad', batch=B, atoms=n, dense_ms=ms_dense,
                          vjp_parameters_ms=ms_pg, ratio=ms_pg / ms_dense, dense_peak_mib=mib_dense,
                          vjp_parameters_peak_mib=mib_pg)), flush=True)


if __name__ == '__main__':
    main()
