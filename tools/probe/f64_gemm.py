#!/usr/bin/env python
"""Time the fp64-MFMA masked GEMM (``tfep_masked_linear_gemm_f64``) at the cfg2 hidden-layer shapes.

First the register-only v_mfma_f64_16x16x4_f64 loop (``tfep_diag_mfma_f64_peak``: the matrix-pipe rate this kernel's
instruction mix can reach), then, per GEMM: ms, TFLOP/s on 2 * nnz(mask) * B (the work the masked product needs), that
rate as a fraction of the measured f64 MFMA rate, the whole module-level ``masked_linear`` call (weight prepare, mask
k-ranges, padding and GEMM), and the dense float64 ``torch.matmul`` of the same shape.  ``TFEP_HIP_LIB`` selects another
build of the library (e.g. ``python -m tfep_amd.build --probe /tmp/lib.so -DTFEP_F64_LDS_PAD=0`` for the unpadded LDS
layout).

    python tools/probe/f64_gemm.py [--batch 8192] [--reps 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from tfep_amd import ops  # noqa: E402
from tfep_amd.nn.masked import create_autoregressive_mask, masked_linear  # noqa: E402

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


def mfma_peak():
    blocks, iters = 256 * 8, 400
    ops.diag_mfma_f64_peak(blocks, 10, device='cuda')
    torch.cuda.synchronize()
    best = 0.0
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        flops = ops.diag_mfma_f64_peak(blocks, iters, device='cuda')
        e1.record()
        torch.cuda.synchronize()
        best = max(best, flops / e0.elapsed_time(e1) / 1e9)
    return best


def hidden_degrees(n_units, n_features):
    """Sorted degrees of a MADE hidden layer (units cycle through 0 .. D - 2, then sorted as the packing sorts them)."""
    return torch.sort(torch.arange(n_units) % (n_features - 1)).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    torch.manual_seed(0)
    peak = mfma_peak()
    print(f'register-only v_mfma_f64_16x16x4_f64 loop: {peak:.1f} TFLOP/s ({peak / 78.6 * 100:.1f} % of the 78.6 datasheet)',
          flush=True)
    tm, tn, tk = ops.tile_sizes()
    D, H, B = 3000, 14998, args.batch
    deg_in = torch.arange(D)
    deg_h = hidden_degrees(H, D)
    results = {'mfma_f64_tflops': peak}
    for name, d_in, d_out in (('3000->14998', deg_in, deg_h), ('14998->14998', deg_h, deg_h)):
        K, N = len(d_in), len(d_out)
        mask = create_autoregressive_mask(d_in, d_out, strictly_less=False, transpose=True, dtype=F64).cuda()
        nnz = int((mask != 0).sum())
        v = torch.randn(N, K, dtype=F64, device='cuda')
        kp, n_pad = ops.round_up(K, tk), ops.round_up(N, tk)
        wp = ops.masked_weight_prepare(v, None, mask, n_rows_padded=n_pad, k_padded=kp)
        kr = ops.mask_k_ranges(mask, tn, (n_pad + tn - 1) // tn, kp)
        xp = ops.pad_columns(torch.randn(B, K, dtype=F64, device='cuda'), kp, F64)
        bias = torch.randn(n_pad, dtype=F64, device='cuda')
        y = torch.empty(B, n_pad, dtype=F64, device='cuda')
        ms = timed(lambda: ops.masked_linear_f64(xp, wp, bias, n_pad, k_ranges=kr, act=1, out=y), args.reps)
        tf = 2.0 * nnz * B / ms / 1e9
        # the module path (torch.ops.tfep.masked_linear: weight prepare + k-ranges + padding + GEMM on every call)
        xm = torch.randn(B, K, dtype=F64, device='cuda')
        bm = torch.randn(N, dtype=F64, device='cuda')
        ms_mod = timed(lambda: masked_linear(xm, v, bm, mask), args.reps)
        del xm
        w_dense = v.T.contiguous()
        x_dense = xp[:, :K]
        ms_mm = timed(lambda: torch.matmul(x_dense, w_dense), args.reps)
        tf_mm = 2.0 * K * N * B / ms_mm / 1e9
        del mask, v, wp, w_dense
        row = dict(shape=f'{B} x {name}', nnz=nnz, density=nnz / (K * N), ms=ms, tflops_masked=tf, frac_of_mfma=tf / peak,
                   module_masked_linear_ms=ms_mod, torch_matmul_ms=ms_mm, torch_matmul_tflops_dense=tf_mm)
        results[name] = row
        print(f'{B} x {name}: masked fp64 GEMM {ms:.2f} ms, {tf:.1f} TFLOP/s on 2 nnz B ({tf / peak * 100:.1f} % of the '
              f'measured f64 MFMA rate; mask density {nnz / (K * N):.3f}) | masked_linear op {ms_mod:.2f} ms | '
              f'torch.matmul float64 dense {ms_mm:.2f} ms ({tf_mm:.1f} TFLOP/s)', flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(results))


if __name__ == '__main__':
    main()
