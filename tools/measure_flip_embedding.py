#!/usr/bin/env python
"""Timings of FlipInvariantEmbedding for README / DESIGN section 4f: the kernel route against ``torch_forward`` in one
process, forward and forward + backward, float32 and float64.  One shape: B = 131 072 rows of 64 quaternions plus 64 plain
features, hidden width 32, embedding dimension 8.  One JSON line per measurement; HIP events, warm-up, the median of the
repetitions.  ``tb_per_s`` counts the bytes the kernel route has to move: x and out once for the forward; x, the cotangent
of out and the cotangent of x once more for the backward.  Run on an MI355X:

    python tools/measure_flip_embedding.py
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfep_amd.nn.embeddings import FlipInvariantEmbedding  # noqa: E402

dev = torch.device('cuda')
B, N_QUAT, N_PLAIN, H, E = 131072, 64, 64, 32, 8
D = 4 * N_QUAT + N_PLAIN


def median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
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


for dtype in (torch.float32, torch.float64):
    torch.manual_seed(0)
    # the quaternions interleaved with the plain features: 4 embedded columns, 1 plain column, ...
    embedded = [5 * q + c for q in range(N_QUAT) for c in range(4)]
    emb = FlipInvariantEmbedding(D, E, embedded_indices=embedded, hidden_layer_width=H).to(dtype).to(dev)
    x = torch.randn(B, D, device=dev, dtype=dtype, generator=torch.Generator(device=dev).manual_seed(1))
    n_out = N_PLAIN + N_QUAT * E
    size = x.element_size()
    fwd_bytes = B * (D + n_out) * size
    bwd_bytes = B * (D + n_out + D) * size
    gout = torch.randn(B, n_out, device=dev, dtype=dtype, generator=torch.Generator(device=dev).manual_seed(2))

    def forward_backward(fn):
        xg = x.detach().requires_grad_(True)
        emb.zero_grad(set_to_none=True)
        fn(xg).backward(gout)

    with torch.no_grad():
        out_k = emb(x)
        assert emb.last_route == 'kernel'
        out_t = emb.torch_forward(x)
        diff = float((out_k - out_t).abs().max())
        t_k, all_k = median_ms(lambda: emb(x), 20)
        t_t, all_t = median_ms(lambda: emb.torch_forward(x), 10)
    report(what='forward', dtype=str(dtype), batch=B, quaternions=N_QUAT, plain=N_PLAIN, hidden=H, emb_dim=E,
           kernel_ms=round(t_k, 4), torch_ms=round(t_t, 4), ratio=round(t_t / t_k, 2),
           kernel_tb_per_s=round(fwd_bytes / t_k / 1e9, 3), max_abs_diff=diff, kernel_all_ms=all_k, torch_all_ms=all_t)
    tb_k, allb_k = median_ms(lambda: forward_backward(emb), 10)
    tb_t, allb_t = median_ms(lambda: forward_backward(emb.torch_forward), 5)
    report(what='forward + backward', dtype=str(dtype), batch=B, kernel_ms=round(tb_k, 4), torch_ms=round(tb_t, 4),
           ratio=round(tb_t / tb_k, 2), kernel_tb_per_s=round((fwd_bytes + bwd_bytes) / tb_k / 1e9, 3),
           kernel_all_ms=allb_k, torch_all_ms=allb_t)
    del emb, x, gout, out_k, out_t
    torch.cuda.empty_cache()
