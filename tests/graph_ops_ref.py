"""A plain restatement of the radial expansions and the segment sum (csrc/graph_ops.hip), for the tests: torch expressions
on CPU tensors, in float64 or float32, as the reference writes them (``tfep/nn/embeddings/radial.py:110-130, 161-176``,
``tfep/nn/graph.py:304-316``); gradients by ``torch.autograd.grad``; the cases the GPU tests run and the comparisons they share.

    gauss      f[i, k] = exp(-exp(lg_k) (r_i - mu_k)^2)
    bp         f[i, k] times s(r_i) = 0.5 cos(pi r_i / r_c) + 0.5
    bp_zero    the same with s = 0 for r > r_c
    segment    out[s] = sum of the rows with ids == s (``index_add_``); ids outside [0, n_segments) are skipped

``tests/test_graph_ops_host.py`` holds these expressions to derivatives written out by hand.
"""
import functools
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
KINDS = ('gauss', 'bp_zero', 'bp')
# below one wave; ragged against the 64 rows of a wave's group and the 4 waves of a workgroup; 1094 groups on 274 workgroups
NS = (1, 63, 257, 70001)
# one lane; a ragged pass; one full pass of the 64 lanes
KS = (1, 5, 64)
R_CUTOFF = 1.25                      # exact in float32: the float32 kernels and the float64 reference cut at the same r


def switching(kind):
    """``(switching, force_zero)`` of a kind."""
    return kind != 'gauss', kind == 'bp_zero'


def expansion(r, means, log_gammas, kind, r_cutoff=R_CUTOFF):
    """``(*r.shape, K)``."""
    disp = (r.unsqueeze(-1) - means).pow(2)
    encoding = torch.exp(-log_gammas.exp() * disp)
    if kind == 'gauss':
        return encoding
    s = 0.5 * torch.cos(math.pi / r_cutoff * r) + 0.5
    if kind == 'bp_zero':
        s = torch.where(r > r_cutoff, torch.zeros_like(s), s)
    return encoding * s.unsqueeze(-1)


def segment_sum(data, ids, n_segments):
    keep = (ids >= 0) & (ids < n_segments)
    out = data.new_zeros(n_segments, data.shape[1])
    return out.index_add_(0, ids[keep], data[keep])


def segment_gather(grad_out, ids):
    keep = (ids >= 0) & (ids < grad_out.shape[0])
    out = grad_out.new_zeros(len(ids), grad_out.shape[1])
    out[keep] = grad_out[ids[keep]]
    return out


@functools.lru_cache(maxsize=None)
def case(n, K, dtype):
    """Inputs of one size as float64 tensors that hold values of ``dtype``: distances on [0, 1.5 r_c] -- the last four are r_c
    itself, its two neighbours in ``dtype`` and 0 (none at n = 1) --, means over [0, r_c], gammas in [1, 30], a normal
    cotangent."""
    gen = torch.Generator().manual_seed(1000 * n + K)
    r = 1.5 * R_CUTOFF * torch.rand(n, generator=gen, dtype=F64)
    rc = torch.tensor(R_CUTOFF, dtype=dtype)
    special = torch.stack([rc, torch.nextafter(rc, rc * 2), torch.nextafter(rc, rc * 0), rc * 0]).to(F64)
    m = min(n - 1, 4)               # (row 0 stays a generic distance: with r_c alone every value of a switched kind is 0)
    r[n - m:] = special[:m]
    means = torch.linspace(0.0, R_CUTOFF, K, dtype=F64) if K > 1 else torch.tensor([0.4 * R_CUTOFF], dtype=F64)
    means = means + 0.02 * torch.randn(K, generator=gen, dtype=F64)
    log_gammas = torch.log(1.0 + 29.0 * torch.rand(K, generator=gen, dtype=F64))
    g = torch.randn(n, K, generator=gen, dtype=F64)
    return tuple(t.to(dtype).to(F64) for t in (r, means, log_gammas, g))


@functools.lru_cache(maxsize=None)
def reference(kind, n, K, dtype, run_dtype=F64):
    """``dict(f, g_r, g_means, g_log_gammas)`` as float64 numpy arrays: the expressions above run in ``run_dtype`` on the
    inputs of ``case(n, K, dtype)``."""
    # (clones: the cached inputs are shared and stay as they are)
    r, means, lg, g = (t.clone().to(run_dtype).requires_grad_(i < 3) for i, t in enumerate(case(n, K, dtype)))
    f = expansion(r, means, lg, kind)
    grads = torch.autograd.grad(f, (r, means, lg), g)
    return {k: v.detach().to(F64).numpy() for k, v in zip(('f', 'g_r', 'g_means', 'g_log_gammas'), (f, *grads))}


def rel_l2(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))
