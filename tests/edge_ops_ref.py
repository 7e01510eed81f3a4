"""A plain restatement of the edge geometry and the pruning (csrc/edge_ops.hip), for the tests: torch expressions on CPU
tensors, in float64 or float32, the gradient written out by hand from the formulas of the kernel's header, and the cases the
GPU tests run.

    geometry   v_e = x[head_e] - x[tail_e], head = edges[1] and tail = edges[0] (swapped with ``inverse``); r_e = |v_e|;
               the directions are v_e, or u_e = v_e / r_e with ``normalize``
    its VJP    g_v = g_d + g_r u, or with ``normalize`` (g_d - u (u . g_d)) / r + g_r u;  g_x[head] += g_v, g_x[tail] -= g_v
    pruning    the edges with r_e <= r_cutoff, in their order (a NaN distance is dropped)

``tests/test_edge_ops_host.py`` holds the hand-written gradient to torch's autograd of the plain expressions.
"""
import functools

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
FLAGS = ((False, False), (True, False), (False, True), (True, True))            # (normalize, inverse)
# The geometry kernels run 256 lanes per workgroup on at most 2048 workgroups, one edge (forward) or one node (backward) per
# lane: 2048 * 256 = 524288 lanes in one grid pass, so 524289 edges take a second pass.
GRID_PASS = 2048 * 256
ES = (1, 63, 64, 65, 257, GRID_PASS + 1)
NS = (2, 65)
MIN_LENGTH = 0.1
PRUNE_TILE = 256                       # edges per workgroup of the count and compaction kernels
PRUNE_ES = (0, 1, PRUNE_TILE - 1, PRUNE_TILE, PRUNE_TILE + 1, 3 * PRUNE_TILE + 1)


def ends(edges, inverse):
    """``(head, tail)``: the directions point from tail to head."""
    return (edges[0], edges[1]) if inverse else (edges[1], edges[0])


def geometry(x, edges, normalize=False, inverse=False):
    """``(distances (E,), directions (E, 3))`` in the dtype of ``x``."""
    head, tail = ends(edges, inverse)
    v = x[head] - x[tail]
    r = v.pow(2).sum(-1).sqrt()
    return r, (v / r.unsqueeze(-1) if normalize else v)


def geometry_vjp(x, edges, g_r, g_d, normalize=False, inverse=False):
    """The cotangent of ``x`` for the cotangents ``g_r (E,)`` and ``g_d (E, 3)`` (``None``: zero), by hand."""
    head, tail = ends(edges, inverse)
    v = x[head] - x[tail]
    r = v.pow(2).sum(-1, keepdim=True).sqrt()
    u = v / r
    g_r = torch.zeros_like(r) if g_r is None else g_r.unsqueeze(-1)
    g_d = torch.zeros_like(v) if g_d is None else g_d
    if normalize:
        g_v = (g_d - u * (u * g_d).sum(-1, keepdim=True)) / r + g_r * u
    else:
        g_v = g_d + g_r * u
    return torch.zeros_like(x).index_add_(0, head, g_v).index_add_(0, tail, -g_v)


def keep_index(distances, r_cutoff):
    return torch.nonzero(distances <= r_cutoff).reshape(-1)


def prune(r_cutoff, edges, distances, *args):
    keep = keep_index(distances, r_cutoff)
    return (edges[:, keep], distances[keep], *[a[keep] for a in args])


@functools.lru_cache(maxsize=None)
def positions(n_nodes, dtype, seed=0):
    """``randn`` positions as a float64 tensor that holds values of ``dtype``, drawn again until every pair of nodes is more
    than ``MIN_LENGTH`` apart: every edge between two different nodes is longer than that by construction."""
    gen = torch.Generator().manual_seed(100 * n_nodes + seed)
    while True:
        x = torch.randn(n_nodes, 3, generator=gen, dtype=F64).to(dtype).to(F64)
        pairs = torch.cdist(x, x) + 10.0 * torch.eye(n_nodes, dtype=F64)
        if float(pairs.min()) > MIN_LENGTH:
            return x


@functools.lru_cache(maxsize=None)
def case(n_edges, n_nodes, dtype):
    """``(x, edges, g_r, g_d)`` of one size, float64 tensors that hold values of ``dtype``: random edges between different
    nodes, the last a repeat of the first; with 65 nodes, nodes 3 and 64 have no edge."""
    gen = torch.Generator().manual_seed(1000 * n_edges + n_nodes)
    x = positions(n_nodes, dtype)
    allowed = torch.tensor([n for n in range(n_nodes) if n_nodes == 2 or n not in (3, 64)])
    src = torch.randint(len(allowed), (n_edges,), generator=gen)
    dst = (src + 1 + torch.randint(len(allowed) - 1, (n_edges,), generator=gen)) % len(allowed)
    edges = torch.stack([allowed[src], allowed[dst]])
    edges[:, -1] = edges[:, 0]
    g_r = torch.randn(n_edges, generator=gen, dtype=F64).to(dtype).to(F64)
    g_d = torch.randn(n_edges, 3, generator=gen, dtype=F64).to(dtype).to(F64)
    return x, edges, g_r, g_d


@functools.lru_cache(maxsize=16)          # (the largest case holds 17 MB per entry)
def reference(n_edges, n_nodes, dtype, normalize, inverse, run_dtype=F64):
    """``dict(distances, directions, gx)`` as float64 numpy arrays: the expressions above run in ``run_dtype`` on the inputs
    of ``case``; ``gx`` by hand in float64, by torch's autograd (the torch route) in float32."""
    x, edges, g_r, g_d = case(n_edges, n_nodes, dtype)
    x, g_r, g_d = (t.clone().to(run_dtype) for t in (x, g_r, g_d))            # (clones: the cached inputs stay as they are)
    if run_dtype == F64:
        r, d = geometry(x, edges, normalize, inverse)
        gx = geometry_vjp(x, edges, g_r, g_d, normalize, inverse)
    else:
        x.requires_grad_(True)
        r, d = geometry(x, edges, normalize, inverse)
        gx, = torch.autograd.grad((r, d), x, (g_r, g_d))
    return {k: v.detach().to(F64).numpy() for k, v in zip(('distances', 'directions', 'gx'), (r, d, gx))}


def rel_l2(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))
