"""Layers and inputs for tests/test_gpu_float64_inverse_backward.py: the kinds of float64 MAF layers that
tests/test_gpu_float64_inverse.py runs the blocked inverse on (same sizes, but 75 features instead of 300 for the RQ-8
layers: the per-degree reference costs one kept conditioner pass per degree; the fixed-feature layer also has a periodic
embedding, so a feature of degree -1 enters the conditioner as a (cos, sin) pair), plus one layer with a hidden width that
is no multiple of 16 and several hidden units per degree."""
import contextlib

import torch

F64 = torch.float64

CASES = ['rq8_asc', 'rq8_desc', 'circ', 'affine_h1', 'affine_h3', 'mixed', 'fixed', 'ragged', 'short', 'wide']


@contextlib.contextmanager
def default_float64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _spline(n, lo, hi, bins, **kw):
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    return NeuralSplineTransformer(torch.full((n,), lo), torch.full((n,), hi), bins, **kw)


def _noise_(t, gen, scale):
    t.copy_(scale * torch.randn(t.shape, generator=gen, dtype=t.dtype))


def make_layer(case, seed=0):
    """``(layer, D, domain)``: one float64 MAF layer on the GPU with seeded, non-identity weights."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.embeddings import PeriodicEmbedding
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import AffineTransformer, MixedTransformer
    kw, dom = {}, (-2.0, 2.0)
    with default_float64():
        if case in ('rq8_asc', 'rq8_desc'):     # 25 parameter rows per feature: the block of 16 degrees is halved to fit the LDS
            D = 75                              # (ten blocks of 8 degrees, the last one ragged)
            deg = generate_degrees(D, 'ascending' if case == 'rq8_asc' else 'descending')
            tr = _spline(D, -2.0, 2.0, 8)
        elif case == 'circ':                    # every feature periodic: (cos, sin) pairs, circular splines
            D, dom = 96, (0.0, 1.0)
            deg = generate_degrees(D)
            tr = _spline(D, 0.0, 1.0, 5, circular=True)
            kw['embedding'] = PeriodicEmbedding(D, [0.0, 1.0], periodic_indices=list(range(D)))
        elif case in ('affine_h1', 'affine_h3'):
            D = 64
            deg = generate_degrees(D, 'descending')
            tr = AffineTransformer()
            kw['hidden_layers'] = 1 if case == 'affine_h1' else 3
        elif case == 'mixed':
            D = 48
            deg = generate_degrees(D)
            idx_s, idx_a = list(range(0, D, 2)), list(range(1, D, 2))
            tr = MixedTransformer([_spline(len(idx_s), -2.0, 2.0, 6, learn_lower_bound=True), AffineTransformer()],
                                  [idx_s, idx_a])
        elif case == 'fixed':                   # features of degree -1 (one of them periodic), two features per degree
            D = 50
            deg = generate_degrees(D, 'descending', conditioning_indices=[0, 7, 31], repeats=2)
            tr = _spline(D - 3, -2.0, 2.0, 4, identity_boundary_slopes=True)
            kw['weight_norm'] = False
            kw['embedding'] = PeriodicEmbedding(D, [-2.0, 2.0], periodic_indices=[7, 11])
        elif case == 'ragged':                  # 37 degrees: not a multiple of the block size
            D = 37
            deg = generate_degrees(D)
            tr = _spline(D, -2.0, 2.0, 9)
        elif case == 'short':                   # fewer degrees than one block
            D = 5
            deg = generate_degrees(D)
            tr = _spline(D, -2.0, 2.0, 8)
        elif case == 'wide':                    # 45 and 23 hidden units on 9 degrees: widths that are no multiples of 16
            D = 10
            deg = generate_degrees(D)
            tr = _spline(D, -2.0, 2.0, 8)
            kw['hidden_layers'] = [45, 23]
        else:
            raise KeyError(case)
        layer = MAF(deg, transformer=tr, **kw)
    gen = torch.Generator().manual_seed(1000 + seed)
    lins = layer._conditioner._linears()
    with torch.no_grad():
        for lin in lins:
            _noise_(lin.bias, gen, 0.1)
        last = lins[-1]
        if last.has_weight_norm:
            _noise_(last.weight_g, gen, 0.1)
        else:
            _noise_(last._parameters['weight'], gen, 0.02)
    layer = layer.double().cuda()
    assert layer.is_float64
    return layer, D, dom


def inputs(layer, D, dom, B, seed):
    """``{'in-domain': y, 'tails': y}``: images of points inside the splines' domain, and points that reach the tails."""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    lo, hi = dom
    x = lo + (hi - lo) * (0.02 + 0.96 * torch.rand(B, D, device='cuda', dtype=F64, generator=gen))
    with torch.no_grad():
        y_in = layer(x)[0]
    y_tail = 1.5 * torch.randn(B, D, device='cuda', dtype=F64, generator=gen)
    return {'in-domain': y_in, 'tails': y_tail}


LOSSES = {
    'gx': lambda x, ldj: x.square().sum(),
    'gldj': lambda x, ldj: ldj.sum(),
    'both': lambda x, ldj: x.square().sum() + ldj.sum(),
}


def gradients(layer, y0, loss, flag, block=None):
    """``[y.grad, parameter gradients ...]`` of ``loss(layer.inverse(y0))`` with ``blocked_inverse_backward = flag``."""
    layer.blocked_inverse_backward = flag
    if block is not None:
        layer.inverse_block_f64 = block
    y = y0.clone().requires_grad_(True)
    params = list(layer.parameters())
    x, ldj = layer.inverse(y)
    grads = torch.autograd.grad(LOSSES[loss](x, ldj), [y] + params, allow_unused=True)
    return [g if g is not None else torch.zeros_like(p) for g, p in zip(grads, [y] + params)], (x.detach(), ldj.detach())
