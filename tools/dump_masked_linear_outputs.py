#!/usr/bin/env python
"""Write what a single masked linear layer computes, forward and backward, through each of its public routes:

  op/...       ``torch.ops.tfep.masked_linear`` with ``torch.autograd.grad``
  func/...     ``MaskedLinearFunc.apply`` with ``torch.autograd.grad``
  module/...   ``MaskedLinear`` under ``masked_weight_norm``
  made/...     the forward of a 2-hidden-layer ``MADE`` (6 features, 40 hidden units)

in float32 and float64, on the shapes of ``SHAPES`` (the smallest that reach every GEMM tile variant), each with and without
mask, weight norm and bias.  Inputs come from fixed seeds on the CPU.

``tests/golden/masked_linear_before_unify.npz`` is this tool's output on an MI355X from the commit before the float32 and
float64 routes of the layer were folded into one (``ops.masked_linear_layer`` / ``ops.masked_linear_layer_backward``):
``tests/test_gpu_masked_linear_unified.py`` holds every later tree to those bits.  The tool uses nothing that commit lacks.
Run on an MI355X:

    python tools/dump_masked_linear_outputs.py OUT.npz

The file keeps each distinct array once (the routes agree bit for bit, and the gradients do not depend on the bias) and, of
an array of more than ``FULL_BELOW`` elements, only the SHA-256 of its bytes: ``load`` gives ``name -> array or digest``,
``matches`` compares an output with either.
"""
import hashlib
import itertools
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tfep_amd.nn.conditioners import MADE, generate_degrees  # noqa: E402
from tfep_amd.nn.masked import (MaskedLinear, MaskedLinearFunc, create_autoregressive_mask,  # noqa: E402
                                masked_weight_norm)

#: name -> (leading input dimensions, K, N): N <= 32 takes the wide-tile float32 kernel, 45 the 32-column tile, 300 (under an
#: autoregressive mask) two 256-row k-range tiles of the float64 GEMM with a K that is no multiple of 32
SHAPES = {'n24': ((5,), 37, 24), 'n45': ((5,), 37, 45), 'n300': ((7,), 70, 300), 'lead': ((2, 3), 37, 24)}
DTYPES = {'f32': torch.float32, 'f64': torch.float64}
FULL_BELOW = 256
GRADS = ('gi', 'gw', 'gb', 'gg')


def cases():
    """``(name, shape, dtype, mask?, weight norm?, bias?)`` of every single-layer case."""
    for (s, d), m, g, b in itertools.product(itertools.product(SHAPES, DTYPES), (0, 1), (0, 1), (0, 1)):
        yield f'{s}-{d}-m{m}g{g}b{b}', s, DTYPES[d], m, g, b


def inputs(shape, dtype, has_mask, has_g, has_bias):
    """The CPU tensors of a case: ``x, weight, bias, mask, weight_g, grad_output``.  The mask is autoregressive with a
    fully masked first row (no input has a smaller degree), so that entry of the gradient of ``weight_g`` is exactly 0."""
    lead, K, N = SHAPES[shape]
    gen = torch.Generator().manual_seed(1000 * K + N + len(lead))
    rnd = lambda *size: torch.randn(*size, generator=gen, dtype=torch.float64).to(dtype)  # noqa: E731
    x, weight, bias, g, grad = rnd(*lead, K), rnd(N, K), rnd(N), rnd(N, 1).abs() + 0.5, rnd(*lead, N)
    mask = create_autoregressive_mask(torch.arange(K) % 7, torch.arange(N) % 8, strictly_less=True, transpose=True,
                                      dtype=dtype)
    assert not mask[0].any() and mask[1:8].any(dim=1).all()
    return x, weight, (bias if has_bias else None), (mask if has_mask else None), (g if has_g else None), grad


def _cuda(tensors, requires_grad=True):
    return [None if t is None else t.cuda().requires_grad_(requires_grad and i in (0, 1, 2, 4))
            for i, t in enumerate(tensors[:5])] + [tensors[5].cuda()]


def _named(y, grads):
    out = {'y': y, **{k: g for k, g in zip(GRADS, grads) if g is not None}}
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def _through_autograd(fn, tensors):
    x, weight, bias, mask, g, grad = _cuda(tensors)
    y = fn(x, weight, bias, mask, g)
    wrt = [t for t in (x, weight, bias, g) if t is not None]
    got = iter(torch.autograd.grad(y, wrt, grad_outputs=grad))
    return _named(y, [None if t is None else next(got) for t in (x, weight, bias, g)])


def op_outputs(tensors):
    return _through_autograd(torch.ops.tfep.masked_linear, tensors)


def func_outputs(tensors):
    return _through_autograd(MaskedLinearFunc.apply, tensors)


def func_backward_alone(tensors, want):
    """``MaskedLinearFunc.backward`` as autograd calls it when only the input (``want='input'``) or only the weight and its
    norm (``'weight'``) require a gradient: the tuple it returns, one entry per argument of ``forward``."""
    x, weight, bias, mask, g, grad = _cuda(tensors, requires_grad=False)
    ctx = types.SimpleNamespace(needs_input_grad=(want == 'input', want == 'weight', False, False, want == 'weight'))
    ctx.save_for_backward = lambda *saved: setattr(ctx, 'saved_tensors', saved)
    MaskedLinearFunc.forward(ctx, x, weight, bias, mask, g)
    return MaskedLinearFunc.backward(ctx, grad)


def module_outputs(tensors):
    """``MaskedLinear`` with ``masked_weight_norm`` (its gradient hooks included), parameters set from the case."""
    x, weight, bias, mask, g, grad = tensors
    lin = MaskedLinear(weight.shape[1], weight.shape[0], bias=bias is not None, mask=mask).to(weight.dtype)
    masked_weight_norm(lin)
    with torch.no_grad():
        lin.weight_v.copy_(weight)
        lin.weight_g.copy_(g)
        if bias is not None:
            lin.bias.copy_(bias)
    lin = lin.cuda()
    x = x.cuda().requires_grad_(True)
    y = lin(x)
    wrt = [x, lin.weight_v] + ([lin.bias] if bias is not None else []) + [lin.weight_g]
    got = torch.autograd.grad(y, wrt, grad_outputs=grad.cuda())
    return _named(y, [got[0], got[1], got[2] if bias is not None else None, got[-1]])


def made_outputs(dtype):
    """``{route: output}`` of the MADE forward: the default route and, in float32, the exact-fp32 GEMMs asked for."""
    torch.manual_seed(7)
    degrees = generate_degrees(6)
    made = MADE(degrees, degrees.repeat(2), hidden_layers=[40, 40]).to(dtype).cuda()
    x = torch.randn(9, 6, generator=torch.Generator().manual_seed(8), dtype=torch.float64).to(dtype).cuda()
    with torch.no_grad():
        out = {'default': made(x)}
        if dtype == torch.float32:
            out['exact'] = made(x, split=False)
    return {k: v.cpu().numpy() for k, v in out.items()}


def route_outputs(route):
    """``name -> array`` of one of the routes ``op``, ``func``, ``module``, ``made``."""
    out = {}
    if route == 'made':
        for d, dtype in DTYPES.items():
            out.update({f'made/{d}/{k}': v for k, v in made_outputs(dtype).items()})
        return out
    for name, shape, dtype, m, g, b in cases():
        if route == 'module' and not g:
            continue
        tensors = inputs(shape, dtype, m, g, b)
        res = {'op': op_outputs, 'func': func_outputs, 'module': module_outputs}[route](tensors)
        out.update({f'{route}/{name}/{k}': v for k, v in res.items()})
    return out


ROUTES = ('op', 'func', 'module', 'made')


def digest(a):
    a = np.ascontiguousarray(a)
    return np.frombuffer(hashlib.sha256(str((a.dtype, a.shape)).encode() + a.tobytes()).digest(), dtype=np.uint8)


def matches(got, expected):
    """Whether the array ``got`` is what ``load`` returned for it: equal elementwise to a stored array, or of the stored
    digest (for an array stored by digest this is bitwise equality)."""
    if expected.dtype == np.uint8:
        return bool((digest(got) == expected).all())
    return got.dtype == expected.dtype and torch.equal(torch.from_numpy(got), torch.from_numpy(expected))


def save(path, out):
    """Each distinct array (or, when large, its digest) once as ``a<i>``, and the index of every name."""
    names, index, stored, seen = sorted(out), [], {}, {}
    for n in names:
        d = digest(out[n]).tobytes()
        if d not in seen:
            seen[d] = len(seen)
            stored[f'a{seen[d]}'] = out[n] if out[n].size <= FULL_BELOW else digest(out[n])
        index.append(seen[d])
    np.savez_compressed(path, names=np.array(names), index=np.array(index, dtype=np.int32), **stored)
    return len(seen)


def load(path):
    with np.load(path) as z:
        return {str(n): z[f'a{i}'] for n, i in zip(z['names'], z['index'])}


if __name__ == '__main__':
    out = {}
    for route in ROUTES:
        out.update(route_outputs(route))
    n = save(sys.argv[1], out)
    print(sys.argv[1], len(out), 'outputs,', n, 'distinct arrays')
