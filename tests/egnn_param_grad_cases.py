"""Reference parameter gradients for the cases of ``egnn_cases.py``: the oracle ``oracle/egnn.py`` is differentiable in its
state dict, so ``autograd.grad(<v, velocity>, parameters)`` of its float64 run is the reference and of its float32 run the
float32 noise floor.  Shared by ``test_egnn_param_grads_host.py`` and ``test_gpu_egnn_param_grads.py``; computed once per
(case, dtype) and left unchanged."""
import functools

import numpy as np
import torch

import egnn_cases as ec
from oracle import egnn as oe

#: |g| relative L2 bound of a kernel gradient tensor: 1e-5 (what test_gpu_egnn_shapes.py holds v^T J to), or 4 x the float32
#: oracle's own distance from the float64 one where that is larger
REL = 1e-5
NOISE_MARGIN = 4.0
#: what the float32 oracle is expected to stay within (the condition the bound above rests on)
FLOAT32_ORACLE_REL = 2.5e-6


@functools.lru_cache(maxsize=None)
def parameter_names(name):
    return tuple(k for k, _ in ec.dynamics(name).named_parameters())


def unused_names(name):
    """The four tensors the velocity does not depend on: the last layer's ``update_h_mlp``."""
    last = f'graph_layer_{ec.case(name)["layers"] - 1}.update_h_mlp.'
    return tuple(k for k in parameter_names(name) if k.startswith(last))


def oracle_value(name, sd, g, dtype=torch.float64):
    """``<g, velocity>`` of the oracle for a state dict."""
    c = ec.case(name)
    vel = oe.egnn_dynamics(torch.tensor(c['t'], dtype=dtype), c['x'].to(dtype), sd, c['cfg'])
    return (vel * g.to(dtype)).sum()


def oracle_param_grads(name, dtype=torch.float64, g=None):
    """dict name -> float64 array (``None`` for an unused tensor) of the gradient of ``<g, velocity>``; ``g`` defaults to
    the case's ``v`` (cached)."""
    if g is None:
        return _cached(name, dtype)
    return _grads(name, dtype, g)


@functools.lru_cache(maxsize=None)
def _cached(name, dtype):
    out = _grads(name, dtype, ec.case(name)['v'])
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def _grads(name, dtype, g):
    c = ec.case(name)
    names = parameter_names(name)
    sd = {k: (p.to(dtype) if p.is_floating_point() else p) for k, p in c['sd64'].items()}
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(True)
    gs = torch.autograd.grad(oracle_value(name, sd, g, dtype), [sd[k] for k in names], allow_unused=True)
    return {k: (None if v is None else v.double().numpy()) for k, v in zip(names, gs)}


def bound(name, key):
    """``max(1e-5, 4 x float32 oracle's rel L2)`` for one tensor, and that float32 figure."""
    e32 = ec.rel_l2(oracle_param_grads(name, torch.float32)[key], oracle_param_grads(name)[key])
    return max(REL, NOISE_MARGIN * e32), e32


def as_numpy(grads):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in grads.items()}
