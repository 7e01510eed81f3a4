"""A plain torch-CPU placement of atoms from a Z-matrix, for the tests of csrc/zmatrix.hip: a loop over the rows in
topological order, vectorised over the batch, in the dtype of its inputs, gradients by ``torch.autograd.grad``.  Written
from the formulas of the header comment of csrc/zmatrix.h; it shares no code with ``tfep_amd``.

    b1 = unit(x_k - x_j)
    w  = unit((x_l - x_k) - ((x_l - x_k) . b1) b1)
    x_i = x_j + d (cos a  b1 + sin a (cos t  w - sin t (b1 x w)))
    log_det_J = sum over the placed atoms of 2 log d + log|sin a|

And the three cases of the tests, from fixed seeds (B = 6 rows, which is no multiple of the rows of a workgroup):
    wide   3 fixed atoms and 70 atoms that all reference them: one level that takes two passes of the 64 lanes, and a
           70-item incidence list on each fixed atom
    chain  3 fixed atoms and 40 atoms, each placed from the previous three: 40 levels of one atom
    tree   5 fixed atoms and 60 placed ones, each bonded to a random atom placed before it (7 levels); the atom labels
           are a random permutation (the fixed atoms are no prefix of the range) and the rows are shuffled
Values: d in [0.9, 1.6], a in [0.6, 2.5], t uniform in (-pi, pi).
"""
import functools
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
B = 6
# seeds for which the reference atoms of every row are far from collinear: ``min_reference_sine`` >= MIN_SINE, asserted
# in tests/test_zmatrix_host.py (a condition on the cases, not a tolerance)
SEEDS = {'wide': 1, 'chain': 1, 'tree': 15}
MIN_SINE = 0.3
CASES = tuple(SEEDS)


def _dot(a, b):
    return (a * b).sum(-1, keepdim=True)


def _unit(a):
    return a / _dot(a, a).sqrt()


def topological_order(z_matrix, fixed_atoms):
    """The rows of ``z_matrix`` in an order in which every reference is in place: repeatedly the first row that can be
    placed."""
    placed = set(int(i) for i in fixed_atoms)
    left = list(range(len(z_matrix)))
    order = []
    while left:
        row = next(r for r in left if all(int(v) in placed for v in z_matrix[r][1:]))
        order.append(row)
        left.remove(row)
        placed.add(int(z_matrix[row][0]))
    return order


def place(d, a, t, x_fixed, z_matrix, fixed_atoms):
    """``(x, log_det_J)``: positions (B, n_atoms, 3) and the log-det (B,) from ``d, a, t`` (B, n_ic; column c for row c of
    ``z_matrix``) and ``x_fixed`` (B, n_fixed, 3)."""
    z = [[int(v) for v in row] for row in z_matrix]
    pos = {int(i): x_fixed[:, f] for f, i in enumerate(fixed_atoms)}
    for r in topological_order(z, fixed_atoms):
        i, j, k, l = z[r]
        b1 = _unit(pos[k] - pos[j])
        r_ = pos[l] - pos[k]
        w = _unit(r_ - _dot(r_, b1) * b1)
        n = torch.linalg.cross(b1, w, dim=-1)
        dr, ar, tr = d[:, r:r + 1], a[:, r:r + 1], t[:, r:r + 1]
        pos[i] = pos[j] + dr * (torch.cos(ar) * b1 + torch.sin(ar) * (torch.cos(tr) * w - torch.sin(tr) * n))
    x = torch.stack([pos[i] for i in range(len(pos))], dim=1)
    return x, (2.0 * torch.log(d) + torch.log(torch.abs(torch.sin(a)))).sum(1)


def min_reference_sine(x, z_matrix):
    """The smallest sine of the angle (x_j, x_k, x_l) at x_k over the rows of ``z_matrix`` and the batch: what the
    placement and its derivative divide by."""
    x = torch.as_tensor(x).detach().to(F64)
    z = torch.as_tensor(z_matrix).long()
    u, v = x[:, z[:, 1]] - x[:, z[:, 2]], x[:, z[:, 3]] - x[:, z[:, 2]]
    cos = _dot(u, v) / (_dot(u, u).sqrt() * _dot(v, v).sqrt())
    return float((1.0 - cos * cos).clamp_min(0.0).sqrt().min())


# ----------------------------------------------------------------------------- the cases

def _z_matrix(name, g):
    """``(z_matrix (n_ic, 4), fixed_atoms (n_fixed,))`` int64."""
    if name == 'wide':
        rows = [[3 + m] + torch.randperm(3, generator=g).tolist() for m in range(70)]
        return torch.tensor(rows), torch.arange(3)
    if name == 'chain':
        return torch.tensor([[i, i - 1, i - 2, i - 3] for i in range(3, 43)]), torch.arange(3)
    if name == 'tree':
        # atom m (before relabelling) is bonded to a random earlier atom j and takes j's own first two references as k
        # and l, so the angle (j, k, l) is the angle j was placed with; a fixed j takes the next two fixed atoms
        label = torch.randperm(65, generator=g)
        refs = {f: [(f + 1) % 5, (f + 2) % 5] for f in range(5)}
        rows = []
        for m in range(5, 65):
            j = int(torch.randint(m, (1,), generator=g))
            refs[m] = [j, refs[j][0]]
            rows.append(label[[m, j] + refs[j]].tolist())
        rows = [rows[r] for r in torch.randperm(60, generator=g).tolist()]
        return torch.tensor(rows), label[:5].clone()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name, seed=None):
    """The float64 inputs of a case: a dict with ``z_matrix``, ``fixed_atoms``, ``d``, ``a``, ``t`` (B, n_ic), ``x_fixed``
    (B, n_fixed, 3) and the cotangents ``cx`` (B, n_atoms, 3) and ``cl`` (B,) of the loss the gradient tests use.  The
    tensors are shared between the tests: do not write to them."""
    seed = SEEDS[name] if seed is None else seed
    g = torch.Generator().manual_seed(1000 * (1 + CASES.index(name)) + seed)
    z, fixed = _z_matrix(name, g)
    n_ic, n_fixed = len(z), len(fixed)
    uniform = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, dtype=F64, generator=g)
    return {
        'seed': seed, 'z_matrix': z, 'fixed_atoms': fixed,
        'd': uniform(0.9, 1.6, B, n_ic), 'a': uniform(0.6, 2.5, B, n_ic),
        't': -uniform(-math.pi, math.pi, B, n_ic),                  # (rand is in [0, 1): the sign flip leaves out -pi)
        'x_fixed': 1.5 * torch.randn(B, n_fixed, 3, dtype=F64, generator=g),
        'cx': torch.randn(B, n_ic + n_fixed, 3, dtype=F64, generator=g), 'cl': torch.randn(B, dtype=F64, generator=g),
    }


INPUTS = ('d', 'a', 't', 'x_fixed')


def inputs(name, rounded):
    """The four float64 inputs of a case; ``rounded``: rounded to float32 and widened again (what a float32 run sees)."""
    c = case(name)
    return [c[k].to(F32).to(F64) if rounded else c[k] for k in INPUTS]


@functools.lru_cache(maxsize=None)
def reference(name, rounded=False, dtype=F64):
    """``{'x', 'log_det_J', 'g_d', 'g_a', 'g_t', 'g_x_fixed'}`` of a case as float64 numpy arrays: the placement run in
    ``dtype`` on the (``rounded``) inputs, and the gradient of ``sum(cx * x) + sum(cl * log_det_J)``.  Computed once."""
    c = case(name)
    args = [v.to(dtype).clone().requires_grad_(True) for v in inputs(name, rounded)]
    x, ldj = place(*args, c['z_matrix'], c['fixed_atoms'])
    loss = (c['cx'].to(dtype) * x).sum() + (c['cl'].to(dtype) * ldj).sum()
    grads = torch.autograd.grad(loss, args)
    out = {'x': x, 'log_det_J': ldj, **{'g_' + k: g for k, g in zip(INPUTS, grads)}}
    return {k: v.detach().to(F64).numpy() for k, v in out.items()}


# ----------------------------------------------------------------------------- comparisons

def circ(a):
    """(sin, cos) of angles: a branch flip at +-pi is no error."""
    a = np.asarray(a, dtype=np.float64)
    return np.stack([np.sin(a), np.cos(a)])


def rel_l2(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))
