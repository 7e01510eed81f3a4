"""Generate tests/golden/geometry.npz from the reference's ``tfep.utils.geometry`` and ``tfep.utils.math``.

Dev-container only (needs the reference, through ``tools/ref_shim.py``; see ``tools/gen_golden.py``).  Everything is
computed by the reference on the CPU in float64; the index-based quantities are also stored as the reference computes
them in float32 from the rounded inputs (``.../f32/...``), which is what the float32 tests measure their bound from.
Gradients are those of ``sum(cotangent * output)`` for the fixed random cotangents stored next to them.

    python tools/gen_golden_geometry.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402,F401
from tfep.utils import geometry as rg  # noqa: E402
from tfep.utils import math as rm  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'geometry.npz')
N_ATOMS, N_ROWS = 7, 11
MIN_SIN, MIN_REJECTION = 0.1, 0.1

# a chain with two extra bonds, and tables in which atom 3 is part of every entry, in every slot
TABLES = {
    'main': dict(pairs=[[0, 1, 2, 3, 4, 5, 0, 6], [1, 2, 3, 4, 5, 6, 4, 2]],
                 triples=[[0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [2, 3, 4, 5, 6]],
                 quads=[[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5], [3, 4, 5, 6]]),
    'hub': dict(pairs=[[3, 1, 3, 3, 5, 6], [0, 3, 2, 4, 3, 3]],
                triples=[[3, 0, 1, 3, 6], [0, 3, 2, 5, 4], [1, 2, 3, 6, 3]],
                quads=[[3, 0, 1, 2, 6], [0, 3, 2, 4, 5], [1, 1, 3, 5, 3], [2, 4, 0, 3, 1]]),
}


def index_coordinates(x, tb):
    """(d, a, t) of positions x (B, n, 3) by the reference's functions."""
    pairs, triples, quads = (torch.tensor(tb[k]) for k in ('pairs', 'triples', 'quads'))
    p = [x[:, triples[i]] for i in range(3)]
    q = [x[:, quads[i]] for i in range(4)]
    return (rg.pdist(x, pairs=pairs), rg.vector_vector_angle(p[0] - p[1], p[2] - p[1]),
            rg.proper_dihedral_angle(q[1] - q[0], q[2] - q[1], q[3] - q[2]))


def well_conditioned(x):
    """Every triple has |sin(angle)| >= MIN_SIN and both rejections of every quad a norm >= MIN_REJECTION."""
    for tb in TABLES.values():
        _, a, _ = index_coordinates(x, tb)
        if float(a.sin().abs().min()) < MIN_SIN:
            return False
        quads = torch.tensor(tb['quads'])
        q = [x[:, quads[i]] for i in range(4)]
        b1 = q[2] - q[1]
        b1 = b1 / b1.norm(dim=-1, keepdim=True)
        for b in (q[0] - q[1], q[3] - q[2]):
            if float((b - (b * b1).sum(-1, keepdim=True) * b1).norm(dim=-1).min()) < MIN_REJECTION:
                return False
    return True


def with_grads(fn, inputs, gen):
    """Outputs of fn(*inputs) (a tensor or a tuple), one random cotangent per output, and the input gradients."""
    inputs = [t.clone().requires_grad_(True) for t in inputs]
    outs = fn(*inputs)
    outs = outs if isinstance(outs, tuple) else (outs,)
    cots = [torch.randn(o.shape, dtype=torch.float64, generator=gen).to(o.dtype) for o in outs]
    grads = torch.autograd.grad(sum((c * o).sum() for c, o in zip(cots, outs)), inputs)
    return [o.detach() for o in outs], cots, list(grads)


def main():
    out = {}
    for seed in range(1000):
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(N_ROWS, N_ATOMS, 3, dtype=torch.float64, generator=gen)
        if well_conditioned(x):
            break
    assert well_conditioned(x), 'no seed gives well-conditioned angles and dihedrals'
    out['seed'] = np.array(seed)
    out['x'] = x.numpy()

    for name, tb in TABLES.items():
        for k, v in tb.items():
            out[f'{name}/{k}'] = np.array(v, dtype=np.int64)
        (d, a, t), cots, (gx,) = with_grads(lambda z: index_coordinates(z, tb), [x], gen)
        for k, v in zip(('d', 'a', 't', 'gd', 'ga', 'gt', 'gx'), (d, a, t, *cots, gx)):
            out[f'{name}/{k}'] = v.numpy()
        # the reference in float32 on the rounded inputs and cotangents
        x32 = x.float().requires_grad_(True)
        o32 = index_coordinates(x32, tb)
        (gx32,) = torch.autograd.grad(sum((c.float() * o).sum() for c, o in zip(cots, o32)), x32)
        for k, v in zip(('d', 'a', 't', 'gx'), (*o32, gx32)):
            out[f'{name}/f32/{k}'] = v.detach().numpy()
    out['pdist_all/d'], out['pdist_all/f32/d'] = rg.pdist(x).numpy(), rg.pdist(x.float()).numpy()

    # the functions of vectors
    u, v, w = (torch.randn(N_ROWS, 3, dtype=torch.float64, generator=gen) for _ in range(3))
    plane = torch.randn(3, dtype=torch.float64, generator=gen)
    for name, fn, inputs in (('vector_vector_angle', rg.vector_vector_angle, [u, v]),
                             ('vector_plane_angle', rg.vector_plane_angle, [u, plane]),
                             ('proper_dihedral_angle', rg.proper_dihedral_angle, [u, v, w])):
        (o,), (c,), grads = with_grads(fn, inputs, gen)
        out.update({f'{name}/in{i}': t.numpy() for i, t in enumerate(inputs)})
        out.update({f'{name}/g{i}': t.numpy() for i, t in enumerate(grads)})
        out[f'{name}/out'], out[f'{name}/cot'] = o.numpy(), c.numpy()
    d, diff = rg.pdist(x, pairs=torch.tensor(TABLES['main']['pairs']), return_diff=True)
    out['pdist_diff/d'], out['pdist_diff/diff'] = d.numpy(), diff.numpy()

    angles = torch.rand(N_ROWS, dtype=torch.float64, generator=gen) * 6.0 - 3.0
    for name, directions in (('rotation_batch', u), ('rotation_single', plane)):
        (o,), (c,), grads = with_grads(rg.rotation_matrix_3d, [angles, directions], gen)
        out.update({f'{name}/angles': angles.numpy(), f'{name}/directions': directions.numpy(), f'{name}/out': o.numpy(),
                    f'{name}/cot': c.numpy(), f'{name}/g_angles': grads[0].numpy(), f'{name}/g_directions': grads[1].numpy()})

    # the polar map, both directions, values and gradients through all three outputs; 37 elements: packs and a tail
    px, py = (torch.randn(37, dtype=torch.float64, generator=gen) for _ in range(2))
    pr = torch.rand(37, dtype=torch.float64, generator=gen) * 2.0 + 0.2
    pa = torch.rand(37, dtype=torch.float64, generator=gen) * 6.0 - 3.0
    for name, fn, inputs in (('cartesian_to_polar', rg.cartesian_to_polar, [px, py]),
                             ('polar_to_cartesian', rg.polar_to_cartesian, [pr, pa])):
        outs, cots, grads = with_grads(lambda a, b: fn(a, b, return_log_det_J=True), inputs, gen)
        for i in range(2):
            out[f'{name}/in{i}'], out[f'{name}/g{i}'] = inputs[i].numpy(), grads[i].numpy()
        for i in range(3):
            out[f'{name}/out{i}'], out[f'{name}/cot{i}'] = outs[i].numpy(), cots[i].numpy()

    # math
    m1, m2 = (torch.randn(N_ROWS, 5, dtype=torch.float64, generator=gen) for _ in range(2))
    out.update({'math/in0': m1.numpy(), 'math/in1': m2.numpy(), 'math/dot': rm.batchwise_dot(m1, m2).numpy(),
                'math/dot_keepdim': rm.batchwise_dot(m1, m2, keepdim=True).numpy(),
                'math/outer': rm.batchwise_outer(m1, m2).numpy()})
    c0, mean0 = rm.cov(m1, return_mean=True)
    c1, mean1 = rm.cov(m1, ddof=0, dim_sample=1, return_mean=True)
    out.update({'math/cov0': c0.numpy(), 'math/mean0': mean0.numpy(), 'math/cov1': c1.numpy(), 'math/mean1': mean1.numpy()})
    wmat = torch.randn(5, 5, dtype=torch.float64, generator=gen)
    z = m1.clone().requires_grad_(True)
    y = torch.tanh(z @ wmat) + 2.0 * z
    out.update({'math/w': wmat.numpy(), 'math/jacobian': rm.batch_autograd_jacobian(z, y, retain_graph=True).numpy(),
                'math/log_abs_det_J': rm.batch_autograd_log_abs_det_J(z, y).numpy()})

    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes, seed {seed}')


if __name__ == '__main__':
    main()
