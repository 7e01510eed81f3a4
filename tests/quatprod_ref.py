"""Torch restatement of the quaternion product transformer (reference ``tfep/nn/transformers/quatprod.py``): the scalar-last
Hamilton product of the normalised parameter quaternion (its conjugate in the inverse direction) with ``x``, written out
component by component; differentiable by autograd, in the dtype of its arguments (the tests hand it float64).  The
log-det of either direction is the constant zero.  ``p = 0`` is 0 / 0 here as in the reference."""
import torch


def quat_torch(x, p, inverse=False):
    """Differentiable torch restatement of the map on (B, D) tensors: scalar-last Hamilton product with the normalised p."""
    B = x.shape[0]
    x, p = x.reshape(B, -1, 4), p.reshape(B, -1, 4)
    q = p / p.norm(dim=-1, keepdim=True)
    if inverse:
        q = q * torch.tensor([-1.0, -1.0, -1.0, 1.0], dtype=q.dtype, device=q.device)
    a1, a2, a3, a4 = q.unbind(-1)
    b1, b2, b3, b4 = x.unbind(-1)
    y = torch.stack([a4 * b1 + a1 * b4 + a2 * b3 - a3 * b2,
                     a4 * b2 - a1 * b3 + a2 * b4 + a3 * b1,
                     a4 * b3 + a1 * b2 - a2 * b1 + a3 * b4,
                     a4 * b4 - a1 * b1 - a2 * b2 - a3 * b3], dim=-1)
    return y.reshape(B, -1)
