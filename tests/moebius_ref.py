"""Float64 torch restatement of the Moebius transformer (reference ``tfep/nn/transformers/moebius.py:374-478`` and the
inverse of ``:142-147``), written from the formulae; CPU tensors, differentiable by autograd.  It serves the shapes that
tests/golden/transformers.npz does not hold (tests/test_gpu_moebius_f64.py).

With ``s = max_radius / (1 + |w|)`` (times ``|x|`` unless ``unit_sphere``), ``u = s w``, ``N = |x|^2 - |u|^2`` (``1 - |u|^2``
on the unit sphere) and ``d = x - u``::

    y = N / |d|^2 d - u

The log-det is ``log |det J|`` of the matrix the reference builds -- ``N (I / |d|^2 - 2 d d^T / |d|^4)``, on a sphere of
radius ``|x|`` multiplied by the projector ``I - x x^T / |x|^2`` and completed with the radial part ``y x^T / |x|^2`` --
through ``torch.linalg.slogdet``, NOT the closed form of ``tfep_amd/csrc/moebius.h``: the two share no arithmetic.  The
norm of ``w = 0`` has torch's zero sub-gradient.
"""
import torch


def moebius(x, w, dimension, max_radius=0.99, unit_sphere=False):
    """``(y, log_det_J)`` of the forward map; ``x`` and ``w`` of shape ``(B, n_vectors * dimension)``."""
    B = x.shape[0]
    xv, wv = x.reshape(B, -1, dimension), w.reshape(B, -1, dimension)
    s = max_radius / (1 + torch.linalg.norm(wv, dim=-1, keepdim=True))
    if unit_sphere:
        x2 = torch.ones_like(s)
    else:
        x_norm = torch.linalg.norm(xv, dim=-1, keepdim=True)
        s = s * x_norm
        x2 = x_norm ** 2
    u = s * wv
    N = x2 - (u * u).sum(dim=-1, keepdim=True)
    d = xv - u
    d2 = (d * d).sum(dim=-1, keepdim=True)
    y = N / d2 * d - u
    eye = torch.eye(dimension, dtype=x.dtype)
    outer = lambda a, b: a.unsqueeze(-1) * b.unsqueeze(-2)                         # noqa: E731
    jac = N.unsqueeze(-1) * (eye / d2.unsqueeze(-1) - 2 * outer(d, d) / d2.unsqueeze(-1) ** 2)
    if not unit_sphere:
        jac = jac @ (eye - outer(xv, xv) / x2.unsqueeze(-1)) + outer(y, xv) / x2.unsqueeze(-1)
    log_det_J = torch.linalg.slogdet(jac)[1].sum(dim=-1)
    return y.reshape(B, -1), log_det_J


def moebius_inverse(y, w, dimension, max_radius=0.99, unit_sphere=False):
    """The inverse: the forward map with ``-w`` (its log-det is that of the inverse map itself)."""
    return moebius(y, -w, dimension, max_radius, unit_sphere)
