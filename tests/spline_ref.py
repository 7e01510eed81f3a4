"""Float64 torch restatement of the rational-quadratic neural spline transformer (reference
``tfep/nn/transformers/spline.py``: ``_get_parameters`` :319-417, ``_assign_bins`` :567-650, forward / inverse :478-494 /
:521-536, the log-det :546-564, the circular shift :236-238 / :257-259), written from the formulae; CPU tensors,
differentiable by autograd, every flag combination (circular, identity boundary slopes, learnable lower / upper bound,
``y0 / yf`` of their own).

The rules it keeps: the bin of ``v`` is ``#{knots < v} - 1`` with the STRICT ``>`` (a point on a knot belongs to the bin
below it, a point on the first knot to the lower tail); outside the knots the map is linear with the boundary slope (what
the reference's two sentinel knots amount to); softplus has torch's threshold 20; the raw slopes are offset by
``log(exp(1 - min_slope) - 1)``, so that a raw slope of zero is a slope of one.

Three intermediates can be taken out of the graph and handed back as autograd leaves (``leaves=True``), for the
sensitivities tests/spline_cases.py reads: the K + 1 knot slopes ``d`` (B, K + 1, D) and the unnormalised softmax
exponentials ``ew``, ``eh`` (B, K, D) of the widths and heights (``exp(raw - max raw)``, what the kernels form before they
divide by the sum).  ``scale=(sd, sew, seh)`` multiplies the three by factors and leaves them in the graph: the reference
with its intermediates moved.
"""
import math

import torch

F64 = torch.float64


def n_parameters_per_feature(n_bins, circular=False, identity_boundary_slopes=False, learn_lower_bound=False,
                             learn_upper_bound=False):
    n = 3 * n_bins + 1 + int(learn_lower_bound) + int(learn_upper_bound)
    if identity_boundary_slopes:
        n -= 1 if circular else 2
    return n


def _softplus(z):
    return torch.where(z > 20.0, z, torch.log1p(torch.exp(torch.clamp(z, max=20.0))))


def intermediates(parameters, x0, xf, n_bins, y0=None, yf=None, circular=False, identity_boundary_slopes=False,
                  learn_lower_bound=False, learn_upper_bound=False, min_bin_size=1e-4, min_slope=1e-4, leaves=False,
                  scale=None):
    """dict of what the map is evaluated from: ``d`` (B, K + 1, D), ``ew``, ``eh`` (B, K, D), the domain ``x0, y0`` (the
    lower corner, (D,) or (B, D)), ``W, H`` (the width and height that the softmax shares out, without the K minimum bins),
    ``xf`` (D,), ``shift`` ((B, D) or None) and ``min_bin``."""
    K = n_bins
    x0, xf = x0.to(F64), xf.to(F64)
    y0 = x0 if y0 is None else y0.to(F64)
    yf = xf if yf is None else yf.to(F64)
    B = parameters.shape[0]
    P = n_parameters_per_feature(K, circular, identity_boundary_slopes, learn_lower_bound, learn_upper_bound)
    p = parameters.reshape(B, P, -1)
    n_slopes = K - 1 if identity_boundary_slopes else (K if circular else K + 1)
    raw = p[:, 2 * K:2 * K + n_slopes]
    shift = p[:, -1] if circular else None
    if circular and not identity_boundary_slopes:
        raw = torch.cat([raw, raw[:, :1]], dim=1)
    if identity_boundary_slopes:
        zero = torch.zeros_like(p[:, :1])
        raw = torch.cat([zero, raw, zero], dim=1)
    d = _softplus(raw + math.log(math.exp(1.0 - min_slope) - 1.0)) + min_slope
    ew = torch.exp(p[:, :K] - p[:, :K].max(dim=1, keepdim=True).values.detach())
    eh = torch.exp(p[:, K:2 * K] - p[:, K:2 * K].max(dim=1, keepdim=True).values.detach())
    if scale is not None:
        d, ew, eh = d * scale[0], ew * scale[1], eh * scale[2]
    if leaves:
        d, ew, eh = (t.detach().clone().requires_grad_(True) for t in (d, ew, eh))

    W = xf - x0 - K * min_bin_size
    H = yf - y0 - K * min_bin_size
    if learn_lower_bound or learn_upper_bound:
        domain_scale = torch.exp(p[:, -1])
        W, H = W * domain_scale, H * domain_scale
        if learn_lower_bound and learn_upper_bound:
            x0, y0 = x0 + p[:, -2], y0 + p[:, -2]
        elif learn_lower_bound:
            x0, y0 = xf - W - K * min_bin_size, yf - H - K * min_bin_size
    return dict(d=d, ew=ew, eh=eh, x0=x0, y0=y0, W=W, H=H, xf=xf, shift=shift, min_bin=min_bin_size, K=K)


def knots(q):
    """``(knots_x, knots_y, widths, heights)``: (B, K + 1, D) and (B, K, D)."""
    B, K, D = q['ew'].shape
    widths = q['ew'] / q['ew'].sum(dim=1, keepdim=True) * q['W'].expand(B, D).unsqueeze(1) + q['min_bin']
    heights = q['eh'] / q['eh'].sum(dim=1, keepdim=True) * q['H'].expand(B, D).unsqueeze(1) + q['min_bin']
    x0, y0 = q['x0'].expand(B, D).unsqueeze(1), q['y0'].expand(B, D).unsqueeze(1)
    return (torch.cat([x0, x0 + torch.cumsum(widths, dim=1)], dim=1), torch.cat([y0, y0 + torch.cumsum(heights, dim=1)], dim=1),
            widths, heights)


def evaluate(v, q, inverse=False):
    """``(out, log_derivative, bin)``, each (B, D): the map (or its inverse) at ``v``, the log of the derivative of that
    direction, and ``#{knots < v} - 1`` (-1: lower tail, K: upper tail).  Without the circular shift."""
    K = q['K']
    kx, ky, widths, heights = knots(q)
    bins = (v.unsqueeze(1) > (ky if inverse else kx)).sum(dim=1) - 1
    lower, upper = bins < 0, bins >= K
    tail = lower | upper
    k = bins.clamp(0, K - 1).unsqueeze(1)
    take = lambda t, i: torch.gather(t, 1, i).squeeze(1)                           # noqa: E731
    w, h, xk, yk = take(widths, k), take(heights, k), take(kx, k), take(ky, k)
    dk, dk1 = take(q['d'], k), take(q['d'], k + 1)
    s = h / w
    t = dk1 + dk - 2 * s
    if inverse:
        ym = torch.where(tail, 0.5 * h, v - yk)                  # (a tail element: the bin's middle, never selected)
        a = h * (s - dk) + ym * t
        b = h * dk - ym * t
        c = -s * ym
        eps = 2 * c / (-b - torch.sqrt(b * b - 4 * a * c))
        out = eps * w + xk
    else:
        eps = torch.where(tail, torch.full_like(v, 0.5), (v - xk) / w)
    e1 = eps * (1 - eps)
    den = s + t * e1
    if not inverse:
        out = yk + h * (s * eps * eps + dk * e1) / den
    ld = torch.log(s * s * (dk1 * eps * eps + 2 * s * e1 + dk * (1 - eps) ** 2) / (den * den))
    # the tails: linear through the first / last knot with its slope
    db = torch.where(lower, q['d'][:, 0], q['d'][:, K])
    bx, by = torch.where(lower, kx[:, 0], kx[:, K]), torch.where(lower, ky[:, 0], ky[:, K])
    out_t = bx + (v - by) / db if inverse else by + db * (v - bx)
    out = torch.where(tail, out_t, out)
    ld = torch.where(tail, torch.log(db), ld)
    return out, (-ld if inverse else ld), bins


def forward_elements(x, parameters, x0, xf, n_bins, **cfg):
    """``(y, log-derivative per element, bins, q)`` of ``NeuralSplineTransformer.forward``."""
    q = intermediates(parameters, x0, xf, n_bins, **cfg)
    if q['shift'] is not None:
        x = torch.remainder(x - q['x0'] + q['shift'], q['xf'] - q['x0']) + q['x0']
    return (*evaluate(x, q), q)


def inverse_elements(y, parameters, x0, xf, n_bins, **cfg):
    """``(x, log-derivative per element, bins, q)`` of ``NeuralSplineTransformer.inverse``."""
    q = intermediates(parameters, x0, xf, n_bins, **cfg)
    x, ld, bins = evaluate(y, q, inverse=True)
    if q['shift'] is not None:
        x = torch.remainder(x - q['x0'] - q['shift'], q['xf'] - q['x0']) + q['x0']
    return x, ld, bins, q


def spline_forward(x, parameters, x0, xf, n_bins, **cfg):
    """``(y, log_det_J)``; ``x`` (B, D), ``parameters`` (B, P D) in the reference layout (column p D + f)."""
    y, ld, _, _ = forward_elements(x, parameters, x0, xf, n_bins, **cfg)
    return y, ld.sum(dim=1)


def spline_inverse(y, parameters, x0, xf, n_bins, **cfg):
    x, ld, _, _ = inverse_elements(y, parameters, x0, xf, n_bins, **cfg)
    return x, ld.sum(dim=1)
