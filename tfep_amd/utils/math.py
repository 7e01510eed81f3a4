"""Small math helpers on batches (reference ``tfep/utils/math.py``): torch expressions on the device of their inputs."""
import torch


def batchwise_dot(x1, x2, keepdim=False):
    """Dot products of the vectors of ``x1`` and ``x2``, both ``(*, N)``: shape ``(*,)``, or ``(*, 1)`` with ``keepdim``."""
    return (x1 * x2).sum(dim=-1, keepdim=keepdim)


def batchwise_outer(x1, x2):
    """Outer products of the vectors of ``x1`` and ``x2``, both ``(*, N)``: shape ``(*, N, N)``."""
    return x1.unsqueeze(-1) * x2.unsqueeze(-2)


def cov(x, ddof=1, dim_sample=0, inplace=False, return_mean=False):
    """Covariance matrix ``(m, m)`` of ``n`` samples of an ``m``-variate variable: ``x`` is ``(n, m)``, or ``(m, n)`` with
    ``dim_sample=1``.  Divides by ``n - ddof``.  ``inplace`` centres ``x`` itself; ``return_mean`` also returns the
    mean (shaped as ``torch.mean(x, dim_sample, keepdim=dim_sample == 1)`` gives it)."""
    if x.dim() != 2:
        raise ValueError('The function supports only 2D matrices')
    if dim_sample not in (0, 1):
        raise ValueError('dim_sample must be either 0 or 1')
    mean = torch.mean(x, dim_sample, keepdim=dim_sample == 1)
    if inplace:
        x -= mean
    else:
        x = x - mean
    n = x.shape[dim_sample] - ddof
    c = (x.t() @ x if dim_sample == 0 else x @ x.t()) / n
    return (c, mean) if return_mean else c


def batch_autograd_jacobian(x, y, **grad_kwargs):
    """Per-sample Jacobian of ``y`` ``(batch_size, *)`` with respect to ``x`` ``(batch_size, *)``: shape ``(batch_size,
    *y.shape[1:], *x.shape[1:])``.  Sample ``b`` of ``y`` must depend on sample ``b`` of ``x`` only.  ``grad_kwargs`` go
    to ``autograd.grad`` (``create_graph``, ``retain_graph``).

    One ``autograd.grad`` per feature of ``y``, not the reference's single batched call: ``is_grads_batched`` maps the
    backward with ``vmap``, and the HIP ops of this package have no batching rule."""
    y_sum = y.sum(dim=0)
    n_y = y_sum.numel()
    basis = torch.eye(n_y, dtype=y.dtype, device=y.device).reshape(n_y, *y_sum.shape)
    kwargs = dict(grad_kwargs)
    keep = kwargs.pop('retain_graph', None)
    keep = kwargs.get('create_graph', False) if keep is None else keep
    jac = torch.stack([torch.autograd.grad(y_sum, x, basis[i], retain_graph=keep or i + 1 < n_y, **kwargs)[0]
                       for i in range(n_y)])
    return jac.transpose(0, 1).reshape(x.shape[0], *y.shape[1:], *x.shape[1:])


def batch_autograd_log_abs_det_J(x, y, **grad_kwargs):
    """``log |det J|`` per sample, ``(batch_size,)``, of ``y`` ``(batch_size, N)`` with respect to ``x`` ``(batch_size, N)``."""
    return torch.linalg.slogdet(batch_autograd_jacobian(x, y, **grad_kwargs))[1]
