"""Tensor-level wrappers of the C ABI of include/tfep_hip.h.

Every function takes float32 HIP tensors or, where the entry point has a ``_f64`` twin, float64 ones (the dtype of its first
tensor picks the kernels, ``_dtype`` / ``_sfx``; mixed dtypes are a TypeError), launches on the current HIP stream of the
tensor's device and returns fresh output tensors (inputs are never modified, like the reference:
flows/autoregressive.py:165-166), unless the caller hands outputs in (``out=`` of the transformer VJPs).  No autograd, no
CPU path.
"""
import ctypes
import os

import torch

from . import _lib, _tables
from ._lib import ParamLayout, SplineDesc, SplineDescF64, call, check_device_tensor, ptr, rows, stream_of
from ._tables import (ZMATRIX_LDS_LIMIT, ZMATRIX_MAX_ATOMS, ZMATRIX_MAX_PLACED, ZMatrixTables, check_edges,  # noqa: F401
                      check_index_table, check_zmatrix, edge_incidence, incidence_lists, index_tables,
                      zmatrix_index_tables, zmatrix_tables)                   # (the host-built integer tables: pure torch)


def _dtype(x):
    """The kernel family of an input: float64 tensors take the float64 kernels, anything else the float32 ones (whose checks
    reject what is not float32)."""
    return torch.float64 if isinstance(x, torch.Tensor) and x.dtype == torch.float64 else torch.float32


def _sfx(dtype):
    return '_f64' if dtype == torch.float64 else ''


_F64 = torch.float64


def _f64(t, name):
    return None if t is None else check_device_tensor(t, name, _F64)


def _mask(mask, dtype):
    """The mask as the kernels of ``dtype`` read it.  float64: any floating-point mask, converted (a 0 / 1 array is exact in
    any float type: a float32 mask on a float64 layer is fine); float32: the mask as it is."""
    if mask is None:
        return None
    if dtype == _F64:
        check_device_tensor(mask, 'mask', mask.dtype if mask.is_floating_point() else _F64)
        return mask.to(_F64).contiguous()
    return mask.contiguous()


def _ldj_out(log_det_J, B, like, dtype=torch.float32):
    """Return (tensor, accumulate flag): accumulate into ``log_det_J`` if given."""
    if log_det_J is None:
        return torch.empty(B, dtype=dtype, device=like.device), 0
    check_device_tensor(log_det_J, 'log_det_J', dtype)
    if log_det_J.shape != (B,) or not log_det_J.is_contiguous():
        raise ValueError('log_det_J must be a contiguous (batch,) tensor')
    return log_det_J, 1


def _check_params(parameters, B, n, name='parameters', dtype=torch.float32, copy=True):
    parameters, ld = rows(parameters, name, dtype, copy)
    if parameters.shape[0] != B or parameters.shape[1] != n:
        raise ValueError(f'{name} must have shape ({B}, {n}), got {tuple(parameters.shape)}')
    return parameters, ld


def _param_block(parameters, B, P, D, dtype, layout=None, name='parameters', copy=True):
    """``(tensor, ParamLayout)`` of P parameters for each of D features: a (B, P D) tensor in the reference layout (column
    p*D + f), which may be a column slice of a wider one (``rows``), or, with ``layout = (ld, stride_p, stride_f)``, the buffer
    that the layout indexes: B rows of stride ``ld``, unit column stride, wide enough for the last feature's last parameter."""
    if layout is None:
        parameters, ld = _check_params(parameters, B, P * D, name, dtype, copy)
        return parameters, ParamLayout(ld, D, 1)
    ld, stride_p, stride_f = (int(v) for v in layout)
    reach = (P - 1) * stride_p + (D - 1) * stride_f
    width = parameters.shape[1] if check_device_tensor(parameters, name, dtype).dim() == 2 else -1
    if (width < 0 or parameters.shape[0] != B or min(stride_p, stride_f) < 0 or not (D == 0 or reach < width <= ld)
            or (width > 1 and parameters.stride(1) != 1) or (B > 1 and parameters.stride(0) != ld)):
        raise ValueError(f'{name} must be the ({B}, > {reach}) buffer that layout {(ld, stride_p, stride_f)} indexes (unit '
                         f'column stride), got shape {tuple(parameters.shape)}, strides {tuple(parameters.stride())}')
    return parameters, ParamLayout(ld, stride_p, stride_f)


def _vjp_args(dt, x, parameters, P, grad_y, grad_log_det_J, layout, out, alloc, ld_only=False):
    """The arguments that the six transformer VJP entry points share, checked against the kernel family ``dt`` (TypeError)
    and for their shapes (ValueError) before anything is launched: ``call(name, *head, <the transformer's own>, *cot, gl,
    *tail)`` with ``head`` = x and the parameters (``_param_block``; ``ld_only``: their row stride, not a layout), ``cot`` =
    grad_y, ``gl`` = grad_log_det_J ((B,), or None: NULL), ``tail`` = the outputs, the sizes and the stream.  ``out = (grad_x,
    grad_parameters)`` is held to the rules of ``x`` and ``parameters`` but never copied (ValueError instead); without it
    grad_x is uninitialised and grad_parameters comes from ``alloc`` (``zeros`` or ``torch.empty``) in the shape of
    ``parameters``.  Also returns ``grads = (grad_x, grad_parameters)`` and ``keep``."""
    x, ldx = rows(x, 'x', dt)
    B, D = x.shape
    gy, ldgy = rows(grad_y, 'grad_y', dt)
    if gy.shape != x.shape:
        raise ValueError(f'grad_y must have the shape of x, {tuple(x.shape)}, got {tuple(gy.shape)}')
    if grad_log_det_J is not None and check_device_tensor(grad_log_det_J, 'grad_log_det_J', dt).shape != (B,):
        raise ValueError(f'grad_log_det_J must have shape ({B},), got {tuple(grad_log_det_J.shape)}')
    gl = None if grad_log_det_J is None else grad_log_det_J.contiguous()
    p, lay = _param_block(parameters, B, P, D, dt, layout)
    if out is None:
        gx, ldgx = torch.empty(B, D, dtype=dt, device=x.device), max(D, 1)
        gp = alloc(*p.shape, dtype=dt, device=x.device)
        glay = ParamLayout(max(gp.shape[1], 1), lay.stride_p, lay.stride_f)
    else:
        gx, ldgx = _check_params(out[0], B, D, 'grad_x', dt, copy=False)
        gp, glay = _param_block(out[1], B, P, D, dt, layout, 'grad_parameters', copy=False)
    if ld_only:
        lay, glay = lay.ld, glay.ld
    # (``keep``: contiguous copies are held in the caller's locals until the launch is queued: a temporary freed inside the
    # argument list hands its block back to the caching allocator, and the NEXT temporary may be written over it)
    return ((ptr(x), ldx, ptr(p), lay), (ptr(gy), ldgy), ptr(gl), (ptr(gp), glay, ptr(gx), ldgx, B, D, stream_of(x)), (gx, gp),
            (x, p, gy, gl))


# ----------------------------------------------------------------------------- affine

def affine(x, parameters, inverse=False, log_det_J=None, layout=None):
    """AffineTransformer.forward / .inverse (reference affine.py:51-106).  float64 tensors run on the float64 kernels.
    ``layout``: see ``_param_block``."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    B, D = x.shape
    parameters, lay = _param_block(parameters, B, 2, D, dt, layout)
    y = torch.empty(B, D, dtype=x.dtype, device=x.device)
    ldj, acc = _ldj_out(log_det_J, B, x, dt)
    fn = ('tfep_affine_inverse' if inverse else 'tfep_affine_forward') + _sfx(dt)
    call(fn, ptr(x), ldx, ptr(parameters), lay, ptr(y), max(D, 1), ptr(ldj), acc, B, D, stream_of(x))
    return y, ldj


def affine_backward(x, parameters, grad_y, grad_log_det_J, *, layout=None, out=None):
    """VJP of ``affine`` (forward) at ``x``: ``(grad_x, grad_parameters)`` (reference affine.py:321-323); ``_vjp_args``."""
    dt = _dtype(x)
    head, cot, gl, tail, grads, keep = _vjp_args(dt, x, parameters, 2, grad_y, grad_log_det_J, layout, out, zeros)
    call('tfep_affine_backward' + _sfx(dt), *head, *cot, gl, *tail)
    return grads


def sos(x, parameters, n_polynomials, log_det_J=None):
    """SOSPolynomialTransformer.forward (reference sos.py:81-108): ``parameters`` (B, (2 K + 1) D) in the reference layout.
    float64 tensors run on the float64 kernels."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    B, D = x.shape
    K = int(n_polynomials)
    if K < 1:
        raise ValueError(f'n_polynomials must be positive, got {K}')
    parameters, lay = _param_block(parameters, B, 2 * K + 1, D, dt)
    y = torch.empty(B, D, dtype=x.dtype, device=x.device)
    ldj, acc = _ldj_out(log_det_J, B, x, dt)
    call('tfep_sos_forward' + _sfx(dt), ptr(x), ldx, ptr(parameters), lay, K, ptr(y), max(D, 1), ptr(ldj), acc, B, D,
         stream_of(x))
    return y, ldj


def sos_backward(x, parameters, n_polynomials, grad_y, *, layout=None, out=None):
    """VJP of ``sos`` at ``x`` for the cotangent of y: ``(grad_x, grad_parameters)``.  The log-det has no cotangent
    (non-differentiable, reference sos.py:222); ``_vjp_args``."""
    dt, K = _dtype(x), int(n_polynomials)
    head, cot, _, tail, grads, keep = _vjp_args(dt, x, parameters, 2 * K + 1, grad_y, None, layout, out, torch.empty)
    call('tfep_sos_backward' + _sfx(dt), *head, K, *cot, *tail)
    return grads


def sos_fused_desc(n_polynomials):
    """The descriptor argument of the fused output-layer kernel for the SOS transformer (kind TFEP_FUSED_SOS): ``n_bins``
    carries the number of polynomials, nothing else is read."""
    return SplineDesc(None, None, None, None, int(n_polynomials), 0, 0, 0, 0, 0.0, 0.0)


def volume_preserving_shift(x, shift, periodic_mask=None, limits=(0.0, 1.0), inverse=False):
    """VolumePreservingShiftTransformer (reference affine.py:366-456); log-det is zero."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    B, D = x.shape
    shift, lds = _check_params(shift, B, D, 'shift', dt)
    y = torch.empty(B, D, dtype=x.dtype, device=x.device)
    if periodic_mask is not None:
        check_device_tensor(periodic_mask, 'periodic_mask', torch.int32)
    call('tfep_volume_preserving_shift' + _sfx(dt), ptr(x), ldx, ptr(shift), lds,
         ptr(periodic_mask), float(limits[0]), float(limits[1]), -1 if inverse else 1,
         ptr(y), max(D, 1), B, D, stream_of(x))
    return y, zeros(B, dtype=x.dtype, device=x.device)


# ----------------------------------------------------------------------------- spline

class SplineConfig:
    """Host mirror of tfep_spline_desc (float32 domain arrays) or, with ``dtype=torch.float64``, of tfep_spline_desc_f64
    (float64 domain arrays and minimum sizes; validated here, before any launch); keeps the (D,) device arrays alive."""

    def __init__(self, x0, xf, y0, yf, n_bins, circular=False, identity_boundary_slopes=False,
                 learn_lower_bound=False, learn_upper_bound=False, min_bin_size=1e-4, min_slope=1e-4,
                 dtype=torch.float32):
        self.dtype = dtype
        self.x0, self.xf, self.y0, self.yf = (check_device_tensor(t.contiguous(), n, dtype)
                                              for t, n in ((x0, 'x0'), (xf, 'xf'), (y0, 'y0'), (yf, 'yf')))
        lib = _lib.load()
        self.desc = (SplineDescF64 if dtype == _F64 else SplineDesc)(
            self.x0.data_ptr(), self.xf.data_ptr(), self.y0.data_ptr(), self.yf.data_ptr(), int(n_bins), int(bool(circular)),
            int(bool(identity_boundary_slopes)), int(bool(learn_lower_bound)), int(bool(learn_upper_bound)),
            float(min_bin_size), float(min_slope))
        n = getattr(lib, 'tfep_spline_n_parameters_per_feature' + _sfx(dtype))(ctypes.byref(self.desc))
        if n < 0:       # (float64: the descriptor was refused, with a message; float32: the count of a negative n_bins)
            raise ValueError(lib.tfep_last_error().decode() if dtype == _F64 else f'spline: n_bins={int(n_bins)} is negative')
        self.n_parameters_per_feature = n

    def take(self, index):
        """This configuration for the features ``index`` (a device index tensor: a subset or a permutation), in that
        order: the four domain arrays indexed, bins, flags and dtype as they are."""
        d = self.desc
        return SplineConfig(self.x0[index], self.xf[index], self.y0[index], self.yf[index], d.n_bins, d.circular,
                            d.identity_boundary_slopes, d.learn_lower_bound, d.learn_upper_bound, d.min_bin_size,
                            d.min_slope, dtype=self.dtype)


def spline(x, parameters, cfg, inverse=False, log_det_J=None, layout=None):
    """NeuralSplineTransformer.forward / .inverse (reference spline.py:184-261).  The kernels are those of ``cfg.dtype``:
    ``x`` and ``parameters`` must be of that dtype.  ``layout``: see ``_param_block``."""
    dt = cfg.dtype
    x, ldx = rows(x, 'x', dt)
    B, D = x.shape
    if cfg.x0.numel() != D:
        raise ValueError(f'spline domain has {cfg.x0.numel()} features, input has {D}')
    parameters, lay = _param_block(parameters, B, cfg.n_parameters_per_feature, D, dt, layout)
    y = torch.empty(B, D, dtype=x.dtype, device=x.device)
    ldj, acc = _ldj_out(log_det_J, B, x, dt)
    fn = ('tfep_spline_inverse' if inverse else 'tfep_spline_forward') + _sfx(dt)
    call(fn, ptr(x), ldx, ptr(parameters), lay, ctypes.byref(cfg.desc), ptr(y), max(D, 1), ptr(ldj), acc, B, D, stream_of(x))
    return y, ldj


def spline_backward(x, parameters, cfg, grad_y, grad_log_det_J, *, layout=None, out=None):
    """VJP of ``spline`` (forward) at ``x``: ``(grad_x, grad_parameters)``, on the kernels of ``cfg.dtype``; ``_vjp_args``."""
    head, cot, gl, tail, grads, keep = _vjp_args(cfg.dtype, x, parameters, cfg.n_parameters_per_feature, grad_y,
                                                 grad_log_det_J, layout, out, zeros)
    if cfg.x0.numel() != grads[0].shape[1]:
        raise ValueError(f'spline domain has {cfg.x0.numel()} features, input has {grads[0].shape[1]}')
    call('tfep_spline_backward' + _sfx(cfg.dtype), *head, ctypes.byref(cfg.desc), *cot, gl, *tail)
    return grads


# ----------------------------------------------------------------------------- moebius

def moebius(x, parameters, dimension, max_radius=0.99, unit_sphere=False, inverse=False, log_det_J=None):
    """MoebiusTransformer.forward / .inverse (reference moebius.py:104-147, :374-478).  float64 tensors run on the float64
    kernels; mixed float32 / float64 arguments are a TypeError."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    B, D = x.shape
    parameters, ldp = _check_params(parameters, B, D, dtype=dt)
    y = torch.empty(B, D, dtype=x.dtype, device=x.device)
    ldj, acc = _ldj_out(log_det_J, B, x, dt)
    call('tfep_moebius_forward' + _sfx(dt), ptr(x), ldx, ptr(parameters), ldp,
         int(dimension), float(max_radius), int(bool(unit_sphere)), -1 if inverse else 1,
         ptr(y), max(D, 1), ptr(ldj), acc, B, D, stream_of(x))
    return y, ldj


def moebius_backward(x, parameters, dimension, max_radius, unit_sphere, grad_y, grad_log_det_J, *, out=None):
    """VJP of ``moebius`` (forward) at ``x``: ``(grad_x, grad_parameters)``; float32 or float64 by ``x``; ``_vjp_args``."""
    dt = _dtype(x)
    head, cot, gl, tail, grads, keep = _vjp_args(dt, x, parameters, 1, grad_y, grad_log_det_J, None, out, zeros, ld_only=True)
    call('tfep_moebius_backward' + _sfx(dt), *head, int(dimension), float(max_radius), int(bool(unit_sphere)), 1, *cot, gl,
         *tail)
    return grads


def symmetrized_moebius(x, parameters, dimension, max_radius=0.99, inverse=False, log_det_J=None):
    """SymmetrizedMoebiusTransformer.forward / .inverse (reference moebius.py:481-629).  float64 tensors run on the float64
    kernels; mixed float32 / float64 arguments are a TypeError."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    B, D = x.shape
    parameters, ldp = _check_params(parameters, B, D, dtype=dt)
    y = torch.empty(B, D, dtype=x.dtype, device=x.device)
    ldj, acc = _ldj_out(log_det_J, B, x, dt)
    call('tfep_symmetrized_moebius' + _sfx(dt), ptr(x), ldx, ptr(parameters), ldp, int(dimension), float(max_radius),
         int(bool(inverse)), ptr(y), max(D, 1), ptr(ldj), acc, B, D, stream_of(x))
    return y, ldj


def symmetrized_moebius_backward(x, parameters, dimension, max_radius, inverse, grad_y, grad_log_det_J, *, out=None):
    """VJP of ``symmetrized_moebius`` in the direction ``inverse`` at its input ``x``: ``(grad_x, grad_parameters)``; the
    log-det carries gradient in both directions; ``_vjp_args``."""
    dt = _dtype(x)
    head, cot, gl, tail, grads, keep = _vjp_args(dt, x, parameters, 1, grad_y, grad_log_det_J, None, out, torch.empty,
                                                 ld_only=True)
    call('tfep_symmetrized_moebius_backward' + _sfx(dt), *head, int(dimension), float(max_radius), int(bool(inverse)), *cot,
         gl, *tail)
    return grads


def quaternion_product(x, parameters, inverse=False, log_det_J=None):
    """QuaternionProductTransformer.forward / .inverse (reference quatprod.py): every 4 contiguous features are a quaternion,
    scalar last.  The log-det is zero (an accumulated ``log_det_J`` is returned untouched).  float64 tensors run on the
    float64 kernels; mixed float32 / float64 arguments are a TypeError; a feature count that is no multiple of 4 is a
    ValueError."""
    if isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape[1] % 4 != 0:
        raise ValueError(f'quaternion_product: n_features={x.shape[1]} is not a multiple of 4 (quaternions)')
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    B, D = x.shape
    parameters, ldp = _check_params(parameters, B, D, dtype=dt)
    y = torch.empty(B, D, dtype=x.dtype, device=x.device)
    ldj, acc = _ldj_out(log_det_J, B, x, dt)
    call('tfep_quaternion_product' + _sfx(dt), ptr(x), ldx, ptr(parameters), ldp, int(bool(inverse)), ptr(y), max(D, 1),
         ptr(ldj), acc, B, D, stream_of(x))
    return y, ldj


def quaternion_product_backward(x, parameters, inverse, grad_y, *, out=None):
    """VJP of ``quaternion_product`` in the direction ``inverse`` at its input ``x``: ``(grad_x, grad_parameters)``.  The
    log-det is the constant zero: its cotangent is no argument; ``_vjp_args``."""
    dt = _dtype(x)
    head, cot, _, tail, grads, keep = _vjp_args(dt, x, parameters, 1, grad_y, None, None, out, torch.empty, ld_only=True)
    call('tfep_quaternion_product_backward' + _sfx(dt), *head, int(bool(inverse)), *cot, *tail)
    return grads


def moebius_split_out(x, parameters, max_radius, cols_padded):
    """Forward map of unit-sphere 2-vectors that also returns y as split-f16 rows ``(y, log_det_J, y_split, y_inv_scale)`` for
    the next masked linear (``tfep_moebius_forward_split_out``)."""
    x, ldx = rows(x, 'x')
    B, D = x.shape
    parameters, ldp = _check_params(parameters, B, D)
    if ldx % 2 or ldp % 2 or x.data_ptr() % 8 or parameters.data_ptr() % 8:
        # (copies, not .contiguous(): a single row counts as contiguous wherever it starts and would keep its pointer)
        x, parameters = (t.clone(memory_format=torch.contiguous_format) for t in (x, parameters))
        ldx = ldp = D
    y = torch.empty(B, D, dtype=x.dtype, device=x.device)
    ldj = torch.empty(B, dtype=x.dtype, device=x.device)
    ys = zeros(B, cols_padded, dtype=torch.float32, device=x.device) if cols_padded > D else \
        torch.empty(B, cols_padded, dtype=torch.float32, device=x.device)
    ys_inv = torch.empty(max(B, 1), dtype=torch.float32, device=x.device)
    call('tfep_moebius_forward_split_out', ptr(x), ldx, ptr(parameters), ldp, float(max_radius), ptr(y), D, ptr(ldj), 0, ptr(ys),
         cols_padded, ptr(ys_inv), B, D, stream_of(x))
    return y, ldj, ys, ys_inv


# ----------------------------------------------------------------------------- embedding / index helpers

def periodic_embedding(x, periodic_indices, nonperiodic_indices, lower, upper):
    """PeriodicEmbedding.forward (reference mafembed.py:112-145)."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    B = x.shape[0]
    n_per, n_non = periodic_indices.numel(), nonperiodic_indices.numel()
    out = torch.empty(B, n_non + 2 * n_per, dtype=x.dtype, device=x.device)
    call('tfep_periodic_embedding' + _sfx(dt), ptr(x), ldx, ptr(periodic_indices), n_per, ptr(nonperiodic_indices), n_non,
         float(lower), float(upper), ptr(out), n_non + 2 * n_per, B, stream_of(x))
    return out


#: the sizes the flip-invariant embedding kernels are built for (``csrc/flipembed.h``)
FLIP_MAX_VECTOR_DIM, FLIP_MAX_HIDDEN, FLIP_MAX_EMBEDDING_DIM = 8, 64, 32


def flip_embedding_supported(vector_dim, hidden, emb_dim):
    """Whether ``tfep_flip_invariant_embedding*`` takes these network sizes."""
    return 1 <= vector_dim <= FLIP_MAX_VECTOR_DIM and 1 <= hidden <= FLIP_MAX_HIDDEN and 1 <= emb_dim <= FLIP_MAX_EMBEDDING_DIM


def _flip_head(x, embedded_indices, nonembedded_indices, vector_dim, parameters, dt):
    """The leading arguments the forward and the backward entry point share; ``parameters``: the eight tensors
    ``embedding_layer.{0,2}.{weight,bias}``, ``weight_layer.{0,2}.{weight,bias}`` in that order.  Returns ``(args, keep,
    n_out)``: ``keep`` holds the contiguous copies until the launch is queued."""
    if len(parameters) != 8:
        raise ValueError('flip_invariant_embedding: eight parameter tensors expected')
    keep = [check_device_tensor(p, 'parameters', dt).contiguous() for p in parameters]
    for t, n in ((embedded_indices, 'embedded_indices'), (nonembedded_indices, 'nonembedded_indices')):
        check_device_tensor(t, n, torch.int32)
    d, (H, d_w), (E, H2) = int(vector_dim), keep[0].shape, keep[2].shape
    shapes = [(H, d), (H,), (E, H), (E,), (H, d), (H,), (1, H), (1,)]
    if [tuple(p.shape) for p in keep] != shapes:
        raise ValueError(f'flip_invariant_embedding: parameter shapes {[tuple(p.shape) for p in keep]} are not those of '
                         f'two perceptrons {d} -> {H} -> {E} / 1')
    n_emb, n_non = embedded_indices.numel(), nonembedded_indices.numel()
    if n_emb + n_non != x.shape[1]:
        raise ValueError(f'flip_invariant_embedding: the index tables cover {n_emb + n_non} features, x has {x.shape[1]}')
    eidx, nidx = embedded_indices.contiguous(), nonembedded_indices.contiguous()
    keep += [eidx, nidx]
    args = (ptr(eidx), n_emb, ptr(nidx), n_non, d, H, E, *(ptr(p) for p in keep[:8]))
    return args, keep, n_non + (n_emb // d if d > 0 else 0) * E


def flip_invariant_embedding(x, embedded_indices, nonembedded_indices, vector_dim, parameters):
    """FlipInvariantEmbedding.forward (reference mafembed.py:270-306) in one launch.  float64 tensors run on the float64
    kernel; mixed float32 / float64 arguments are a TypeError; sizes over the limits a ValueError."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    B = x.shape[0]
    head, keep, n_out = _flip_head(x, embedded_indices, nonembedded_indices, vector_dim, parameters, dt)
    out = torch.empty(B, n_out, dtype=dt, device=x.device)
    call('tfep_flip_invariant_embedding' + _sfx(dt), ptr(x), ldx, *head, ptr(out), max(n_out, 1), B, stream_of(x))
    return out


def flip_invariant_embedding_backward(x, embedded_indices, nonembedded_indices, vector_dim, parameters, grad_out,
                                      grads=None, gx=None):
    """VJP of ``flip_invariant_embedding`` for the cotangent ``grad_out`` (its first ``n_out`` columns; any row stride):
    ``(gx, grads)`` with ``grads`` the eight parameter gradients.  ``grads`` given: the call ADDS to them (the layer
    backward's batch chunks); ``gx`` given: written in place (contiguous, the shape of ``x``)."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    B, D = x.shape
    head, keep, n_out = _flip_head(x, embedded_indices, nonembedded_indices, vector_dim, parameters, dt)
    grad_out, ldg = rows(grad_out, 'grad_out', dt)
    if grad_out.shape[0] != B or grad_out.shape[1] < n_out:
        raise ValueError(f'flip_invariant_embedding_backward: grad_out must be ({B}, >= {n_out}), got {tuple(grad_out.shape)}')
    if gx is None:
        gx = torch.empty(B, D, dtype=dt, device=x.device)
    elif check_device_tensor(gx, 'gx', dt).shape != x.shape or not gx.is_contiguous():
        raise ValueError('flip_invariant_embedding_backward: gx must be a contiguous tensor of the shape of x')
    accumulate = grads is not None
    if accumulate:
        for g, p in zip(grads, keep[:8]):
            if check_device_tensor(g, 'grads', dt).shape != p.shape or not g.is_contiguous():
                raise ValueError('flip_invariant_embedding_backward: grads must be contiguous and shaped like the parameters')
    else:
        # (an empty batch launches nothing: its gradients are zeros, filled by a kernel -- see ``zeros``)
        grads = [(zeros if B == 0 else torch.empty)(*p.shape, dtype=dt, device=x.device) for p in keep[:8]]
    n_bytes = _lib.load().tfep_flip_invariant_embedding_backward_workspace_bytes(B, *head[1:2], *head[4:7])
    if n_bytes < 0:
        raise ValueError(_lib.load().tfep_last_error().decode())
    ws = torch.empty(max(n_bytes // 8, 1), dtype=torch.float64, device=x.device)
    call('tfep_flip_invariant_embedding_backward' + _sfx(dt), ptr(x), ldx, *head, ptr(grad_out), ldg, ptr(gx), max(D, 1),
         *(ptr(g) for g in grads), int(accumulate), ptr(ws), B, stream_of(x))
    return gx, list(grads)


# ----------------------------------------------------------------------------- frames of the Cartesian wrappers

def _selection(subset, weights, origin, dim, dt):
    """The centroid's selection as the frame kernels take it: ``(args, origin, keep)`` with ``args = (subset, n_subset,
    weights)`` as pointers and a count, ``origin`` the checked flat origin (None if none was given); the tensors of ``keep``
    live until the launch is queued."""
    keep = []
    n_sub = 0
    if subset is not None:
        subset = check_device_tensor(subset, 'subset', torch.int32).contiguous()
        n_sub = subset.numel()
        keep.append(subset)
    if weights is not None:
        weights = check_device_tensor(weights, 'weights', dt).reshape(-1).contiguous()
        keep.append(weights)
    if origin is not None:
        origin = check_device_tensor(origin, 'origin', dt).reshape(-1).contiguous()
        if origin.numel() != dim:
            raise ValueError(f'origin has {origin.numel()} entries, dim is {dim}')
        keep.append(origin)
    return (ptr(subset), n_sub, ptr(weights)), origin, keep


def _points(x, width, name):
    if x.shape[1] % width != 0:
        raise ValueError(f'{name} has {x.shape[1]} features, no multiple of {width}')
    return x.shape[1] // width


def _check_weights(weights, subset, n_points):
    n_sel = n_points if subset is None else subset.numel()
    if weights is not None and weights.numel() != n_sel:
        raise ValueError(f'weights has {weights.numel()} entries for {n_sel} points of the centroid')


def centroid_shift(x, subset, weights, origin, dim):
    """``(shift, y)``: ``shift = origin - centroid`` as (B, dim) and ``y = x + shift`` on every point
    (``tfep_centroid_shift``; reference flows/centroid.py).  ``subset``: int32 point indices or None (all points);
    ``weights``: normalised, one per selected point, or None.  float64 tensors run on the float64 kernels; mixed float32 /
    float64 arguments are a TypeError."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    B, dim = x.shape[0], int(dim)
    n = _points(x, max(dim, 1), 'x')
    _check_weights(weights, subset, n)
    sel, origin, keep = _selection(subset, weights, origin, dim, dt)
    shift = torch.empty(B, dim, dtype=dt, device=x.device)
    y = torch.empty(B, x.shape[1], dtype=dt, device=x.device)
    call('tfep_centroid_shift' + _sfx(dt), ptr(x), ldx, *sel, ptr(origin), dim, n, ptr(shift), ptr(y), max(x.shape[1], 1), B,
         stream_of(x))
    return shift, y


def centroid_shift_backward(grad_y, grad_shift, subset, weights, dim):
    """VJP of ``centroid_shift``: the cotangent of ``x``."""
    dt = _dtype(grad_y)
    gy, ldgy = rows(grad_y, 'grad_y', dt)
    B, dim = gy.shape[0], int(dim)
    n = _points(gy, max(dim, 1), 'grad_y')
    _check_weights(weights, subset, n)
    gs = None
    if grad_shift is not None:
        gs = check_device_tensor(grad_shift, 'grad_shift', dt).contiguous()
        if tuple(gs.shape) != (B, dim):
            raise ValueError(f'grad_shift must be ({B}, {dim}), got {tuple(gs.shape)}')
    sel, _, keep = _selection(subset, weights, None, dim, dt)
    gx = torch.empty(B, gy.shape[1], dtype=dt, device=gy.device)
    call('tfep_centroid_shift_backward' + _sfx(dt), *sel, dim, n, ptr(gy), ldgy, ptr(gs), ptr(gx), max(gy.shape[1], 1), B,
         stream_of(gy))
    return gx


def centroid_restore(y, shift, subset, weights, origin, fixed_point, fixed_entry, dim, translate_back):
    """``y`` with the fixed point placed where it restores the centroid (skipped for a one-point subset), minus ``shift``
    when ``translate_back`` (``tfep_centroid_restore``).  ``fixed_entry``: the fixed point's position in the selection;
    ``fixed_point``: the point itself."""
    dt = _dtype(y)
    y, ldy = rows(y, 'y', dt)
    B, dim = y.shape[0], int(dim)
    n = _points(y, max(dim, 1), 'y')
    _check_weights(weights, subset, n)
    shift = check_device_tensor(shift, 'shift', dt).contiguous()
    if tuple(shift.shape) != (B, dim):
        raise ValueError(f'shift must be ({B}, {dim}), got {tuple(shift.shape)}')
    sel, origin, keep = _selection(subset, weights, origin, dim, dt)
    out = torch.empty(B, y.shape[1], dtype=dt, device=y.device)
    call('tfep_centroid_restore' + _sfx(dt), ptr(y), ldy, ptr(shift), *sel, ptr(origin), int(fixed_point), int(fixed_entry),
         dim, n, int(bool(translate_back)), ptr(out), max(y.shape[1], 1), B, stream_of(y))
    return out


def centroid_restore_backward(grad_out, subset, weights, fixed_point, fixed_entry, dim, translate_back):
    """VJP of ``centroid_restore``: the cotangents ``(grad_y, grad_shift)``."""
    dt = _dtype(grad_out)
    g, ldg = rows(grad_out, 'grad_out', dt)
    B, dim = g.shape[0], int(dim)
    n = _points(g, max(dim, 1), 'grad_out')
    _check_weights(weights, subset, n)
    sel, _, keep = _selection(subset, weights, None, dim, dt)
    gy = torch.empty(B, g.shape[1], dtype=dt, device=g.device)
    gshift = torch.empty(B, dim, dtype=dt, device=g.device)
    call('tfep_centroid_restore_backward' + _sfx(dt), *sel, int(fixed_point), int(fixed_entry), dim, n,
         int(bool(translate_back)), ptr(g), ldg, ptr(gy), max(g.shape[1], 1), ptr(gshift), B, stream_of(g))
    return gy, gshift


def _frame(axis_point, plane_point, axis, plane_axis, normal, round_off):
    return (int(axis_point), int(plane_point), int(axis), int(plane_axis), int(normal), int(bool(round_off)))


def frame_orient(x, axis_point, plane_point, axis, plane_axis, normal, round_off):
    """``(y, R)``: every point of a row rotated into the frame that puts point ``axis_point`` on ``axis`` and point
    ``plane_point`` on the plane of ``axis`` and ``plane_axis`` (``tfep_frame_orient``; the rotation of
    ``utils.geometry.reference_frame_rotation_matrix(..., project_on_positive_axis=False)``), and that rotation as (B, 9).
    ``axis``, ``plane_axis``: 0..2; ``normal``: +-(1 + index of the third axis), signed like the plane normal.  ``round_off``
    writes exact zeros into the three constrained coordinates."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    B, n = x.shape[0], _points(x, 3, 'x')
    y = torch.empty(B, x.shape[1], dtype=dt, device=x.device)
    rot = torch.empty(B, 9, dtype=dt, device=x.device)
    call('tfep_frame_orient' + _sfx(dt), ptr(x), ldx, *_frame(axis_point, plane_point, axis, plane_axis, normal, round_off),
         ptr(y), max(x.shape[1], 1), ptr(rot), n, B, stream_of(x))
    return y, rot


def frame_orient_backward(x, grad_y, grad_rot, axis_point, plane_point, axis, plane_axis, normal, round_off):
    """VJP of ``frame_orient`` at ``x``: the cotangent of ``x`` from those of ``y`` and (optionally) of ``R``, including the
    dependence of ``R`` on the two defining points."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    gy, ldgy = rows(grad_y, 'grad_y', dt)
    B, n = x.shape[0], _points(x, 3, 'x')
    if gy.shape != x.shape:
        raise ValueError('frame_orient_backward: grad_y must have the shape of x')
    gr = None
    if grad_rot is not None:
        gr = check_device_tensor(grad_rot, 'grad_rot', dt).contiguous()
        if tuple(gr.shape) != (B, 9):
            raise ValueError(f'grad_rot must be ({B}, 9), got {tuple(gr.shape)}')
    gx = torch.empty(B, x.shape[1], dtype=dt, device=x.device)
    call('tfep_frame_orient_backward' + _sfx(dt), ptr(x), ldx,
         *_frame(axis_point, plane_point, axis, plane_axis, normal, round_off), ptr(gy), ldgy, ptr(gr), ptr(gx),
         max(x.shape[1], 1), n, B, stream_of(x))
    return gx


def _rotation(rot, B, dt):
    rot = check_device_tensor(rot, 'R', dt).contiguous()
    if tuple(rot.shape) != (B, 9):
        raise ValueError(f'R must be ({B}, 9), got {tuple(rot.shape)}')
    return rot


def frame_rotate(x, rot, transposed=False):
    """``y_i = x_i R`` on the points (row vectors) of every row, ``x_i R^T`` with ``transposed`` (``tfep_frame_rotate``):
    ``utils.geometry.batchwise_rotate(x, R, inverse=not transposed)``.  ``rot``: (B, 9)."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    B, n = x.shape[0], _points(x, 3, 'x')
    rot = _rotation(rot, B, dt)
    y = torch.empty(B, x.shape[1], dtype=dt, device=x.device)
    call('tfep_frame_rotate' + _sfx(dt), ptr(x), ldx, ptr(rot), int(bool(transposed)), ptr(y), max(x.shape[1], 1), n, B,
         stream_of(x))
    return y


def frame_rotate_backward(x, rot, grad_y, transposed=False):
    """VJP of ``frame_rotate``: the cotangents ``(grad_x, grad_R)``."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    gy, ldgy = rows(grad_y, 'grad_y', dt)
    B, n = x.shape[0], _points(x, 3, 'x')
    if gy.shape != x.shape:
        raise ValueError('frame_rotate_backward: grad_y must have the shape of x')
    rot = _rotation(rot, B, dt)
    gx = torch.empty(B, x.shape[1], dtype=dt, device=x.device)
    grot = torch.empty(B, 9, dtype=dt, device=x.device)
    call('tfep_frame_rotate_backward' + _sfx(dt), ptr(x), ldx, ptr(rot), int(bool(transposed)), ptr(gy), ldgy, ptr(gx),
         max(x.shape[1], 1), ptr(grot), n, B, stream_of(x))
    return gx, grot


# ----------------------------------------------------------------------------- internal coordinates, polar map

def _table_args(x, tables):
    """``(n_atoms, pointer / count arguments, counts)`` of prepared tables (``index_tables``) for the rows ``x``."""
    n = _points(x, 3, 'x')
    pairs, triples, quads, atom_start, atom_items = tables
    args, counts = [], []
    for t, (name, n_rows) in zip((pairs, triples, quads), _tables.TABLE_ROWS):
        check_device_tensor(t, name, torch.int32)
        if t.dim() != 2 or t.shape[0] != n_rows or not t.is_contiguous():
            raise ValueError(f'{name} must be a contiguous ({n_rows}, n) int32 table, got {tuple(t.shape)}')
        args += [ptr(t), t.shape[1]]
        counts.append(t.shape[1])
    check_device_tensor(atom_start, 'atom_start', torch.int32)
    check_device_tensor(atom_items, 'atom_items', torch.int32)
    if tuple(atom_start.shape) != (n + 1,) or atom_items.dim() != 1 or not atom_items.is_contiguous():
        raise ValueError(f'atom_start must be ({n + 1},) and atom_items 1-D: build both with ops.index_tables')
    return n, args, counts


def internal_coordinates(x, pairs, triples, quads, atom_start, atom_items):
    """``(d, a, t)``: distances over ``pairs``, angles at the middle atom over ``triples``, proper dihedrals over
    ``quads`` of the rows ``x`` (B, 3 n_atoms; any row stride), in one launch (``tfep_internal_coordinates``).  The five
    table tensors are those of ``index_tables``, which validates them.  float64 rows run on the float64 kernels."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    n, targs, counts = _table_args(x, (pairs, triples, quads, atom_start, atom_items))
    B = x.shape[0]
    d, a, t = (torch.empty(B, c, dtype=dt, device=x.device) for c in counts)
    call('tfep_internal_coordinates' + _sfx(dt), ptr(x), ldx, *targs, ptr(d), ptr(a), ptr(t), n, B, stream_of(x))
    return d, a, t


def internal_coordinates_backward(x, pairs, triples, quads, atom_start, atom_items, grad_d, grad_a, grad_t):
    """VJP of ``internal_coordinates`` at ``x``: the cotangent of ``x``, every coordinate written; an atom's
    contributions are summed in table order, so the result is reproducible bit for bit."""
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    n, targs, counts = _table_args(x, (pairs, triples, quads, atom_start, atom_items))
    B = x.shape[0]
    grads = []
    for g, c, name in zip((grad_d, grad_a, grad_t), counts, ('grad_d', 'grad_a', 'grad_t')):
        g = check_device_tensor(g, name, dt).contiguous()
        if tuple(g.shape) != (B, c):
            raise ValueError(f'{name} must be ({B}, {c}), got {tuple(g.shape)}')
        grads.append(g)
    gx = torch.empty(B, x.shape[1], dtype=dt, device=x.device)
    call('tfep_internal_coordinates_backward' + _sfx(dt), ptr(x), ldx, *targs, ptr(atom_start), ptr(atom_items),
         atom_items.numel(), *(ptr(g) for g in grads), ptr(gx), max(x.shape[1], 1), n, B, stream_of(x))
    return gx


def _polar_inputs(dt, *named):
    out = [check_device_tensor(t, name, dt).contiguous() for t, name in named]
    if any(t.shape != out[0].shape for t in out):
        raise ValueError('polar: ' + ', '.join(n for _, n in named) + ' must have one shape')
    return out


def polar(a, b, to_cartesian, with_log_det_J):
    """The polar map of the plane, element-wise (``tfep_polar``): ``(r, angle, log_det_J)`` of the Cartesian ``(a, b)``,
    or with ``to_cartesian`` ``(x, y, log_det_J)`` of the polar ``(a, b)``; the log-det is ``-log r`` / ``+log r`` as the
    reference returns it, and an empty tensor without ``with_log_det_J``."""
    dt = _dtype(a)
    a, b = _polar_inputs(dt, (a, 'a'), (b, 'b'))
    o0, o1 = torch.empty_like(a), torch.empty_like(a)
    ldj = torch.empty_like(a) if with_log_det_J else a.new_empty(0)
    call('tfep_polar' + _sfx(dt), ptr(a), ptr(b), int(bool(to_cartesian)), ptr(o0), ptr(o1),
         ptr(ldj) if with_log_det_J else None, a.numel(), stream_of(a))
    return o0, o1, ldj


def polar_backward(a, b, to_cartesian, grad_0, grad_1, grad_log_det_J):
    """VJP of ``polar``: the cotangents of ``(a, b)``; ``grad_log_det_J`` may be None."""
    dt = _dtype(a)
    named = [(a, 'a'), (b, 'b'), (grad_0, 'grad_0'), (grad_1, 'grad_1')]
    if grad_log_det_J is not None:
        named.append((grad_log_det_J, 'grad_log_det_J'))
    a, b, g0, g1, *gl = _polar_inputs(dt, *named)
    ga, gb = torch.empty_like(a), torch.empty_like(a)
    call('tfep_polar_backward' + _sfx(dt), ptr(a), ptr(b), int(bool(to_cartesian)), ptr(g0), ptr(g1),
         ptr(gl[0]) if gl else None, ptr(ga), ptr(gb), a.numel(), stream_of(a))
    return ga, gb


# ----------------------------------------------------------------------------- placement from a Z-matrix

def _zmatrix_args(tables, n_atoms=None):
    """The table arguments of the placement entry points, with the sizes ``(n_ic, n_fixed, n_atoms)``."""
    rows_, level_start, fixed, atom_start, atom_items = tables
    for t, name in zip(tables, ZMatrixTables._fields):
        check_device_tensor(t, name, torch.int32)
        if not t.is_contiguous():
            raise ValueError(f'{name} must be contiguous: build the tables with ops.zmatrix_tables')
    if rows_.dim() != 2 or rows_.shape[0] != 5 or level_start.dim() != 1 or level_start.numel() < 1 or fixed.dim() != 1:
        raise ValueError('rows must be (5, n_ic), level_start (n_levels + 1,) and fixed (n_fixed,): build them with '
                         'ops.zmatrix_tables')
    n_ic, n_fixed = rows_.shape[1], fixed.numel()
    n = n_ic + n_fixed
    if tuple(atom_start.shape) != (n + 1,) or atom_items.dim() != 1:
        raise ValueError(f'atom_start must be ({n + 1},) and atom_items 1-D: build both with ops.zmatrix_tables')
    args = [ptr(rows_), n_ic, ptr(level_start), level_start.numel() - 1, ptr(fixed), n_fixed]
    return args, n_ic, n_fixed, n


def _zmatrix_values(dt, B, n_ic, *named):
    """The (pointer, row stride) arguments of ``d, a, t``, and the tensors they point into (to be held until the launch)."""
    args, held = [], []
    for t, name in named:
        t, ld = rows(t, name, dt)
        if tuple(t.shape) != (B, n_ic):
            raise ValueError(f'{name} must be ({B}, {n_ic}), got {tuple(t.shape)}')
        args += [ptr(t), ld]
        held.append(t)
    return args, held


def zmatrix_place(d, a, t, x_fixed, rows_, level_start, fixed, atom_start, atom_items):
    """``(x, log_det_J)``: the positions (B, 3 n_atoms) of the rows placed from the internal coordinates ``d, a, t`` (B,
    n_ic; the caller's Z-matrix row order, any row stride) and the fixed atoms ``x_fixed`` (B, 3 n_fixed; any row stride),
    and the log-det (B,) of the map, in one launch (``tfep_zmatrix_place``).  The five table tensors are those of
    ``zmatrix_tables``, which validates them.  float64 rows run on the float64 kernels."""
    dt = _dtype(d)
    targs, n_ic, n_fixed, n = _zmatrix_args((rows_, level_start, fixed, atom_start, atom_items))
    x_fixed, ldf = rows(x_fixed, 'x_fixed', dt)
    B = x_fixed.shape[0]
    if x_fixed.shape[1] != 3 * n_fixed:
        raise ValueError(f'x_fixed must be ({B}, {3 * n_fixed}), got {tuple(x_fixed.shape)}')
    values, held = _zmatrix_values(dt, B, n_ic, (d, 'd'), (a, 'a'), (t, 't'))  # noqa: F841  (held: alive to the launch)
    x = torch.empty(B, 3 * n, dtype=dt, device=x_fixed.device)
    ldj = torch.empty(B, dtype=dt, device=x_fixed.device)
    call('tfep_zmatrix_place' + _sfx(dt), *values, ptr(x_fixed), ldf, *targs, ptr(x), max(3 * n, 1), ptr(ldj), n, B,
         stream_of(x_fixed))
    return x, ldj


def zmatrix_place_backward(x, d, a, t, rows_, level_start, fixed, atom_start, atom_items, grad_x, grad_log_det_J):
    """VJP of ``zmatrix_place`` at its output ``x``: the cotangents ``(g_d, g_a, g_t, g_x_fixed)`` in one launch; an atom's
    contributions are summed in table order, so the result is reproducible bit for bit."""
    dt = _dtype(x)
    targs, n_ic, n_fixed, n = _zmatrix_args((rows_, level_start, fixed, atom_start, atom_items))
    x, ldx = rows(x, 'x', dt)
    B = x.shape[0]
    grad_x, ldgx = rows(grad_x, 'grad_x', dt)
    if x.shape[1] != 3 * n or tuple(grad_x.shape) != tuple(x.shape):
        raise ValueError(f'x and grad_x must be ({B}, {3 * n}), got {tuple(x.shape)} and {tuple(grad_x.shape)}')
    gl = check_device_tensor(grad_log_det_J, 'grad_log_det_J', dt).contiguous()
    if tuple(gl.shape) != (B,):
        raise ValueError(f'grad_log_det_J must be ({B},), got {tuple(gl.shape)}')
    values, held = _zmatrix_values(dt, B, n_ic, (d, 'd'), (a, 'a'), (t, 't'))  # noqa: F841  (held: alive to the launch)
    gd, ga, gt = (torch.empty(B, n_ic, dtype=dt, device=x.device) for _ in range(3))
    g_fixed = torch.empty(B, 3 * n_fixed, dtype=dt, device=x.device)
    call('tfep_zmatrix_place_backward' + _sfx(dt), ptr(x), ldx, *values, *targs, ptr(atom_start), ptr(atom_items),
         atom_items.numel(), ptr(grad_x), ldgx, ptr(gl), ptr(gd), ptr(ga), ptr(gt), ptr(g_fixed), n, B, stream_of(x))
    return gd, ga, gt, g_fixed


# ----------------------------------------------------------------------------- the relative frame of mixed coordinates

def _remove_flags(remove):
    flags = tuple(int(bool(r)) for r in remove)
    if len(flags) != 3:
        raise ValueError(f'remove must hold 3 flags (origin, axis, plane), got {len(flags)}')
    return flags


def relative_frame_width(n_c, remove):
    """The number of coordinates ``relative_frame_encode`` makes of ``n_c`` atoms: ``d01, d02, a102n``, 3 for every atom
    that is no reference atom, and the reference DOFs that ``remove`` keeps (origin 3, axis 2, plane 1)."""
    ro, ra, rp = _remove_flags(remove)
    return 3 + 3 * (int(n_c) - 3) + 3 * (1 - ro) + 2 * (1 - ra) + (1 - rp)


def _relative_frame_atoms(x, name):
    n_c = _points(x, 3, name)
    if n_c < 3:
        raise ValueError(f'{name} holds {n_c} atoms: the relative frame needs the origin, axis and plane atoms (n_c >= 3)')
    return n_c


def _relative_frame_n_c(coords, remove):
    """The number of atoms behind a row of ``coords``; ValueError when the width disagrees with ``remove``."""
    extra = coords.shape[1] - relative_frame_width(3, remove)
    if extra < 0 or extra % 3 != 0:
        raise ValueError(f'coords has {coords.shape[1]} columns, which is not 3 + 3 (n_c - 3) + the kept reference DOFs '
                         f'({relative_frame_width(3, remove) - 3}) for remove={tuple(bool(r) for r in remove)}')
    return 3 + extra // 3


def _per_row(t, name, width, B, dt):
    t = check_device_tensor(t, name, dt).contiguous()
    if tuple(t.shape) != ((B, width) if width else (B,)):
        raise ValueError(f'{name} must be ({B}, {width}), got {tuple(t.shape)}' if width else
                         f'{name} must be ({B},), got {tuple(t.shape)}')
    return t


def relative_frame_encode(x_cart, remove):
    """``(coords, origin, R, log_det_J)``: the atoms of the rows ``x_cart`` (B, 3 n_c; any row stride), whose LAST THREE are
    the origin, axis and plane atoms, in the frame of those three (``tfep_relative_frame_encode``; csrc/relframe.h).
    ``coords`` (B, ``relative_frame_width(n_c, remove)``), ``origin`` (B, 3), ``R`` (B, 9), ``log_det_J`` (B,).  float64 rows
    run on the float64 kernels."""
    dt = _dtype(x_cart)
    x, ldx = rows(x_cart, 'x_cart', dt)
    B, n_c, remove = x.shape[0], _relative_frame_atoms(x, 'x_cart'), _remove_flags(remove)
    width = relative_frame_width(n_c, remove)
    coords = torch.empty(B, width, dtype=dt, device=x.device)
    origin, rot, ldj = (torch.empty(B, *s, dtype=dt, device=x.device) for s in ((3,), (9,), ()))
    call('tfep_relative_frame_encode' + _sfx(dt), ptr(x), ldx, n_c, *remove, ptr(coords), width, ptr(origin), ptr(rot),
         ptr(ldj), B, stream_of(x))
    return coords, origin, rot, ldj


def relative_frame_encode_backward(x_cart, remove, grad_coords, grad_origin, grad_rot, grad_log_det_J):
    """VJP of ``relative_frame_encode`` at ``x_cart``: the cotangent of ``x_cart`` from those of the four outputs,
    including the dependence of ``R`` and ``origin`` on the reference atoms."""
    dt = _dtype(x_cart)
    x, ldx = rows(x_cart, 'x_cart', dt)
    B, n_c, remove = x.shape[0], _relative_frame_atoms(x, 'x_cart'), _remove_flags(remove)
    gc, ldgc = rows(grad_coords, 'grad_coords', dt)
    if tuple(gc.shape) != (B, relative_frame_width(n_c, remove)):
        raise ValueError(f'grad_coords must be ({B}, {relative_frame_width(n_c, remove)}), got {tuple(gc.shape)}')
    go, gr, gl = (_per_row(grad_origin, 'grad_origin', 3, B, dt), _per_row(grad_rot, 'grad_rot', 9, B, dt),
                  _per_row(grad_log_det_J, 'grad_log_det_J', 0, B, dt))
    gx = torch.empty(B, 3 * n_c, dtype=dt, device=x.device)
    call('tfep_relative_frame_encode_backward' + _sfx(dt), ptr(x), ldx, n_c, *remove, ptr(gc), ldgc, ptr(go), ptr(gr),
         ptr(gl), ptr(gx), 3 * n_c, B, stream_of(x))
    return gx


def relative_frame_decode(coords, origin, rot, remove):
    """``(x_cart, log_det_J)``: the inverse of ``relative_frame_encode`` (``tfep_relative_frame_decode``) from ``coords`` (B,
    W; any row stride), ``origin`` (B, 3) and ``R`` (B, 9).  A removed reference DOF is exactly 0 in the frame, a kept one is
    read from ``coords``.  A width that disagrees with ``remove`` is a ValueError."""
    dt = _dtype(coords)
    c, ldc = rows(coords, 'coords', dt)
    B, remove = c.shape[0], _remove_flags(remove)
    n_c = _relative_frame_n_c(c, remove)
    origin, rot = _per_row(origin, 'origin', 3, B, dt), _per_row(rot, 'R', 9, B, dt)
    x = torch.empty(B, 3 * n_c, dtype=dt, device=c.device)
    ldj = torch.empty(B, dtype=dt, device=c.device)
    call('tfep_relative_frame_decode' + _sfx(dt), ptr(c), ldc, ptr(origin), ptr(rot), n_c, *remove, ptr(x), 3 * n_c,
         ptr(ldj), B, stream_of(c))
    return x, ldj


def relative_frame_decode_backward(coords, origin, rot, remove, grad_x_cart, grad_log_det_J):
    """VJP of ``relative_frame_decode``: the cotangents ``(g_coords, g_origin, g_R)``."""
    dt = _dtype(coords)
    c, ldc = rows(coords, 'coords', dt)
    B, remove = c.shape[0], _remove_flags(remove)
    n_c = _relative_frame_n_c(c, remove)
    origin, rot = _per_row(origin, 'origin', 3, B, dt), _per_row(rot, 'R', 9, B, dt)
    gx, ldgx = rows(grad_x_cart, 'grad_x_cart', dt)
    if tuple(gx.shape) != (B, 3 * n_c):
        raise ValueError(f'grad_x_cart must be ({B}, {3 * n_c}), got {tuple(gx.shape)}')
    gl = _per_row(grad_log_det_J, 'grad_log_det_J', 0, B, dt)
    gc = torch.empty(B, c.shape[1], dtype=dt, device=c.device)
    go, gr = torch.empty(B, 3, dtype=dt, device=c.device), torch.empty(B, 9, dtype=dt, device=c.device)
    call('tfep_relative_frame_decode_backward' + _sfx(dt), ptr(c), ldc, ptr(origin), ptr(rot), n_c, *remove, ptr(gx), ldgx,
         ptr(gl), ptr(gc), c.shape[1], ptr(go), ptr(gr), B, stream_of(c))
    return gc, go, gr


def gather_columns(src, idx):
    dt = _dtype(src)
    src, lds = rows(src, 'src', dt)
    B, n = src.shape[0], idx.numel()
    dst = torch.empty(B, n, dtype=src.dtype, device=src.device)
    call('tfep_gather_columns' + _sfx(dt), ptr(src), lds, ptr(idx), n, ptr(dst), n, B, stream_of(src))
    return dst


def scatter_columns(src, idx, dst):
    """dst[:, idx[j]] = src[:, j] (in place on ``dst``, which the caller owns)."""
    dt = _dtype(src)
    src, lds = rows(src, 'src', dt)
    B, n = src.shape[0], idx.numel()
    if not dst.is_contiguous():
        raise ValueError('dst must be contiguous')
    if torch.float64 in (dt, dst.dtype):
        check_device_tensor(dst, 'dst', dt)
    call('tfep_scatter_columns' + _sfx(dt), ptr(src), lds, ptr(idx), n, ptr(dst), dst.shape[1], B, stream_of(src))
    return dst


# ----------------------------------------------------------------------------- masked linear

_TILES = {}


def tile_sizes():
    if 'wide' not in _TILES:                    # (constants of the library: asked once, not on every launch)
        lib = _lib.load()
        _TILES['wide'] = (lib.tfep_masked_linear_tile_m(), lib.tfep_masked_linear_tile_n(), lib.tfep_masked_linear_tile_k())
    return _TILES['wide']


def round_up(n, m):
    return (n + m - 1) // m * m


def pad_columns(x, k_padded, dtype=torch.float32):
    """Return ``x`` as a (B, k_padded) buffer with zero padding (GEMM operand contract).  ``dtype``: what ``x`` must be
    (float32, or float64 for the float64 GEMM)."""
    x, _ = rows(x, 'x', dtype)
    B, K = x.shape
    if K == k_padded and x.stride(0) == K and x.data_ptr() % 16 == 0:
        return x
    out = zeros(B, k_padded, dtype=x.dtype, device=x.device)
    out[:, :K] = x
    return out


def masked_weight_prepare(weight_v, weight_g=None, mask=None, row_of_out=None, col_of_in=None,
                          n_rows_padded=None, k_padded=None, out=None, col_cut=None, clear=True, in_of_col=None):
    """Effective masked weight, permuted + zero padded (reference masked.py:369-371, :433-439, :270).  ``col_cut``:
    prefix mask rows (see ``masked_weight_prepare_split``); ``clear=False``: ``out`` was zeroed once and always holds the
    same layer, so its padding needs no clearing.  With ``col_cut``, ``clear=False`` and ``in_of_col`` (the inverse of
    ``col_of_in``) long rows take the LDS-staged prefix kernel, which writes only the live prefix of each packed row.
    float64 parameters take ``tfep_masked_weight_prepare_f64``, which has no prefix form: ``col_cut`` is a ValueError."""
    dt = _dtype(weight_v)
    if dt == _F64 and col_cut is not None:
        raise ValueError('masked_weight_prepare: the prefix-mask form (col_cut) is float32-only')
    check_device_tensor(weight_v, 'weight', dt)
    N, K = weight_v.shape
    tk = tile_sizes()[2]
    n_rows_padded = N if n_rows_padded is None else n_rows_padded
    k_padded = round_up(K, tk) if k_padded is None else k_padded
    if out is None:
        out = torch.empty(n_rows_padded, k_padded, dtype=dt, device=weight_v.device)
    check_device_tensor(out, 'out', dt)
    # (contiguous copies live in locals until the launch is queued; a temporary freed inside the argument list could be
    # overwritten by the next one)
    v_c = weight_v.contiguous()
    g_c = None if weight_g is None else check_device_tensor(weight_g, 'weight_g', dt).contiguous()
    m_c = _mask(mask, dt)
    if dt == _F64:
        call('tfep_masked_weight_prepare_f64', ptr(v_c), ptr(g_c), ptr(m_c), N, K, ptr(row_of_out), ptr(col_of_in),
             int(bool(clear)), ptr(out), n_rows_padded, out.shape[1], stream_of(weight_v))
        return out
    if col_cut is not None and not clear and (in_of_col is not None or col_of_in is None) and 8192 <= K <= 16384 and \
            out.shape[1] % 4 == 0 and out.shape[1] >= round_up(K, 8) and os.environ.get('TFEP_PACK_LDS', '1') != '0':
        call('tfep_masked_weight_prepare_prefix', ptr(v_c), ptr(g_c), N, K, ptr(row_of_out), ptr(in_of_col), ptr(col_cut),
             ptr(out), n_rows_padded, out.shape[1], stream_of(weight_v))
        return out
    call('tfep_masked_weight_prepare', ptr(v_c), ptr(g_c), ptr(m_c), N, K, ptr(row_of_out), ptr(col_of_in), ptr(col_cut),
         int(bool(clear)), ptr(out), n_rows_padded, k_padded, stream_of(weight_v))
    return out


def mask_k_ranges(mask, tile_n, n_tiles, k_padded, row_of_out=None, col_of_in=None):
    dt = _dtype(mask)
    check_device_tensor(mask, 'mask', dt)
    N, K = mask.shape
    out = torch.empty(n_tiles, 2, dtype=torch.int32, device=mask.device)
    m_c = mask.contiguous()
    call('tfep_mask_k_ranges' + _sfx(dt), ptr(m_c), N, K, ptr(row_of_out), ptr(col_of_in), tile_n,
         tile_sizes()[2], n_tiles, k_padded, ptr(out), stream_of(mask))
    return out


def heavy_first_order(k_ranges):
    """Column tiles sorted by descending k-range length (host-side, once per mask)."""
    kr = k_ranges.cpu().long()
    order = torch.argsort(kr[:, 1] - kr[:, 0], descending=True, stable=True)
    return order.to(device=k_ranges.device, dtype=torch.int32)


def xcd_balanced_tile_list(live, n_xcd=8, group=32):
    """Launch order of the live output tiles of a block-sparse product (``tile_list`` of ``tfep_gemm_desc``).

    ``live``: (row tiles, column tiles) bool / uint8 CPU tensor.  Workgroup ids go round-robin to the 8 XCDs and each XCD
    works through its own share, so the live tiles are listed in the order of the 8 x 4 super-tile walk (neighbours share
    operand panels in the XCD's L2), cut into groups of 32, and group k is placed at the positions of XCD k % 8: every XCD
    gets the same number of tiles whatever the shape of the live region.  Returns an int32 (n_positions, 2) CPU tensor,
    -1 = no tile."""
    live = torch.as_tensor(live).cpu().bool()
    mt, nt = torch.nonzero(live, as_tuple=True)
    # order of the 8 x 4 super-tile walk: column super-tile, row super-tile, then column-major inside the super-tile
    key = (((nt // 4) * ((live.shape[0] + 7) // 8) + mt // 8) * 4 + nt % 4) * 8 + mt % 8
    order = torch.argsort(key)
    mt, nt = mt[order], nt[order]
    n = mt.numel()
    n_groups = (n + group - 1) // group
    n_rounds = max(1, (n_groups + n_xcd - 1) // n_xcd)
    out = torch.full((n_rounds * group * n_xcd, 2), -1, dtype=torch.int32)
    i = torch.arange(n)
    k, w = i // group, i % group
    pos = ((k // n_xcd) * group + w) * n_xcd + k % n_xcd
    out[pos, 0], out[pos, 1] = mt.to(torch.int32), nt.to(torch.int32)
    return out


def split_wide_tile_n():
    """Widest column tile of the split-f16 kernel's plain linear product (400)."""
    if 'xwide' not in _TILES:
        _TILES['xwide'] = _lib.load().tfep_split_wide_tile_n()
    return _TILES['xwide']


def narrow_tile_n():
    if 'narrow' not in _TILES:
        _TILES['narrow'] = _lib.load().tfep_masked_linear_narrow_tile_n()
    return _TILES['narrow']


def few_wide_tiles(B, N):
    """True when a (B x N) product is at most 128 of the 256 x 256 tiles, half the CUs (and more than one 32-column tile wide):
    one workgroup per wide tile then leaves CUs idle and the run time is one workgroup's walk over k, see
    ``masked_linear_packed``.  Measured (tools/probe/tile_choice.py, exact-fp32 kernels, dense): B 1024 x K 800 x N 800
    (16 wide tiles) 214 us wide / 42 us narrow; 4096 x 800 x 800 (64) 221 / 73; 8192 x 800 x 800 (128) 227 / 119;
    4096 x 800 x 3200 (208) 236 / 207."""
    tm, tn, _ = tile_sizes()
    # (the narrow tile runs dense -- the mask tables are per wide tile -- so at ~200 tiles, where the two are level on a
    # dense product, the wide tile with its k-ranges wins: the line is drawn at half the CUs)
    return ((B + tm - 1) // tm) * ((N + tn - 1) // tn) <= 128 and N > narrow_tile_n()


def masked_linear_packed(x_padded, w_packed, bias, n_out, k_ranges=None, col_map=None, act=0, out=None,
                         out_cols=None, tile_order=None):
    """y = act(x W^T + b) on packed operands (reference masked.py:265-277 + made.py:320).  Small products (cfg1-sized
    layers: a handful of 256 x 256 tiles) run on the 32-column tile instead, dense: more workgroups, shorter chains."""
    if x_padded.dtype == torch.float64:
        if col_map is not None:
            raise ValueError('masked_linear_packed: col_map is float32-only')
        # (tile_order only orders the launch of the float32 kernel; the float64 kernel's tiles all take similar time)
        return masked_linear_f64(x_padded, w_packed, bias, n_out, k_ranges=k_ranges, act=act, out=out, out_cols=out_cols)
    B = x_padded.shape[0]
    n_rows_w, k_padded = w_packed.shape
    if out is None:
        out = torch.empty(B, n_out if out_cols is None else out_cols, dtype=torch.float32, device=x_padded.device)
    tile_n = 0
    if col_map is None and few_wide_tiles(B, n_out):
        tile_n, k_ranges, tile_order = narrow_tile_n(), None, None      # (the mask tables are per 256-column tile)
    call('tfep_masked_linear_forward', ptr(x_padded), x_padded.shape[1], ptr(w_packed), k_padded,
         ptr(bias), ptr(k_ranges), ptr(tile_order), ptr(col_map), ptr(out), out.shape[1], B, n_out, n_rows_w,
         k_padded, int(act), tile_n,
         stream_of(x_padded))
    return out


def gemm_slice(x_padded, w_packed, row0, n_rows, bias, k_ranges, kr_offset, out, col0, act):
    """Row slice of a packed masked linear layer with the narrow column tile:
    ``out[:, col0:col0+n_rows] = act(x W[row0:row0+n_rows]^T + bias[row0:row0+n_rows])``.
    ``k_ranges[kr_offset:]`` holds the [k_begin, k_end) of the slice's 32-row tiles."""
    B = x_padded.shape[0]
    k_padded = w_packed.shape[1]
    esz = 4
    call('tfep_masked_linear_forward', ptr(x_padded), x_padded.shape[1],
         ctypes.c_void_p(w_packed.data_ptr() + row0 * k_padded * esz), k_padded,
         ctypes.c_void_p(bias.data_ptr() + row0 * esz),
         ctypes.c_void_p(k_ranges.data_ptr() + kr_offset * 2 * 4), None, None,
         ctypes.c_void_p(out.data_ptr() + col0 * esz), out.shape[1], B, n_rows, n_rows, k_padded, int(act),
         _lib.load().tfep_masked_linear_narrow_tile_n(), stream_of(x_padded))


# ----------------------------------------------------------------------------- float64 masked linear

def masked_linear_f64(x_padded, w_packed, bias, n_out, k_ranges=None, act=0, accumulate=0, elu_grad_of=None, out=None,
                      out_cols=None, kr_tile_n=None):
    """``y (+)= act(x W^T + b) [* elu'(elu_grad_of)]`` on packed float64 operands, every product on the fp64-MFMA GEMM
    (``tfep_masked_linear_gemm_f64``).  ``k_ranges``: per tile of ``kr_tile_n`` rows of ``w_packed`` (default: the wide
    tile, 256; any multiple of 128), as ``mask_k_ranges(mask, kr_tile_n, ...)`` makes them -- a table of another
    granularity is an error, not a silently wrong range."""
    if kr_tile_n is None:
        kr_tile_n = tile_sizes()[1]
    if k_ranges is not None and tuple(k_ranges.shape) != ((n_out + kr_tile_n - 1) // kr_tile_n, 2):
        raise ValueError(f'masked_linear_f64: k_ranges has shape {tuple(k_ranges.shape)}, expected '
                         f'({(n_out + kr_tile_n - 1) // kr_tile_n}, 2) for {n_out} outputs in tiles of {kr_tile_n}')
    _f64(x_padded, 'x')
    _f64(w_packed, 'weight')
    _f64(bias, 'bias')
    _f64(elu_grad_of, 'elu_grad_of')
    B = x_padded.shape[0]
    n_rows_w, k_padded = w_packed.shape
    if out is None:
        out = torch.empty(B, n_out if out_cols is None else out_cols, dtype=_F64, device=x_padded.device)
    _f64(out, 'out')
    call('tfep_masked_linear_gemm_f64', ptr(x_padded), x_padded.stride(0) if B > 1 else x_padded.shape[1], ptr(w_packed),
         k_padded, ptr(bias), ptr(k_ranges), int(kr_tile_n), ptr(out), out.shape[1], B, n_out, n_rows_w, k_padded, int(act),
         int(accumulate), ptr(elu_grad_of), 0 if elu_grad_of is None else elu_grad_of.shape[1], stream_of(x_padded))
    return out


def masked_k_ranges_f64(mask, n_pad, k_pad):
    """k-ranges (per wide tile) of a float64 layer's mask for ``masked_linear_f64``, or None without a mask.  Each range
    bounds the non-zero columns of its 256 rows: a degree-sorted (block-triangular) mask skips its zero k-tiles, any
    other mask is still exact (the range then covers whatever its rows touch)."""
    if mask is None:
        return None
    tn = tile_sizes()[1]
    return mask_k_ranges(_mask(mask, _F64), tn, (n_pad + tn - 1) // tn, k_pad)


# ----------------------------------------------------------------------------- one masked linear layer, forward and backward

def gemm(x, w, y, B, N, n_rows_w, bias=None, k_ranges=None, act=0, accumulate=0, elu_grad_of=None, tile_live=None,
         split=False, w_split=None, x_split=None, tile_list=None, tile_n=0):
    """``y (+)= act(x w^T + bias) [* elu'(elu_grad_of)]`` on packed float32 operands (``tfep_masked_linear_gemm``): the
    product of the backward pass, with nothing checked or copied on the way.  ``split``: run on split-f16 operands (x
    converted here with one scale per row; ``w_split`` / ``x_split`` = already converted ``(rows, inv_scale)`` of w / x,
    else w is converted here with one scale for the matrix)."""
    d = _lib.GemmDesc()
    if split:
        xs, x_inv = x_split if x_split is not None else split_rows(x, x.shape[1])
        ws, w_inv = w_split if w_split is not None else split_rows(w, w.shape[1], per_tensor=True)
        d.split, d.x_inv_scale, d.w_inv_scale = 1, x_inv.data_ptr(), w_inv.data_ptr()
        x, w = xs, ws
    d.x, d.ldx = x.data_ptr(), x.shape[1]
    d.w, d.ldw = w.data_ptr(), w.shape[1]
    d.bias = bias.data_ptr() if bias is not None else None
    d.k_ranges = k_ranges.data_ptr() if k_ranges is not None else None
    d.tile_order, d.col_map = None, None
    d.y, d.ldy = y.data_ptr(), y.shape[1]
    d.B, d.N, d.n_rows_w, d.k_padded, d.act, d.accumulate = B, N, n_rows_w, w.shape[1], act, accumulate
    if elu_grad_of is not None:
        d.elu_grad_of, d.ld_elu_grad_of = elu_grad_of.data_ptr(), elu_grad_of.shape[1]
    d.tile_live = tile_live.data_ptr() if tile_live is not None else None
    if tile_list is not None:
        d.tile_list, d.n_tile_list = tile_list.data_ptr(), tile_list.shape[0]
    d.tile_n = tile_n                  # (0 = the default 256 columns; the tables above count tiles of this width)
    if not split and few_wide_tiles(B, N):
        # a cfg1-sized product is one or two 256 x 256 tiles: one workgroup walks the whole k range while 255 CUs idle
        # (130 us for a 224 x 224 x 1024 grad_weight).  The 32-column tile spreads it over the columns; the mask tables are
        # per 256-column tile and only save work (masked weights are zeros, masked gradients are dropped later): dense.
        d.tile_n, d.k_ranges, d.tile_live = narrow_tile_n(), None, None
        d.tile_list, d.n_tile_list = None, 0
    call('tfep_masked_linear_gemm', ctypes.byref(d), stream_of(x))
    return y


def transpose(src, n_rows, n_cols, out):
    """out (cols_pad x rows_pad, zero filled by the caller) <- src[:n_rows, :n_cols]^T (``tfep_transpose[_f64]``)."""
    dt = _dtype(src)
    check_device_tensor(src, 'src', dt)
    check_device_tensor(out, 'out', dt)
    call('tfep_transpose' + _sfx(dt), ptr(src), src.shape[1], n_rows, n_cols, ptr(out), out.shape[1], stream_of(src))
    return out


def column_sums(x, n_rows, n_cols, out=None, accumulate=0):
    """out[c] (+)= sum_{r < n_rows} x[r, c] for c < n_cols (``tfep_column_sums[_f64]``)."""
    dt = _dtype(x)
    check_device_tensor(x, 'x', dt)
    if out is None:
        out = torch.empty(n_cols, dtype=dt, device=x.device)
    check_device_tensor(out, 'out', dt)
    call('tfep_column_sums' + _sfx(dt), ptr(x), x.shape[1], n_rows, n_cols, ptr(out), int(accumulate), stream_of(x))
    return out


def weight_norm_backward(gw_packed, weight_v, weight_g=None, mask=None, row_of_out=None, col_of_in=None):
    """``(grad_v, grad_g)`` of the masked (weight-normalised) parametrisation from the gradient of the packed weight
    (``tfep_weight_norm_backward[_f64]``); ``grad_g`` is None without weight norm."""
    dt = _dtype(weight_v)
    check_device_tensor(gw_packed, 'gw_packed', dt)
    check_device_tensor(weight_v, 'weight', dt)
    N, K = weight_v.shape
    v_c = weight_v.contiguous()
    g_c = None if weight_g is None else check_device_tensor(weight_g, 'weight_g', dt).contiguous()
    m_c = _mask(mask, dt)
    grad_v = torch.empty(N, K, dtype=dt, device=weight_v.device)
    grad_g = None if weight_g is None else torch.empty(weight_g.shape, dtype=dt, device=weight_v.device)
    call('tfep_weight_norm_backward' + _sfx(dt), ptr(gw_packed), gw_packed.shape[1], ptr(v_c), ptr(g_c), ptr(m_c), N, K,
         ptr(row_of_out), ptr(col_of_in), ptr(grad_v), ptr(grad_g), stream_of(weight_v))
    return grad_v, grad_g


def masked_linear_operands(x2, weight, weight_g, mask):
    """``(x_padded, w_packed)``: the input and the effective weight ``M o W`` (``W = g v/||v||`` with ``weight_g``) of one
    masked linear layer, zero padded to whole k-tiles as the GEMMs take them.  ``x2`` (2-D) must be of the parameters'
    dtype."""
    n_out, k = weight.shape
    tk = tile_sizes()[2]
    k_pad, n_pad = round_up(k, tk), round_up(n_out, tk)
    w = masked_weight_prepare(weight, weight_g, mask, n_rows_padded=n_pad, k_padded=k_pad)
    return pad_columns(x2, k_pad, _dtype(weight)), w


def masked_linear_layer(x2, weight, weight_g, mask, bias):
    """One masked linear layer from its parameters: ``(y, x_padded, w_packed)`` with ``y = x2 (M o W)^T + b`` (reference
    masked.py:265-277, :351-404) and the packed operands of the product, which ``masked_linear_layer_backward`` takes.
    float32 parameters run on the fp32-MFMA GEMM, float64 ones on the fp64-MFMA GEMM with the k-ranges of the mask."""
    xp, w = masked_linear_operands(x2, weight, weight_g, mask)
    n_out, (n_pad, k_pad) = weight.shape[0], w.shape
    if xp.dtype == _F64:
        y = masked_linear_f64(xp, w, bias, n_out, k_ranges=masked_k_ranges_f64(mask, n_pad, k_pad))
    else:
        y = masked_linear_packed(xp, w, bias, n_out)
    return y, xp, w


def _plain_product(x, w, out, accumulate=0):
    """``out (+)= x w^T`` on packed operands of either dtype, every column of ``out``."""
    if x.dtype == _F64:
        return masked_linear_f64(x, w, None, out.shape[1], accumulate=accumulate, out=out)
    return gemm(x, w, out, x.shape[0], out.shape[1], out.shape[1], accumulate=accumulate)


def masked_linear_layer_backward(grad_output, x_padded, w_packed, weight, weight_g, mask, n_out, k, want_input=True,
                                 want_weight=True, want_bias=True):
    """The analytic backward of ``masked_linear_layer`` (reference masked.py:220-302, :351-404) from its packed operands:
    ``(grad_input (B, k), grad_v, grad_g, grad_bias)``, None where not wanted (``grad_g`` also without weight norm).  Every
    product runs on the MFMA GEMM of the parameters' dtype: ``grad_input = g W`` and ``grad_W = g^T x`` (operands transposed
    so that both stay K-contiguous).  A float32 layer converts a ``grad_output`` of another dtype; for a float64 layer it is a
    TypeError."""
    dt = _dtype(weight)
    n_pad, k_pad = w_packed.shape
    tk = tile_sizes()[2]
    kw = dict(dtype=dt, device=x_padded.device)
    g2 = grad_output.reshape(-1, n_out)
    if dt != _F64:
        g2 = g2.float()
    B = g2.shape[0]
    gp = pad_columns(g2, n_pad, dt)
    grad_input = grad_v = grad_g = grad_bias = None
    if want_input:
        wt = transpose(w_packed, n_pad, k_pad, zeros(k_pad, n_pad, **kw))
        grad_input = _plain_product(gp, wt, torch.empty(B, k_pad, **kw))[:, :k]
    if want_weight:
        Bp = round_up(max(B, 1), tk)
        gT = transpose(gp, B, n_pad, zeros(n_pad, Bp, **kw))
        xT = transpose(x_padded, B, k_pad, zeros(k_pad, Bp, **kw))
        # float32 adds the product to a cleared buffer, float64 writes it: ``0 + s`` and ``s`` differ in the sign of a zero
        # sum, and each dtype keeps the bits it has always given
        add = int(dt != _F64)
        gw = _plain_product(gT, xT, (zeros if add else torch.empty)(n_pad, k_pad, **kw), accumulate=add)
        grad_v, grad_g = weight_norm_backward(gw, weight, weight_g, mask)
    if want_bias:
        grad_bias = column_sums(gp, B, n_out)
    return grad_input, grad_v, grad_g, grad_bias


def diag_mfma_f64_peak(blocks, iters, device=None):
    """Run the register-only f64 MFMA loop (``tfep_diag_mfma_f64_peak``); returns its flop count."""
    scratch = torch.empty(blocks * 256, dtype=_F64, device=device)
    call('tfep_diag_mfma_f64_peak', ptr(scratch), int(blocks), int(iters), stream_of(scratch))
    return blocks * 4 * iters * 64 * 2048


# ----------------------------------------------------------------------------- split-precision operands

def split_gemm_enabled():
    """The MADE GEMMs of the forward pass run on split-f16 operands (3 fp16 MFMAs per fp32 product, fp32-equivalent
    results) unless ``TFEP_SPLIT_GEMM=0`` selects the exact-fp32 MFMA kernel."""
    return os.environ.get('TFEP_SPLIT_GEMM', '1') != '0'


def split_rows(x, cols_padded, per_tensor=False, out=None, inv_scale=None):
    """fp32 rows -> split-f16 rows (``tfep_split_rows``).  Returns ``(split, inv_scale)``: ``split`` is a
    (rows, cols_padded) float32-TYPED container of the bit pattern, ``inv_scale`` has one entry per row, or
    [1/scale, scratch] with ``per_tensor``."""
    x, ldx = rows(x, 'x')
    R, C = x.shape
    if out is None:
        out = torch.empty(R, cols_padded, dtype=torch.float32, device=x.device)
    if inv_scale is None:
        inv_scale = torch.empty(2 if per_tensor else max(R, 1), dtype=torch.float32, device=x.device)
    call('tfep_split_rows', ptr(x), ldx, R, C, ptr(out), out.shape[1], cols_padded, ptr(inv_scale), int(per_tensor),
         stream_of(x))
    return out, inv_scale


def zeros(*shape, dtype=torch.float32, device=None):
    """``torch.zeros`` as a fill KERNEL.  ``torch.zeros`` clears with ``hipMemsetAsync``; captured in a HIP graph that becomes
    a memset node, and memset nodes were seen to leave garbage behind on replay (ROCm 7.0 / MI355X: the padding of a packed
    weight buffer cleared by ``hipMemsetAsync`` read back as ~1e36 by a later kernel of the same graph while eager runs
    were clean -- the replayed blocked inverse differed from the eager one from the second block on; earlier, a 4-byte
    memset was corrupted by a second capture).  Everything on a capturable path clears its buffers with kernels."""
    return torch.full(tuple(shape), 0.0, dtype=dtype, device=device)


def split_columns_scaled(x, col0, cols, out, inv_scale):
    """Columns ``[col0, col0 + cols)`` (whole groups of 8; ``col0 % 8 == 0``) of the fp32 rows ``x`` into the same columns
    of the split rows ``out``, with the caller's per-row ``inv_scale`` (powers of two): for operands filled incrementally
    (``tfep_split_columns_scaled``)."""
    x, ldx = rows(x, 'x')
    call('tfep_split_columns_scaled', ptr(x), ldx, x.shape[0], int(col0), int(cols), ptr(out), out.shape[1], ptr(inv_scale),
         stream_of(x))
    return out


def column_absmax(x):
    """``max_r |x[r, c]|`` per column of a 2-D tensor as a (1, cols) float32 tensor (``tfep_column_absmax``; NaN survives)."""
    x, ldx = rows(x, 'x')
    out = torch.empty(1, x.shape[1], dtype=torch.float32, device=x.device)
    call('tfep_column_absmax', ptr(x), ldx, x.shape[0], x.shape[1], ptr(out), stream_of(x))
    return out


def range_flag(tensors, bits=19):
    """Number of rows, over the 2-D fp32 ``tensors``, whose own dynamic range exceeds what the split-f16 operand format
    carries at fp32 accuracy (a non-zero element below ``2^-bits`` of the row maximum, or a non-finite element):
    ``range_flag_device`` read back once (ONE host synchronisation for the whole list)."""
    c = range_flag_device(tensors, bits)
    return 0 if c is None else int(c.item())


def range_flag_device(tensors, bits=19, count=None):
    """``tfep_range_flag`` on every tensor into one device counter (int32, 1 element), a new one or ``count`` added to, and
    no read-back: capturable in a HIP graph (a new counter is cleared by a fill kernel, see ``zeros``).  ``count`` itself
    (None for a new one) when there is nothing to check."""
    tensors = [t for t in tensors if t is not None and t.numel() > 0]
    if not tensors:
        return count
    if count is None:
        count = zeros(1, dtype=torch.int32, device=tensors[0].device)
    for t in tensors:
        check_device_tensor(t, 'range_flag input')
        if t.dim() != 2 or t.stride(1) != 1:
            t = t.reshape(t.shape[0], -1).contiguous() if t.dim() > 1 else t.reshape(1, -1).contiguous()
        call('tfep_range_flag', ptr(t), t.stride(0) if t.shape[0] > 1 else t.shape[1], t.shape[0], t.shape[1], int(bits),
             ptr(count), stream_of(t))
    return count


def abs_reduce(x, what):
    """``what='row_max'``: max_k |x[row, k]| per row;  ``'max_row_sum'``: max_row sum_k |x[row, k]| as a 1-element tensor
    (``tfep_abs_reduce``: plain kernels, capturable in a HIP graph, unlike torch's multi-block reductions whose semaphores are
    cleared with a small memset)."""
    x, ldx = rows(x, 'x')
    mode = {'row_max': 0, 'max_row_sum': 1}[what]
    out = torch.empty(x.shape[0] if mode == 0 else 1, dtype=torch.float32, device=x.device)
    call('tfep_abs_reduce', ptr(x), ldx, x.shape[0], x.shape[1], mode, ptr(out), stream_of(x))
    return out


def pow2_inv_scale(bound):
    """1 / s for the power of two s that puts ``bound`` (> 0, per row) into [2^14, 2^15): the inverse scale of a split row
    whose entries are known to stay below ``bound`` (the split format keeps an absolute error of 2^-40 of the scaled
    maximum, so a loose bound costs nothing)."""
    e = torch.floor(torch.log2(bound.clamp_min(1e-30).double()))
    return torch.exp2(e - 14.0).float()


def masked_weight_prepare_split(weight_v, weight_g, mask, row_of_out, in_of_col, out, inv_scale, col_cut=None):
    """Effective masked weight written directly as split-f16 rows into ``out`` (n_rows_padded, k_padded), whose
    padding rows must already be zero (``tfep_masked_weight_prepare_split``).  ``inv_scale``: 4 floats --
    [1/scale, scratch, max_j sum_k |w_jk|, unused].  ``col_cut`` (int32 per output row): the mask rows are prefixes of the
    packed columns, ``mask[o, in_of_col[c]] == (c < col_cut[o])`` -- the mask is then not read."""
    check_device_tensor(weight_v, 'weight')
    if inv_scale.numel() < 4:
        raise ValueError('inv_scale must have 4 entries')
    N, K = weight_v.shape
    v_c = weight_v.contiguous()
    g_c = None if weight_g is None else weight_g.contiguous()
    m_c = None if mask is None else mask.contiguous()
    call('tfep_masked_weight_prepare_split', ptr(v_c), ptr(g_c), ptr(m_c), N, K, ptr(row_of_out), ptr(in_of_col), ptr(col_cut),
         ptr(out), out.shape[1], out.shape[1], ptr(inv_scale), stream_of(weight_v))
    return out, inv_scale


def masked_linear_split(x_split, x_inv_scale, w_split, w_inv_scale, bias, n_out, k_ranges=None, act=0, out=None,
                        tile_order=None, split_out=False, bias_absmax=None, k_split=1):
    """``masked_linear_packed`` on split-f16 operands; the output is ordinary fp32, or -- ``split_out`` with
    ``act=1`` -- the ELU activations as split rows for the next layer: returns ``(rows, inv_scale)`` then.
    ``w_inv_scale`` is the 4-float buffer of ``masked_weight_prepare_split`` (its entry 2 bounds the outputs).
    ``k_split`` > 1 (plain linear product only): the k range is cut into that many slices whose partial sums go to the
    slabs ``out[s]`` of an ``(k_split, B, n_out)`` output (bias in slab 0); the caller adds them."""
    B = x_split.shape[0]
    n_rows_w, k_padded = w_split.shape
    if out is None:
        out = torch.empty((B, n_out) if k_split <= 1 else (k_split, B, n_out), dtype=torch.float32, device=x_split.device)
    d = _lib.GemmDesc()
    if split_out:
        if bias_absmax is None:
            bias_absmax = abs_reduce(bias.reshape(1, -1), 'row_max') if bias is not None else zeros(1, device=out.device)
        y_inv = torch.empty(max(B, 1), dtype=torch.float32, device=out.device)
        d.split_out, d.y_inv_scale = 1, y_inv.data_ptr()
        d.w_l1max, d.bias_absmax = w_inv_scale.data_ptr() + 8, bias_absmax.data_ptr()
    d.x, d.ldx = x_split.data_ptr(), x_split.shape[1]
    d.w, d.ldw = w_split.data_ptr(), k_padded
    d.bias = bias.data_ptr() if bias is not None else None
    d.k_ranges = k_ranges.data_ptr() if k_ranges is not None else None
    d.tile_order = tile_order.data_ptr() if tile_order is not None else None
    d.col_map = None
    d.y, d.ldy = out.data_ptr(), out.shape[-1]
    d.B, d.N, d.n_rows_w, d.k_padded, d.act, d.accumulate = B, n_out, n_rows_w, k_padded, int(act), 0
    d.split, d.x_inv_scale, d.w_inv_scale = 1, x_inv_scale.data_ptr(), w_inv_scale.data_ptr()
    if k_split > 1:
        d.k_split, d.slab_stride = int(k_split), out.shape[-2] * out.shape[-1]
    call('tfep_masked_linear_gemm', ctypes.byref(d), stream_of(x_split))
    return (out, y_inv) if split_out else out


# ----------------------------------------------------------------------------- reductions

def tfep_reduce(target_potentials, log_det_J=None, ref_potentials=None, log_weights=None, bias=None,
                kT=1.0, ignore_nan=False):
    """The 9 float64 sufficient statistics of the TFEP loss / estimator (see tfep_hip.h).  float64 inputs (all of them)
    take ``tfep_tfep_reduce_f64``, which forms the residuals in fp64."""
    dt = _dtype(target_potentials)
    t = check_device_tensor(target_potentials.contiguous(), 'target_potentials', dt)
    N = t.numel()
    opt = []
    for v, n in ((log_det_J, 'log_det_J'), (ref_potentials, 'ref_potentials'), (log_weights, 'log_weights'),
                 (bias, 'bias')):
        if v is not None:
            v = check_device_tensor(v.contiguous(), n, dt)
            if v.numel() != N:
                raise ValueError(f'{n} must have {N} elements')
        opt.append(v)
    nws = _lib.load().tfep_tfep_reduce_workspace_doubles(N)
    ws = torch.empty(nws, dtype=torch.float64, device=t.device)
    out = torch.empty(9, dtype=torch.float64, device=t.device)
    call('tfep_tfep_reduce' + _sfx(dt), ptr(t), ptr(opt[0]), ptr(opt[1]), ptr(opt[2]), ptr(opt[3]), float(kT),
         int(bool(ignore_nan)), N, ptr(ws), ptr(out), stream_of(t))
    return out


# ----------------------------------------------------------------------------- radial expansion, segment sum

def _radial_inputs(r, means, log_gammas):
    """``(r flattened, means, log_gammas, dtype)``: contiguous, of the dtype of ``r`` (TypeError otherwise), ``K >= 1``."""
    dt = _dtype(r)
    check_device_tensor(r, 'r', dt)
    check_device_tensor(means, 'means', dt)
    check_device_tensor(log_gammas, 'log_gammas', dt)
    if means.dim() != 1 or means.shape != log_gammas.shape or means.numel() < 1:
        raise ValueError('means and log_gammas must be 1-D, of one length >= 1')
    return r.contiguous().reshape(-1), means.contiguous(), log_gammas.contiguous(), dt


def radial_expansion(r, means, log_gammas, r_cutoff=0.0, switching=False, force_zero=True):
    """``exp(-exp(log_gamma_k) (r - mean_k)^2)``, times the Behler-Parrinello switch with ``switching``: ``(*r.shape, K)`` of
    the dtype of ``r``.  float32 is ``tfep_radial_expansion`` (the kernel the modules call), float64 its twin."""
    flat, means, log_gammas, dt = _radial_inputs(r, means, log_gammas)
    K = means.numel()
    out = torch.empty(flat.numel(), K, dtype=dt, device=flat.device)
    call('tfep_radial_expansion' + _sfx(dt), ptr(flat), flat.numel(), ptr(means), ptr(log_gammas), K, float(r_cutoff),
         int(bool(switching)), int(bool(force_zero)), ptr(out), stream_of(flat))
    return out.reshape(*r.shape, K)


def radial_expansion_backward(r, means, log_gammas, grad_out, r_cutoff=0.0, switching=False, force_zero=True):
    """VJP of ``radial_expansion`` for the cotangent ``grad_out (*r.shape, K)``: ``(g_r, g_means, g_log_gammas)``.  The sums
    over the rows have one order per ``(r.numel(), K)``: two calls give the same bits."""
    flat, means, log_gammas, dt = _radial_inputs(r, means, log_gammas)
    n, K = flat.numel(), means.numel()
    g = check_device_tensor(grad_out, 'grad_out', dt).contiguous()
    if g.shape != (*r.shape, K):
        raise ValueError(f'grad_out must be {(*r.shape, K)}, got {tuple(g.shape)}')
    g_r = torch.empty(n, dtype=dt, device=flat.device)
    g_means, g_lg = torch.empty_like(means), torch.empty_like(log_gammas)
    n_ws = _lib.load().tfep_radial_expansion_backward_workspace_doubles(n, K)
    if n_ws < 0:
        raise ValueError(_lib.load().tfep_last_error().decode())
    ws = torch.empty(max(n_ws, 1), dtype=torch.float64, device=flat.device)
    call('tfep_radial_expansion_backward' + _sfx(dt), ptr(flat), n, ptr(means), ptr(log_gammas), K, float(r_cutoff),
         int(bool(switching)), int(bool(force_zero)), ptr(g), ptr(g_r), ptr(g_means), ptr(g_lg), ptr(ws), stream_of(flat))
    return g_r.reshape(r.shape), g_means, g_lg


def _segment_ids(segment_ids, n_rows, device):
    ids = segment_ids.to(device=device, dtype=torch.int64).contiguous()
    if ids.shape != (n_rows,):
        raise ValueError('segment_ids must have one entry per row of data')
    return ids


def segment_sum(data, segment_ids, n_segments):
    """``out[s] = sum of the rows of data with segment_ids == s`` (ids out of range are skipped), float32 or float64."""
    dt = _dtype(data)
    check_device_tensor(data, 'data', dt)
    if data.dim() != 2 or data.shape[1] < 1:
        raise ValueError('data must be (n_rows, n_columns >= 1)')
    data = data.contiguous()
    ids = _segment_ids(segment_ids, data.shape[0], data.device)
    out = torch.empty(int(n_segments), data.shape[1], dtype=dt, device=data.device)
    call('tfep_segment_sum' + _sfx(dt), ptr(data), ptr(ids), data.shape[0], data.shape[1], int(n_segments), ptr(out),
         stream_of(data))
    return out


def segment_gather(grad_out, segment_ids):
    """VJP of ``segment_sum``: row ``i`` is ``grad_out[segment_ids[i]]``, zeros where the id names no segment."""
    dt = _dtype(grad_out)
    check_device_tensor(grad_out, 'grad_out', dt)
    if grad_out.dim() != 2 or grad_out.shape[1] < 1:
        raise ValueError('grad_out must be (n_segments, n_columns >= 1)')
    g = grad_out.contiguous()
    if segment_ids.dim() != 1:
        raise ValueError('segment_ids must be 1-D')
    ids = _segment_ids(segment_ids, segment_ids.shape[0], g.device)
    out = torch.empty(ids.shape[0], g.shape[1], dtype=dt, device=g.device)
    call('tfep_segment_gather' + _sfx(dt), ptr(g), ptr(ids), ids.shape[0], g.shape[1], g.shape[0], ptr(out), stream_of(g))
    return out


# ----------------------------------------------------------------------------- edge geometry, pruning

def _edge_inputs(x, edges):
    dt = _dtype(x)
    x, ldx = rows(x, 'x', dt)
    if x.shape[1] != 3:
        raise ValueError(f'x must be (n_nodes, 3), got {tuple(x.shape)}')
    if not isinstance(edges, torch.Tensor) or edges.device != x.device:
        raise ValueError('edges must be a tensor on the device of x')
    return dt, x, ldx, _tables.edge_entry(edges, x.shape[0])


def edge_geometry(x, edges, normalize=False, inverse=False):
    """``(distances (E,), directions (E, 3))`` across the edges ``(2, E)`` of the nodes ``x`` (n_nodes, 3; any row stride):
    ``x[edges[1]] - x[edges[0]]`` (negated with ``inverse``), its length, and with ``normalize`` the unit vector (NaN for an
    edge of length 0).  One launch (``tfep_edge_geometry``); float32 or float64, the dtype of ``x``."""
    dt, x, ldx, entry = _edge_inputs(x, edges)
    edges = entry[0]
    E = edges.shape[1]
    distances = torch.empty(E, dtype=dt, device=x.device)
    directions = torch.empty(E, 3, dtype=dt, device=x.device)
    call('tfep_edge_geometry' + _sfx(dt), ptr(x), ldx, ptr(edges), x.shape[0], E, int(bool(normalize)), int(bool(inverse)),
         ptr(distances), ptr(directions), stream_of(x))
    return distances, directions


def edge_geometry_backward(x, edges, grad_distances, grad_directions, normalize=False, inverse=False):
    """VJP of ``edge_geometry`` at ``x``: the cotangent of ``x``, every row written.  Either cotangent may be ``None`` (zero).
    One lane per node over ``edge_incidence(edges)``, the contributions added in list order: no atomics, and the gradient of
    a node has the same bits whatever else is in the batch."""
    dt, x, ldx, entry = _edge_inputs(x, edges)
    edges = entry[0]
    N, E = x.shape[0], edges.shape[1]
    grads = []
    for g, shape, name in ((grad_distances, (E,), 'grad_distances'), (grad_directions, (E, 3), 'grad_directions')):
        if g is not None:
            g = check_device_tensor(g, name, dt).contiguous()
            if tuple(g.shape) != shape:
                raise ValueError(f'{name} must be {shape}, got {tuple(g.shape)}')
        grads.append(g)
    node_ptr, incident = _tables.edge_incidence(edges, N, entry) if E else (None, None)
    gx = torch.empty(N, 3, dtype=dt, device=x.device)
    call('tfep_edge_geometry_backward' + _sfx(dt), ptr(x), ldx, ptr(edges), N, E, ptr(node_ptr), ptr(incident),
         int(bool(normalize)), int(bool(inverse)), ptr(grads[0]), ptr(grads[1]), ptr(gx), 3, stream_of(x))
    return gx


def edge_prune(distances, r_cutoff):
    """The ids of the edges with ``distances <= r_cutoff`` in ascending order, int64 (a NaN distance is dropped): an ordered
    stream compaction without atomics (``tfep_edge_prune_count``, one read of the total, ``tfep_edge_prune_compact``).  The
    cutoff is compared in the dtype of ``distances``, as torch compares a tensor with a Python number."""
    dt = _dtype(distances)
    d = check_device_tensor(distances, 'distances', dt).detach().contiguous()
    if d.dim() != 1:
        raise ValueError(f'distances must be (n_edges,), got {tuple(d.shape)}')
    E = d.shape[0]
    if E == 0:
        return torch.empty(0, dtype=torch.int64, device=d.device)
    ws = torch.empty(_lib.load().tfep_edge_prune_workspace_int64s(E), dtype=torch.int64, device=d.device)
    call('tfep_edge_prune_count' + _sfx(dt), ptr(d), E, float(r_cutoff), ptr(ws), stream_of(d))
    n_kept = int(ws[-1])                                              # the one synchronisation, as of nonzero()
    keep_index = torch.empty(n_kept, dtype=torch.int64, device=d.device)
    call('tfep_edge_prune_compact' + _sfx(dt), ptr(d), E, float(r_cutoff), ptr(ws), ptr(keep_index), n_kept, stream_of(d))
    return keep_index


def edge_select_edges(edges, keep_index):
    """``edges[:, keep_index]`` of int64 edges ``(2, E)`` on the HIP device (``tfep_edge_select_edges``)."""
    check_device_tensor(edges, 'edges', torch.int64)
    check_device_tensor(keep_index, 'keep_index', torch.int64)
    if edges.dim() != 2 or edges.shape[0] != 2 or keep_index.dim() != 1:
        raise ValueError('edges must be (2, n_edges) and keep_index 1-D')
    edges, keep_index = edges.contiguous(), keep_index.contiguous()
    out = torch.empty(2, keep_index.shape[0], dtype=torch.int64, device=edges.device)
    call('tfep_edge_select_edges', ptr(edges), edges.shape[1], ptr(keep_index), keep_index.shape[0], ptr(out), stream_of(edges))
    return out
