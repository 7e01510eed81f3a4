"""The kernels as custom torch ops: ``torch.ops.tfep.*`` (north star: "exposed as custom torch ops").

Each op is a thin dispatcher entry over one C-ABI entry point of ``include/tfep_hip.h``, through its wrapper in
``tfep_amd.ops`` (only ``fused_output_transformer`` launches from here, ``_fused_launch``): a schema, a HIP ("cuda" device
type) implementation, a fake / meta implementation (shapes and dtypes only, so that ``torch.compile``, ``make_fx`` and
fake-tensor tracing see through them) and, where a VJP kernel exists, an autograd formula whose backward is itself a
registered op.  There is no CPU implementation: calling an op with CPU tensors fails in the dispatcher ("no kernel for
CPU") -- the same no-fallback policy as the rest of the package.

  tfep::affine_forward / affine_inverse / affine_backward            reference transformers/affine.py:281-363
  tfep::sos_forward / sos_backward                                    reference transformers/sos.py:81-265 (SOS_OPS)
  tfep::spline_forward / spline_inverse / spline_backward            reference transformers/spline.py:184-261, 424-564
  tfep::moebius_forward / moebius_inverse / moebius_backward         reference transformers/moebius.py:104-147, 374-478
  tfep::symmetrized_moebius_forward / _inverse / _backward           reference transformers/moebius.py:193-372, 481-629
                                                                     (SYMMETRIZED_MOEBIUS_OPS)
  tfep::quaternion_product_forward / _inverse / _backward            reference transformers/quatprod.py
                                                                     (QUATERNION_PRODUCT_OPS)
  tfep::flip_invariant_embedding / _backward                         reference embeddings/mafembed.py:174-348
                                                                     (FLIP_EMBEDDING_OPS)
  tfep::centroid_shift / centroid_restore / frame_orient / frame_rotate, each with its _backward
                                                                     reference flows/centroid.py, flows/oriented.py,
                                                                     utils/geometry.py:239-411 (FRAME_OPS)
  tfep::internal_coordinates / _backward, polar_forward / polar_backward
                                                                     reference utils/geometry.py:28-178, 414-471
                                                                     (GEOMETRY_OPS)
  tfep::zmatrix_place / zmatrix_place_backward                       the inverse of internal_coordinates on a Z-matrix
                                                                     (ZMATRIX_OPS; the reference imports it from bgflow)
  tfep::relative_frame_encode / relative_frame_decode, each with its _backward
                                                                     reference app/mixedmaf.py:1216-1271, 1321-1375
                                                                     (RELATIVE_FRAME_OPS)
  tfep::radial_expansion / _backward, segment_sum / segment_gather   reference embeddings/radial.py:110-130, 161-176,
                                                                     graph.py:304-316 (GRAPH_OPS)
  tfep::edge_geometry / _backward, edge_prune, edge_select           reference graph.py:222-301 (EDGE_OPS)
  tfep::masked_linear / masked_linear_backward                       reference masked.py:220-302, 351-404
  tfep::fused_output_transformer                                     masked.py:188-208 (last layer) + the transformer
  tfep::tfep_reduce                                                  loss.py:125-140, analysis/estimator.py:73-86

The Module API (``tfep_amd.nn``, ``tfep_amd.loss``) routes through these ops.
"""
import ctypes
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.library import custom_op

from . import _lib, ops

_DEV = 'cuda'          # PyTorch-ROCm's name for the HIP device type


def _pair_like(x):
    return x.new_empty(x.shape), x.new_empty((x.shape[0],))


# ============================================================================= affine

@custom_op('tfep::affine_forward', mutates_args=(), device_types=_DEV)
def affine_forward(x: Tensor, parameters: Tensor) -> Tuple[Tensor, Tensor]:
    return ops.affine(x, parameters, inverse=False)


@custom_op('tfep::affine_inverse', mutates_args=(), device_types=_DEV)
def affine_inverse(y: Tensor, parameters: Tensor) -> Tuple[Tensor, Tensor]:
    return ops.affine(y, parameters, inverse=True)


@custom_op('tfep::affine_backward', mutates_args=(), device_types=_DEV)
def affine_backward(x: Tensor, parameters: Tensor, grad_y: Tensor, grad_log_det_J: Tensor) -> Tuple[Tensor, Tensor]:
    return ops.affine_backward(x, parameters, grad_y, grad_log_det_J)


affine_forward.register_fake(lambda x, parameters: _pair_like(x))
affine_inverse.register_fake(lambda y, parameters: _pair_like(y))
affine_backward.register_fake(lambda x, parameters, gy, gl: (x.new_empty(x.shape), parameters.new_empty(parameters.shape)))


def _vjp_inputs(ctx, grads):
    """Upstream gradients of (y, log_det_J), zeros where autograd passes None."""
    x = ctx.saved_tensors[0]
    gy, gl = grads
    # (fill kernels, ``ops.zeros``: a captured training step gets no memset node)
    gy = ops.zeros(*x.shape, dtype=x.dtype, device=x.device) if gy is None else gy
    gl = ops.zeros(x.shape[0], dtype=x.dtype, device=x.device) if gl is None else gl
    return gy, gl


def _save_xp(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])


def _affine_bwd(ctx, gy, gl):
    x, p = ctx.saved_tensors
    gy, gl = _vjp_inputs(ctx, (gy, gl))
    return torch.ops.tfep.affine_backward(x, p, gy, gl)


affine_forward.register_autograd(_affine_bwd, setup_context=_save_xp)


# ============================================================================= sum-of-squares polynomial

@custom_op('tfep::sos_forward', mutates_args=(), device_types=_DEV)
def sos_forward(x: Tensor, parameters: Tensor, n_polynomials: int) -> Tuple[Tensor, Tensor]:
    return ops.sos(x, parameters, n_polynomials)


@custom_op('tfep::sos_backward', mutates_args=(), device_types=_DEV)
def sos_backward(x: Tensor, parameters: Tensor, n_polynomials: int, grad_y: Tensor) -> Tuple[Tensor, Tensor]:
    """VJP of ``sos_forward`` for the cotangent of y; the log-det has none (non-differentiable, reference sos.py:222)."""
    return ops.sos_backward(x, parameters, n_polynomials, grad_y)


sos_forward.register_fake(lambda x, parameters, n_polynomials: _pair_like(x))
sos_backward.register_fake(lambda x, parameters, n_polynomials, gy: (x.new_empty(x.shape), parameters.new_empty(parameters.shape)))


def _sos_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.n_polynomials = inputs[2]
    ctx.mark_non_differentiable(output[1])           # the log-det (reference sos.py:222)


def _sos_bwd(ctx, gy, gl):
    x, p = ctx.saved_tensors
    gy = ops.zeros(*x.shape, dtype=x.dtype, device=x.device) if gy is None else gy   # (gl is ignored: the log-det carries no gradient)
    return (*torch.ops.tfep.sos_backward(x, p, ctx.n_polynomials, gy), None)


sos_forward.register_autograd(_sos_bwd, setup_context=_sos_setup)


# ============================================================================= rational-quadratic spline

def _spline_cfg(x0, xf, y0, yf, n_bins, circular, identity, learn_lower, learn_upper, min_bin, min_slope):
    """The descriptor of the domain arrays' dtype: float64 arrays select the float64 kernels (and then x and the parameters
    must be float64 too)."""
    return ops.SplineConfig(x0, xf, y0, yf, n_bins, circular, identity, learn_lower, learn_upper, min_bin, min_slope,
                            dtype=ops._dtype(x0))


@custom_op('tfep::spline_forward', mutates_args=(), device_types=_DEV)
def spline_forward(x: Tensor, parameters: Tensor, x0: Tensor, xf: Tensor, y0: Tensor, yf: Tensor, n_bins: int,
                   circular: bool, identity_boundary_slopes: bool, learn_lower_bound: bool, learn_upper_bound: bool,
                   min_bin_size: float, min_slope: float) -> Tuple[Tensor, Tensor]:
    cfg = _spline_cfg(x0, xf, y0, yf, n_bins, circular, identity_boundary_slopes, learn_lower_bound, learn_upper_bound,
                      min_bin_size, min_slope)
    return ops.spline(x, parameters, cfg, inverse=False)


@custom_op('tfep::spline_inverse', mutates_args=(), device_types=_DEV)
def spline_inverse(y: Tensor, parameters: Tensor, x0: Tensor, xf: Tensor, y0: Tensor, yf: Tensor, n_bins: int,
                   circular: bool, identity_boundary_slopes: bool, learn_lower_bound: bool, learn_upper_bound: bool,
                   min_bin_size: float, min_slope: float) -> Tuple[Tensor, Tensor]:
    cfg = _spline_cfg(x0, xf, y0, yf, n_bins, circular, identity_boundary_slopes, learn_lower_bound, learn_upper_bound,
                      min_bin_size, min_slope)
    return ops.spline(y, parameters, cfg, inverse=True)


@custom_op('tfep::spline_backward', mutates_args=(), device_types=_DEV)
def spline_backward(x: Tensor, parameters: Tensor, grad_y: Tensor, grad_log_det_J: Tensor, x0: Tensor, xf: Tensor,
                    y0: Tensor, yf: Tensor, n_bins: int, circular: bool, identity_boundary_slopes: bool,
                    learn_lower_bound: bool, learn_upper_bound: bool, min_bin_size: float,
                    min_slope: float) -> Tuple[Tensor, Tensor]:
    cfg = _spline_cfg(x0, xf, y0, yf, n_bins, circular, identity_boundary_slopes, learn_lower_bound, learn_upper_bound,
                      min_bin_size, min_slope)
    return ops.spline_backward(x, parameters, cfg, grad_y, grad_log_det_J)


spline_forward.register_fake(lambda x, parameters, *cfg: _pair_like(x))
spline_inverse.register_fake(lambda y, parameters, *cfg: _pair_like(y))
spline_backward.register_fake(lambda x, parameters, gy, gl, *cfg: (x.new_empty(x.shape),
                                                                   parameters.new_empty(parameters.shape)))


def _spline_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], *inputs[2:6])
    ctx.cfg = tuple(inputs[6:])


def _spline_bwd(ctx, gy, gl):
    x, p, x0, xf, y0, yf = ctx.saved_tensors
    gy, gl = _vjp_inputs(ctx, (gy, gl))
    gx, gp = torch.ops.tfep.spline_backward(x, p, gy, gl, x0, xf, y0, yf, *ctx.cfg)
    return (gx, gp) + (None,) * 11


spline_forward.register_autograd(_spline_bwd, setup_context=_spline_setup)


# ============================================================================= Moebius

@custom_op('tfep::moebius_forward', mutates_args=(), device_types=_DEV)
def moebius_forward(x: Tensor, parameters: Tensor, dimension: int, max_radius: float,
                    unit_sphere: bool) -> Tuple[Tensor, Tensor]:
    return ops.moebius(x, parameters, dimension, max_radius, unit_sphere, inverse=False)


@custom_op('tfep::moebius_inverse', mutates_args=(), device_types=_DEV)
def moebius_inverse(y: Tensor, parameters: Tensor, dimension: int, max_radius: float,
                    unit_sphere: bool) -> Tuple[Tensor, Tensor]:
    return ops.moebius(y, parameters, dimension, max_radius, unit_sphere, inverse=True)


@custom_op('tfep::moebius_backward', mutates_args=(), device_types=_DEV)
def moebius_backward(x: Tensor, parameters: Tensor, grad_y: Tensor, grad_log_det_J: Tensor, dimension: int,
                     max_radius: float, unit_sphere: bool) -> Tuple[Tensor, Tensor]:
    return ops.moebius_backward(x, parameters, dimension, max_radius, unit_sphere, grad_y, grad_log_det_J)


moebius_forward.register_fake(lambda x, parameters, *a: _pair_like(x))
moebius_inverse.register_fake(lambda y, parameters, *a: _pair_like(y))
moebius_backward.register_fake(lambda x, parameters, gy, gl, *a: (x.new_empty(x.shape),
                                                                  parameters.new_empty(parameters.shape)))


def _moebius_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.cfg = tuple(inputs[2:])


def _moebius_bwd(ctx, gy, gl):
    x, p = ctx.saved_tensors
    gy, gl = _vjp_inputs(ctx, (gy, gl))
    gx, gp = torch.ops.tfep.moebius_backward(x, p, gy, gl, *ctx.cfg)
    return gx, gp, None, None, None


def _moebius_inverse_bwd(ctx, gy, gl):
    # the inverse is the forward map on negated parameters (reference moebius.py:142-147): its VJP at -p, and d(-p)/dp = -1
    y, p = ctx.saved_tensors
    gy, gl = _vjp_inputs(ctx, (gy, gl))
    gx, gp = torch.ops.tfep.moebius_backward(y, -p, gy, gl, *ctx.cfg)
    return gx, -gp, None, None, None


moebius_forward.register_autograd(_moebius_bwd, setup_context=_moebius_setup)
moebius_inverse.register_autograd(_moebius_inverse_bwd, setup_context=_moebius_setup)


# ============================================================================= symmetrized Moebius

@custom_op('tfep::symmetrized_moebius_forward', mutates_args=(), device_types=_DEV)
def symmetrized_moebius_forward(x: Tensor, parameters: Tensor, dimension: int, max_radius: float) -> Tuple[Tensor, Tensor]:
    return ops.symmetrized_moebius(x, parameters, dimension, max_radius, inverse=False)


@custom_op('tfep::symmetrized_moebius_inverse', mutates_args=(), device_types=_DEV)
def symmetrized_moebius_inverse(y: Tensor, parameters: Tensor, dimension: int, max_radius: float) -> Tuple[Tensor, Tensor]:
    return ops.symmetrized_moebius(y, parameters, dimension, max_radius, inverse=True)


@custom_op('tfep::symmetrized_moebius_backward', mutates_args=(), device_types=_DEV)
def symmetrized_moebius_backward(x: Tensor, parameters: Tensor, grad_y: Tensor, grad_log_det_J: Tensor, dimension: int,
                                 max_radius: float, inverse: bool) -> Tuple[Tensor, Tensor]:
    """VJP of ``symmetrized_moebius_forward`` (``inverse`` False) or ``_inverse`` (True) at its input ``x``; the log-det
    carries gradient in both directions."""
    return ops.symmetrized_moebius_backward(x, parameters, dimension, max_radius, inverse, grad_y, grad_log_det_J)


symmetrized_moebius_forward.register_fake(lambda x, parameters, *a: _pair_like(x))
symmetrized_moebius_inverse.register_fake(lambda y, parameters, *a: _pair_like(y))
symmetrized_moebius_backward.register_fake(lambda x, parameters, gy, gl, *a: (x.new_empty(x.shape),
                                                                              parameters.new_empty(parameters.shape)))


def _symmoebius_bwd(inverse):
    def bwd(ctx, gy, gl):
        x, p = ctx.saved_tensors
        gy, gl = _vjp_inputs(ctx, (gy, gl))
        gx, gp = torch.ops.tfep.symmetrized_moebius_backward(x, p, gy, gl, *ctx.cfg, inverse)
        return gx, gp, None, None
    return bwd


symmetrized_moebius_forward.register_autograd(_symmoebius_bwd(False), setup_context=_moebius_setup)
symmetrized_moebius_inverse.register_autograd(_symmoebius_bwd(True), setup_context=_moebius_setup)


# ============================================================================= quaternion product

@custom_op('tfep::quaternion_product_forward', mutates_args=(), device_types=_DEV)
def quaternion_product_forward(x: Tensor, parameters: Tensor) -> Tuple[Tensor, Tensor]:
    return ops.quaternion_product(x, parameters, inverse=False)


@custom_op('tfep::quaternion_product_inverse', mutates_args=(), device_types=_DEV)
def quaternion_product_inverse(y: Tensor, parameters: Tensor) -> Tuple[Tensor, Tensor]:
    return ops.quaternion_product(y, parameters, inverse=True)


@custom_op('tfep::quaternion_product_backward', mutates_args=(), device_types=_DEV)
def quaternion_product_backward(x: Tensor, parameters: Tensor, grad_y: Tensor, inverse: bool) -> Tuple[Tensor, Tensor]:
    """VJP of ``quaternion_product_forward`` (``inverse`` False) or ``_inverse`` (True) at its input ``x``.  The log-det is
    the constant zero: its cotangent is no argument."""
    return ops.quaternion_product_backward(x, parameters, inverse, grad_y)


quaternion_product_forward.register_fake(lambda x, parameters: _pair_like(x))
quaternion_product_inverse.register_fake(lambda y, parameters: _pair_like(y))
quaternion_product_backward.register_fake(lambda x, parameters, gy, inverse: (x.new_empty(x.shape),
                                                                              parameters.new_empty(parameters.shape)))


def _quatprod_bwd(inverse):
    def bwd(ctx, gy, gl):
        x, p = ctx.saved_tensors
        gy, _ = _vjp_inputs(ctx, (gy, gl))
        return torch.ops.tfep.quaternion_product_backward(x, p, gy, inverse)
    return bwd


quaternion_product_forward.register_autograd(_quatprod_bwd(False), setup_context=_save_xp)
quaternion_product_inverse.register_autograd(_quatprod_bwd(True), setup_context=_save_xp)


# ============================================================================= flip-invariant embedding

@custom_op('tfep::flip_invariant_embedding', mutates_args=(), device_types=_DEV)
def flip_invariant_embedding(x: Tensor, embedded_indices: Tensor, nonembedded_indices: Tensor, vector_dim: int,
                             emb_w1: Tensor, emb_b1: Tensor, emb_w2: Tensor, emb_b2: Tensor, wgt_w1: Tensor,
                             wgt_b1: Tensor, wgt_w2: Tensor, wgt_b2: Tensor) -> Tensor:
    """``FlipInvariantEmbedding.forward``: the index tables are int32, the eight parameters those of
    ``embedding_layer.{0,2}`` and ``weight_layer.{0,2}``."""
    return ops.flip_invariant_embedding(x, embedded_indices, nonembedded_indices, vector_dim,
                                        (emb_w1, emb_b1, emb_w2, emb_b2, wgt_w1, wgt_b1, wgt_w2, wgt_b2))


@custom_op('tfep::flip_invariant_embedding_backward', mutates_args=(), device_types=_DEV)
def flip_invariant_embedding_backward(x: Tensor, embedded_indices: Tensor, nonembedded_indices: Tensor, vector_dim: int,
                                      emb_w1: Tensor, emb_b1: Tensor, emb_w2: Tensor, emb_b2: Tensor, wgt_w1: Tensor,
                                      wgt_b1: Tensor, wgt_w2: Tensor, wgt_b2: Tensor, grad_out: Tensor
                                      ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """VJP of ``flip_invariant_embedding``: ``(gx, the eight parameter gradients)``."""
    gx, grads = ops.flip_invariant_embedding_backward(x, embedded_indices, nonembedded_indices, vector_dim,
                                                      (emb_w1, emb_b1, emb_w2, emb_b2, wgt_w1, wgt_b1, wgt_w2, wgt_b2),
                                                      grad_out.contiguous())
    return (gx, *grads)


@flip_invariant_embedding.register_fake
def _(x, embedded_indices, nonembedded_indices, vector_dim, emb_w1, emb_b1, emb_w2, *rest):
    n_vectors = embedded_indices.numel() // vector_dim
    return x.new_empty((x.shape[0], nonembedded_indices.numel() + n_vectors * emb_w2.shape[0]))


@flip_invariant_embedding_backward.register_fake
def _(x, embedded_indices, nonembedded_indices, vector_dim, *rest):
    return (x.new_empty(x.shape), *(p.new_empty(p.shape) for p in rest[:8]))


def _flip_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], inputs[2], *inputs[4:])
    ctx.vector_dim = inputs[3]


def _flip_bwd(ctx, grad_out):
    x, eidx, nidx, *params = ctx.saved_tensors
    gx, *grads = torch.ops.tfep.flip_invariant_embedding_backward(x, eidx, nidx, ctx.vector_dim, *params, grad_out)
    return (gx, None, None, None, *grads)


flip_invariant_embedding.register_autograd(_flip_bwd, setup_context=_flip_setup)


# ============================================================================= frames of the Cartesian wrappers

@custom_op('tfep::centroid_shift', mutates_args=(), device_types=_DEV)
def centroid_shift(x: Tensor, subset: Optional[Tensor], weights: Optional[Tensor], origin: Tensor,
                   dim: int) -> Tuple[Tensor, Tensor]:
    """``(shift, y)`` of ``CenteredCentroidFlow``: ``shift = origin - centroid`` (B, dim), ``y = x + shift``.  ``subset``:
    int32 point indices (distinct), ``weights``: normalised; float32 or float64, all alike (else TypeError)."""
    return ops.centroid_shift(x, subset, weights, origin, dim)


@custom_op('tfep::centroid_shift_backward', mutates_args=(), device_types=_DEV)
def centroid_shift_backward(grad_y: Tensor, grad_shift: Tensor, subset: Optional[Tensor], weights: Optional[Tensor],
                            dim: int) -> Tensor:
    return ops.centroid_shift_backward(grad_y, grad_shift, subset, weights, dim)


@custom_op('tfep::centroid_restore', mutates_args=(), device_types=_DEV)
def centroid_restore(y: Tensor, shift: Tensor, subset: Optional[Tensor], weights: Optional[Tensor], origin: Tensor,
                     fixed_point: int, fixed_entry: int, dim: int, translate_back: bool) -> Tensor:
    """The fixed point placed so that the centroid is ``origin`` again, then ``- shift`` with ``translate_back``."""
    return ops.centroid_restore(y, shift, subset, weights, origin, fixed_point, fixed_entry, dim, translate_back)


@custom_op('tfep::centroid_restore_backward', mutates_args=(), device_types=_DEV)
def centroid_restore_backward(grad_out: Tensor, subset: Optional[Tensor], weights: Optional[Tensor], fixed_point: int,
                              fixed_entry: int, dim: int, translate_back: bool) -> Tuple[Tensor, Tensor]:
    """``(grad_y, grad_shift)``."""
    return ops.centroid_restore_backward(grad_out, subset, weights, fixed_point, fixed_entry, dim, translate_back)


@custom_op('tfep::frame_orient', mutates_args=(), device_types=_DEV)
def frame_orient(x: Tensor, axis_point: int, plane_point: int, axis: int, plane_axis: int, normal: int,
                 round_off: bool) -> Tuple[Tensor, Tensor]:
    """``(y, R)`` of ``OrientedFlow``: the row in its constrained frame and the rotation as (B, 9)."""
    return ops.frame_orient(x, axis_point, plane_point, axis, plane_axis, normal, round_off)


@custom_op('tfep::frame_orient_backward', mutates_args=(), device_types=_DEV)
def frame_orient_backward(x: Tensor, grad_y: Tensor, grad_rot: Tensor, axis_point: int, plane_point: int, axis: int,
                          plane_axis: int, normal: int, round_off: bool) -> Tensor:
    return ops.frame_orient_backward(x, grad_y, grad_rot, axis_point, plane_point, axis, plane_axis, normal, round_off)


@custom_op('tfep::frame_rotate', mutates_args=(), device_types=_DEV)
def frame_rotate(x: Tensor, rot: Tensor, transposed: bool) -> Tensor:
    """``y_i = x_i R`` (``transposed``: ``x_i R^T``) with the (B, 9) rotations of ``frame_orient``."""
    return ops.frame_rotate(x, rot, transposed)


@custom_op('tfep::frame_rotate_backward', mutates_args=(), device_types=_DEV)
def frame_rotate_backward(x: Tensor, rot: Tensor, grad_y: Tensor, transposed: bool) -> Tuple[Tensor, Tensor]:
    """``(grad_x, grad_R)``."""
    return ops.frame_rotate_backward(x, rot, grad_y, transposed)


centroid_shift.register_fake(lambda x, subset, weights, origin, dim: (x.new_empty((x.shape[0], dim)), x.new_empty(x.shape)))
centroid_shift_backward.register_fake(lambda gy, gs, subset, weights, dim: gy.new_empty(gy.shape))
centroid_restore.register_fake(lambda y, shift, *rest: y.new_empty(y.shape))
centroid_restore_backward.register_fake(
    lambda g, subset, weights, fixed_point, fixed_entry, dim, translate_back: (g.new_empty(g.shape),
                                                                               g.new_empty((g.shape[0], dim))))
frame_orient.register_fake(lambda x, *rest: (x.new_empty(x.shape), x.new_empty((x.shape[0], 9))))
frame_orient_backward.register_fake(lambda x, *rest: x.new_empty(x.shape))
frame_rotate.register_fake(lambda x, rot, transposed: x.new_empty(x.shape))
frame_rotate_backward.register_fake(lambda x, rot, gy, transposed: (x.new_empty(x.shape), rot.new_empty(rot.shape)))


def _meta(t):
    return tuple(t.shape), t.dtype, t.device


def _or_zeros(g, meta):
    """An upstream gradient, zeros (filled by a kernel, see ``ops.zeros``) where autograd passes None."""
    return ops.zeros(*meta[0], dtype=meta[1], device=meta[2]) if g is None else g


def _centroid_shift_setup(ctx, inputs, output):
    x, subset, weights, origin, dim = inputs
    ctx.save_for_backward(subset, weights)
    ctx.dim, ctx.like = dim, (_meta(output[0]), _meta(output[1]))


def _centroid_shift_bwd(ctx, g_shift, g_y):
    subset, weights = ctx.saved_tensors
    shift, y = ctx.like
    gx = torch.ops.tfep.centroid_shift_backward(_or_zeros(g_y, y), _or_zeros(g_shift, shift), subset, weights, ctx.dim)
    return gx, None, None, None, None


def _centroid_restore_setup(ctx, inputs, output):
    y, shift, subset, weights, origin, fixed_point, fixed_entry, dim, translate_back = inputs
    ctx.save_for_backward(subset, weights)
    ctx.cfg = (fixed_point, fixed_entry, dim, translate_back)


def _centroid_restore_bwd(ctx, g):
    subset, weights = ctx.saved_tensors
    gy, gshift = torch.ops.tfep.centroid_restore_backward(g, subset, weights, *ctx.cfg)
    return gy, gshift, None, None, None, None, None, None, None


def _frame_orient_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])
    ctx.cfg = tuple(inputs[1:])
    ctx.like = (_meta(output[0]), _meta(output[1]))


def _frame_orient_bwd(ctx, g_y, g_rot):
    (x,) = ctx.saved_tensors
    y, rot = ctx.like
    gx = torch.ops.tfep.frame_orient_backward(x, _or_zeros(g_y, y), _or_zeros(g_rot, rot), *ctx.cfg)
    return (gx, *([None] * 6))


def _frame_rotate_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.transposed = inputs[2]


def _frame_rotate_bwd(ctx, g):
    x, rot = ctx.saved_tensors
    gx, grot = torch.ops.tfep.frame_rotate_backward(x, rot, g, ctx.transposed)
    return gx, grot, None


centroid_shift.register_autograd(_centroid_shift_bwd, setup_context=_centroid_shift_setup)
centroid_restore.register_autograd(_centroid_restore_bwd, setup_context=_centroid_restore_setup)
frame_orient.register_autograd(_frame_orient_bwd, setup_context=_frame_orient_setup)
frame_rotate.register_autograd(_frame_rotate_bwd, setup_context=_frame_rotate_setup)


# ============================================================================= internal coordinates, polar map

@custom_op('tfep::internal_coordinates', mutates_args=(), device_types=_DEV)
def internal_coordinates(x: Tensor, pairs: Tensor, triples: Tensor, quads: Tensor, atom_start: Tensor,
                         atom_items: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """``(d, a, t)`` of the rows ``x`` (B, 3 n_atoms): distances, angles and proper dihedrals over the int32 tables of
    ``ops.index_tables`` (which validates them on the host; the incidence list serves the backward)."""
    return ops.internal_coordinates(x, pairs, triples, quads, atom_start, atom_items)


@custom_op('tfep::internal_coordinates_backward', mutates_args=(), device_types=_DEV)
def internal_coordinates_backward(x: Tensor, pairs: Tensor, triples: Tensor, quads: Tensor, atom_start: Tensor,
                                  atom_items: Tensor, grad_d: Tensor, grad_a: Tensor, grad_t: Tensor) -> Tensor:
    return ops.internal_coordinates_backward(x, pairs, triples, quads, atom_start, atom_items, grad_d, grad_a, grad_t)


@custom_op('tfep::polar_forward', mutates_args=(), device_types=_DEV)
def polar_forward(a: Tensor, b: Tensor, to_cartesian: bool, with_log_det_J: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """``(r, angle, log_det_J)`` of Cartesian ``(a, b)``, or ``(x, y, log_det_J)`` of polar ``(a, b)`` with
    ``to_cartesian``; the log-det is an empty tensor without ``with_log_det_J``."""
    return ops.polar(a, b, to_cartesian, with_log_det_J)


@custom_op('tfep::polar_backward', mutates_args=(), device_types=_DEV)
def polar_backward(a: Tensor, b: Tensor, to_cartesian: bool, grad_0: Tensor, grad_1: Tensor,
                   grad_log_det_J: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    return ops.polar_backward(a, b, to_cartesian, grad_0, grad_1, grad_log_det_J)


internal_coordinates.register_fake(lambda x, pairs, triples, quads, atom_start, atom_items: tuple(
    x.new_empty((x.shape[0], t.shape[1])) for t in (pairs, triples, quads)))
internal_coordinates_backward.register_fake(lambda x, *rest: x.new_empty(x.shape))
polar_forward.register_fake(lambda a, b, to_cartesian, with_log_det_J: (
    a.new_empty(a.shape), a.new_empty(a.shape), a.new_empty(a.shape if with_log_det_J else (0,))))
polar_backward.register_fake(lambda a, b, to_cartesian, g0, g1, gl: (a.new_empty(a.shape), a.new_empty(a.shape)))


def _internal_coordinates_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)
    ctx.like = tuple(_meta(o) for o in output)


def _internal_coordinates_bwd(ctx, g_d, g_a, g_t):
    grads = (_or_zeros(g, like) for g, like in zip((g_d, g_a, g_t), ctx.like))
    return (torch.ops.tfep.internal_coordinates_backward(*ctx.saved_tensors, *grads), *([None] * 5))


def _polar_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.to_cartesian, ctx.with_log_det_J = inputs[2], inputs[3]
    ctx.like = _meta(output[0])


def _polar_bwd(ctx, g_0, g_1, g_l):
    a, b = ctx.saved_tensors
    g_l = _or_zeros(g_l, ctx.like) if ctx.with_log_det_J else None
    ga, gb = torch.ops.tfep.polar_backward(a, b, ctx.to_cartesian, _or_zeros(g_0, ctx.like), _or_zeros(g_1, ctx.like), g_l)
    return ga, gb, None, None


internal_coordinates.register_autograd(_internal_coordinates_bwd, setup_context=_internal_coordinates_setup)
polar_forward.register_autograd(_polar_bwd, setup_context=_polar_setup)


# ============================================================================= placement from a Z-matrix

@custom_op('tfep::zmatrix_place', mutates_args=(), device_types=_DEV)
def zmatrix_place(d: Tensor, a: Tensor, t: Tensor, x_fixed: Tensor, rows: Tensor, level_start: Tensor, fixed: Tensor,
                  atom_start: Tensor, atom_items: Tensor) -> Tuple[Tensor, Tensor]:
    """``(x, log_det_J)``: the rows (B, 3 n_atoms) placed from ``d, a, t`` (B, n_ic) and the fixed atoms ``x_fixed`` (B,
    3 n_fixed) over the int32 tables of ``ops.zmatrix_tables`` (which validates them on the host; the incidence list
    serves the backward)."""
    return ops.zmatrix_place(d, a, t, x_fixed, rows, level_start, fixed, atom_start, atom_items)


@custom_op('tfep::zmatrix_place_backward', mutates_args=(), device_types=_DEV)
def zmatrix_place_backward(x: Tensor, d: Tensor, a: Tensor, t: Tensor, rows: Tensor, level_start: Tensor, fixed: Tensor,
                           atom_start: Tensor, atom_items: Tensor, grad_x: Tensor,
                           grad_log_det_J: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    return ops.zmatrix_place_backward(x, d, a, t, rows, level_start, fixed, atom_start, atom_items, grad_x, grad_log_det_J)


zmatrix_place.register_fake(lambda d, a, t, x_fixed, rows, level_start, fixed, atom_start, atom_items: (
    d.new_empty((d.shape[0], 3 * (rows.shape[1] + fixed.shape[0]))), d.new_empty((d.shape[0],))))
zmatrix_place_backward.register_fake(lambda x, d, a, t, rows, level_start, fixed, *rest: (
    d.new_empty(d.shape), d.new_empty(d.shape), d.new_empty(d.shape), d.new_empty((d.shape[0], 3 * fixed.shape[0]))))


def _zmatrix_place_setup(ctx, inputs, output):
    d, a, t, _, *tables = inputs
    ctx.save_for_backward(output[0], d, a, t, *tables)
    ctx.like = tuple(_meta(o) for o in output)


def _zmatrix_place_bwd(ctx, g_x, g_l):
    grads = (_or_zeros(g, like) for g, like in zip((g_x, g_l), ctx.like))
    return (*torch.ops.tfep.zmatrix_place_backward(*ctx.saved_tensors, *grads), *([None] * 5))


zmatrix_place.register_autograd(_zmatrix_place_bwd, setup_context=_zmatrix_place_setup)


# ============================================================================= relative frame of the mixed coordinates

@custom_op('tfep::relative_frame_encode', mutates_args=(), device_types=_DEV)
def relative_frame_encode(x_cart: Tensor, remove_origin: bool, remove_axis: bool,
                          remove_plane: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``(coords, origin, R, log_det_J)`` of the rows ``x_cart`` (B, 3 n_c), whose last three atoms are the origin, axis and
    plane atoms: ``[d01, d02, a102n | the other atoms in the frame | kept reference DOFs]``, (B, 3), (B, 9), (B,).  float32
    or float64; fewer than 3 atoms is a ValueError."""
    return ops.relative_frame_encode(x_cart, (remove_origin, remove_axis, remove_plane))


@custom_op('tfep::relative_frame_encode_backward', mutates_args=(), device_types=_DEV)
def relative_frame_encode_backward(x_cart: Tensor, remove_origin: bool, remove_axis: bool, remove_plane: bool,
                                   grad_coords: Tensor, grad_origin: Tensor, grad_rot: Tensor,
                                   grad_log_det_J: Tensor) -> Tensor:
    return ops.relative_frame_encode_backward(x_cart, (remove_origin, remove_axis, remove_plane), grad_coords, grad_origin,
                                              grad_rot, grad_log_det_J)


@custom_op('tfep::relative_frame_decode', mutates_args=(), device_types=_DEV)
def relative_frame_decode(coords: Tensor, origin: Tensor, rot: Tensor, remove_origin: bool, remove_axis: bool,
                          remove_plane: bool) -> Tuple[Tensor, Tensor]:
    """``(x_cart, log_det_J)`` from the outputs of ``relative_frame_encode``; all of one dtype (else TypeError), a width of
    ``coords`` that disagrees with the flags is a ValueError."""
    return ops.relative_frame_decode(coords, origin, rot, (remove_origin, remove_axis, remove_plane))


@custom_op('tfep::relative_frame_decode_backward', mutates_args=(), device_types=_DEV)
def relative_frame_decode_backward(coords: Tensor, origin: Tensor, rot: Tensor, remove_origin: bool, remove_axis: bool,
                                   remove_plane: bool, grad_x_cart: Tensor,
                                   grad_log_det_J: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """``(g_coords, g_origin, g_R)``."""
    return ops.relative_frame_decode_backward(coords, origin, rot, (remove_origin, remove_axis, remove_plane), grad_x_cart,
                                              grad_log_det_J)


@relative_frame_encode.register_fake
def _(x_cart, remove_origin, remove_axis, remove_plane):
    B, n_c = x_cart.shape[0], x_cart.shape[1] // 3
    width = ops.relative_frame_width(n_c, (remove_origin, remove_axis, remove_plane))
    return x_cart.new_empty((B, width)), x_cart.new_empty((B, 3)), x_cart.new_empty((B, 9)), x_cart.new_empty((B,))


@relative_frame_decode.register_fake
def _(coords, origin, rot, remove_origin, remove_axis, remove_plane):
    n_c = 3 + (coords.shape[1] - ops.relative_frame_width(3, (remove_origin, remove_axis, remove_plane))) // 3
    return coords.new_empty((coords.shape[0], 3 * n_c)), coords.new_empty((coords.shape[0],))


relative_frame_encode_backward.register_fake(lambda x_cart, *rest: x_cart.new_empty(x_cart.shape))
relative_frame_decode_backward.register_fake(lambda coords, origin, rot, *rest: (
    coords.new_empty(coords.shape), origin.new_empty(origin.shape), rot.new_empty(rot.shape)))


def _relative_frame_encode_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])
    ctx.remove = tuple(inputs[1:])
    ctx.like = tuple(_meta(o) for o in output)


def _relative_frame_encode_bwd(ctx, g_coords, g_origin, g_rot, g_l):
    (x_cart,) = ctx.saved_tensors
    grads = (_or_zeros(g, like) for g, like in zip((g_coords, g_origin, g_rot, g_l), ctx.like))
    return torch.ops.tfep.relative_frame_encode_backward(x_cart, *ctx.remove, *grads), None, None, None


def _relative_frame_decode_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:3])
    ctx.remove = tuple(inputs[3:])
    ctx.like = tuple(_meta(o) for o in output)


def _relative_frame_decode_bwd(ctx, g_x, g_l):
    grads = (_or_zeros(g, like) for g, like in zip((g_x, g_l), ctx.like))
    return (*torch.ops.tfep.relative_frame_decode_backward(*ctx.saved_tensors, *ctx.remove, *grads), None, None, None)


relative_frame_encode.register_autograd(_relative_frame_encode_bwd, setup_context=_relative_frame_encode_setup)
relative_frame_decode.register_autograd(_relative_frame_decode_bwd, setup_context=_relative_frame_decode_setup)


# ============================================================================= radial expansion, segment sum

@custom_op('tfep::radial_expansion', mutates_args=(), device_types=_DEV)
def radial_expansion(r: Tensor, means: Tensor, log_gammas: Tensor, r_cutoff: float, switching: bool,
                     force_zero: bool) -> Tensor:
    """``(*r.shape, K)``: the Gaussian basis of ``GaussianBasisExpansion``, times the Behler-Parrinello switch with
    ``switching``.  float32 or float64, the dtype of ``r``; ``means`` / ``log_gammas`` of another dtype are a TypeError."""
    return ops.radial_expansion(r, means, log_gammas, r_cutoff, switching, force_zero)


@custom_op('tfep::radial_expansion_backward', mutates_args=(), device_types=_DEV)
def radial_expansion_backward(r: Tensor, means: Tensor, log_gammas: Tensor, grad_out: Tensor, r_cutoff: float,
                              switching: bool, force_zero: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """``(g_r, g_means, g_log_gammas)``; bit-reproducible (no atomics)."""
    return ops.radial_expansion_backward(r, means, log_gammas, grad_out, r_cutoff, switching, force_zero)


@custom_op('tfep::segment_sum', mutates_args=(), device_types=_DEV)
def segment_sum(data: Tensor, segment_ids: Tensor, n_segments: int) -> Tensor:
    """``unsorted_segment_sum``: ``(n_segments, n_columns)`` of the dtype of ``data`` (float32 or float64); rows whose id is
    outside ``[0, n_segments)`` are skipped."""
    return ops.segment_sum(data, segment_ids, n_segments)


@custom_op('tfep::segment_gather', mutates_args=(), device_types=_DEV)
def segment_gather(grad_out: Tensor, segment_ids: Tensor) -> Tensor:
    """VJP of ``segment_sum``: ``grad_out[segment_ids]``, zero rows where the id names no segment."""
    return ops.segment_gather(grad_out, segment_ids)


radial_expansion.register_fake(lambda r, means, *rest: r.new_empty((*r.shape, means.shape[0])))
radial_expansion_backward.register_fake(lambda r, means, log_gammas, *rest: (
    r.new_empty(r.shape), means.new_empty(means.shape), log_gammas.new_empty(log_gammas.shape)))
segment_sum.register_fake(lambda data, segment_ids, n_segments: data.new_empty((n_segments, data.shape[1])))
segment_gather.register_fake(lambda grad_out, segment_ids: grad_out.new_empty((segment_ids.shape[0], grad_out.shape[1])))


def _radial_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:3])
    ctx.cfg = tuple(inputs[3:])


# (first derivatives only: the VJP kernels have no VJP of their own, and a second backward raises instead of returning zeros)
@torch.autograd.function.once_differentiable
def _radial_bwd(ctx, g):
    g_r, g_means, g_lg = torch.ops.tfep.radial_expansion_backward(*ctx.saved_tensors, g, *ctx.cfg)
    return g_r, g_means, g_lg, None, None, None


def _segment_sum_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1])


@torch.autograd.function.once_differentiable
def _segment_sum_bwd(ctx, g):
    (ids,) = ctx.saved_tensors
    return torch.ops.tfep.segment_gather(g, ids), None, None


radial_expansion.register_autograd(_radial_bwd, setup_context=_radial_setup)
segment_sum.register_autograd(_segment_sum_bwd, setup_context=_segment_sum_setup)


# ============================================================================= edge geometry, pruning

@custom_op('tfep::edge_geometry', mutates_args=(), device_types=_DEV)
def edge_geometry(x: Tensor, edges: Tensor, normalize: bool, inverse: bool) -> Tuple[Tensor, Tensor]:
    """``(distances (E,), directions (E, 3))`` of the edges ``(2, E)`` (integers, validated on the host: ValueError) over the
    nodes ``x`` (n_nodes, 3): ``x[edges[1]] - x[edges[0]]``, negated with ``inverse``, divided by its length with
    ``normalize``.  float32 or float64, the dtype of ``x``."""
    return ops.edge_geometry(x, edges, normalize, inverse)


@custom_op('tfep::edge_geometry_backward', mutates_args=(), device_types=_DEV)
def edge_geometry_backward(x: Tensor, edges: Tensor, grad_distances: Optional[Tensor], grad_directions: Optional[Tensor],
                           normalize: bool, inverse: bool) -> Tensor:
    """The cotangent of ``x``; a missing cotangent is a zero.  Bit-reproducible (no atomics), and the rows of a sample do not
    depend on the rest of the batch."""
    return ops.edge_geometry_backward(x, edges, grad_distances, grad_directions, normalize, inverse)


@custom_op('tfep::edge_prune', mutates_args=(), device_types=_DEV)
def edge_prune(distances: Tensor, r_cutoff: float) -> Tensor:
    """``keep_index``: the ids of the edges with ``distances <= r_cutoff``, ascending, int64.  Not differentiable."""
    return ops.edge_prune(distances, r_cutoff)


@custom_op('tfep::edge_select', mutates_args=(), device_types=_DEV)
def edge_select(data: Tensor, keep_index: Tensor) -> Tensor:
    """``data[keep_index]`` of a float32 / float64 tensor with one leading row per edge (the row gather
    ``tfep_segment_gather``); its VJP is the segment sum."""
    flat = ops.segment_gather(data.reshape(data.shape[0], _row_width(data.shape)), keep_index)
    return flat.reshape(keep_index.shape[0], *data.shape[1:])


def _row_width(shape):
    width = 1
    for n in shape[1:]:
        width *= n
    return width


edge_geometry.register_fake(lambda x, edges, normalize, inverse: (
    x.new_empty((edges.shape[1],)), x.new_empty((edges.shape[1], 3))))
edge_geometry_backward.register_fake(lambda x, *rest: x.new_empty(x.shape))
edge_select.register_fake(lambda data, keep_index: data.new_empty((keep_index.shape[0], *data.shape[1:])))


@edge_prune.register_fake
def _(distances, r_cutoff):
    n_kept = torch.library.get_ctx().new_dynamic_size()
    return distances.new_empty((n_kept,), dtype=torch.int64)


def _edge_geometry_setup(ctx, inputs, output):
    ctx.set_materialize_grads(False)                                 # an unused output reaches the kernel as NULL
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.flags = tuple(inputs[2:])


@torch.autograd.function.once_differentiable
def _edge_geometry_bwd(ctx, g_distances, g_directions):
    x, edges = ctx.saved_tensors
    return torch.ops.tfep.edge_geometry_backward(x, edges, g_distances, g_directions, *ctx.flags), None, None, None


def _edge_select_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1])
    ctx.shape = tuple(inputs[0].shape)


@torch.autograd.function.once_differentiable
def _edge_select_bwd(ctx, g):
    (keep_index,) = ctx.saved_tensors
    flat = torch.ops.tfep.segment_sum(g.reshape(g.shape[0], _row_width(ctx.shape)), keep_index, ctx.shape[0])
    return flat.reshape(ctx.shape), None


edge_geometry.register_autograd(_edge_geometry_bwd, setup_context=_edge_geometry_setup)
edge_select.register_autograd(_edge_select_bwd, setup_context=_edge_select_setup)


# ============================================================================= masked linear

@custom_op('tfep::masked_linear', mutates_args=(), device_types=_DEV)
def masked_linear(input: Tensor, weight: Tensor, bias: Optional[Tensor], mask: Optional[Tensor],
                  weight_g: Optional[Tensor]) -> Tensor:
    x2 = input.reshape(-1, input.shape[-1])
    n_out, k = weight.shape
    # (F.linear's shape errors: a narrower input would otherwise be zero padded up to the tile size without a word)
    if input.shape[-1] != k:
        raise RuntimeError(f'masked_linear: input has {input.shape[-1]} features, weight is {n_out} x {k}')
    if mask is not None and tuple(mask.shape) != (n_out, k):
        raise RuntimeError(f'masked_linear: mask is {tuple(mask.shape)}, weight is {n_out} x {k}')
    if bias is not None and bias.numel() != n_out:
        raise RuntimeError(f'masked_linear: bias has {bias.numel()} entries for {n_out} output features')
    if weight_g is not None and weight_g.numel() != n_out:
        raise RuntimeError(f'masked_linear: weight_g has {weight_g.numel()} entries for {n_out} output features')
    # (float64 parameters: the fp64-MFMA GEMM; input and parameters of one dtype, else TypeError)
    y = ops.masked_linear_layer(x2, weight, weight_g, mask, bias)[0]
    return y.reshape(*input.shape[:-1], n_out)


@masked_linear.register_fake
def _(input, weight, bias, mask, weight_g):
    return input.new_empty((*input.shape[:-1], weight.shape[0]))


@custom_op('tfep::masked_linear_backward', mutates_args=(), device_types=_DEV)
def masked_linear_backward(grad_output: Tensor, input: Tensor, weight: Tensor, mask: Optional[Tensor],
                           weight_g: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``(grad_input, grad_weight, grad_bias, grad_weight_g)``; grad_weight_g is empty (0 elements) without weight norm."""
    n_out, k = weight.shape
    xp, w = ops.masked_linear_operands(input.reshape(-1, k), weight, weight_g, mask)      # (the op saved them unpacked)
    gi, gv, gg, gb = ops.masked_linear_layer_backward(grad_output, xp, w, weight, weight_g, mask, n_out, k)
    gg = gg.reshape(n_out, 1) if weight_g is not None else weight.new_empty((0,))
    return gi.reshape(input.shape).contiguous(), gv, gb, gg


@masked_linear_backward.register_fake
def _(grad_output, input, weight, mask, weight_g):
    n_out = weight.shape[0]
    gg = weight.new_empty((n_out, 1)) if weight_g is not None else weight.new_empty((0,))
    return input.new_empty(input.shape), weight.new_empty(weight.shape), weight.new_empty((n_out,)), gg


def _ml_setup(ctx, inputs, output):
    input, weight, bias, mask, weight_g = inputs
    ctx.save_for_backward(input, weight, mask, weight_g)
    ctx.has_bias = bias is not None


def _ml_bwd(ctx, grad_output):
    input, weight, mask, weight_g = ctx.saved_tensors
    gi, gw, gb, gg = torch.ops.tfep.masked_linear_backward(grad_output.contiguous(), input, weight, mask, weight_g)
    return gi, gw, (gb if ctx.has_bias else None), None, (gg if weight_g is not None else None)


masked_linear.register_autograd(_ml_bwd, setup_context=_ml_setup)


# ============================================================================= fused MADE output layer + transformer

def _fused_launch(h, h_inv_scale, w, w_inv_scale, bias, k_ranges, tile_order, kind, x, y, feat_index, feat_tr, n_slots,
                  n_rows, x0, xf, y0, yf, n_bins, circular, identity_boundary_slopes, learn_lower_bound, learn_upper_bound,
                  min_bin_size, min_slope):
    x, ldx = _lib.rows(x, 'x')
    B, D = x.shape
    if y.shape != x.shape or y.stride(-1) != 1 or (B > 1 and y.stride(0) != D):
        raise RuntimeError('fused_output_transformer: y must be a contiguous tensor of the shape of x')
    ldj = torch.empty(B, dtype=torch.float32, device=x.device)
    ws = torch.empty(n_slots // 16, B, dtype=torch.float64, device=x.device)
    desc = None
    if kind == 1:
        desc = _spline_cfg(x0, xf, y0, yf, n_bins, circular, identity_boundary_slopes, learn_lower_bound,
                           learn_upper_bound, min_bin_size, min_slope).desc
    elif kind == 3:
        desc = ops.sos_fused_desc(n_bins)                 # SOS: n_bins = number of polynomials
    tail = (_lib.ptr(bias), _lib.ptr(k_ranges), _lib.ptr(tile_order), kind,
            ctypes.byref(desc) if desc is not None else None,
            _lib.ptr(x), ldx, _lib.ptr(y), D, _lib.ptr(feat_index), _lib.ptr(feat_tr),
            n_slots, _lib.ptr(ws), _lib.ptr(ldj), 0, B, n_rows, w.shape[1], _lib.stream_of(x))
    if h_inv_scale is not None:
        _lib.call('tfep_fused_output_transformer_forward_split', _lib.ptr(h), h.shape[1], _lib.ptr(h_inv_scale),
                  _lib.ptr(w), w.shape[1], _lib.ptr(w_inv_scale), *tail)
    else:
        _lib.call('tfep_fused_output_transformer_forward', _lib.ptr(h), h.shape[1], _lib.ptr(w), w.shape[1], *tail)
    return ldj


@custom_op('tfep::fused_output_transformer', mutates_args=(), device_types=_DEV)
def fused_output_transformer(h: Tensor, h_inv_scale: Optional[Tensor], w: Tensor, w_inv_scale: Optional[Tensor],
                             bias: Tensor, k_ranges: Tensor, tile_order: Tensor, kind: int, x: Tensor, y_init: Optional[Tensor],
                             feat_index: Tensor, feat_tr: Tensor, n_slots: int, n_rows: int,
                             x0: Optional[Tensor], xf: Optional[Tensor], y0: Optional[Tensor], yf: Optional[Tensor],
                             n_bins: int, circular: bool, identity_boundary_slopes: bool, learn_lower_bound: bool,
                             learn_upper_bound: bool, min_bin_size: float, min_slope: float) -> Tuple[Tensor, Tensor]:
    """``tfep_fused_output_transformer_forward[_split]``: the MADE output-layer GEMM with the affine (kind 0), RQ-spline
    (kind 1) or SOS (kind 3, ``n_bins`` = number of polynomials) transformer and the log-det in its epilogue.  ``h`` / ``w``: last hidden activations and packed output
    weights -- split-f16 rows when ``h_inv_scale`` / ``w_inv_scale`` are given, fp32 otherwise.  ``y_init``: the input
    with its fixed features (copied through), or None when every feature is transformed."""
    y = y_init.clone() if y_init is not None else torch.empty(x.shape, dtype=x.dtype, device=x.device)
    ldj = _fused_launch(h, h_inv_scale, w, w_inv_scale, bias, k_ranges, tile_order, kind, x, y, feat_index, feat_tr, n_slots,
                        n_rows, x0, xf, y0, yf, n_bins, circular, identity_boundary_slopes, learn_lower_bound,
                        learn_upper_bound, min_bin_size, min_slope)
    return y, ldj


@fused_output_transformer.register_fake
def _(h, h_inv_scale, w, w_inv_scale, bias, k_ranges, tile_order, kind, x, y_init, *rest):
    return x.new_empty(x.shape), x.new_empty((x.shape[0],))


@custom_op('tfep::fused_output_transformer_', mutates_args=('y',), device_types=_DEV)
def fused_output_transformer_(h: Tensor, h_inv_scale: Optional[Tensor], w: Tensor, w_inv_scale: Optional[Tensor],
                              bias: Tensor, k_ranges: Tensor, tile_order: Tensor, kind: int, x: Tensor, y: Tensor,
                              feat_index: Tensor, feat_tr: Tensor, n_slots: int, n_rows: int,
                              x0: Optional[Tensor], xf: Optional[Tensor], y0: Optional[Tensor], yf: Optional[Tensor],
                              n_bins: int, circular: bool, identity_boundary_slopes: bool, learn_lower_bound: bool,
                              learn_upper_bound: bool, min_bin_size: float, min_slope: float) -> Tensor:
    """The same launch writing the columns ``feat_index`` of an existing ``y`` (in place) and returning the log-det of
    those features: the groups of a mixed transformer are one launch each on their rows of the packed weights."""
    return _fused_launch(h, h_inv_scale, w, w_inv_scale, bias, k_ranges, tile_order, kind, x, y, feat_index, feat_tr, n_slots,
                         n_rows, x0, xf, y0, yf, n_bins, circular, identity_boundary_slopes, learn_lower_bound,
                         learn_upper_bound, min_bin_size, min_slope)


@fused_output_transformer_.register_fake
def _(h, h_inv_scale, w, w_inv_scale, bias, k_ranges, tile_order, kind, x, y, *rest):
    return x.new_empty((x.shape[0],))


# ============================================================================= TFEP reductions

@custom_op('tfep::tfep_reduce', mutates_args=(), device_types=_DEV)
def tfep_reduce(target_potentials: Tensor, log_det_J: Optional[Tensor], ref_potentials: Optional[Tensor],
                log_weights: Optional[Tensor], bias: Optional[Tensor], kT: float, ignore_nan: bool) -> Tensor:
    return ops.tfep_reduce(target_potentials, log_det_J, ref_potentials, log_weights, bias, kT=kT, ignore_nan=ignore_nan)


@tfep_reduce.register_fake
def _(target_potentials, log_det_J, ref_potentials, log_weights, bias, kT, ignore_nan):
    return target_potentials.new_empty((9,), dtype=torch.float64)


OPS = ('affine_forward', 'affine_inverse', 'affine_backward', 'spline_forward', 'spline_inverse', 'spline_backward',
       'moebius_forward', 'moebius_inverse', 'moebius_backward', 'masked_linear', 'masked_linear_backward',
       'fused_output_transformer', 'fused_output_transformer_', 'tfep_reduce')
# (a tuple of their own: OPS is the list the existing op tests iterate over)
SOS_OPS = ('sos_forward', 'sos_backward')
SYMMETRIZED_MOEBIUS_OPS = ('symmetrized_moebius_forward', 'symmetrized_moebius_inverse', 'symmetrized_moebius_backward')
QUATERNION_PRODUCT_OPS = ('quaternion_product_forward', 'quaternion_product_inverse', 'quaternion_product_backward')
FLIP_EMBEDDING_OPS = ('flip_invariant_embedding', 'flip_invariant_embedding_backward')
FRAME_OPS = ('centroid_shift', 'centroid_restore', 'frame_orient', 'frame_rotate', 'centroid_shift_backward',
             'centroid_restore_backward', 'frame_orient_backward', 'frame_rotate_backward')
GEOMETRY_OPS = ('internal_coordinates', 'internal_coordinates_backward', 'polar_forward', 'polar_backward')
ZMATRIX_OPS = ('zmatrix_place', 'zmatrix_place_backward')
RELATIVE_FRAME_OPS = ('relative_frame_encode', 'relative_frame_decode', 'relative_frame_encode_backward',
                      'relative_frame_decode_backward')
GRAPH_OPS = ('radial_expansion', 'radial_expansion_backward', 'segment_sum', 'segment_gather')
EDGE_OPS = ('edge_geometry', 'edge_geometry_backward', 'edge_prune', 'edge_select')
