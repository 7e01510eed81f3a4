"""Geometry of point coordinates (reference ``tfep/utils/geometry.py``): internal coordinates, rotations, rigid
frames, the polar map.

Rigid frames: only what ``OrientedFlow`` / ``CenteredCentroidFlow`` need.  The reference composes two Rodrigues
rotations from angles (acos / asin / sin / cos); here both rotations are written in closed form from dot
and cross products, which gives the same matrices without the inverse-trig round trip and stays
differentiable.  These are O(batch) 3x3 operations around the hot path and run as
ordinary torch ops on the input's device.

Internal coordinates: ``internal_coordinates`` (and ``pdist`` without ``return_diff``) compute distances, angles and
dihedrals from point INDICES in one HIP launch, forward and backward (``csrc/geometry.hip``; HIP tensors only).  The
functions that take difference VECTORS (``vector_vector_angle``, ``vector_plane_angle``, ``proper_dihedral_angle``) and
``rotation_matrix_3d`` are torch expressions on the device of their inputs, which are materialised already.
``cartesian_to_polar`` / ``polar_to_cartesian`` run on the element-wise polar kernel.

Z-matrices: ``cartesian_to_zmatrix`` is ``internal_coordinates`` on the tables of a Z-matrix, ``zmatrix_to_cartesian`` places
the atoms back, level by level of the dependency graph, in one HIP launch forward and one backward (``csrc/zmatrix.hip``);
each returns the log-det of its direction.  The reference takes this step from ``bgflow``.

Relative frame: ``cartesian_to_relative_frame`` / ``relative_frame_to_cartesian`` express the Cartesian atoms of the mixed
coordinates in the frame of three of them and back, one HIP launch each way and one for each backward
(``csrc/relframe.hip``); ``normalize_angles`` / ``normalize_torsions`` and their inverses are torch expressions.
"""
import math
from functools import lru_cache
from typing import Optional, Tuple

import torch

from .. import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.tfep.*)
from .math import batchwise_dot, batchwise_outer


# ----------------------------------------------------------------------------- internal coordinates

@lru_cache(maxsize=8)
def _all_pairs(n_particles):
    """The (2, n (n - 1) / 2) table of all pairs: one tensor per size, so ``ops.index_tables`` prepares it once."""
    return torch.triu_indices(n_particles, n_particles, offset=1)


def internal_coordinates(x, pairs=None, triples=None, quads=None):
    """Distances, angles and proper dihedrals of a batch of configurations from atom indices, in one HIP launch.

    ``x``: positions, ``(batch_size, n_particles, 3)`` or flattened ``(batch_size, 3 * n_particles)``, a float32 or float64
    HIP tensor (a column slice of a wider tensor is read in place).  ``pairs`` ``(2, P)``, ``triples`` ``(3, A)``,
    ``quads`` ``(4, T)``: integer index tables on any device (validated on the host, ValueError on an index outside
    ``[0, n_particles)``; pass the same tensor object at every call and it is validated and uploaded once).

    Returns ``(d, a, t)`` of shapes ``(batch_size, P)``, ``(batch_size, A)``, ``(batch_size, T)``; a table not given has
    no columns.  ``d[b, i]`` is the distance of atoms ``pairs[0, i]`` and ``pairs[1, i]``; ``a[b, i]`` the angle in
    ``[0, pi]`` at atom ``triples[1, i]`` -- ``vector_vector_angle(p0 - p1, p2 - p1)`` --; ``t[b, i]`` the dihedral in
    ``(-pi, pi]`` of the four atoms of ``quads[:, i]`` -- ``proper_dihedral_angle(p1 - p0, p2 - p1, p3 - p2)``, zero for
    collinear atoms.  Differentiable in ``x``; the backward is one launch and reproducible bit for bit.
    """
    if x.dim() == 3 and x.shape[2] == 3:
        x = x.reshape(x.shape[0], -1)
    if x.dim() != 2 or x.shape[1] % 3 != 0:
        raise ValueError(f'x must be (batch, n_particles, 3) or (batch, 3 n_particles), got {tuple(x.shape)}')
    tables = ops.index_tables(pairs, triples, quads, x.shape[1] // 3, x.device)
    return torch.ops.tfep.internal_coordinates(x, *tables)


def pdist(x, pairs=None, return_diff=False):
    """Euclidean distances between pairs of particles of ``x`` ``(batch_size, n_particles, D)`` (reference
    geometry.py:28-68).  ``pairs``: ``(2, n_pairs)`` indices, all pairs when not given.  Returns ``(batch_size, n_pairs)``
    and, with ``return_diff``, the vectors ``p1 - p0`` as ``(batch_size, n_pairs, D)``.

    Without ``return_diff`` this is ``internal_coordinates`` (D = 3, HIP tensors); with it a torch expression, the
    difference tensor being a result anyway."""
    if pairs is None:
        pairs = _all_pairs(x.shape[-2])
    if return_diff:
        pairs = torch.as_tensor(pairs, device=x.device)
        diff = x[:, pairs[1]] - x[:, pairs[0]]
        return torch.sqrt(torch.sum(diff ** 2, dim=-1)), diff
    if x.dim() != 3 or x.shape[2] != 3:
        raise ValueError(f'pdist without return_diff takes (batch, n_particles, 3) positions, got {tuple(x.shape)}')
    return internal_coordinates(x, pairs=pairs)[0]


def _n_atoms(z_matrix, fixed_atoms):
    return len(z_matrix) + len(fixed_atoms)


def zmatrix_to_cartesian(d, a, t, x_fixed, z_matrix, fixed_atoms):
    """Place the atoms of a batch of configurations from a Z-matrix, in one HIP launch: the inverse of
    ``cartesian_to_zmatrix``.

    ``z_matrix``: ``(n_ic, 4)`` integer rows ``(i, j, k, l)`` in any order -- atom ``i`` is placed at distance ``d`` from
    ``j``, angle ``a`` (``i``-``j``-``k``) and dihedral ``t`` (``i``-``j``-``k``-``l``), in the conventions of
    ``internal_coordinates``.  ``fixed_atoms``: ``(n_fixed,)`` the atoms whose positions are given, at least three; fixed
    and placed atoms together are all ``n_ic + n_fixed`` atoms.  Both on any device, validated on the host (ValueError;
    ``ops.check_zmatrix``); pass the same tensor objects at every call and they are validated and uploaded once.
    ``d``, ``a``, ``t``: ``(batch_size, n_ic)``, column ``c`` for row ``c`` of ``z_matrix``; ``x_fixed``: ``(batch_size,
    n_fixed, 3)`` or ``(batch_size, 3 n_fixed)`` in the order of ``fixed_atoms``.  float32 or float64 HIP tensors of one
    dtype (column slices of wider tensors are read in place).

    Returns ``(x, log_det_J)``: the positions in the layout of ``x_fixed`` with all atoms, and the log absolute Jacobian
    determinant ``sum(2 log d + log|sin a|)`` of ``(d, a, t, x_fixed) -> x``.  Differentiable in ``d``, ``a``, ``t`` and
    ``x_fixed``; the backward is one launch and reproducible bit for bit.  Degenerate input (``d = 0``, ``sin a = 0``,
    collinear reference atoms) gives NaN or infinite values."""
    atoms_3d = x_fixed.dim() == 3 and x_fixed.shape[2] == 3
    if atoms_3d:
        x_fixed = x_fixed.reshape(x_fixed.shape[0], -1)
    if x_fixed.dim() != 2 or x_fixed.shape[1] != 3 * len(fixed_atoms):
        raise ValueError(f'x_fixed must be (batch, {len(fixed_atoms)}, 3) or (batch, {3 * len(fixed_atoms)}), got '
                         f'{tuple(x_fixed.shape)}')
    tables = ops.zmatrix_tables(z_matrix, fixed_atoms, _n_atoms(z_matrix, fixed_atoms), x_fixed.device)
    for v, name in ((d, 'd'), (a, 'a'), (t, 't'), (x_fixed, 'x_fixed')):          # one dtype, on the HIP device
        ops.check_device_tensor(v, name, ops._dtype(d))
    x, log_det_J = torch.ops.tfep.zmatrix_place(d, a, t, x_fixed, *tables)
    return (x.reshape(x.shape[0], -1, 3) if atoms_3d else x), log_det_J


def cartesian_to_zmatrix(x, z_matrix, fixed_atoms):
    """The internal coordinates of a Z-matrix, on the ``internal_coordinates`` kernel: the inverse of
    ``zmatrix_to_cartesian`` (see there for ``z_matrix`` and ``fixed_atoms``).

    ``x``: ``(batch_size, n_atoms, 3)`` or ``(batch_size, 3 n_atoms)``, float32 or float64 HIP tensor.  Returns ``(d, a, t,
    x_fixed, log_det_J)``: ``d``, ``a``, ``t`` ``(batch_size, n_ic)`` in the row order of ``z_matrix``, ``a`` in ``[0, pi]``
    and ``t`` in ``(-pi, pi]``; ``x_fixed`` the positions of ``fixed_atoms`` in the layout of ``x``; and the log absolute
    Jacobian determinant ``-sum(2 log d + log|sin a|)`` of ``x -> (d, a, t, x_fixed)``.  Differentiable in ``x``."""
    atoms_3d = x.dim() == 3 and x.shape[2] == 3
    if atoms_3d:
        x = x.reshape(x.shape[0], -1)
    n_atoms = _n_atoms(z_matrix, fixed_atoms)
    if x.dim() != 2 or x.shape[1] != 3 * n_atoms:
        raise ValueError(f'x must be (batch, {n_atoms}, 3) or (batch, {3 * n_atoms}), got {tuple(x.shape)}')
    tables, fixed = ops.zmatrix_index_tables(z_matrix, fixed_atoms, n_atoms, x.device)
    ops.check_device_tensor(x, 'x', ops._dtype(x))
    d, a, t = torch.ops.tfep.internal_coordinates(x, *tables)
    x_fixed = x.reshape(x.shape[0], n_atoms, 3).index_select(1, fixed)
    log_det_J = -(2.0 * torch.log(d) + torch.log(torch.abs(torch.sin(a)))).sum(1)
    return d, a, t, (x_fixed if atoms_3d else x_fixed.reshape(x.shape[0], -1)), log_det_J


def _remove_flags(remove_ref_rototranslation):
    flags = torch.as_tensor(remove_ref_rototranslation).reshape(-1).tolist()
    if len(flags) != 3:
        raise ValueError(f'remove_ref_rototranslation must hold 3 flags (origin, axis, plane), got {len(flags)}')
    return tuple(bool(f) for f in flags)


def cartesian_to_relative_frame(x_cart, remove_ref_rototranslation):
    """The Cartesian atoms of a batch in the frame of three of them, in one HIP launch (``csrc/relframe.hip``): the
    relative frame of the reference's mixed coordinates (``app/mixedmaf.py:1216-1271``).

    ``x_cart``: ``(batch_size, n_c, 3)`` or ``(batch_size, 3 n_c)``, a float32 or float64 HIP tensor (a column slice of a
    wider tensor is read in place) whose LAST THREE atoms are the origin, axis and plane atoms, in that order; ``n_c >= 3``.
    The frame has the origin atom at 0, the axis atom on the positive x axis and the plane atom in the x-y plane (the
    rotation of ``reference_frame_rotation_matrix(..., project_on_positive_axis=True)``).
    ``remove_ref_rototranslation``: 3 flags, whether the rototranslational DOFs of the origin (3), axis (2) and plane (1) atom,
    which are zero in the frame, are left out.

    Returns ``(coords, origin, R, log_det_J)``.  ``coords`` ``(batch_size, W)``: ``[d01, d02, a102n | the n_c - 3 other atoms
    in the frame, 3 each | kept reference DOFs]`` with ``d01`` the axis atom's distance from the origin, ``(d02, a102)`` the
    polar coordinates of the plane atom, ``a102n = (a102 + pi) / (2 pi)`` in ``[0, 1]``, and the kept DOFs in the order
    origin ``x, y, z``, axis ``y, z``, plane ``z``.  ``origin`` ``(batch_size, 3)`` and ``R`` ``(batch_size, 3, 3)`` take the
    way back; ``log_det_J = -log d02 - log 2 pi``.  Differentiable in ``x_cart`` through all four outputs."""
    if x_cart.dim() == 3 and x_cart.shape[2] == 3:
        x_cart = x_cart.reshape(x_cart.shape[0], -1)
    if x_cart.dim() != 2 or x_cart.shape[1] % 3 != 0 or x_cart.shape[1] < 9:
        raise ValueError(f'x_cart must be (batch, n_c, 3) or (batch, 3 n_c) with n_c >= 3, got {tuple(x_cart.shape)}')
    remove = _remove_flags(remove_ref_rototranslation)
    ops.check_device_tensor(x_cart, 'x_cart', ops._dtype(x_cart))
    coords, origin, rot, log_det_J = torch.ops.tfep.relative_frame_encode(x_cart, *remove)
    return coords, origin, rot.reshape(-1, 3, 3), log_det_J


def relative_frame_to_cartesian(coords, origin, R, remove_ref_rototranslation):
    """The inverse of ``cartesian_to_relative_frame``, in one HIP launch (reference ``app/mixedmaf.py:1321-1375``).

    ``coords`` ``(batch_size, W)`` in the layout above (a column slice is read in place), ``origin`` ``(batch_size, 3)``,
    ``R`` ``(batch_size, 3, 3)``: float32 or float64 HIP tensors of one dtype (else TypeError).  A removed reference DOF is
    exactly 0 in the frame, a kept one is read from ``coords``; a width ``W`` that disagrees with the flags is a ValueError.

    Returns ``(x_cart, log_det_J)``: ``(batch_size, n_c, 3)`` and ``log 2 pi + log d02``.  Differentiable in ``coords``,
    ``origin`` and ``R``."""
    if coords.dim() != 2:
        raise ValueError(f'coords must be (batch, W), got {tuple(coords.shape)}')
    remove = _remove_flags(remove_ref_rototranslation)
    for v, name in ((coords, 'coords'), (origin, 'origin'), (R, 'R')):            # one dtype, on the HIP device
        ops.check_device_tensor(v, name, ops._dtype(coords))
    x, log_det_J = torch.ops.tfep.relative_frame_decode(coords, origin.reshape(coords.shape[0], 3),
                                                       R.reshape(coords.shape[0], 9), *remove)
    return x.reshape(x.shape[0], -1, 3), log_det_J


def _scaled(value, shift, scale):
    """``((value + shift) * scale, log_det_J)`` over the last dimension: the log-det is ``n log scale``."""
    log_det_J = torch.full(value.shape[:-1], value.shape[-1] * math.log(scale), dtype=value.dtype, device=value.device)
    return (value + shift) * scale, log_det_J


def normalize_angles(angles):
    """``(angles / pi, log_det_J)``: bond angles ``(*, n)`` in ``[0, pi]`` to ``[0, 1]``; ``log_det_J = -n log pi``, shape
    ``(*,)``.  (The reference takes this from ``bgflow``; these formulas are this project's definition.)"""
    return _scaled(angles, 0.0, 1.0 / math.pi)


def unnormalize_angles(angles):
    """The inverse of ``normalize_angles``: ``(angles * pi, +n log pi)``."""
    return _scaled(angles, 0.0, math.pi)


def normalize_torsions(torsions):
    """``((torsions + pi) / (2 pi), log_det_J)``: torsions ``(*, n)`` in ``[-pi, pi]`` to ``[0, 1]``; ``log_det_J = -n log
    2 pi``, shape ``(*,)``."""
    return _scaled(torsions, math.pi, 1.0 / (2.0 * math.pi))


def unnormalize_torsions(torsions):
    """The inverse of ``normalize_torsions``: ``(2 pi torsions - pi, +n log 2 pi)``."""
    value, log_det_J = _scaled(torsions, 0.0, 2.0 * math.pi)
    return value - math.pi, log_det_J


def vector_vector_angle(x1, x2):
    """Angle in ``[0, pi]`` between the vectors of ``x1`` and ``x2``, both ``(*, D)`` (reference geometry.py:71-99)."""
    cos_theta = batchwise_dot(x1, x2) / (torch.linalg.vector_norm(x1, dim=-1) * torch.linalg.vector_norm(x2, dim=-1))
    return torch.acos(torch.clamp(cos_theta, min=-1, max=1))       # (the clamp catches round-off)


def vector_plane_angle(x, plane):
    """Angle between the vectors ``x`` ``(batch_size, N)`` or ``(N,)`` and the plane of normal ``plane`` ``(N,)``
    (reference geometry.py:102-124)."""
    cos_theta = batchwise_dot(x, plane) / (torch.linalg.vector_norm(x, dim=-1) * torch.linalg.vector_norm(plane, dim=-1))
    return torch.asin(torch.clamp(cos_theta, min=-1, max=1))


def proper_dihedral_angle(x1, x2, x3):
    """Proper dihedral between the planes ``x1``-``x2`` and ``x2``-``x3`` for ``x1 = p1 - p0``, ``x2 = p2 - p1``,
    ``x3 = p3 - p2``, all ``(*, 3)`` (reference geometry.py:127-178): the angle, in the plane perpendicular to ``x2``,
    from the rejection of ``-x1`` to that of ``x3``."""
    x2 = x2 / torch.linalg.vector_norm(x2, dim=-1, keepdim=True)
    v = -x1 - batchwise_dot(-x1, x2, keepdim=True) * x2
    w = x3 - batchwise_dot(x3, x2, keepdim=True) * x2
    return torch.atan2(batchwise_dot(torch.linalg.cross(x2, v, dim=-1), w), batchwise_dot(v, w))


# ----------------------------------------------------------------------------- rotations and rigid frames

def rotation_matrix_3d(angles, directions):
    """Matrices ``(batch_size, 3, 3)`` rotating by ``angles`` ``(batch_size,)`` about ``directions`` ``(batch_size, 3)`` or
    ``(3,)``, by Rodrigues' formula (reference geometry.py:185-236)."""
    k = torch.nn.functional.normalize(directions, dim=-1)
    if k.dim() < 2:
        k = k.unsqueeze(0)
    k = k.expand(len(angles), 3)
    cosa = torch.cos(angles)[:, None, None]
    eye = torch.eye(3, dtype=angles.dtype, device=angles.device)
    return cosa * eye + (1 - cosa) * batchwise_outer(k, k) + _skew(torch.sin(angles).unsqueeze(-1) * k)


def get_axis_from_name(name: str) -> torch.Tensor:
    """Unit vector of the named Cartesian axis (reference geometry.py:279-293)."""
    try:
        i = 'xyz'.index(name)
    except ValueError:
        raise ValueError("'name' must be one of 'x', 'y', 'z'") from None
    v = torch.zeros(3)
    v[i] = 1.0
    return v


def _skew(w):
    """(B,3) -> (B,3,3) cross-product matrices [w]x."""
    z = torch.zeros_like(w[:, 0])
    return torch.stack([
        torch.stack([z, -w[:, 2], w[:, 1]], dim=1),
        torch.stack([w[:, 2], z, -w[:, 0]], dim=1),
        torch.stack([-w[:, 1], w[:, 0], z], dim=1),
    ], dim=1)


def batchwise_rotate(x: torch.Tensor, rotation_matrices: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """Rotate every point of ``x`` (B,N,3) by its sample's matrix (B,3,3) (reference geometry.py:239-276)."""
    if inverse:
        return torch.matmul(x, rotation_matrices)
    return torch.matmul(x, rotation_matrices.transpose(1, 2))


def reference_frame_rotation_matrix(
        axis_atom_positions: torch.Tensor,
        plane_atom_positions: torch.Tensor,
        axis: torch.Tensor,
        plane_axis: torch.Tensor,
        plane_normal: Optional[torch.Tensor] = None,
        project_on_positive_axis: bool = False,
) -> torch.Tensor:
    """Rotation matrices (B,3,3) that put one point on ``axis`` and another on the ``axis``/``plane_axis``
    plane (same contract as reference geometry.py:296-411).

    The first rotation is the minimal one taking the axis point's direction onto ``axis`` (or onto
    ``-axis`` when that is closer and ``project_on_positive_axis`` is False).  The second is about ``axis``
    and brings the plane point onto the nearest half of the ``plane_axis`` line, so the axis point stays put.
    """
    dtype = axis_atom_positions.dtype
    axis = axis.to(axis_atom_positions)
    plane_axis = plane_axis.to(axis_atom_positions)
    if plane_normal is None:
        plane_normal = torch.linalg.cross(axis, plane_axis, dim=0)
    plane_normal = plane_normal.to(axis_atom_positions)
    plane_normal = plane_normal / torch.linalg.vector_norm(plane_normal)
    eye = torch.eye(3, dtype=dtype, device=axis.device)

    # R1: minimal rotation u -> axis, with u = +-(unit axis point).
    u = axis_atom_positions / torch.linalg.vector_norm(axis_atom_positions, dim=1, keepdim=True)
    c = u @ axis
    if not project_on_positive_axis:
        flip = torch.where(c < 0, -torch.ones_like(c), torch.ones_like(c))
        u = u * flip.unsqueeze(1)
        c = c * flip
    w = torch.linalg.cross(u, axis.expand_as(u), dim=1)
    K = _skew(w)
    # Rodrigues with sin = |w|, cos = c:  I + [w]x + [w]x^2 / (1 + c).  For the antiparallel case
    # (only reachable with project_on_positive_axis=True) rotate by pi about plane_axis x axis.
    denom = 1.0 + c
    safe = denom > 1e-12
    r1 = eye + K + torch.matmul(K, K) / torch.where(safe, denom, torch.ones_like(denom))[:, None, None]
    if project_on_positive_axis:
        n = torch.linalg.cross(plane_axis, axis, dim=0)
        flip_pi = 2.0 * torch.outer(n, n) - eye
        r1 = torch.where(safe[:, None, None], r1, flip_pi)

    # R2: rotation about axis by phi with cos(phi) = |q_p|/|q|, sin(phi) = -sign(q_p) q_n/|q|, where
    # q is the rotated plane point projected perpendicular to axis.
    p = torch.matmul(r1, plane_atom_positions.unsqueeze(2)).squeeze(2)
    q_p = p @ plane_axis
    q_n = p @ plane_normal
    q_norm = torch.sqrt(q_p * q_p + q_n * q_n)
    sgn = torch.sign(q_p)
    cos2 = torch.where(sgn == 0, torch.ones_like(q_p), q_p.abs() / q_norm)
    sin2 = torch.where(sgn == 0, torch.zeros_like(q_p), -sgn * q_n / q_norm)
    aa = torch.outer(axis, axis)
    kx = _skew(axis.unsqueeze(0))[0]
    r2 = cos2[:, None, None] * eye + sin2[:, None, None] * kx + (1.0 - cos2)[:, None, None] * aa

    return torch.matmul(r2, r1)


# ----------------------------------------------------------------------------- polar coordinates

def cartesian_to_polar(x: torch.Tensor, y: torch.Tensor, return_log_det_J: bool = False) -> Tuple[torch.Tensor]:
    """``(r, angle)`` of the Cartesian ``(x, y)``, element-wise, and with ``return_log_det_J`` the log absolute Jacobian
    determinant of the map as the reference returns it, ``-log r`` (reference geometry.py:414-441).  HIP tensors."""
    r, angle, log_det_J = torch.ops.tfep.polar_forward(x, y, False, return_log_det_J)
    return (r, angle, log_det_J) if return_log_det_J else (r, angle)


def polar_to_cartesian(r: torch.Tensor, angle: torch.Tensor, return_log_det_J: bool = False) -> Tuple[torch.Tensor]:
    """``(x, y)`` of the polar ``(r, angle)``, element-wise, and with ``return_log_det_J`` also ``log r`` (reference
    geometry.py:444-471).  HIP tensors."""
    x, y, log_det_J = torch.ops.tfep.polar_forward(r, angle, True, return_log_det_J)
    return (x, y, log_det_J) if return_log_det_J else (x, y)
