"""Flow wrapper that maps mixed (internal + Cartesian) coordinates with the wrapped flow: the coordinate change of the
reference's ``MixedMAFMap`` (``app/mixedmaf.py:954-1381``, ``_CartesianToMixedFlow``).

Some atoms are described by the bonds, angles and torsions of a Z-matrix, the others stay Cartesian, in the frame of three
of them (the origin, axis and plane atoms).  Way in: ``cartesian_to_zmatrix`` (the ``internal_coordinates`` kernel), the
two normalisations to ``[0, 1]``, then ``cartesian_to_relative_frame`` (``csrc/relframe.hip``); way back:
``relative_frame_to_cartesian``, the un-normalisations, ``zmatrix_to_cartesian`` (``csrc/zmatrix.hip``).  One launch for
each kernel step and one more for its backward.  The reference takes the Z-matrix step and the normalisations from
``bgflow``, which is no dependency here.
"""
from typing import Dict, Optional, Tuple

import torch

from ... import ops
from ...utils import geometry
from ...utils.misc import atom_to_flattened_indices, ensure_tensor_sequence, remove_and_shift_sorted_indices


class CartesianToMixedFlow(torch.nn.Module):
    """Map ``x`` ``(batch_size, 3 n_atoms)`` or ``(batch_size, n_atoms, 3)`` through ``flow`` in mixed coordinates.

    ``cartesian_atom_indices``: ``(n_c,)`` the sorted atoms that stay Cartesian, the reference atoms among them.
    ``z_matrix``: ``(n_ic, 4)`` rows ``(i, j, k, l)`` for every other atom (``tfep_amd.utils.geometry.zmatrix_to_cartesian``).
    ``reference_atom_indices``: the origin, axis and plane atoms, in this order; they are moved to the end of the Cartesian
    atoms.  ``remove_ref_rototranslation``: 3 flags, whether the rototranslational DOFs of the origin (3), axis (2) and
    plane (1) atom -- all zero in the relative frame -- are kept out of what ``flow`` sees.

    ``flow`` maps ``n_dofs_out`` features laid out as ``[bonds | angles / pi | (torsions + pi) / 2 pi | d01 | d02 | a102n |
    cartesians | kept reference DOFs]``: ``n_ic`` of each internal coordinate in the row order of ``z_matrix``; the axis
    atom's distance ``d01`` from the origin, the plane atom's polar coordinates ``d02`` and ``a102n = (a102 + pi) / 2 pi``;
    the other Cartesian atoms in the relative frame, 3 each, in the order of ``cartesian_atom_indices``; and the reference
    DOFs that are not removed (origin ``x, y, z``, axis ``y, z``, plane ``z``).  ``get_dof_indices_by_type`` names the columns.

    ``forward`` converts, runs ``flow``, converts back and returns ``(y, log_det_J)`` with all log-dets added; ``inverse``
    does the same with ``flow.inverse``.  The origin and the rotation of the way in are carried to the way back with their
    gradients.  Keeping distances positive and the normalised angles inside ``(0, 1)`` is the wrapped flow's concern (a
    spline over ``[0, 1]``, for instance).  Eager only: the host-side table lookup is not captured by ``GraphedFlow``.
    """

    def __init__(self, flow: torch.nn.Module, cartesian_atom_indices, z_matrix, reference_atom_indices,
                 remove_ref_rototranslation):
        super().__init__()
        self.flow = flow
        remove = torch.as_tensor(remove_ref_rototranslation)
        if remove.numel() != 3:
            raise ValueError(f'remove_ref_rototranslation must hold 3 flags, got {remove.numel()}')
        self.register_buffer('remove_ref_rototranslation', remove.reshape(3).bool())
        self._remove_host = (None, None)

        z_matrix = ensure_tensor_sequence(z_matrix).reshape(-1, 4)
        cartesian = ensure_tensor_sequence(cartesian_atom_indices)
        reference = ensure_tensor_sequence(reference_atom_indices)
        if reference.dim() != 1 or len(reference) != 3 or len(set(reference.tolist())) != 3:
            raise ValueError(f'reference_atom_indices must be three distinct atoms (origin, axis, plane), got '
                             f'{reference.tolist()}')
        if not set(reference.tolist()) <= set(cartesian.tolist()):
            raise ValueError(f'the reference atoms {reference.tolist()} must be Cartesian atoms')
        n_atoms = len(cartesian) + len(z_matrix)
        listed = sorted(cartesian.tolist() + z_matrix[:, 0].tolist())
        if listed != list(range(n_atoms)):
            raise ValueError(f'the Cartesian atoms and the atoms placed by the Z-matrix must be every one of the {n_atoms} '
                             'atoms exactly once')
        # the reference atoms go last, in their own order
        cartesian = remove_and_shift_sorted_indices(cartesian, removed_indices=reference.sort().values, remove=True,
                                                    shift=False)
        cartesian = torch.cat([cartesian, reference.to(cartesian.dtype)])
        ops.check_zmatrix(z_matrix, cartesian, n_atoms)
        self.register_buffer('_z_matrix', z_matrix)
        self.register_buffer('_cartesian_atom_indices', cartesian)

    @property
    def cartesian_atom_indices(self) -> torch.Tensor:
        """The atoms in Cartesian coordinates, the origin, axis and plane atoms last."""
        return self._cartesian_atom_indices

    @property
    def z_matrix(self) -> torch.Tensor:
        return self._z_matrix

    @property
    def n_ic_atoms(self) -> int:
        """The number of atoms in internal coordinates (the reference atoms are not among them)."""
        return len(self._z_matrix)

    @property
    def n_dofs_out(self) -> int:
        """The number of mixed coordinates."""
        return self._splits()[-1]

    def n_parameters(self):
        """int: The total number of parameters that can be optimized."""
        return self.flow.n_parameters()

    def _remove(self) -> Tuple[bool, bool, bool]:
        """The three flags on the host; read from the buffer again only when it is another tensor or was written to."""
        flags = self.remove_ref_rototranslation
        key = (id(flags), flags._version)
        if self._remove_host[0] != key:
            self._remove_host = (key, tuple(flags.tolist()))
        return self._remove_host[1]

    def _n_kept(self) -> int:
        return sum(n for n, removed in zip((3, 2, 1), self._remove()) if not removed)

    def _splits(self):
        """The end column of bonds, angles, torsions, d01, d02, a102 and of the Cartesian block (kept DOFs included)."""
        n_ic = self.n_ic_atoms
        sizes = [n_ic, n_ic, n_ic, 1, 1, 1, 3 * (len(self._cartesian_atom_indices) - 3) + self._n_kept()]
        return torch.cumsum(torch.tensor(sizes), dim=0).tolist()

    def get_dof_indices_by_type(self, conditioning_atom_indices: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The columns of the mixed coordinates by type, with the reference's keys: ``'distances'`` (bonds, ``d01``,
        ``d02``), ``'angles'`` (angles, ``a102``), ``'torsions'``, ``'d01'``, ``'d02'``, ``'a102'``, ``'cartesians'``,
        ``'reference'`` (the kept reference DOFs, always zero on the way in; empty when all are removed) and
        ``'conditioning'``: the columns of the atoms in ``conditioning_atom_indices`` (Cartesian atoms; of a reference atom
        its ``d01`` or ``d02``, ``a102``), sorted, or ``None`` when there are none.  The conditioning columns are also
        listed under their type."""
        ends = self._splits()
        starts = [0] + ends[:-1]
        names = ('distances', 'angles', 'torsions', 'd01', 'd02', 'a102', 'cartesians')
        by_type = {name: torch.arange(lo, hi) for name, lo, hi in zip(names, starts, ends)}
        by_type['distances'] = torch.cat([by_type['distances'], by_type['d01'], by_type['d02']])
        by_type['angles'] = torch.cat([by_type['angles'], by_type['a102']])
        n_mapped = len(by_type['cartesians']) - self._n_kept()
        by_type['reference'] = by_type['cartesians'][n_mapped:]
        by_type['cartesians'] = by_type['cartesians'][:n_mapped]
        by_type['conditioning'] = None
        if conditioning_atom_indices is not None:
            conditioning = set(torch.as_tensor(conditioning_atom_indices).tolist())
            *others, _, axis_atom, plane_atom = self._cartesian_atom_indices.tolist()
            positions = torch.tensor([i for i, atom in enumerate(others) if atom in conditioning], dtype=torch.int64)
            columns = [by_type['cartesians'][atom_to_flattened_indices(positions)]]
            if axis_atom in conditioning:
                columns.append(by_type['d01'])
            if plane_atom in conditioning:
                columns += [by_type['d02'], by_type['a102']]
            columns = torch.cat(columns).sort().values
            if len(columns):
                by_type['conditioning'] = columns
        return by_type

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor]:
        return self._pass(x, inverse=False)

    def inverse(self, y: torch.Tensor) -> Tuple[torch.Tensor]:
        return self._pass(y, inverse=True)

    def _pass(self, x, inverse):
        y, log_det_in, origin, rotation = self.cartesian_to_mixed(x)
        y, log_det_flow = self.flow.inverse(y) if inverse else self.flow(y)
        y, log_det_out = self.mixed_to_cartesian(y, origin, rotation)
        return y.reshape(x.shape), log_det_in + log_det_flow + log_det_out

    def cartesian_to_mixed(self, x: torch.Tensor) -> Tuple[torch.Tensor]:
        """``(y, log_det_J, origin, R)``: the mixed coordinates ``(batch_size, n_dofs_out)`` of ``x``, the log-det of the
        change, and the origin ``(batch_size, 3)`` and rotation ``(batch_size, 3, 3)`` of the relative frame."""
        d, a, t, x_cart, log_det_J = geometry.cartesian_to_zmatrix(x.reshape(x.shape[0], -1), self._z_matrix,
                                                                   self._cartesian_atom_indices)
        a, log_det_a = geometry.normalize_angles(a)
        t, log_det_t = geometry.normalize_torsions(t)
        coords, origin, rotation, log_det_frame = geometry.cartesian_to_relative_frame(x_cart, self._remove())
        return torch.cat([d, a, t, coords], dim=1), log_det_J + log_det_a + log_det_t + log_det_frame, origin, rotation

    def mixed_to_cartesian(self, y: torch.Tensor, origin: torch.Tensor, rotation: torch.Tensor) -> Tuple[torch.Tensor]:
        """``(x, log_det_J)``: the positions ``(batch_size, 3 n_atoms)`` of the mixed coordinates ``y`` in the frame given by
        ``origin`` and ``rotation``, and the log-det of the change."""
        n_ic = self.n_ic_atoms
        if y.dim() != 2 or y.shape[1] != self.n_dofs_out:
            raise ValueError(f'y must be (batch, {self.n_dofs_out}), got {tuple(y.shape)}')
        d, a, t, coords = torch.split(y, [n_ic, n_ic, n_ic, y.shape[1] - 3 * n_ic], dim=1)
        x_cart, log_det_frame = geometry.relative_frame_to_cartesian(coords, origin, rotation, self._remove())
        a, log_det_a = geometry.unnormalize_angles(a)
        t, log_det_t = geometry.unnormalize_torsions(t)
        x, log_det_J = geometry.zmatrix_to_cartesian(d, a, t, x_cart.reshape(y.shape[0], -1), self._z_matrix,
                                                    self._cartesian_atom_indices)
        return x, log_det_J + log_det_a + log_det_t + log_det_frame
