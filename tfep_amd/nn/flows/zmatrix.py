"""Flow wrapper that maps the internal coordinates of a Z-matrix (bonds, angles, torsions) with the wrapped flow.

The way in is ``cartesian_to_zmatrix`` (the ``internal_coordinates`` kernel), the way back ``zmatrix_to_cartesian`` (the
placement kernel, ``csrc/zmatrix.hip``), one launch each and one more for each backward.  This is the coordinate change
of the reference's ``MixedMAFMap`` (``app/mixedmaf.py:954-1400``, which imports it from ``bgflow``) and nothing else of
it: the removal of the reference frame and the normalisation of the torsions are not part of this module; they are in
``CartesianToMixedFlow`` (``nn/flows/mixed.py``), which is the whole coordinate change.
"""
from typing import Tuple

import torch

from ...utils.geometry import cartesian_to_zmatrix, zmatrix_to_cartesian
from ...utils.misc import ensure_tensor_sequence


class ZMatrixFlow(torch.nn.Module):
    """Map ``x`` ``(batch_size, 3 n_atoms)`` through ``flow`` in the internal coordinates of ``z_matrix``.

    ``z_matrix``: ``(n_ic, 4)`` rows ``(i, j, k, l)``; ``fixed_atoms``: ``(n_fixed,)``, at least three atoms (see
    ``tfep_amd.utils.geometry.zmatrix_to_cartesian``).  ``flow`` maps ``3 n_atoms`` features laid out as ``[d | a | t |
    x_fixed]``: ``n_ic`` distances, ``n_ic`` angles, ``n_ic`` dihedrals in the row order of ``z_matrix`` and the ``3
    n_fixed`` coordinates of the fixed atoms in the order of ``fixed_atoms``.

    ``forward`` converts to that layout, runs ``flow``, places the atoms back and returns ``(y, log_det_J)`` with the
    three log-dets added; ``inverse`` does the same with ``flow.inverse``.

    The wrapped flow is free to move an angle out of ``(0, pi)``, a distance below zero or a dihedral across ``+-pi``.
    The placement accepts such values, but the way in returns angles in ``[0, pi]``, distances ``>= 0`` and dihedrals in
    ``(-pi, pi]``, so the composition is then no longer inverted by ``inverse``: keeping the angles inside ``(0, pi)`` (a
    bounded transformer, for instance) and treating the dihedrals as periodic (a circular transformer) is the caller's
    concern.  Eager only: the host-side table lookup is not captured by ``GraphedFlow``.
    """

    def __init__(self, flow: torch.nn.Module, z_matrix, fixed_atoms):
        super().__init__()
        self.flow = flow
        self.register_buffer('_z_matrix', ensure_tensor_sequence(z_matrix))
        self.register_buffer('_fixed_atoms', ensure_tensor_sequence(fixed_atoms))

    def n_parameters(self):
        """int: The total number of parameters that can be optimized."""
        return self.flow.n_parameters()

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor]:
        return self._pass(x, inverse=False)

    def inverse(self, y: torch.Tensor) -> Tuple[torch.Tensor]:
        return self._pass(y, inverse=True)

    def _pass(self, x, inverse):
        n_ic, n_fixed = len(self._z_matrix), len(self._fixed_atoms)
        d, a, t, x_fixed, log_det_in = cartesian_to_zmatrix(x, self._z_matrix, self._fixed_atoms)
        mixed = torch.cat([d, a, t, x_fixed.reshape(x.shape[0], -1)], dim=1)
        mixed, log_det_flow = self.flow.inverse(mixed) if inverse else self.flow(mixed)
        d, a, t, x_fixed = torch.split(mixed, [n_ic, n_ic, n_ic, 3 * n_fixed], dim=1)
        y, log_det_out = zmatrix_to_cartesian(d, a, t, x_fixed, self._z_matrix, self._fixed_atoms)
        return y.reshape(x.shape), log_det_in + log_det_flow + log_det_out
