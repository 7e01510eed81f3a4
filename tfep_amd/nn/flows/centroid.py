"""Flow wrapper that constrains the (weighted) centroid (reference ``tfep/nn/flows/centroid.py:30-268``).

``TFEPMapBase`` puts this around the MAF stack to remove the translational degrees of freedom.  The wrapped
flow and the column gather / scatter of :class:`PartialFlow` run on the HIP kernels.  The translation and centroid
arithmetic has two routes: the frame kernels (``torch.ops.tfep.centroid_shift`` / ``centroid_restore``, one launch each,
``csrc/frames.hip``) and O(batch x features) torch ops on the input's device.
"""
from typing import Optional, Sequence, Tuple

import torch

from ...utils.misc import atom_to_flattened, atom_to_flattened_indices, ensure_tensor_sequence, flattened_to_atom
from ... import torch_ops  # noqa: F401  (registers torch.ops.tfep.*)
from .partial import PartialFlow


def _optional_tensor(values):
    return None if values is None else ensure_tensor_sequence(values)


class CenteredCentroidFlow(PartialFlow):
    """Translate the centroid to ``origin``, map all points but one with the wrapped flow, then place the
    remaining point so that the centroid is unchanged.  Arguments and attributes as reference
    centroid.py:52-112.

    ``frame_kernels`` selects the route of the centroid arithmetic: ``None`` (default) takes the frame kernels for a
    float64 input and the torch ops for a float32 one, ``True`` the kernels in either dtype, ``False`` the torch ops in
    either dtype.  The kernels take ``space_dimension <= 3`` and distinct subset indices; anything else runs on the torch
    ops.  ``last_route`` is ``'kernels'`` or ``'torch'`` after a pass."""

    #: None: kernels for float64 inputs, torch ops for float32 ones; True / False: kernels / torch ops in either dtype
    frame_kernels = None
    #: the route of the last pass ('kernels' / 'torch'), None before the first
    last_route = None

    def __init__(
            self,
            flow: torch.nn.Module,
            space_dimension: int,
            subset_point_indices: Optional[Sequence[int]] = None,
            weights: Optional[Sequence[float]] = None,
            fixed_point_idx: int = 0,
            origin: Optional[Sequence[float]] = None,
            translate_back: bool = True,
            return_partial: bool = False,
    ):
        if translate_back and return_partial:
            raise ValueError("'return_partial=True' is supported only if 'translate_back=False'")
        if origin is not None and len(origin) != space_dimension:
            raise ValueError("'origin' must have length equal to 'space_dimension'.")
        subset, weights = _optional_tensor(subset_point_indices), _optional_tensor(weights)
        if subset is not None and weights is not None and len(weights) != len(subset):
            raise ValueError("'weights' must have the same length as 'subset_point_indices'.")

        # `fixed_point_idx` counts within the subset when there is one: the point itself is subset[fixed_point_idx].
        fixed_point = int(fixed_point_idx if subset is None else subset[fixed_point_idx])
        super().__init__(flow, fixed_indices=atom_to_flattened_indices(torch.tensor([fixed_point]), space_dimension),
                         return_partial=return_partial)

        self._space_dimension = space_dimension
        self.translate_back = translate_back
        self.register_buffer('_fixed_point_idx', torch.as_tensor(fixed_point_idx))
        self.register_buffer('_subset_point_indices', subset)
        # normalised, as a column: multiplies (batch, n_points, dim) directly
        self.register_buffer('_weights', None if weights is None else (weights / weights.sum()).unsqueeze(1))
        self.register_buffer('origin', torch.zeros(space_dimension) if origin is None else ensure_tensor_sequence(origin))
        # Host copies so that no pass reads a device scalar back.
        self._host_fixed_point_idx = int(fixed_point_idx)
        self._host_fixed_point = fixed_point
        self._single_point_centroid = subset is not None and len(subset) <= 1
        self._kernels_supported = space_dimension <= 3 and (subset is None or len(set(subset.tolist())) == len(subset))

    @property
    def space_dimension(self):
        """int: The dimensionality of a single point in space."""
        return self._space_dimension

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor]:
        return self._transform(x, inverse=False)

    def inverse(self, y: torch.Tensor) -> Tuple[torch.Tensor]:
        if not self.translate_back:
            raise ValueError("The inverse of CenteredCentroidFlow can be computed"
                             " only if 'translate_back' is set to True during both"
                             " the forward and inverse transformations.")
        return self._transform(y, inverse=True)

    def takes_kernel_route(self, x):
        """Whether a pass on ``x`` runs the centroid arithmetic on the frame kernels (see ``frame_kernels``)."""
        wanted = x.dtype == torch.float64 if self.frame_kernels is None else bool(self.frame_kernels)
        return wanted and self._kernels_supported

    def _selection(self, x):
        """The kernels' operands in the input's dtype: int32 subset (cached with the gather indices), flat weights, origin."""
        subset = self._subset_point_indices
        if subset is not None:
            key = ('subset', str(x.device))
            if key not in self._i32:
                self._i32[key] = subset.to(device=x.device, dtype=torch.int32)
            subset = self._i32[key]
        # weights and origin in the input's dtype: buffers of that dtype are used as they are, others are cast once and
        # the casts kept until a buffer is replaced or written (load_state_dict)
        bufs = tuple(b for b in (self._weights, self.origin) if b is not None)
        if all(b.dtype == x.dtype and b.device == x.device for b in bufs):
            return subset, None if self._weights is None else self._weights.reshape(-1), self.origin
        key = ('cast', str(x.device), x.dtype)
        stamp = tuple((b._version, b.data_ptr()) for b in bufs)
        cached = self._i32.get(key)
        if cached is None or cached[0] != stamp:
            cached = (stamp, None if self._weights is None else self._weights.reshape(-1).to(x), self.origin.to(x))
            self._i32[key] = cached
        return subset, cached[1], cached[2]

    def _transform_kernels(self, x, inverse):
        dim = self._space_dimension
        subset, weights, origin = self._selection(x)
        shift, x_centered = torch.ops.tfep.centroid_shift(x, subset, weights, origin, dim)
        out = PartialFlow.inverse(self, x_centered) if inverse else PartialFlow.forward(self, x_centered)
        if self.return_partial:
            return out
        y = out[0]
        if not self._single_point_centroid or self.translate_back:
            y = torch.ops.tfep.centroid_restore(y, shift, subset, weights, origin, self._host_fixed_point,
                                                self._host_fixed_point_idx, dim, self.translate_back)
        return (y, *out[1:])

    def _transform(self, x, inverse):
        if self.takes_kernel_route(x):
            self.last_route = 'kernels'
            return self._transform_kernels(x, inverse)
        self.last_route = 'torch'
        dim = self._space_dimension
        pts = flattened_to_atom(x, dim)
        shift = (self.origin - self._centroid(pts)).unsqueeze(1)
        x_centered = atom_to_flattened(pts + shift)

        out = PartialFlow.inverse(self, x_centered) if inverse else PartialFlow.forward(self, x_centered)
        if self.return_partial:
            return out
        y = out[0]

        # Put the fixed point where it restores the centroid (nothing to do when the centroid IS that point).
        if not self._single_point_centroid:
            y_pts = flattened_to_atom(y, dim)
            rest, w_fixed = self._centroid(y_pts, exclude_fixed_point=True)
            fixed_pos = (self.origin - rest) / w_fixed
            f = self._host_fixed_point
            y_pts = torch.cat([y_pts[:, :f], fixed_pos.unsqueeze(1), y_pts[:, f + 1:]], dim=1)
            y = atom_to_flattened(y_pts)
        if self.translate_back:
            y = atom_to_flattened(flattened_to_atom(y, dim) - shift)
        return (y, *out[1:])

    def _centroid(self, pts, exclude_fixed_point=False):
        """Centroid (B, dim) of the selected points; with ``exclude_fixed_point`` the fixed point's
        contribution is left out and its weight is returned too."""
        if self._subset_point_indices is not None:
            pts = pts[:, self._subset_point_indices]
        if self._weights is None:
            centroid = pts.mean(dim=1)
            w_fixed = 1.0 / pts.shape[1]
        else:
            centroid = (pts * self._weights).sum(dim=1)
            w_fixed = self._weights[self._host_fixed_point_idx]
        if exclude_fixed_point:
            return centroid - pts[:, self._host_fixed_point_idx] * w_fixed, w_fixed
        return centroid
