"""Quaternion product transformer (reference ``tfep/nn/transformers/quatprod.py``)."""
import torch

from ... import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.tfep.*)
from .transformer import MAFTransformer


class QuaternionProductTransformer(MAFTransformer):
    r""":math:`y = \hat p \otimes x` on quaternions, :math:`\hat p = p / \|p\|` the normalised parameter quaternion; the
    inverse is :math:`x = \hat p^* \otimes y`.

    Every 4 contiguous features are one quaternion with the scalar LAST, ``(x, y, z, w)``, and the Hamilton product -- the
    convention of the ``roma`` package that the reference calls (this package does not need it).  The map is a rigid
    rotation of each quaternion: it preserves the norm and the volume, so ``log_det_J`` is zero.  float32 and float64, on
    HIP kernels of its own (``tfep_amd/csrc/quatprod.h``).  A zero parameter quaternion gives NaN, as in the reference.
    """

    #: features per quaternion
    dimension = 4

    def forward(self, x, parameters):
        _check_quaternions(x)
        ops.check_device_tensor(x, 'x', ops._dtype(x))                     # float32, or float64 (the float64 kernels)
        return tuple(torch.ops.tfep.quaternion_product_forward(x, parameters))         # differentiable

    def inverse(self, y, parameters):
        _check_quaternions(y)
        ops.check_device_tensor(y, 'y', ops._dtype(y))
        return tuple(torch.ops.tfep.quaternion_product_inverse(y, parameters))         # differentiable

    def get_identity_parameters(self, n_features: int) -> torch.Tensor:
        if n_features % 4 != 0:
            raise ValueError(f'n_features={n_features} is not a multiple of 4 (quaternions)')
        return torch.tensor([0.0, 0.0, 0.0, 1.0]).repeat(n_features // 4)

    def get_degrees_out(self, degrees_in: torch.Tensor) -> torch.Tensor:
        return degrees_in.detach().clone()


def _check_quaternions(x):
    if isinstance(x, torch.Tensor) and x.dim() > 0 and x.shape[-1] % 4 != 0:
        raise ValueError(f'QuaternionProductTransformer: n_features={x.shape[-1]} is not a multiple of 4 (quaternions)')
