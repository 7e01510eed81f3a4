"""Moebius and symmetrized Moebius transformers (reference ``tfep/nn/transformers/moebius.py:27-372``)."""
import torch

from ... import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.tfep.*)
from .transformer import MAFTransformer


def _float32_only(x):
    if isinstance(x, torch.Tensor) and x.dtype == torch.float64:
        raise TypeError('MoebiusTransformer: float64 is not supported for the Moebius transformer yet (float32 only)')


def moebius_float64(tr):
    """Is ``tr`` a Moebius transformer that has opted in to the float64 kernels (``float64_kernels``)?"""
    return isinstance(tr, MoebiusTransformer) and bool(tr.float64_kernels)


class MoebiusTransformer(MAFTransformer):
    r""":math:`y = \frac{\|x\|^2 - \|w\|^2}{\|x - w\|^2}(x - w) - w` on ``dimension``-vectors.

    ``w`` is rescaled to ``max_radius/(1+|w|) * |x| * w`` (``|x| = 1`` if ``unit_sphere``); the
    inverse is the forward map with ``-w`` (reference moebius.py:142-147).
    """

    #: Opt-in: run float64 tensors on the float64 kernels (``tfep_moebius_forward_f64`` / ``_backward_f64``: IEEE division,
    #: square root and logarithm), alone, in a float64 MAF layer or as a member of a float64 mixed transformer.  False (the
    #: default): float64 is refused with a TypeError, as before the float64 kernels existed.  A class attribute; an
    #: instance may set its own.
    float64_kernels = False

    def __init__(self, dimension: int, max_radius: float = 0.99, unit_sphere: bool = False):
        super().__init__()
        self.dimension = dimension
        self.max_radius = max_radius
        self.unit_sphere = unit_sphere

    def _check(self, x, name):
        if self.float64_kernels:
            ops.check_device_tensor(x, name, ops._dtype(x))                # float32, or float64 (the float64 kernels)
        else:
            _float32_only(x)
            ops.check_device_tensor(x, name)

    def forward(self, x, parameters):
        self._check(x, 'x')
        return tuple(torch.ops.tfep.moebius_forward(x, parameters, int(self.dimension), float(self.max_radius),
                                                    bool(self.unit_sphere)))                   # differentiable

    def inverse(self, y, parameters):
        self._check(y, 'y')
        return tuple(torch.ops.tfep.moebius_inverse(y, parameters, int(self.dimension), float(self.max_radius),
                                                    bool(self.unit_sphere)))

    def get_identity_parameters(self, n_features: int) -> torch.Tensor:
        return torch.zeros(size=(n_features,))

    def get_degrees_out(self, degrees_in: torch.Tensor) -> torch.Tensor:
        return degrees_in.detach().clone()


class SymmetrizedMoebiusTransformer(MAFTransformer):
    r""":math:`y = \|x\| \frac{f(x; w) + f(x; -w)}{\|f(x; w) + f(x; -w)\|}` on ``dimension``-vectors, :math:`f` the Moebius
    map of :class:`MoebiusTransformer` on the sphere of radius :math:`\|x\|` (reference moebius.py:193-372).

    Even in ``w``, with a closed-form inverse and log-det (``tfep_amd/csrc/symmoebius.h``); float32 and float64.  A class of
    its own, not a ``MoebiusTransformer``: none of that transformer's float32-only speed paths apply.  ``w = 0`` is the
    identity but has zero parameter gradient, so the identity parameters are random numbers of at most ``identity_eps``.
    """

    def __init__(self, dimension: int, max_radius: float = 0.99, identity_eps: float = 1e-9):
        super().__init__()
        self.dimension = dimension
        self.max_radius = max_radius
        self.identity_eps = identity_eps

    def forward(self, x, parameters):
        ops.check_device_tensor(x, 'x', ops._dtype(x))                     # float32, or float64 (the float64 kernels)
        return tuple(torch.ops.tfep.symmetrized_moebius_forward(x, parameters, int(self.dimension),
                                                                float(self.max_radius)))         # differentiable

    def inverse(self, y, parameters):
        ops.check_device_tensor(y, 'y', ops._dtype(y))
        return tuple(torch.ops.tfep.symmetrized_moebius_inverse(y, parameters, int(self.dimension),
                                                                float(self.max_radius)))         # differentiable

    def get_identity_parameters(self, n_features: int) -> torch.Tensor:
        par = torch.rand(n_features)                                        # (one draw: the reference's random stream)
        return (2 * par - 1) * self.identity_eps

    def get_degrees_out(self, degrees_in: torch.Tensor) -> torch.Tensor:
        return degrees_in.detach().clone()
