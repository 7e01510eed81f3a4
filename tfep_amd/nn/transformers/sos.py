"""Sum-of-squares polynomial transformer (reference ``tfep/nn/transformers/sos.py``)."""
import math

import torch

from ... import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.tfep.*)
from .transformer import MAFTransformer


class SOSPolynomialTransformer(MAFTransformer):
    r""":math:`y_i = a_0 + \int_0^{x_i} \sum_{k=1}^K (a_{k0} + a_{k1} z)^2 dz` (reference sos.py:26-163; Jaini et al. 2019).

    ``parameters[:, p * n_features + i]`` is parameter ``p`` of feature ``i``: ``p = 0`` is :math:`a_0`, ``p = 1 + 2k`` is
    :math:`a_{k0}` and ``p = 2 + 2k`` is :math:`a_{k1}` (sos.py:96-99).  The log-det carries no gradient, as in the
    reference (``mark_non_differentiable``, sos.py:222).  There is no inverse.
    """

    def __init__(self, n_polynomials=2):
        super().__init__()
        if n_polynomials < 2:
            raise ValueError('n_polynomials must be strictly greater than 1.')
        self.n_polynomials = n_polynomials

    @property
    def degree_polynomials(self):
        """The degree of each squared polynomial."""
        return 1

    @property
    def parameters_per_polynomial(self):
        """Number of parameters of each squared polynomial."""
        return self.degree_polynomials + 1

    @property
    def n_parameters_per_feature(self):
        """Number of parameters per transformed feature: 2 K + 1."""
        return self.parameters_per_polynomial * self.n_polynomials + 1

    def forward(self, x, parameters):
        ops.check_device_tensor(x, 'x', ops._dtype(x))                     # float32, or float64 (the float64 kernels)
        # differentiable in x and the parameters (tfep::sos_backward); the log-det is not
        return tuple(torch.ops.tfep.sos_forward(x, parameters, int(self.n_polynomials)))

    def inverse(self, y, parameters):
        raise NotImplementedError('Inversion of SOS polynomial transformer has not been implemented yet.')

    def get_identity_parameters(self, n_features: int) -> torch.Tensor:
        # the squared linear coefficients sum to 1 (sos.py:141-144)
        identity = torch.zeros(size=(self.n_parameters_per_feature, n_features))
        identity[1::self.parameters_per_polynomial].fill_(math.sqrt(1 / self.n_polynomials))
        return identity.flatten()

    def get_degrees_out(self, degrees_in: torch.Tensor) -> torch.Tensor:
        return degrees_in.tile((self.n_parameters_per_feature,))
