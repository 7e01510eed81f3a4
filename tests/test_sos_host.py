"""CPU tests of the sum-of-squares polynomial transformer (reference transformers/sos.py): the module API, a numpy
restatement of the map against tests/golden/sos.npz, the C ABI declarations and the host-side routing rules.  No kernel
is launched."""
import os
import re

import numpy as np
import pytest
import torch

from tfep_amd.nn.conditioners import generate_degrees
from tfep_amd.nn.flows import MAF
from tfep_amd.nn.transformers import MixedTransformer, NeuralSplineTransformer, SOSPolynomialTransformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'sos.npz')


def sos_np(x, par, K):
    """y, log_det_J, dy/dx of the SOS map on (B, D) x and (B, (2K+1) D) parameters in the reference layout."""
    B, D = x.shape
    p = par.reshape(B, 2 * K + 1, D)
    a0, a, b = p[:, 0], p[:, 1::2], p[:, 2::2]
    xe = x[:, None, :]
    y = a0 + x * (a * a).sum(1) + x ** 2 * (a * b).sum(1) + x ** 3 * (b * b).sum(1) / 3
    dydx = ((a + b * xe) ** 2).sum(1)
    return y, np.log(dydx).sum(1), dydx


def sos_vjp_np(x, par, K, gy):
    """(g_x, g_parameters) of sum(gy * y): the reference's backward (sos.py:226-257)."""
    B, D = x.shape
    p = par.reshape(B, 2 * K + 1, D)
    a, b = p[:, 1::2], p[:, 2::2]
    xe, g = x[:, None, :], gy[:, None, :]
    gp = np.empty_like(p)
    gp[:, 0] = gy
    gp[:, 1::2] = g * (2 * a * xe + b * xe ** 2)
    gp[:, 2::2] = g * (a * xe ** 2 + 2.0 / 3.0 * b * xe ** 3)
    return gy * sos_np(x, par, K)[2], gp.reshape(B, -1)


def test_module_api_matches_the_reference():
    for K in (2, 3, 5):
        tr = SOSPolynomialTransformer(K)
        assert tr.n_polynomials == K and tr.degree_polynomials == 1 and tr.parameters_per_polynomial == 2
        assert tr.n_parameters_per_feature == 2 * K + 1
        ident = tr.get_identity_parameters(4)
        assert ident.shape == ((2 * K + 1) * 4,) and ident.dtype == torch.float32
        rows = ident.reshape(2 * K + 1, 4)
        assert torch.all(rows[0] == 0) and torch.all(rows[2::2] == 0)
        assert torch.allclose(rows[1::2], torch.full((K, 4), float(np.sqrt(1 / K))))
        deg = torch.tensor([3, 0, 2, 1])
        assert torch.equal(tr.get_degrees_out(deg), deg.tile((2 * K + 1,)))
        assert tr.state_dict() == {} and list(tr.parameters()) == [] and list(tr.buffers()) == []
    assert SOSPolynomialTransformer().n_polynomials == 2
    for K in (1, 0, -3):
        with pytest.raises(ValueError, match='n_polynomials must be strictly greater than 1.'):
            SOSPolynomialTransformer(K)
    with pytest.raises(NotImplementedError, match='Inversion of SOS polynomial transformer has not been implemented yet.'):
        SOSPolynomialTransformer(2).inverse(torch.zeros(2, 3), torch.zeros(2, 15))


def test_identity_parameters_map_x_to_x():
    K, D = 3, 5
    x = np.random.default_rng(0).normal(size=(4, D))
    par = np.tile(SOSPolynomialTransformer(K).get_identity_parameters(D).double().numpy(), (4, 1))
    y, ldj, _ = sos_np(x, par, K)
    assert np.allclose(y, x, atol=1e-6) and np.allclose(ldj, 0.0, atol=1e-6)


def test_numpy_restatement_matches_the_reference_golden():
    g = np.load(GOLDEN)
    n = 0
    for K in (2, 3, 5):
        for D in (2, 5, 8):
            name = f'tr/K{K}_D{D}'
            x, par, w = (g[f'{name}/{k}'].astype(np.float64) for k in ('x', 'par', 'w'))
            y, ldj, _ = sos_np(x, par, K)
            gx, gp = sos_vjp_np(x, par, K, w)
            for got, key in ((y, 'y'), (ldj, 'ldj'), (gx, 'gx'), (gp, 'gpar')):
                ref = g[f'{name}/{key}_f64']
                assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (name, key)
            n += 1
    assert n == 9


def test_header_declares_the_sos_entry_points_and_the_fused_kind():
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    declared = set(re.findall(r'\b(tfep_[a-z0-9_]+)\s*\(', header))
    for name in ('tfep_sos_forward', 'tfep_sos_backward', 'tfep_sos_forward_f64', 'tfep_sos_backward_f64'):
        assert name in declared, name
    assert re.search(r'TFEP_FUSED_SOS\s*=\s*3', header)


def test_sos_ops_are_registered_outside_the_op_list():
    import tfep_amd.torch_ops as to
    assert to.SOS_OPS == ('sos_forward', 'sos_backward') and not set(to.SOS_OPS) & set(to.OPS)
    s = str(torch.ops.tfep.sos_forward.default._schema)
    assert 'n_polynomials' in s and '-> (Tensor, Tensor)' in s
    assert 'grad_y' in str(torch.ops.tfep.sos_backward.default._schema)


def test_fused_kind_and_inverse_routing_rules():
    """SOS of 2 or 3 polynomials has a fused output-layer epilogue (kind 3, alone or as a mixed member); other K take the
    generic path.  Neither the blocked inverse nor the fused inverse claims an SOS layer."""
    from tfep_amd.nn.flows import _backward
    from tfep_amd.nn.flows.autoregressive import _FUSED_MIXED, _FUSED_SOS

    def layer(tr, D=6):
        return MAF(generate_degrees(D, 'ascending'), transformer=tr, initialize_identity=False)
    assert _FUSED_SOS == 3 and _FUSED_MIXED == 2
    for K, kind in ((2, 3), (3, 3), (4, None), (16, None)):
        lay = layer(SOSPolynomialTransformer(K))
        assert lay._fused_kind() == kind, K
        assert not lay._blocked_ok() and not lay._fused_inverse_supported(2)
        assert _backward.supported(lay)
    mixed = MixedTransformer([SOSPolynomialTransformer(2), NeuralSplineTransformer(torch.zeros(3), torch.ones(3), 8)],
                             [[0, 2, 4], [1, 3, 5]])
    lay = layer(mixed)
    assert lay._fused_kind() == _FUSED_MIXED and not lay._blocked_ok() and not lay._fused_inverse_supported(2)
    assert _backward.supported(lay)
    mixed = MixedTransformer([SOSPolynomialTransformer(5), NeuralSplineTransformer(torch.zeros(3), torch.ones(3), 8)],
                             [[0, 2, 4], [1, 3, 5]])
    assert layer(mixed)._fused_kind() is None


def test_identity_initialised_layer_sets_the_identity_parameters():
    D, K = 5, 2
    lay = MAF(generate_degrees(D), transformer=SOSPolynomialTransformer(K))
    out = lay._conditioner.layers[-1]
    assert torch.allclose(out.bias, SOSPolynomialTransformer(K).get_identity_parameters(D))
