"""CPU tests of the symmetrized Moebius transformer (reference transformers/moebius.py:193-372, :481-629): the module API
and the seeded identity parameters against tests/golden/symmoebius.npz, the C ABI declarations, the registered ops, the
host-side routing rules of a layer with this transformer, dtype and device errors.  No kernel is launched."""
import os
import re

import numpy as np
import pytest
import torch

from tfep_amd.nn.conditioners import generate_degrees
from tfep_amd.nn.flows import MAF
from tfep_amd.nn.transformers import (MixedTransformer, MoebiusTransformer, NeuralSplineTransformer,
                                      SymmetrizedMoebiusTransformer)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'symmoebius.npz')
SYMBOLS = ('tfep_symmetrized_moebius', 'tfep_symmetrized_moebius_backward', 'tfep_symmetrized_moebius_f64',
           'tfep_symmetrized_moebius_backward_f64')


def test_module_api_matches_the_reference():
    tr = SymmetrizedMoebiusTransformer(4)
    assert (tr.dimension, tr.max_radius, tr.identity_eps) == (4, 0.99, 1e-9)
    tr = SymmetrizedMoebiusTransformer(3, max_radius=0.7, identity_eps=1e-3)
    assert (tr.dimension, tr.max_radius, tr.identity_eps) == (3, 0.7, 1e-3)
    assert tr.state_dict() == {} and list(tr.parameters()) == [] and list(tr.buffers()) == []
    deg = torch.tensor([3, 3, 3, 0, 0, 0])
    out = tr.get_degrees_out(deg)
    assert torch.equal(out, deg) and out is not deg and out.data_ptr() != deg.data_ptr()
    ident = tr.get_identity_parameters(12)
    assert ident.shape == (12,) and ident.dtype == torch.float32 and float(ident.abs().max()) <= 1e-3
    assert torch.all(SymmetrizedMoebiusTransformer(3, identity_eps=0.0).get_identity_parameters(6) == 0)
    assert not issubclass(SymmetrizedMoebiusTransformer, MoebiusTransformer)
    assert not isinstance(tr, MoebiusTransformer)


def test_seeded_identity_parameters_match_the_reference():
    g = np.load(GOLDEN)
    torch.manual_seed(7)
    ident = SymmetrizedMoebiusTransformer(3).get_identity_parameters(12)
    np.testing.assert_array_equal(ident.numpy(), g['identity/seed7_n12'])
    # one torch.rand(n) call from the global generator: the stream continues where the reference's does
    torch.manual_seed(7)
    torch.rand(12)
    after = torch.rand(3)
    torch.manual_seed(7)
    SymmetrizedMoebiusTransformer(3).get_identity_parameters(12)
    assert torch.equal(torch.rand(3), after)


def test_golden_holds_data_only_and_no_degenerate_points():
    g = np.load(GOLDEN, allow_pickle=False)
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    for k in g.files:
        assert g[k].dtype.kind in 'fiub', k                      # plain numbers, no objects
        assert g[k].dtype.kind != 'f' or np.isfinite(g[k]).all(), k
    for dim in (2, 3, 4):
        for R in (0.99, 0.7):
            name = f'tr/d{dim}_R{R}'
            for k in ('x', 'w', 'yin'):
                v = g[f'{name}/{k}'].reshape(32, 6, dim)
                assert g[f'{name}/{k}'].dtype == np.float32 and np.linalg.norm(v, axis=-1).min() > 1e-3
            assert g[f'{name}/y_f64'].dtype == np.float64 and g[f'{name}/y_f32'].dtype == np.float32
            # |y| = |x| per vector in the reference's float64 results
            for a, b in (('x', 'y_f64'), ('yin', 'y_inv_f64')):
                na = np.linalg.norm(g[f'{name}/{a}'].astype(np.float64).reshape(32, 6, dim), axis=-1)
                nb = np.linalg.norm(g[f'{name}/{b}'].reshape(32, 6, dim), axis=-1)
                np.testing.assert_allclose(nb, na, rtol=1e-12)


def test_header_bindings_and_ops_are_registered():
    from tfep_amd import _lib, torch_ops
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    declared = set(re.findall(r'\b(tfep_[a-z0-9_]+)\s*\(', header))
    for s in SYMBOLS:
        assert s in declared and s in _lib.EXPORTED_SYMBOLS, s
    assert _lib.ABI_VERSION == 8
    assert torch_ops.SYMMETRIZED_MOEBIUS_OPS == ('symmetrized_moebius_forward', 'symmetrized_moebius_inverse',
                                                 'symmetrized_moebius_backward')
    for name in torch_ops.SYMMETRIZED_MOEBIUS_OPS:
        assert name not in torch_ops.OPS
        assert hasattr(torch.ops.tfep, name), name
    # shapes through the fake implementations (meta tensors: nothing runs)
    x, p = torch.empty(5, 12, device='meta'), torch.empty(5, 12, device='meta')
    for op in (torch.ops.tfep.symmetrized_moebius_forward, torch.ops.tfep.symmetrized_moebius_inverse):
        y, l = op(x, p, 3, 0.99)
        assert y.shape == (5, 12) and l.shape == (5,)
    gx, gp = torch.ops.tfep.symmetrized_moebius_backward(x, p, x, torch.empty(5, device='meta'), 3, 0.99, True)
    assert gx.shape == (5, 12) and gp.shape == (5, 12)


def _layer(dim, n_vec, straddle=False, **kw):
    D = dim * n_vec
    deg = generate_degrees(D, 'ascending') if straddle else generate_degrees(D, 'ascending', repeats=dim)
    return MAF(deg, transformer=SymmetrizedMoebiusTransformer(dim), **kw)


def test_routing_rules():
    from tfep_amd.nn.flows import _backward
    for dim in (2, 3, 4):
        layer = _layer(dim, 4)
        assert layer._fused_kind() is None
        layer.fused = True
        assert layer._fused_kind() is None
        layer.fused = None
        assert layer._blocked_ok() is True                       # every vector inside one degree
        assert layer._fused_inverse_supported(3) is False        # per-degree steps, no block-kernel kind
        assert layer._sub_transformer(torch.arange(dim), 'cpu')[0] == 'symmoebius'
        assert _layer(dim, 4, straddle=True)._blocked_ok() is False
        assert _backward.supported(layer) and _backward.generic_supported(layer)
        layer.blocked_inverse = False
        assert layer._blocked_ok() is False
    assert _layer(3, 4).double()._blocked_ok() is False          # float64: the reference's pass per degree
    # the one-launch layer kernel is for the plain d = 2 Moebius transformer only
    layer = _layer(2, 4)
    layer.layer_kernel = True
    assert not layer._layer_kernel_ok(torch.empty(8, 8))
    # identity initialisation uses the (tiny, random) identity parameters
    torch.manual_seed(3)
    layer = _layer(3, 4, initialize_identity=True)
    bias = layer._conditioner.layers[-1].bias.detach()
    assert float(bias.abs().max()) <= 1e-9 and float(bias.abs().max()) > 0


def test_mixed_member_routing_and_float64_acceptance():
    from tfep_amd.nn.flows import _backward
    from tfep_amd.nn.transformers.mixed import check_float64_members
    mixed = MixedTransformer([SymmetrizedMoebiusTransformer(2), NeuralSplineTransformer(torch.full((6,), -4.0), torch.full((6,), 4.0), 8)],
                             [[0, 1, 2, 3], [4, 5, 6, 7, 8, 9]])
    layer = MAF(generate_degrees(10, 'ascending'), transformer=mixed, initialize_identity=False)
    assert layer._fused_kind() is None and layer._blocked_ok() is False
    assert _backward.supported(layer)
    check_float64_members(mixed)                                  # accepted; the plain Moebius member is still refused
    with pytest.raises(TypeError):
        check_float64_members(MixedTransformer([MoebiusTransformer(2), SymmetrizedMoebiusTransformer(2)], [[0, 1], [2, 3]]))
    assert torch.equal(mixed.get_degrees_out(torch.arange(10))[:4], torch.arange(4))


def test_cpu_tensors_and_wrong_dtypes_are_refused():
    from tfep_amd import ops
    from tfep_amd._lib import TfepHipError
    tr = SymmetrizedMoebiusTransformer(3)
    for dt in (torch.float32, torch.float64):
        x, w = torch.randn(4, 6, dtype=dt), torch.randn(4, 6, dtype=dt)
        for fn in (tr.forward, tr.inverse, lambda a, b: ops.symmetrized_moebius(a, b, 3, 0.99)):
            with pytest.raises(TfepHipError, match='no CPU fallback'):
                fn(x, w)
    with pytest.raises(TypeError):
        ops.symmetrized_moebius([1.0], [1.0], 3, 0.99)
