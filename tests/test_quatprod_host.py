"""CPU tests of the quaternion product transformer (reference transformers/quatprod.py): the module API, the C ABI
declarations, the registered ops, the host-side routing rules of a layer with this transformer, dtype / shape / device
errors, and the golden file itself.  No kernel is launched.

tests/golden/quatprod.npz comes from the reference class run on ``tools/roma_standin.py`` (the ``roma`` package the
reference imports is not a dependency of anything here).  The stand-in is this project's own code, so its results are pinned
here twice, independently of it: against the 16 terms of the Hamilton product written out in numpy below, and against
``scipy.spatial.transform.Rotation`` (scalar-last quaternions, composition = Hamilton product)."""
import os
import re

import numpy as np
import pytest
import torch

from tfep_amd.nn.conditioners import generate_degrees
from tfep_amd.nn.flows import MAF
from tfep_amd.nn.transformers import MixedTransformer, NeuralSplineTransformer, QuaternionProductTransformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'quatprod.npz')
SYMBOLS = ('tfep_quaternion_product', 'tfep_quaternion_product_backward', 'tfep_quaternion_product_f64',
           'tfep_quaternion_product_backward_f64')
OPS = ('quaternion_product_forward', 'quaternion_product_inverse', 'quaternion_product_backward')


def hamilton(a, b):
    """a (x) b for (..., 4) arrays, scalar last: the 16 products written out."""
    a1, a2, a3, a4 = (a[..., i] for i in range(4))
    b1, b2, b3, b4 = (b[..., i] for i in range(4))
    return np.stack([a4 * b1 + a1 * b4 + a2 * b3 - a3 * b2,
                     a4 * b2 - a1 * b3 + a2 * b4 + a3 * b1,
                     a4 * b3 + a1 * b2 - a2 * b1 + a3 * b4,
                     a4 * b4 - a1 * b1 - a2 * b2 - a3 * b3], axis=-1)


def test_module_api_matches_the_reference():
    tr = QuaternionProductTransformer()                          # no constructor arguments
    with pytest.raises(TypeError):
        QuaternionProductTransformer(4)
    assert tr.state_dict() == {} and list(tr.parameters()) == [] and list(tr.buffers()) == []
    deg = torch.tensor([3, 3, 3, 3, 0, 0, 0, 0])
    out = tr.get_degrees_out(deg)
    assert torch.equal(out, deg) and out is not deg and out.data_ptr() != deg.data_ptr()
    ident = tr.get_identity_parameters(12)
    assert ident.shape == (12,) and ident.dtype == torch.float32
    assert torch.equal(ident, torch.tensor([0., 0., 0., 1.] * 3))
    np.testing.assert_array_equal(ident.numpy(), np.load(GOLDEN)['identity/n12'])
    assert tr.get_identity_parameters(0).shape == (0,)
    import tfep_amd.nn.transformers as pkg
    assert pkg.QuaternionProductTransformer is QuaternionProductTransformer
    # every transformer name of the reference's package (tfep/nn/transformers/__init__.py) is exported now
    for name in ('AffineTransformer', 'VolumePreservingShiftTransformer', 'MixedTransformer', 'MoebiusTransformer',
                 'SymmetrizedMoebiusTransformer', 'SOSPolynomialTransformer', 'NeuralSplineTransformer',
                 'QuaternionProductTransformer'):
        assert hasattr(pkg, name), name


def test_header_bindings_and_ops_are_registered():
    from tfep_amd import _lib, torch_ops
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    declared = set(re.findall(r'\b(tfep_[a-z0-9_]+)\s*\(', header))
    for s in SYMBOLS:
        assert s in declared and s in _lib.EXPORTED_SYMBOLS, s
    assert _lib.ABI_VERSION == 8
    assert re.search(r'#define\s+TFEP_HIP_ABI_VERSION\s+8\b', header)
    assert torch_ops.QUATERNION_PRODUCT_OPS == OPS
    for name in OPS:
        assert name not in torch_ops.OPS
        assert hasattr(torch.ops.tfep, name), name
    # shapes through the fake implementations (meta tensors: nothing runs)
    x, p = torch.empty(5, 12, device='meta'), torch.empty(5, 12, device='meta')
    for op in (torch.ops.tfep.quaternion_product_forward, torch.ops.tfep.quaternion_product_inverse):
        y, l = op(x, p)
        assert y.shape == (5, 12) and l.shape == (5,)
    gx, gp = torch.ops.tfep.quaternion_product_backward(x, p, x, True)
    assert gx.shape == (5, 12) and gp.shape == (5, 12)


def test_built_library_exports_the_symbols_and_checks_its_arguments():
    """The argument checks of the C entry points come before any HIP call: they run on a machine without a GPU."""
    from tfep_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.tfep_quaternion_product(None, 6, None, 6, 0, None, 6, None, 0, 4, 6, None) != 0          # D % 4
    assert 'multiple of 4' in lib.tfep_last_error().decode()
    assert lib.tfep_quaternion_product(None, 8, None, 8, 0, None, 8, None, 0, 4, 8, None) != 0          # NULL
    assert lib.tfep_quaternion_product_f64(None, 8, None, 8, 0, None, 8, None, 0, -1, 8, None) != 0     # B < 0
    assert lib.tfep_quaternion_product(None, 8, None, 8, 2, None, 8, None, 0, 4, 8, None) != 0          # inverse flag
    assert lib.tfep_quaternion_product_backward(None, 6, None, 6, 0, None, 6, None, 6, None, 6, 4, 6, None) != 0
    assert lib.tfep_quaternion_product_backward_f64(None, 8, None, 8, 0, None, 8, None, 8, None, 8, 4, 8, None) != 0
    assert lib.tfep_quaternion_product(None, 8, None, 8, 0, None, 8, None, 0, 0, 8, None) == 0          # B = 0: nothing to do


def test_no_roma_import_in_the_package():
    pkg = os.path.join(ROOT, 'tfep_amd')
    for folder, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                text = open(os.path.join(folder, f)).read()
                assert not re.search(r'^\s*(import|from)\s+roma\b', text, flags=re.M), os.path.join(folder, f)
    import sys
    import tfep_amd.nn.flows  # noqa: F401
    assert 'roma' not in sys.modules


def _layer(n_quat, straddle=False, **kw):
    D = 4 * n_quat
    deg = generate_degrees(D, 'ascending') if straddle else generate_degrees(D, 'ascending', repeats=4)
    return MAF(deg, transformer=QuaternionProductTransformer(), **kw)


def test_routing_rules():
    from tfep_amd.nn.flows import _backward
    layer = _layer(3)
    assert layer._fused_kind() is None
    layer.fused = True
    assert layer._fused_kind() is None
    layer.fused = None
    assert layer._blocked_ok() is True                           # every quaternion inside one degree
    assert layer._fused_inverse_supported(3) is False            # per-degree steps, no block-kernel kind
    assert layer._sub_transformer(torch.arange(4), 'cpu')[0] == 'quatprod'
    assert _layer(3, straddle=True)._blocked_ok() is False       # quaternions across degrees: the pass per degree
    assert _backward.supported(layer) and _backward.generic_supported(layer)
    layer.blocked_inverse = False
    assert layer._blocked_ok() is False
    f64 = _layer(3).double()
    assert f64._blocked_ok() is False and f64._blocked_f64_ok() is False         # float64: the pass per degree
    layer = _layer(2)
    layer.layer_kernel = True
    assert not layer._layer_kernel_ok(torch.empty(8, 8))
    # identity initialisation: the last bias is (0, 0, 0, 1) per quaternion
    layer = _layer(2, initialize_identity=True)
    bias = layer._conditioner.layers[-1].bias.detach()
    assert torch.equal(bias, torch.tensor([0., 0., 0., 1.] * 2))


def test_mixed_member_routing_and_float64_acceptance():
    from tfep_amd.nn.flows import _backward
    from tfep_amd.nn.transformers.mixed import check_float64_members
    mixed = MixedTransformer([QuaternionProductTransformer(), NeuralSplineTransformer(torch.full((4,), -4.0), torch.full((4,), 4.0), 8)],
                             [[0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11]])
    layer = MAF(generate_degrees(12, 'ascending', repeats=4), transformer=mixed, initialize_identity=False)
    assert layer._fused_kind() is None and layer._blocked_ok() is False
    assert _backward.supported(layer)
    check_float64_members(mixed)                                  # accepted in float64
    assert torch.equal(mixed.get_degrees_out(torch.arange(12))[:8], torch.arange(8))
    assert torch.equal(mixed.get_identity_parameters(12)[:8], torch.tensor([0., 0., 0., 1.] * 2))


def test_cpu_tensors_wrong_types_and_feature_counts_are_refused():
    from tfep_amd import ops
    from tfep_amd._lib import TfepHipError
    tr = QuaternionProductTransformer()
    for dt in (torch.float32, torch.float64):
        x, p = torch.randn(4, 8, dtype=dt), torch.randn(4, 8, dtype=dt)
        for fn in (tr.forward, tr.inverse, ops.quaternion_product):
            with pytest.raises(TfepHipError, match='no CPU fallback'):
                fn(x, p)
        x, p = torch.randn(4, 6, dtype=dt), torch.randn(4, 6, dtype=dt)
        for fn in (tr.forward, tr.inverse, ops.quaternion_product):
            with pytest.raises(ValueError, match='multiple of 4'):
                fn(x, p)
    with pytest.raises(ValueError, match='multiple of 4'):
        tr.get_identity_parameters(6)
    with pytest.raises(TypeError):
        ops.quaternion_product([1.0], [1.0])
    with pytest.raises(TypeError):
        tr.forward([1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])


def test_golden_holds_data_only_and_is_small():
    g = np.load(GOLDEN, allow_pickle=False)
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'symmoebius.npz'))
    for k in g.files:
        assert g[k].dtype.kind in 'fiub', k                      # plain numbers, no objects
        assert g[k].dtype.kind != 'f' or np.isfinite(g[k]).all(), k
    for n in (1, 3):
        name = f'tr/n{n}'
        for k in ('x', 'p', 'yin', 'gy'):
            assert g[f'{name}/{k}'].dtype == np.float32 and g[f'{name}/{k}'].shape == (16, 4 * n)
        assert np.linalg.norm(g[f'{name}/p'].reshape(16, n, 4), axis=-1).min() > 1e-2      # away from the NaN at p = 0
        assert g[f'{name}/y_f64'].dtype == np.float64 and g[f'{name}/y_f32'].dtype == np.float32
        for sfx in ('', '_inv'):
            assert g[f'{name}/ldj{sfx}_f64'].shape == (16,) and not g[f'{name}/ldj{sfx}_f64'].any()
            assert g[f'{name}/ldj{sfx}_f32'].dtype == np.float32 and not g[f'{name}/ldj{sfx}_f32'].any()
    for name in ('quat', 'mixquat', 'straddle'):
        assert any(k.startswith(f'{name}/sd/') for k in g.files)
        for sfx in ('', '_inv'):
            assert f'{name}/y{sfx}_f64' in g.files and f'{name}/gx{sfx}_f64' in g.files and f'{name}/loss{sfx}_f32' in g.files


@pytest.mark.parametrize('n', [1, 3])
def test_golden_against_a_hamilton_product_written_out_in_numpy(n):
    """y_f64, the inverse and the reference-autograd gradients of sum(gy * y) against numpy float64 on the same inputs."""
    g = np.load(GOLDEN)
    name = f'tr/n{n}'
    x, p, yin, gy = (g[f'{name}/{k}'].astype(np.float64).reshape(16, n, 4) for k in ('x', 'p', 'yin', 'gy'))
    norm = np.sqrt((p * p).sum(-1, keepdims=True))
    q = p / norm
    conj = np.array([-1.0, -1.0, -1.0, 1.0])
    tol = dict(rtol=0, atol=4e-15)

    def through_normalisation(gq):
        return (gq - q * (q * gq).sum(-1, keepdims=True)) / norm
    # forward: y = q (x) x
    np.testing.assert_allclose(hamilton(q, x).reshape(16, -1), g[f'{name}/y_f64'], **tol)
    np.testing.assert_allclose(hamilton(q * conj, gy).reshape(16, -1), g[f'{name}/gx_f64'], **tol)
    np.testing.assert_allclose(through_normalisation(hamilton(gy, x * conj)).reshape(16, -1), g[f'{name}/gpar_f64'], **tol)
    # inverse: x = conj(q) (x) y
    np.testing.assert_allclose(hamilton(q * conj, yin).reshape(16, -1), g[f'{name}/y_inv_f64'], **tol)
    np.testing.assert_allclose(hamilton(q, gy).reshape(16, -1), g[f'{name}/gx_inv_f64'], **tol)
    np.testing.assert_allclose(through_normalisation(hamilton(yin, gy * conj)).reshape(16, -1), g[f'{name}/gpar_inv_f64'], **tol)
    # the map is a rotation of R^4: norms are kept, and the inverse undoes the forward
    np.testing.assert_allclose(np.linalg.norm(g[f'{name}/y_f64'].reshape(16, n, 4), axis=-1), np.linalg.norm(x, axis=-1),
                               rtol=1e-14)
    y = g[f'{name}/y_f64'].reshape(16, n, 4)
    np.testing.assert_allclose(hamilton(q * conj, y), x, **tol)
    # the float32 reference run is the same map to float32 rounding
    np.testing.assert_allclose(g[f'{name}/y_f32'], g[f'{name}/y_f64'], rtol=0, atol=1e-6)


@pytest.mark.parametrize('n', [1, 3])
def test_golden_against_scipy_rotation_composition(n):
    Rotation = pytest.importorskip('scipy.spatial.transform').Rotation
    g = np.load(GOLDEN)
    name = f'tr/n{n}'
    p = g[f'{name}/p'].astype(np.float64).reshape(-1, 4)
    for inp, out, inverse in (('x', 'y_f64', False), ('yin', 'y_inv_f64', True)):
        x = g[f'{name}/{inp}'].astype(np.float64).reshape(-1, 4)
        rp = Rotation.from_quat(p)                                  # scalar last; normalises, as the transformer does
        # (from_quat normalises x too -- the stored x is a unit quaternion rounded to float32 -- so its norm is put back)
        got = ((rp.inv() if inverse else rp) * Rotation.from_quat(x)).as_quat() * np.linalg.norm(x, axis=-1, keepdims=True)
        np.testing.assert_allclose(got, g[f'{name}/{out}'].reshape(-1, 4), rtol=0, atol=4e-15)      # signs included
