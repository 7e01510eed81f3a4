"""GPU tests of the sum-of-squares polynomial transformer (reference transformers/sos.py) on its HIP kernels: the
element-wise forward / VJP kernels, the fused MADE output-layer epilogue (exact-fp32 and split-f16), training through the
layer backward, float64 layers, routing of the (missing) inverse, HIP-graph replay, against tests/golden/sos.npz."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sos.npz')
D_FLOW = 10


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _golden():
    return np.load(GOLDEN)


def build_flow(name, g=None):
    """The tfep_amd twin of tools/gen_golden.py:sos_flows(name), weights from the golden (reference state_dict schema)."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF, SequentialFlow
    from tfep_amd.nn.transformers import MixedTransformer, NeuralSplineTransformer, SOSPolynomialTransformer
    D = D_FLOW
    if name == 'flow':
        flow = SequentialFlow(
            MAF(generate_degrees(D, 'ascending'), transformer=SOSPolynomialTransformer(2), initialize_identity=False),
            MAF(generate_degrees(D, 'descending'), transformer=SOSPolynomialTransformer(3), weight_norm=False,
                initialize_identity=False))
    else:
        mixed = MixedTransformer(
            [SOSPolynomialTransformer(2), NeuralSplineTransformer(torch.full((5,), -4.0), torch.full((5,), 4.0), 8)],
            [[0, 2, 4, 6, 8], [1, 3, 5, 7, 9]])
        flow = SequentialFlow(MAF(generate_degrees(D, 'ascending'), transformer=mixed, initialize_identity=False))
    if g is not None:
        sd = flow.state_dict()
        prefix = f'{name}/sd/'
        gold = {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}
        assert set(gold) == {k for k in sd if not k.endswith('.mask')}
        for k, v in gold.items():
            t = torch.from_numpy(np.asarray(v))
            assert t.shape == sd[k].shape and t.dtype == sd[k].dtype, k
            sd[k] = t
        flow.load_state_dict(sd, strict=True)
    return flow.cuda()


def _set_path(flow, path):
    for layer in flow:
        layer.fused = path != 'generic'
        layer.split_gemm = path == 'split'


# ------------------------------------------------------------------ the transformer

@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_transformer_forward_and_gradients_against_the_reference(dtype):
    from tfep_amd.nn.transformers import SOSPolynomialTransformer
    g = _golden()
    tol = 1e-6 if dtype == torch.float32 else 1e-12
    for K in (2, 3, 5):
        for D in (2, 5, 8):
            name = f'tr/K{K}_D{D}'
            x = torch.from_numpy(g[f'{name}/x']).to('cuda', dtype).requires_grad_(True)
            p = torch.from_numpy(g[f'{name}/par']).to('cuda', dtype).requires_grad_(True)
            w = torch.from_numpy(g[f'{name}/w']).to('cuda', dtype)
            y, ldj = SOSPolynomialTransformer(K)(x, p)
            assert y.dtype == dtype and ldj.dtype == dtype and ldj.shape == (x.shape[0],)
            assert y.requires_grad and ldj.requires_grad is False
            (y * w).sum().backward()
            ref_l = g[f'{name}/ldj_f64']
            assert rel(y.detach().cpu(), g[f'{name}/y_f64']) <= tol, name
            err_l = np.abs(ldj.cpu().numpy() - ref_l)
            assert bool((err_l <= 10 * tol * np.maximum(1.0, np.abs(ref_l))).all()), (name, err_l.max())
            assert rel(x.grad.cpu(), g[f'{name}/gx_f64']) <= tol, name
            assert rel(p.grad.cpu(), g[f'{name}/gpar_f64']) <= tol, name


def test_gradcheck_float64():
    from tfep_amd import torch_ops  # noqa: F401
    gen = torch.Generator(device='cuda').manual_seed(3)
    for K, D in ((2, 3), (3, 4)):
        x = torch.randn(3, D, device='cuda', dtype=torch.float64, generator=gen).requires_grad_(True)
        p = torch.randn(3, (2 * K + 1) * D, device='cuda', dtype=torch.float64, generator=gen).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda a, b: torch.ops.tfep.sos_forward(a, b, K)[0], (x, p))


def test_opcheck_and_dtype_errors():
    import tfep_amd.torch_ops as to
    gen = torch.Generator(device='cuda').manual_seed(4)
    for dt in (torch.float32, torch.float64):
        x = torch.randn(5, 6, device='cuda', dtype=dt, generator=gen)
        p = torch.randn(5, 5 * 6, device='cuda', dtype=dt, generator=gen)
        gy = torch.randn(5, 6, device='cuda', dtype=dt, generator=gen)
        samples = {'sos_forward': [(x, p, 2), (x.requires_grad_(True), p.requires_grad_(True), 2)],
                   'sos_backward': [(x.detach(), p.detach(), 2, gy)]}
        for name in to.SOS_OPS:
            for args in samples[name]:
                torch.library.opcheck(getattr(torch.ops.tfep, name).default, args)
    x32 = torch.randn(5, 6, device='cuda')
    with pytest.raises(TypeError):
        torch.ops.tfep.sos_forward(x32, torch.randn(5, 30, device='cuda', dtype=torch.float64), 2)
    with pytest.raises(TypeError):
        torch.ops.tfep.sos_backward(x32.double(), torch.randn(5, 30, device='cuda', dtype=torch.float64), 2, x32)
    with pytest.raises(ValueError):
        torch.ops.tfep.sos_forward(x32, torch.randn(5, 31, device='cuda'), 2)


@pytest.mark.parametrize('K', [2, 3, 4])
def test_affine_equivalence(K):
    """reference tests/nn/transformers/test_sos.py: a0 = shift and a_k0 = sqrt(exp(log-scale) / K) is the affine map."""
    from tfep_amd.nn.transformers import AffineTransformer, SOSPolynomialTransformer
    gen = torch.Generator(device='cuda').manual_seed(K)
    B, D = 2, 5
    for dt in (torch.float64, torch.float32):
        x = torch.randn(B, D, device='cuda', dtype=dt, generator=gen)
        ap = torch.randn(B, 2, D, device='cuda', dtype=dt, generator=gen)
        sp = torch.zeros(B, 1 + 2 * K, D, device='cuda', dtype=dt)
        sp[:, 0] = ap[:, 0]
        sp[:, 1::2] = torch.sqrt(torch.exp(ap[:, 1]) / K)[:, None]
        ya, la = AffineTransformer()(x, ap.reshape(B, -1))
        ys, ls = SOSPolynomialTransformer(K)(x, sp.reshape(B, -1))
        assert torch.allclose(ya, ys, rtol=1e-5, atol=1e-6) and torch.allclose(la, ls, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------ flows

@pytest.mark.parametrize('path', ['exact', 'split', 'generic'])
@pytest.mark.parametrize('name', ['flow', 'mixed'])
def test_flow_forward_and_loss_gradients_against_the_reference(name, path):
    from tfep_amd.loss import BoltzmannKLDivLoss
    g = _golden()
    flow = build_flow(name, g)
    _set_path(flow, path)
    x = torch.from_numpy(g[f'{name}/x']).cuda().requires_grad_(True)
    c, d = torch.from_numpy(g[f'{name}/c']).cuda(), torch.from_numpy(g[f'{name}/d']).cuda()
    with torch.no_grad():
        y0, l0 = flow(x)
    assert rel(y0.cpu(), g[f'{name}/y_f64']) <= 1e-5
    assert np.abs(l0.cpu().numpy() - g[f'{name}/ldj_f64']).max() <= 1e-5 * max(1.0, np.abs(g[f'{name}/ldj_f64']).max())
    y, ldj = flow(x)
    assert torch.equal(y.detach(), y0) and torch.equal(ldj.detach(), l0)
    loss = BoltzmannKLDivLoss()((c * y ** 2 + d * y).sum(dim=1), ldj)
    np.testing.assert_allclose(float(loss.detach()), float(g[f'{name}/loss_f64']), rtol=2e-5)
    loss.backward()
    assert rel(x.grad.cpu(), g[f'{name}/gx_f64']) < 5e-5
    for k, p in flow.named_parameters():
        ref = g[f'{name}/grad_f64/{k}']
        assert p.grad is not None and tuple(p.grad.shape) == ref.shape, k
        err = np.abs(p.grad.cpu().numpy().astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-8)
        assert err < 2e-4, (k, err)


@pytest.mark.parametrize('name', ['flow', 'mixed'])
def test_float64_flow_against_the_reference(name):
    from tfep_amd.loss import BoltzmannKLDivLoss
    g = _golden()
    flow = build_flow(name, g).double()
    x = torch.from_numpy(g[f'{name}/x']).cuda().double().requires_grad_(True)
    c, d = (torch.from_numpy(g[f'{name}/{k}']).cuda().double() for k in ('c', 'd'))
    y, ldj = flow(x)
    assert y.dtype == torch.float64
    assert rel(y.detach().cpu(), g[f'{name}/y_f64']) <= 1e-12
    assert np.abs(ldj.detach().cpu().numpy() - g[f'{name}/ldj_f64']).max() <= 1e-12 * max(1.0, np.abs(g[f'{name}/ldj_f64']).max())
    loss = BoltzmannKLDivLoss()((c * y ** 2 + d * y).sum(dim=1), ldj)
    loss.backward()
    np.testing.assert_allclose(float(loss.detach()), float(g[f'{name}/loss_f64']), rtol=1e-12)
    assert rel(x.grad.cpu(), g[f'{name}/gx_f64']) < 1e-10
    for k, p in flow.named_parameters():
        ref = g[f'{name}/grad_f64/{k}']
        assert np.abs(p.grad.cpu().numpy() - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1e-8), k


def test_mixed_fused_equals_generic_and_stays_on_the_fused_path():
    """A MixedTransformer with an SOS member keeps the one-launch-per-group fused forward; it equals the generic path."""
    from tfep_amd.nn.flows.autoregressive import _FUSED_MIXED
    g = _golden()
    flow = build_flow('mixed', g)
    layer = flow[0]
    x = torch.from_numpy(g['mixed/x']).cuda()
    assert layer._fused_kind() == _FUSED_MIXED
    plan = layer._fused_plan(x.device, _FUSED_MIXED, layer._tables(x.device))
    assert [grp['kind'] for grp in plan['groups']] == [3, 1]          # the SOS group, then the spline group
    assert [grp['P'] * grp['FT'] for grp in plan['groups']] == [15, 25]
    out = {}
    with torch.no_grad():
        for path in ('exact', 'split', 'generic'):
            _set_path(flow, path)
            out[path] = flow(x)
    ys, ls = out['split']
    (ye, le), (yg, lg) = out['exact'], out['generic']
    for yy, ll in ((ye, le), (ys, ls)):
        assert rel(yy.cpu(), yg.cpu()) <= 1e-5 and float((ll - lg).abs().max()) <= 1e-5 * max(1.0, float(lg.abs().max()))


def test_identity_initialised_layer_is_the_identity():
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import SOSPolynomialTransformer
    D = 40
    x = torch.randn(300, D, generator=torch.Generator().manual_seed(5)).cuda()
    for K in (2, 3, 4):
        layer = MAF(generate_degrees(D), transformer=SOSPolynomialTransformer(K)).cuda()
        for path in ('exact', 'split', 'generic'):
            _set_path([layer], path)
            with torch.no_grad():
                y, l = layer(x)
            assert torch.allclose(y, x, atol=1e-5), (K, path)
            assert float(l.abs().max()) < 1e-4, (K, path)


@pytest.mark.parametrize('path', ['exact', 'split', 'generic'])
def test_rows_do_not_depend_on_the_batch(path):
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import SOSPolynomialTransformer
    D = 96
    torch.manual_seed(6)
    layer = MAF(generate_degrees(D), transformer=SOSPolynomialTransformer(2), initialize_identity=False).cuda()
    _set_path([layer], path)
    x = torch.randn(700, D, generator=torch.Generator().manual_seed(7)).cuda()
    with torch.no_grad():
        y, l = layer(x)
        ys, ls = layer(x[301:330].contiguous())
    assert torch.equal(y[301:330], ys) and torch.equal(l[301:330], ls)
    if path == 'generic':                                       # and the float64 layer
        layer64 = copy.deepcopy(layer).double()
        with torch.no_grad():
            y, l = layer64(x.double())
            ys, ls = layer64(x[301:330].double().contiguous())
        assert torch.equal(y[301:330], ys) and torch.equal(l[301:330], ls)


def test_inverse_raises_the_reference_error_in_both_grad_modes():
    g = _golden()
    msg = 'Inversion of SOS polynomial transformer has not been implemented yet.'
    for name in ('flow', 'mixed'):
        flow = build_flow(name, g)
        y = torch.from_numpy(g[f'{name}/x']).cuda()
        with torch.no_grad():
            with pytest.raises(NotImplementedError, match=msg):
                flow.inverse(y)
            with pytest.raises(NotImplementedError, match=msg):
                flow[0].inverse(y)
        with pytest.raises(NotImplementedError, match=msg):
            flow.inverse(y.clone().requires_grad_(True))
        with pytest.raises(NotImplementedError, match=msg):
            flow.double().inverse(y.double())
    torch.cuda.synchronize()
    # the device is fine afterwards
    with torch.no_grad():
        flow = build_flow('flow', g)
        yy, _ = flow(torch.from_numpy(g['flow/x']).cuda())
    assert bool(torch.isfinite(yy).all())


def test_graphed_flow_replay_equals_eager():
    from tfep_amd.graphs import GraphedFlow
    g = _golden()
    flow = build_flow('flow', g)
    x = torch.from_numpy(g['flow/x']).cuda()
    with torch.no_grad():
        y0, l0 = flow(x)
        gf = GraphedFlow(flow, x.shape[0], D_FLOW)
        y1, l1 = gf(x)
        assert torch.equal(y0, y1) and torch.equal(l0, l1)
        x2 = x * 0.5
        y2, l2 = gf(x2)
        ye, le = flow(x2)
        assert torch.equal(y2, ye) and torch.equal(l2, le)


# ------------------------------------------------------------------ cfg2 width

_CFG2 = {}


@pytest.mark.parametrize('path', ['split', 'exact', 'generic'])
def test_cfg2_width_layer_against_its_float64_copy(path):
    """One MAF + SOS(2) layer at the BASELINE cfg2 width (D = 3000, hidden 14 998, P D = 15 000) at B = 8192:
    every forward path against the same layer run in float64 (a ``.double()`` copy of the float32 weights) to the error
    budget of the cfg2 spline parity test, rel L2(y) <= 1e-5."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import SOSPolynomialTransformer
    D, B = 3000, 8192
    if 'layer' not in _CFG2:
        torch.manual_seed(0)
        with torch.device('cuda'):
            layer = MAF(generate_degrees(D, 'ascending'), transformer=SOSPolynomialTransformer(2), hidden_layers=[14998, 14998],
                        initialize_identity=False)
        x = torch.randn(B, D, generator=torch.Generator().manual_seed(1234)).cuda()
        with torch.no_grad():
            y64, l64 = copy.deepcopy(layer).double()(x.double())
        _CFG2.update(layer=layer, x=x, ref=(y64.cpu().numpy(), l64.cpu().numpy()))
    layer, x = _CFG2['layer'], _CFG2['x']
    y64, l64 = _CFG2['ref']
    _set_path([layer], path)
    with torch.no_grad():
        y, l = layer(x)
    y, l = y.cpu().numpy(), l.cpu().numpy().astype(np.float64)
    r = rel(y, y64)
    err_l = np.abs(l - l64)
    print(f'cfg2 SOS layer ({path}) vs float64: rel L2(y) {r:.2e}, max |d ldj| {err_l.max():.2e} '
          f'(|ldj| median {np.median(np.abs(l64)):.1f})')
    assert r <= 1e-5
    assert bool((err_l <= 1e-4 * np.maximum(1.0, np.abs(l64))).all()), err_l.max()
