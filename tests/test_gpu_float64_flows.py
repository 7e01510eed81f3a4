"""GPU tests of float64 flows: the float64 transformer kernels (affine, volume-preserving shift, RQ spline in every layout,
mixed, periodic embedding), MADE, MAF / SequentialFlow forward, inverse and training, and the float64 loss -- against the
float64 goldens of tests/golden/, to the tolerances tests/test_oracle_golden.py holds the float64 numpy oracle to.

Transformers are built under ``torch.set_default_dtype(torch.float64)`` (their scalar buffers, e.g. ``min_bin_size``,
then hold the reference's float64 values); flows are built from the float32 fixture state and converted with
``.double()``, as a user would."""
import contextlib
import json

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

F64 = torch.float64
NON_MOEBIUS = ['affine', 'spline', 'circular', 'identslopes', 'mixed', 'learnlow', 'learnup', 'learnboth']


def dev(a, dtype=F64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def close(got, ref, rtol, atol=0.0, what=''):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, np.asarray(ref, np.float64), rtol=rtol, atol=atol, err_msg=what)


def grad_close(got, ref, what):
    """max |got - ref| <= 1e-9 max |ref| (per tensor)."""
    got = got.detach().cpu().numpy()
    ref = np.asarray(ref, np.float64)
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)
    assert err <= 1e-9, (what, err)


@contextlib.contextmanager
def default_float64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def f64_flow(npz_name, name, configs=None):
    g = gu.load(npz_name)
    flow = gu.build_flow(name, g, configs=configs).double()
    assert all(p.dtype == F64 for p in flow.parameters())
    return flow, g


# ------------------------------------------------------------------ 1. transformers

def test_affine_and_volume_preserving_shift_float64():
    from tfep_amd.nn.transformers import AffineTransformer, VolumePreservingShiftTransformer
    g = gu.load('transformers.npz')
    t = AffineTransformer()
    y, l = t(dev(g['affine/x']), dev(g['affine/par']))
    assert y.dtype == F64 and l.dtype == F64
    close(y, g['affine/y_f64'], 1e-12, 1e-14, 'y')
    close(l, g['affine/ldj_f64'], 1e-12, 1e-12, 'ldj')
    x, l = t.inverse(dev(g['affine/inv_in']), dev(g['affine/par']))
    close(x, g['affine/xinv_f64'], 1e-12, 1e-14, 'x')
    close(l, g['affine/ldjinv_f64'], 1e-12, 1e-12, 'ldj inverse')

    t = VolumePreservingShiftTransformer(torch.from_numpy(g['volpres/periodic_indices']),
                                         torch.from_numpy(g['volpres/periodic_limits']))
    y, l = t(dev(g['volpres/x']), dev(g['volpres/par']))
    assert y.dtype == F64 and torch.all(l == 0)
    close(y, g['volpres/y_f64'], 1e-12, 1e-14, 'volpres y')
    x, l = t.inverse(y, dev(g['volpres/par']))
    pidx = g['volpres/periodic_indices'].astype(np.int64)
    lo, hi = (float(v) for v in g['volpres/periodic_limits'])
    # Python `%` in fp64: the inverse lands where (y - b) % period + lower puts it
    ref = g['volpres/y_f64'] - g['volpres/par'].astype(np.float64)
    ref[:, pidx] = np.mod(ref[:, pidx], hi - lo) + lo
    close(x, ref, 1e-12, 1e-14, 'volpres inverse')
    xi, li = t.inverse(dev(g['volpres/inv_in']), dev(g['volpres/par']))
    close(xi, g['volpres/xinv_f64'], 1e-12, 1e-14, 'volpres inverse golden')
    assert torch.all(li == 0)


def _spline_names():
    return sorted(json.loads(str(gu.load('transformers.npz')['spline/meta'])).keys())


def _spline(meta):
    with default_float64():
        t = gu.build_transformer(dict(type='spline', x0=meta['x0'], xf=meta['xf'], n_bins=meta['n_bins'],
                                      y0=meta['y0'], yf=meta['yf'], circular=meta['circular'],
                                      identity_boundary_slopes=meta['identity_boundary_slopes'],
                                      learn_lower_bound=meta['learn_lower_bound'],
                                      learn_upper_bound=meta['learn_upper_bound']))
    return t.double().cuda()


@pytest.mark.parametrize('name', _spline_names())
def test_spline_variants_float64(name):
    g = gu.load('transformers.npz')
    t = _spline(json.loads(str(g['spline/meta']))[name])
    par = dev(g[name + '/par'])
    y, l = t(dev(g[name + '/x']), par)
    assert y.dtype == F64 and l.dtype == F64
    close(y, g[name + '/y_f64'], 1e-10, 1e-11, 'y')
    close(l, g[name + '/ldj_f64'], 1e-10, 1e-10, 'ldj')
    x, l = t.inverse(dev(g[name + '/inv_in']), par)
    close(x, g[name + '/xinv_f64'], 1e-9, 1e-10, 'x')
    close(l, g[name + '/ldjinv_f64'], 1e-9, 1e-9, 'ldj inverse')


def test_spline_float64_every_bin_count_round_trips():
    """n_bins 1 .. 32 (the three kernel instantiations), in and out of the domain: inverse(forward(x)) == x and the two
    log-dets cancel."""
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    gen = torch.Generator(device='cuda').manual_seed(3)
    D, B = 5, 33
    for K in (1, 2, 7, 8, 9, 16, 17, 31, 32):
        with default_float64():
            t = NeuralSplineTransformer(torch.full((D,), -2.0), torch.full((D,), 2.0), K).cuda()
        P = t.n_parameters_per_feature
        par = torch.randn(B, P * D, device='cuda', dtype=F64, generator=gen)
        x = 3.0 * torch.randn(B, D, device='cuda', dtype=F64, generator=gen)
        y, l = t(x, par)
        x2, l2 = t.inverse(y, par)
        assert torch.allclose(x2, x, rtol=1e-12, atol=1e-12), K
        assert torch.allclose(l + l2, torch.zeros_like(l), atol=1e-11), K


def test_mixed_and_periodic_embedding_float64():
    from tfep_amd.nn.embeddings import PeriodicEmbedding
    g = gu.load('transformers.npz')
    spec = dict(type='mixed',
                transformers=[dict(type='spline', x0=np.full(3, -1.0), xf=np.full(3, 1.0), n_bins=4),
                              dict(type='affine'),
                              dict(type='spline', x0=np.full(2, -1.0), xf=np.full(2, 1.0), n_bins=3, circular=True)],
                indices=[[0, 2, 5], [1, 3], [4, 6]])
    with default_float64():
        t = gu.build_transformer(spec)
    t = t.cuda()
    par = dev(g['mixed/par'])
    y, l = t(dev(g['mixed/x']), par)
    close(y, g['mixed/y_f64'], 1e-10, 1e-11, 'mixed y')
    close(l, g['mixed/ldj_f64'], 1e-10, 1e-10, 'mixed ldj')
    x, l = t.inverse(dev(g['mixed/inv_in']), par)
    close(x, g['mixed/xinv_f64'], 1e-9, 1e-10, 'mixed x')
    close(l, g['mixed/ldjinv_f64'], 1e-9, 1e-9, 'mixed ldj inverse')

    emb = PeriodicEmbedding(6, [0.0, 1.0], periodic_indices=[1, 2, 5]).double().cuda()
    out = emb(dev(g['pemb/x']))
    assert out.dtype == F64
    close(out, g['pemb/y_f64'], 1e-12, 1e-14, 'periodic embedding')
    # backward kernel against torch autograd of the same formula in float64
    x = dev(g['pemb/x']).requires_grad_(True)
    gout = torch.randn(out.shape, device='cuda', dtype=F64)
    (emb(x) * gout).sum().backward()
    xr = dev(g['pemb/x']).requires_grad_(True)
    t_ = (xr[:, [1, 2, 5]] - 0.0) * (2 * np.pi / 1.0)
    ref = torch.cat([xr[:, [0, 3, 4]], torch.stack([torch.cos(t_), torch.sin(t_)], dim=2).reshape(len(xr), -1)], dim=1)
    (ref * gout).sum().backward()
    assert torch.allclose(x.grad, xr.grad, rtol=1e-12, atol=1e-13)


# ------------------------------------------------------------------ 2. MADE

@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd'])
def test_made_float64(name):
    from tfep_amd.nn.conditioners import MADE
    g = gu.load('made.npz')
    meta = json.loads(str(g['meta']))[name]
    made = MADE(torch.tensor(meta['degrees_in']), torch.tensor(meta['degrees_out']), meta['hidden_layers'],
                meta['weight_norm'])
    made.load_state_dict({k: torch.from_numpy(v) for k, v in gu.sub(g, f'{name}/sd/').items()}, strict=True)
    made = made.double().cuda()
    x = dev(g[f'{name}/x'])
    y = made(x)
    assert y.dtype == F64
    close(y, g[f'{name}/y_f64'], 1e-9, 1e-10, 'y')
    h = x
    for i in range(len(made.layers) // 2):              # the hidden activations through the float64 modules
        h = made.layers[2 * i + 1](made.layers[2 * i](h))
        close(h, g[f'{name}/hidden{i}_f64'], 1e-9, 1e-10, f'hidden{i}')
    with pytest.raises(TypeError):
        made(x.float())


# ------------------------------------------------------------------ 3. / 4. flows forward and inverse

@pytest.mark.parametrize('name', ['cfg1', 'rq4', 'cond', 'circ', 'mixflow'])
def test_flow_forward_float64(name):
    flow, g = f64_flow('flows.npz', name)
    with torch.no_grad():
        y, ldj = flow(dev(g[f'{name}/x']))
    assert y.dtype == F64 and ldj.dtype == F64
    close(y, g[f'{name}/y_f64'], 1e-9, 1e-10, 'y')
    close(ldj, g[f'{name}/ldj_f64'], 1e-9, 1e-9, 'ldj')


@pytest.mark.parametrize('name', ['rq4', 'cond', 'circ', 'mixflow'])
def test_flow_inverse_float64(name):
    flow, g = f64_flow('flows.npz', name)
    rtol = 1e-7 if name == 'rq4' else 1e-8
    with torch.no_grad():
        x, ldj = flow.inverse(dev(g[f'{name}/inv_in']))
        close(x, g[f'{name}/xinv_f64'], rtol, 1e-9, 'x')
        close(ldj, g[f'{name}/ldjinv_f64'], rtol, 1e-8, 'ldj')
        # round trip x -> y -> x
        x0 = dev(g[f'{name}/x'])
        y, l_f = flow(x0)
        x1, l_i = flow.inverse(y)
    close(x1, x0.cpu().numpy(), 1e-9, 1e-9, 'round trip')
    close(l_f + l_i, np.zeros(len(x0)), 0, 1e-8, 'log-dets cancel')


# ------------------------------------------------------------------ 5. / 6. training gradients

def _check_grads(flow, g, name):
    for k, p in flow.named_parameters():
        ref = g[f'{name}/grad/{k}']
        assert p.grad is not None and tuple(p.grad.shape) == ref.shape and p.grad.dtype == F64, k
        grad_close(p.grad, ref, k)
    for layer in flow:                                       # masked weights never receive gradient
        for lin in layer._conditioner.layers[::2]:
            wv = lin.weight_v if lin.has_weight_norm else lin._parameters['weight']
            assert torch.all(wv.grad[lin.mask == 0] == 0)


@pytest.mark.parametrize('name', NON_MOEBIUS)
def test_training_gradients_float64(name):
    from tfep_amd.loss import BoltzmannKLDivLoss
    flow, g = f64_flow('grads.npz', name, gu.grad_flow_configs())
    x = dev(g[f'{name}/x']).requires_grad_(True)
    c, d = dev(g[f'{name}/c']), dev(g[f'{name}/d'])
    y, ldj = flow(x)
    assert y.requires_grad and ldj.requires_grad and y.dtype == F64
    loss = BoltzmannKLDivLoss()((c * y ** 2 + d * y).sum(dim=1), ldj)
    # (the loss is a function of the flow output: it is held to the flow forward's tolerance, not the reduction's)
    close(loss, g[f'{name}/loss_f64'], 1e-9, 0, 'loss')
    loss.backward()
    grad_close(x.grad, g[f'{name}/gx_f64'], 'gx')
    _check_grads(flow, g, name)


@pytest.mark.parametrize('name', NON_MOEBIUS)
def test_inverse_gradients_float64(name):
    from tfep_amd.loss import BoltzmannKLDivLoss
    flow, g = f64_flow('inv_grads.npz', name, gu.grad_flow_configs())
    y = dev(g[f'{name}/y']).requires_grad_(True)
    c, d = dev(g[f'{name}/c']), dev(g[f'{name}/d'])
    x, ldj = flow.inverse(y)
    assert x.requires_grad and ldj.requires_grad and x.dtype == F64
    close(x, g[f'{name}/x_f64'], 1e-8, 1e-9, 'x')
    loss = BoltzmannKLDivLoss()((c * x ** 2 + d * x).sum(dim=1), ldj)
    # (a function of the inverse's output: held to the flow inverse's tolerance)
    close(loss, g[f'{name}/loss_f64'], 1e-8, 0, 'loss')
    loss.backward()
    grad_close(y.grad, g[f'{name}/gy_f64'], 'gy')
    _check_grads(flow, g, name)


# ------------------------------------------------------------------ 7. loss

def test_boltzmann_loss_float64():
    from tfep_amd.loss import BoltzmannKLDivLoss
    g = gu.load('loss.npz')
    uB, ldj, lw, uA = (dev(g[k]) for k in ('uB', 'ldj', 'lw', 'uA'))
    L = BoltzmannKLDivLoss()

    def check(v, key):
        assert v.dtype == F64
        ref = float(g[key])
        if np.isnan(ref):
            assert torch.isnan(v), key
        else:
            np.testing.assert_allclose(float(v), ref, rtol=1e-12, err_msg=key)
    check(L(uB, ldj), 'loss_plain_f64')
    check(L(uB, ldj, ref_potentials=uA), 'loss_ref_f64')
    check(L(uB, ldj, log_weights=lw), 'loss_weighted_f64')
    check(L(uB, ldj, log_weights=lw, ref_potentials=uA), 'loss_all_f64')
    check(L(uB), 'loss_noldj_f64')
    un = uB.clone()
    un[[3, 77]] = float('nan')
    Ln = BoltzmannKLDivLoss(ignore_nan=True)
    check(Ln(un, ldj), 'loss_nan_plain_f64')
    check(Ln(un, ldj, log_weights=lw), 'loss_nan_weighted_f64')
    check(L(un, ldj), 'loss_nan_propagates_f64')
    with pytest.raises(TypeError):
        L(uB, ldj.float())


# ------------------------------------------------------------------ 8. batch independence

@pytest.mark.parametrize('name', ['rq4', 'mixflow'])
def test_row_is_bitwise_batch_independent_float64(name):
    flow, g = f64_flow('flows.npz', name)
    x0 = dev(g[f'{name}/x'])
    gen = torch.Generator(device='cuda').manual_seed(11)
    big = torch.randn(257, x0.shape[1], device='cuda', dtype=F64, generator=gen) * x0.std() + x0.mean()
    big[100] = x0[0]
    with torch.no_grad():
        y1, l1 = flow(x0[:1].clone())
        yb, lb = flow(big)
        xi1, li1 = flow.inverse(y1)
        xib, lib = flow.inverse(yb)
    assert torch.equal(y1[0], yb[100]) and torch.equal(l1[0], lb[100])
    assert torch.equal(xi1[0], xib[100]) and torch.equal(li1[0], lib[100])


# ------------------------------------------------------------------ 9. opcheck

def test_opcheck_float64_transformer_ops():
    import tfep_amd.torch_ops  # noqa: F401
    gen = torch.Generator(device='cuda').manual_seed(0)
    B, D = 5, 4

    def r(*shape, grad=False):
        return torch.randn(*shape, device='cuda', generator=gen, dtype=F64).requires_grad_(grad)
    torch.library.opcheck(torch.ops.tfep.affine_forward.default, (r(B, D, grad=True), r(B, 2 * D, grad=True)))
    torch.library.opcheck(torch.ops.tfep.affine_inverse.default, (r(B, D), r(B, 2 * D)))
    torch.library.opcheck(torch.ops.tfep.affine_backward.default, (r(B, D), r(B, 2 * D), r(B, D), r(B)))
    lo, hi = torch.full((D,), -3.0, device='cuda', dtype=F64), torch.full((D,), 3.0, device='cuda', dtype=F64)
    K = 5
    cfg = (lo, hi, lo, hi, K, False, False, False, False, 1e-4, 1e-4)
    P = 3 * K + 1
    torch.library.opcheck(torch.ops.tfep.spline_forward.default, (r(B, D, grad=True), r(B, P * D, grad=True), *cfg))
    torch.library.opcheck(torch.ops.tfep.spline_inverse.default, (r(B, D), r(B, P * D), *cfg))
    torch.library.opcheck(torch.ops.tfep.spline_backward.default, (r(B, D), r(B, P * D), r(B, D), r(B), *cfg))
    torch.library.opcheck(torch.ops.tfep.tfep_reduce.default, (r(9), r(9), r(9), r(9), None, 1.0, False))


# ------------------------------------------------------------------ 10. routing and the dtype contract

def test_float32_switches_are_inert_on_float64_layers():
    flow, g = f64_flow('flows.npz', 'rq4')
    for layer in flow:
        layer.fused, layer.split_gemm, layer.layer_kernel, layer.blocked_inverse = True, True, True, True
    with torch.no_grad():
        y, ldj = flow(dev(g['rq4/x']))
        x, ldji = flow.inverse(dev(g['rq4/inv_in']))
    close(y, g['rq4/y_f64'], 1e-9, 1e-10, 'y')
    close(ldj, g['rq4/ldj_f64'], 1e-9, 1e-9, 'ldj')
    close(x, g['rq4/xinv_f64'], 1e-7, 1e-9, 'x')


def test_mixed_dtypes_raise_type_error():
    from tfep_amd.nn.transformers import AffineTransformer
    flow, g = f64_flow('flows.npz', 'rq4')
    with pytest.raises(TypeError):
        flow(dev(g['rq4/x'], torch.float32))
    with pytest.raises(TypeError):
        flow.inverse(dev(g['rq4/inv_in'], torch.float32))
    flow32 = gu.build_flow('rq4', g)
    with pytest.raises(TypeError):
        flow32(dev(g['rq4/x']))
    t = AffineTransformer()
    with pytest.raises(TypeError):
        t(torch.zeros(3, 4, device='cuda', dtype=F64), torch.zeros(3, 8, device='cuda'))
    with pytest.raises(TypeError):
        t(torch.zeros(3, 4, device='cuda'), torch.zeros(3, 8, device='cuda', dtype=F64))


def test_float64_moebius_raises_type_error():
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import AffineTransformer, MixedTransformer, MoebiusTransformer
    t = MoebiusTransformer(2)
    with pytest.raises(TypeError, match='float64 is not supported'):
        t(torch.zeros(3, 4, device='cuda', dtype=F64), torch.zeros(3, 4, device='cuda', dtype=F64))
    maf = MAF(generate_degrees(4, repeats=2), transformer=MoebiusTransformer(2)).double().cuda()
    with pytest.raises(TypeError, match='float64 is not supported'):
        maf(torch.zeros(3, 4, device='cuda', dtype=F64))
    mixed = MixedTransformer([MoebiusTransformer(2), AffineTransformer()], [[0, 1], [2, 3]])
    maf = MAF(generate_degrees(4, repeats=2), transformer=mixed).double().cuda()
    with pytest.raises(TypeError, match='float64 is not supported'):
        maf(torch.zeros(3, 4, device='cuda', dtype=F64))
