"""GPU tests of the blocked float64 backward through the MAF inverse for vector-valued members
(``AutoregressiveFlow.blocked_inverse_backward_vectors``, kernel ``tfep_inverse_backward_chain_vec_f64``): symmetrized
Moebius and quaternion-product layers, alone and as members of a mixed transformer beside an RQ spline.  The flows, inputs
and goldens are those of tests/test_gpu_blocked_f64_vectors.py (D = 24, hidden [40, 40]: ``sym3``, ``quat``, ``mixed``), plus
two single layers built here: 2-vectors with five vectors per degree (more than the four waves of a workgroup) and
8-vectors (the largest dimension).

Bounds, none of them taken from what the kernels return: gradients, against the reference's goldens and against the
per-degree route, max |d| <= 1e-9 max |ref| per tensor, the loss rtol 1e-9 -- the project's float64 gradient bounds
(tests/test_gpu_float64_inverse_backward.py, tests/test_gpu_blocked_f64_vectors.py); residual of the solve
1e-9 max(1, max |gx|, max |u|); batch invariance and the scalar members through either entry point: ``torch.equal``.
Inputs are images of random points: no zero vector, no zero quaternion parameter (NaN in the reference too)."""
import ctypes

import numpy as np
import pytest
import torch

import inverse_backward_cases as ibc
import test_gpu_blocked_f64_vectors as tv
from test_gpu_float64_inverse_backward import count_generic_inverse

pytestmark = pytest.mark.gpu

F64 = torch.float64
BLOCKS = (1, 2, 16)
LOCAL = ['sym2x5', 'sym8']


def set_flags(layers, vectors=True):
    for layer in layers:
        layer.blocked_inverse_f64_vectors = True
        layer.blocked_inverse_backward = True
        layer.blocked_inverse_backward_vectors = vectors


def local_layer(name):
    """A single float64 layer without a golden: seeded, non-identity weights."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import SymmetrizedMoebiusTransformer
    dim, D, repeats = {'sym2x5': (2, 40, 10), 'sym8': (8, 16, 8)}[name]
    torch.manual_seed(100 + dim)
    with ibc.default_float64():
        layer = MAF(generate_degrees(D, repeats=repeats), transformer=SymmetrizedMoebiusTransformer(dim),
                    initialize_identity=False)
    return layer.double().cuda()


def layers_of(name):
    layers = [local_layer(name)] if name in LOCAL else list(tv.build_flow(name))
    set_flags(layers)
    return layers


def images(layer, B, seed):
    D = layer._inverse_masks.shape[1]
    gen = torch.Generator(device='cuda').manual_seed(seed)
    x = 1.2 * torch.randn(B, D, device='cuda', dtype=F64, generator=gen)
    with torch.no_grad():
        return layer(x)[0]


def gradients(layer, y0, loss, vectors, block=None):
    """``[y.grad, parameter gradients ...]`` of ``loss(layer.inverse(y0))`` with ``blocked_inverse_backward_vectors = vectors``."""
    layer.blocked_inverse_backward_vectors = vectors
    if block is not None:
        layer.inverse_block_f64 = block
    y = y0.clone().requires_grad_(True)
    params = list(layer.parameters())
    x, ldj = layer.inverse(y)
    grads = torch.autograd.grad(ibc.LOSSES[loss](x, ldj), [y] + params, allow_unused=True)
    return [g if g is not None else torch.zeros_like(p) for g, p in zip(grads, [y] + params)]


# ------------------------------------------------------------------ 1. the route

@pytest.mark.parametrize('name', ['quat', 'mixed'])
def test_route_is_taken_and_makes_no_pass_per_degree(name):
    from tfep_amd.nn.flows.autoregressive import AutoregressiveFlow
    assert AutoregressiveFlow.blocked_inverse_backward_vectors is False
    layer = layers_of(name)[0]
    y0 = images(layer, 33, seed=1)
    for flag, route, calls in ((True, 'blocked_f64', 0), (False, 'per_degree', 1)):
        layer.blocked_inverse_backward_vectors = flag
        layer.last_inverse_backward_route = None
        y = y0.clone().requires_grad_(True)
        with count_generic_inverse() as counter:
            x, ldj = layer.inverse(y)
            assert layer.last_inverse_backward_route is None            # set when the backward runs
            (x.square().sum() + ldj.sum()).backward()
        assert layer.last_inverse_backward_route == route
        assert counter.n == calls
        assert layer.last_inverse_route == 'blocked_f64'
        assert y.grad is not None and bool(torch.isfinite(y.grad).all())


# ------------------------------------------------------------------ 2. the reference's gradient goldens

@pytest.mark.parametrize('name', tv.NAMES)
def test_inverse_gradients_match_the_reference_goldens(name):
    from tfep_amd.loss import BoltzmannKLDivLoss
    g = tv.golden()
    flow = tv.build_flow(name)
    set_flags(flow)
    x = tv.dev(g[f'{name}/x']).requires_grad_(True)
    c, d = tv.dev(g[f'{name}/c']), tv.dev(g[f'{name}/d'])
    y, ldj = flow.inverse(x)
    loss = BoltzmannKLDivLoss()((c * y ** 2 + d * y).sum(dim=1), ldj)
    with count_generic_inverse() as counter:
        loss.backward()
    assert counter.n == 0 and [layer.last_inverse_backward_route for layer in flow] == ['blocked_f64'] * len(flow)
    assert tv.routes(flow) == ['blocked_f64'] * len(flow)
    np.testing.assert_allclose(float(loss.detach()), float(g[f'{name}/loss_inv']), rtol=1e-9)
    errs = {'gx': tv.max_err(x.grad, g[f'{name}/gx_inv'])}
    for k, prm in flow.named_parameters():
        ref = g[f'{name}/grad_inv/{k}']
        assert prm.grad is not None and tuple(prm.grad.shape) == ref.shape and prm.grad.dtype == F64, k
        errs[k] = tv.max_err(prm.grad, ref)
    print(f'{name}: largest gradient error {max(errs.values()):.3e} (bound 1e-9)')
    assert all(e <= 1e-9 for e in errs.values()), errs


# ------------------------------------------------------------------ 3. against the per-degree route

@pytest.mark.parametrize('B', [130, 65, 1])
@pytest.mark.parametrize('name', tv.NAMES + LOCAL)
def test_blocked_backward_matches_the_per_degree_route(name, B):
    worst = 0.0
    for li, layer in enumerate(layers_of(name)):
        names = ['y'] + [k for k, _ in layer.named_parameters()]
        kinds = layer._blocked_f64_host_plan()['kinds']
        y0 = images(layer, B, seed=7 + li)
        for loss in ibc.LOSSES:
            with count_generic_inverse() as counter:
                ref = gradients(layer, y0, loss, vectors=False, block=16)
            assert layer.last_inverse_backward_route == 'per_degree' and counter.n == 1
            assert all(bool(torch.isfinite(t).all()) for t in ref)
            # Parameter gradients that are zero in exact arithmetic have no scale of their own for a relative bound: a
            # symmetrized Moebius map and a quaternion product keep |x_v| = |y_v| whatever their parameters are, so
            # sum x^2 does not depend on the weights of a layer that has only such members, and a quaternion layer's
            # log-det is the constant 0.  Both routes then return rounding noise (1e-16 .. 1e-13 of the cotangents'
            # scale); it is held to the absolute form of the bound, the one of the residual test:
            # 1e-9 max(1, max |g_y|).  g_y and every other tensor keep the relative bound.
            zero_by_symmetry = (loss == 'gx' and all(k in (2, 3) for k in kinds)) or all(k == 3 for k in kinds)
            scale = max(1.0, float(ref[0].abs().max()))
            for block in BLOCKS:
                with count_generic_inverse() as counter:
                    got = gradients(layer, y0, loss, vectors=True, block=block)
                assert layer.last_inverse_backward_route == 'blocked_f64' and counter.n == 0
                assert layer._blocked_f64_backward_plan()['block'] <= block
                for k, a, b in zip(names, got, ref):
                    if k != 'y' and zero_by_symmetry:
                        noise = max(float(a.abs().max()), float(b.abs().max()))
                        assert noise <= 1e-9 * scale, (name, li, B, loss, block, k, noise)
                        continue
                    e = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
                    worst = max(worst, e)
                    assert e <= 1e-9, (name, li, B, loss, block, k, e)
    print(f'{name} B={B}: worst relative difference to the per-degree route {worst:.3e} (bound 1e-9)')


# ------------------------------------------------------------------ 4. the residual of the solve

@pytest.mark.parametrize('name', ['mixed', 'sym8'])
def test_forward_vjp_of_the_solution_returns_gx(name):
    layer = layers_of(name)[0]
    D = layer._inverse_masks.shape[1]
    y0 = images(layer, 130, seed=5)
    gen = torch.Generator(device='cuda').manual_seed(11)
    gx = torch.randn(130, D, device='cuda', dtype=F64, generator=gen)
    gl = torch.randn(130, device='cuda', dtype=F64, generator=gen)
    y = y0.clone().requires_grad_(True)
    x, ldj = layer.inverse(y)
    (u,) = torch.autograd.grad([x, ldj], [y], [gx, gl])
    assert layer.last_inverse_backward_route == 'blocked_f64'
    x_ = x.detach().clone().requires_grad_(True)
    y2, l2 = layer(x_)
    # J^T u + gl grad_x ldj_f = gx: the forward layer's own VJP with the cotangents (u, gl)
    (back,) = torch.autograd.grad([y2, l2], [x_], [u, gl])
    res = float((back - gx).abs().max())
    bound = 1e-9 * max(1.0, float(gx.abs().max()), float(u.abs().max()))
    print(f'{name}: residual {res:.3e} (bound {bound:.3e})')
    assert res <= bound


# ------------------------------------------------------------------ 5. batch invariance

def test_blocked_backward_is_bitwise_batch_invariant():
    layer = layers_of('mixed')[0]
    y0 = images(layer, 130, seed=3)
    full = gradients(layer, y0, 'both', vectors=True)
    again = gradients(layer, y0, 'both', vectors=True)
    assert layer.last_inverse_backward_route == 'blocked_f64'
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    for r in (0, 63, 64, 129):
        alone = gradients(layer, y0[r:r + 1].clone(), 'both', vectors=True)
        assert torch.equal(alone[0][0], full[0][r]), r


# ------------------------------------------------------------------ 6. scalar members: either entry point, the same bits

def test_scalar_members_give_the_same_bits_through_the_vector_entry_point():
    layer, D, dom = ibc.make_layer('mixed')
    y0 = ibc.inputs(layer, D, dom, 130, seed=9)['tails']
    calls = []
    from tfep_amd import _lib
    orig = _lib.call

    def spy(name, *a):
        if name.startswith('tfep_inverse_backward_chain'):
            calls.append(name)
        return orig(name, *a)
    _lib.call = spy
    try:
        for block in BLOCKS:
            scalar, _ = ibc.gradients(layer, y0, 'both', flag=True, block=block)
            assert set(calls) == {'tfep_inverse_backward_chain_f64'}
            del calls[:]
            layer._blocked_backward_force_vec = True
            vec, _ = ibc.gradients(layer, y0, 'both', flag=True, block=block)
            layer._blocked_backward_force_vec = False
            assert set(calls) == {'tfep_inverse_backward_chain_vec_f64'}
            del calls[:]
            assert layer.last_inverse_backward_route == 'blocked_f64'
            assert all(torch.equal(a, b) for a, b in zip(scalar, vec)), block
    finally:
        _lib.call = orig


# ------------------------------------------------------------------ 7. Moebius keeps the pass per degree

def test_moebius_keeps_the_pass_per_degree():
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import MoebiusTransformer
    torch.manual_seed(3)
    tr = MoebiusTransformer(2)
    tr.float64_kernels = True
    with ibc.default_float64():
        layer = MAF(generate_degrees(8, repeats=2), transformer=tr, initialize_identity=False)
    layer = layer.double().cuda()
    set_flags([layer])
    y = images(layer, 9, seed=2).requires_grad_(True)
    with count_generic_inverse() as counter:
        x, ldj = layer.inverse(y)
        (x.square().sum() + ldj.sum()).backward()
    assert layer.last_inverse_route == 'blocked_f64' and layer.last_inverse_backward_route == 'per_degree' and counter.n == 1


# ------------------------------------------------------------------ 8. empty batch, C ABI

def test_empty_batch_runs_and_launches_nothing():
    layer = layers_of('quat')[0]

    def never(*a, **k):
        raise AssertionError('the blocked solve was entered for an empty batch')
    layer._inverse_backward_blocked_f64 = never
    y = torch.empty(0, 24, device='cuda', dtype=F64, requires_grad=True)
    x, ldj = layer.inverse(y)
    assert tuple(x.shape) == (0, 24) and tuple(ldj.shape) == (0,)
    (x.square().sum() + ldj.sum()).backward()
    assert layer.last_inverse_backward_route == 'blocked_f64'
    assert tuple(y.grad.shape) == (0, 24)
    for p in layer.parameters():
        assert p.grad is not None and p.grad.shape == p.shape and float(p.grad.abs().max()) == 0.0


def test_inverse_backward_chain_vec_f64_argument_checks():
    """Every case is refused (or returns) before a launch: no kernel runs here."""
    from tfep_amd import _lib
    _lib.load()
    with pytest.raises(ValueError, match='descriptor is NULL'):
        _lib.call('tfep_inverse_backward_chain_vec_f64', None, None)
    buf = torch.zeros(4, 32, device='cuda', dtype=F64)
    tab = torch.zeros(64, device='cuda', dtype=torch.int32)
    p = buf.data_ptr()

    def desc(kind=3, dim=4, radius=0.0, chain=None, **kw):
        v = _lib.InverseBackwardChainVecF64Desc()
        d = v.chain
        d.B, d.n_linears, d.n_steps = 1, 2, 1
        d.r, d.tau_x, d.ldr, d.A, d.c, d.ldA, d.u, d.ldu = p, p, 32, p, p, 32, p, 32
        d.steps, d.feats = tab.data_ptr(), tab.data_ptr()
        for l in range(2):
            d.ga[l], d.ldga[l], d.wt[l], d.ldwt[l], d.h[l], d.ldh[l], d.G[l], d.ldG[l] = p, 32, p, 32, p, 32, p, 32
            d.R[l] = 16
            d.lds_row0[l] = 16 * l
        v.n_members, v.member_kind[0], v.member_dim[0], v.member_max_radius[0] = 1, kind, dim, radius
        v.y, v.ldy, v.theta, v.ldtheta, v.gl = p, 32, p, 32, p
        for k, val in (chain or {}).items():
            setattr(d, k, val)
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    def call(v):
        _lib.call('tfep_inverse_backward_chain_vec_f64', ctypes.byref(v), _lib.stream_of(buf))

    # no-ops: an empty batch (pointers unused), a block without steps
    call(desc(chain=dict(B=0, r=None, u=None), y=None, theta=None, gl=None))
    call(desc(2, 3, 0.99, chain=dict(n_steps=0)))
    for args, msg in [((4, 4, 0.5), 'kind must be'), ((5, 2, 0.5), 'kind must be'), ((7, 4, 0.5), 'kind must be'),
                      ((-1, 4, 0.5), 'kind must be'), ((2, 1, 0.5), 'must be in 2..8'), ((2, 9, 0.5), 'must be in 2..8'),
                      ((3, 3, 0.5), 'must be 4'), ((3, 5, 0.5), 'must be 4'), ((2, 3, 0.0), 'max_radius'),
                      ((2, 3, 1.0), 'max_radius'), ((2, 3, float('nan')), 'max_radius')]:
        with pytest.raises(ValueError, match=msg):
            call(desc(*args))
    for kw, msg in [(dict(n_members=0), 'n_members'), (dict(n_members=5), 'n_members'),
                    (dict(y=None), 'NULL pointer'), (dict(theta=None), 'NULL pointer'), (dict(gl=None), 'NULL pointer'),
                    (dict(y=p + 4), 'aligned'), (dict(theta=p + 4), 'aligned'), (dict(gl=p + 4), 'aligned'),
                    (dict(ldy=0), 'row strides of y / theta'), (dict(ldtheta=0), 'row strides of y / theta')]:
        with pytest.raises(ValueError, match=msg):
            call(desc(**kw))
    # the checks of tfep_inverse_backward_chain_f64 apply
    for chain, msg in [(dict(B=-1), 'negative batch'), (dict(n_linears=6), 'n_linears'), (dict(n_steps=-1), 'negative step'),
                       (dict(r=None), 'NULL pointer'), (dict(ldu=0), 'row strides')]:
        with pytest.raises(ValueError, match=msg):
            call(desc(chain=chain))
    # tau_x / A / c may be NULL only when no member is element-wise
    with pytest.raises(ValueError, match='NULL pointer'):
        call(desc(0, 0, 0.0, chain=dict(tau_x=None)))
