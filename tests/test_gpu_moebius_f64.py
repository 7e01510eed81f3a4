"""GPU tests of the opt-in float64 Moebius transformer (``MoebiusTransformer.float64_kernels``): the kernels
``tfep_moebius_forward_f64`` / ``tfep_moebius_backward_f64``, the float64 layer routes, and member kinds 5 / 6 of the
float64 blocked inverse (``tfep_inverse_chain_vec_f64``).  Every test sets the flag on its own instances.

References: the reference's float64 fixtures (tests/golden/transformers.npz, flows.npz, grads.npz, inv_grads.npz) and, for
the shapes they do not hold, tests/moebius_ref.py on the CPU (the Jacobian through ``slogdet``: no arithmetic shared with
the kernels' closed form; tests/test_moebius_f64_host.py holds it to the fixtures at 1e-12).

Bounds, none of them taken from what the kernels return:
* transformer and VJP against the fixtures / ``moebius_ref``: the project's float64 bound, relative L2 <= 1e-10 per tensor
  and 1e-10 max(1, |log-det|) per sample;
* flows against the reference: those tests/test_gpu_float64_flows.py applies to the spline and affine flows of the same
  fixtures (forward rtol 1e-9 / atol 1e-10, log-det atol 1e-9; inverse rtol 1e-8, atol 1e-9 / 1e-8; gradients 1e-9 of the
  tensor's largest entry, the loss rtol 1e-9 forward and 1e-8 inverse);
* blocked against the pass per degree: those of tests/test_gpu_blocked_f64_vectors.py (x within 1e-10 max|x| + 1e-11,
  log-det within 1e-9 max(1, |ldj|)); the blocked route against the fixture: relative L2 <= 1e-10;
* a row alone against the same row in a batch, a graph replay against eager, float32 with against without the flag:
  ``torch.equal``;
* central differences of the float64 inverse (step 1e-4 along a random direction): truncation is step^2 / 6 = 1.7e-9 times
  the third directional derivative, round-off about 1e-16 |loss| / step = 1e-12, so 1e-5 relative holds for third
  derivatives up to several thousand times the first (the float32 test of tests/test_gpu_backward.py takes step 2e-3 and
  2 %).
"""
import functools
import json

import numpy as np
import pytest
import torch

import golden_util as gu
import moebius_ref
import test_gpu_float64_flows as tf

pytestmark = pytest.mark.gpu
F64 = torch.float64
CASES = ['d2_u0', 'd2_u1', 'd3_u0', 'd3_u1']


def rel_l2(got, ref):
    got, ref = (np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float64) for t in (got, ref))
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def ldj_err(got, ref):
    got, ref = (np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float64) for t in (got, ref))
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def check(what, y, y_ref, l, l_ref):
    ey, el = rel_l2(y, y_ref), ldj_err(l, l_ref)
    print(f'{what}: rel L2 {ey:.3e}, log-det {el:.3e} (bound 1e-10)')
    assert ey <= 1e-10 and el <= 1e-10, (what, ey, el)


def moebius(dimension, unit_sphere=False, flag=True, **kw):
    from tfep_amd.nn.transformers import MoebiusTransformer
    tr = MoebiusTransformer(dimension, unit_sphere=unit_sphere, **kw)
    if flag:
        tr.float64_kernels = True
    return tr


def opt_in(flow, vectors=False):
    """Set both switches on the instances of ``flow`` (a SequentialFlow of MAF layers)."""
    from tfep_amd.nn.transformers import MixedTransformer, MoebiusTransformer
    for layer in flow:
        tr = layer._transformer
        for t in (tr._transformers if type(tr) is MixedTransformer else [tr]):
            if type(t) is MoebiusTransformer:
                t.float64_kernels = True
        layer.blocked_inverse_f64_vectors = vectors
    return flow


def routes(flow):
    return [layer.last_inverse_route for layer in flow]


# ------------------------------------------------------------------ 1. the transformer against the reference's fixtures

@pytest.mark.parametrize('name', CASES)
def test_transformer_against_the_reference_fixtures(name):
    g = gu.load('transformers.npz')
    meta = json.loads(str(g['moebius/meta']))[f'moebius/{name}']
    tr = moebius(meta['dimension'], meta['unit_sphere'], max_radius=meta['max_radius'])
    x, par, yin = (tf.dev(g[f'moebius/{name}/{k}']) for k in ('x', 'par', 'inv_in'))
    y, l = tr(x, par)
    assert y.dtype == F64 and l.dtype == F64
    check(f'{name} forward', y, g[f'moebius/{name}/y_f64'], l, g[f'moebius/{name}/ldj_f64'])
    xi, li = tr.inverse(yin, par)
    assert xi.dtype == F64 and li.dtype == F64
    check(f'{name} inverse', xi, g[f'moebius/{name}/xinv_f64'], li, g[f'moebius/{name}/ldjinv_f64'])


# ------------------------------------------------------------------ 2. / 3. shapes, against moebius_ref

DIMS = [1, 2, 3, 5, 8]             # 2, 3: compile-time instantiations; 1, 5, 8: the runtime-dimension kernel
SHAPES = [(1, 1), (5, 65), (5, 1), (1, 65)]      # (B, vectors per row): 65 = a second pass for one lane; 5 = 4 rows per workgroup + 1


@functools.lru_cache(maxsize=None)
def shape_case(dim, unit_sphere, B, nvec):
    """Inputs, cotangents and the CPU reference (values and gradients, forward and inverse) of one shape; computed once."""
    gen = torch.Generator().manual_seed(1000 * dim + 100 * int(unit_sphere) + 10 * B + nvec)
    D = nvec * dim
    x = torch.randn(B, D, dtype=F64, generator=gen)
    if unit_sphere:
        x = (x.reshape(B, nvec, dim) / x.reshape(B, nvec, dim).norm(dim=-1, keepdim=True)).reshape(B, D)
    w = torch.randn(B, D, dtype=F64, generator=gen)
    gy, gl = torch.randn(B, D, dtype=F64, generator=gen), torch.randn(B, dtype=F64, generator=gen)
    out = dict(x=x, w=w, gy=gy, gl=gl)
    for key, fn in (('fwd', moebius_ref.moebius), ('inv', moebius_ref.moebius_inverse)):
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y, l = fn(xr, wr, dim, 0.99, unit_sphere)
        ((y * gy).sum() + (l * gl).sum()).backward()
        out[key] = (y.detach(), l.detach(), xr.grad, wr.grad)
    return out


@pytest.mark.parametrize('unit_sphere', [False, True])
@pytest.mark.parametrize('dim', DIMS)
def test_shapes_against_the_float64_restatement(dim, unit_sphere):
    tr = moebius(dim, unit_sphere)
    for B, nvec in SHAPES:
        c = shape_case(dim, unit_sphere, B, nvec)
        D = nvec * dim
        x, w = c['x'].cuda(), c['w'].cuda()
        for key, fn in (('fwd', tr.forward), ('inv', tr.inverse)):
            y_ref, l_ref = c[key][:2]
            y, l = fn(x, w)
            check(f'd={dim} u={unit_sphere} B={B} nvec={nvec} {key}', y, y_ref, l, l_ref)
            # x and the parameters as column slices of wider tensors: row strides that differ from D (and, for the
            # odd offset, rows that do not start on the boundary of a packed 2-vector)
            wide_x, wide_w = torch.zeros(B, D + 3, dtype=F64, device='cuda'), torch.zeros(B, D + 5, dtype=F64, device='cuda')
            wide_x[:, 1:D + 1], wide_w[:, 2:D + 2] = x, w
            ys, ls = fn(wide_x[:, 1:D + 1], wide_w[:, 2:D + 2])
            assert torch.equal(ys, y) and torch.equal(ls, l)
        # accumulation onto a non-zero log-det (the argument of ops.moebius)
        from tfep_amd import ops
        start = torch.linspace(-2.0, 3.0, B, dtype=F64, device='cuda')
        acc = start.clone()
        ya, la = ops.moebius(x, w, dim, 0.99, unit_sphere, log_det_J=acc)
        assert la is acc and rel_l2(ya, c['fwd'][0]) <= 1e-10
        assert ldj_err(acc, start.cpu() + c['fwd'][1]) <= 1e-10
    # a row alone against the same row inside the batch
    c = shape_case(dim, unit_sphere, 5, 65)
    x, w = c['x'].cuda(), c['w'].cuda()
    yb, lb = tr(x, w)
    for r in (0, 3, 4):
        y1, l1 = tr(x[r:r + 1].clone(), w[r:r + 1].clone())
        assert torch.equal(y1[0], yb[r]) and torch.equal(l1[0], lb[r]), (dim, unit_sphere, r)


@pytest.mark.parametrize('unit_sphere', [False, True])
@pytest.mark.parametrize('dim', DIMS)
def test_vjp_against_autograd_through_the_restatement(dim, unit_sphere):
    import tfep_amd.torch_ops  # noqa: F401
    for B, nvec in SHAPES:
        c = shape_case(dim, unit_sphere, B, nvec)
        for key, op in (('fwd', torch.ops.tfep.moebius_forward), ('inv', torch.ops.tfep.moebius_inverse)):
            x, w = c['x'].cuda().requires_grad_(True), c['w'].cuda().requires_grad_(True)
            y, l = op(x, w, dim, 0.99, unit_sphere)
            ((y * c['gy'].cuda()).sum() + (l * c['gl'].cuda()).sum()).backward()
            ex, ew = rel_l2(x.grad, c[key][2]), rel_l2(w.grad, c[key][3])
            if dim == 1 and not unit_sphere:
                # (|x|^2 - u^2) / (x - u) - u = x for every w: the parameter gradient is exactly zero, a relative error
                # against it is undefined, and both sides hold round-off only -- each is held to the bound absolutely, in
                # units of the cotangents
                scale = float(torch.cat([c['gy'].flatten(), c['gl']]).norm())
                ew = max(float(w.grad.norm()), float(c[key][3].norm())) / scale
            print(f'd={dim} u={unit_sphere} B={B} nvec={nvec} {key}: grad x {ex:.3e}, grad w {ew:.3e} (bound 1e-10)')
            assert x.grad.dtype == F64 and w.grad.dtype == F64
            assert ex <= 1e-10 and ew <= 1e-10, (dim, unit_sphere, B, nvec, key, ex, ew)


@pytest.mark.parametrize('unit_sphere', [False, True])
def test_w_zero_has_the_zero_subgradient_of_the_norm(unit_sphere):
    import tfep_amd.torch_ops  # noqa: F401
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 6, dtype=F64, generator=gen)
    if unit_sphere:
        x = (x.reshape(4, 2, 3) / x.reshape(4, 2, 3).norm(dim=-1, keepdim=True)).reshape(4, 6)
    w = torch.randn(4, 6, dtype=F64, generator=gen)
    w[1], w[2, :3] = 0.0, 0.0                                  # a whole row and one vector of a row
    gy, gl = torch.randn(4, 6, dtype=F64, generator=gen), torch.randn(4, dtype=F64, generator=gen)
    for ref_fn, op in ((moebius_ref.moebius, torch.ops.tfep.moebius_forward), (moebius_ref.moebius_inverse, torch.ops.tfep.moebius_inverse)):
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y, l = ref_fn(xr, wr, 3, 0.99, unit_sphere)
        ((y * gy).sum() + (l * gl).sum()).backward()
        xd, wd = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
        y, l = op(xd, wd, 3, 0.99, unit_sphere)
        ((y * gy.cuda()).sum() + (l * gl.cuda()).sum()).backward()
        assert bool(torch.isfinite(wd.grad).all()) and bool(torch.isfinite(xd.grad).all())
        assert rel_l2(xd.grad, xr.grad) <= 1e-10 and rel_l2(wd.grad, wr.grad) <= 1e-10


def test_opcheck_on_float64_inputs():
    import tfep_amd.torch_ops  # noqa: F401
    c = shape_case(3, False, 5, 1)
    x, w, gy, gl = (c[k].cuda() for k in ('x', 'w', 'gy', 'gl'))
    for op in (torch.ops.tfep.moebius_forward, torch.ops.tfep.moebius_inverse):
        torch.library.opcheck(op.default, (x.clone().requires_grad_(True), w.clone().requires_grad_(True), 3, 0.99, False))
        torch.library.opcheck(op.default, (x, w, 3, 0.99, False))
    torch.library.opcheck(torch.ops.tfep.moebius_backward.default, (x, w, gy, gl, 3, 0.99, False))


# ------------------------------------------------------------------ 4. the dtype contract

def test_dtype_contract():
    from tfep_amd import ops
    from tfep_amd.nn.transformers import MoebiusTransformer
    x64, x32 = torch.ones(3, 4, device='cuda', dtype=F64), torch.ones(3, 4, device='cuda')
    tr = moebius(2)
    for a, b in ((x64, x32), (x32, x64)):
        with pytest.raises(TypeError):
            tr(a, b)
        with pytest.raises(TypeError):
            tr.inverse(a, b)
        with pytest.raises(TypeError):
            ops.moebius_backward(a, b, 2, 0.99, False, a, None)
        with pytest.raises(TypeError):
            ops.moebius_backward(a, a, 2, 0.99, False, b, None)
    fresh = MoebiusTransformer(2)
    for fn in (fresh.forward, fresh.inverse):
        with pytest.raises(TypeError, match='MoebiusTransformer: float64 is not supported for the Moebius transformer yet '
                                            r'\(float32 only\)'):
            fn(x64, x64)


# ------------------------------------------------------------------ 5. flows against the reference

def f64_flow(npz_name, name, configs=None, vectors=False):
    flow, g = tf.f64_flow(npz_name, name, configs)
    return opt_in(flow, vectors), g


def test_flow_forward_and_inverse_against_the_reference():
    flow, g = f64_flow('flows.npz', 'moeb')
    with torch.no_grad():
        y, ldj = flow(tf.dev(g['moeb/x']))
        assert y.dtype == F64 and ldj.dtype == F64
        tf.close(y, g['moeb/y_f64'], 1e-9, 1e-10, 'y')
        tf.close(ldj, g['moeb/ldj_f64'], 1e-9, 1e-9, 'ldj')
        x, ldj = flow.inverse(tf.dev(g['moeb/inv_in']))
        assert routes(flow) == ['per_degree', 'per_degree']
        tf.close(x, g['moeb/xinv_f64'], 1e-8, 1e-9, 'x')
        tf.close(ldj, g['moeb/ldjinv_f64'], 1e-8, 1e-8, 'ldj')


def test_training_gradients_against_the_reference():
    from tfep_amd.loss import BoltzmannKLDivLoss
    flow, g = f64_flow('grads.npz', 'moebius', gu.grad_flow_configs())
    x = tf.dev(g['moebius/x']).requires_grad_(True)
    c, d = tf.dev(g['moebius/c']), tf.dev(g['moebius/d'])
    y, ldj = flow(x)
    assert y.requires_grad and ldj.requires_grad and y.dtype == F64
    loss = BoltzmannKLDivLoss()((c * y ** 2 + d * y).sum(dim=1), ldj)
    tf.close(loss, g['moebius/loss_f64'], 1e-9, 0, 'loss')
    loss.backward()
    tf.grad_close(x.grad, g['moebius/gx_f64'], 'gx')
    tf._check_grads(flow, g, 'moebius')


@pytest.mark.parametrize('vectors', [False, True])
def test_inverse_gradients_against_the_reference(vectors):
    """Two layers, d = 2 on the unit sphere and d = 3 general; ``vectors``: the values come from the blocked route."""
    from tfep_amd.loss import BoltzmannKLDivLoss
    flow, g = f64_flow('inv_grads.npz', 'moebius', gu.grad_flow_configs(), vectors)
    y = tf.dev(g['moebius/y']).requires_grad_(True)
    c, d = tf.dev(g['moebius/c']), tf.dev(g['moebius/d'])
    x, ldj = flow.inverse(y)
    assert routes(flow) == ['blocked_f64' if vectors else 'per_degree'] * 2
    assert x.requires_grad and ldj.requires_grad and x.dtype == F64
    tf.close(x, g['moebius/x_f64'], 1e-8, 1e-9, 'x')
    loss = BoltzmannKLDivLoss()((c * x ** 2 + d * x).sum(dim=1), ldj)
    tf.close(loss, g['moebius/loss_f64'], 1e-8, 0, 'loss')
    loss.backward()
    tf.grad_close(y.grad, g['moebius/gy_f64'], 'gy')
    tf._check_grads(flow, g, 'moebius')


# ------------------------------------------------------------------ 6. mixed

MIXED12 = [[0, 1, 4, 5], [2, 3, 6, 7], [8, 9, 10, 11]]
#: D = 24, degrees of three features each: the two components of a Moebius vector sit in slots 0 and 2 of their degree
MIXED24 = [[0, 2, 6, 8, 12, 14, 18, 20], [1, 3, 4, 5, 7, 9, 13, 19], [10, 11, 15, 16, 17, 21, 22, 23]]


def mixed_layer(D, seed=2):
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import AffineTransformer, MixedTransformer, NeuralSplineTransformer
    idx, repeats = (MIXED12, 2) if D == 12 else (MIXED24, 3)
    torch.manual_seed(seed)
    n = len(idx[1])
    tr = MixedTransformer([moebius(2), NeuralSplineTransformer(torch.full((n,), -4.0), torch.full((n,), 4.0), 8), AffineTransformer()], idx)
    return MAF(generate_degrees(D, repeats=repeats), transformer=tr, hidden_layers=[40, 40], initialize_identity=False).double().cuda()


def mixed_by_members(layer, x):
    """The layer's forward member by member: the conditioner by autograd, the Moebius member through moebius_ref on the
    CPU, the spline and affine members through their float64 ops."""
    tr, made = layer._transformer, layer._conditioner
    theta = made.layers(made._embed(x))
    splits = tr.host_splits() + [theta.shape[1]]
    y, ldj = torch.zeros_like(x), 0.0
    for k, (t, ind, a, b) in enumerate(zip(tr._transformers, tr._indices, splits[:-1], splits[1:])):
        ind = ind.to(x.device).long()
        if k == 0:
            yg, lg = moebius_ref.moebius(x[:, ind].cpu(), theta[:, a:b].cpu(), t.dimension, t.max_radius, t.unit_sphere)
            yg, lg = yg.cuda(), lg.cuda()
        else:
            yg, lg = t(x[:, ind].contiguous(), theta[:, a:b].contiguous())
        y = y.index_copy(1, ind, yg)
        ldj = ldj + lg
    return y, ldj


def test_mixed_layer_round_trip_and_gradients_member_by_member():
    D, B = 12, 33
    layer = mixed_layer(D)
    gen = torch.Generator(device='cuda').manual_seed(5)
    x0 = 1.2 * torch.randn(B, D, device='cuda', dtype=F64, generator=gen)
    c = torch.linspace(0.2, 1.0, D, device='cuda', dtype=F64)

    def loss_of(y, ldj):
        return ((c * y ** 2).sum(dim=1) + ldj).mean()
    with torch.no_grad():
        y, l_f = layer(x0)
        x1, l_i = layer.inverse(y)
    assert layer.last_inverse_route == 'per_degree'
    tf.close(x1, x0.cpu().numpy(), 1e-9, 1e-9, 'round trip')
    tf.close(l_f + l_i, np.zeros(B), 0, 1e-8, 'log-dets cancel')
    x = x0.clone().requires_grad_(True)
    y, ldj = layer(x)
    loss = loss_of(y, ldj)
    loss.backward()
    got = {'x': x.grad.clone(), **{k: p.grad.clone() for k, p in layer.named_parameters()}}
    layer.zero_grad()
    xr = x0.clone().requires_grad_(True)
    y_ref, l_ref = mixed_by_members(layer, xr)
    tf.close(y, y_ref.detach().cpu().numpy(), 1e-9, 1e-10, 'y')
    tf.close(ldj, l_ref.detach().cpu().numpy(), 1e-9, 1e-9, 'ldj')
    loss_ref = loss_of(y_ref, l_ref)
    tf.close(loss, float(loss_ref), 1e-9, 0, 'loss')
    loss_ref.backward()
    tf.grad_close(got['x'], xr.grad.cpu().numpy(), 'gx')
    for k, p in layer.named_parameters():
        tf.grad_close(got[k], p.grad.cpu().numpy(), k)


def test_mixed_layer_inverse_is_differentiable_in_float64():
    """The float64 twin of tests/test_gpu_backward.py::test_inverse_of_a_mixed_transformer_with_a_moebius_member_is_
    differentiable: central differences along random directions, for the input and for every parameter at once."""
    D, B = 12, 33
    layer = mixed_layer(D, seed=4)
    y = 0.8 * torch.randn(B, D, device='cuda', dtype=F64, generator=torch.Generator(device='cuda').manual_seed(9))
    c = torch.linspace(0.2, 1.0, D, device='cuda', dtype=F64)
    params = [p for p in layer.parameters() if p.requires_grad]

    def loss(y_):
        x, ldj = layer.inverse(y_)
        return ((c * x ** 2).sum(dim=1) + ldj).mean()
    y_req = y.clone().requires_grad_(True)
    val = loss(y_req)
    val.backward()
    gy, gp = y_req.grad.clone(), [p.grad.clone() for p in params]
    assert gy.dtype == F64 and all(bool(torch.isfinite(t).all()) for t in [gy] + gp) and float(gy.abs().max()) > 0
    with torch.no_grad():
        assert abs(float(val) - float(loss(y))) <= 1e-12 * max(1.0, abs(float(val)))
        gen = torch.Generator(device='cuda').manual_seed(4)
        eps = 1e-4
        vy = torch.randn(B, D, device='cuda', dtype=F64, generator=gen)
        fd = (float(loss(y + eps * vy)) - float(loss(y - eps * vy))) / (2 * eps)
        an = float((gy * vy).sum())
        print(f'input: central difference {fd:.10e}, backward {an:.10e}')
        assert abs(fd - an) <= 1e-5 * max(abs(an), 1e-3), (fd, an)
        vp = [torch.randn(p.shape, device='cuda', dtype=F64, generator=gen) * (p.abs().mean() + 1e-3) for p in params]
        an = float(sum((g_ * v).sum() for g_, v in zip(gp, vp)))
        vals = []
        for s_ in (+1, -1):
            for p, v in zip(params, vp):
                p.add_(s_ * eps * v)
            vals.append(float(loss(y)))
            for p, v in zip(params, vp):
                p.sub_(s_ * eps * v)
        fd = (vals[0] - vals[1]) / (2 * eps)
        print(f'parameters: central difference {fd:.10e}, backward {an:.10e}')
        assert abs(fd - an) <= 1e-5 * max(abs(an), 1e-3), (fd, an)


# ------------------------------------------------------------------ 7. the blocked inverse

BLOCKED = ['d2_unit', 'd3_general', 'mixed', 'd1']
BATCHES = [1, 64, 65, 130]


@functools.lru_cache(maxsize=None)
def blocked_layer(name):
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    torch.manual_seed(BLOCKED.index(name) + 20)
    if name == 'mixed':
        layer = mixed_layer(24, seed=21)
    else:
        dim, unit = {'d2_unit': (2, True), 'd3_general': (3, False), 'd1': (1, True)}[name]
        order = 'descending' if name == 'd3_general' else 'ascending'
        layer = MAF(generate_degrees(24, order, repeats=dim), transformer=moebius(dim, unit), hidden_layers=[40, 40],
                    initialize_identity=False).double().cuda()
    layer.blocked_inverse_f64_vectors = True
    gen = torch.Generator(device='cuda').manual_seed(11)
    y = 1.2 * torch.randn(max(BATCHES), 24, device='cuda', dtype=F64, generator=gen)
    if name == 'd2_unit':                                     # the images of a unit-sphere layer lie on the unit circle
        v = y.reshape(-1, 12, 2)
        y = (v / v.norm(dim=-1, keepdim=True)).reshape(-1, 24)
    if name == 'd1':
        # d = 1: the general map is the identity for every w ((x^2 - u^2) / (x - u) - u = x) and so is the unit-sphere map at
        # x = +-1; the unit-sphere formula just off the "sphere" (1 <= |y| <= 1.1, |u| <= 0.99) is a map that moves
        y = torch.sign(y) * (1.0 + 0.1 * torch.rand(y.shape, device='cuda', dtype=F64, generator=gen))
    return layer, y


@pytest.mark.parametrize('block', [1, 2, 16])
@pytest.mark.parametrize('name', BLOCKED)
def test_blocked_matches_pass_per_degree_and_rows_do_not_depend_on_the_batch(name, block):
    layer, y_all = blocked_layer(name)
    layer.inverse_block_f64 = block
    hp = layer._blocked_f64_host_plan()
    assert hp is not None and len(hp['blocks']) == -(-layer._inverse_masks.shape[0] // block)
    assert {'d2_unit': [6], 'd3_general': [5], 'mixed': [5, 1, 0], 'd1': [6]}[name] == hp['kinds']
    big = None
    for B in reversed(BATCHES):
        y = y_all[:B].clone()
        with torch.no_grad():
            xb, lb = layer.inverse(y)
            assert layer.last_inverse_route == 'blocked_f64'
            layer.blocked_inverse_f64_vectors = False
            xp, lp = layer.inverse(y)
            assert layer.last_inverse_route == 'per_degree'
            layer.blocked_inverse_f64_vectors = True
        assert bool(torch.isfinite(xp).all()) and bool(torch.isfinite(lp).all())
        ex, bound_x = float((xb - xp).abs().max()), 1e-10 * float(xp.abs().max()) + 1e-11
        el = float(((lb - lp).abs() / lp.abs().clamp(min=1.0)).max())
        print(f'{name} block={block} B={B}: max|dx| = {ex:.3e} (bound {bound_x:.3e}), max rel |dldj| = {el:.3e} (bound 1e-9)')
        assert ex <= bound_x and el <= 1e-9, (name, block, B, ex, bound_x, el)
        assert float((xb - y).abs().max()) > 1e-3                       # (not the identity)
        if big is None:
            big = (xb, lb)
        else:
            assert torch.equal(xb, big[0][:B]) and torch.equal(lb, big[1][:B]), (name, block, B)
    with torch.no_grad():
        for r in (63, 64, 129):
            x1, l1 = layer.inverse(y_all[r:r + 1].clone())
            assert torch.equal(x1[0], big[0][r]) and torch.equal(l1[0], big[1][r]), (name, block, r)


def test_one_flag_alone_or_a_straddling_vector_keeps_the_pass_per_degree():
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    y = torch.randn(7, 12, device='cuda', dtype=F64, generator=torch.Generator(device='cuda').manual_seed(0))
    for flag, vectors, repeats, want in ((True, True, 2, 'blocked_f64'), (True, False, 2, 'per_degree'), (True, True, 1, 'per_degree')):
        layer = MAF(generate_degrees(12, repeats=repeats), transformer=moebius(2, flag=flag), hidden_layers=[20, 20],
                    initialize_identity=False).double().cuda()
        layer.blocked_inverse_f64_vectors = vectors
        with torch.no_grad():
            layer.inverse(y)
        assert layer.last_inverse_route == want, (flag, vectors, repeats)
    # the layer's switch without the transformer's: float64 is refused as before
    layer = MAF(generate_degrees(12, repeats=2), transformer=moebius(2, flag=False), hidden_layers=[20, 20]).double().cuda()
    layer.blocked_inverse_f64_vectors = True
    with pytest.raises(TypeError, match='float64 is not supported for the Moebius transformer yet'):
        layer.inverse(y)


def test_blocked_route_against_the_reference_fixture():
    flow, g = f64_flow('flows.npz', 'moeb', vectors=True)
    with torch.no_grad():
        x, ldj = flow.inverse(tf.dev(g['moeb/inv_in']))
    assert routes(flow) == ['blocked_f64', 'blocked_f64']
    check('moeb blocked inverse', x, g['moeb/xinv_f64'], ldj, g['moeb/ldjinv_f64'])


# ------------------------------------------------------------------ 8. HIP graphs

@pytest.mark.parametrize('inverse', [False, True])
def test_graph_replay_equals_eager(inverse):
    from tfep_amd.graphs import GraphedFlow
    flow, g = f64_flow('flows.npz', 'moeb', vectors=True)
    data = tf.dev(g['moeb/inv_in' if inverse else 'moeb/x'])
    graph = GraphedFlow(flow, data.shape[0], data.shape[1], inverse=inverse)
    assert graph.static_in.dtype is F64
    for d in (data, data.flip(0)):
        with torch.no_grad():
            want = flow.inverse(d) if inverse else flow(d)
        if inverse:
            assert routes(flow) == ['blocked_f64', 'blocked_f64']
        got = graph(d)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ------------------------------------------------------------------ 9. float32 untouched

@pytest.mark.parametrize('name', ['d2_u1', 'd3_u0'])
def test_float32_bits_do_not_depend_on_the_flag(name):
    g = gu.load('transformers.npz')
    meta = json.loads(str(g['moebius/meta']))[f'moebius/{name}']
    x, par = (torch.from_numpy(g[f'moebius/{name}/{k}']).cuda() for k in ('x', 'par'))
    outs = []
    for flag in (False, True):
        tr = moebius(meta['dimension'], meta['unit_sphere'], flag=flag, max_radius=meta['max_radius'])
        outs.append((*tr(x, par), *tr.inverse(x, par)))
    assert all(t.dtype == torch.float32 for t in outs[0])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
