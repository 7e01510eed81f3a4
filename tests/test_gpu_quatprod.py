"""GPU tests of the quaternion product transformer (reference transformers/quatprod.py) on its HIP kernels: forward, inverse
and the VJP of both in float32 and float64, MAF layers (forward, blocked and pass-per-degree inverse, training through the
layer backward and through the inverse), a mixed transformer with this member, against tests/golden/quatprod.npz.

Bounds: the project's parity bounds.  float32 values: rel L2 1e-5 against the ``_f64`` golden, log-det 1e-5 max(1, max|ldj|);
float64 values: rtol 1e-9, atol 1e-10 (the ``close(..., 1e-9, 1e-10)`` of tests/test_gpu_float64_flows.py; log-det atol 1e-9 as
there).  Gradients as tests/test_gpu_symmoebius.py and tests/test_gpu_backward.py: transformer 1e-5 (float32) / 1e-9 (float64)
rel L2; float32 flows loss 2e-5, input gradient 5e-5 rel L2, parameter gradients 2e-4 of the tensor's largest entry, each or
4 x the error of the reference's OWN float32 run (the stored ``*_f32`` results) where that is larger: ``f32_bound``; float64 flows
1e-9 of the largest entry.  No bound depends on what the kernels return."""
import ctypes
import os

import numpy as np
import pytest
import torch

from quatprod_ref import quat_torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'quatprod.npz')
DTYPES = [torch.float32, torch.float64]


def _np(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64)


def rel(a, b):
    a, b = _np(a), _np(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def max_err(got, ref):
    return float(np.abs(_np(got) - _np(ref)).max() / max(np.abs(_np(ref)).max(), 1e-300))


def ldj_err(got, ref):
    return float(np.abs(_np(got) - _np(ref)).max())


def f32_bound(bound, g, key, err):
    """``bound``, or 4 x the error ``err(f32, f64)`` of the reference's own float32 result where that is larger."""
    return max(bound, 4.0 * err(g[key + '_f32'], g[key + '_f64']))


def _golden():
    return np.load(GOLDEN)


def _case(g, n, dt, *keys):
    return [torch.from_numpy(g[f'tr/n{n}/{k}']).cuda().to(dt) for k in keys]


# ------------------------------------------------------------------ the transformer against the golden

@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', [1, 3])
def test_transformer_forward_and_inverse_against_the_reference(n, dt):
    from tfep_amd.nn.transformers import QuaternionProductTransformer
    g = _golden()
    x, p, yin = _case(g, n, dt, 'x', 'p', 'yin')
    tr = QuaternionProductTransformer()
    for sfx, fn, inp in (('', tr.forward, x), ('_inv', tr.inverse, yin)):
        y, ldj = fn(inp, p)
        assert y.dtype == dt and ldj.dtype == dt and y.shape == inp.shape and ldj.shape == (inp.shape[0],)
        assert bool((ldj == 0).all())                                      # exactly zero
        ref = g[f'tr/n{n}/y{sfx}_f64']
        print(f'tr/n{n}{sfx} {dt}: y rel L2 {rel(y, ref):.3e}, max abs {np.abs(_np(y) - ref).max():.3e}')
        if dt == torch.float32:
            assert rel(y, ref) <= 1e-5
        else:
            np.testing.assert_allclose(_np(y), ref, rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', [1, 3])
def test_transformer_gradients_against_the_reference(n, dt):
    """Reference-autograd gradients of sum(gy * y), both directions, through the class (the ops' autograd registrations)."""
    from tfep_amd.nn.transformers import QuaternionProductTransformer
    g = _golden()
    x, p, yin, gy = _case(g, n, dt, 'x', 'p', 'yin', 'gy')
    tr = QuaternionProductTransformer()
    tol = 1e-5 if dt == torch.float32 else 1e-9
    for sfx, fn, inp in (('', tr.forward, x), ('_inv', tr.inverse, yin)):
        xx, pp = inp.clone().requires_grad_(True), p.clone().requires_grad_(True)
        y, ldj = fn(xx, pp)
        ((gy * y).sum() + 3.0 * ldj.sum()).backward()                      # (the log-det is constant: its cotangent adds nothing)
        e_x, e_p = rel(xx.grad, g[f'tr/n{n}/gx{sfx}_f64']), rel(pp.grad, g[f'tr/n{n}/gpar{sfx}_f64'])
        print(f'tr/n{n}{sfx} {dt}: gx rel L2 {e_x:.3e}, gpar rel L2 {e_p:.3e} (bound {tol:.1e})')
        assert e_x <= tol and e_p <= tol
        assert xx.grad.dtype == dt and pp.grad.dtype == dt


# ------------------------------------------------------------------ properties of the map

@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('B,D', [(16, 4), (16, 12), (4099, 1028)])
def test_norms_flip_equivariance_identity_and_round_trip(B, D, dt):
    """The reference's shapes and one with many workgroups (4099 rows of 257 quaternions: more quaternions than lanes, a last
    block that is not full).  Norm tolerances: a few units of the format's rounding (float32 results are fp64 values rounded
    once; float64 ones carry the rounding of q and of four products)."""
    from tfep_amd import ops
    from tfep_amd.nn.transformers import QuaternionProductTransformer
    gen = torch.Generator(device='cuda').manual_seed(17 + D)
    x = torch.randn(B, D, device='cuda', dtype=dt, generator=gen)
    p = 2 * torch.randn(B, D, device='cuda', dtype=dt, generator=gen)
    tr = QuaternionProductTransformer()
    y, l = tr.forward(x, p)
    assert bool((l == 0).all()) and l.dtype == dt
    nx, ny = x.reshape(B, -1, 4).norm(dim=-1), y.reshape(B, -1, 4).norm(dim=-1)
    assert torch.allclose(ny, nx, rtol=1e-6 if dt == torch.float32 else 1e-14, atol=0)          # |y| = |x| per quaternion
    y_flip, _ = tr.forward(-x, p)
    assert torch.equal(y_flip, -y)                                                               # T(-x) = -T(x), exactly
    xb, lb = tr.inverse(y, p)
    assert bool((lb == 0).all())
    if dt == torch.float64:
        assert float((xb - x).abs().max()) <= 1e-11 * float(x.abs().max())
    else:
        assert rel(xb, x) <= 1e-5
    ref = quat_torch(x.double(), p.double())
    if dt == torch.float32:
        assert rel(y, ref) <= 1e-5
    else:
        np.testing.assert_allclose(_np(y), _np(ref), rtol=1e-9, atol=1e-10)
    ident = tr.get_identity_parameters(D).to(device='cuda', dtype=dt).expand(B, D).contiguous()
    for fn in (tr.forward, tr.inverse, lambda a, b: ops.quaternion_product(a, b)):
        y0, l0 = fn(x, ident)
        assert torch.equal(y0, x) and bool((l0 == 0).all())                                      # bit for bit


def test_zero_parameter_quaternion_is_not_finite_and_stays_local():
    """p = 0 is 0 / 0 in the reference; here too, for that quaternion only (no equality is tested at that point)."""
    from tfep_amd import ops
    for dt in DTYPES:
        gen = torch.Generator(device='cuda').manual_seed(5)
        x = torch.randn(6, 12, device='cuda', dtype=dt, generator=gen)
        p = torch.randn(6, 12, device='cuda', dtype=dt, generator=gen)
        p0 = p.clone()
        p0[2, 4:8] = 0
        for inverse in (False, True):
            y, _ = ops.quaternion_product(x, p, inverse=inverse)
            y0, l0 = ops.quaternion_product(x, p0, inverse=inverse)
            assert not bool(torch.isfinite(y0[2, 4:8]).any())
            keep = torch.ones(6, 12, dtype=torch.bool, device='cuda')
            keep[2, 4:8] = False
            assert torch.equal(y0[keep], y[keep]) and bool((l0 == 0).all())


# ------------------------------------------------------------------ VJP through the ops

@pytest.mark.parametrize('dt', DTYPES)
def test_autograd_through_the_ops_against_a_torch_restatement(dt):
    """Many rows, more quaternions than lanes; float64 torch autograd of ``quat_torch`` on the same (rounded) inputs."""
    gen = torch.Generator(device='cuda').manual_seed(9)
    B, D = 301, 4 * 130
    x = torch.randn(B, D, device='cuda', dtype=dt, generator=gen)
    p = 2 * torch.randn(B, D, device='cuda', dtype=dt, generator=gen)
    cy = torch.randn(B, D, device='cuda', dtype=dt, generator=gen)
    tol = 1e-5 if dt == torch.float32 else 1e-9
    for inverse, op in ((False, torch.ops.tfep.quaternion_product_forward), (True, torch.ops.tfep.quaternion_product_inverse)):
        xx, pp = x.clone().requires_grad_(True), p.clone().requires_grad_(True)
        y, l = op(xx, pp)
        ((cy * y).sum() + l.sum()).backward()
        xr, pr = x.double().clone().requires_grad_(True), p.double().clone().requires_grad_(True)
        (cy.double() * quat_torch(xr, pr, inverse)).sum().backward()
        e_x, e_p = rel(xx.grad, xr.grad), rel(pp.grad, pr.grad)
        print(f'inverse={inverse} {dt}: gx rel L2 {e_x:.3e}, gpar rel L2 {e_p:.3e}')
        assert e_x <= tol and e_p <= tol
        gx, gp = torch.ops.tfep.quaternion_product_backward(x, p, cy, inverse)
        assert torch.equal(gx, xx.grad) and torch.equal(gp, pp.grad)
        # only the log-det has a cotangent: zero gradients, not None
        xx.grad = pp.grad = None
        y, l = op(xx, pp)
        l.sum().backward()
        assert bool((xx.grad == 0).all()) and bool((pp.grad == 0).all())


def test_gradcheck_float64():
    gen = torch.Generator(device='cuda').manual_seed(7)
    x = torch.randn(3, 8, device='cuda', dtype=torch.float64, generator=gen).requires_grad_(True)
    p = (2 * torch.randn(3, 8, device='cuda', dtype=torch.float64, generator=gen)).requires_grad_(True)
    for op in (torch.ops.tfep.quaternion_product_forward, torch.ops.tfep.quaternion_product_inverse):
        assert torch.autograd.gradcheck(lambda a, b: op(a, b), (x, p), eps=1e-6, atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize('dt', DTYPES)
def test_opcheck(dt):
    gen = torch.Generator(device='cuda').manual_seed(8)
    x = torch.randn(5, 12, device='cuda', dtype=dt, generator=gen).requires_grad_(True)
    p = (2 * torch.randn(5, 12, device='cuda', dtype=dt, generator=gen)).requires_grad_(True)
    gy = torch.randn(5, 12, device='cuda', dtype=dt, generator=gen)
    torch.library.opcheck(torch.ops.tfep.quaternion_product_forward.default, (x, p))
    torch.library.opcheck(torch.ops.tfep.quaternion_product_inverse.default, (x, p))
    torch.library.opcheck(torch.ops.tfep.quaternion_product_backward.default, (x.detach(), p.detach(), gy, False))
    torch.library.opcheck(torch.ops.tfep.quaternion_product_backward.default, (x.detach(), p.detach(), gy, True))


# ------------------------------------------------------------------ edge cases

@pytest.mark.parametrize('dt', DTYPES)
def test_rows_do_not_depend_on_the_batch(dt):
    from tfep_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(2)
    x = torch.randn(1000, 1200, device='cuda', dtype=dt, generator=gen)                # 300 quaternions: more than lanes
    p = 2 * torch.randn(1000, 1200, device='cuda', dtype=dt, generator=gen)
    gy = torch.randn(1000, 1200, device='cuda', dtype=dt, generator=gen)
    for inverse in (False, True):
        y, l = ops.quaternion_product(x, p, inverse=inverse)
        y1, l1 = ops.quaternion_product(x[617:618], p[617:618], inverse=inverse)
        assert torch.equal(y1[0], y[617]) and torch.equal(l1[0], l[617])
        gx, gp = torch.ops.tfep.quaternion_product_backward(x, p, gy, inverse)
        gx1, gp1 = torch.ops.tfep.quaternion_product_backward(x[617:618], p[617:618], gy[617:618], inverse)
        assert torch.equal(gx1[0], gx[617]) and torch.equal(gp1[0], gp[617])


@pytest.mark.parametrize('dt', DTYPES)
def test_strided_and_unaligned_rows_take_the_scalar_path(dt):
    """Column slices as a mixed transformer hands them over: rows that start off a 16-byte boundary (every operand in turn),
    a row stride that is no multiple of 16 bytes, a column stride of 2 (copied by ``rows``): the same bits as contiguous."""
    from tfep_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(3)
    big = torch.randn(20, 43, device='cuda', dtype=dt, generator=gen)
    pbig = 2 * torch.randn(20, 43, device='cuda', dtype=dt, generator=gen)
    p = pbig[:, :12].contiguous()
    for inverse in (False, True):
        for x in (big[:, 3:15], big[:, 1:13], big[:, 4:28:2], big[:, :12]):
            assert not x.is_contiguous()
            y, l = ops.quaternion_product(x, p, inverse=inverse)
            yc, lc = ops.quaternion_product(x.contiguous(), p, inverse=inverse)
            assert torch.equal(y, yc) and torch.equal(l, lc)
        x = big[:, :12].contiguous()
        yc, _ = ops.quaternion_product(x, p, inverse=inverse)
        for ps in (pbig[:, 1:13], pbig[:, 5:17], pbig[:, :12]):                    # unaligned / strided parameters only
            ps.copy_(p)
            assert not ps.is_contiguous()
            y, _ = ops.quaternion_product(x, ps, inverse=inverse)
            assert torch.equal(y, yc)
        # the VJP kernel on strided operands and outputs (the layer backward hands it a column block of theta / gtheta)
        from tfep_amd import _lib
        sfx = '_f64' if dt == torch.float64 else ''
        size = x.element_size()
        gy = torch.randn(20, 12, device='cuda', dtype=dt, generator=gen)
        gxc, gpc = torch.ops.tfep.quaternion_product_backward(x, p, gy, inverse)
        gp_big, gx_big = torch.zeros_like(pbig), torch.zeros_like(big)
        pbig[:, 1:13].copy_(p)

        def at(t, n):
            return ctypes.c_void_p(t.data_ptr() + n * size)
        _lib.call('tfep_quaternion_product_backward' + sfx, _lib.ptr(x), 12, at(pbig, 1), 43, int(inverse), _lib.ptr(gy), 12,
                  at(gp_big, 1), 43, at(gx_big, 2), 43, 20, 12, _lib.stream_of(x))
        assert torch.equal(gp_big[:, 1:13], gpc) and torch.equal(gx_big[:, 2:14], gxc)
        assert not bool(gp_big[:, 13:].any()) and not bool(gp_big[:, :1].any())     # nothing outside the block
        assert not bool(gx_big[:, 14:].any()) and not bool(gx_big[:, :2].any())


def test_empty_batches_accumulation_and_errors():
    from tfep_amd import _lib, ops
    from tfep_amd.nn.transformers import QuaternionProductTransformer
    gen = torch.Generator(device='cuda').manual_seed(4)
    x = torch.randn(20, 12, device='cuda', generator=gen)
    p = torch.randn(20, 12, device='cuda', generator=gen)
    acc = torch.full((20,), 2.0, device='cuda')                       # an accumulated log-det is left untouched
    y, l2 = ops.quaternion_product(x, p, log_det_J=acc)
    assert l2 is acc and bool((acc == 2.0).all())
    y, l = ops.quaternion_product(x, p, log_det_J=None)
    assert bool((l == 0).all())
    tr = QuaternionProductTransformer()
    for dt in DTYPES:                                                 # B = 0
        e, ep = torch.empty(0, 12, device='cuda', dtype=dt), torch.empty(0, 12, device='cuda', dtype=dt)
        for fn in (tr.forward, tr.inverse):
            y, l = fn(e, ep)
            assert y.shape == (0, 12) and l.shape == (0,) and y.dtype == dt and l.dtype == dt
        e = torch.empty(0, 12, device='cuda', dtype=dt, requires_grad=True)
        y, l = torch.ops.tfep.quaternion_product_inverse(e, ep)
        (y.sum() + l.sum()).backward()
        assert e.grad.shape == (0, 12)
    with pytest.raises(TypeError):                                    # mixed float32 / float64
        tr.forward(x, p.double())
    with pytest.raises(TypeError):
        tr.inverse(x.double(), p)
    with pytest.raises(TypeError):
        torch.ops.tfep.quaternion_product_backward(x, p, x.double(), False)
    with pytest.raises(ValueError, match='multiple of 4'):
        tr.forward(x[:, :6].contiguous(), p[:, :6].contiguous())
    with pytest.raises(ValueError):
        ops.quaternion_product(x, p[:, :8].contiguous())              # parameters of another width
    lib = _lib.load()
    assert lib.tfep_quaternion_product(None, 12, None, 12, 0, None, 12, None, 0, 4, 12, None) != 0
    assert lib.tfep_quaternion_product_backward_f64(None, 12, None, 12, 0, None, 12, None, 12, None, 12, 4, 12, None) != 0
    assert lib.tfep_quaternion_product(_lib.ptr(x), 12, _lib.ptr(p), 12, 0, _lib.ptr(y), 12, None, 0, 20, 6, None) != 0


# ------------------------------------------------------------------ flows

def build_flow(name, g=None):
    """The tfep_amd twin of tools/gen_golden.py:quatprod_flows()[name], weights from the golden."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF, SequentialFlow
    from tfep_amd.nn.transformers import MixedTransformer, NeuralSplineTransformer, QuaternionProductTransformer
    if name == 'quat':             # D = 8: two quaternions, each inside one degree
        flow = SequentialFlow(
            MAF(generate_degrees(8, 'ascending', repeats=4), transformer=QuaternionProductTransformer(), initialize_identity=False),
            MAF(generate_degrees(8, 'descending', repeats=4), transformer=QuaternionProductTransformer(), initialize_identity=False))
    elif name == 'mixquat':        # two quaternions beside four spline features
        mixed = MixedTransformer(
            [QuaternionProductTransformer(), NeuralSplineTransformer(torch.full((4,), -4.0), torch.full((4,), 4.0), 8)],
            [[0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11]])
        flow = SequentialFlow(MAF(generate_degrees(12, 'ascending', repeats=4), transformer=mixed, initialize_identity=False))
    else:                          # 'straddle': one degree per feature
        flow = SequentialFlow(MAF(generate_degrees(8, 'ascending'), transformer=QuaternionProductTransformer(),
                                  initialize_identity=False))
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


@pytest.mark.parametrize('direction', ['forward', 'inverse'])
@pytest.mark.parametrize('name', ['quat', 'mixquat'])
def test_flow_values_loss_and_gradients_against_the_reference(name, direction):
    """float32 flows: values to the plain float32 bounds; loss, input gradient and parameter gradients to the bounds of
    tests/test_gpu_symmoebius.py (see the module docstring)."""
    from tfep_amd.loss import BoltzmannKLDivLoss
    g = _golden()
    flow = build_flow(name, g)
    sfx = '' if direction == 'forward' else '_inv'
    fn = flow.forward if direction == 'forward' else flow.inverse
    x = torch.from_numpy(g[f'{name}/x']).cuda().requires_grad_(True)
    c, d = torch.from_numpy(g[f'{name}/c']).cuda(), torch.from_numpy(g[f'{name}/d']).cuda()
    with torch.no_grad():
        y0, l0 = fn(x)
    ref_l = g[f'{name}/ldj{sfx}_f64']
    e_y, e_l = rel(y0, g[f'{name}/y{sfx}_f64']), ldj_err(l0, ref_l)
    b_l = 1e-5 * max(1.0, np.abs(ref_l).max())
    print(f'{name}{sfx}: y rel L2 {e_y:.3e} (bound 1e-5), ldj err {e_l:.3e} (bound {b_l:.3e})')
    assert e_y <= 1e-5 and e_l <= b_l
    if name == 'quat':
        assert bool((l0 == 0).all())
    y, ldj = fn(x)
    assert torch.equal(y.detach(), y0) and torch.equal(ldj.detach(), l0)
    loss = BoltzmannKLDivLoss()((c * y ** 2 + d * y).sum(dim=1), ldj)
    loss.backward()
    ref_loss = float(g[f'{name}/loss{sfx}_f64'])
    e_loss = abs(float(loss.detach()) - ref_loss) / abs(ref_loss)
    b_loss = f32_bound(2e-5, g, f'{name}/loss{sfx}', lambda a, b: abs(float(a) - float(b)) / abs(float(b)))
    e_gx, b_gx = rel(x.grad, g[f'{name}/gx{sfx}_f64']), f32_bound(5e-5, g, f'{name}/gx{sfx}', rel)
    print(f'{name}{sfx}: loss rel {e_loss:.3e} (bound {b_loss:.3e}), gx rel L2 {e_gx:.3e} (bound {b_gx:.3e})')
    assert e_loss <= b_loss and e_gx <= b_gx
    for k, prm in flow.named_parameters():
        ref = g[f'{name}/grad{sfx}_f64/{k}']
        assert prm.grad is not None and tuple(prm.grad.shape) == ref.shape, k
        err = max_err(prm.grad, ref)
        bound = max(2e-4, 4.0 * max_err(g[f'{name}/grad{sfx}_f32/{k}'], ref))
        print(f'{name}{sfx}: grad {k} max err {err:.3e} (bound {bound:.3e})')
        assert err <= bound, (k, err)


@pytest.mark.parametrize('direction', ['forward', 'inverse'])
@pytest.mark.parametrize('name', ['quat', 'mixquat'])
def test_float64_flow_against_the_reference(name, direction):
    from tfep_amd.loss import BoltzmannKLDivLoss
    g = _golden()
    flow = build_flow(name, g).double()
    sfx = '' if direction == 'forward' else '_inv'
    fn = flow.forward if direction == 'forward' else flow.inverse
    x = torch.from_numpy(g[f'{name}/x']).cuda().double().requires_grad_(True)
    c, d = (torch.from_numpy(g[f'{name}/{k}']).cuda().double() for k in ('c', 'd'))
    y, ldj = fn(x)
    assert y.dtype == torch.float64 and ldj.dtype == torch.float64
    print(f'{name}{sfx} float64: y max abs err {np.abs(_np(y) - g[f"{name}/y{sfx}_f64"]).max():.3e}')
    np.testing.assert_allclose(_np(y), g[f'{name}/y{sfx}_f64'], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(_np(ldj), g[f'{name}/ldj{sfx}_f64'], rtol=1e-9, atol=1e-9)
    if direction == 'inverse':
        assert all(layer.last_inverse_route == 'per_degree' for layer in flow)       # no float64 blocked inverse for it
    loss = BoltzmannKLDivLoss()((c * y ** 2 + d * y).sum(dim=1), ldj)
    loss.backward()
    np.testing.assert_allclose(float(loss.detach()), float(g[f'{name}/loss{sfx}_f64']), rtol=1e-9)
    errs = {'gx': max_err(x.grad, g[f'{name}/gx{sfx}_f64'])}
    for k, prm in flow.named_parameters():
        assert prm.grad is not None, k
        errs[k] = max_err(prm.grad, g[f'{name}/grad{sfx}_f64/{k}'])
    print(f'{name}{sfx} float64: largest gradient error {max(errs.values()):.3e}')
    assert all(e <= 1e-9 for e in errs.values()), errs          # grad_close of test_gpu_float64_flows.py


def test_blocked_inverse_equals_the_pass_per_degree_inverse():
    g = _golden()
    flow = build_flow('quat', g)
    y = torch.from_numpy(g['quat/x']).cuda()
    assert all(layer._blocked_ok() for layer in flow)
    with torch.no_grad():
        xb, lb = flow.inverse(y)
        assert all(layer.last_inverse_route == 'blocked' for layer in flow)
        for layer in flow:
            layer.blocked_inverse = False
        assert not any(layer._blocked_ok() for layer in flow)
        xp, lp = flow.inverse(y)
        assert all(layer.last_inverse_route == 'per_degree' for layer in flow)
    assert rel(xb, xp) <= 1e-5 and bool((lb == 0).all()) and bool((lp == 0).all())
    assert rel(xb, g['quat/y_inv_f64']) <= 1e-5 and rel(xp, g['quat/y_inv_f64']) <= 1e-5
    # a flow of these layers round-trips
    with torch.no_grad():
        for layer in flow:
            layer.blocked_inverse = True
        x = torch.from_numpy(g['quat/x']).cuda()
        xr, _ = flow.inverse(flow(x)[0])
    assert rel(xr, x) <= 1e-5


@pytest.mark.parametrize('dt', DTYPES)
def test_quaternions_that_straddle_degrees_take_the_pass_per_degree(dt):
    """One degree per feature: the layer is not autoregressive per quaternion, so ``inverse`` is not the inverse map; what it
    returns is defined by the reference's algorithm (one conditioner pass per degree), and must match the golden."""
    g = _golden()
    flow = build_flow('straddle', g).to(dt)
    x = torch.from_numpy(g['straddle/x']).cuda().to(dt)
    assert not flow[0]._blocked_ok()
    with torch.no_grad():
        y, l = flow(x)
        xi, li = flow.inverse(x)
    assert flow[0].last_inverse_route == 'per_degree'
    assert bool((l == 0).all()) and bool((li == 0).all())
    for got, key in ((y, 'straddle/y_f64'), (xi, 'straddle/y_inv_f64')):
        print(f'{key} {dt}: rel L2 {rel(got, g[key]):.3e}')
        if dt == torch.float32:
            assert rel(got, g[key]) <= 1e-5
        else:
            np.testing.assert_allclose(_np(got), g[key], rtol=1e-9, atol=1e-10)
