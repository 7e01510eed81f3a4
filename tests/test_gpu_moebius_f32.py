"""GPU tests of the float32 Moebius kernels -- the default route of ``MoebiusTransformer``: ``moebius_kernel<float, DIM>``
(DIM = 2, 3 at compile time, the packed ``float2`` path of d = 2, DIM = 0 for any d), ``moebius_backward_kernel<float>`` and
the split-f16 side output of ``tfep_moebius_forward_split_out`` -- against the float64 restatement tests/moebius_ref.py
evaluated at the same float32 numbers (tests/moebius_cases.py; tests/test_moebius_cases_host.py holds the cases and the
restatements to their own conditions).  The float64 switch stays off.

Bounds, derived and none of them taken from what the kernels return.  The kernels compute in fp64 (the helpers of
``fp64_fast.h`` are good to about an fp64 ulp) and round once, on the store: half a float32 ulp, 2^-24 relative.  Four
times that is allowed:

* ``y``: relative L2 <= 2^-22 per tensor, and per element ``|y - ref| <= 2^-22 max(|ref_i|, 1e-6 max|ref vector|)``;
* log-det: ``|l - ref| <= 2^-22 max(1, |ref|)`` per sample; accumulated onto a start value: ``2^-22 max(1, |start + ref|)``;
* gradients: relative L2 <= 2^-22 per tensor; the parameter gradient of the identity map (dim = 1 off the sphere) is exactly
  zero, a relative error against it is undefined, and both sides hold round-off only -- each is held to the bound
  absolutely, in units of the cotangents' norm (as tests/test_gpu_moebius_f64.py);
* the split halves: bitwise those of the restatement; their sum within ``2^-22 |y| + 2^-39`` of ``y``
  (``moebius_cases.split_bound``);
* strided views, a row alone against the row in a batch, ``out=`` buffers, the contiguous fallback: ``torch.equal``;
* the round trip: see ``test_round_trip``.
"""
import pytest
import torch

import moebius_cases as mc

pytestmark = pytest.mark.gpu
F32 = torch.float32
BOUND = 2.0 ** -22


def transformer(c):
    from tfep_amd.nn.transformers import MoebiusTransformer
    tr = MoebiusTransformer(c['dim'], max_radius=c['max_radius'], unit_sphere=c['unit_sphere'])
    assert tr.float64_kernels is False
    return tr


def value_errors(y, l, y_ref, l_ref, dim):
    """(relative L2 of y, largest per-element error of y in units of ``max(|ref_i|, 1e-6 max|ref vector|)``, largest
    log-det error in units of ``max(1, |ref|)``)."""
    y, l = y.detach().cpu().double(), l.detach().cpu().double()
    B = y_ref.shape[0]
    floor = 1e-6 * y_ref.reshape(B, -1, dim).abs().amax(dim=-1, keepdim=True).expand(B, y_ref.shape[1] // dim, dim).reshape(B, -1)
    e_el = float(((y - y_ref).abs() / torch.maximum(y_ref.abs(), floor)).max()) if y.numel() else 0.0
    e_ld = float(((l - l_ref).abs() / l_ref.abs().clamp(min=1.0)).max()) if l.numel() else 0.0
    return mc.rel_l2(y, y_ref), e_el, e_ld


def check_values(what, y, l, y_ref, l_ref, dim):
    assert y.dtype == F32 and l.dtype == F32 and y.shape == y_ref.shape and l.shape == l_ref.shape
    e2, ee, el = value_errors(y, l, y_ref, l_ref, dim)
    print(f'{what}: y rel L2 {e2 / BOUND:.3f}, y per element {ee / BOUND:.3f}, log-det {el / BOUND:.3f} (units of 2^-22, bound 1)')
    assert e2 <= BOUND and ee <= BOUND and el <= BOUND, (what, e2, ee, el)


# ------------------------------------------------------------------ 1. forward and inverse

@pytest.mark.parametrize('name', mc.NAMES)
def test_forward_and_inverse_against_float64(name):
    from tfep_amd import ops
    c = mc.case(name)
    tr = transformer(c)
    x, w = c['x'].cuda(), c['w'].cuda()
    for key, fn, inverse in (('fwd', tr.forward, False), ('inv', tr.inverse, True)):
        y, l = fn(x, w)
        check_values(f'{name} {key}', y, l, c[key][0], c[key][1], c['dim'])
        yo, lo = ops.moebius(x, w, c['dim'], c['max_radius'], c['unit_sphere'], inverse=inverse)
        check_values(f'{name} {key} (ops.moebius)', yo, lo, c[key][0], c[key][1], c['dim'])
        assert torch.equal(yo, y) and torch.equal(lo, l)


@pytest.mark.parametrize('name', mc.NAMES)
def test_strided_and_misaligned_views_give_the_same_bits(name):
    """``x`` and ``w`` as column slices of wider tensors: row strides that differ from D and, at the odd offset, d = 2 rows
    off the 8-byte boundary (the scalar path of ``moebius_kernel<float, 2>``) -- the same bits as the contiguous call
    (d = 2: the packed ``float2`` path)."""
    c = mc.case(name)
    tr = transformer(c)
    x, w = c['x'].cuda(), c['w'].cuda()
    B, D = x.shape
    for fn in (tr.forward, tr.inverse):
        y, l = fn(x, w)
        for ox, ow in ((1, 2), (2, 1), (1, 1), (2, 4)):         # the last: even offsets and, with + 6, even row strides
            wide_x = torch.full((B, D + 6), 7.0, dtype=F32, device='cuda')
            wide_w = torch.full((B, D + 6 + (ox & 1)), -3.0, dtype=F32, device='cuda')
            wide_x[:, ox:ox + D], wide_w[:, ow:ow + D] = x, w
            ys, ls = fn(wide_x[:, ox:ox + D], wide_w[:, ow:ow + D])
            assert torch.equal(ys, y) and torch.equal(ls, l), (name, ox, ow)


@pytest.mark.parametrize('name', mc.RANDOM)
def test_accumulation_onto_a_log_det(name):
    from tfep_amd import ops
    c = mc.case(name)
    x, w = c['x'].cuda(), c['w'].cuda()
    start = torch.linspace(-2.0, 3.0, c['B'], dtype=F32, device='cuda')
    for key, inverse in (('fwd', False), ('inv', True)):
        acc = start.clone()
        y, l = ops.moebius(x, w, c['dim'], c['max_radius'], c['unit_sphere'], inverse=inverse, log_det_J=acc)
        assert l is acc
        y0, _ = ops.moebius(x, w, c['dim'], c['max_radius'], c['unit_sphere'], inverse=inverse)
        assert torch.equal(y, y0)
        want = start.cpu().double() + c[key][1]
        err = float(((acc.cpu().double() - want).abs() / want.abs().clamp(min=1.0)).max())
        print(f'{name} {key}: accumulated log-det {err / BOUND:.3f} (units of 2^-22, bound 1)')
        assert err <= BOUND, (name, key, err)


@pytest.mark.parametrize('unit_sphere', [0, 1])
@pytest.mark.parametrize('dim', mc.DIMS)
def test_a_row_alone_equals_the_row_in_a_batch(dim, unit_sphere):
    c = mc.case(f'r_d{dim}_u{unit_sphere}_b5_n65')
    tr = transformer(c)
    x, w = c['x'].cuda(), c['w'].cuda()
    for fn in (tr.forward, tr.inverse):
        yb, lb = fn(x, w)
        for r in (0, 3, 4):
            y1, l1 = fn(x[r:r + 1].clone(), w[r:r + 1].clone())
            assert torch.equal(y1[0], yb[r]) and torch.equal(l1[0], lb[r]), (dim, unit_sphere, r)


@pytest.mark.parametrize('dim', [2, 5])
def test_empty_batch(dim):
    from tfep_amd import ops
    from tfep_amd.nn.transformers import MoebiusTransformer
    tr = MoebiusTransformer(dim)
    z = torch.zeros(0, 3 * dim, dtype=F32, device='cuda')
    for y, l in (tr(z, z), tr.inverse(z, z), ops.moebius(z, z, dim, 0.99, False), ops.moebius(z, z, dim, 0.99, True, inverse=True)):
        assert y.shape == (0, 3 * dim) and l.shape == (0,) and y.dtype == F32 and l.dtype == F32 and y.is_cuda and l.is_cuda


@pytest.mark.parametrize('name', mc.NAMES)
def test_round_trip(name):
    """``inverse(forward(x))`` against ``x``.  The kernel's image ``y~`` is within 2^-22 |y| of the map's (relative L2, the
    bound above); the inverse kernel returns the inverse map of ``y~`` to within 2^-22 of ITS norm, which is |x| (the map
    keeps the norm of every vector); and the inverse map takes ``y~ - y`` to at most ``L |y~ - y|``, ``L`` its Lipschitz
    factor.  The Jacobian of either direction is ``c R`` on the tangent space of the sphere through x (``R`` a reflection,
    ``c = (|x|^2 - |u|^2) / |x - u|^2``) and the identity along x, so its singular values are c and 1, and with
    ``|u| <= max_radius |x|``: ``1 / L <= c <= L = (1 + max_radius) / (1 - max_radius)``.  Together, with |y| = |x|:
    relative L2 <= 2^-22 (1 + L) -- 4.8e-5 at max_radius = 0.99."""
    c = mc.case(name)
    tr = transformer(c)
    x, w = c['x'].cuda(), c['w'].cuda()
    lipschitz = (1.0 + c['max_radius']) / (1.0 - c['max_radius'])
    for there, back in ((tr.forward, tr.inverse), (tr.inverse, tr.forward)):
        y, l = there(x, w)
        x1, l1 = back(y, w)
        err = mc.rel_l2(x1, x)
        print(f'{name}: round trip {err:.3e} (bound {BOUND * (1 + lipschitz):.3e})')
        assert err <= BOUND * (1.0 + lipschitz), (name, err)


# ------------------------------------------------------------------ 2. the VJP

def kernel_grads(c, key):
    import tfep_amd.torch_ops  # noqa: F401
    op = torch.ops.tfep.moebius_forward if key == 'fwd' else torch.ops.tfep.moebius_inverse
    x, w = c['x'].cuda().requires_grad_(True), c['w'].cuda().requires_grad_(True)
    y, l = op(x, w, c['dim'], c['max_radius'], c['unit_sphere'])
    ((y * c['gy'].cuda()).sum() + (l * c['gl'].cuda()).sum()).backward()
    assert x.grad.dtype == F32 and w.grad.dtype == F32
    return x.grad, w.grad


#: (the cases of ``moebius_cases.GRAD_DROPPED`` -- none -- would be left out here: the reference's own gradient is not
#: stable enough there to judge 2^-22; tests/test_moebius_cases_host.py measures it)
@pytest.mark.parametrize('name', [n for n in mc.NAMES if n not in mc.GRAD_DROPPED])
def test_vjp_against_autograd_through_the_restatement(name):
    c = mc.case(name)
    for key in ('fwd', 'inv'):
        gx, gw = kernel_grads(c, key)
        assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gw).all())
        ex, ew = mc.grad_errors(c, key, gx, gw)
        print(f'{name} {key}: grad x {ex / BOUND:.3f}, grad w {ew / BOUND:.3f} (units of 2^-22, bound 1)')
        assert ex <= BOUND and ew <= BOUND, (name, key, ex, ew)


@pytest.mark.parametrize('name', [n for n in mc.EDGE if 'wzero' in n])
def test_w_zero_has_the_zero_subgradient_of_the_norm(name):
    """The vectors with ``w = 0`` alone: finite gradients, those of the reference (whose ``|w|`` has the zero sub-gradient)."""
    c = mc.case(name)
    dim = c['dim']
    zero = (c['w'].reshape(c['B'], -1, dim) == 0).all(dim=-1)
    assert int(zero.sum()) == c['nvec'] + 1                     # the whole of row 1 and the first vector of row 2
    for key in ('fwd', 'inv'):
        gx, gw = (g.cpu().reshape(c['B'], -1, dim)[zero] for g in kernel_grads(c, key))
        rx, rw = (g.reshape(c['B'], -1, dim)[zero] for g in c[key][2:])
        assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gw).all())
        assert float(rw.abs().max()) > 0
        ex, ew = mc.rel_l2(gx, rx), mc.rel_l2(gw, rw)
        print(f'{name} {key}, vectors with w = 0: grad x {ex / BOUND:.3f}, grad w {ew / BOUND:.3f} (units of 2^-22, bound 1)')
        assert ex <= BOUND and ew <= BOUND, (name, key, ex, ew)


VJP_CASES = ['r_d2_u1_b5_n65', 'r_d3_u0_b5_n65', 'r_d5_u0_b5_n65', 'r_d1_u1_b5_n1']


def _backward(c, x, w, gy, gl, **kw):
    from tfep_amd import ops
    return ops.moebius_backward(x, w, c['dim'], c['max_radius'], c['unit_sphere'], gy, gl, **kw)


@pytest.mark.parametrize('name', VJP_CASES)
def test_backward_arguments(name):
    """``ops.moebius_backward`` itself: an absent log-det cotangent, ``out=`` buffers with row strides of their own, and the
    op's values against the reference."""
    c = mc.case(name)
    x, w, gy, gl = (c[k].cuda() for k in ('x', 'w', 'gy', 'gl'))
    B, D = x.shape
    gx, gw = _backward(c, x, w, gy, gl)
    ex, ew = mc.grad_errors(c, 'fwd', gx, gw)
    assert ex <= BOUND and ew <= BOUND, (name, ex, ew)
    # no cotangent of the log-det is a cotangent of zeros
    gx0, gw0 = _backward(c, x, w, gy, None)
    gxz, gwz = _backward(c, x, w, gy, torch.zeros_like(gl))
    assert torch.equal(gx0, gxz) and torch.equal(gw0, gwz)
    assert not torch.equal(gx0, gx)
    # out= column slices of wider tensors: the same bits inside, the sentinel outside
    for ox, ow in ((1, 2), (2, 1)):
        wide_gx = torch.full((B, D + 3), 7.0, dtype=F32, device='cuda')
        wide_gw = torch.full((B, D + 5), -3.0, dtype=F32, device='cuda')
        ox_, ow_ = _backward(c, x, w, gy, gl, out=(wide_gx[:, ox:ox + D], wide_gw[:, ow:ow + D]))
        assert ox_.data_ptr() == wide_gx[:, ox:ox + D].data_ptr() and ow_.data_ptr() == wide_gw[:, ow:ow + D].data_ptr()
        assert torch.equal(wide_gx[:, ox:ox + D], gx) and torch.equal(wide_gw[:, ow:ow + D], gw)
        assert bool((wide_gx[:, :ox] == 7.0).all()) and bool((wide_gx[:, ox + D:] == 7.0).all())
        assert bool((wide_gw[:, :ow] == -3.0).all()) and bool((wide_gw[:, ow + D:] == -3.0).all())
    # strided inputs and cotangents
    wide = [torch.zeros(B, D + 2 + k, dtype=F32, device='cuda') for k in range(3)]
    for t, src in zip(wide, (x, w, gy)):
        t[:, 1:D + 1] = src
    gxs, gws = _backward(c, *[t[:, 1:D + 1] for t in wide], gl)
    assert torch.equal(gxs, gx) and torch.equal(gws, gw)


@pytest.mark.parametrize('name', VJP_CASES)
def test_backward_sign_argument_is_the_vjp_of_the_inverse(name):
    """``sign = -1`` of ``tfep_moebius_backward`` (the VJP of the inverse: the map on negated parameters, the gradient
    negated back) against the route the autograd op takes -- the forward VJP at ``-w``, negated on the host: the same
    bits, and the reference's inverse gradients to the bound."""
    from tfep_amd import ops
    c = mc.case(name)
    x, w, gy, gl = (c[k].cuda() for k in ('x', 'w', 'gy', 'gl'))
    B, D = x.shape
    gx, gw = torch.empty_like(x), torch.empty_like(w)
    ops.call('tfep_moebius_backward', ops.ptr(x), D, ops.ptr(w), D, c['dim'], c['max_radius'], int(c['unit_sphere']), -1,
             ops.ptr(gy), D, ops.ptr(gl), ops.ptr(gw), D, ops.ptr(gx), D, B, D, ops.stream_of(x))
    hx, hw = _backward(c, x, -w, gy, gl)
    assert torch.equal(gx, hx) and torch.equal(gw, -hw)
    ex, ew = mc.grad_errors(c, 'inv', gx, gw)
    assert ex <= BOUND and ew <= BOUND, (name, ex, ew)


@pytest.mark.parametrize('unit_sphere', [0, 1])
@pytest.mark.parametrize('dim', [1, 2, 3, 8])
def test_vjp_of_a_row_alone_equals_the_row_in_a_batch(dim, unit_sphere):
    c = mc.case(f'r_d{dim}_u{unit_sphere}_b5_n65')
    x, w, gy, gl = (c[k].cuda() for k in ('x', 'w', 'gy', 'gl'))
    gx, gw = _backward(c, x, w, gy, gl)
    for r in (0, 3, 4):
        gx1, gw1 = _backward(c, *[t[r:r + 1].clone() for t in (x, w, gy, gl)])
        assert torch.equal(gx1[0], gx[r]) and torch.equal(gw1[0], gw[r]), (dim, unit_sphere, r)


# ------------------------------------------------------------------ 3. the split-f16 side output

def split_inputs(B, nvec):
    gen = torch.Generator().manual_seed(100 * B + nvec)
    x = torch.randn(B, nvec, 2, dtype=torch.float64, generator=gen)
    x = (x / x.norm(dim=-1, keepdim=True)).reshape(B, 2 * nvec).float()
    return x.cuda(), torch.randn(B, 2 * nvec, generator=gen).cuda()


@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('nvec', [4, 68, 132])          # D = 8, 136, 264: groups on a lane's first, second and third pass
def test_split_out(nvec, B, padded):
    from tfep_amd import ops
    D = 2 * nvec
    cols = (-(-D // 32) * 32 + 32) if padded else D
    x, w = split_inputs(B, nvec)
    y, l, ys, ys_inv = ops.moebius_split_out(x, w, 0.99, cols)
    y0, l0 = ops.moebius(x, w, 2, 0.99, True)
    assert torch.equal(y, y0) and torch.equal(l, l0)
    assert ys.shape == (B, cols) and ys.dtype == F32 and ys_inv.dtype == F32
    assert bool((ys_inv[:B] == 2.0 ** -14).all())
    hi, lo, padding = mc.split_decode(ys, D)
    hi_ref, lo_ref = mc.split_halves(y)
    assert torch.equal(hi.view(torch.int16), hi_ref.view(torch.int16))
    assert torch.equal(lo.view(torch.int16), lo_ref.view(torch.int16))
    assert float(lo.float().abs().max()) > 0
    err = (mc.split_reconstruct(hi, lo) - y.double()).abs()
    assert bool((err <= mc.split_bound(y)).all()), float((err / mc.split_bound(y)).max())
    assert padding.shape == (B, cols - D) and bool((padding.view(torch.int32) == 0).all())
    # misaligned inputs (an odd column offset, odd row strides): the wrapper's contiguous copies, the same bits
    wide_x, wide_w = torch.zeros(B, D + 3, dtype=F32, device='cuda'), torch.zeros(B, D + 5, dtype=F32, device='cuda')
    wide_x[:, 1:D + 1], wide_w[:, 3:D + 3] = x, w
    for out, want in zip(ops.moebius_split_out(wide_x[:, 1:D + 1], wide_w[:, 3:D + 3], 0.99, cols), (y, l, ys, ys_inv)):
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    # aligned views with even row strides: no copy, the same bits
    wide_x, wide_w = torch.zeros(B, D + 4, dtype=F32, device='cuda'), torch.zeros(B, D + 6, dtype=F32, device='cuda')
    wide_x[:, 2:D + 2], wide_w[:, 4:D + 4] = x, w
    for out, want in zip(ops.moebius_split_out(wide_x[:, 2:D + 2], wide_w[:, 4:D + 4], 0.99, cols), (y, l, ys, ys_inv)):
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))


def test_split_out_refuses_partial_groups_and_short_rows():
    from tfep_amd import ops
    x, w = split_inputs(2, 8)
    with pytest.raises(ValueError, match='moebius_split_out: n_features=12 must be a multiple of 8'):
        ops.moebius_split_out(x[:, :12].contiguous(), w[:, :12].contiguous(), 0.99, 32)
    with pytest.raises(ValueError, match='moebius_split_out: split rows too short'):
        ops.moebius_split_out(x, w, 0.99, 8)                    # cols_padded = 8 < D = 16
