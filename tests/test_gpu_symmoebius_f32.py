"""GPU tests of the float32 symmetrized Moebius kernels -- ``symmoebius_kernel<float, DIM, INVERSE>`` (DIM = 2, 3, 4 at compile
time, the packed 8- and 16-byte paths of d = 2 and d = 4, DIM = 0 for any d) and ``symmoebius_backward_kernel<float, DIM,
INVERSE>`` -- against the float64 restatement tests/symmoebius_ref.py of the reference's formulae, evaluated at the same
float32 numbers (tests/symmoebius_cases.py; tests/test_symmoebius_cases_host.py holds the cases and the restatement to their
own conditions, and the kernels' closed form to the restatement).

Bounds, derived and none of them taken from what the kernels return.  The kernels compute in fp64 (the helpers of
``fp64_fast.h`` are good to about an fp64 ulp) and round once, on the store: half a float32 ulp, 2^-24 relative.  Four
times that is allowed:

* ``y``: relative L2 <= 2^-22 per tensor, and per element ``|y - ref| <= 2^-22 max(|ref_i|, 1e-6 max|ref vector|)``;
* log-det: ``|l - ref| <= 2^-22 max(1, |ref|)`` per row; accumulated onto a start value: ``2^-22 max(1, |start + ref|)``;
* gradients: relative L2 <= 2^-22 per tensor, against autograd through the restatement and, at the vectors where the
  reference's inverse is 0 / 0, the inverse-function theorem on its forward map; at vectors with ``w = 0`` the parameter
  gradient is exactly zero in the reference, a relative error against it is undefined, and both sides hold round-off
  only -- each is held to the bound absolutely, in units of the cotangents' norm
  (``symmoebius_cases.wzero_gradient_error``);
* strided and misaligned views, a row alone against the row in a batch, ``out=`` buffers, the two routes: ``torch.equal``;
* the round trip: see ``test_round_trip``.
"""
import pytest
import torch

import symmoebius_cases as sc

pytestmark = pytest.mark.gpu
F32 = torch.float32
BOUND = 2.0 ** -22


def transformer(c):
    from tfep_amd.nn.transformers import SymmetrizedMoebiusTransformer
    return SymmetrizedMoebiusTransformer(c['dim'], max_radius=c['max_radius'])


def sym(c, x, w, inverse, **kw):
    from tfep_amd import ops
    return ops.symmetrized_moebius(x, w, c['dim'], c['max_radius'], inverse=inverse, **kw)


def backward(c, x, w, gy, gl, inverse, **kw):
    from tfep_amd import ops
    return ops.symmetrized_moebius_backward(x, w, c['dim'], c['max_radius'], inverse, gy, gl, **kw)


def value_errors(y, l, y_ref, l_ref, dim):
    """(relative L2 of y, largest per-element error of y in units of ``max(|ref_i|, 1e-6 max|ref vector|)``, largest
    log-det error in units of ``max(1, |ref|)``)."""
    y, l = y.detach().cpu().double(), l.detach().cpu().double()
    B = y_ref.shape[0]
    floor = 1e-6 * y_ref.reshape(B, -1, dim).abs().amax(dim=-1, keepdim=True).expand(B, y_ref.shape[1] // dim, dim).reshape(B, -1)
    e_el = float(((y - y_ref).abs() / torch.maximum(y_ref.abs(), floor)).max()) if y.numel() else 0.0
    e_ld = float(((l - l_ref).abs() / l_ref.abs().clamp(min=1.0)).max()) if l.numel() else 0.0
    return sc.rel_l2(y, y_ref), e_el, e_ld


def check_values(what, y, l, y_ref, l_ref, dim):
    assert y.dtype == F32 and l.dtype == F32 and y.shape == y_ref.shape and l.shape == l_ref.shape
    e2, ee, el = value_errors(y, l, y_ref, l_ref, dim)
    print(f'{what}: y rel L2 {e2 / BOUND:.3f}, y per element {ee / BOUND:.3f}, log-det {el / BOUND:.3f} (units of 2^-22, bound 1)')
    assert e2 <= BOUND and ee <= BOUND and el <= BOUND, (what, e2, ee, el)


def column_slice(t, offset, stride, fill):
    """``(wide, view)``: ``t`` as the columns ``offset ...`` of a ``(B, stride)`` tensor of ``fill``."""
    B, D = t.shape
    wide = torch.full((B, stride), fill, dtype=t.dtype, device=t.device)
    wide[:, offset:offset + D] = t
    return wide, wide[:, offset:offset + D]


def untouched(wide, offset, D, fill):
    return bool((wide[:, :offset] == fill).all()) and bool((wide[:, offset + D:] == fill).all())


# ------------------------------------------------------------------ 1. forward and inverse

@pytest.mark.parametrize('name', sc.NAMES)
def test_forward_and_inverse_against_float64(name):
    c = sc.case(name)
    tr = transformer(c)
    x, w = c['x'].cuda(), c['w'].cuda()
    for key, fn, inverse in (('fwd', tr.forward, False), ('inv', tr.inverse, True)):
        y, l = fn(x, w)
        check_values(f'{name} {key}', y, l, c[key][0], c[key][1], c['dim'])
        yo, lo = sym(c, x, w, inverse)
        assert torch.equal(yo, y) and torch.equal(lo, l)


@pytest.mark.parametrize('name', sc.RANDOM)
def test_accumulation_onto_a_log_det(name):
    c = sc.case(name)
    x, w = c['x'].cuda(), c['w'].cuda()
    start = torch.linspace(-2.0, 3.0, c['B'], dtype=F32, device='cuda')
    for key, inverse in (('fwd', False), ('inv', True)):
        acc = start.clone()
        y, l = sym(c, x, w, inverse, log_det_J=acc)
        assert l is acc
        y0, _ = sym(c, x, w, inverse)
        assert torch.equal(y, y0)
        want = start.cpu().double() + c[key][1]
        err = float(((acc.cpu().double() - want).abs() / want.abs().clamp(min=1.0)).max())
        print(f'{name} {key}: accumulated log-det {err / BOUND:.3f} (units of 2^-22, bound 1)')
        assert err <= BOUND, (name, key, err)


@pytest.mark.parametrize('dim', sc.DIMS)
def test_a_row_alone_equals_the_row_in_a_batch(dim):
    c = sc.case(f'r_d{dim}_b5_n65')
    x, w, gy, gl = (c[k].cuda() for k in ('x', 'w', 'gy', 'gl'))
    for inverse in (False, True):
        yb, lb = sym(c, x, w, inverse)
        gxb, gwb = backward(c, x, w, gy, gl, inverse)
        for r in (0, 3, 4):
            xr, wr, gyr, glr = (t[r:r + 1].clone() for t in (x, w, gy, gl))
            y1, l1 = sym(c, xr, wr, inverse)
            assert torch.equal(y1[0], yb[r]) and torch.equal(l1[0], lb[r]), (dim, inverse, r)
            gx1, gw1 = backward(c, xr, wr, gyr, glr, inverse)
            assert torch.equal(gx1[0], gxb[r]) and torch.equal(gw1[0], gwb[r]), (dim, inverse, r)


@pytest.mark.parametrize('dim', [2, 5])
def test_empty_batch(dim):
    from tfep_amd import ops
    from tfep_amd.nn.transformers import SymmetrizedMoebiusTransformer
    tr = SymmetrizedMoebiusTransformer(dim)
    z, zl = torch.zeros(0, 3 * dim, dtype=F32, device='cuda'), torch.zeros(0, dtype=F32, device='cuda')
    for y, l in (tr(z, z), tr.inverse(z, z), ops.symmetrized_moebius(z, z, dim, 0.99),
                 ops.symmetrized_moebius(z, z, dim, 0.99, inverse=True)):
        assert y.shape == (0, 3 * dim) and l.shape == (0,) and y.dtype == F32 and l.dtype == F32 and y.is_cuda and l.is_cuda
    for inverse in (False, True):
        for gl in (zl, None):
            gx, gw = ops.symmetrized_moebius_backward(z, z, dim, 0.99, inverse, z, gl)
            assert gx.shape == gw.shape == (0, 3 * dim) and gx.dtype == F32 and gw.dtype == F32 and gx.is_cuda and gw.is_cuda


@pytest.mark.parametrize('name', sc.NAMES)
def test_round_trip(name):
    """``inverse(forward(x))`` against ``x``, and the other way round.  The first kernel's image ``y~`` is within 2^-22 |y| of
    the map's (relative L2, the bound above); the second kernel returns the image of ``y~`` under its map to within 2^-22 of
    ITS norm, which is |x| (either map keeps the norm of every vector); and that map takes ``y~ - y`` to at most
    ``L |y~ - y|``, ``L`` its Lipschitz factor.  With ``theta`` the angle of ``x`` to ``w`` the forward map keeps the plane of
    the two and turns ``tan theta`` into ``(1 + r2) / (1 - r2) tan theta``: its Jacobian has the singular values 1 (along x),
    ``(1 - r2) (1 + r2) / H`` (in the plane, along the sphere) and ``(1 + r2) / sqrt(H)`` (d - 2 times, across the plane) --
    their product is the log-det of ``symmoebius.h`` -- and the inverse's are the same with ``1 + r2`` and ``1 - r2`` swapped.
    ``(1 - r2)^2 <= H <= (1 + r2)^2`` and ``r2 <= max_radius^2``, so all of them lie in ``[1 / L, L]`` with
    ``L = (1 + max_radius^2) / (1 - max_radius^2)``.  Together, with |y| = |x|: relative L2 <= 2^-22 (1 + L) -- 2.4e-5 at
    max_radius = 0.99."""
    c = sc.case(name)
    tr = transformer(c)
    x, w = c['x'].cuda(), c['w'].cuda()
    lipschitz = (1.0 + c['max_radius'] ** 2) / (1.0 - c['max_radius'] ** 2)
    for there, back in ((tr.forward, tr.inverse), (tr.inverse, tr.forward)):
        y, l = there(x, w)
        x1, l1 = back(y, w)
        err = sc.rel_l2(x1, x)
        print(f'{name}: round trip {err / BOUND:.3f} x 2^-22 (bound {1 + lipschitz:.1f} x 2^-22)')
        assert err <= BOUND * (1.0 + lipschitz), (name, err)


@pytest.mark.parametrize('dim', sc.DIMS)
def test_a_zero_vector_is_nan_and_stays_local(dim):
    """``x = 0`` is 0 / 0 in the reference; here too: NaN in that vector and in the row's log-det, every other vector of the
    row and every other row bit for bit those of the run without it (no equality is tested at that point)."""
    c = sc.case(f'r_d{dim}_b5_n65')
    x, w = c['x'].cuda(), c['w'].cuda()
    x0 = x.clone()
    x0[2, 3 * dim:4 * dim] = 0.0
    keep = torch.ones_like(x, dtype=torch.bool)
    keep[2, 3 * dim:4 * dim] = False
    rows = torch.tensor([0, 1, 3, 4], device='cuda')
    for inverse in (False, True):
        y, l = sym(c, x, w, inverse)
        y0, l0 = sym(c, x0, w, inverse)
        assert bool(torch.isnan(y0[2, 3 * dim:4 * dim]).all()) and bool(torch.isnan(l0[2]))
        assert torch.equal(y0[keep], y[keep]) and torch.equal(l0[rows], l[rows])


# ------------------------------------------------------------------ 2. the VJP

def kernel_grads(c, key, with_gl=True):
    import tfep_amd.torch_ops  # noqa: F401
    op = torch.ops.tfep.symmetrized_moebius_forward if key == 'fwd' else torch.ops.tfep.symmetrized_moebius_inverse
    x, w = c['x'].cuda().requires_grad_(True), c['w'].cuda().requires_grad_(True)
    y, l = op(x, w, c['dim'], c['max_radius'])
    loss = (y * c['gy'].cuda()).sum()
    if with_gl:
        loss = loss + (l * c['gl'].cuda()).sum()
    loss.backward()
    assert x.grad.dtype == F32 and w.grad.dtype == F32
    return x.grad, w.grad


#: (the cases of ``symmoebius_cases.GRAD_DROPPED`` -- none -- would be left out here: the reference's own gradient is not
#: stable enough there to judge 2^-22; tests/test_symmoebius_cases_host.py measures it)
@pytest.mark.parametrize('name', [n for n in sc.NAMES if n not in sc.GRAD_DROPPED])
def test_vjp_against_the_reference_gradients(name):
    """Through the autograd registrations of ``tfep::symmetrized_moebius_forward`` / ``_inverse`` and through
    ``ops.symmetrized_moebius_backward`` itself (the same bits); an absent log-det cotangent is a cotangent of zeros."""
    c = sc.case(name)
    x, w, gy, gl = (c[k].cuda() for k in ('x', 'w', 'gy', 'gl'))
    for key, inverse in (('fwd', False), ('inv', True)):
        gx, gw = kernel_grads(c, key)
        assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gw).all())
        ex, ew, ez = sc.grad_errors(c, key, gx, gw)
        print(f'{name} {key}: grad x {ex / BOUND:.3f}, grad w {ew / BOUND:.3f}, grad w at w = 0 {ez / BOUND:.3f} '
              f'(units of 2^-22, bound 1)')
        assert ex <= BOUND and ew <= BOUND and ez <= BOUND, (name, key, ex, ew, ez)
        ox, ow = backward(c, x, w, gy, gl, inverse)
        assert torch.equal(ox, gx) and torch.equal(ow, gw)
        gx0, gw0 = backward(c, x, w, gy, None, inverse)
        gxz, gwz = backward(c, x, w, gy, torch.zeros_like(gl), inverse)
        assert torch.equal(gx0, gxz) and torch.equal(gw0, gwz) and not torch.equal(gw0, gw)
        ax, aw = kernel_grads(c, key, with_gl=False)
        assert torch.equal(ax, gx0) and torch.equal(aw, gw0)


@pytest.mark.parametrize('dim', sc.EDGE_DIMS)
def test_w_zero_has_the_zero_subgradient_of_the_norm(dim):
    """The vectors with ``w = 0`` alone (the ``wn > 0`` branch of ``symmoebius_vjp_vector``): finite gradients, the point's
    those of the reference, the parameter's zero like the reference's."""
    name = f'e_wzero_d{dim}'
    c = sc.case(name)
    zero = c['wzero']
    assert int(zero.sum()) == c['nvec'] + 1                     # the whole of row 1 and the first vector of row 2
    for key in ('fwd', 'inv'):
        gx, gw = (g.cpu().reshape(c['B'], -1, dim)[zero] for g in kernel_grads(c, key))
        rx, rw = (g.reshape(c['B'], -1, dim)[zero] for g in c[key][2:])
        assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gw).all())
        ex = sc.rel_l2(gx, rx)
        ew = max(float(gw.double().norm()), float(rw.norm())) / sc.cotangent_norm(c)
        print(f'{name} {key}, vectors with w = 0: grad x {ex / BOUND:.3f}, |grad w| / |cotangents| {ew / BOUND:.3f} '
              f'(units of 2^-22, bound 1)')
        assert ex <= BOUND and ew <= BOUND, (name, key, ex, ew)


# ------------------------------------------------------------------ 3. alignment tiers

def _offsets(dim):
    """d = 2 and d = 4 pack a vector into one 8- or 16-byte access when the x, w and y rows are aligned; d = 3 and d = 5
    take the scalar path always: one offset suffices there."""
    return (0, 1, 2, 3) if dim in (2, 4) else (1,)


@pytest.mark.parametrize('dim', [2, 3, 4, 5])
def test_strided_and_misaligned_inputs_give_the_same_bits(dim):
    """``x`` and ``w`` as column slices of wider tensors at float offsets 0 .. 3, each alone and both together, with row strides
    of D + 4 (rows keep the alignment of the first), D + 5 (odd: with B = 5 rows of one launch alternate between the packed
    and the scalar path) and D + 6 (d = 4: every other row off the 16-byte boundary): the bits of the contiguous call."""
    c = sc.case(f'r_d{dim}_b5_n65')
    x, w = c['x'].cuda(), c['w'].cuda()
    D = x.shape[1]
    for inverse in (False, True):
        y, l = sym(c, x, w, inverse)
        for which in ('x', 'w', 'xw'):
            for off in _offsets(dim):
                for extra in (4, 5, 6):
                    xs = column_slice(x, off, D + extra, 7.0)[1] if 'x' in which else x
                    ws = column_slice(w, off, D + extra + (1 if which == 'xw' else 0), -3.0)[1] if 'w' in which else w
                    ys, ls = sym(c, xs, ws, inverse)
                    assert torch.equal(ys, y) and torch.equal(ls, l), (dim, inverse, which, off, extra)


@pytest.mark.parametrize('dim', [2, 3, 4, 5])
def test_a_misaligned_output_gives_the_same_bits(dim):
    """``tfep_symmetrized_moebius`` writing ``y`` into a column slice (the only way to a ``y`` row off the vector boundary: the
    ``yr`` term of ``packed``), inputs contiguous: the same bits inside, the sentinel outside."""
    from tfep_amd import ops
    c = sc.case(f'r_d{dim}_b5_n65')
    x, w = c['x'].cuda(), c['w'].cuda()
    B, D = x.shape
    for inverse in (False, True):
        y, l = sym(c, x, w, inverse)
        for off in _offsets(dim):
            for extra in (4, 5, 6):
                wide, ys = column_slice(torch.zeros_like(y), off, D + extra, 7.0)
                ls = torch.full((B,), 9.0, dtype=F32, device='cuda')
                ops.call('tfep_symmetrized_moebius', ops.ptr(x), D, ops.ptr(w), D, dim, c['max_radius'], int(inverse),
                         ops.ptr(ys), D + extra, ops.ptr(ls), 0, B, D, ops.stream_of(x))
                assert torch.equal(ys, y) and torch.equal(ls, l), (dim, inverse, off, extra)
                assert untouched(wide, off, D, 7.0), (dim, inverse, off, extra)


@pytest.mark.parametrize('dim', [2, 3, 4, 5])
def test_vjp_on_strided_and_misaligned_operands_gives_the_same_bits(dim):
    """``x``, ``w`` and ``gy`` as column slices, each alone and all together, and ``out=`` slices for ``gx`` and ``gparams``, each
    alone: the bits of the contiguous call, the sentinels around the outputs unchanged."""
    c = sc.case(f'r_d{dim}_b5_n65')
    x, w, gy, gl = (c[k].cuda() for k in ('x', 'w', 'gy', 'gl'))
    B, D = x.shape
    for inverse in (False, True):
        gx, gw = backward(c, x, w, gy, gl, inverse)
        for which in ('x', 'w', 'g', 'xwg'):
            for off in _offsets(dim):
                for extra in (4, 5):
                    xs = column_slice(x, off, D + extra, 7.0)[1] if 'x' in which else x
                    ws = column_slice(w, off, D + extra + 2, -3.0)[1] if 'w' in which else w
                    gs = column_slice(gy, off, D + extra + 1, 5.0)[1] if 'g' in which else gy
                    sx, sw = backward(c, xs, ws, gs, gl, inverse)
                    assert torch.equal(sx, gx) and torch.equal(sw, gw), (dim, inverse, which, off, extra)
        for which in ('gx', 'gw'):
            for off in _offsets(dim):
                for extra in (4, 5):
                    # (the other output at offset 0 with a row stride of D + 4: every row of it aligned)
                    wide_x, out_x = column_slice(torch.zeros_like(x), off if which == 'gx' else 0, D + (extra if which == 'gx' else 4), 7.0)
                    wide_w, out_w = column_slice(torch.zeros_like(w), off if which == 'gw' else 0, D + (extra if which == 'gw' else 4), -3.0)
                    rx, rw = backward(c, x, w, gy, gl, inverse, out=(out_x, out_w))
                    assert rx.data_ptr() == out_x.data_ptr() and rw.data_ptr() == out_w.data_ptr()
                    assert torch.equal(out_x, gx) and torch.equal(out_w, gw), (dim, inverse, which, off, extra)
                    assert untouched(wide_x, off if which == 'gx' else 0, D, 7.0)
                    assert untouched(wide_w, off if which == 'gw' else 0, D, -3.0)
