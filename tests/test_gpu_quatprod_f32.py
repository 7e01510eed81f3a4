"""GPU tests of the float32 quaternion product kernels -- ``quatprod_kernel<float, INVERSE>`` (three alignment flags: x,
parameters, y) and ``quatprod_backward_kernel<float, INVERSE>`` (five: x, parameters, gy, gparams, gx) -- against the float64
restatement tests/quatprod_ref.py evaluated at the same float32 numbers (tests/quatprod_cases.py;
tests/test_quatprod_cases_host.py holds the cases and the restatement to their own conditions).

Bounds, derived and none of them taken from what the kernels return.  The kernels compute in fp64 (the helpers of
``fp64_fast.h`` are good to about an fp64 ulp) and round once, on the store: half a float32 ulp, 2^-24 relative.  Four
times that is allowed:

* ``y``: relative L2 <= 2^-22 per tensor, and per element ``|y - ref| <= 2^-22 max(|ref_i|, 1e-6 max|ref quaternion|)``;
* log-det: exactly 0.0; an accumulated ``log_det_J`` comes back bit for bit;
* gradients: relative L2 <= 2^-22 per tensor and per row (the rows of ``e_pscale`` differ by 1e10 in ``1 / |p|``: a tensor
  norm would hide the small one; every element is an fp64 value rounded once, so a row meets what the tensor meets);
* strided and misaligned views, a row alone against the row in a batch, ``out=`` buffers, the two routes, the identity,
  ``T(-x) = -T(x)``: ``torch.equal``;
* the round trip: the map is orthogonal (Lipschitz factor 1), so the two roundings add up: 2 x 2^-22.
"""
import pytest
import torch

import quatprod_cases as qc

pytestmark = pytest.mark.gpu
F32 = torch.float32
BOUND = 2.0 ** -22


def quat(x, p, inverse, **kw):
    from tfep_amd import ops
    return ops.quaternion_product(x, p, inverse=inverse, **kw)


def backward(x, p, gy, inverse, **kw):
    from tfep_amd import ops
    return ops.quaternion_product_backward(x, p, inverse, gy, **kw)


def check_values(what, y, l, y_ref):
    assert y.dtype == F32 and l.dtype == F32 and y.shape == y_ref.shape and l.shape == (y_ref.shape[0],)
    B = y_ref.shape[0]
    yd = y.detach().cpu().double()
    floor = 1e-6 * y_ref.reshape(B, -1, 4).abs().amax(dim=-1, keepdim=True).expand(B, y_ref.shape[1] // 4, 4).reshape(B, -1)
    e2 = qc.rel_l2(y, y_ref)
    ee = float(((yd - y_ref).abs() / torch.maximum(y_ref.abs(), floor)).max())
    print(f'{what}: y rel L2 {e2 / BOUND:.3f}, y per element {ee / BOUND:.3f} (units of 2^-22, bound 1)')
    assert e2 <= BOUND and ee <= BOUND, (what, e2, ee)
    assert bool((l == 0).all()) and not bool(torch.signbit(l).any())                # exactly 0.0


def row_rel_l2(got, ref):
    got, ref = got.detach().cpu().double(), ref.double()
    return float(((got - ref).norm(dim=1) / ref.norm(dim=1).clamp(min=1e-300)).max())


def column_slice(t, offset, stride, fill):
    """``(wide, view)``: ``t`` as the columns ``offset ...`` of a ``(B, stride)`` tensor of ``fill``."""
    B, D = t.shape
    wide = torch.full((B, stride), fill, dtype=t.dtype, device=t.device)
    wide[:, offset:offset + D] = t
    return wide, wide[:, offset:offset + D]


def untouched(wide, offset, D, fill):
    return bool((wide[:, :offset] == fill).all()) and bool((wide[:, offset + D:] == fill).all())


# ------------------------------------------------------------------ 1. forward and inverse

@pytest.mark.parametrize('name', qc.NAMES)
def test_forward_and_inverse_against_float64(name):
    from tfep_amd.nn.transformers import QuaternionProductTransformer
    c = qc.case(name)
    tr = QuaternionProductTransformer()
    x, p = c['x'].cuda(), c['p'].cuda()
    for key, fn, inverse in (('fwd', tr.forward, False), ('inv', tr.inverse, True)):
        y, l = fn(x, p)
        check_values(f'{name} {key}', y, l, c[key][0])
        yo, lo = quat(x, p, inverse)
        assert torch.equal(yo, y) and torch.equal(lo, l)
        acc = torch.linspace(-2.0, 3.0, c['B'], dtype=F32, device='cuda')
        start = acc.clone()
        ya, la = quat(x, p, inverse, log_det_J=acc)
        assert la is acc and torch.equal(acc, start) and torch.equal(ya, y)          # bit for bit


@pytest.mark.parametrize('name', qc.NAMES)
def test_round_trip(name):
    """``inverse(forward(x))`` against ``x`` and the other way round.  The first kernel's image is within 2^-22 |y| of the
    map's, the second returns the image of that to within 2^-22 of its norm, and the map between them is orthogonal: it
    carries the first error over unchanged.  |y| = |x|: relative L2 <= 2 x 2^-22."""
    c = qc.case(name)
    x, p = c['x'].cuda(), c['p'].cuda()
    for first in (False, True):
        y, _ = quat(x, p, first)
        x1, _ = quat(y, p, not first)
        err = qc.rel_l2(x1, x)
        print(f'{name}: round trip {err / BOUND:.3f} x 2^-22 (bound 2)')
        assert err <= 2 * BOUND, (name, err)


def test_scalar_parameters_are_the_identity_and_the_map_is_odd():
    """``p = (0, 0, 0, s)``: ``x`` bit for bit for s > 0 (``s / |s|`` is 1 to an fp64 ulp, and the product rounds back to the
    float32 it came from), ``-x`` for s < 0; and ``T(-x) = -T(x)`` bit for bit on every case."""
    c = qc.case('r_d4_b5_n65')
    x = c['x'].cuda()
    B, D = x.shape
    scales = torch.tensor([1.0, 2.5, 1e-6, 1e4, 0.75], dtype=F32, device='cuda')
    p = torch.zeros(B, D // 4, 4, dtype=F32, device='cuda')
    p[:, :, 3] = scales[:, None]
    p = p.reshape(B, D)
    for inverse in (False, True):
        y, l = quat(x, p, inverse)
        assert torch.equal(y, x) and bool((l == 0).all())
        y, l = quat(x, -p, inverse)
        assert torch.equal(y, -x)
    for name in qc.NAMES:
        c = qc.case(name)
        x, p = c['x'].cuda(), c['p'].cuda()
        for inverse in (False, True):
            assert torch.equal(quat(-x, p, inverse)[0], -quat(x, p, inverse)[0]), (name, inverse)


def test_a_zero_parameter_quaternion_is_nan_and_stays_local():
    """``p = 0`` is 0 / 0 in the reference; here too: NaN in that quaternion's four outputs and eight gradients, every other
    quaternion bit for bit that of the run without it, the log-det still exactly 0 (no equality is tested at that point)."""
    c = qc.case('r_d4_b5_n65')
    x, p, gy = c['x'].cuda(), c['p'].cuda(), c['gy'].cuda()
    p0 = p.clone()
    p0[2, 12:16] = 0.0
    keep = torch.ones_like(x, dtype=torch.bool)
    keep[2, 12:16] = False
    for inverse in (False, True):
        y, _ = quat(x, p, inverse)
        y0, l0 = quat(x, p0, inverse)
        assert bool(torch.isnan(y0[2, 12:16]).all()) and torch.equal(y0[keep], y[keep])
        assert bool((l0 == 0).all())
        gx, gp = backward(x, p, gy, inverse)
        gx0, gp0 = backward(x, p0, gy, inverse)
        assert bool(torch.isnan(gx0[2, 12:16]).all()) and bool(torch.isnan(gp0[2, 12:16]).all())
        assert torch.equal(gx0[keep], gx[keep]) and torch.equal(gp0[keep], gp[keep])


def test_a_row_alone_equals_the_row_in_a_batch():
    c = qc.case('r_d4_b5_n65')
    x, p, gy = c['x'].cuda(), c['p'].cuda(), c['gy'].cuda()
    for inverse in (False, True):
        yb, lb = quat(x, p, inverse)
        gxb, gpb = backward(x, p, gy, inverse)
        for r in (0, 3, 4):
            xr, pr, gr = (t[r:r + 1].clone() for t in (x, p, gy))
            y1, l1 = quat(xr, pr, inverse)
            assert torch.equal(y1[0], yb[r]) and torch.equal(l1[0], lb[r]), (inverse, r)
            gx1, gp1 = backward(xr, pr, gr, inverse)
            assert torch.equal(gx1[0], gxb[r]) and torch.equal(gp1[0], gpb[r]), (inverse, r)


def test_empty_batch():
    from tfep_amd.nn.transformers import QuaternionProductTransformer
    tr = QuaternionProductTransformer()
    z = torch.zeros(0, 12, dtype=F32, device='cuda')
    for y, l in (tr(z, z), tr.inverse(z, z), quat(z, z, False), quat(z, z, True)):
        assert y.shape == (0, 12) and l.shape == (0,) and y.dtype == F32 and l.dtype == F32 and y.is_cuda and l.is_cuda
    for inverse in (False, True):
        gx, gp = backward(z, z, z, inverse)
        assert gx.shape == gp.shape == (0, 12) and gx.dtype == F32 and gp.dtype == F32 and gx.is_cuda and gp.is_cuda


# ------------------------------------------------------------------ 2. the VJP

def kernel_grads(c, key, with_gl=True):
    import tfep_amd.torch_ops  # noqa: F401
    op = torch.ops.tfep.quaternion_product_forward if key == 'fwd' else torch.ops.tfep.quaternion_product_inverse
    x, p = c['x'].cuda().requires_grad_(True), c['p'].cuda().requires_grad_(True)
    y, l = op(x, p)
    loss = (y * c['gy'].cuda()).sum()
    if with_gl:
        loss = loss + 3.0 * l.sum()                             # (the log-det is constant: its cotangent adds nothing)
    loss.backward()
    assert x.grad.dtype == F32 and p.grad.dtype == F32
    return x.grad, p.grad


#: (the cases of ``quatprod_cases.GRAD_DROPPED`` -- none -- would be left out here; tests/test_quatprod_cases_host.py
#: measures the reference's stability)
@pytest.mark.parametrize('name', [n for n in qc.NAMES if n not in qc.GRAD_DROPPED])
def test_vjp_against_autograd_through_the_restatement(name):
    """Through the autograd registrations of ``tfep::quaternion_product_forward`` / ``_inverse`` and through
    ``ops.quaternion_product_backward`` itself: the same bits."""
    c = qc.case(name)
    x, p, gy = c['x'].cuda(), c['p'].cuda(), c['gy'].cuda()
    for key, inverse in (('fwd', False), ('inv', True)):
        gx, gp = kernel_grads(c, key)
        assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gp).all())
        ex, ep = qc.grad_errors(c, key, gx, gp)
        rx, rp = row_rel_l2(gx, c[key][1]), row_rel_l2(gp, c[key][2])
        print(f'{name} {key}: grad x {ex / BOUND:.3f} (worst row {rx / BOUND:.3f}), grad p {ep / BOUND:.3f} (worst row '
              f'{rp / BOUND:.3f}) (units of 2^-22, bound 1)')
        assert max(ex, ep, rx, rp) <= BOUND, (name, key, ex, ep, rx, rp)
        ox, op_ = backward(x, p, gy, inverse)
        assert torch.equal(ox, gx) and torch.equal(op_, gp)
        ax, ap = kernel_grads(c, key, with_gl=False)
        assert torch.equal(ax, gx) and torch.equal(ap, gp)


# ------------------------------------------------------------------ 3. alignment tiers

OFFSETS = (0, 1, 2, 3)
#: row strides of D + 4 (a multiple of 4: every row keeps the alignment of the first), D + 5 (odd: of B = 5 rows only every
#: fourth keeps it) and D + 6 (rows alternate between two alignments)
EXTRA = (4, 5, 6)


def test_strided_and_misaligned_inputs_give_the_same_bits():
    """``x`` and ``p`` as column slices of wider tensors at float offsets 0 .. 3, each alone (``px`` or ``pp`` false alone) and
    both together: the bits of the contiguous call."""
    c = qc.case('r_d4_b5_n65')
    x, p = c['x'].cuda(), c['p'].cuda()
    D = x.shape[1]
    for inverse in (False, True):
        y, l = quat(x, p, inverse)
        for which in ('x', 'p', 'xp'):
            for off in OFFSETS:
                for extra in EXTRA:
                    xs = column_slice(x, off, D + extra, 7.0)[1] if 'x' in which else x
                    ps = column_slice(p, off, D + extra + (1 if which == 'xp' else 0), -3.0)[1] if 'p' in which else p
                    ys, ls = quat(xs, ps, inverse)
                    assert torch.equal(ys, y) and torch.equal(ls, l), (inverse, which, off, extra)


def test_a_misaligned_output_gives_the_same_bits():
    """``tfep_quaternion_product`` writing ``y`` into a column slice (the only way to ``py == false``), inputs contiguous: the
    same bits inside, the sentinel outside; the log-det written is 0."""
    from tfep_amd import ops
    c = qc.case('r_d4_b5_n65')
    x, p = c['x'].cuda(), c['p'].cuda()
    B, D = x.shape
    for inverse in (False, True):
        y, _ = quat(x, p, inverse)
        for off in OFFSETS:
            for extra in EXTRA:
                wide, ys = column_slice(torch.zeros_like(y), off, D + extra, 7.0)
                ls = torch.full((B,), 9.0, dtype=F32, device='cuda')
                ops.call('tfep_quaternion_product', ops.ptr(x), D, ops.ptr(p), D, int(inverse), ops.ptr(ys), D + extra,
                         ops.ptr(ls), 0, B, D, ops.stream_of(x))
                assert torch.equal(ys, y) and bool((ls == 0).all()), (inverse, off, extra)
                assert untouched(wide, off, D, 7.0), (inverse, off, extra)


def test_vjp_on_strided_and_misaligned_operands_gives_the_same_bits():
    """The five alignment flags of ``quatprod_backward_kernel``: ``x``, ``p`` and ``gy`` as column slices, each alone and all
    together, and ``out=`` slices for ``gx`` and ``gparams``, each alone: the bits of the contiguous call, the sentinels
    around the outputs unchanged."""
    c = qc.case('r_d4_b5_n65')
    x, p, gy = c['x'].cuda(), c['p'].cuda(), c['gy'].cuda()
    B, D = x.shape
    for inverse in (False, True):
        gx, gp = backward(x, p, gy, inverse)
        for which in ('x', 'p', 'g', 'xpg'):
            for off in OFFSETS:
                for extra in EXTRA:
                    xs = column_slice(x, off, D + extra, 7.0)[1] if 'x' in which else x
                    ps = column_slice(p, off, D + extra + 2, -3.0)[1] if 'p' in which else p
                    gs = column_slice(gy, off, D + extra + 1, 5.0)[1] if 'g' in which else gy
                    sx, sp = backward(xs, ps, gs, inverse)
                    assert torch.equal(sx, gx) and torch.equal(sp, gp), (inverse, which, off, extra)
        for which in ('gx', 'gp'):
            for off in OFFSETS:
                for extra in EXTRA:
                    off_x, off_p = (off, 0) if which == 'gx' else (0, off)
                    # (the other output at offset 0 with a row stride of D + 4: every row of it aligned)
                    wide_x, out_x = column_slice(torch.zeros_like(x), off_x, D + (extra if which == 'gx' else 4), 7.0)
                    wide_p, out_p = column_slice(torch.zeros_like(p), off_p, D + (extra if which == 'gp' else 4), -3.0)
                    rx, rp = backward(x, p, gy, inverse, out=(out_x, out_p))
                    assert rx.data_ptr() == out_x.data_ptr() and rp.data_ptr() == out_p.data_ptr()
                    assert torch.equal(out_x, gx) and torch.equal(out_p, gp), (inverse, which, off, extra)
                    assert untouched(wide_x, off_x, D, 7.0) and untouched(wide_p, off_p, D, -3.0)
