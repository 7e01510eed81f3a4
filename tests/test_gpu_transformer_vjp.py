"""The six transformer VJP wrappers of ``tfep_amd.ops`` in the forms that ``transformer_vjp`` relies on and no other test
reaches: a parameter block inside a wider buffer, caller-allocated outputs, the feature-major ``layout``, no log-det
cotangent, and what they refuse before anything is launched.  The values themselves are held to the reference's
gradients by the tests of the custom ops; here the strided forms are compared with the plain contiguous call of
``torch.ops.tfep.X_backward``.

The comparisons are bitwise: none of the six kernels uses an atomic.  affine, SOS, Moebius, symmetrized Moebius and
quaternion product compute every output element in one lane from the element's own inputs; the two spline kernels
(float32 ``spline_backward_kernel``, float64 ``spline64_backward_kernel``) do the same per feature, and staging the
feature-major parameters through LDS moves values without changing them.  The strides only move where a value is
read and written."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, D = 70, 8                        # past one 64-row pass; four 2-vectors, two quaternions, eight scalar features
N_BINS, N_POLY = 4, 2
SENTINEL = -7777.0
F32, F64 = torch.float32, torch.float64

#: wrapper -> (parameters per feature, takes grad_log_det_J, takes layout, dtypes)
WRAPPERS = {'affine': (2, True, True, (F32, F64)),
            'sos': (2 * N_POLY + 1, False, True, (F32, F64)),
            'spline': (3 * N_BINS + 1, True, True, (F32, F64)),
            'moebius': (1, True, False, (F32,)),
            'symmetrized_moebius': (1, True, False, (F32, F64)),
            'quaternion_product': (1, False, False, (F32, F64))}
CASES = [(name, dt) for name, spec in WRAPPERS.items() for dt in spec[3]]
LAYOUT_CASES = [(name, dt) for name, dt in CASES if WRAPPERS[name][2]]
GL_CASES = [(name, dt) for name, dt in CASES if WRAPPERS[name][1]]


def _spline_args(dt):
    """A 4-bin spline whose four domain arrays differ from feature to feature."""
    f = torch.arange(D, device='cuda', dtype=dt)
    return (-2.0 - 0.1 * f, 3.0 + 0.2 * f, -1.0 - 0.3 * f, 2.0 + 0.05 * f, N_BINS, False, False, False, False, 1e-4, 1e-4)


def _inputs(name, dt, seed=0):
    """``(x, parameters, grad_y, grad_log_det_J)``, contiguous, drawn as the tests of the custom ops draw them."""
    g = torch.Generator(device='cuda').manual_seed(seed)

    def r(*shape):
        return torch.randn(*shape, device='cuda', dtype=dt, generator=g)
    x = r(B, D)
    if name == 'spline':                                          # inside the domain
        x0, xf = _spline_args(dt)[:2]
        x = x0 + (xf - x0) * (0.05 + 0.9 * torch.rand(B, D, device='cuda', dtype=dt, generator=g))
    elif name == 'moebius':                                       # on the unit sphere
        x = x / x.reshape(B, D // 2, 2).norm(dim=-1).repeat_interleave(2, dim=1)
    elif name == 'symmetrized_moebius':
        x = 2 * x
    return x, r(B, WRAPPERS[name][0] * D), r(B, D), r(B)


def _wrapper(name, dt, x, p, gy, gl, **kw):
    from tfep_amd import ops
    if name == 'affine':
        return ops.affine_backward(x, p, gy, gl, **kw)
    if name == 'sos':
        return ops.sos_backward(x, p, N_POLY, gy, **kw)
    if name == 'spline':
        return ops.spline_backward(x, p, ops.SplineConfig(*_spline_args(dt), dtype=dt), gy, gl, **kw)
    if name == 'moebius':
        return ops.moebius_backward(x, p, 2, 0.99, True, gy, gl, **kw)
    if name == 'symmetrized_moebius':
        return ops.symmetrized_moebius_backward(x, p, 2, 0.9, False, gy, gl, **kw)
    return ops.quaternion_product_backward(x, p, False, gy, **kw)


def _custom_op(name, dt, x, p, gy, gl):
    """The plain contiguous call of ``torch.ops.tfep.X_backward``."""
    import tfep_amd.torch_ops  # noqa: F401
    t = torch.ops.tfep
    if name == 'affine':
        return t.affine_backward(x, p, gy, gl)
    if name == 'sos':
        return t.sos_backward(x, p, N_POLY, gy)
    if name == 'spline':
        return t.spline_backward(x, p, gy, gl, *_spline_args(dt))
    if name == 'moebius':
        return t.moebius_backward(x, p, gy, gl, 2, 0.99, True)
    if name == 'symmetrized_moebius':
        return t.symmetrized_moebius_backward(x, p, gy, gl, 2, 0.9, False)
    return t.quaternion_product_backward(x, p, gy, False)


def _sentinels(*shape, dt):
    return torch.full(shape, SENTINEL, device='cuda', dtype=dt)


def _feature_major(t, P):
    """Reference layout (column p D + f) -> feature major (column f P + p)."""
    return t.reshape(B, P, D).transpose(1, 2).reshape(B, P * D)


@pytest.mark.parametrize('name,dt', CASES)
def test_parameter_block_inside_a_wider_buffer_and_caller_outputs(name, dt):
    x, p, gy, gl = _inputs(name, dt)
    n_par = p.shape[1]
    cols = slice(3, 3 + n_par)
    theta = torch.randn(B, n_par + 7, device='cuda', dtype=dt)
    theta[:, cols] = p
    gtheta, gx = _sentinels(B, n_par + 7, dt=dt), _sentinels(B, D, dt=dt)
    out = _wrapper(name, dt, x, theta[:, cols], gy, gl, out=(gx, gtheta[:, cols]))
    assert out[0] is gx and out[1].data_ptr() == gtheta[:, cols].data_ptr()
    gx_ref, gp_ref = _custom_op(name, dt, x, p, gy, gl)
    assert torch.equal(gx, gx_ref)
    assert torch.equal(gtheta[:, cols], gp_ref)
    assert bool((gtheta[:, :3] == SENTINEL).all()) and bool((gtheta[:, 3 + n_par:] == SENTINEL).all())
    # without ``out``: fresh tensors, the same values
    gx2, gp2 = _wrapper(name, dt, x, theta[:, cols], gy, gl)
    assert torch.equal(gx2, gx_ref) and torch.equal(gp2, gp_ref) and gp2.is_contiguous()


@pytest.mark.parametrize('name,dt', LAYOUT_CASES)
def test_feature_major_layout_in_a_padded_buffer(name, dt):
    x, p, gy, gl = _inputs(name, dt, seed=1)
    P = WRAPPERS[name][0]
    ld = P * D + 5
    theta = torch.randn(B, ld, device='cuda', dtype=dt)
    theta[:, :P * D] = _feature_major(p, P)
    gtheta, gx = _sentinels(B, ld, dt=dt), _sentinels(B, D, dt=dt)
    _wrapper(name, dt, x, theta, gy, gl, layout=(ld, 1, P), out=(gx, gtheta))
    gx_ref, gp_ref = _custom_op(name, dt, x, p, gy, gl)
    assert torch.equal(gx, gx_ref)
    assert torch.equal(gtheta[:, :P * D], _feature_major(gp_ref, P))
    assert bool((gtheta[:, P * D:] == SENTINEL).all())


@pytest.mark.parametrize('name,dt', [(n, d) for n, d in LAYOUT_CASES if n != 'sos'])
def test_forward_wrappers_take_the_same_layout(name, dt):
    from tfep_amd import ops
    x, p, _, _ = _inputs(name, dt, seed=2)
    P = WRAPPERS[name][0]
    ld = P * D + 5
    theta = torch.randn(B, ld, device='cuda', dtype=dt)
    theta[:, :P * D] = _feature_major(p, P)
    if name == 'affine':
        forward = ops.affine
    else:
        cfg = ops.SplineConfig(*_spline_args(dt), dtype=dt)

        def forward(x, parameters, **kw):
            return ops.spline(x, parameters, cfg, **kw)
    got, ref = forward(x, theta, layout=(ld, 1, P)), forward(x, p)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    with pytest.raises(ValueError):                               # a layout that runs past the buffer
        forward(x, theta[:, :P * D - 1], layout=(ld, 1, P))


@pytest.mark.parametrize('name,dt', CASES)
def test_rejections_come_before_any_launch(name, dt):
    x, p, gy, gl = _inputs(name, dt, seed=3)
    P, _, takes_layout, _ = WRAPPERS[name]
    n_par = p.shape[1]
    gx = _sentinels(B, D, dt=dt)

    def intact(*buffers):
        return all(bool((b == SENTINEL).all()) for b in (gx, *buffers))

    # a gradient block with a column stride of two
    gwide = _sentinels(B, 2 * n_par, dt=dt)
    with pytest.raises(ValueError):
        _wrapper(name, dt, x, p, gy, gl, out=(gx, gwide[:, ::2]))
    # ... and a transposed grad_x
    gxt = _sentinels(D, B, dt=dt)
    gp = _sentinels(B, n_par, dt=dt)
    with pytest.raises(ValueError):
        _wrapper(name, dt, x, p, gy, gl, out=(gxt.t(), gp))
    # grad_y of the wrong shape
    with pytest.raises(ValueError):
        _wrapper(name, dt, x, p, gy[:, :D - 1], gl, out=(gx, gp))
    with pytest.raises(ValueError):
        _wrapper(name, dt, x, p, gy[:B - 1], gl, out=(gx, gp))
    # parameters of the wrong width
    with pytest.raises(ValueError):
        _wrapper(name, dt, x, p[:, :n_par - 1], gy, gl, out=(gx, gp))
    # one tensor of the other dtype
    other = F32 if dt == F64 else F64
    with pytest.raises(TypeError):
        _wrapper(name, dt, x, p, gy.to(other), gl, out=(gx, gp))
    with pytest.raises(TypeError):
        _wrapper(name, dt, x, p, gy, gl, out=(gx, gp.to(other)))
    assert intact(gwide, gxt, gp)
    if takes_layout:                                              # a layout that runs past the buffer's width
        ld = P * D + 5
        theta = torch.randn(B, ld, device='cuda', dtype=dt)
        gtheta = _sentinels(B, ld, dt=dt)
        with pytest.raises(ValueError):
            _wrapper(name, dt, x, theta[:, :P * D - 1], gy, gl, layout=(ld, 1, P), out=(gx, gtheta))
        with pytest.raises(ValueError):
            _wrapper(name, dt, x, theta, gy, gl, layout=(ld, 1, P), out=(gx, gtheta[:, :P * D - 1]))
        with pytest.raises(ValueError):                           # ... or whose row stride is not the buffer's
            _wrapper(name, dt, x, theta, gy, gl, layout=(ld - 1, 1, P), out=(gx, gtheta))
        assert intact(gtheta)


@pytest.mark.parametrize('name,dt', GL_CASES)
def test_no_log_det_cotangent_is_a_zero_cotangent(name, dt):
    x, p, gy, gl = _inputs(name, dt, seed=4)
    gx0, gp0 = _wrapper(name, dt, x, p, gy, torch.zeros_like(gl))
    gx, gp = _wrapper(name, dt, x, p, gy, None)
    assert torch.equal(gx, gx0) and torch.equal(gp, gp0)
    gx1, gp1 = _wrapper(name, dt, x, p, gy, gl)                   # (and the cotangent does reach the kernel)
    assert not torch.equal(gp1, gp0)


@pytest.mark.parametrize('dt', [F32, F64])
def test_spline_config_take_follows_a_permutation_and_a_subset(dt):
    from tfep_amd import ops
    x, p, _, _ = _inputs('spline', dt, seed=5)
    P = WRAPPERS['spline'][0]
    cfg = ops.SplineConfig(*_spline_args(dt), dtype=dt)
    y, ldj = ops.spline(x, p, cfg)
    p3 = p.reshape(B, P, D)
    # one feature at a time: its own y and its own term of the log-det
    terms = torch.empty(B, D, device='cuda', dtype=dt)
    for f in range(D):
        sub = cfg.take(torch.tensor([f], device='cuda'))
        assert sub.dtype == dt and sub.n_parameters_per_feature == P
        y_f, terms[:, f] = ops.spline(x[:, f:f + 1], p3[:, :, f], sub)
        assert torch.equal(y_f[:, 0], y[:, f])
    perm = torch.randperm(D, device='cuda', generator=torch.Generator(device='cuda').manual_seed(6))
    assert not torch.equal(perm, torch.arange(D, device='cuda'))
    y_p, ldj_p = ops.spline(x[:, perm], p3[:, :, perm].reshape(B, P * D), cfg.take(perm))
    assert torch.equal(y_p, y[:, perm])
    # the log-det is the sum of the D terms in another order: at most D - 1 roundings of partial sums that |terms| bounds
    # (float32: the sum runs in float64 and is rounded once)
    bound = D * torch.finfo(dt).eps * terms.abs().sum(dim=1)
    assert bool(((ldj_p - ldj).abs() <= bound).all()), float(((ldj_p - ldj).abs() / bound).max())
