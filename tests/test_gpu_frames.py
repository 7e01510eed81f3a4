"""GPU tests of the frame kernels (csrc/frames.hip) and of the Cartesian flow wrappers in float64: CenteredCentroidFlow /
OrientedFlow / PartialFlow / PCAWhitenedFlow.

The reference formula of the kernel route is the torch route of the same classes (``frame_kernels=False``: utils/geometry.py,
centroid.py, oriented.py as they were), float64, same input: values and gradients agree to a relative L2 of 1e-10, the
float64 contract of the project.  Against the reference's fixtures (which build the rotation through acos / asin) the
kernel route is allowed 4x the error measured for the torch route on the same input, with a floor of 1e-12."""
import contextlib
import itertools

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
BATCHES = (1, 3, 65)
N_POINTS = (2, 3, 64, 65, 130)          # the minimum, below / exactly / past one pass of the 64 lanes, more than two passes
FRAMES = (('x', 'xy'), ('y', 'xy'), ('y', 'yz'), ('z', 'yz'), ('x', 'xz'), ('z', 'xz'))


def rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def rand(*shape, seed=0, dtype=F64):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randn(*shape, device='cuda', dtype=dtype, generator=g)


class Stretch(torch.nn.Module):
    """A stand-in for the wrapped flow that runs in any dtype and moves every coordinate (so that restoring the centroid
    and rotating back have something to do): y_j = (1.25 + 0.5 cos j) x_j + 0.3 sin j."""

    def _ab(self, x):
        j = torch.arange(x.shape[1], device=x.device, dtype=x.dtype)
        return 1.25 + 0.5 * torch.cos(j), 0.3 * torch.sin(j)

    def forward(self, x):
        a, b = self._ab(x)
        return a * x + b, torch.log(a).sum().expand(len(x))

    def inverse(self, y):
        a, b = self._ab(y)
        return (y - b) / a, -torch.log(a).sum().expand(len(y))

    def n_parameters(self):
        return 0


def both_routes(make):
    """The same wrapper twice: on the frame kernels and on the torch ops."""
    k, t = make().cuda(), make().cuda()
    k.frame_kernels, t.frame_kernels = True, False
    return k, t


def run_both(make, x, inverse=False):
    k, t = both_routes(make)
    with torch.no_grad():
        out_k = k.inverse(x) if inverse else k(x)
        out_t = t.inverse(x) if inverse else t(x)
    assert k.last_route == 'kernels' and t.last_route == 'torch'
    return out_k, out_t


PAD = 5                                  # extra columns of the wider tensor a sliced input is cut from (2 left, 3 right)


def points(B, n, dim=3, seed=0, sliced=False):
    """(B, n dim) float64 input; ``sliced``: a column slice of a wider tensor (row stride > width)."""
    if not sliced:
        return 1.5 * rand(B, n * dim, seed=seed)
    wide = 1.5 * rand(B, n * dim + PAD, seed=seed)
    return wide[:, 2:2 + n * dim]


def strided(t):
    """The values of ``t`` as a column slice of a wider tensor."""
    wide = torch.zeros(t.shape[0], t.shape[1] + PAD, device=t.device, dtype=t.dtype)
    view = wide[:, 2:2 + t.shape[1]]
    view.copy_(t)
    return view


def is_strided(x):
    """Whether the kernels see a row stride other than the row's width (a one-row tensor has no row stride to speak of)."""
    return x.shape[0] > 1 and x.stride(0) == x.shape[1] + PAD and x.stride(1) == 1


def leaf(t, sliced=False):
    """A differentiable copy of ``t`` as ``(leaf, input)``; ``sliced``: the input is a column slice of the wider leaf, so
    the kernels read a strided tensor and the gradient lands in the slice of ``leaf.grad`` (zeros around it)."""
    if not sliced:
        x = t.detach().clone().requires_grad_(True)
        return x, x
    wide = strided(t.detach())._base.requires_grad_(True)
    x = wide[:, 2:2 + t.shape[1]]
    assert is_strided(x) or len(t) == 1
    return wide, x


@contextlib.contextmanager
def default_float64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


# ------------------------------------------------------------------ 1. the wrappers run in float64 (fails before this change)

def build_wrapped(name, g):
    import tfep_amd.nn.flows as flows
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import AffineTransformer, NeuralSplineTransformer
    from oracle.made import generate_degrees
    cfg = gu.wrapper_configs()[name]
    n_in = gu.wrapper_n_inner(cfg)
    if cfg.get('spline'):
        tr = NeuralSplineTransformer(x0=torch.full((n_in,), -8.0), xf=torch.full((n_in,), 8.0), n_bins=6)
    else:
        tr = AffineTransformer()
    inner = MAF(degrees_in=torch.as_tensor(generate_degrees(n_in, 'ascending')), transformer=tr, initialize_identity=False)
    flow = gu.build_wrapped(cfg, inner, flows)
    sd = flow.state_dict()
    for k, v in gu.sub(g, f'{name}/sd/').items():
        assert k in sd, k
        sd[k] = torch.from_numpy(np.asarray(v))
    flow.load_state_dict(sd, strict=True)
    return flow.cuda(), cfg


def wrappers_of(flow):
    from tfep_amd.nn.flows import CenteredCentroidFlow, OrientedFlow
    return [m for m in flow.modules() if isinstance(m, (CenteredCentroidFlow, OrientedFlow))]


def set_route(flow, setting):
    for m in wrappers_of(flow):
        m.frame_kernels = setting


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(F64).cuda()


def fixture_errors(name, g, setting):
    """Errors of the float64 flow against the reference's float64 fixture with the given route: forward y / log-det and,
    where the fixture has them, inverse x / log-det (relative L2; max abs for the log-dets)."""
    flow, cfg = build_wrapped(name, g)
    flow = flow.double()
    set_route(flow, setting)
    errs = {}
    with torch.no_grad():
        y, ldj = flow(dev64(g[f'{name}/x']))
        assert y.dtype == F64 and ldj.dtype == F64 and y.shape == g[f'{name}/y_f64'].shape
        errs['y'] = rel(y, g[f'{name}/y_f64'])
        errs['ldj'] = float(np.abs(ldj.cpu().numpy() - g[f'{name}/ldj_f64']).max())
        if cfg['inverse']:
            x, ldji = flow.inverse(dev64(g[f'{name}/inv_in']))
            errs['xinv'] = rel(x, g[f'{name}/xinv_f64'])
            errs['ldjinv'] = float(np.abs(ldji.cpu().numpy() - g[f'{name}/ldjinv_f64']).max())
    want = 'kernels' if setting in (None, True) else 'torch'
    assert all(m.last_route == want for m in wrappers_of(flow)), [m.last_route for m in wrappers_of(flow)]
    return errs


def test_float64_nested_flow_runs_forward_and_inverse():
    """CenteredCentroidFlow(OrientedFlow(PartialFlow(MAF with an RQ spline))) in float64, as ``flow.double()`` gives it, with
    nothing else set: the kernel route.  Before float64 wrappers PartialFlow raised a TypeError on the input."""
    g = gu.load('wrappers.npz')
    kernel, torch_route = fixture_errors('nested', g, None), fixture_errors('nested', g, False)
    print('nested float64 vs fixture: kernels', kernel, 'torch', torch_route)
    for key, err in kernel.items():
        assert err <= max(4 * torch_route[key], 1e-12), (key, err, torch_route[key])
    flow, _ = build_wrapped('nested', g)
    flow = flow.double()
    x0 = dev64(g['nested/x'])
    with torch.no_grad():
        y, l_f = flow(x0)
        x1, l_i = flow.inverse(y)
    # the tolerances tests/test_gpu_float64_flows.py holds the round trip of a float64 flow to
    np.testing.assert_allclose(x1.cpu().numpy(), x0.cpu().numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose((l_f + l_i).cpu().numpy(), np.zeros(len(x0)), rtol=0, atol=1e-8)


@pytest.mark.parametrize('name', list(gu.wrapper_configs()))
def test_float64_wrappers_against_the_reference_fixtures(name):
    g = gu.load('wrappers.npz')
    kernel, torch_route = fixture_errors(name, g, True), fixture_errors(name, g, False)
    print(f'{name} float64 vs fixture: kernels', kernel, 'torch', torch_route)
    for key, err in kernel.items():
        assert err <= max(4 * torch_route[key], 1e-12), (key, err, torch_route[key])


# ------------------------------------------------------------------ 2. kernels against the torch route, float64

def orient_cases(n):
    """(axis point, plane point) in either order, the last point of the row included, with every flag combination the
    constructor allows spread over the six frames."""
    pairs = [(0, 1), (1, 0), (n - 1, 0), (0, n - 1)] if n > 2 else [(0, 1), (1, 0)]
    flags = [dict(round_off_imprecisions=True, rotate_back=True), dict(round_off_imprecisions=False, rotate_back=True),
             dict(round_off_imprecisions=True, rotate_back=False), dict(round_off_imprecisions=False, rotate_back=False),
             dict(round_off_imprecisions=True, rotate_back=False, return_partial=True),
             dict(round_off_imprecisions=False, rotate_back=False, return_partial=True)]
    for i, ((axis, plane), (a, p)) in enumerate(itertools.product(FRAMES, pairs)):
        yield dict(axis=axis, plane=plane, axis_point_idx=a, plane_point_idx=p, **flags[i % len(flags)])


def special_rows(x, kw):
    """Row 0: the axis point nearer -axis (the flip).  Last row: the axis point exactly on +axis and the plane point with
    an in-plane coordinate of exactly zero, so that q_p == 0 (the sign == 0 branch).  Written in place: a sliced input
    stays the column slice it is."""
    a, p, ax = kw['axis_point_idx'], kw['plane_point_idx'], 'xyz'.index(kw['axis'])
    pl = 'xyz'.index(next(c for c in kw['plane'] if c != kw['axis']))
    x[0, 3 * a + ax] = -x[0, 3 * a + ax].abs() - 0.5
    if len(x) > 1:
        x[-1, 3 * a:3 * a + 3] = 0.0
        x[-1, 3 * a + ax] = 2.0
        x[-1, 3 * p + pl] = 0.0
    return x


@pytest.mark.parametrize('n', N_POINTS)
def test_oriented_kernels_match_the_torch_route_float64(n):
    from tfep_amd.nn.flows import OrientedFlow
    for B, (i, kw) in itertools.product(BATCHES, enumerate(orient_cases(n))):
        x = special_rows(points(B, n, seed=100 + i, sliced=i % 3 == 0), kw)
        assert is_strided(x) == (i % 3 == 0 and B > 1)          # (the module hands x to frame_orient as it is)
        out_k, out_t = run_both(lambda: OrientedFlow(Stretch(), **kw), x)
        assert out_k[0].shape == out_t[0].shape and out_k[0].dtype == F64
        assert rel(out_k[0], out_t[0]) <= 1e-10 and rel(out_k[1], out_t[1]) <= 1e-10, (B, n, kw, rel(out_k[0], out_t[0]))
        if kw['rotate_back']:
            y = out_t[0]
            inv_k, inv_t = run_both(lambda: OrientedFlow(Stretch(), **kw), y, inverse=True)
            assert rel(inv_k[0], inv_t[0]) <= 1e-10, (B, n, kw)
            # and the inverse undoes the forward -- except on the q_p == 0 row (the last one), where the map is not
            # invertible: its in-plane rotation is the identity, so the plane point is not ON the plane and the
            # round-off (or the wrapped flow, which never sees that coordinate) discards where it was
            keep = slice(0, max(B - 1, 1))
            assert rel(inv_k[0][keep], x[keep]) <= 1e-9


@pytest.mark.parametrize('n', N_POINTS)
def test_frame_orient_op_float64(n):
    """The op itself: the framed row and R against utils/geometry.py, exact zeros, R R^T = 1 and det R = 1 to 1e-12, on the
    flip row and the q_p == 0 row too."""
    import tfep_amd.torch_ops  # noqa: F401
    from tfep_amd.nn.flows import OrientedFlow
    from tfep_amd.utils.geometry import batchwise_rotate, reference_frame_rotation_matrix
    for B, (i, kw) in itertools.product(BATCHES, enumerate(orient_cases(n))):
        flow = OrientedFlow(Stretch(), **kw).cuda()
        a, p = flow._points
        x = special_rows(points(B, n, seed=200 + i, sliced=i % 2 == 0), kw)
        assert is_strided(x) == (i % 2 == 0 and B > 1)
        round_off = kw['round_off_imprecisions']
        y, rot = torch.ops.tfep.frame_orient(x, a, p, *flow._frame, round_off)
        if is_strided(x):                                    # the same bits as from a contiguous copy
            yc, rotc = torch.ops.tfep.frame_orient(x.contiguous(), a, p, *flow._frame, round_off)
            assert torch.equal(y, yc) and torch.equal(rot, rotc)
        pts = x.reshape(B, n, 3)
        ref_rot = reference_frame_rotation_matrix(pts[:, a], pts[:, p], flow._axis, flow._plane_axis, flow._plane_normal)
        ref_y = batchwise_rotate(pts, ref_rot).reshape(B, -1)
        if round_off:
            ref_y = ref_y.index_fill(1, flow._fixed_indices, 0.0)
        R = rot.reshape(B, 3, 3)
        assert rel(R, ref_rot) <= 1e-10 and rel(y, ref_y) <= 1e-10, (B, n, kw)
        eye = torch.eye(3, device='cuda', dtype=F64).expand(B, 3, 3)
        assert float((R @ R.transpose(1, 2) - eye).abs().max()) <= 1e-12
        assert float((torch.linalg.det(R) - 1.0).abs().max()) <= 1e-12
        if round_off:
            assert torch.all(y[:, flow._fixed_indices] == 0)
        else:       # (not on the q_p == 0 row, the last one: there the plane point stays where it is, off the plane)
            regular = y[:max(B - 1, 1)]
            assert float(regular[:, flow._fixed_indices].abs().max()) <= 1e-11 * float(x.abs().max())
        if B > 1:                                            # the q_p == 0 row: R1 = 1 and R2 = 1 exactly
            assert torch.equal(R[-1], eye[-1])
        # rotating back: y R, and its transposed form -- from a contiguous row and from a column slice
        for view in ((lambda t: t), strided):
            y_in = view(y)
            assert is_strided(y_in) == (view is strided and B > 1)
            back = torch.ops.tfep.frame_rotate(y_in, rot, False)
            assert rel(back, batchwise_rotate(y.reshape(B, n, 3), ref_rot, inverse=True).reshape(B, -1)) <= 1e-10
            again = torch.ops.tfep.frame_rotate(view(back), rot, True)
            assert rel(again, batchwise_rotate(back.reshape(B, n, 3), ref_rot).reshape(B, -1)) <= 1e-10


def centroid_cases(n, dim):
    """Subsets with and without weights, the fixed point first and last in the subset, a single-point subset, a non-zero
    origin, translate_back and return_partial off and on."""
    origin = [0.5, -1.0, 2.0][:dim]
    subset = [n - 1, 0] if n < 4 else [n - 1, 1, 0, n // 2]
    w = [1.0, 12.0, 16.0, 14.0][:len(subset)]
    yield dict()
    yield dict(origin=origin, fixed_point_idx=n - 1)
    yield dict(weights=[1.0 + 0.25 * (i % 7) for i in range(n)], fixed_point_idx=n // 2, translate_back=False)
    yield dict(subset_point_indices=subset, fixed_point_idx=0, origin=origin)
    yield dict(subset_point_indices=subset, fixed_point_idx=len(subset) - 1, translate_back=False)
    yield dict(subset_point_indices=subset, weights=w, fixed_point_idx=0, translate_back=False, origin=origin)
    yield dict(subset_point_indices=subset, weights=w, fixed_point_idx=len(subset) - 1, origin=origin)
    yield dict(subset_point_indices=[n - 1])
    yield dict(subset_point_indices=[0], origin=origin, translate_back=False)
    yield dict(subset_point_indices=subset, weights=w, fixed_point_idx=1, translate_back=False, return_partial=True)
    yield dict(translate_back=False, return_partial=True, origin=origin)


@pytest.mark.parametrize('n', N_POINTS)
def test_centroid_kernels_match_the_torch_route_float64(n):
    from tfep_amd.nn.flows import CenteredCentroidFlow
    for B, dim in itertools.product(BATCHES, (3, 2, 1)):
        for i, kw in enumerate(centroid_cases(n, dim)):
            x = points(B, n, dim, seed=300 + i, sliced=i % 3 == 1)
            assert is_strided(x) == (i % 3 == 1 and B > 1)

            def make():
                # built under a float64 default dtype: the constructor normalises the weights in the default dtype, and
                # float32-normalised weights sum to 1 only to 6e-8, which is then the accuracy of the round trip
                with default_float64():
                    return CenteredCentroidFlow(Stretch(), space_dimension=dim, **kw)
            out_k, out_t = run_both(make, x)
            assert out_k[0].shape == out_t[0].shape and out_k[0].dtype == F64
            assert rel(out_k[0], out_t[0]) <= 1e-10 and rel(out_k[1], out_t[1]) <= 1e-10, (B, n, dim, kw, rel(out_k[0], out_t[0]))
            if kw.get('translate_back', True):
                inv_k, inv_t = run_both(make, strided(out_t[0]) if i % 2 else out_t[0], inverse=True)
                assert rel(inv_k[0], inv_t[0]) <= 1e-10, (B, n, dim, kw)
                assert rel(inv_k[0], x) <= 1e-9, (B, n, dim, kw, rel(inv_k[0], x))      # the inverse undoes the forward


def test_centroid_of_more_than_three_dimensions_takes_the_torch_route():
    from tfep_amd.nn.flows import CenteredCentroidFlow
    flow = CenteredCentroidFlow(Stretch(), space_dimension=4).cuda()
    flow.frame_kernels = True
    with torch.no_grad():
        y, _ = flow(points(3, 5, 4))
    assert flow.last_route == 'torch' and y.dtype == F64


# ------------------------------------------------------------------ 3. VJPs against torch autograd through the torch route

VJP_N = (2, 3, 65)


def grads_of(flow, x, weight_seed, inverse=False, sliced=False):
    """The gradient of a weighted sum of the flow's output at the leaf ``x`` is cut from (``leaf``: with ``sliced`` the flow
    -- and so the kernels, forward and backward -- sees a column slice of the wider leaf)."""
    wide, x = leaf(x, sliced)
    y, ldj = flow.inverse(x) if inverse else flow(x)
    c = rand(*y.shape, seed=weight_seed)
    (y * c).sum().backward()
    return wide.grad


@pytest.mark.parametrize('n', VJP_N)
def test_wrapper_vjps_match_autograd_of_the_torch_route_float64(n):
    from tfep_amd.nn.flows import CenteredCentroidFlow, OrientedFlow
    B = 3
    for i, kw in enumerate(orient_cases(n)):
        if kw.get('return_partial'):
            continue
        x = special_rows(points(B, n, seed=400 + i), kw)
        sl = i % 2 == 1
        k, t = both_routes(lambda: OrientedFlow(Stretch(), **kw))
        # (with rotate_back the loss reaches x through R twice: the framing and the rotation back)
        assert rel(grads_of(k, x, 7, sliced=sl), grads_of(t, x, 7, sliced=sl)) <= 1e-10, (n, kw)
        if kw['rotate_back']:
            assert rel(grads_of(k, x, 8, True, sl), grads_of(t, x, 8, True, sl)) <= 1e-10, (n, kw)
    for dim in (3, 2, 1):
        for i, kw in enumerate(centroid_cases(n, dim)):
            if kw.get('return_partial'):
                continue
            x = points(B, n, dim, seed=500 + i)
            sl = i % 2 == 0
            k, t = both_routes(lambda: CenteredCentroidFlow(Stretch(), space_dimension=dim, **kw))
            assert rel(grads_of(k, x, 9, sliced=sl), grads_of(t, x, 9, sliced=sl)) <= 1e-10, (n, dim, kw)


@pytest.mark.parametrize('n', VJP_N)
def test_op_vjps_match_autograd_float64(n):
    """The four ops one by one, every differentiable input and output: x and R of frame_rotate, x of frame_orient from a
    loss on R alone and from a loss on y, x / y and shift of the two centroid ops."""
    import tfep_amd.torch_ops  # noqa: F401
    from tfep_amd.nn.flows import CenteredCentroidFlow, OrientedFlow
    from tfep_amd.utils.geometry import batchwise_rotate, reference_frame_rotation_matrix
    from tfep_amd.utils.misc import atom_to_flattened, flattened_to_atom
    B = 3

    def check(got, ref, what):
        for k, (a, b) in enumerate(zip(got, ref)):
            assert rel(a, b) <= 1e-10, (what, k, rel(a, b))

    for i, kw in enumerate(orient_cases(n)):
        flow = OrientedFlow(Stretch(), **kw).cuda()
        a, p = flow._points
        round_off = kw['round_off_imprecisions']
        x = special_rows(points(B, n, seed=600 + i), kw)
        cy, cr = rand(B, 3 * n, seed=1), rand(B, 9, seed=2)

        def torch_orient(x):
            pts = x.reshape(B, n, 3)
            rot = reference_frame_rotation_matrix(pts[:, a], pts[:, p], flow._axis, flow._plane_axis, flow._plane_normal)
            y = batchwise_rotate(pts, rot).reshape(B, -1)
            return (y.index_fill(1, flow._fixed_indices, 0.0) if round_off else y), rot.reshape(B, 9)
        # every loss from a contiguous leaf and from a column slice of a wider leaf: then frame_orient, frame_rotate and
        # their backward kernels read a strided x (the cotangent autograd hands them is contiguous)
        for (wy, wr, what), sl in itertools.product(((1.0, 0.0, 'y alone'), (0.0, 1.0, 'R alone'), (1.0, 1.0, 'y and R')),
                                                    (False, True)):
            xs = [leaf(x, sl), leaf(x, sl)]
            assert is_strided(xs[0][1]) == sl
            for (_, xi), fn in zip(xs, (lambda v: torch.ops.tfep.frame_orient(v, a, p, *flow._frame, round_off), torch_orient)):
                y, rot = fn(xi)
                (wy * (y * cy).sum() + wr * (rot * cr).sum()).backward()
            check([xs[0][0].grad], [xs[1][0].grad], ('frame_orient', what, sl, kw))
        rot0 = torch_orient(x)[1].detach()
        for transposed, sl in itertools.product((False, True), (False, True)):
            xs, rs = [leaf(x, sl), leaf(x, sl)], [leaf(rot0)[0], leaf(rot0)[0]]
            assert is_strided(xs[0][1]) == sl
            (torch.ops.tfep.frame_rotate(xs[0][1], rs[0], transposed) * cy).sum().backward()
            ref = batchwise_rotate(xs[1][1].reshape(B, n, 3), rs[1].reshape(B, 3, 3), inverse=not transposed).reshape(B, -1)
            (ref * cy).sum().backward()
            check([xs[0][0].grad, rs[0].grad], [xs[1][0].grad, rs[1].grad], ('frame_rotate', transposed, sl))
        # the backward ops called directly with a strided x AND a strided cotangent: the bits of the contiguous call
        xv, gv, gr = strided(x), strided(cy), cr
        assert is_strided(xv) and is_strided(gv)
        frame = (a, p, *flow._frame, round_off)
        assert torch.equal(torch.ops.tfep.frame_orient_backward(xv, gv, gr, *frame),
                           torch.ops.tfep.frame_orient_backward(x, cy, gr, *frame))
        assert torch.equal(torch.ops.tfep.frame_orient_backward(xv, cy, gr, *frame),
                           torch.ops.tfep.frame_orient_backward(x, cy, gr, *frame))
        for got, want in zip(torch.ops.tfep.frame_rotate_backward(xv, rot0, gv, True),
                             torch.ops.tfep.frame_rotate_backward(x, rot0, cy, True)):
            assert torch.equal(got, want)

    for dim in (3, 2, 1):
        for i, kw in enumerate(centroid_cases(n, dim)):
            flow = CenteredCentroidFlow(Stretch(), space_dimension=dim, **kw).double().cuda()
            subset, weights, origin = flow._selection(points(1, n, dim))
            x, y_in = points(B, n, dim, seed=700 + i), points(B, n, dim, seed=701 + i)
            cs, cy = rand(B, dim, seed=3), rand(B, n * dim, seed=4)
            sl = i % 2 == 1                       # a column slice of a wider leaf for every other case
            (wx0, x0), (wx1, x1) = leaf(x, sl), leaf(x, sl)
            assert is_strided(x0) == sl
            shift, y = torch.ops.tfep.centroid_shift(x0, subset, weights, origin, dim)
            ((shift * cs).sum() + (y * cy).sum()).backward()
            pts = flattened_to_atom(x1, dim)
            shift_t = flow.origin - flow._centroid(pts)
            ((shift_t * cs).sum() + (atom_to_flattened(pts + shift_t.unsqueeze(1)) * cy).sum()).backward()
            check([shift, wx0.grad], [shift_t, wx1.grad], ('centroid_shift', dim, kw))
            # centroid_restore: centroid.py's placement of the fixed point and the translation back
            (wy0, y0), (wy1, y1) = leaf(y_in, sl), leaf(y_in, sl)
            s0, s1 = leaf(shift.detach())[0], leaf(shift.detach())[0]
            f = flow._host_fixed_point
            out = torch.ops.tfep.centroid_restore(y0, s0, subset, weights, origin, f, flow._host_fixed_point_idx, dim,
                                                  flow.translate_back)
            (out * cy).sum().backward()
            ref = y1
            if not flow._single_point_centroid:
                y_pts = flattened_to_atom(ref, dim)
                rest, w_fixed = flow._centroid(y_pts, exclude_fixed_point=True)
                fixed_pos = (flow.origin - rest) / w_fixed
                ref = atom_to_flattened(torch.cat([y_pts[:, :f], fixed_pos.unsqueeze(1), y_pts[:, f + 1:]], dim=1))
            if flow.translate_back:
                ref = atom_to_flattened(flattened_to_atom(ref, dim) - s1.unsqueeze(1))
            (ref * cy).sum().backward()
            zero = torch.zeros_like(s0)
            check([out, wy0.grad, s0.grad], [ref, wy1.grad, zero if s1.grad is None else s1.grad],
                  ('centroid_restore', dim, kw))
            # the backward ops called directly with a strided cotangent: the bits of the contiguous call
            gv = strided(cy)
            assert torch.equal(torch.ops.tfep.centroid_shift_backward(gv, cs, subset, weights, dim),
                               torch.ops.tfep.centroid_shift_backward(cy, cs, subset, weights, dim))
            cfg = (subset, weights, f, flow._host_fixed_point_idx, dim, flow.translate_back)
            for got, want in zip(torch.ops.tfep.centroid_restore_backward(gv, *cfg),
                                 torch.ops.tfep.centroid_restore_backward(cy, *cfg)):
                assert torch.equal(got, want)


# ------------------------------------------------------------------ 4. float32

@pytest.mark.parametrize('name', list(gu.wrapper_configs()))
def test_float32_frame_kernels_within_the_reference_noise(name):
    """float32 flows with ``frame_kernels=True`` on every wrapper, held to the margins of tests/test_gpu_wrappers.py: the
    reference's own float32-vs-float64 noise stored in the fixture."""
    g = gu.load('wrappers.npz')
    flow, cfg = build_wrapped(name, g)
    set_route(flow, True)
    x = torch.from_numpy(g[f'{name}/x']).cuda()
    with torch.no_grad():
        y, ldj = flow(x)
    assert all(m.last_route == 'kernels' for m in wrappers_of(flow)) and y.dtype == F32
    noise_y = rel(g[f'{name}/y_f32'], g[f'{name}/y_f64'])
    assert rel(y, g[f'{name}/y_f64']) < max(2 * noise_y, 2e-6)
    noise_l = np.abs(g[f'{name}/ldj_f32'].astype(np.float64) - g[f'{name}/ldj_f64']).max()
    assert np.abs(ldj.cpu().numpy().astype(np.float64) - g[f'{name}/ldj_f64']).max() < max(4 * noise_l, 2e-5)
    if cfg['inverse']:
        with torch.no_grad():
            xi, li = flow.inverse(torch.from_numpy(g[f'{name}/inv_in']).cuda())
        assert rel(xi, g[f'{name}/xinv_f64']) < 2e-5
        assert np.abs(li.cpu().numpy().astype(np.float64) - g[f'{name}/ldjinv_f64']).max() < 1e-4


@pytest.mark.parametrize('name', list(gu.wrapper_configs()))
def test_float32_default_equals_the_outputs_from_before_the_frame_kernels_bit_for_bit(name):
    """With no attribute set a float32 flow takes the torch ops and computes, bit for bit, what the commit before the frame
    kernels computed on the ``wrappers.npz`` inputs (``wrappers_f32_before_frames.npz``, written from that commit by
    tools/dump_wrapper_outputs.py), forward and inverse; ``frame_kernels=False`` gives the same bits."""
    g, before = gu.load('wrappers.npz'), gu.load('wrappers_f32_before_frames.npz')
    for setting in (None, False):
        flow, cfg = build_wrapped(name, g)
        set_route(flow, setting)
        assert all(m.frame_kernels is setting for m in wrappers_of(flow))
        with torch.no_grad():
            got = dict(zip(('y', 'ldj'), flow(torch.from_numpy(g[f'{name}/x']).cuda())))
            if cfg['inverse']:
                got.update(zip(('xinv', 'ldjinv'), flow.inverse(torch.from_numpy(g[f'{name}/inv_in']).cuda())))
        assert all(m.last_route == 'torch' for m in wrappers_of(flow))
        assert sorted(got) == sorted(k.split('/')[1] for k in before.files if k.startswith(name + '/'))
        for key, value in got.items():
            assert value.dtype == F32 and np.array_equal(value.cpu().numpy(), before[f'{name}/{key}']), (setting, key)


# ------------------------------------------------------------------ 5. batch independence, opcheck, dtype contract

@pytest.mark.parametrize('dtype', [F32, F64])
def test_row_is_bitwise_batch_independent(dtype):
    import tfep_amd.torch_ops  # noqa: F401
    n = 130
    big = points(65, n, seed=11).to(dtype)
    one = big[:1].clone()
    sub = torch.tensor([n - 1, 3, 70], dtype=torch.int32, device='cuda')
    w = torch.tensor([0.2, 0.3, 0.5], dtype=dtype, device='cuda')
    origin = torch.tensor([0.5, -1.0, 2.0], dtype=dtype, device='cuda')

    def run(x):
        shift, y = torch.ops.tfep.centroid_shift(x, sub, w, origin, 3)
        out = torch.ops.tfep.centroid_restore(y, shift, sub, w, origin, 3, 1, 3, True)
        framed, rot = torch.ops.tfep.frame_orient(out, 129, 1, 2, 1, -1, True)
        back = torch.ops.tfep.frame_rotate(framed, rot, False)
        g = torch.ops.tfep.frame_orient_backward(x, back, rot, 129, 1, 2, 1, -1, True)
        gx, grot = torch.ops.tfep.frame_rotate_backward(x, rot, back, True)
        gs = torch.ops.tfep.centroid_shift_backward(back, shift, sub, w, 3)
        gy, gsh = torch.ops.tfep.centroid_restore_backward(back, sub, w, 3, 1, 3, True)
        return shift, y, out, framed, rot, back, g, gx, grot, gs, gy, gsh
    for a, b in zip(run(one), run(big)):
        assert a.dtype == dtype and torch.equal(a[0], b[0])


@pytest.mark.parametrize('dtype', [F32, F64])
def test_opcheck_frame_ops(dtype):
    import tfep_amd.torch_ops  # noqa: F401
    B, n = 5, 4

    def r(*shape, grad=False, seed=0):
        return rand(*shape, seed=seed, dtype=dtype).requires_grad_(grad)
    sub = torch.tensor([3, 0, 2], dtype=torch.int32, device='cuda')
    w = torch.tensor([0.2, 0.3, 0.5], dtype=dtype, device='cuda')
    origin = torch.tensor([0.5, -1.0, 2.0], dtype=dtype, device='cuda')
    t = torch.ops.tfep
    for subset, weights in ((sub, w), (None, None)):
        torch.library.opcheck(t.centroid_shift.default, (r(B, 3 * n, grad=True), subset, weights, origin, 3))
        torch.library.opcheck(t.centroid_restore.default,
                              (r(B, 3 * n, grad=True), r(B, 3, grad=True, seed=1), subset, weights, origin, 0, 1 if subset is not None else 0, 3, True))
        torch.library.opcheck(t.centroid_shift_backward.default, (r(B, 3 * n), r(B, 3), subset, weights, 3))
        torch.library.opcheck(t.centroid_restore_backward.default, (r(B, 3 * n), subset, weights, 0, 1 if subset is not None else 0, 3, True))
    torch.library.opcheck(t.frame_orient.default, (r(B, 3 * n, grad=True), 3, 1, 1, 0, -3, True))
    torch.library.opcheck(t.frame_orient_backward.default, (r(B, 3 * n), r(B, 3 * n, seed=1), r(B, 9), 3, 1, 1, 0, -3, True))
    torch.library.opcheck(t.frame_rotate.default, (r(B, 3 * n, grad=True), r(B, 9, grad=True, seed=2), False))
    torch.library.opcheck(t.frame_rotate_backward.default, (r(B, 3 * n), r(B, 9), r(B, 3 * n, seed=3), True))


def test_mixed_dtypes_are_type_errors_and_bad_shapes_value_errors():
    import tfep_amd.torch_ops  # noqa: F401
    t = torch.ops.tfep
    x64, x32 = rand(3, 12), rand(3, 12, dtype=F32)
    o64, o32 = rand(3), rand(3, dtype=F32)
    with pytest.raises(TypeError):
        t.centroid_shift(x64, None, None, o32, 3)
    with pytest.raises(TypeError):
        t.centroid_shift(x32, None, rand(4), o32, 3)
    with pytest.raises(TypeError):
        t.centroid_restore(x64, rand(3, 3, dtype=F32), None, None, o64, 0, 0, 3, True)
    with pytest.raises(TypeError):
        t.frame_rotate(x32, rand(3, 9), False)
    with pytest.raises(TypeError):
        t.frame_orient_backward(x64, x32, rand(3, 9), 0, 1, 0, 1, 3, True)
    with pytest.raises(ValueError, match='no multiple of 3'):
        t.frame_orient(rand(3, 10), 0, 1, 0, 1, 3, True)
    with pytest.raises(ValueError, match='n_points=1'):
        t.frame_orient(rand(3, 3), 0, 0, 0, 1, 3, True)
    with pytest.raises(ValueError, match='plane_point=4 out of range'):
        t.frame_orient(x64, 0, 4, 0, 1, 3, True)
    with pytest.raises(ValueError, match='weights has 2 entries for 4 points'):
        t.centroid_shift(x64, None, rand(2), o64, 3)
    # degenerate geometry is not special-cased: a zero-length axis point gives NaN, as the torch code does
    x = x64.clone()
    x[1, 0:3] = 0.0
    y, rot = t.frame_orient(x, 0, 1, 0, 1, 3, False)
    assert torch.isnan(rot[1]).all() and torch.isnan(y[1]).all() and torch.isfinite(y[[0, 2]]).all()


# ------------------------------------------------------------------ 6. training

def test_training_gradients_of_the_float64_nested_flow():
    """One backward of y.sum() + ldj.sum() through CenteredCentroidFlow(OrientedFlow(PartialFlow(MAF))) in float64, against
    the reference's float64 autograd (tests/golden/wrappers_f64.npz): parameter gradients to the tolerance of
    tests/test_gpu_float64_flows.py::test_training_gradients_float64 (max |got - ref| <= 1e-9 max |ref| per tensor)."""
    g, g64 = gu.load('wrappers.npz'), gu.load('wrappers_f64.npz')
    flow, _ = build_wrapped('nested', g)
    flow = flow.double()
    x = dev64(g['nested/x']).requires_grad_(True)
    y, ldj = flow(x)
    assert all(m.last_route == 'kernels' for m in wrappers_of(flow)) and y.requires_grad and ldj.requires_grad
    (y.sum() + ldj.sum()).backward()
    n = 0
    for k, p in flow.named_parameters():
        ref = g64[f'nested/gsum_p/{k}']
        assert p.grad is not None and p.grad.dtype == F64 and tuple(p.grad.shape) == ref.shape, k
        err = np.abs(p.grad.cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-300)
        assert err <= 1e-9, (k, err)
        n += 1
    assert n > 0
    # the input gradient passes through the frame kernels' VJPs: 4x the torch route's own distance to the reference
    torch_flow, _ = build_wrapped('nested', g)
    torch_flow = torch_flow.double()
    set_route(torch_flow, False)
    xt = dev64(g['nested/x']).requires_grad_(True)
    yt, lt = torch_flow(xt)
    (yt.sum() + lt.sum()).backward()
    e_k, e_t = rel(x.grad, g64['nested/gsum_x_f64']), rel(xt.grad, g64['nested/gsum_x_f64'])
    print('nested float64 input gradient vs fixture: kernels', e_k, 'torch', e_t)
    assert e_k <= max(4 * e_t, 1e-12)


# ------------------------------------------------------------------ 7. PCA

def build_pca(name, g):
    from oracle.made import generate_degrees
    from tfep_amd.nn.flows import MAF, PCAWhitenedFlow
    from tfep_amd.nn.transformers import AffineTransformer, NeuralSplineTransformer
    cfg = gu.pca_configs()[name]
    D = cfg['D']
    tr = NeuralSplineTransformer(x0=torch.full((D,), -9.0), xf=torch.full((D,), 9.0), n_bins=5) if cfg['spline'] \
        else AffineTransformer()
    inner = MAF(degrees_in=torch.as_tensor(generate_degrees(D, cfg['order'])), transformer=tr, initialize_identity=False)
    flow = PCAWhitenedFlow(inner, gu.pca_data(cfg), blacken=cfg['blacken'])
    sd = flow.state_dict()
    for k, v in gu.sub(g, f'{name}/sd/').items():
        sd[k] = torch.from_numpy(np.asarray(v))
    flow.load_state_dict(sd, strict=True)
    return flow.cuda()


@pytest.mark.parametrize('name', list(gu.pca_configs()))
def test_pca_whitened_flow_float64(name):
    """Forward, inverse and log-det (``pca_spline_white``: blacken off, so the whitening log-det is in it) of a float64
    PCAWhitenedFlow against the reference's float64 run, relative L2 <= 1e-10."""
    g = gu.load('pca.npz')
    flow = build_pca(name, g).double()
    assert flow.whitening_matrix.dtype == F64
    with torch.no_grad():
        y, ldj = flow(dev64(g[f'{name}/x']))
        xi, li = flow.inverse(dev64(g[f'{name}/inv_in']))
    assert y.dtype == F64 and ldj.dtype == F64
    errs = dict(y=rel(y, g[f'{name}/y_f64']), ldj=rel(ldj, g[f'{name}/ldj_f64']), xinv=rel(xi, g[f'{name}/xinv_f64']),
                ldjinv=rel(li, g[f'{name}/ldjinv_f64']))
    print(f'{name} float64 vs fixture:', errs)
    for key, err in errs.items():
        assert err <= 1e-10, (key, err)
    with pytest.raises(TypeError):
        flow(torch.from_numpy(g[f'{name}/x']).cuda())                       # a float32 input on float64 buffers
    with pytest.raises(TypeError):
        build_pca(name, g)(dev64(g[f'{name}/x']))                           # and a float64 input on float32 buffers


def test_pca_built_from_float64_data_keeps_float64_operands():
    from tfep_amd.nn.flows import PCAWhitenedFlow
    data = gu.pca_data(dict(D=8, n_data=500, seed=31)).double()

    class Identity(torch.nn.Module):
        def forward(self, x):
            return x, torch.zeros(len(x), device=x.device, dtype=x.dtype)
        inverse = forward
    flow = PCAWhitenedFlow(Identity(), data, blacken=True).cuda()
    x = data.cuda()
    with torch.no_grad():
        y, ldj = flow(x)
    assert y.dtype == F64 and all(t.dtype == F64 for t in flow._operands(x.device))
    assert rel(y, x) <= 1e-10 and torch.equal(ldj, torch.zeros_like(ldj))
