"""GPU tests of the float64 blocked inverse (``AutoregressiveFlow._inverse_blocked_f64``: fp64-MFMA panel GEMMs + the chain
kernel ``tfep_inverse_chain_f64``): the route is taken and makes no conditioner pass, the reference goldens, agreement with
the pass per degree at sizes no golden covers, bitwise batch invariance, autograd through ``LazyInverseFunction``, and the
argument checks of the new C entry point.

Bounds.  Goldens: those of tests/test_gpu_float64_flows.py::test_flow_inverse_float64.  Blocked against the pass per degree
(both fp64 evaluations of the same sums in another order): x within 1e-10 max|x| + 1e-11, log-det within
1e-9 max(1, |ldj|) per sample -- the project's float64 forward bound (1e-9 / 1e-10) tightened by one decade, because no
reference rounding sits between the two sides."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

F64 = torch.float64


def dev(a, dtype=F64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def close(got, ref, rtol, atol=0.0, what=''):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    np.testing.assert_allclose(got, np.asarray(ref, np.float64), rtol=rtol, atol=atol, err_msg=what)


@contextlib.contextmanager
def default_float64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def f64_flow(name):
    g = gu.load('flows.npz')
    return gu.build_flow(name, g).double(), g


@contextlib.contextmanager
def count_conditioner_passes(flow):
    """Counts the calls of every layer's ``get_transformer_parameters`` (one conditioner forward pass each)."""
    counts = [0] * len(flow)
    originals = []
    for i, layer in enumerate(flow):
        orig = layer.get_transformer_parameters
        originals.append(orig)

        def wrapped(x, _orig=orig, _i=i):
            counts[_i] += 1
            return _orig(x)
        layer.get_transformer_parameters = wrapped
    try:
        yield counts
    finally:
        for layer in flow:
            del layer.get_transformer_parameters


# ------------------------------------------------------------------ 1. the route is taken

@pytest.mark.parametrize('name', ['rq4', 'circ', 'mixflow'])
def test_blocked_route_is_taken_and_makes_no_conditioner_pass(name):
    flow, g = f64_flow(name)
    y = dev(g[f'{name}/inv_in'])
    with torch.no_grad(), count_conditioner_passes(flow) as counts:
        xb, lb = flow.inverse(y)
    assert [layer.last_inverse_route for layer in flow] == ['blocked_f64'] * len(flow)
    assert counts == [0] * len(flow)
    assert all(not layer._blocked_ok() for layer in flow)            # (the float32 predicate stays False on float64 layers)
    for layer in flow:
        layer.blocked_inverse = False
    with torch.no_grad(), count_conditioner_passes(flow) as counts:
        xp, lp = flow.inverse(y)
    assert [layer.last_inverse_route for layer in flow] == ['per_degree'] * len(flow)
    assert counts == [layer._inverse_masks.shape[0] for layer in flow]
    close(xb, xp.cpu().numpy(), 1e-9, 1e-10, 'blocked against per degree')
    close(lb, lp.cpu().numpy(), 1e-9, 1e-9, 'log-det blocked against per degree')


def test_conditioning_features_keep_the_pass_per_degree():
    """A layer with ``_conditioner_indices`` is not claimed: per-degree route, bit-identical to ``blocked_inverse = False``.
    The golden ``cond`` flow is a MAF whose degree -1 features are FIXED features that the conditioner reads at their place
    in x (``_conditioner_indices`` is empty, as in the reference's MAF): those layers qualify for the blocked route, and the
    flow still matches its golden."""
    from tfep_amd.nn.conditioners.made import MADE
    from tfep_amd.nn.flows.autoregressive import AutoregressiveFlow
    from tfep_amd.nn.transformers import AffineTransformer
    torch.manual_seed(5)
    made = MADE(degrees_in=torch.tensor([-1, 0, 1, 2]), degrees_out=torch.tensor([0, 1, 2, 0, 1, 2]))
    layer = AutoregressiveFlow(5, [[2], [3], [4]], made, AffineTransformer(), conditioner_indices=[0, 2, 3, 4],
                               initialize_identity=False).double().cuda()
    assert len(layer._conditioner_indices) > 0
    y = torch.randn(33, 5, device='cuda', dtype=F64, generator=torch.Generator(device='cuda').manual_seed(1))
    with torch.no_grad():
        x1, l1 = layer.inverse(y)
        assert layer.last_inverse_route == 'per_degree'
        layer.blocked_inverse = False
        x2, l2 = layer.inverse(y)
    assert layer.last_inverse_route == 'per_degree'
    assert torch.equal(x1, x2) and torch.equal(l1, l2)

    flow, g = f64_flow('cond')
    assert all(len(layer._conditioner_indices) == 0 and layer.has_fixed_indices for layer in flow)
    with torch.no_grad():
        x, ldj = flow.inverse(dev(g['cond/inv_in']))
    assert [layer.last_inverse_route for layer in flow] == ['blocked_f64'] * len(flow)
    close(x, g['cond/xinv_f64'], 1e-8, 1e-9, 'x')
    close(ldj, g['cond/ldjinv_f64'], 1e-8, 1e-8, 'ldj')


# ------------------------------------------------------------------ 2. reference goldens

@pytest.mark.parametrize('name', ['rq4', 'cond', 'circ', 'mixflow'])
def test_blocked_inverse_matches_the_reference_goldens(name):
    flow, g = f64_flow(name)
    rtol = 1e-7 if name == 'rq4' else 1e-8
    with torch.no_grad():
        x, ldj = flow.inverse(dev(g[f'{name}/inv_in']))
        assert all(layer.last_inverse_route == 'blocked_f64' for layer in flow)
        close(x, g[f'{name}/xinv_f64'], rtol, 1e-9, 'x')
        close(ldj, g[f'{name}/ldjinv_f64'], rtol, 1e-8, 'ldj')
        x0 = dev(g[f'{name}/x'])
        y, l_f = flow(x0)
        x1, l_i = flow.inverse(y)
    close(x1, x0.cpu().numpy(), 1e-9, 1e-9, 'round trip')
    close(l_f + l_i, np.zeros(len(x0)), 0, 1e-8, 'log-dets cancel')


# ------------------------------------------------------------------ 3. against the pass per degree

def _spline(n, lo, hi, bins, **kw):
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    return NeuralSplineTransformer(torch.full((n,), lo), torch.full((n,), hi), bins, **kw)


def _noise_(t, gen, scale):
    t.copy_(scale * torch.randn(t.shape, generator=gen, dtype=t.dtype))


def make_layer(case, seed=0):
    """One float64 MAF layer with seeded, non-identity weights (a freshly built layer is the identity map)."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.embeddings import PeriodicEmbedding
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import AffineTransformer, MixedTransformer
    kw, dom = {}, (-2.0, 2.0)
    with default_float64():
        if case in ('rq8_asc', 'rq8_desc'):
            D = 300
            deg = generate_degrees(D, 'ascending' if case == 'rq8_asc' else 'descending')
            tr = _spline(D, -2.0, 2.0, 8)
        elif case == 'circ':
            D, dom = 96, (0.0, 1.0)
            deg = generate_degrees(D)
            tr = _spline(D, 0.0, 1.0, 5, circular=True)
            kw['embedding'] = PeriodicEmbedding(D, [0.0, 1.0], periodic_indices=list(range(D)))
        elif case in ('affine_h1', 'affine_h3'):
            D = 64
            deg = generate_degrees(D, 'descending')
            tr = AffineTransformer()
            kw['hidden_layers'] = 1 if case == 'affine_h1' else 3
        elif case == 'mixed':
            D = 48
            deg = generate_degrees(D)
            idx_s, idx_a = list(range(0, D, 2)), list(range(1, D, 2))
            tr = MixedTransformer([_spline(len(idx_s), -2.0, 2.0, 6, learn_lower_bound=True), AffineTransformer()],
                                  [idx_s, idx_a])
        elif case == 'fixed':
            D = 50
            deg = generate_degrees(D, 'descending', conditioning_indices=[0, 7, 31], repeats=2)
            tr = _spline(D - 3, -2.0, 2.0, 4, identity_boundary_slopes=True)
            kw['weight_norm'] = False
        elif case == 'ragged':              # 37 degrees: not a multiple of the block size
            D = 37
            deg = generate_degrees(D)
            tr = _spline(D, -2.0, 2.0, 9)
        elif case == 'short':               # fewer degrees than one block
            D = 5
            deg = generate_degrees(D)
            tr = _spline(D, -2.0, 2.0, 8)
        else:
            raise KeyError(case)
        layer = MAF(deg, transformer=tr, **kw)
    gen = torch.Generator().manual_seed(1000 + seed)
    lins = layer._conditioner._linears()
    with torch.no_grad():
        for lin in lins:
            _noise_(lin.bias, gen, 0.1)
        last = lins[-1]
        if last.has_weight_norm:
            _noise_(last.weight_g, gen, 0.1)
        else:
            _noise_(last._parameters['weight'], gen, 0.02)
    layer = layer.double().cuda()
    assert layer.is_float64
    return layer, D, dom


CASES = ['rq8_asc', 'rq8_desc', 'circ', 'affine_h1', 'affine_h3', 'mixed', 'fixed', 'ragged', 'short']


def _inputs(layer, D, dom, B, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    lo, hi = dom
    x = lo + (hi - lo) * (0.02 + 0.96 * torch.rand(B, D, device='cuda', dtype=F64, generator=gen))      # in the domain
    with torch.no_grad():
        y_in = layer(x)[0]
    y_tail = 1.5 * torch.randn(B, D, device='cuda', dtype=F64, generator=gen)                            # reaches the tails
    return {'in-domain': y_in, 'tails': y_tail}


def _both_routes(layer, y):
    with torch.no_grad():
        layer.blocked_inverse = True
        xb, lb = layer.inverse(y)
        assert layer.last_inverse_route == 'blocked_f64'
        layer.blocked_inverse = False
        xp, lp = layer.inverse(y)
        assert layer.last_inverse_route == 'per_degree'
        layer.blocked_inverse = True
    return xb, lb, xp, lp


@pytest.mark.parametrize('B', [257, 1])
@pytest.mark.parametrize('case', CASES)
def test_blocked_matches_pass_per_degree(case, B):
    layer, D, dom = make_layer(case)
    if case == 'ragged':
        assert layer._inverse_masks.shape[0] % layer._blocked_f64_host_plan()['block'] != 0
    if case == 'short':
        assert layer._inverse_masks.shape[0] < layer._blocked_f64_host_plan()['block']
    for what, y in _inputs(layer, D, dom, B, seed=7).items():
        xb, lb, xp, lp = _both_routes(layer, y)
        assert bool(torch.isfinite(xp).all()) and bool(torch.isfinite(lp).all())
        ex = float((xb - xp).abs().max())
        bound_x = 1e-10 * float(xp.abs().max()) + 1e-11
        el = float(((lb - lp).abs() / lp.abs().clamp(min=1.0)).max())
        print(f'{case} B={B} {what}: max|dx| = {ex:.3e} (bound {bound_x:.3e}), max rel |dldj| = {el:.3e} (bound 1e-9)')
        assert ex <= bound_x, (case, B, what, ex, bound_x)
        assert el <= 1e-9, (case, B, what, el)
        if layer.has_fixed_indices:
            fixed = layer._fixed_indices.long()
            assert torch.equal(xb[:, fixed], y[:, fixed])


# ------------------------------------------------------------------ 4. batch invariance

@pytest.mark.parametrize('case', ['rq8_desc', 'circ', 'mixed', 'fixed'])
def test_blocked_inverse_is_bitwise_batch_invariant(case):
    layer, D, dom = make_layer(case)
    y = _inputs(layer, D, dom, 257, seed=3)['in-domain']
    with torch.no_grad():
        xb, lb = layer.inverse(y)
        xb2, lb2 = layer.inverse(y)
        assert layer.last_inverse_route == 'blocked_f64'
        assert torch.equal(xb, xb2) and torch.equal(lb, lb2)
        for r in (0, 63, 64, 100, 256):
            x1, l1 = layer.inverse(y[r:r + 1].clone())
            assert torch.equal(x1[0], xb[r]) and torch.equal(l1[0], lb[r]), r


# ------------------------------------------------------------------ 5. autograd

def test_autograd_through_lazy_inverse_on_blocked_values():
    layer, D, dom = make_layer('rq8_asc')
    y0 = _inputs(layer, D, dom, 64, seed=9)['in-domain']
    grads = []
    for blocked in (True, False):
        layer.blocked_inverse = blocked
        layer.zero_grad(set_to_none=True)
        y = y0.clone().requires_grad_(True)
        x, ldj = layer.inverse(y)
        assert x.requires_grad and ldj.requires_grad
        assert layer.last_inverse_route == ('blocked_f64' if blocked else 'per_degree')
        (x.square().sum() + ldj.sum()).backward()
        grads.append([y.grad.clone()] + [p.grad.clone() for p in layer.parameters()])
    for gb, gp in zip(*grads):
        err = float((gb - gp).abs().max()) / max(float(gp.abs().max()), 1e-300)
        assert err <= 1e-9, err


# ------------------------------------------------------------------ 6. C ABI

def test_inverse_chain_f64_argument_checks():
    from tfep_amd import _lib
    lib = _lib.load()
    with pytest.raises(ValueError, match='descriptor is NULL'):
        _lib.call('tfep_inverse_chain_f64', None, None)

    buf = torch.zeros(4, 32, device='cuda', dtype=F64)
    tab = torch.zeros(64, device='cuda', dtype=torch.int32)

    def desc(**kw):
        d = _lib.InverseChainF64Desc()
        d.B, d.n_linears, d.n_steps, d.n_members, d.par_cols, d.max_feats = 1, 2, 1, 1, 2, 1
        d.y, d.ldy, d.x, d.ldx, d.log_det_J = buf.data_ptr(), 32, buf.data_ptr(), 32, buf.data_ptr()
        d.steps, d.feats = tab.data_ptr(), tab.data_ptr()
        for l in range(2):
            d.a[l], d.lda[l], d.w[l], d.ldw[l], d.bias[l] = buf.data_ptr(), 32, buf.data_ptr(), 32, buf.data_ptr()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d

    def call(d):
        _lib.call('tfep_inverse_chain_f64', ctypes.byref(d), _lib.stream_of(buf))

    call(desc(B=0, y=None, x=None, log_det_J=None))                        # an empty batch is a no-op, pointers unused
    call(desc(n_steps=0))
    for kw, msg in [(dict(B=-1), 'negative batch'), (dict(n_linears=1), 'n_linears'), (dict(n_linears=6), 'n_linears'),
                    (dict(n_members=5), 'n_members'), (dict(par_cols=0), 'parameter counts'), (dict(y=None), 'NULL pointer'),
                    (dict(steps=None), 'NULL pointer'), (dict(ldx=0), 'row strides'), (dict(a=(1, None)), 'NULL operand'),
                    (dict(w=(0, buf.data_ptr() + 4)), 'aligned'), (dict(k0=(1, 8)), 'multiple of 16'),
                    (dict(n_old=(0, 16)), 'n_old'), (dict(n_cols=(1, 40)), 'row strides of linear 1'),
                    (dict(lds_col0=(1, 3)), 'lds_col0'), (dict(has_panel=(1, 1)), 'zout'),
                    (dict(member_kind=(0, 2)), 'kind must be'), (dict(par_cols=1), 'par_cols >= 2')]:
        with pytest.raises(ValueError, match=msg):
            call(desc(**kw))
    # the state of one block must fit the LDS
    big = torch.zeros(1, 4096, device='cuda', dtype=F64)
    d = desc(n_cols=(0, 2000))
    d.a[0], d.lda[0], d.w[0], d.ldw[0] = big.data_ptr(), 4096, big.data_ptr(), 4096
    d.lds_col0[1] = 2000
    with pytest.raises(ValueError, match='LDS'):
        call(d)
    assert lib.tfep_inverse_chain_f64_lds_bytes(279, 25, 1) == (279 + 25 + 1) * 64 * 8
    assert lib.tfep_inverse_chain_f64_lds_bytes(-1, 25, 1) < 0


def test_empty_batch_through_the_blocked_route():
    layer, D, _ = make_layer('short')
    with torch.no_grad():
        x, ldj = layer.inverse(torch.empty(0, D, device='cuda', dtype=F64))
    assert layer.last_inverse_route == 'blocked_f64'
    assert tuple(x.shape) == (0, D) and tuple(ldj.shape) == (0,) and x.dtype == F64 and ldj.dtype == F64
