"""GPU tests of the opt-in float64 blocked inverse for vector-valued transformers
(``AutoregressiveFlow.blocked_inverse_f64_vectors``, chain kernel ``tfep_inverse_chain_vec_f64``): symmetrized Moebius and
quaternion-product layers, alone and as members of a mixed transformer beside an RQ spline, against
tests/golden/blocked_f64_vectors.npz (``tools/gen_golden.py blocked_f64_vectors``) and the existing float64 goldens.

Bounds, none of them taken from what the kernels return:
* against the reference: those tests/test_gpu_quatprod.py applies to float64 flows -- values rtol 1e-9, atol 1e-10, log-det
  atol 1e-9 (rtol 1e-9); gradients 1e-9 of the tensor's largest entry (``max_err``), the loss rtol 1e-9;
* blocked against the pass per degree (flag off, same layer, same input): the float64 bound of
  tests/test_gpu_float64_inverse.py::test_blocked_matches_pass_per_degree -- x within 1e-10 max|x| + 1e-11, log-det within
  1e-9 max(1, |ldj|) per sample;
* round trip: ``close(..., 1e-9, 1e-9)`` of tests/test_gpu_float64_flows.py;
* a row alone against the same row inside a batch, and a graph replay against the eager call: ``torch.equal``.

Shapes: D = 24 with hidden width 40 (the later blocks have panel GEMMs and columns past the last multiple of 16); block
sizes 1, 2 and 16 put the vectors' degrees on block boundaries; B in {1, 63, 64, 65, 130}: the tail of the 64-row workgroup
and a second and third workgroup."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import test_gpu_quatprod as tq
import test_gpu_symmoebius as ts

pytestmark = pytest.mark.gpu
F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'blocked_f64_vectors.npz')
NAMES = ['sym3', 'quat', 'mixed']
#: the ``mixed`` flow: member indices and the ascending degrees (tools/gen_golden.py: BLOCKED_F64_MIXED_*)
MIXED_INDICES = [[0, 2, 3, 5, 6, 8, 9, 11], list(range(12, 20)), [1, 4, 7, 10, 20, 21, 22, 23]]
MIXED_DEGREES = [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 + [4] * 4 + [5] * 4 + [6, 7, 8, 9]


def _np(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64)


def max_err(got, ref):
    return float(np.abs(_np(got) - _np(ref)).max() / max(np.abs(_np(ref)).max(), 1e-300))


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(F64).cuda()


def load_golden_state(flow, g, name):
    sd = flow.state_dict()
    prefix = f'{name}/sd/'
    gold = {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}
    assert set(gold) == {k for k in sd if not k.endswith('.mask')}
    for k, v in gold.items():
        t = torch.from_numpy(np.asarray(v))
        assert t.shape == sd[k].shape and t.dtype == sd[k].dtype, k
        sd[k] = t
    flow.load_state_dict(sd, strict=True)


def build_flow(name, vectors=True):
    """The float64 tfep_amd twin of tools/gen_golden.py:blocked_f64_vector_flows()[name], weights from the golden."""
    from tfep_amd.nn.conditioners import generate_degrees as gd
    from tfep_amd.nn.flows import MAF, SequentialFlow
    from tfep_amd.nn.transformers import (MixedTransformer, NeuralSplineTransformer, QuaternionProductTransformer,
                                          SymmetrizedMoebiusTransformer)
    if name == 'sym3':
        make, degs = (lambda: SymmetrizedMoebiusTransformer(3)), [gd(24, o, repeats=3) for o in ('ascending', 'descending')]
    elif name == 'quat':
        make, degs = QuaternionProductTransformer, [gd(24, o, repeats=4) for o in ('ascending', 'descending')]
    else:
        def make():
            return MixedTransformer([SymmetrizedMoebiusTransformer(2), QuaternionProductTransformer(),
                                     NeuralSplineTransformer(torch.full((8,), -4.0), torch.full((8,), 4.0), 8)], MIXED_INDICES)
        asc = torch.tensor(MIXED_DEGREES)
        degs = [asc, 9 - asc]
    flow = SequentialFlow(*(MAF(d, transformer=make(), hidden_layers=[40, 40], initialize_identity=False) for d in degs))
    load_golden_state(flow, golden(), name)
    flow = flow.double().cuda()
    set_flag(flow, vectors)
    return flow


def set_flag(flow, on):
    for layer in flow:
        layer.blocked_inverse_f64_vectors = on


def routes(flow):
    return [layer.last_inverse_route for layer in flow]


def inputs(flow, B, seed):
    """``y = flow(x)`` of random x (inside the spline domain (-4, 4); no zero vector)."""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    x = 1.2 * torch.randn(B, 24, device='cuda', dtype=F64, generator=gen)
    with torch.no_grad():
        return x, flow(x)[0]


# ------------------------------------------------------------------ 1. the route

@pytest.mark.parametrize('name', NAMES)
def test_the_flag_selects_the_blocked_route(name):
    flow = build_flow(name)
    y = dev(golden()[f'{name}/x'])
    with torch.no_grad():
        flow.inverse(y)
        assert routes(flow) == ['blocked_f64', 'blocked_f64']
        for layer in flow:
            hp = layer._blocked_f64_host_plan()
            assert any(k >= 2 for k in hp['kinds']) and hp['feats'][:, 6].max() == max(t.dimension for t, k in
                                                                                        zip(hp['members'], hp['kinds']) if k >= 2)
        set_flag(flow, False)
        flow.inverse(y)
        assert routes(flow) == ['per_degree', 'per_degree']


def test_mixed_slot_order_interleaves_and_later_blocks_have_panels():
    flow = build_flow('mixed')
    hp = flow[0]._blocked_f64_host_plan()
    # degree 0: slots 0, 1, 2 = features 0 (vector component 0), 1 (spline), 2 (component 1)
    assert hp['feats'][:3, [0, 1, 6, 7]].tolist() == [[0, 0, 1, 2], [1, 2, 0, -1], [2, 0, 2, -1]]
    flow[0].inverse_block_f64 = 1
    hp = flow[0]._blocked_f64_host_plan()
    pairs = [(k0, n) for b in hp['blocks'] for k0, n in zip(b['k0'], b['n_old'])]
    assert len(hp['blocks']) == 10
    assert any(k0 >= 16 and n == 0 for k0, n in pairs) and any(k0 >= 16 and n > 0 for k0, n in pairs)
    assert any(k0 == 0 and n > 0 for k0, n in pairs)


def test_a_float32_layer_keeps_its_blocked_route():
    g = tq._golden()
    flow = tq.build_flow('quat', g)
    set_flag(flow, True)
    with torch.no_grad():
        flow.inverse(torch.from_numpy(g['quat/x']).cuda())
    assert routes(flow) == ['blocked', 'blocked']


@pytest.mark.parametrize('which', ['straddle', 'symmoebius_mixed'])
def test_vectors_that_straddle_degrees_keep_the_pass_per_degree(which):
    """One degree per feature: no vector lies inside one degree, so the layer keeps the reference's algorithm, flag or not,
    and still matches its golden."""
    if which == 'straddle':
        g, name = tq._golden(), 'straddle'
        flow = tq.build_flow(name, g).double()
    else:
        g, name = ts._golden(), 'mixed'
        flow = ts.build_flow(name, g).double()
    set_flag(flow, True)
    x = torch.from_numpy(g[f'{name}/x']).cuda().double()
    with torch.no_grad():
        xi, li = flow.inverse(x)
    assert routes(flow) == ['per_degree']
    np.testing.assert_allclose(_np(xi), g[f'{name}/y_inv_f64'], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(_np(li), g[f'{name}/ldj_inv_f64'], rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------ 2. values against the reference

@pytest.mark.parametrize('name', NAMES)
def test_inverse_against_the_reference(name):
    g = golden()
    flow = build_flow(name)
    with torch.no_grad():
        x, ldj = flow.inverse(dev(g[f'{name}/x']))
    assert routes(flow) == ['blocked_f64', 'blocked_f64'] and x.dtype == F64 and ldj.dtype == F64
    print(f'{name}: x max abs err {np.abs(_np(x) - g[f"{name}/y_inv"]).max():.3e}, '
          f'ldj max abs err {np.abs(_np(ldj) - g[f"{name}/ldj_inv"]).max():.3e}')
    np.testing.assert_allclose(_np(x), g[f'{name}/y_inv'], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(_np(ldj), g[f'{name}/ldj_inv'], rtol=1e-9, atol=1e-9)
    if name == 'quat':
        assert bool((ldj == 0).all())                                         # exactly zero


@pytest.mark.parametrize('which', ['quatprod', 'symmoebius'])
def test_existing_float64_goldens_on_the_blocked_route(which):
    if which == 'quatprod':
        g, name = tq._golden(), 'quat'
        flow = tq.build_flow(name, g).double()
    else:
        g, name = ts._golden(), 'flow'
        flow = ts.build_flow(name, g).double()
    set_flag(flow, True)
    with torch.no_grad():
        x, ldj = flow.inverse(torch.from_numpy(g[f'{name}/x']).cuda().double())
    assert routes(flow) == ['blocked_f64', 'blocked_f64']
    np.testing.assert_allclose(_np(x), g[f'{name}/y_inv_f64'], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(_np(ldj), g[f'{name}/ldj_inv_f64'], rtol=1e-9, atol=1e-9)
    if which == 'quatprod':
        assert bool((ldj == 0).all())


# ------------------------------------------------------------------ 3. blocked against the pass per degree

BATCHES = [1, 63, 64, 65, 130]


@pytest.mark.parametrize('block', [1, 2, 16])
@pytest.mark.parametrize('name', NAMES)
def test_blocked_matches_pass_per_degree_and_rows_do_not_depend_on_the_batch(name, block):
    flow = build_flow(name)
    for layer in flow:
        layer.inverse_block_f64 = block
        blocks = layer._blocked_f64_host_plan()['blocks']
        assert len(blocks) == -(-layer._inverse_masks.shape[0] // block)
    _, y_all = inputs(flow, max(BATCHES), seed=11)
    for li, layer in enumerate(flow):
        big = None
        for B in reversed(BATCHES):
            y = y_all[:B].clone()
            with torch.no_grad():
                layer.blocked_inverse_f64_vectors = True
                xb, lb = layer.inverse(y)
                assert layer.last_inverse_route == 'blocked_f64'
                layer.blocked_inverse_f64_vectors = False
                xp, lp = layer.inverse(y)
                assert layer.last_inverse_route == 'per_degree'
                layer.blocked_inverse_f64_vectors = True
            assert bool(torch.isfinite(xp).all()) and bool(torch.isfinite(lp).all())
            ex = float((xb - xp).abs().max())
            bound_x = 1e-10 * float(xp.abs().max()) + 1e-11
            el = float(((lb - lp).abs() / lp.abs().clamp(min=1.0)).max())
            print(f'{name} layer {li} block={block} B={B}: max|dx| = {ex:.3e} (bound {bound_x:.3e}), '
                  f'max rel |dldj| = {el:.3e} (bound 1e-9)')
            assert ex <= bound_x, (name, li, block, B, ex, bound_x)
            assert el <= 1e-9, (name, li, block, B, el)
            if name == 'quat':
                assert bool((lb == 0).all())
            if big is None:
                big = (xb, lb)
            else:                                   # the same rows inside the B = 130 batch, bit for bit
                assert torch.equal(xb, big[0][:B]) and torch.equal(lb, big[1][:B]), (name, li, block, B)
        with torch.no_grad():
            for r in (63, 64, 129):                 # a row alone: last of a workgroup, first of the next, the very last
                x1, l1 = layer.inverse(y_all[r:r + 1].clone())
                assert torch.equal(x1[0], big[0][r]) and torch.equal(l1[0], big[1][r]), (name, li, block, r)


# ------------------------------------------------------------------ 4. round trip

@pytest.mark.parametrize('name', NAMES)
def test_round_trip(name):
    flow = build_flow(name)
    x, y = inputs(flow, 65, seed=5)
    with torch.no_grad():
        _, l_f = flow(x)
        x1, l_i = flow.inverse(y)
    assert routes(flow) == ['blocked_f64', 'blocked_f64']
    print(f'{name}: round trip max |x - x\'| = {float((x1 - x).abs().max()):.3e}')
    np.testing.assert_allclose(_np(x1), _np(x), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(_np(l_f + l_i), np.zeros(65), rtol=0, atol=1e-8)      # (test_gpu_float64_inverse.py: log-dets cancel)


# ------------------------------------------------------------------ 5. gradients through the inverse

@pytest.mark.parametrize('name', NAMES)
def test_gradients_through_the_inverse_against_the_reference(name):
    from tfep_amd.loss import BoltzmannKLDivLoss
    g = golden()
    flow = build_flow(name)
    x = dev(g[f'{name}/x']).requires_grad_(True)
    c, d = dev(g[f'{name}/c']), dev(g[f'{name}/d'])
    y, ldj = flow.inverse(x)
    assert routes(flow) == ['blocked_f64', 'blocked_f64'] and y.requires_grad and ldj.requires_grad
    np.testing.assert_allclose(_np(y), g[f'{name}/y_inv'], rtol=1e-9, atol=1e-10)
    loss = BoltzmannKLDivLoss()((c * y ** 2 + d * y).sum(dim=1), ldj)
    loss.backward()
    np.testing.assert_allclose(float(loss.detach()), float(g[f'{name}/loss_inv']), rtol=1e-9)
    errs = {'gx': max_err(x.grad, g[f'{name}/gx_inv'])}
    for k, prm in flow.named_parameters():
        assert prm.grad is not None, k
        errs[k] = max_err(prm.grad, g[f'{name}/grad_inv/{k}'])
    print(f'{name}: largest gradient error {max(errs.values()):.3e} (bound 1e-9)')
    assert all(e <= 1e-9 for e in errs.values()), errs


# ------------------------------------------------------------------ 6. HIP graph

@pytest.mark.parametrize('name', NAMES)
def test_graph_replay_equals_eager(name):
    from tfep_amd.graphs import GraphedFlow
    flow = build_flow(name)
    _, y = inputs(flow, 64, seed=3)
    graph = GraphedFlow(flow, 64, 24, inverse=True)
    assert graph.static_in.dtype is F64
    for data in (y, 0.5 * y):
        with torch.no_grad():
            want = flow.inverse(data)
        assert routes(flow) == ['blocked_f64', 'blocked_f64']
        got = graph(data)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ------------------------------------------------------------------ 7. C ABI

def test_inverse_chain_vec_f64_argument_checks():
    """Every case is refused (or returns) before a launch: no kernel runs here."""
    from tfep_amd import _lib
    _lib.load()
    with pytest.raises(ValueError, match='descriptor is NULL'):
        _lib.call('tfep_inverse_chain_vec_f64', None, None)
    buf = torch.zeros(4, 32, device='cuda', dtype=F64)
    tab = torch.zeros(64, device='cuda', dtype=torch.int32)

    def desc(kind, dim, radius, **kw):
        v = _lib.InverseChainVecF64Desc()
        d = v.chain
        d.B, d.n_linears, d.n_steps, d.n_members, d.par_cols, d.max_feats = 1, 2, 1, 1, 2, 1
        d.y, d.ldy, d.x, d.ldx, d.log_det_J = buf.data_ptr(), 32, buf.data_ptr(), 32, buf.data_ptr()
        d.steps, d.feats = tab.data_ptr(), tab.data_ptr()
        for l in range(2):
            d.a[l], d.lda[l], d.w[l], d.ldw[l], d.bias[l] = buf.data_ptr(), 32, buf.data_ptr(), 32, buf.data_ptr()
        d.member_kind[0], v.member_dim[0], v.member_max_radius[0] = kind, dim, radius
        for k, val in kw.items():
            setattr(d, k, val)
        return v

    def call(v):
        _lib.call('tfep_inverse_chain_vec_f64', ctypes.byref(v), _lib.stream_of(buf))

    call(desc(3, 4, 0.0, B=0, y=None, x=None, log_det_J=None))               # an empty batch is a no-op, pointers unused
    call(desc(2, 3, 0.99, n_steps=0))
    for args, msg in [((4, 4, 0.5), 'kind must be'), ((-1, 4, 0.5), 'kind must be'), ((3, 3, 0.5), 'must be 4'),
                      ((3, 0, 0.5), 'must be 4'), ((2, 1, 0.5), 'must be in 2..8'), ((2, 9, 0.5), 'must be in 2..8'),
                      ((2, 3, 0.0), 'max_radius'), ((2, 3, 1.0), 'max_radius'), ((2, 3, float('nan')), 'max_radius')]:
        with pytest.raises(ValueError, match=msg):
            call(desc(*args))
    # the checks of tfep_inverse_chain_f64 apply
    for kw, msg in [(dict(B=-1), 'negative batch'), (dict(n_linears=6), 'n_linears'), (dict(n_members=5), 'n_members'),
                    (dict(y=None), 'NULL pointer'), (dict(ldx=0), 'row strides')]:
        with pytest.raises(ValueError, match=msg):
            call(desc(3, 4, 0.0, **kw))
    with pytest.raises(ValueError, match='par_cols >= 2'):
        call(desc(0, 0, 0.0, par_cols=1))
    # the scalar entry point still refuses the vector kinds
    with pytest.raises(ValueError, match='kind must be'):
        _lib.call('tfep_inverse_chain_f64', ctypes.byref(desc(2, 3, 0.5).chain), _lib.stream_of(buf))
