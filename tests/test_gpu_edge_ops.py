"""``torch.ops.tfep.edge_geometry`` / ``edge_prune`` and the opt-in routes of ``compute_edge_distances`` and
``prune_long_edges`` (csrc/edge_ops.hip) against the plain reference of tests/edge_ops_ref.py: values and the position gradient
for both dtypes and all four flag settings over edge counts below, at and above a wave, ragged against a workgroup and past one
grid pass; one cotangent alone; reproducibility bit for bit and independence of the batch; a strided ``x``; an edge of length
zero; the compaction against the boolean-mask route at every tile boundary, with its gradients; a message-passing toy end to
end; refusals.

Bounds.  float64: relative L2 <= 1e-10 on distances, directions and the gradient.  float32: nothing fixed in advance -- the
bound of a tensor is 4 x the relative L2 error of the torch route run in float32 on the same (rounded) inputs against the
float64 reference.  The pruned tensors and their gradients: ``torch.equal`` to the default route's.  Every
figure is printed before it is asserted.
"""
import pytest
import torch

import edge_ops_ref as er
import graph_ops_ref as gr
import tfep_amd.torch_ops  # noqa: F401  (registers torch.ops.tfep.*)
from tfep_amd import _lib
from tfep_amd.nn import graph
from tfep_amd.nn.embeddings import BehlerParrinelloRadialExpansion

pytestmark = pytest.mark.gpu

F32, F64 = er.F32, er.F64
TOL64 = 1e-10
dtypes = pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
flags = pytest.mark.parametrize('normalize,inverse', er.FLAGS)
KEYS = ('distances', 'directions', 'gx')


def _dev(t, dtype=None, grad=False):
    t = torch.as_tensor(t).detach().to('cuda') if dtype is None else torch.as_tensor(t).detach().to('cuda', dtype)
    return t.requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


def _run(x, edges, g_r, g_d, normalize, inverse):
    """Values and the position gradient of the public route on device tensors; a ``None`` cotangent is left out."""
    x = x.detach().requires_grad_(True)
    r, d = graph.compute_edge_distances(x, edges, normalize, inverse, differentiable=True)
    outputs, cots = zip(*[(o, c) for o, c in ((r, g_r), (d, g_d)) if c is not None])
    gx, = torch.autograd.grad(outputs, x, cots)
    return dict(zip(KEYS, (r.detach(), d.detach(), gx)))


def _case(n_edges, n_nodes, dtype):
    x, edges, g_r, g_d = er.case(n_edges, n_nodes, dtype)
    return _dev(x, dtype), _dev(edges), _dev(g_r, dtype), _dev(g_d, dtype)


# ------------------------------------------------------------------ values and gradients

@dtypes
@flags
@pytest.mark.parametrize('n_nodes', er.NS)
@pytest.mark.parametrize('n_edges', er.ES)
def test_geometry_matches_the_reference(n_edges, n_nodes, normalize, inverse, dtype):
    got = _run(*_case(n_edges, n_nodes, dtype), normalize, inverse)
    ref = er.reference(n_edges, n_nodes, dtype, normalize, inverse)
    ref32 = er.reference(n_edges, n_nodes, dtype, normalize, inverse, F32) if dtype == F32 else ref
    assert float(ref['distances'].min()) > er.MIN_LENGTH
    assert got['distances'].shape == (n_edges,) and got['directions'].shape == (n_edges, 3) and got['gx'].shape == (n_nodes, 3)
    for k in KEYS:
        assert got[k].dtype == dtype
        rel = er.rel_l2(_np(got[k]), ref[k])
        own = er.rel_l2(ref32[k], ref[k])
        bound = TOL64 if dtype == F64 else 4.0 * own
        print(f'E={n_edges} N={n_nodes} normalize={normalize} inverse={inverse} {k} {dtype}: rel L2 {rel:.3e} (bound {bound:.3e}'
              + (f', ratio to the torch route\'s float32 error {rel / own if own else float("nan"):.3f})' if dtype == F32 else ')'))
        assert rel <= bound, (k, rel, bound)
    if n_nodes == 65:                                                   # nodes 3 and 64 have no edge: their rows are written, zero
        assert bool((got['gx'][[3, 64]] == 0).all())


@dtypes
def test_more_nodes_than_one_grid_pass(dtype):
    """The backward runs one lane per node: 524289 nodes take a second pass of its grid.  The edges of the 257-edge case
    spread over the whole range, the last node included."""
    n_nodes = er.GRID_PASS + 1
    x, edges, g_r, g_d = er.case(257, 65, dtype)
    gen = torch.Generator().manual_seed(17)
    big = torch.randn(n_nodes, 3, generator=gen, dtype=F64).to(dtype).to(F64)
    where = torch.arange(65) * (n_nodes // 65)
    where[5] = n_nodes - 1                                              # (node 5 has edges; nodes 3 and 64 have none)
    big[where] = x
    big_edges = where[edges]
    got = _run(_dev(big, dtype), _dev(big_edges), _dev(g_r, dtype), _dev(g_d, dtype), True, False)
    want = er.geometry_vjp(big, big_edges, g_r, g_d, True, False)
    rel = er.rel_l2(_np(got['gx']), want.numpy())
    small = er.reference(257, 65, dtype, True, False)
    bound = TOL64 if dtype == F64 else 4.0 * er.rel_l2(er.reference(257, 65, dtype, True, False, F32)['gx'], small['gx'])
    print(f'N={n_nodes} gx {dtype}: rel L2 {rel:.3e} (bound {bound:.3e})')
    assert rel <= bound
    touched = torch.zeros(n_nodes, dtype=torch.bool)
    touched[big_edges.reshape(-1)] = True
    assert bool(touched[-1]) and bool((got['gx'].cpu()[~touched] == 0).all())


# ------------------------------------------------------------------ one cotangent alone

@dtypes
@flags
def test_a_missing_cotangent_is_a_zero(normalize, inverse, dtype):
    x, edges, g_r, g_d = _case(257, 65, dtype)
    only_r = _run(x, edges, g_r, None, normalize, inverse)['gx']
    only_d = _run(x, edges, None, g_d, normalize, inverse)['gx']
    assert torch.equal(only_r, _run(x, edges, g_r, torch.zeros_like(g_d), normalize, inverse)['gx'])
    assert torch.equal(only_d, _run(x, edges, torch.zeros_like(g_r), g_d, normalize, inverse)['gx'])
    assert bool((only_r != only_d).any())
    # the op itself, with None for either
    assert torch.equal(torch.ops.tfep.edge_geometry_backward(x, edges, g_r, None, normalize, inverse), only_r)
    assert torch.equal(torch.ops.tfep.edge_geometry_backward(x, edges, None, g_d, normalize, inverse), only_d)
    if dtype == F64:
        ref = er.geometry_vjp(x.cpu(), edges.cpu(), None, g_d.cpu(), normalize, inverse)
        assert er.rel_l2(_np(only_d), ref.numpy()) <= TOL64


# ------------------------------------------------------------------ reproducibility

@dtypes
@flags
def test_gradient_is_reproducible_and_independent_of_the_batch(normalize, inverse, dtype):
    n_nodes, n_edges, batch = 65, 257, 7
    x, edges, g_r, g_d = _case(n_edges, n_nodes, dtype)
    alone = _run(x, edges, g_r, g_d, normalize, inverse)
    again = _run(x, edges.clone(), g_r, g_d, normalize, inverse)       # (a clone: the incidence list is built anew)
    for k in KEYS:
        assert torch.equal(alone[k], again[k]), k
    # the sample as number 4 of 7, the edges offset accordingly
    others = [_dev(er.positions(n_nodes, dtype, seed=s + 1), dtype) for s in range(batch)]
    others[4] = x
    xb = torch.cat(others)
    eb = torch.cat([edges + s * n_nodes for s in range(batch)], dim=1)
    whole = _run(xb, eb, g_r.repeat(batch), g_d.repeat(batch, 1), normalize, inverse)
    rows, cols = slice(4 * n_nodes, 5 * n_nodes), slice(4 * n_edges, 5 * n_edges)
    assert torch.equal(whole['gx'][rows], alone['gx'])
    assert torch.equal(whole['distances'][cols], alone['distances']) and torch.equal(whole['directions'][cols], alone['directions'])
    assert not torch.equal(whole['gx'][:n_nodes], alone['gx'])


# ------------------------------------------------------------------ row stride

@dtypes
def test_a_strided_x_gives_the_same_bits(dtype):
    x, edges, g_r, g_d = _case(257, 65, dtype)
    wide = torch.randn(65, 6, device='cuda', dtype=dtype)
    wide[:, 1:4] = x
    view = wide[:, 1:4]
    assert view.stride() == (6, 1) and not view.is_contiguous()
    for normalize, inverse in er.FLAGS:
        a, b = _run(view, edges, g_r, g_d, normalize, inverse), _run(x, edges, g_r, g_d, normalize, inverse)
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k
    # through the view's own graph: the gradient reaches the wide tensor's columns 1..3 only
    wide.requires_grad_(True)
    r, _ = graph.compute_edge_distances(wide[:, 1:4], edges, differentiable=True)
    r.sum().backward()
    assert bool((wide.grad[:, [0, 4, 5]] == 0).all()) and bool((wide.grad[:, 1:4] != 0).any())


# ------------------------------------------------------------------ zero length

@dtypes
@pytest.mark.parametrize('normalize', [False, True])
def test_an_edge_of_length_zero(normalize, dtype):
    x, edges, g_r, g_d = er.case(65, 65, dtype)
    x, edges = x.clone(), edges.clone()
    x[64] = x[3]                                                        # nodes 3 and 64 have no other edge
    edges[:, 30] = torch.tensor([3, 64])
    got = _run(_dev(x, dtype), _dev(edges), _dev(g_r, dtype), _dev(g_d, dtype), normalize, False)
    assert float(got['distances'][30]) == 0.0
    valid = torch.arange(65, device='cuda') != 30
    assert bool(got['distances'][valid].isfinite().all()) and bool(got['directions'][valid].isfinite().all())
    if normalize:
        assert bool(got['directions'][30].isnan().all())
    else:
        assert bool((got['directions'][30] == 0).all())
    nan_rows = got['gx'].isnan().all(1)
    assert nan_rows.nonzero().reshape(-1).tolist() == [3, 64]
    others = torch.ones(65, dtype=torch.bool, device='cuda')
    others[[3, 64]] = False
    assert bool(got['gx'][others].isfinite().all())
    # the finite rows have the bits of the list without the edge: the other nodes' lists keep their order
    keep = valid.cpu()
    without = _run(_dev(x, dtype), _dev(edges[:, keep]), _dev(g_r[keep], dtype), _dev(g_d[keep], dtype), normalize, False)
    assert torch.equal(got['gx'][others], without['gx'][others]) and bool((without['gx'][[3, 64]] == 0).all())


# ------------------------------------------------------------------ pruning

def _prune_case(n_edges, dtype):
    gen = torch.Generator().manual_seed(n_edges)
    distances = (0.5 + torch.rand(n_edges, generator=gen, dtype=F64)).to(dtype)           # [0.5, 1.5)
    edges = torch.randint(0, 1000, (2, n_edges), generator=gen)
    return edges.cuda(), distances.cuda(), torch.randn(n_edges, 3, generator=gen).cuda(), \
        torch.randn(n_edges, 5, generator=gen, dtype=F64).cuda()


@dtypes
@pytest.mark.parametrize('which', ['all kept', 'none kept', 'one NaN', 'cutoff on a distance', 'median'])
@pytest.mark.parametrize('n_edges', er.PRUNE_ES)
def test_pruning_equals_the_default_route(n_edges, which, dtype):
    edges, distances, a3, a5 = _prune_case(n_edges, dtype)
    cutoff = {'all kept': 2.0, 'none kept': 0.25, 'one NaN': 2.0}.get(which)
    if which == 'one NaN' and n_edges:
        distances[n_edges // 2] = float('nan')
    if which == 'cutoff on a distance':
        cutoff = float(distances[(2 * n_edges) // 3]) if n_edges else 1.0                  # that edge stays: <=
    if which == 'median':
        cutoff = float(distances.median()) if n_edges else 1.0
    leaves = [t.clone().requires_grad_(True) for t in (distances, a3, a5)]
    twins = [t.clone().requires_grad_(True) for t in (distances, a3, a5)]
    want = graph.prune_long_edges(cutoff, edges, *leaves)
    got = graph.prune_long_edges(cutoff, edges, *twins, kernel=True)
    n_kept = want[1].shape[0]
    print(f'E={n_edges} {which} {dtype}: cutoff {cutoff}, {n_kept} kept')
    assert n_kept == {'all kept': n_edges, 'none kept': 0, 'one NaN': max(n_edges - 1, 0)}.get(which, n_kept)
    if which == 'cutoff on a distance' and n_edges:
        assert bool((want[1] == cutoff).any())
    if which == 'median' and n_edges > 1:
        assert 0 < n_kept < n_edges
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w)
    assert got[0].is_contiguous() and torch.equal(torch.ops.tfep.edge_prune(distances, cutoff),
                                                  er.keep_index(distances.cpu(), cutoff).cuda())
    # gradients through the pruned distances and arguments
    cots = [torch.randn_like(t) for t in want[1:]]
    grads_want = torch.autograd.grad(want[1:], leaves, cots)
    grads_got = torch.autograd.grad(got[1:], twins, cots)
    for g, w in zip(grads_got, grads_want):
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w)


def test_pruning_past_one_grid_pass_of_tiles():
    """The compaction kernels run 2048 workgroups of one 256-edge tile each: 2048 * 256 + 1 edges put a second tile on the
    first workgroup and more than one count on a lane of the scan."""
    n_edges = er.GRID_PASS + 1
    gen = torch.Generator(device='cuda').manual_seed(3)
    distances = torch.rand(n_edges, device='cuda', generator=gen)
    keep = torch.ops.tfep.edge_prune(distances, 0.37)
    assert torch.equal(keep, torch.nonzero(distances <= 0.37).reshape(-1))
    assert torch.equal(torch.ops.tfep.edge_prune(distances.double(), 0.37), torch.nonzero(distances.double() <= 0.37).reshape(-1))


# ------------------------------------------------------------------ end to end

def test_a_message_passing_toy_end_to_end():
    """3 samples x 9 nodes in float64: edge geometry, pruning, a trainable Behler-Parrinello expansion, messages that use the
    unit vectors, and a segment sum over the source nodes -- all on the kernels.  Value and gradients against the same
    composition in torch on the CPU."""
    gen = torch.Generator().manual_seed(5)
    B, N, K, H, r_c, r_prune = 3, 9, 6, 4, 1.5, 1.2
    x0 = 0.7 * torch.randn(B * N, 3, generator=gen, dtype=F64)
    edges = graph.get_all_edges(B, N)
    w0, b0 = 0.5 * torch.randn(H, K, generator=gen, dtype=F64), 0.1 * torch.randn(H, generator=gen, dtype=F64)
    v0 = torch.randn(3, H, generator=gen, dtype=F64)
    readout = torch.randn(B * N, H, generator=gen, dtype=F64)

    rbf = BehlerParrinelloRadialExpansion.from_range(r_c, K, r_c, trainable_means=True, trainable_stds=True).double().cuda()
    rbf.differentiable = True
    w, b, v = (t.cuda().requires_grad_(True) for t in (w0, b0, v0))
    x = x0.cuda().requires_grad_(True)
    dev_edges = edges.cuda()
    distances, directions = graph.compute_edge_distances(x, dev_edges, normalize_directions=True, differentiable=True)
    kept_edges, kept_distances, kept_directions = graph.prune_long_edges(r_prune, dev_edges, distances, directions, kernel=True)
    messages = (rbf(kept_distances) @ w.t() + b) * torch.tanh(kept_directions @ v)
    nodes = graph.unsorted_segment_sum(messages, kept_edges[0], B * N, differentiable=True)
    loss = (torch.tanh(nodes) * readout.cuda()).sum()
    loss.backward()

    means = rbf._means.detach().cpu().clone().requires_grad_(True)
    lg = rbf._log_gammas.detach().cpu().clone().requires_grad_(True)
    xr, wr, br, vr = (t.clone().requires_grad_(True) for t in (x0, w0, b0, v0))
    d_ref, u_ref = er.geometry(xr, edges, True)
    e_ref, d_ref, u_ref = er.prune(r_prune, edges, d_ref, u_ref)
    assert 0 < e_ref.shape[1] < edges.shape[1] and torch.equal(kept_edges.cpu(), e_ref)
    m_ref = (gr.expansion(d_ref, means, lg, 'bp_zero', r_c) @ wr.t() + br) * torch.tanh(u_ref @ vr)
    loss_ref = (torch.tanh(gr.segment_sum(m_ref, e_ref[0], B * N)) * readout).sum()
    loss_ref.backward()

    print(f'toy: {e_ref.shape[1]} of {edges.shape[1]} edges kept, loss {loss.item():.12e} against {loss_ref.item():.12e}')
    assert abs(loss.item() - loss_ref.item()) <= TOL64 * abs(loss_ref.item())
    for name, got, ref in (('positions', x.grad, xr.grad), ('_means', rbf._means.grad, means.grad),
                           ('_log_gammas', rbf._log_gammas.grad, lg.grad), ('weight', w.grad, wr.grad), ('bias', b.grad, br.grad),
                           ('direction weight', v.grad, vr.grad)):
        assert got is not None, name
        rel = er.rel_l2(_np(got), ref.numpy())
        print(f'toy {name}: rel L2 {rel:.3e}')
        assert got.dtype == F64 and rel <= TOL64, (name, rel)


# ------------------------------------------------------------------ refusals and limits

@dtypes
def test_an_empty_batch(dtype):
    x = torch.randn(4, 3, device='cuda', dtype=dtype, requires_grad=True)
    edges = torch.empty(2, 0, dtype=torch.int64, device='cuda')
    r, d = graph.compute_edge_distances(x, edges, True, differentiable=True)
    assert r.shape == (0,) and d.shape == (0, 3) and r.dtype == d.dtype == dtype
    gx, = torch.autograd.grad(r.sum() + d.sum(), x)
    assert gx.shape == (4, 3) and gx.dtype == dtype and bool((gx == 0).all())
    pruned = graph.prune_long_edges(1.0, edges, r.detach(), d.detach(), kernel=True)
    assert [tuple(t.shape) for t in pruned] == [(2, 0), (0,), (0, 3)]
    assert pruned[0].dtype == torch.int64 and pruned[1].dtype == pruned[2].dtype == dtype
    no_nodes = graph.compute_edge_distances(x.detach()[:0], graph.get_all_edges(2, 1).cuda(), differentiable=True)
    assert no_nodes[0].shape == (0,) and no_nodes[0].dtype == dtype


def test_refusals():
    x, edges, g_r, g_d = _case(63, 65, F32)
    with pytest.raises(TypeError):
        torch.ops.tfep.edge_geometry(x.half(), edges, False, False)
    with pytest.raises(TypeError):
        torch.ops.tfep.edge_geometry_backward(x, edges, g_r.double(), g_d, False, False)
    with pytest.raises(TypeError):
        torch.ops.tfep.edge_geometry_backward(x.double(), edges, g_r.double(), g_d, False, False)
    r, d = graph.compute_edge_distances(x, edges, differentiable=True)
    with pytest.raises(TypeError):
        graph.prune_long_edges(1.0, edges, r, d.half(), kernel=True)
    with pytest.raises(TypeError):
        graph.prune_long_edges(1.0, edges, r, torch.arange(63, device='cuda'), kernel=True)
    with pytest.raises(TypeError):
        torch.ops.tfep.edge_prune(r.half(), 1.0)
    # shapes and indices: the host's ValueError, before any launch
    for bad in (edges[:1], edges.t(), edges.reshape(2, 63, 1)):
        with pytest.raises(ValueError):
            graph.compute_edge_distances(x, bad.contiguous(), differentiable=True)
    for value in (-1, 65):
        bad = edges.clone()
        bad[1, 7] = value
        with pytest.raises(ValueError, match='outside'):
            graph.compute_edge_distances(x, bad, differentiable=True)
    with pytest.raises(ValueError):
        graph.compute_edge_distances(x[:, :2], edges, differentiable=True)
    with pytest.raises(ValueError):
        torch.ops.tfep.edge_geometry_backward(x, edges, g_r[:5], g_d, False, False)
    with pytest.raises(ValueError):
        graph.prune_long_edges(1.0, edges, r, d[:5], kernel=True)
    with pytest.raises(ValueError):
        graph.prune_long_edges(1.0, edges[:, :5], r, kernel=True)
    # CPU tensors: the package's error from the public surface, the dispatcher's from the ops
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        graph.compute_edge_distances(x.cpu(), edges.cpu(), differentiable=True)
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        graph.prune_long_edges(1.0, edges.cpu(), r.detach().cpu(), kernel=True)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.tfep.edge_prune(r.detach().cpu(), 1.0)
    # edges on the host are moved, as unsorted_segment_sum moves its ids
    moved = graph.compute_edge_distances(x, edges.cpu(), differentiable=True)
    assert torch.equal(moved[0], r)


@dtypes
def test_second_derivatives_raise(dtype):
    x, edges, _, _ = _case(63, 65, dtype)
    x = x.requires_grad_(True)
    r, d = torch.ops.tfep.edge_geometry(x, edges, True, False)
    gx, = torch.autograd.grad((r ** 2).sum() + (d ** 2).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match='differentiate twice'):
        gx.sum().backward()
    leaf = r.detach().requires_grad_(True)
    kept = torch.ops.tfep.edge_select(leaf, torch.arange(0, 63, 2, device='cuda'))
    g, = torch.autograd.grad((kept ** 2).sum(), leaf, create_graph=True)
    with pytest.raises(RuntimeError, match='differentiate twice'):
        g.sum().backward()


@dtypes
def test_opcheck(dtype):
    x, edges, g_r, g_d = _case(63, 65, dtype)
    checks = ('test_schema', 'test_autograd_registration', 'test_faketensor')
    torch.library.opcheck(torch.ops.tfep.edge_geometry.default, (x.clone().requires_grad_(True), edges, True, False),
                          test_utils=checks)
    torch.library.opcheck(torch.ops.tfep.edge_geometry_backward.default, (x, edges, g_r, None, False, True), test_utils=checks)
    # (the fake kernel of edge_prune returns an unbacked size: tests/test_edge_ops_host.py runs it under FakeTensorMode)
    torch.library.opcheck(torch.ops.tfep.edge_prune.default, (g_r, 0.1), test_utils=checks[:2])
    keep = torch.arange(0, 63, 3, device='cuda')
    torch.library.opcheck(torch.ops.tfep.edge_select.default, (g_d.clone().requires_grad_(True), keep), test_utils=checks)
