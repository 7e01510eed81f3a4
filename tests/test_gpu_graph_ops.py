"""``torch.ops.tfep.radial_expansion`` / ``segment_sum`` and the opt-in differentiable route of the radial modules and of
``unsorted_segment_sum`` (csrc/graph_ops.hip) against the plain reference of tests/graph_ops_ref.py: values and every
gradient of the three expansion kinds in float32 and float64 over sizes below one wave, ragged against a wave's 64 rows and a
workgroup's four waves, and large enough for hundreds of workspace rows; reproducibility bit for bit; the segment sum with
ids out of range and empty segments and its gather; a trainable message-passing toy end to end; the default route unchanged;
the error contract.

Bounds.  float64: relative L2 <= 1e-10 (segment sum: 1e-12).  float32 expansions: nothing fixed in advance -- the bound of a
tensor is 4 x the relative L2 error of the REFERENCE run in float32 on the same (rounded) inputs against its float64 run
(DESIGN section 4h).  float32 segment sum: rtol = atol = 1e-6 as tests/test_gpu_continuous.py; the data are below 0.25 and a
segment has at most 8 rows, so a partial sum stays below 2 and seven additions err by at most 7 x 2^-24 x 2 = 8.3e-7.  Every
figure is printed before it is asserted.
"""
import numpy as np
import pytest
import torch

import graph_ops_ref as gr
import tfep_amd.torch_ops  # noqa: F401  (registers torch.ops.tfep.*)
from tfep_amd import _lib
from tfep_amd.nn import graph
from tfep_amd.nn.embeddings import BehlerParrinelloRadialExpansion, GaussianBasisExpansion

pytestmark = pytest.mark.gpu

F32, F64 = gr.F32, gr.F64
TOL64 = 1e-10
dtypes = pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
KEYS = ('f', 'g_r', 'g_means', 'g_log_gammas')


def _dev(t, dtype, grad=False):
    return torch.as_tensor(t).detach().to('cuda', dtype).requires_grad_(grad)


def _np(t):
    return t.detach().cpu().numpy()


def _run(kind, n, K, dtype, rows=slice(None)):
    """Values and gradients of the op on (the rows ``rows`` of) a case, on the device."""
    r, means, lg, g = gr.case(n, K, dtype)
    r, means, lg, g = _dev(r[rows], dtype, True), _dev(means, dtype, True), _dev(lg, dtype, True), _dev(g[rows], dtype)
    f = torch.ops.tfep.radial_expansion(r, means, lg, gr.R_CUTOFF, *gr.switching(kind))
    return dict(zip(KEYS, (f, *torch.autograd.grad(f, (r, means, lg), g)))), r


# ------------------------------------------------------------------ values and gradients

@dtypes
@pytest.mark.parametrize('K', gr.KS)
@pytest.mark.parametrize('n', gr.NS)
@pytest.mark.parametrize('kind', gr.KINDS)
def test_expansion_matches_the_reference(kind, n, K, dtype):
    got, r = _run(kind, n, K, dtype)
    ref = gr.reference(kind, n, K, dtype)
    ref32 = gr.reference(kind, n, K, dtype, F32) if dtype == F32 else ref          # (the float64 bound does not use it)
    assert got['f'].shape == (n, K) and got['g_r'].shape == (n,) and got['g_means'].shape == got['g_log_gammas'].shape == (K,)
    for k in KEYS:
        assert got[k].dtype == dtype
        rel = gr.rel_l2(_np(got[k]), ref[k])
        own = gr.rel_l2(ref32[k], ref[k])
        bound = TOL64 if dtype == F64 else 4.0 * own
        print(f'{kind} n={n} K={K} {k} {dtype}: rel L2 {rel:.3e} (bound {bound:.3e}'
              + (f', ratio to the reference\'s float32 error {rel / own if own else float("nan"):.3f})' if dtype == F32 else ')'))
        assert rel <= bound, (k, rel, bound)
    if kind == 'bp_zero':
        beyond = r.detach() > gr.R_CUTOFF
        assert n == 1 or bool(beyond.any())
        assert bool((got['g_r'][beyond] == 0).all()) and bool((got['f'][beyond] == 0).all())


@dtypes
def test_expansion_keeps_the_shape_of_its_input(dtype):
    """Any shape of ``r``; a trailing axis of 1 is dropped by the modules only."""
    r, means, lg, _ = gr.case(63, 5, dtype)
    r, means, lg = _dev(r[:60].reshape(3, 4, 5), dtype, True), _dev(means, dtype), _dev(lg, dtype)
    f = torch.ops.tfep.radial_expansion(r, means, lg, gr.R_CUTOFF, True, False)
    assert f.shape == (3, 4, 5, 5)
    flat = torch.ops.tfep.radial_expansion(r.detach().reshape(-1), means, lg, gr.R_CUTOFF, True, False)
    assert torch.equal(f.detach().reshape(60, 5), flat)
    g_r, = torch.autograd.grad(f.sum(), r)
    assert g_r.shape == r.shape
    empty = torch.ops.tfep.radial_expansion(r.detach()[:0], means.requires_grad_(True), lg, gr.R_CUTOFF, True, False)
    assert empty.shape == (0, 4, 5, 5)
    g_means, = torch.autograd.grad(empty.sum(), means)
    assert bool((g_means == 0).all())


# ------------------------------------------------------------------ reproducibility

@dtypes
@pytest.mark.parametrize('K', [5, 64])
def test_parameter_gradients_are_reproducible_bit_for_bit(K, dtype):
    a, _ = _run('bp_zero', 70001, K, dtype)
    b, _ = _run('bp_zero', 70001, K, dtype)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


@dtypes
@pytest.mark.parametrize('K', [5, 64])
def test_distance_gradient_of_a_row_does_not_depend_on_the_batch(K, dtype):
    whole, _ = _run('bp', 70001, K, dtype)
    for rows in (slice(100, 3001), slice(69990, 70001), slice(64, 65)):
        part, _ = _run('bp', 70001, K, dtype, rows)
        assert torch.equal(part['g_r'], whole['g_r'][rows]), rows
        assert torch.equal(part['f'], whole['f'][rows]), rows


# ------------------------------------------------------------------ segment sum

def _segment_case(n_cols, dtype, n_rows=280):
    """Four rows per id, ids from -3 to 66 over 64 segments; segments 7 and 11 left empty (their rows go to 8 and 12)."""
    gen = torch.Generator().manual_seed(n_cols)
    ids = torch.arange(n_rows) % 70 - 3
    ids = torch.where(ids == 7, ids + 1, torch.where(ids == 11, ids + 1, ids))[torch.randperm(n_rows, generator=gen)]
    data = (0.5 * torch.rand(n_rows, n_cols, generator=gen, dtype=F64) - 0.25).to(dtype).to(F64)
    cot = torch.randn(64, n_cols, generator=gen, dtype=F64).to(dtype).to(F64)
    return data, ids, cot


def _assert_segment_sum_close(got, ref, dtype):
    got = _np(got).astype(np.float64)
    print(f'segment sum {dtype}: rel L2 {gr.rel_l2(got, ref):.3e}, max abs {np.abs(got - ref).max():.3e}')
    if dtype == F64:
        assert gr.rel_l2(got, ref) <= 1e-12
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    else:
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-6)


@dtypes
@pytest.mark.parametrize('n_cols', [1, 3, 64])
def test_segment_sum_op_and_its_gather(n_cols, dtype):
    data, ids, cot = _segment_case(n_cols, dtype)
    ref = gr.segment_sum(data, ids, 64)
    assert bool((ref[7] == 0).all() and (ref[11] == 0).all()) and int(((ids < 0) | (ids >= 64)).sum()) == 24
    x = _dev(data, dtype, True)
    out = torch.ops.tfep.segment_sum(x, ids.cuda(), 64)
    assert out.shape == (64, n_cols) and out.dtype == dtype
    _assert_segment_sum_close(out, ref.numpy(), dtype)
    assert bool((out[7] == 0).all() and (out[11] == 0).all())
    g, = torch.autograd.grad(out, x, _dev(cot, dtype))
    want = gr.segment_gather(cot, ids).to(dtype)
    assert g.dtype == dtype and torch.equal(g.cpu(), want)
    outside = (ids < 0) | (ids >= 64)
    assert bool((g.cpu()[outside] == 0).all())
    # through the public function, ids on the host as get_all_edges returns them
    assert torch.equal(graph.unsorted_segment_sum(x.detach(), ids, 64, differentiable=True)[[7, 11]], out.detach()[[7, 11]])


@dtypes
def test_segment_sum_past_one_grid_pass_and_with_unaligned_rows(dtype):
    """40 000 x 64: more elements (and 16-byte units) than one pass of the capped grid; then a cotangent that starts 4 or 8
    bytes into its block, which takes the element-wise gather."""
    gen = torch.Generator().manual_seed(5)
    n_rows, n_seg = 40000, 5000                                    # 8 rows per segment
    ids = (torch.arange(n_rows) % n_seg)[torch.randperm(n_rows, generator=gen)]
    data = (0.5 * torch.rand(n_rows, 64, generator=gen, dtype=F64) - 0.25).to(dtype).to(F64)
    x = _dev(data, dtype, True)
    out = torch.ops.tfep.segment_sum(x, ids.cuda(), n_seg)
    _assert_segment_sum_close(out, gr.segment_sum(data, ids, n_seg).numpy(), dtype)
    cot = torch.randn(n_seg * 64 + 1, generator=gen, dtype=F64).to(dtype).cuda()
    aligned, shifted = cot[:-1].reshape(n_seg, 64), cot[1:].reshape(n_seg, 64)
    assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    for c in (aligned, shifted):
        g, = torch.autograd.grad(out, x, c, retain_graph=True)
        assert torch.equal(g, c[ids.cuda()])


@dtypes
def test_segment_sum_of_an_empty_input_is_zero(dtype):
    x = torch.zeros(0, 3, device='cuda', dtype=dtype, requires_grad=True)
    out = torch.ops.tfep.segment_sum(x, torch.zeros(0, dtype=torch.int64, device='cuda'), 4)
    assert out.shape == (4, 3) and out.dtype == dtype and bool((out == 0).all())
    g, = torch.autograd.grad(out.sum(), x)
    assert g.shape == (0, 3)
    no_segments = torch.ops.tfep.segment_sum(torch.ones(5, 3, device='cuda', dtype=dtype),
                                             torch.zeros(5, dtype=torch.int64, device='cuda'), 0)
    assert no_segments.shape == (0, 3)


# ------------------------------------------------------------------ end to end

def test_a_message_passing_toy_trains_end_to_end():
    """2 samples x 5 nodes in float64: distances over all edges, a trainable Behler-Parrinello expansion, a linear layer and
    a segment sum over the source nodes.  Every gradient against the same network in torch on the CPU."""
    gen = torch.Generator().manual_seed(3)
    B, N, K, H, r_c = 2, 5, 6, 4, 1.25
    x0 = 0.6 * torch.randn(B * N, 3, generator=gen, dtype=F64)
    edges = graph.get_all_edges(B, N)
    w0, b0 = 0.5 * torch.randn(H, K, generator=gen, dtype=F64), 0.1 * torch.randn(H, generator=gen, dtype=F64)
    readout = torch.randn(B * N, H, generator=gen, dtype=F64)

    rbf = BehlerParrinelloRadialExpansion.from_range(r_c, K, r_c, trainable_means=True, trainable_stds=True).double().cuda()
    rbf.differentiable = True
    lin = torch.nn.Linear(K, H).double().cuda()
    with torch.no_grad():
        lin.weight.copy_(w0)
        lin.bias.copy_(b0)
    x = x0.cuda().requires_grad_(True)
    distances, _ = graph.compute_edge_distances(x, edges.cuda())
    messages = lin(rbf(distances))
    nodes = graph.unsorted_segment_sum(messages, edges[0], B * N, differentiable=True)
    loss = (torch.tanh(nodes) * readout.cuda()).sum()
    loss.backward()

    means = rbf._means.detach().cpu().clone().requires_grad_(True)
    lg = rbf._log_gammas.detach().cpu().clone().requires_grad_(True)
    xr, w, b = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    d_ref, _ = graph.compute_edge_distances(xr, edges)
    assert bool((d_ref > r_c).any()) and bool((d_ref < r_c).any())
    nodes_ref = gr.segment_sum(gr.expansion(d_ref, means, lg, 'bp_zero', r_c) @ w.t() + b, edges[0], B * N)
    loss_ref = (torch.tanh(nodes_ref) * readout).sum()
    loss_ref.backward()

    assert abs(loss.item() - loss_ref.item()) <= 1e-10 * abs(loss_ref.item())
    for name, got, ref in (('_means', rbf._means.grad, means.grad), ('_log_gammas', rbf._log_gammas.grad, lg.grad),
                           ('weight', lin.weight.grad, w.grad), ('bias', lin.bias.grad, b.grad), ('positions', x.grad, xr.grad)):
        assert got is not None, name
        rel = gr.rel_l2(_np(got), ref.numpy())
        print(f'toy {name}: rel L2 {rel:.3e}')
        assert got.dtype == F64 and rel <= TOL64, (name, rel)


# ------------------------------------------------------------------ the default route is unchanged

@pytest.mark.parametrize('kind', gr.KINDS)
def test_default_forward_is_cut_off_from_autograd_and_unchanged(kind):
    r = _dev(gr.case(257, 5, F32)[0], F32, True)
    if kind == 'gauss':
        module = GaussianBasisExpansion.from_range(5, 1.0, trainable_means=True, trainable_stds=True).cuda()
        cfg = (0.0, 0, 1)
    else:
        module = BehlerParrinelloRadialExpansion(gr.R_CUTOFF, torch.linspace(0, 1, 5), torch.full((5,), 0.3), True, True,
                                                 force_zero_after_cutoff=kind == 'bp_zero').cuda()
        cfg = (gr.R_CUTOFF, 1, int(kind == 'bp_zero'))
    assert torch.is_grad_enabled() and module.differentiable is False
    out = module(r)
    assert out.requires_grad is False and out.grad_fn is None and out.dtype == F32 and out.shape == (257, 5)
    out.cpu().numpy()                                              # (what the existing helper tests do in grad mode)
    direct = torch.empty(257, 5, dtype=F32, device='cuda')
    means, lg = module._means.detach().contiguous(), module._log_gammas.detach().contiguous()
    _lib.call('tfep_radial_expansion', _lib.ptr(r), 257, _lib.ptr(means), _lib.ptr(lg), 5, *cfg, _lib.ptr(direct),
              _lib.stream_of(r))
    assert torch.equal(out, direct)
    # the opt-in route runs the same float32 forward kernel: the same bits, now with a graph
    module.differentiable = True
    again = module(r)
    assert again.requires_grad and torch.equal(again.detach(), out)
    assert list(module.state_dict()) == ['_means', '_log_gammas']


def test_default_segment_sum_is_cut_off_from_autograd_and_unchanged():
    gen = torch.Generator().manual_seed(9)
    data = torch.randn(50, 3, generator=gen).cuda().requires_grad_(True)
    ids = torch.randperm(50, generator=gen)                          # one row per segment: no order of additions to differ
    out = graph.unsorted_segment_sum(data, ids, 50)
    assert out.requires_grad is False and out.dtype == F32
    direct = torch.empty(50, 3, dtype=F32, device='cuda')
    dev_ids = ids.cuda()
    _lib.call('tfep_segment_sum', _lib.ptr(data), _lib.ptr(dev_ids), 50, 3, 50, _lib.ptr(direct), _lib.stream_of(data))
    assert torch.equal(out, direct) and torch.equal(out[ids.cuda()], data.detach())
    assert torch.equal(graph.unsorted_segment_sum(data, ids, 50, differentiable=True).detach(), out)
    with pytest.raises(TypeError):
        graph.unsorted_segment_sum(data.detach().double(), ids, 50)                  # float64 is the opt-in route's


# ------------------------------------------------------------------ errors

def test_error_contract():
    r, means, lg, _ = (_dev(t, F32) for t in gr.case(63, 5, F32))
    ids = torch.arange(63, device='cuda') % 7
    for args in ((r.double(), means, lg), (r, means.double(), lg), (r, means, lg.double()), (r.half(), means, lg)):
        with pytest.raises(TypeError):
            torch.ops.tfep.radial_expansion(*args, 1.0, True, True)
    with pytest.raises(TypeError):
        torch.ops.tfep.segment_sum(torch.zeros(63, 2, device='cuda', dtype=torch.float16), ids, 7)
    with pytest.raises(TypeError):
        torch.ops.tfep.radial_expansion_backward(r, means, lg, torch.zeros(63, 5, device='cuda', dtype=F64), 1.0, True, True)
    with pytest.raises(ValueError):
        torch.ops.tfep.radial_expansion(r, means, lg[:4], 1.0, True, True)
    with pytest.raises(ValueError):
        torch.ops.tfep.radial_expansion(r, means, lg, 0.0, True, True)               # a switch needs a positive cutoff
    with pytest.raises(ValueError):
        torch.ops.tfep.segment_sum(r.reshape(-1, 1), ids[:5], 7)
    # a trainable parameter of another dtype than the data; fixed buffers are cast
    module = BehlerParrinelloRadialExpansion.from_range(1.0, 5, 1.0, trainable_means=True).cuda()
    module.differentiable = True
    with pytest.raises(TypeError, match='_means'):
        module(r.double())
    fixed = BehlerParrinelloRadialExpansion.from_range(1.0, 5, 1.0).cuda()
    fixed.differentiable = True
    assert fixed(r.double()).dtype == F64 and fixed(r).dtype == F32 and fixed(r.reshape(-1, 1)).shape == (63, 5)
    # CPU tensors: the package's error from the public surface, the dispatcher's from the ops
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        module(r.cpu())
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        graph.unsorted_segment_sum(r.cpu().reshape(-1, 1), ids.cpu(), 7, differentiable=True)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.tfep.radial_expansion(r.cpu(), means.cpu(), lg.cpu(), 1.0, True, True)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.tfep.segment_sum(r.cpu().reshape(-1, 1), ids.cpu(), 7)


@dtypes
def test_second_derivatives_raise(dtype):
    r, means, lg, _ = (_dev(t, dtype, True) for t in gr.case(63, 5, dtype))
    f = torch.ops.tfep.radial_expansion(r, means, lg, gr.R_CUTOFF, True, True)
    g_r, g_means = torch.autograd.grad((f ** 2).sum(), (r, means), create_graph=True)
    with pytest.raises(RuntimeError, match='differentiate twice'):
        (g_r.sum() + g_means.sum()).backward()
    data = torch.randn(63, 2, device='cuda', dtype=dtype, requires_grad=True)
    out = torch.ops.tfep.segment_sum(data, torch.arange(63, device='cuda') % 7, 7)
    g, = torch.autograd.grad((out ** 2).sum(), data, create_graph=True)
    with pytest.raises(RuntimeError, match='differentiate twice'):
        g.sum().backward()


@dtypes
def test_opcheck(dtype):
    r, means, lg, g = (_dev(t, dtype) for t in gr.case(63, 5, dtype))
    checks = ('test_schema', 'test_autograd_registration', 'test_faketensor')
    grad = [t.clone().requires_grad_(True) for t in (r, means, lg)]
    torch.library.opcheck(torch.ops.tfep.radial_expansion.default, (*grad, gr.R_CUTOFF, True, True), test_utils=checks)
    torch.library.opcheck(torch.ops.tfep.radial_expansion_backward.default, (r, means, lg, g, gr.R_CUTOFF, True, False),
                          test_utils=checks)
    ids = torch.arange(63, device='cuda') % 9 - 1
    torch.library.opcheck(torch.ops.tfep.segment_sum.default, (g.clone().requires_grad_(True), ids, 7), test_utils=checks)
    torch.library.opcheck(torch.ops.tfep.segment_gather.default, (g[:7].contiguous(), ids), test_utils=checks)
