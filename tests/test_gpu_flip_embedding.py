"""GPU tests of FlipInvariantEmbedding on its HIP kernels (csrc/flipembed.hip), float32 and float64: the module against the
reference in float64 (tests/golden/flipembed.npz at the shapes where a kernel can go wrong, tests/golden/embeddings.npz for
the configurations of the existing module tests), its gradients, bitwise flip invariance, determinism, the torch fallback,
MAF layers with this embedding in float64, and the registered ops.

Tolerances are the project's own: float32 rel L2 < 2e-6 on outputs (test_gpu_embeddings.py), 1e-4 rel L2 on gx and 3e-4 per
entry on parameter gradients (test_embedded_flow_gradients); float64 rtol 1e-9 / atol 1e-10 on outputs and 1e-9 of the
largest entry on gradients (test_gpu_float64_flows.py)."""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = [F32, F64]
ZERO_GRADIENT = 'weight_layer.2.bias'         # softmax over the pair is shift invariant: analytically zero


def flip_configs():
    """The configurations of tests/golden/flipembed.npz (tools/gen_golden.py::flipembed_configs)."""
    return {
        'q257': dict(n_features_in=4, embedding_dimension=3, hidden_layer_width=32),
        'strided': dict(n_features_in=14, embedding_dimension=5, vector_dimension=4, hidden_layer_width=16,
                        embedded_indices=[2, 3, 4, 5, 8, 9, 10, 11, 13, 0, 1, 6]),
        'max': dict(n_features_in=16, embedding_dimension=32, vector_dimension=8, hidden_layer_width=64),
        'min': dict(n_features_in=3, embedding_dimension=1, vector_dimension=1, hidden_layer_width=1),
    }


@functools.lru_cache(maxsize=None)
def golden(name):
    return gu.load(name)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def check_output(out, ref, dtype, what=''):
    assert out.dtype == dtype
    got = out.detach().cpu().numpy().astype(np.float64)
    print(what, 'rel L2', rel(got, ref), 'max abs', np.abs(got - ref).max())
    if dtype == F64:
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-10, err_msg=what)
    else:
        assert rel(got, ref) < 2e-6, what


def check_gradients(gx, grads, ref_gx, ref_grads, dtype):
    """``grads`` / ``ref_grads``: name -> gradient.  The analytically zero gradient is asserted to be exactly zero: its
    reference value is the rounding noise of autograd's sum (~1e-16), nothing to compare to."""
    gx = gx.detach().cpu().numpy().astype(np.float64)
    gmax = max(np.abs(r).max() for r in ref_grads.values())
    for k, ref in ref_grads.items():
        got = grads[k].detach().cpu().numpy().astype(np.float64)
        assert got.shape == ref.shape and grads[k].dtype == dtype, k
        if k.endswith(ZERO_GRADIENT):
            assert not got.any(), (k, got)
            assert np.abs(ref).max() <= 1e-12 * gmax, k
            continue
        if dtype == F64:
            err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)
            print(k, 'max err / max', err)
            assert err <= 1e-9, (k, err)
        else:
            err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-4 * gmax)
            print(k, 'max err / scale', err)
            assert err < 3e-4, (k, err)
    if dtype == F64:
        err = np.abs(gx - ref_gx).max() / max(np.abs(ref_gx).max(), 1e-300)
        print('gx max err / max', err)
        assert err <= 1e-9, err
    else:
        print('gx rel L2', rel(gx, ref_gx))
        assert rel(gx, ref_gx) < 1e-4


def build_flip(name, dtype):
    from tfep_amd.nn.embeddings import FlipInvariantEmbedding
    g = golden('flipembed.npz')
    emb = FlipInvariantEmbedding(**flip_configs()[name])
    emb.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in gu.sub(g, f'{name}/sd/').items()})
    return emb.to(dtype).cuda(), torch.from_numpy(g[f'{name}/x']).to(dtype).cuda(), g


def flip_members(module):
    from tfep_amd.nn.embeddings import FlipInvariantEmbedding
    return [m for m in module.modules() if isinstance(m, FlipInvariantEmbedding)]


def cosine_weights(out):
    """c[b, j] = cos(b + 2 j), formed in float64 like the golden's (a float32 cosine is 3e-8 off: more than the float64
    gradient bound) and rounded to the dtype of ``out``."""
    rows = torch.arange(out.shape[0], device='cuda', dtype=F64).unsqueeze(1)
    cols = torch.arange(out.shape[1], device='cuda', dtype=F64).unsqueeze(0)
    return torch.cos(rows + 2.0 * cols).to(out.dtype)


# ------------------------------------------------------------------ 1. parity of the module

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(flip_configs()))
def test_module_parity(name, dtype):
    emb, x, g = build_flip(name, dtype)
    with torch.no_grad():
        out = emb(x)
    assert emb.last_route == 'kernel'
    check_output(out, g[f'{name}/out'], dtype, name)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(gu.embedding_configs()))
def test_module_parity_on_the_existing_configurations(name, dtype):
    import tfep_amd.nn.embeddings as E
    g = golden('embeddings.npz')
    emb = gu.build_embedding(gu.embedding_configs()[name], E)
    emb.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in gu.sub(g, f'emb/{name}/sd/').items()})
    emb = emb.to(dtype).cuda()
    with torch.no_grad():
        out = emb(torch.from_numpy(g[f'emb/{name}/x']).to(dtype).cuda())
    members = flip_members(emb)
    assert members and all(m.last_route == 'kernel' for m in members)
    check_output(out, g[f'emb/{name}/out_f64'], dtype, name)


# ------------------------------------------------------------------ 2. gradients of the module

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(flip_configs()))
def test_module_gradients(name, dtype):
    emb, x, g = build_flip(name, dtype)
    x.requires_grad_(True)
    out = emb(x)
    assert emb.last_route == 'kernel' and out.requires_grad
    (out * cosine_weights(out)).sum().backward()
    check_gradients(x.grad, {k: p.grad for k, p in emb.named_parameters()}, g[f'{name}/gx'],
                    {k: g[f'{name}/gp/{k}'] for k, _ in emb.named_parameters()}, dtype)
    assert sum(1 for _ in emb.named_parameters()) == 8


# ------------------------------------------------------------------ 3. bitwise flip invariance

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['strided', 'max'])
def test_flip_invariance_is_bitwise(name, dtype):
    emb, x, _ = build_flip(name, dtype)
    flipped = x.clone()
    flipped[:, emb._embedded_indices] = -flipped[:, emb._embedded_indices]
    rest = emb._nonembedded_indices
    assert torch.equal(flipped[:, rest], x[:, rest]) and not torch.equal(flipped, x)
    with torch.no_grad():
        a, b = emb(x), emb(flipped)
    assert emb.last_route == 'kernel'
    assert torch.equal(a, b)
    assert float(a[:, len(rest):].abs().max()) > 0


# ------------------------------------------------------------------ 4. determinism and row independence

@pytest.mark.parametrize('dtype', DTYPES)
def test_backward_is_deterministic_rows_are_independent_and_chunks_accumulate(dtype):
    from tfep_amd import ops
    emb, x, g = build_flip('q257', dtype)
    params = [p.detach() for p in emb.network_parameters()]
    names = [k for k, _ in emb.named_parameters()]
    eidx, nidx = emb.device_indices(x.device)
    with torch.no_grad():
        out = emb(x)
        alone = emb(x[200:201].clone())
    assert torch.equal(alone[0], out[200])
    gout = cosine_weights(out)
    gx1, grads1 = ops.flip_invariant_embedding_backward(x, eidx, nidx, 4, params, gout)
    gx2, grads2 = ops.flip_invariant_embedding_backward(x, eidx, nidx, 4, params, gout)
    assert torch.equal(gx1, gx2) and all(torch.equal(a, b) for a, b in zip(grads1, grads2))
    # two halves of the batch, the second added to the first
    h = 128
    gxa, acc = ops.flip_invariant_embedding_backward(x[:h], eidx, nidx, 4, params, gout[:h])
    gxb, acc2 = ops.flip_invariant_embedding_backward(x[h:], eidx, nidx, 4, params, gout[h:], grads=acc)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(acc, acc2))
    assert torch.equal(torch.cat([gxa, gxb]), gx1)                     # (per row: no sum over the batch)
    ref = {k: g[f'q257/gp/{k}'] for k in names}
    check_gradients(torch.cat([gxa, gxb]), dict(zip(names, acc)), g['q257/gx'], ref, dtype)
    check_gradients(gx1, dict(zip(names, grads1)), g['q257/gx'], ref, dtype)


# Backward launches of more than one workgroup.  The VJP kernel gives a workgroup 256 x ITEMS items (ITEMS = 4 for E <= 8,
# 2 for E <= 16, 1 above), one workspace row per workgroup, at most 2048 workgroups: 'wg3' is 3 workgroups at 4 items per
# lane, 'wg12' 12 workgroups at the widest embedding, 'stride' 2050 batches on 2048 workgroups (two of them take a second
# batch and add to their row).  The smallest networks that reach those item counts keep the cases quick.
MULTI = {
    'wg3': (3000, dict(n_features_in=5, embedding_dimension=3, embedded_indices=[0, 1, 2, 3], hidden_layer_width=8)),
    'wg12': (3000, dict(n_features_in=4, embedding_dimension=32, hidden_layer_width=4)),
    'stride': (4100, dict(n_features_in=128, embedding_dimension=17, vector_dimension=1, hidden_layer_width=2)),
}


@functools.lru_cache(maxsize=None)
def multi_case(name):
    """Module state, input, cotangent and the float64 autograd gradients of ``torch_forward`` on the device (the reference's
    own code, kept verbatim in the module), computed once for both dtypes; inputs and weights are float32-rounded."""
    from tfep_amd.nn.embeddings import FlipInvariantEmbedding
    B, kw = MULTI[name]
    torch.manual_seed(sorted(MULTI).index(name))
    emb = FlipInvariantEmbedding(**kw)
    sd = {k: v.clone() for k, v in emb.state_dict().items()}
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(B, kw['n_features_in'], generator=gen)
    emb = emb.double().cuda()
    xg = x.double().cuda().requires_grad_(True)
    out = emb.torch_forward(xg)
    gout = torch.randn(out.shape, generator=gen)
    (out * gout.double().cuda()).sum().backward()
    ref = {k: p.grad.cpu().numpy() for k, p in emb.named_parameters()}
    return kw, sd, x, gout, xg.grad.cpu().numpy(), ref


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(MULTI))
def test_backward_over_several_workgroups(name, dtype):
    from tfep_amd import _lib, ops
    from tfep_amd.nn.embeddings import FlipInvariantEmbedding
    kw, sd, x, gout, ref_gx, ref = multi_case(name)
    emb = FlipInvariantEmbedding(**kw)
    emb.load_state_dict(sd)
    emb = emb.to(dtype).cuda()
    x, gout = x.to(dtype).cuda(), gout.to(dtype).cuda()
    d, H, E = emb.vector_dimension, emb.hidden_layer_width, emb.embedding_dimension
    EP = 4 if E <= 4 else 8 if E <= 8 else 16 if E <= 16 else 32
    n_rows = _lib.load().tfep_flip_invariant_embedding_backward_workspace_bytes(
        x.shape[0], len(emb._embedded_indices), d, H, E) // (8 * (H * (2 * d + 3 + EP) + EP + 1))
    n_items = x.shape[0] * (len(emb._embedded_indices) // d)
    items_per_workgroup = 256 * (4 if EP <= 8 else 2 if EP == 16 else 1)
    assert n_rows == {'wg3': 3, 'wg12': 12, 'stride': 2048}[name]
    assert (n_items > n_rows * items_per_workgroup) == (name == 'stride')          # only 'stride' takes a second batch
    params = [p.detach() for p in emb.network_parameters()]
    names = [k for k, _ in emb.named_parameters()]
    eidx, nidx = emb.device_indices(x.device)
    gx1, grads1 = ops.flip_invariant_embedding_backward(x, eidx, nidx, d, params, gout)
    gx2, grads2 = ops.flip_invariant_embedding_backward(x, eidx, nidx, d, params, gout)
    assert torch.equal(gx1, gx2) and all(torch.equal(a, b) for a, b in zip(grads1, grads2))
    check_gradients(gx1, dict(zip(names, grads1)), ref_gx, ref, dtype)


# ------------------------------------------------------------------ 5. fallback

def test_over_the_limits_takes_the_torch_route():
    from tfep_amd.nn.embeddings import FlipInvariantEmbedding
    torch.manual_seed(3)
    emb = FlipInvariantEmbedding(n_features_in=9, embedding_dimension=4, embedded_indices=[1, 2, 3, 4, 5, 6, 7, 8],
                                 hidden_layer_width=65).cuda()
    assert not emb.within_kernel_limits()
    x = torch.randn(7, 9, device='cuda')
    with torch.no_grad():
        out = emb(x)
        assert emb.last_route == 'torch'
        assert torch.equal(out, emb.torch_forward(x))


@pytest.mark.parametrize('dtype', DTYPES)
def test_kernel_agrees_with_its_own_torch_forward(dtype):
    import tfep_amd.nn.embeddings as E
    g = golden('embeddings.npz')
    emb = gu.build_embedding(gu.embedding_configs()['flip_some'], E)
    emb.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in gu.sub(g, 'emb/flip_some/sd/').items()})
    emb = emb.to(dtype).cuda()
    x = torch.from_numpy(g['emb/flip_some/x']).to(dtype).cuda()
    with torch.no_grad():
        out = emb(x)
        assert emb.last_route == 'kernel'
        ref = emb.torch_forward(x)
    check_output(out, ref.cpu().numpy().astype(np.float64), dtype, 'flip_some against torch_forward')


# ------------------------------------------------------------------ 6. MAF layers

def build_flow(name, g):
    import tfep_amd.nn.embeddings as E
    from tfep_amd.nn.flows import MAF, SequentialFlow
    from tfep_amd.nn.transformers import AffineTransformer, NeuralSplineTransformer
    cfg = gu.embedded_flow_configs()[name]
    n_tr = sum(1 for d in cfg['degrees_in'] if d >= 0)
    tr = (NeuralSplineTransformer(x0=torch.full((n_tr,), -4.0), xf=torch.full((n_tr,), 4.0), n_bins=8)
          if cfg['transformer'] == 'spline' else AffineTransformer())
    flow = SequentialFlow(MAF(degrees_in=torch.as_tensor(cfg['degrees_in']), transformer=tr,
                              embedding=gu.build_embedding(cfg['embedding'], E), initialize_identity=False))
    sd = flow.state_dict()
    for k, v in gu.sub(g, f'{name}/sd/').items():
        sd[k] = torch.from_numpy(np.asarray(v))
    flow.load_state_dict(sd, strict=True)
    return flow.cuda()


def close(got, ref, rtol, atol, what):
    np.testing.assert_allclose(got.detach().cpu().numpy(), np.asarray(ref, np.float64), rtol=rtol, atol=atol, err_msg=what)


@pytest.mark.parametrize('name', list(gu.embedded_flow_configs()))
def test_float64_layers_forward_inverse_and_gradients(name):
    g = golden('embeddings.npz')
    flow = build_flow(name, g).double()
    members = flip_members(flow)
    assert members and all(p.dtype == F64 for p in flow.parameters())
    x = torch.from_numpy(g[f'{name}/x']).to(F64).cuda()
    with torch.no_grad():
        y, ldj = flow(x)
        xi, li = flow.inverse(torch.from_numpy(g[f'{name}/inv_in']).to(F64).cuda())
    assert y.dtype == F64 and all(m.last_route == 'kernel' for m in members)
    assert [layer.last_inverse_route for layer in flow] == ['per_degree']
    close(y, g[f'{name}/y_f64'], 1e-9, 1e-10, 'y')
    close(ldj, g[f'{name}/ldj_f64'], 1e-9, 1e-9, 'ldj')
    close(xi, g[f'{name}/xinv_f64'], 1e-8, 1e-9, 'x')
    close(li, g[f'{name}/ldjinv_f64'], 1e-8, 1e-8, 'ldj of the inverse')
    xg = x.clone().requires_grad_(True)
    y, ldj = flow(xg)
    ((y * cosine_weights(y)).sum() + ldj.sum()).backward()
    names = [k for k, _ in flow.named_parameters()]
    check_gradients(xg.grad, {k: p.grad for k, p in flow.named_parameters()}, g[f'{name}/gx_f64'],
                    {k: g[f'{name}/gp/{k}'] for k in names}, F64)
    assert sum('embedding_layer' in k or 'weight_layer' in k for k in names) == 8
    with pytest.raises(TypeError):
        flow(x.float())


@pytest.mark.parametrize('name', list(gu.embedded_flow_configs()))
def test_float32_layers_run_the_embedding_on_its_kernels(name, monkeypatch):
    from tfep_amd import ops
    g = golden('embeddings.npz')
    flow = build_flow(name, g)
    members = flip_members(flow)
    calls = []                       # the keyword arguments of every call of the VJP wrapper
    backward = ops.flip_invariant_embedding_backward
    monkeypatch.setattr(ops, 'flip_invariant_embedding_backward', lambda *a, **kw: calls.append(kw) or backward(*a, **kw))
    x = torch.from_numpy(g[f'{name}/x']).cuda()
    with torch.no_grad():
        y, ldj = flow(x)
    assert all(m.last_route == 'kernel' for m in members)
    assert rel(y.cpu(), g[f'{name}/y_f64']) < max(2 * rel(g[f'{name}/y_f32'], g[f'{name}/y_f64']), 2e-6)
    for m in members:
        m.last_route = None
    xg = x.clone().requires_grad_(True)
    y, ldj = flow(xg)
    ((y * cosine_weights(y)).sum() + ldj.sum()).backward()
    assert calls and all(m.last_route == 'kernel' for m in members)
    if name == 'flipflow':
        # the layer backward calls the entry point itself and accumulates into its own buffers (the registered op, which
        # the autograd branch of a MixedEmbedding goes through, passes neither ``grads`` nor ``gx``)
        assert all(kw.get('grads') is not None and kw.get('gx') is not None for kw in calls), calls
    else:
        assert all('grads' not in kw and 'gx' not in kw for kw in calls)
    names = [k for k, _ in flow.named_parameters()]
    check_gradients(xg.grad, {k: p.grad for k, p in flow.named_parameters()}, g[f'{name}/gx_f64'],
                    {k: g[f'{name}/gp/{k}'] for k in names}, F32)


def test_float64_layer_with_an_unknown_embedding_still_raises():
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.embeddings import MAFEmbedding
    from tfep_amd.nn.flows import MAF

    class Identity(MAFEmbedding):
        def forward(self, x):
            return x

        def get_degrees_out(self, degrees_in):
            return degrees_in

    maf = MAF(generate_degrees(4), embedding=Identity()).double().cuda()
    with pytest.raises(TypeError, match='float64 is not supported for the Identity embedding'):
        maf(torch.zeros(3, 4, device='cuda', dtype=F64))


# ------------------------------------------------------------------ 7. ops

@pytest.mark.parametrize('dtype', DTYPES)
def test_ops_pass_opcheck(dtype):
    emb, x, _ = build_flip('strided', dtype)
    eidx, nidx = emb.device_indices(x.device)
    params = [p.detach().clone().requires_grad_(True) for p in emb.network_parameters()]
    torch.library.opcheck(torch.ops.tfep.flip_invariant_embedding.default,
                          (x.clone().requires_grad_(True), eidx, nidx, 4, *params))
    with torch.no_grad():
        out = emb(x)
    torch.library.opcheck(torch.ops.tfep.flip_invariant_embedding_backward.default,
                          (x, eidx, nidx, 4, *[p.detach() for p in params], cosine_weights(out)))


def test_graphed_flow_replays_the_eager_result():
    from tfep_amd.graphs import GraphedFlow
    g = golden('embeddings.npz')
    flow = build_flow('flipflow', g)
    x = torch.from_numpy(g['flipflow/x']).cuda()
    with torch.no_grad():
        y0, l0 = flow(x)
        gf = GraphedFlow(flow, x.shape[0], x.shape[1])
        y1, l1 = gf(x)
        assert torch.equal(y0, y1) and torch.equal(l0, l1)
        x2 = x * 0.5
        y2, l2 = gf(x2)
        ye, le = flow(x2)
        assert torch.equal(y2, ye) and torch.equal(l2, le)
