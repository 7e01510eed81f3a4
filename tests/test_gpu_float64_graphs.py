"""GPU tests of HIP-graph replay in float64 (``tfep_amd.graphs.GraphedFlow`` / ``GraphedTrainingStep`` with ``dtype``).

The eager and the graphed side of every comparison launch the same kernels on the same data, so every comparison between
them is ``torch.equal`` -- bit for bit.  No host decision had to be replaced by device code of another arithmetic, so no
comparison uses a tolerance; the one tolerance here is the round trip ``inverse(forward(x)) == x`` of the float64 flow,
1e-10.

Shapes: B = 3 (fewer rows than a wave) and B = 65 (one row past a wave), D between 4 and 20 -- the smallest sizes at which
the routes still branch (blocked inverse with three blocks, the pass per degree, fixed features, every transformer and
embedding kernel, the frame kernels).  The graphs are made one after the other in one process."""
import contextlib
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

F64 = torch.float64
BATCHES = [3, 65]


@contextlib.contextmanager
def default_float64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def rand(B, D, seed, scale=3.0, dtype=F64):
    """Uniform in (-scale, scale): inside the spline domains used here (-4, 4)."""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, D, generator=g, dtype=torch.float64) * 2 - 1) * scale).to(dtype).cuda()


def spline(D, n_bins=8):
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    return NeuralSplineTransformer(torch.full((D,), -4.0), torch.full((D,), 4.0), n_bins)


def spline_maf2(D=12, seed=0):
    """The 2-layer float64 MAF of the issue: RQ spline with 8 bins, ascending / descending degrees, random weights."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF, SequentialFlow
    torch.manual_seed(seed)
    with default_float64():
        flow = SequentialFlow(*[MAF(generate_degrees(D, o), transformer=spline(D), initialize_identity=False)
                                for o in ('ascending', 'descending')])
    return flow.cuda()


def eager(flow, x, inverse=False):
    with torch.no_grad():
        return (flow.inverse if inverse else flow)(x)


def assert_replays_eager(flow, x, inverse=False, **kw):
    """A graph of ``flow`` at the shape of ``x`` gives the eager result bit for bit, on ``x`` and on other data (a replay
    computes: it does not return what the capture left in the static tensors); float64, and no range guard."""
    from tfep_amd.graphs import GraphedFlow
    ref = eager(flow, x, inverse)
    g = GraphedFlow(flow, x.shape[0], x.shape[1], inverse=inverse, **kw)
    assert g.static_in.dtype is F64
    for data in (x, 0.5 * x):
        want = eager(flow, data, inverse)
        got = g(data)
        assert got[0].dtype is F64 and got[1].dtype is F64
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(ref[0], eager(flow, 0.5 * x, inverse)[0])
    assert g.n_guarded_calls == 0 and g.last_call_guarded is False and g._flag_total is None
    return g


# ------------------------------------------------------------------ forward / inverse of the MAF

@pytest.mark.parametrize('B', BATCHES)
def test_forward_of_a_float64_maf(B):
    """``GraphedFlow(flow, B, D)`` infers float64 from the parameters.  (Before ``dtype``: a TypeError at construction, the
    float64 layer's own, on the float32 static input.)"""
    flow = spline_maf2()
    assert_replays_eager(flow, rand(B, 12, seed=B))


@pytest.mark.parametrize('block', [4, 5])
@pytest.mark.parametrize('B', BATCHES)
def test_blocked_inverse_of_a_float64_maf(B, block):
    """Blocks of 4 degrees (three full blocks of the 12) and of 5 (5 + 5 + 2: the block size does not divide D)."""
    flow = spline_maf2()
    for layer in flow:
        layer.inverse_block_f64 = block
        assert len(layer._blocked_f64_host_plan()['blocks']) == 3
    x = rand(B, 12, seed=10 + B)
    y = eager(flow, x)[0]
    g_inv = assert_replays_eager(flow, y, inverse=True)
    assert [layer.last_inverse_route for layer in flow] == ['blocked_f64', 'blocked_f64']
    from tfep_amd.graphs import GraphedFlow
    g_fwd = GraphedFlow(flow, B, 12)
    x_back, ldj_back = g_inv(g_fwd(x)[0])
    err = float((x_back - x).abs().max())
    print(f'round trip through two graphs, B={B}, block={block}: max |x - x\'| = {err:.3e}')
    assert err <= 1e-10


@pytest.mark.parametrize('B', BATCHES)
def test_per_degree_inverse_of_a_float64_layer(B):
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    torch.manual_seed(1)
    with default_float64():
        layer = MAF(generate_degrees(6), transformer=spline(6), initialize_identity=False).cuda()
    layer.blocked_inverse = False
    assert_replays_eager(layer, rand(B, 6, seed=20 + B), inverse=True)
    assert layer.last_inverse_route == 'per_degree'


def test_replay_reads_the_current_parameters():
    from tfep_amd.graphs import GraphedFlow
    flow = spline_maf2(seed=2)
    x = rand(65, 12, seed=30)
    g = GraphedFlow(flow, 65, 12)
    y0, l0 = g(x)
    assert torch.equal(y0, eager(flow, x)[0])
    with torch.no_grad():
        for layer in flow:
            layer._conditioner.layers[-1].weight_v.add_(0.01)
    y1, l1 = g(x)
    want = eager(flow, x)
    assert torch.equal(y1, want[0]) and torch.equal(l1, want[1])
    assert not torch.equal(y1, y0)


# ------------------------------------------------------------------ one case per remaining float64 route

def _layer(name):
    """``(flow, D, has_inverse)`` of one float64 route, random weights."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.embeddings import FlipInvariantEmbedding, PeriodicEmbedding
    from tfep_amd.nn.flows import MAF, CenteredCentroidFlow, OrientedFlow, PartialFlow, PCAWhitenedFlow
    from tfep_amd.nn.transformers import (AffineTransformer, MixedTransformer, QuaternionProductTransformer,
                                          SOSPolynomialTransformer, SymmetrizedMoebiusTransformer,
                                          VolumePreservingShiftTransformer)
    torch.manual_seed(40)

    def maf(D, **kw):
        kw.setdefault('degrees_in', generate_degrees(D))
        return MAF(initialize_identity=False, **kw)
    with default_float64():
        if name == 'affine':
            return maf(7, transformer=AffineTransformer()), 7, True
        if name == 'mixed, fixed features':
            # 9 features, two of them conditioning (fixed: copied through); of the 7 transformed ones 3 go through a spline, 2
            # through an affine map and 2 through a volume-preserving shift, one of those periodic
            shift = VolumePreservingShiftTransformer(torch.tensor([1]), torch.tensor([-4.0, 4.0]))
            mixed = MixedTransformer([spline(3, 4), AffineTransformer(), shift], [[0, 2, 5], [1, 3], [4, 6]])
            return maf(9, degrees_in=generate_degrees(9, conditioning_indices=[2, 6]), transformer=mixed), 9, True
        if name == 'symmetrized moebius':
            return maf(8, degrees_in=generate_degrees(8, repeats=2), transformer=SymmetrizedMoebiusTransformer(2)), 8, True
        if name == 'quaternion product':
            return maf(8, degrees_in=generate_degrees(8, repeats=4), transformer=QuaternionProductTransformer()), 8, True
        if name == 'sos':
            return maf(5, transformer=SOSPolynomialTransformer(2)), 5, False
        if name == 'periodic embedding':
            emb = PeriodicEmbedding(7, limits=[-4.0, 4.0], periodic_indices=[1, 4])
            return maf(7, transformer=spline(7), embedding=emb), 7, True
        if name == 'flip-invariant embedding':
            emb = FlipInvariantEmbedding(n_features_in=10, embedding_dimension=3, embedded_indices=[2, 3, 4, 5, 6, 7, 8, 9])
            return maf(10, degrees_in=torch.tensor([0, 1, 2, 2, 2, 2, 3, 3, 3, 3]), transformer=spline(10), embedding=emb), 10, True
        if name == 'partial':
            return PartialFlow(maf(5, transformer=AffineTransformer()), fixed_indices=[1, 4, 6]), 8, True
        if name == 'centered centroid':
            return CenteredCentroidFlow(maf(9, transformer=AffineTransformer()), space_dimension=3), 12, True
        if name == 'oriented':
            return OrientedFlow(maf(9, transformer=AffineTransformer())), 12, True
        if name == 'pca':
            g = torch.Generator().manual_seed(41)
            data = torch.randn(200, 6, generator=g, dtype=F64) @ (torch.randn(6, 6, generator=g, dtype=F64) / 2 + torch.eye(6)) + 1.0
            flow = PCAWhitenedFlow(maf(6, transformer=AffineTransformer()), data, blacken=True)
            assert flow.whitening_matrix.dtype is F64
            return flow, 6, True
    raise ValueError(name)


ROUTES = ['affine', 'mixed, fixed features', 'symmetrized moebius', 'quaternion product', 'sos', 'periodic embedding',
          'flip-invariant embedding', 'partial', 'centered centroid', 'oriented', 'pca']


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('name', ROUTES)
def test_every_other_float64_route(name, B):
    flow, D, has_inverse = _layer(name)
    flow = flow.cuda()
    assert all(p.dtype is F64 for p in flow.parameters())
    x = rand(B, D, seed=50 + B, scale=1.5)
    assert_replays_eager(flow, x)
    if has_inverse:
        assert_replays_eager(flow, eager(flow, x)[0], inverse=True)
    if name in ('centered centroid', 'oriented'):
        assert flow.last_route == 'kernels'
    if name == 'flip-invariant embedding':
        assert flow._embedding.last_route == 'kernel'


# ------------------------------------------------------------------ training step

def test_training_step_of_a_float64_maf():
    """Three replays of the captured step -- forward, loss, backward, AdamW -- against three eager steps from a copy."""
    from tfep_amd.graphs import GraphedTrainingStep
    from tfep_amd.loss import BoltzmannKLDivLoss
    D, B = 12, 65
    flow = spline_maf2(seed=3)
    twin = copy.deepcopy(flow)
    loss_mod = BoltzmannKLDivLoss()

    def loss_fn(y, ldj):
        return loss_mod(0.5 * (y ** 2).sum(dim=1), ldj)         # the potential of a standard normal, in torch ops
    kw = dict(lr=1e-3, weight_decay=0.01, capturable=True)
    opt, opt_twin = torch.optim.AdamW(flow.parameters(), **kw), torch.optim.AdamW(twin.parameters(), **kw)
    xs = [rand(B, D, seed=60 + i) for i in range(3)]

    before = copy.deepcopy((flow.state_dict(), opt.state_dict()))
    step = GraphedTrainingStep(flow, loss_fn, opt, B, D)
    assert step.static_in.dtype is F64 and step.static_loss.dtype is F64
    # construction leaves the model and the optimiser as it found them; state the warm-up created is zeroed, the value a
    # fresh optimiser starts from (the documented contract of the float32 class)
    for k, v in flow.state_dict().items():
        assert torch.equal(v, before[0][k]), k
    assert opt.state_dict()['param_groups'] == before[1]['param_groups']
    assert all(float(v.abs().sum()) == 0.0 for st in opt.state.values() for v in st.values() if torch.is_tensor(v))

    for i, x in enumerate(xs):
        opt_twin.zero_grad(set_to_none=True)
        loss = loss_fn(*twin(x))
        loss.backward()
        opt_twin.step()
        got = step(x)
        assert got.dtype is F64
        assert float(got) == float(loss.detach()), (i, float(got), float(loss.detach()))
        del loss
    assert all(p.grad is not None and p.grad.dtype is F64 for p in step.params)
    for (n, p), q in zip(flow.named_parameters(), twin.parameters()):
        assert torch.equal(p, q), n
    assert step.range_guard_tripped() is False and step._flag_total is None
    with pytest.raises(TypeError):
        step(xs[0].float())


# ------------------------------------------------------------------ dtype contract

def test_dtype_contract():
    from tfep_amd.graphs import GraphedFlow, GraphedTrainingStep
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    flow = spline_maf2(seed=4)
    x = rand(3, 12, seed=70)
    g = GraphedFlow(flow, 3, 12)
    with pytest.raises(TypeError, match='float64'):
        g(x.float())
    assert torch.equal(g(x)[0], eager(flow, x)[0])               # (the refused call left the graph as it was)
    with pytest.raises(ValueError, match='float16'):
        GraphedFlow(flow, 3, 12, dtype=torch.float16)
    with pytest.raises(ValueError, match='float16'):
        GraphedTrainingStep(flow, lambda y, l: l.mean(), torch.optim.SGD(flow.parameters(), lr=0.1), 3, 12, dtype=torch.float16)
    assert torch.equal(GraphedFlow(flow, 3, 12, dtype=F64)(x)[0], eager(flow, x)[0])
    assert g.n_guarded_calls == 0 and g.last_call_guarded is False

    # a float32 flow with dtype=None is what it was
    torch.manual_seed(5)
    flow32 = MAF(generate_degrees(12), transformer=spline(12), initialize_identity=False).cuda()
    x32 = rand(65, 12, seed=71, dtype=torch.float32)
    g32 = GraphedFlow(flow32, 65, 12)
    assert g32.static_in.dtype is torch.float32
    got, want = g32(x32), eager(flow32, x32)
    assert got[0].dtype is torch.float32 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    got = g32(x32.double())                                       # (converts, as it always has)
    assert torch.equal(got[0], want[0])
