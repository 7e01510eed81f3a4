"""Host tests (no GPU) of the opt-in float64 Moebius transformer (``MoebiusTransformer.float64_kernels``): the switch and
the refusals it leaves in place, the C ABI, the planning of the float64 blocked inverse (member kinds 5 and 6 of
``tfep_inverse_chain_vec_f64``), and the float64 restatement tests/moebius_ref.py against the reference's fixtures."""
import json
import os
import re

import numpy as np
import pytest
import torch

import golden_util as gu
import moebius_ref
from tfep_amd.nn.conditioners import generate_degrees
from tfep_amd.nn.embeddings import PeriodicEmbedding
from tfep_amd.nn.flows import MAF
from tfep_amd.nn.flows import _blocked_f64 as bf
from tfep_amd.nn.transformers import AffineTransformer, MixedTransformer, MoebiusTransformer, NeuralSplineTransformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
SYMBOLS = ('tfep_moebius_forward_f64', 'tfep_moebius_backward_f64')


def test_the_flag_defaults_to_false_on_the_class():
    assert MoebiusTransformer.float64_kernels is False
    tr = MoebiusTransformer(2)
    assert tr.float64_kernels is False and 'float64_kernels' not in tr.__dict__
    tr.float64_kernels = True                                   # an instance sets its own
    assert MoebiusTransformer.float64_kernels is False and MoebiusTransformer(2).float64_kernels is False


def test_without_the_flag_float64_is_refused_as_before():
    from tfep_amd.nn.flows import _backward
    from tfep_amd.nn.transformers.mixed import check_float64_members
    z = torch.zeros(2, 4, dtype=F64)
    with pytest.raises(TypeError, match='MoebiusTransformer: float64 is not supported for the Moebius transformer yet'):
        MoebiusTransformer(2)(z, z)
    with pytest.raises(TypeError, match='MoebiusTransformer: float64 is not supported for the Moebius transformer yet'):
        MoebiusTransformer(2).inverse(z, z)
    mixed = MixedTransformer([MoebiusTransformer(2), AffineTransformer()], [[0, 1], [2, 3]])
    with pytest.raises(TypeError, match='mixed transformer with a Moebius member'):
        check_float64_members(mixed)
    with pytest.raises(TypeError, match='float64 is not supported for this transformer yet'):
        _backward.transformer_vjp(MoebiusTransformer(2), z, z, 0, z, None, z.clone(), z.clone())
    # with the flag the same calls get past the refusal, to the check that a kernel input lives on the device
    mixed._transformers[0].float64_kernels = True
    check_float64_members(mixed)
    on = MoebiusTransformer(2)
    on.float64_kernels = True
    from tfep_amd._lib import TfepHipError
    with pytest.raises(TfepHipError, match='x is on cpu'):
        on(z, z)


def test_header_and_bindings_carry_the_two_entry_points():
    import ctypes
    from tfep_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    declared = set(re.findall(r'\b(tfep_[a-z0-9_]+)\s*\(', header))
    for s in SYMBOLS:
        assert s in declared and s in _lib.EXPORTED_SYMBOLS, s
    # the signatures of the float32 entry points: max_radius is a double in both (the float32 kernels compute in fp64 too)
    for base in ('tfep_moebius_forward', 'tfep_moebius_backward'):
        f32, f64 = _lib._SIGNATURES[base], _lib._SIGNATURES[base + '_f64']
        assert f32[0] is f64[0] and len(f32[1]) == len(f64[1])
        assert all(a is b for a, b in zip(f32[1], f64[1])) and f32[1][5] is ctypes.c_double
    assert re.search(r'member_kind 5\s+Moebius', header) and re.search(r'member_kind 6\s+the same on the unit sphere', header)


# ------------------------------------------------------------------ planning of the float64 blocked inverse

def _layer(dimension, unit_sphere, D=12, repeats=None, flag=True, vectors=True, **kw):
    tr = MoebiusTransformer(dimension, unit_sphere=unit_sphere)
    tr.float64_kernels = flag
    maf = MAF(generate_degrees(D, repeats=repeats or dimension), transformer=tr, hidden_layers=[20, 20], **kw).double()
    maf.blocked_inverse_f64_vectors = vectors
    return maf


@pytest.mark.parametrize('unit_sphere', [False, True])
def test_a_moebius_member_gets_kind_5_or_6_only_with_both_flags(unit_sphere):
    maf = _layer(3, unit_sphere)
    assert maf._blocked_f64_ok()
    hp = maf._blocked_f64_host_plan()
    assert hp['kinds'] == [6 if unit_sphere else 5]
    assert hp['feats'][:, 6].tolist() == [1, 2, 3] * 4                       # 1 + component
    assert hp['feats'][:, 7].tolist() == [1, 2, -1, 4, 5, -1, 7, 8, -1, 10, 11, -1]
    assert hp['feats'][:, 2].tolist() == [1] * 12 and hp['par_cols'] == 2    # one parameter per feature
    for flag, vectors in ((True, False), (False, True), (False, False)):
        off = _layer(3, unit_sphere, flag=flag, vectors=vectors)
        assert not off._blocked_f64_ok(), (flag, vectors)
        assert off._make_blocked_f64_host_plan(16) is None


def test_mixed_members_keep_their_kinds_beside_a_moebius_member():
    tr = MixedTransformer([MoebiusTransformer(2, unit_sphere=True), NeuralSplineTransformer(torch.full((4,), -4.0), torch.full((4,), 4.0), 8),
                           AffineTransformer()], [[0, 1, 4, 5], [2, 3, 6, 7], [8, 9, 10, 11]])
    maf = MAF(generate_degrees(12, repeats=2), transformer=tr, hidden_layers=[20, 20]).double()
    maf.blocked_inverse_f64_vectors = True
    assert not maf._blocked_f64_ok()                                         # the member has not opted in
    tr._transformers[0].float64_kernels = True
    assert maf._blocked_f64_ok() and maf._blocked_f64_host_plan()['kinds'] == [6, 1, 0]


def test_dimension_one_gets_head_links():
    """Every feature of a d = 1 member is a vector of one component: a head (1 + component = 1) with no next slot, so
    the chain kernel evaluates it like any other vector."""
    maf = _layer(1, False, D=6, repeats=1)
    assert maf._blocked_f64_ok()
    hp = maf._blocked_f64_host_plan()
    assert hp['kinds'] == [5] and hp['feats'][:, 6].tolist() == [1] * 6 and hp['feats'][:, 7].tolist() == [-1] * 6
    links = bf.vector_links(np.arange(4), [0, 0, 1, 1], None, np.arange(4), [1])
    assert links.tolist() == [[1, -1]] * 4


def test_a_straddling_vector_or_a_periodic_component_has_no_plan():
    assert not _layer(2, True, repeats=1)._blocked_f64_ok()                   # one degree per feature: every 2-vector straddles
    assert not _layer(3, False, repeats=2)._blocked_f64_ok()
    emb = PeriodicEmbedding(12, limits=[0.0, 1.0], periodic_indices=[0, 1])
    assert not _layer(2, True, embedding=emb)._blocked_f64_ok()
    # the pure function says the same
    assert bf.vector_links(np.arange(4), [0, 1, 1, 2], None, np.arange(4), [2]) is None
    assert bf.vector_links(np.arange(4), [0, 0, 1, 1], None, np.arange(4), [2], [False, True, False, False]) is None
    assert bf.vector_links(np.arange(4), [0, 0, 1, 1], None, np.arange(4), [2]) is not None


def test_the_plan_cache_key_changes_with_either_flag():
    maf = _layer(2, True)
    plan = maf._blocked_f64_host_plan()
    assert plan is not None and maf._blocked_f64_host_plan() is plan          # cached
    n = len(maf._dev)
    maf._transformer.float64_kernels = False
    assert maf._blocked_f64_host_plan() is None and len(maf._dev) == n + 1
    maf._transformer.float64_kernels = True
    maf.blocked_inverse_f64_vectors = False
    assert maf._blocked_f64_host_plan() is None and len(maf._dev) == n + 2
    maf.blocked_inverse_f64_vectors = True
    assert maf._blocked_f64_host_plan() is plan and len(maf._dev) == n + 2


# ------------------------------------------------------------------ the float64 restatement

@pytest.mark.parametrize('name', ['d2_u0', 'd2_u1', 'd3_u0', 'd3_u1'])
def test_moebius_ref_reproduces_the_reference_fixtures(name):
    g = gu.load('transformers.npz')
    meta = json.loads(str(g['moebius/meta']))[f'moebius/{name}']
    x, par, yin = (torch.from_numpy(g[f'moebius/{name}/{k}']).double() for k in ('x', 'par', 'inv_in'))
    y, l = moebius_ref.moebius(x, par, **meta)
    np.testing.assert_allclose(y.numpy(), g[f'moebius/{name}/y_f64'], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(l.numpy(), g[f'moebius/{name}/ldj_f64'], rtol=1e-11, atol=1e-11)
    xi, li = moebius_ref.moebius_inverse(yin, par, **meta)
    np.testing.assert_allclose(xi.numpy(), g[f'moebius/{name}/xinv_f64'], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(li.numpy(), g[f'moebius/{name}/ldjinv_f64'], rtol=1e-11, atol=1e-11)


def test_moebius_ref_has_the_zero_subgradient_at_w_zero():
    x = torch.randn(3, 4, dtype=F64, generator=torch.Generator().manual_seed(0))
    w = torch.zeros(3, 4, dtype=F64, requires_grad=True)
    y, l = moebius_ref.moebius(x, w, 2)
    (y.sum() + l.sum()).backward()
    assert bool(torch.isfinite(w.grad).all()) and torch.allclose(y.detach(), x)
