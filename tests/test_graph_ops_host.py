"""Host side of the differentiable radial expansion and segment sum: the plain reference of tests/graph_ops_ref.py against
derivatives written out by hand, the C ABI tables, and the opt-in switches (no kernel is launched)."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import graph_ops_ref as gr
from tfep_amd import _lib
from tfep_amd.nn import graph
from tfep_amd.nn.embeddings import BehlerParrinelloRadialExpansion, GaussianBasisExpansion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
SYMBOLS = ('tfep_radial_expansion_f64', 'tfep_radial_expansion_backward', 'tfep_radial_expansion_backward_f64',
           'tfep_radial_expansion_backward_workspace_doubles', 'tfep_segment_sum_f64', 'tfep_segment_gather',
           'tfep_segment_gather_f64')


def _closed_form(r, mu, lg, kind, r_c):
    """``(f, df/dr, df/dmu, df/dlg)`` of one distance and one basis function, in plain Python floats."""
    gamma = math.exp(lg)
    e = math.exp(-gamma * (r - mu) ** 2)
    s, ds = 1.0, 0.0
    if kind != 'gauss':
        s, ds = 0.5 * math.cos(math.pi * r / r_c) + 0.5, -(math.pi / (2 * r_c)) * math.sin(math.pi * r / r_c)
        if kind == 'bp_zero' and r > r_c:
            s = ds = 0.0
    f = s * e
    return f, f * (-2 * gamma * (r - mu)) + e * ds, f * 2 * gamma * (r - mu), -f * gamma * (r - mu) ** 2


@pytest.mark.parametrize('kind', gr.KINDS)
def test_reference_matches_closed_form_derivatives(kind):
    r_c = gr.R_CUTOFF
    points = [0.0, 0.3, 0.9 * r_c, r_c, math.nextafter(r_c, 2 * r_c), 1.4 * r_c]
    means, lgs = [0.1, 0.7, 1.2], [math.log(2.0), math.log(11.0), math.log(0.5)]
    r = torch.tensor(points, dtype=F64, requires_grad=True)
    mu = torch.tensor(means, dtype=F64, requires_grad=True)
    lg = torch.tensor(lgs, dtype=F64, requires_grad=True)
    f = gr.expansion(r, mu, lg, kind)
    want = np.array([[_closed_form(p, m, l, kind, r_c) for m, l in zip(means, lgs)] for p in points])      # (n, K, 4)
    np.testing.assert_allclose(f.detach().numpy(), want[..., 0], rtol=1e-13, atol=1e-300)
    for i in range(len(points)):
        for k in range(len(means)):
            g_r, g_mu, g_lg = torch.autograd.grad(f[i, k], (r, mu, lg), retain_graph=True)
            got = (g_r[i].item(), g_mu[k].item(), g_lg[k].item())
            np.testing.assert_allclose(got, want[i, k, 1:], rtol=1e-12, atol=1e-15, err_msg=f'{kind} r={points[i]} k={k}')
            assert g_r.count_nonzero() <= 1 and g_mu.count_nonzero() <= 1 and g_lg.count_nonzero() <= 1
    if kind == 'bp_zero':
        g_r, = torch.autograd.grad(f.sum(), r)
        assert (g_r[-2:] == 0).all() and (f[-2:] == 0).all() and g_r[3] != 0


def test_reference_segment_sum_and_its_gradient():
    data = torch.arange(12.0, dtype=F64).reshape(6, 2).requires_grad_(True)
    ids = torch.tensor([2, 0, 2, 5, -1, 0])
    out = gr.segment_sum(data, ids, 4)
    assert out.tolist() == [[12.0, 14.0], [0.0, 0.0], [4.0, 6.0], [0.0, 0.0]]
    cot = torch.arange(8.0, dtype=F64).reshape(4, 2) + 1
    g, = torch.autograd.grad(out, data, cot)
    assert torch.equal(g, gr.segment_gather(cot, ids))
    assert g.tolist() == [[5.0, 6.0], [1.0, 2.0], [5.0, 6.0], [0.0, 0.0], [0.0, 0.0], [1.0, 2.0]]


def test_cases_hold_values_of_their_dtype_and_the_special_distances():
    for dtype in (gr.F32, F64):
        r, means, lg, g = gr.case(63, 5, dtype)
        for t in (r, means, lg, g):
            assert t.dtype == F64 and torch.equal(t.to(dtype).to(F64), t)
        rc = torch.tensor(gr.R_CUTOFF, dtype=dtype)
        assert r[-4:].tolist() == [float(rc), float(torch.nextafter(rc, rc * 2)), float(torch.nextafter(rc, rc * 0)), 0.0]
        assert r[-3] > gr.R_CUTOFF > r[-2] and 0 <= r.min() and r.max() <= 1.5 * gr.R_CUTOFF
    ref = gr.reference('bp_zero', 63, 5, F64)
    assert ref['f'].shape == (63, 5) and ref['g_r'].shape == (63,) and ref['g_means'].shape == ref['g_log_gammas'].shape == (5,)
    assert not any(t.requires_grad for t in gr.case(63, 5, F64))          # the shared inputs are left as they were
    assert gr.case(1, 1, F64)[0].shape == (1,) and float(torch.tensor(gr.R_CUTOFF, dtype=gr.F32)) == gr.R_CUTOFF


def test_c_abi_tables():
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    declared = set(re.findall(r'\b(tfep_[a-z0-9_]+)\s*\(', header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
    sig = _lib._SIGNATURES
    assert sig['tfep_segment_sum_f64'] == sig['tfep_segment_sum']
    assert sig['tfep_segment_gather'] == sig['tfep_segment_gather_f64']
    # r_cutoff: a float in the float32 entry points, a double in the float64 ones
    assert sig['tfep_radial_expansion'][1][5] is _lib.c_float and sig['tfep_radial_expansion_f64'][1][5] is _lib.c_double
    f32, f64 = sig['tfep_radial_expansion_backward'][1], sig['tfep_radial_expansion_backward_f64'][1]
    assert len(f32) == len(f64) == 14 and f32[5] is _lib.c_float and f64[5] is _lib.c_double
    assert f32[:5] + f32[6:] == f64[:5] + f64[6:]
    assert sig['tfep_radial_expansion_backward_workspace_doubles'] == (_lib.c_int64, [_lib.c_int64, _lib.c_int])
    from tfep_amd.build import SOURCES
    assert 'graph_ops.hip' in SOURCES


def test_differentiable_is_opt_in():
    assert GaussianBasisExpansion.differentiable is False and BehlerParrinelloRadialExpansion.differentiable is False
    gb = GaussianBasisExpansion.from_range(4, 1.0, trainable_means=True, trainable_stds=True)
    bp = BehlerParrinelloRadialExpansion.from_range(2.0, 4, 2.0, trainable_stds=True)
    assert gb.differentiable is False and bp.differentiable is False
    bp.differentiable = True                                          # an instance attribute: the class keeps its default
    assert BehlerParrinelloRadialExpansion.differentiable is False
    assert list(gb.state_dict()) == ['_means', '_log_gammas'] and list(bp.state_dict()) == ['_log_gammas']
    assert inspect.signature(graph.unsorted_segment_sum).parameters['differentiable'].default is False
    import tfep_amd.torch_ops as t
    assert t.GRAPH_OPS == ('radial_expansion', 'radial_expansion_backward', 'segment_sum', 'segment_gather')
    for name in t.GRAPH_OPS:
        assert hasattr(torch.ops.tfep, name)


def test_differentiable_route_has_no_cpu_fallback():
    bp = BehlerParrinelloRadialExpansion.from_range(2.0, 4, 2.0, trainable_stds=True)
    bp.differentiable = True
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        bp(torch.rand(5))
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        graph.unsorted_segment_sum(torch.rand(4, 2), torch.tensor([0, 1, 0, 1]), 2, differentiable=True)
