"""Host tests (no GPU) of what tests/test_gpu_spline_f32.py rests on: the float64 restatement tests/spline_ref.py against the
numpy oracle and the fixtures, and the cases of tests/spline_cases.py -- that the edge rows are what their names say, that
the knot rows are clear of their knots, and that the reference's own gradients are stable enough to judge the kernels by."""
import json

import numpy as np
import pytest
import torch

import golden_util as gu
import spline_cases as sc
import spline_ref
from oracle import transformers as otr

F64 = torch.float64
TOL = 1e-12


def _sentinel(q, bins, inverse):
    """(B, D): for an element in a tail, the magnitude of the sentinel knot that the oracle (like the reference) places 1000
    domain widths out and evaluates the tail from -- ``x0 -+ 1000 W`` in x, the boundary slope times that in y; 0 inside."""
    K = q['K']
    kx, ky, _, _ = spline_ref.knots(q)
    dx = 1000.0 * (kx[:, K] - kx[:, 0])
    lower = bins < 0
    if inverse:
        mag = torch.where(lower, (kx[:, 0] - dx).abs(), (kx[:, K] + dx).abs())
    else:
        mag = torch.where(lower, (ky[:, 0] - q['d'][:, 0] * dx).abs(), (ky[:, K] + q['d'][:, K] * dx).abs())
    return torch.where(lower | (bins >= K), mag, torch.zeros_like(mag)).detach()


def _agree(what, got, ldj, ref, ref_ldj, sentinel):
    """Every element of the values and the log-det of every sample, in units of max(1, |ref|), to 1e-12.  A tail element of
    the oracle is a difference of numbers of the sentinel knot's magnitude (5500 times the boundary slope here), each
    rounded at that size, which the restatement's linear tail never forms: four float64 roundings of that magnitude,
    ``2^-50 |sentinel|``, are allowed on top there -- from the oracle's formulation, not from what was seen."""
    ref, ref_ldj = torch.as_tensor(ref), torch.as_tensor(ref_ldj)
    e_y = float(((got.detach() - ref).abs() / (TOL * ref.abs().clamp(min=1.0) + 2.0 ** -50 * sentinel)).max())
    e_l = float(((ldj.detach() - ref_ldj).abs() / (TOL * ref_ldj.abs().clamp(min=1.0))).max())
    assert e_y <= 1.0 and e_l <= 1.0, (what, e_y, e_l)
    return e_y, e_l


def test_the_restatement_agrees_with_the_oracle_on_every_case():
    worst = (0.0, 0.0)
    for name in sc.NAMES:
        c = sc.case(name)
        kw = {k: (v.double().numpy() if isinstance(v, torch.Tensor) else v) for k, v in sc.flags(c).items()}
        args = (c['par'].double().numpy(), c['x0'].double().numpy(), c['xf'].double().numpy(), c['K'])
        q = spline_ref.intermediates(c['par'].double(), c['x0'], c['xf'], c['K'], **sc.flags(c))
        for key, fn, v in (('fwd', otr.spline_forward, c['x']), ('inv', otr.spline_inverse, c['yin'])):
            out, ldj = fn(v.double().numpy(), *args, **kw)
            e = _agree((name, key), c[key]['out'], c[key]['ldj'], out, ldj, _sentinel(q, c[key]['bins'], key == 'inv'))
            worst = tuple(max(a, b) for a, b in zip(worst, e))
    print(f'restatement against the oracle, largest over {len(sc.NAMES)} cases: per element {worst[0]:.3f}, log-det {worst[1]:.3f} of the bound')


@pytest.mark.parametrize('name', sorted(json.loads(str(gu.load('transformers.npz')['spline/meta']))))
def test_the_restatement_agrees_with_the_fixtures(name):
    g = gu.load('transformers.npz')
    meta = json.loads(str(g['spline/meta']))[name]
    t = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=F64)     # noqa: E731
    cfg = dict(y0=t(meta['y0']), yf=t(meta['yf']), circular=meta['circular'],
               identity_boundary_slopes=meta['identity_boundary_slopes'], learn_lower_bound=meta['learn_lower_bound'],
               learn_upper_bound=meta['learn_upper_bound'])
    par = torch.from_numpy(g[name + '/par']).double()
    assert par.shape[1] == meta['P'] * len(meta['x0'])
    assert meta['P'] == spline_ref.n_parameters_per_feature(meta['n_bins'], *list(cfg.values())[2:])
    args = (par, t(meta['x0']), t(meta['xf']), meta['n_bins'])
    y, ld, bins, q = spline_ref.forward_elements(torch.from_numpy(g[name + '/x']).double(), *args, **cfg)
    _agree((name, 'fwd'), y, ld.sum(dim=1), g[name + '/y_f64'], g[name + '/ldj_f64'], _sentinel(q, bins, False))
    x, ld, bins, q = spline_ref.inverse_elements(torch.from_numpy(g[name + '/inv_in']).double(), *args, **cfg)
    _agree((name, 'inv'), x, ld.sum(dim=1), g[name + '/xinv_f64'], g[name + '/ldjinv_f64'], _sentinel(q, bins, True))


def test_every_case_is_finite_and_small():
    assert len(set(sc.NAMES)) == len(sc.NAMES) == 60 + 16 + 24 + 8
    for name in sc.NAMES:
        c = sc.case(name)
        B, D, P = c['B'], c['D'], c['P']
        assert B <= 5 and D <= 130 and c['K'] in sc.TIERS + (4, 5)
        assert all(c[k].dtype == torch.float32 for k in ('x0', 'xf', 'y0', 'yf', 'par', 'x', 'yin', 'gy', 'gl')), name
        assert c['par'].shape == (B, P * D) and c['x'].shape == c['yin'].shape == c['gy'].shape == (B, D) and c['gl'].shape == (B,)
        for key in ('fwd', 'inv'):
            r = c[key]
            assert all(r[k].dtype == F64 and bool(torch.isfinite(r[k]).all()) for k in ('out', 'ld', 'ldj', 'out_bound', 'ld_bound')), (name, key)
            assert bool((r['out_bound'] > 0).all()) and bool((r['ld_bound'] > 0).all())
        assert all(bool(torch.isfinite(g).all()) for g in c['grad'])
        assert c['grad'][0].shape == (B, D) and c['grad'][1].shape == (B, P * D) and float(c['grad'][1].norm()) > 0


def test_the_builder_is_deterministic():
    for name in ('r_k8_d65_b5', 'r_k32_d130_b1', 'l_circ_k8', 'l_identboth_k17', 's_1100_k5', 's_0110_k8', 'e_rows_k17', 'e_narrow_k8', 'e_slopes_k8'):
        a = sc.case(name)
        sc.case.cache_clear()
        b = sc.case(name)
        assert a is not b
        for k in ('par', 'x', 'yin', 'gy', 'gl', 'x0', 'xf', 'y0', 'yf'):
            assert torch.equal(a[k], b[k]), (name, k)
        for key in ('fwd', 'inv'):
            assert all(torch.equal(a[key][k], b[key][k]) for k in a[key]), (name, key)
        assert all(torch.equal(s, t) for s, t in zip(a['grad'], b['grad']))


def test_the_random_cases_keep_to_their_recipe():
    """|raw slope + offset| <= 8, every bin at least 1e-2 of the domain, inputs in both tails and inside; circular cases at
    least 1e-3 of the period away from the wrap point, in both directions."""
    for name in sc.RANDOM + sc.LAYOUT + sc.SHARED:
        c = sc.case(name)
        B, K, D, P = c['B'], c['K'], c['D'], c['P']
        circ, ident, lo, up = c['layout']
        p = c['par'].double().reshape(B, P, D)
        n_slopes = K - 1 if ident else (K if circ else K + 1)
        assert float((p[:, 2 * K:2 * K + n_slopes] + sc.SLOPE_OFFSET).abs().max()) <= 8.0, name
        q = spline_ref.intermediates(c['par'].double(), c['x0'], c['xf'], K, **sc.flags(c))
        kx, ky, widths, heights = spline_ref.knots(q)
        assert bool((widths >= 1e-2 * (kx[:, -1:] - kx[:, :1])).all()) and bool((heights >= 1e-2 * (ky[:, -1:] - ky[:, :1])).all()), name
        if circ:
            period = (c['xf'] - c['x0']).double()
            u = torch.remainder(c['x'].double() - c['x0'].double() + q['shift'], period) / period
            pre = spline_ref.evaluate(c['yin'].double(), q, inverse=True)[0]
            r = torch.remainder(pre - c['x0'].double() - q['shift'], period) / period
            assert all(float(t.min()) >= 1e-3 and float(t.max()) <= 1 - 1e-3 for t in (u, r)), name
            assert bool(((c['fwd']['bins'] >= 0) & (c['fwd']['bins'] < K)).all())
        elif B * D >= 63:
            for key in ('fwd', 'inv'):
                bins = c[key]['bins']
                assert bool((bins < 0).any()) and bool((bins >= K).any()) and bool(((bins >= 0) & (bins < K)).any()), (name, key)
    assert all(bool((sc.case(n)['par'] == sc.case(n)['par'][:1]).all()) for n in sc.SHARED)
    import test_gpu_torch_ops
    assert set(sc.FUSED_LAYOUTS) == set(test_gpu_torch_ops._FUSED_LAYOUTS) | {(8, False, False, False, False)} and len(sc.FUSED_LAYOUTS) == 24
    assert [(sc.case(n)['K'], *sc.case(n)['layout']) for n in sc.SHARED] == list(sc.FUSED_LAYOUTS)
    # every layout is there, and the y-domain of the random cases is one of its own
    assert {sc.case(n)['layout'] for n in sc.LAYOUT} == set(sc.LAYOUTS.values()) and len(set(sc.LAYOUTS.values())) == 8
    assert not torch.equal(sc.case('r_k8_d65_b5')['y0'], sc.case('r_k8_d65_b5')['x0'])


@pytest.mark.parametrize('K', sc.TIERS)
def test_the_edge_rows_are_what_their_names_say(K):
    c = sc.case(f'e_rows_k{K}')
    D = c['D']
    assert bool((c['par'] == c['par'][:1]).all())                                   # one row of parameters
    q = spline_ref.intermediates(c['par'].double(), c['x0'], c['xf'], K, **sc.flags(c))
    kx, ky, _, _ = spline_ref.knots(q)
    even = torch.arange(D) % 2 == 0
    j = sc.knot_of_feature(K, D)
    for key, v, kn in (('fwd', c['x'], kx[0]), ('inv', c['yin'], ky[0])):
        bins = c[key]['bins']
        below, mid, above = v[0], v[1], v[2]
        assert torch.equal(torch.nextafter(mid, torch.full_like(mid, -np.inf)), below)
        assert torch.equal(torch.nextafter(mid, torch.full_like(mid, np.inf)), above)
        if K > 1:
            knot = torch.gather(kn, 0, j[None])[0]
            assert bool((below.double() < knot).all()) and bool((above.double() > knot).all())
            assert bool(((mid.double() - knot).abs() <= 0.5 * (above.double() - below.double()) * 0.5 + 1e-15).all())   # the nearest
            # the bin of ``v`` is #{knots < v} - 1: below the knot bin j - 1, above it bin j, on its nearest float by the comparison
            assert torch.equal(bins[0], j - 1) and torch.equal(bins[2], j)
            assert torch.equal(bins[1], torch.where(mid.double() > knot, j, j - 1))
            # clear of EVERY knot by the margin
            dist = (v[:3, None, :].double() - kn[None]).abs().amin(dim=(0, 1))
            assert bool((dist >= sc.knot_margin(c)).all()), float((dist / sc.knot_margin(c)).min())
        else:
            assert bool((bins[:3] == 0).all())
        # row 3: on the first knot the lower tail (strict >), on the last one the last bin or -- where the float64 sum of
        # the widths comes out an ulp short of the float32 xf -- the upper tail; the map is continuous there
        if key == 'fwd':
            assert torch.equal(v[3], torch.where(even, c['x0'], c['xf']))
        else:
            assert torch.equal(v[3], torch.where(even, c['y0'], c['yf']))
        assert bool((bins[3][even] == -1).all()) and bool((bins[3][~even] >= K - 1).all())
        assert bool((bins[4][even] == -1).all()) and bool((bins[4][~even] == K).all())
    assert bool((c['x'][4].abs() == 1e3).all()) and float(c['fwd']['out'][4].abs().min()) > 50.0
    assert sc.rel_l2(c['inv']['out'][4], c['x'][4]) <= 2.0 ** -22                     # yin row 4: the image of x row 4
    assert float(c['gl'][3]) == 0.0 and bool((c['gl'][[0, 1, 2, 4]] != 0).all())
    assert sc.rel_l2(c['fwd']['out'][3], torch.where(even, c['y0'], c['yf'])) <= 1e-15


def test_the_narrow_bin_and_the_slope_rows():
    c = sc.case('e_narrow_k8')
    q = spline_ref.intermediates(c['par'].double(), c['x0'], c['xf'], 8, **sc.flags(c))
    _, _, widths, heights = spline_ref.knots(q)
    for t in (widths, heights):
        assert bool((t[:, 0] > sc.MIN_BIN).all()) and bool((t[:, 0] < 1.1 * sc.MIN_BIN).all())
        assert float(t[:, 1:].min()) > 1e-2
    assert bool((c['fwd']['bins'][:3] == 0).all()) and bool((c['inv']['bins'][:3] == 0).all())
    c = sc.case('e_slopes_k8')
    raw = c['par'].reshape(5, c['P'], c['D'])[:, 16:25]
    assert int((raw == 25.0).sum()) == 5 * 5 * 33 and int((raw == -25.0).sum()) == 5 * 4 * 32
    d = spline_ref.intermediates(c['par'].double(), c['x0'], c['xf'], 8, **sc.flags(c))['d']
    assert abs(float(d.max()) - (25.0 + sc.SLOPE_OFFSET + sc.MIN_SLOPE)) < 1e-12    # past the threshold: the identity
    assert sc.MIN_SLOPE < float(d.min()) < sc.MIN_SLOPE * (1 + 1e-6)
    f, rows = torch.arange(c['D']), torch.arange(3)[:, None]
    for key in ('fwd', 'inv'):
        assert torch.equal(c[key]['bins'][:3], (f[None] + rows) % 8)
        assert bool((c[key]['bins'][3] == -1).all()) and bool((c[key]['bins'][4] == 8).all())


def test_grad_dropped_matches_the_measurement():
    """``GRAD_DROPPED`` holds exactly the cases whose reference gradient moves by more than 2^-18 under the error model
    (``spline_cases.grad_movement``), two at the most."""
    over = []
    worst = 0.0
    for name in sc.NAMES:
        m = max(sc.grad_movement(name))
        worst = max(worst, m)
        if name in sc.EDGE:
            print(f'{name}: the reference gradient moves by {m / sc.GRAD_DROP_ABOVE:.3f} x 2^-18')
        if m > sc.GRAD_DROP_ABOVE:
            over.append(name)
    print(f'largest over the {len(sc.NAMES)} cases: {worst / sc.GRAD_DROP_ABOVE:.3f} x 2^-18')
    assert tuple(over) == tuple(sc.GRAD_DROPPED) and len(sc.GRAD_DROPPED) <= 2


def test_round_trip_in_float64():
    for name in sc.NAMES:
        c = sc.case(name)
        args = (c['par'].double(), c['x0'], c['xf'], c['K'])
        y, l = spline_ref.spline_forward(c['x'].double(), *args, **sc.flags(c))
        x, li = spline_ref.spline_inverse(y, *args, **sc.flags(c))
        e = sc.rel_l2(x, c['x'])
        el = float(((l + li).abs() / l.abs().clamp(min=1.0)).max())
        assert e <= TOL and el <= TOL, (name, e, el)
