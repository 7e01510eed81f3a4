"""Host tests (no GPU) of what tests/test_gpu_moebius_f32.py rests on: the cases of tests/moebius_cases.py and their float64
reference, the stability of that reference where the map is stiffest, how much of the fixtures' 1e-5 was input rounding,
and the torch restatement of the split-f16 side output."""
import json

import numpy as np
import pytest
import torch

import golden_util as gu
import moebius_cases as mc
import moebius_ref

F64 = torch.float64


def test_every_reference_value_and_gradient_is_finite():
    assert len(set(mc.NAMES)) == len(mc.NAMES) == 40 + 11
    for name in mc.NAMES:
        c = mc.case(name)
        assert all(c[k].dtype == torch.float32 for k in ('x', 'w', 'gy', 'gl')), name
        assert c['x'].numel() <= 5 * 520 and c['x'].shape == c['w'].shape == c['gy'].shape and c['gl'].shape == (c['B'],)
        for key in ('fwd', 'inv'):
            assert all(t.dtype == F64 and bool(torch.isfinite(t).all()) for t in c[key]), (name, key)
            assert c[key][0].shape == c['x'].shape and c[key][1].shape == (c['B'],)
        if c['unit_sphere']:
            norms = c['x'].double().reshape(c['B'], -1, c['dim']).norm(dim=-1)
            assert float((norms - 1).abs().max()) <= 2.0 ** -23, name          # float32 rounding of a unit vector


def test_the_edge_rows_are_what_their_names_say():
    for dim in (2, 3):
        for u in (0, 1):
            c = mc.case(f'e_wbig_d{dim}_u{u}')
            xv, wv = (c[k].double().reshape(3, 2, dim) for k in ('x', 'w'))
            cos = (xv * wv).sum(-1) / (xv.norm(dim=-1) * wv.norm(dim=-1))
            assert torch.allclose(wv.norm(dim=-1), torch.full((3, 2), 1e4, dtype=F64), rtol=1e-6)
            assert bool((cos[0] >= 1 - 1e-12).all()) and bool((cos[1] <= -1 + 1e-12).all()) and bool((cos[2].abs() <= 1e-7).all())
            # c = N / |d|^2 of the parallel row: (1 + r) / (1 - r) with r = 0.99 1e4 / (1 + 1e4)
            r = 0.99 * 1e4 / (1 + 1e4)
            ldj = c['fwd'][1][0]
            want = 2 * (dim if u else dim - 1) * np.log((1 + r) / (1 - r))
            assert abs(float(ldj) - want) <= 1e-4 * want, (dim, u, float(ldj), want)
            z = mc.case(f'e_wzero_d{dim}_u{u}')
            zero = (z['w'].reshape(3, 3, dim) == 0).all(-1)
            assert zero.tolist() == [[False] * 3, [True] * 3, [True, False, False]]
            # w = 0: the identity (on the sphere x / |x|^2, with |x| = 1 to a float32 ulp)
            tol = 2.0 ** -22 if u else 1e-15
            assert mc.rel_l2(z['fwd'][0][1], z['x'][1]) <= tol and float(z['fwd'][1][1].abs()) <= 2 * dim * 3 * tol
        s = mc.case(f'e_xscale_d{dim}_u0')
        norms = s['x'].double().reshape(2, 2, dim).norm(dim=-1)
        assert torch.allclose(norms[0], torch.full((2,), 1e-6, dtype=F64), rtol=1e-6)
        assert torch.allclose(norms[1], torch.full((2,), 1e4, dtype=F64), rtol=1e-6)
    assert mc.case('e_r07_d3_u0')['max_radius'] == 0.7 and all(mc.case(n)['max_radius'] == 0.99 for n in mc.NAMES[:-1])


def test_dimension_one_off_the_sphere_is_the_identity_map():
    """``(|x|^2 - u^2) / (x - u) - u = x`` for every ``w``: the parameter gradient is exactly zero and both sides of a
    comparison hold round-off only, which ``grad_errors`` measures absolutely, in units of the cotangents' norm."""
    for name in mc.RANDOM:
        c = mc.case(name)
        if not mc.identity_parameter_gradient(c):
            continue
        assert c['dim'] == 1 and not c['unit_sphere']
        for key in ('fwd', 'inv'):
            y, l, gx, gw = c[key]
            assert mc.rel_l2(y, c['x']) <= 1e-15 and float(l.abs().max()) <= 1e-13 * c['nvec']
            assert float(gw.norm()) <= 1e-12 * mc.cotangent_norm(c), (name, key)
            assert mc.rel_l2(gx, c['gy']) <= 1e-11
            ex, ew = mc.grad_errors(c, key, gx, gw)
            assert ex == 0.0 and ew == float(gw.norm()) / mc.cotangent_norm(c)
    assert sum(mc.identity_parameter_gradient(mc.case(n)) for n in mc.NAMES) == len(mc.SHAPES)


def test_the_builder_is_deterministic():
    for name in ('r_d2_u1_b5_n65', 'r_d5_u0_b1_n1', 'e_wbig_d3_u0', 'e_xscale_d2_u0', 'e_r07_d3_u0'):
        a = mc.case(name)
        mc.case.cache_clear()
        b = mc.case(name)
        assert a is not b
        for k in ('x', 'w', 'gy', 'gl'):
            assert torch.equal(a[k], b[k]), (name, k)
        for key in ('fwd', 'inv'):
            assert all(torch.equal(s, t) for s, t in zip(a[key], b[key])), (name, key)


def test_the_reference_gradients_are_stable_where_the_map_is_stiffest():
    """The rows with c = 197 amplify fp64 round-off by a few orders of magnitude.  The reference's own gradients, run again
    at inputs moved by one float64 ulp, must stay within 1 % of the 2^-22 the kernels are held to; a case where they do not
    is left out of the gradient comparison, by name, in ``moebius_cases.GRAD_DROPPED`` (two at the most)."""
    unstable = []
    for name in mc.NAMES:
        ratio = mc.reference_stability(name)
        if name in mc.EDGE:
            print(f'{name}: the reference gradient moves by {ratio:.3e} x 2^-22 under one float64 ulp')
        if ratio > 0.01:
            unstable.append(name)
    worst = max(mc.reference_stability(n) for n in mc.NAMES)
    print(f'largest over the {len(mc.NAMES)} cases: {worst:.3e} x 2^-22')
    assert tuple(unstable) == tuple(mc.GRAD_DROPPED) and len(mc.GRAD_DROPPED) <= 2


@pytest.mark.parametrize('name', ['d2_u0', 'd2_u1', 'd3_u0', 'd3_u1'])
def test_how_much_of_the_fixtures_bound_was_input_rounding(name):
    """The reference at the fixtures' inputs rounded to float32 against the fixtures' float64 outputs: the share of the 1e-5
    of tests/test_gpu_parity.py::test_moebius that input rounding explains (printed; no gate on the kernels).  A relative
    input error of 2^-24 would reach the output multiplied by the map's Lipschitz factor, at most (1 + R) / (1 - R) = 199:
    1.2e-5 at the worst.  Measured: the fixtures' inputs ARE float32 numbers, stored as such, so rounding moves nothing
    and none of the 1e-5 was input rounding -- the reference agrees with the fixtures to float64 round-off."""
    g = gu.load('transformers.npz')
    meta = json.loads(str(g['moebius/meta']))[f'moebius/{name}']
    lipschitz = (1 + meta['max_radius']) / (1 - meta['max_radius'])
    for inp, fn, out, ldj in (('x', moebius_ref.moebius, 'y_f64', 'ldj_f64'), ('inv_in', moebius_ref.moebius_inverse, 'xinv_f64', 'ldjinv_f64')):
        x64, p64 = (torch.from_numpy(g[f'moebius/{name}/{k}']).double() for k in (inp, 'par'))
        x32, p32 = x64.float().double(), p64.float().double()
        y, l = fn(x32, p32, **meta)
        ref_y, ref_l = torch.from_numpy(g[f'moebius/{name}/{out}']), torch.from_numpy(g[f'moebius/{name}/{ldj}'])
        ey = mc.rel_l2(y, ref_y)
        el = float(((l - ref_l).abs() / ref_l.abs().clamp(min=1.0)).max())
        moved = max(mc.rel_l2(x32, x64), mc.rel_l2(p32, p64))
        print(f'{name} {out}: inputs moved by {moved:.3e}; y moves by {ey:.3e} (rel L2), log-det by {el:.3e}: '
              f'{ey / 1e-5:.1%} and {el / 1e-5:.1%} of 1e-5')
        if moved == 0.0:                                       # (fixtures whose inputs are float32 numbers already)
            assert ey <= 1e-12 and el <= 1e-11
        else:
            assert 0.0 < ey <= 2.0 ** -24 * (1 + lipschitz) and el <= 2.0 ** -24 * 2 * lipschitz * y.shape[1]


def test_the_split_restatement_reconstructs_y():
    """``hi + lo`` of ``moebius_cases.split_halves`` against ``y`` for random ``|y| <= 1``, down to values whose lo half is a
    float16 subnormal, and the group layout of ``split_decode`` against a row laid out by hand."""
    gen = torch.Generator().manual_seed(0)
    y = torch.cat([2 * torch.rand(5, 256, generator=gen) - 1,
                   (2 * torch.rand(5, 256, generator=gen) - 1) * 10.0 ** -torch.randint(1, 9, (5, 256), generator=gen).float(),
                   torch.tensor([[1.0, -1.0, 0.0, 2.0 ** -14, 1 - 2.0 ** -24, 2.0 ** -30, 0.5 + 2.0 ** -13, -0.3]]).expand(5, 8)], dim=1)
    assert float(y.abs().max()) <= 1.0
    hi, lo = mc.split_halves(y)
    assert hi.dtype == torch.float16 and lo.dtype == torch.float16
    err = (mc.split_reconstruct(hi, lo) - y.double()).abs()
    worst = float((err / mc.split_bound(y)).max())
    print(f'largest reconstruction error: {worst:.3f} of the bound 2^-22 |y| + 2^-39')
    assert bool((err <= mc.split_bound(y)).all())
    assert float(err.max()) > 0                                  # (a bound of zero would not do: lo rounds)
    # hi alone is the float16 of t: 11 significant bits
    assert bool(((hi.double() / mc.SPLIT_SCALE - y.double()).abs() <= 2.0 ** -11 * y.double().abs() + 2.0 ** -39).all())
    # the layout: per 8 features 8 hi halves, then 8 lo halves; words past D are padding
    B, D, cols = 5, 520, 576
    row = torch.zeros(B, 2 * cols, dtype=torch.float16)
    for g_ in range(D // 8):
        row[:, 16 * g_:16 * g_ + 8] = hi[:, 8 * g_:8 * g_ + 8]
        row[:, 16 * g_ + 8:16 * g_ + 16] = lo[:, 8 * g_:8 * g_ + 8]
    buf = row.view(torch.float32)
    assert buf.shape == (B, cols)
    h2, l2, padding = mc.split_decode(buf, D)
    assert torch.equal(h2, hi) and torch.equal(l2, lo) and padding.shape == (B, cols - D) and bool((padding == 0).all())
