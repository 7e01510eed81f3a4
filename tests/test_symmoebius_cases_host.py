"""Host tests (no GPU) of what tests/test_gpu_symmoebius_f32.py rests on: the cases of tests/symmoebius_cases.py and their
float64 reference (tests/symmoebius_ref.py) held to the map's own conditions, the inverse-function-theorem gradients against
autograd, the closed form of ``tfep_amd/csrc/symmoebius.h`` (restated here, and only here) against the reference's
formulae, the stability of the reference where the map is stiffest, and how much of the goldens' 1e-5 was input rounding."""
import numpy as np
import pytest
import torch

import golden_util as gu
import symmoebius_cases as sc
import symmoebius_ref as ref

F64 = torch.float64
BOUND = 2.0 ** -22


def _vec(t, c):
    return t.double().reshape(c['B'], c['nvec'], c['dim'])


def test_every_reference_value_and_gradient_is_finite():
    assert len(set(sc.NAMES)) == len(sc.NAMES) == 20 + 12 + 5
    for name in sc.NAMES:
        c = sc.case(name)
        assert all(c[k].dtype == torch.float32 for k in ('x', 'w', 'gy', 'gl')), name
        assert c['x'].numel() <= 5 * 65 * 8 and c['x'].shape == c['w'].shape == c['gy'].shape and c['gl'].shape == (c['B'],)
        assert float(_vec(c['x'], c).norm(dim=-1).min()) > 0, name                 # x = 0 is left out
        for key in ('fwd', 'inv'):
            assert all(t.dtype == F64 and bool(torch.isfinite(t).all()) for t in c[key]), (name, key)
            assert c[key][0].shape == c[key][2].shape == c[key][3].shape == c['x'].shape and c[key][1].shape == (c['B'],)
        if name in sc.RANDOM or 'r07' in name or 'xscale' in name:
            assert not bool(ref.degenerate(c['x'].double(), c['w'].double(), c['dim']).any()), name
    assert all(sc.case(n)['max_radius'] == (0.7 if 'r07' in n else 0.99) for n in sc.NAMES)


def test_the_edge_rows_are_what_their_names_say():
    r = 0.99 * sc.WBIG / (1 + sc.WBIG)
    for dim in sc.EDGE_DIMS:
        c = sc.case(f'e_wbig_d{dim}')
        xv, wv = _vec(c['x'], c), _vec(c['w'], c)
        assert c['B'] == 3 and c['nvec'] == 2
        x64, w64 = sc.wbig_rows(dim)
        assert torch.equal(c['x'].double(), x64) and torch.equal(c['w'].double(), w64)        # float32 numbers as written
        cos = (xv * wv).sum(-1) / (xv.norm(dim=-1) * wv.norm(dim=-1))
        assert torch.allclose(wv.norm(dim=-1), torch.full((3, 2), sc.WBIG, dtype=F64), rtol=2.0 ** -20, atol=0)
        assert float((cos[0] - 1).abs().max()) <= 1e-15 and float((cos[1] + 1).abs().max()) <= 1e-15
        assert bool((cos[2] == 0).all())                       # integer dot products: exactly orthogonal
        # exactly parallel in the float32 numbers the kernel reads: every 2 x 2 minor vanishes (products exact in float64)
        minors = xv[:2].unsqueeze(-1) * wv[:2].unsqueeze(-2) - xv[:2].unsqueeze(-2) * wv[:2].unsqueeze(-1)
        assert bool((minors == 0).all())
        deg = ref.degenerate(c['x'].double(), c['w'].double(), dim)
        assert deg.tolist() == [[True, True], [True, True], [False, False]]
        # the poles are fixed points of the forward restatement; log-det there: (1 + r2)^(d-1) / (1 - r2)^(d-1) per vector
        y, l = c['fwd'][0], c['fwd'][1]
        assert sc.rel_l2(y[:2], c['x'][:2]) <= 1e-12
        want = 2 * (dim - 1) * np.log((1 + r * r) / (1 - r * r))
        assert abs(float(l[0]) - want) <= 1e-5 * want and abs(float(l[1]) - want) <= 1e-5 * want, (dim, l, want)
        H_pole = (1 - r * r) ** 2
        assert 3.5e-4 < H_pole < 4.5e-4
        # the inverse there: the point itself, minus the forward log-det
        assert torch.equal(c['inv'][0][:2], c['x'][:2].double()) and torch.equal(c['inv'][1][:2], -l[:2])

        z = sc.case(f'e_wzero_d{dim}')
        assert z['wzero'].tolist() == [[False] * 3, [True] * 3, [True, False, False]]
        assert torch.equal(ref.degenerate(z['x'].double(), z['w'].double(), dim), z['wzero'])
        for key in ('fwd', 'inv'):                             # w = 0: the identity, log-det 0, no parameter gradient
            y, l, gx, gw = z[key]
            assert sc.rel_l2(y[1], z['x'][1]) <= 1e-15 and float(l[1].abs()) <= 1e-14
            assert float(_vec(gw, z)[z['wzero']].abs().max()) <= 1e-14 * sc.cotangent_norm(z), (dim, key)
            assert sc.rel_l2(gx[1], z['gy'][1]) <= 1e-14
            assert sc.wzero_gradient_error(z, key, gw) <= 1e-14

        s = sc.case(f'e_xscale_d{dim}')
        norms = _vec(s['x'], s).norm(dim=-1)
        assert torch.allclose(norms[0], torch.full((2,), 1e-6, dtype=F64), rtol=1e-6)
        assert torch.allclose(norms[1], torch.full((2,), 1e4, dtype=F64), rtol=1e-6)


def test_the_restatements_meet_the_conditions_of_the_map():
    """To 1e-12 relative, on every case: ``inverse(forward(x)) = x`` and the log-dets cancel, ``|y| = |x|`` per vector in
    both directions, and the map is even in ``w``."""
    for name in sc.NAMES:
        c = sc.case(name)
        x, w, dim, R = c['x'].double(), c['w'].double(), c['dim'], c['max_radius']
        for key, fn in (('fwd', ref.symmetrized_moebius), ('inv', ref.symmetrized_moebius_inverse)):
            y, l = c[key][0], c[key][1]
            nx, ny = _vec(x, c).norm(dim=-1), _vec(y, c).norm(dim=-1)
            assert float(((ny - nx).abs() / nx).max()) <= 1e-12, (name, key)
            y2, l2 = fn(x, -w, dim, R)
            assert sc.rel_l2(y2, y) <= 1e-12 and float((l2 - l).abs().max()) <= 1e-12 * max(1.0, float(l.abs().max())), (name, key)
        xb, lb = ref.symmetrized_moebius_inverse(c['fwd'][0], w, dim, R)
        per_vec = (_vec(xb, c) - _vec(x, c)).norm(dim=-1) / _vec(x, c).norm(dim=-1)
        assert float(per_vec.max()) <= 1e-12, (name, float(per_vec.max()))
        assert float((lb + c['fwd'][1]).abs().max()) <= 1e-12 * max(1.0, float(lb.abs().max())), name
        yf, lf = ref.symmetrized_moebius(c['inv'][0], w, dim, R)
        per_vec = (_vec(yf, c) - _vec(x, c)).norm(dim=-1) / _vec(x, c).norm(dim=-1)
        assert float(per_vec.max()) <= 1e-12 and float((lf + c['inv'][1]).abs().max()) <= 1e-12 * max(1.0, float(lf.abs().max())), name


def test_inverse_function_theorem_gradients_equal_autograd_on_the_random_cases():
    """The construction that gives the inverse's gradients at the degenerate vectors, on vectors where autograd through the
    reference's plane solution is defined too: every vector of the small random cases, the first and the 65th vector of
    every row of the ``n65`` ones."""
    worst = 0.0
    for name in sc.RANDOM + tuple(n for n in sc.EDGE if 'r07' in n):
        c = sc.case(name)
        mask = torch.ones(c['B'], c['nvec'], dtype=torch.bool)
        if c['nvec'] == 65:
            mask[:, 1:64] = False
        gx, gw = ref.ift_gradients_all(c['inv'][0], c['w'].double(), c['gy'].double(), c['gl'].double(), c['dim'], c['max_radius'], mask)
        keep = mask.unsqueeze(-1).expand(-1, -1, c['dim']).reshape(gx.shape)
        ex, ew = sc.rel_l2(gx[keep], c['inv'][2][keep]), sc.rel_l2(gw[keep], c['inv'][3][keep])
        worst = max(worst, ex, ew)
        assert ex <= 1e-12 and ew <= 1e-12, (name, ex, ew)
    print(f'inverse-function theorem against autograd, largest relative L2: {worst:.3e}')


def closed_form(x, w, dim, R, inverse):
    """The closed form of ``tfep_amd/csrc/symmoebius.h:5-13`` in float64 torch: ``y = (alpha x + beta p u) / sqrt(H)``."""
    B = x.shape[0]
    xv, wv = x.reshape(B, -1, dim), w.reshape(B, -1, dim)
    u = R / (1 + wv.norm(dim=-1, keepdim=True)) * wv
    r2 = (u * u).sum(-1, keepdim=True)
    p = (xv * u).sum(-1, keepdim=True)
    t2 = p * p / (xv * xv).sum(-1, keepdim=True)
    c1, c2 = 1 - r2, 1 + r2
    if inverse:
        alpha, beta, H, numer = c1, 2.0, c1 * c1 + 4 * t2, c1 ** (dim - 1) * c2
    else:
        alpha, beta, H, numer = c2, -2.0, c1 * c1 + 4 * (r2 - t2), c1 * c2 ** (dim - 1)
    y = (alpha * xv + beta * p * u) / H.sqrt()
    return y.reshape(B, -1), (numer.log() - 0.5 * dim * H.log()).squeeze(-1).sum(1)


def test_the_kernels_closed_form_is_the_reference_map():
    """The kernels evaluate a closed form of this project's own, in both directions.  Here it is held to the restatement of
    the reference's formulae on every case -- the poles and ``w = 0`` included, where the reference's inverse is 0 / 0 and the
    restatement takes the inverse through the forward map -- to 1 % of every bound of the GPU test: values per tensor and
    per element, log-det per row, gradients per tensor.  That is what licenses 2^-22 for the kernels, which round an fp64
    evaluation of this form once."""
    worst = dict(y=0.0, el=0.0, ld=0.0, g=0.0)
    for name in sc.NAMES:
        c = sc.case(name)
        dim, R = c['dim'], c['max_radius']
        for key, inverse in (('fwd', False), ('inv', True)):
            xr, wr = c['x'].double().requires_grad_(True), c['w'].double().requires_grad_(True)
            y, l = closed_form(xr, wr, dim, R, inverse)
            ((y * c['gy'].double()).sum() + (l * c['gl'].double()).sum()).backward()
            y_ref, l_ref = c[key][0], c[key][1]
            floor = 1e-6 * _vec(y_ref, c).abs().amax(dim=-1, keepdim=True).expand(-1, -1, dim).reshape(y_ref.shape)
            e_y = sc.rel_l2(y, y_ref)
            e_el = float(((y.detach() - y_ref).abs() / torch.maximum(y_ref.abs(), floor)).max())
            e_ld = float(((l.detach() - l_ref).abs() / l_ref.abs().clamp(min=1.0)).max())
            e_g = max(sc.grad_errors(c, key, xr.grad, wr.grad))
            for k, e in (('y', e_y), ('el', e_el), ('ld', e_ld), ('g', e_g)):
                worst[k] = max(worst[k], e)
            assert max(e_y, e_el, e_ld, e_g) <= 0.01 * BOUND, (name, key, e_y, e_el, e_ld, e_g)
    print('closed form against the restatement, largest over the cases in units of 2^-22: '
          + ', '.join(f'{k} {v / BOUND:.2e}' for k, v in worst.items()))


def test_the_builder_is_deterministic():
    for name in ('r_d2_b5_n65', 'r_d5_b1_n1', 'e_wbig_d3', 'e_wzero_d4', 'e_xscale_d2', 'e_r07_d8'):
        a = sc.case(name)
        sc.case.cache_clear()
        b = sc.case(name)
        assert a is not b
        for k in ('x', 'w', 'gy', 'gl'):
            assert torch.equal(a[k], b[k]), (name, k)
        for key in ('fwd', 'inv'):
            assert all(torch.equal(s, t) for s, t in zip(a[key], b[key])), (name, key)


def test_the_reference_gradients_are_stable_where_the_map_is_stiffest():
    """At the poles of ``e_wbig`` ``H = (1 - r2)^2 = 4e-4``, and the Jacobian has the factor 100.  The reference's own gradients,
    run again at inputs moved by one float64 ulp, must stay within 1 % of the 2^-22 the kernels are held to; a case where
    they do not is left out of the gradient comparison, by name, in ``symmoebius_cases.GRAD_DROPPED`` (two at the most)."""
    unstable = []
    for name in sc.NAMES:
        ratio = sc.reference_stability(name)
        if name in sc.EDGE:
            print(f'{name}: the reference gradient moves by {ratio:.3e} x 2^-22 under one float64 ulp')
        if ratio > 0.01:
            unstable.append(name)
    worst = max(sc.reference_stability(n) for n in sc.NAMES)
    print(f'largest over the {len(sc.NAMES)} cases: {worst:.3e} x 2^-22 (|w| = {sc.WBIG:g} in e_wbig)')
    assert tuple(unstable) == tuple(sc.GRAD_DROPPED) and len(sc.GRAD_DROPPED) <= 2


@pytest.mark.parametrize('name', [f'd{d}_R{R}' for d in (2, 3, 4) for R in (0.99, 0.7)])
def test_how_much_of_the_goldens_bound_was_input_rounding(name):
    """The restatement at the golden's inputs rounded to float32 against the golden's float64 outputs: the share of the 1e-5
    of tests/test_gpu_symmoebius.py that input rounding explains (printed; no gate on the kernels).  A relative input
    error of 2^-24 reaches the output multiplied by the map's Lipschitz factor, at most (1 + R^2) / (1 - R^2) = 99.5:
    6e-6 at the worst.  The golden's inputs are stored as float32 numbers, so rounding moves nothing and none of the 1e-5
    was input rounding: the restatement agrees with the golden to float64 round-off."""
    g = gu.load('symmoebius.npz')
    d, R = int(name[1]), float(name.split('_R')[1])
    lipschitz = (1 + R * R) / (1 - R * R)
    for inp, inverse, out, ldj in (('x', False, 'y_f64', 'ldj_f64'), ('yin', True, 'y_inv_f64', 'ldj_inv_f64')):
        x64, p64 = (torch.from_numpy(g[f'tr/{name}/{k}']).double() for k in (inp, 'w'))
        x32, p32 = x64.float().double(), p64.float().double()
        y, l = ref.sym_torch(x32, p32, d, R, inverse)
        ref_y, ref_l = torch.from_numpy(g[f'tr/{name}/{out}']), torch.from_numpy(g[f'tr/{name}/{ldj}'])
        ey = sc.rel_l2(y, ref_y)
        el = float(((l - ref_l).abs() / ref_l.abs().clamp(min=1.0)).max())
        moved = max(sc.rel_l2(x32, x64), sc.rel_l2(p32, p64))
        print(f'{name} {out}: inputs moved by {moved:.3e}; y moves by {ey:.3e} (rel L2), log-det by {el:.3e}: '
              f'{ey / 1e-5:.1%} and {el / 1e-5:.1%} of 1e-5')
        if moved == 0.0:                                       # (a golden whose inputs are float32 numbers already)
            assert ey <= 1e-12 and el <= 1e-11
        else:
            assert 0.0 < ey <= 2.0 ** -24 * (1 + lipschitz) and el <= 2.0 ** -24 * 2 * lipschitz * y.shape[1]
