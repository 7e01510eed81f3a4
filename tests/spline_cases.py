"""Float32 inputs at which the float32 rational-quadratic spline kernels take every path -- ``rq_spline_element<KMAX, INVERSE>``
(KMAX = 8 / 16 / 32), ``rq_spline_forward_full<K>`` (the fused epilogue), ``rq_spline_inverse_selects`` (the blocked inverse),
``rq_spline_backward<KMAX>`` with its LDS-staged and unstaged parameter paths, and the two parameter expansions -- with the
float64 reference of ``tests/spline_ref.py`` evaluated on those very float32 numbers cast up: the rounding of the inputs
(the minimum bin size and slope included: both are float32 numbers) is no part of any error measured against it.  CPU only;
shared by ``test_spline_cases_host.py`` (the conditions the cases rest on) and ``test_gpu_spline_f32.py`` (the kernels).

Cases (at most 5 rows x 130 features)
-------------------------------------
* ``r_k{K}_d{D}_b{B}``: random, plain layout with ``y0 / yf`` of their own, K in 1, 8, 9, 16, 17, 32 (both ends of every KMAX
  instantiation), D in 1, 63, 64, 65, 130 (a partial wave, a full one, a second lane pass, a partial last stage of 64), B in
  1, 5 (five rows: one more than a workgroup holds).
* ``l_{layout}_k{K}``: one per distinct flag combination (``LAYOUTS``) at K = 8 and 17, 5 rows x 65 features.
* ``s_{flags}_k{K}``: every layout that has a fused epilogue (``FUSED_LAYOUTS``: K = 4, 5, 8), 5 rows x 65 features, one row of
  parameters shared by the 5 rows.
* ``e_rows_k{K}``: edge rows, written out and not drawn, plain layout, every K above, 5 rows x 65 features that share one
  row of parameters: rows 0 / 1 / 2 the float32 number below / nearest to / above interior knot ``1 + f mod (K - 1)`` of
  feature f (the x-knots for the forward input ``x``, the y-knots for the inverse input ``yin``; K = 1 has no interior knot:
  the three float32 numbers round the middle of the domain), row 3 ``x == x0`` (even f) and ``x == xf`` (odd f) exactly, row 4
  far out in the tails, ``x = -1e3`` (even f) and ``+1e3`` (odd f); ``yin``: the images of those.  The domain of the edge
  cases is [1.5, 7] (elsewhere [-3, 2.5]): next to zero the float32 neighbours of a knot are closer to it than the margin below.
* ``e_narrow_k8``: raw width and height 0 of every feature at -12, so that bin 0 is about ``min_bin_size`` wide (the first
  bin, and a domain [0, 1.1] that starts within 0.01 of zero: its lower knot is the float32 ``x0`` itself and ``v - knot``
  loses no digits, so that the float64 reference is good to 1e-12 there); rows 0 .. 2 inside that bin at 0.1, 0.5, 0.9 of its width, rows 3, 4 random.
* ``e_slopes_k8``: raw slopes of +25 (even knots of even features, past the softplus threshold) and -25 (odd knots of odd
  features); rows 0 .. 2 at 0.3, 0.5, 0.7 of bin ``(f + row) mod K``, row 3 in the lower and row 4 in the upper tail.

Random raw widths and heights are uniform in ``[-1.5 c, 1.5 c]`` with ``c = min(1, log(1 / (0.011 K)) / 3)``: every softmax
share is at least ``exp(-3 c) / K >= 0.011``, every bin at least 1e-2 of the domain.  Raw slopes: ``z = raw + slope_offset =
7.9 u^3``, u uniform in [-1, 1]: ``|z| <= 8``.  ``x`` (``yin``) is uniform over the domain and a quarter of its length on
either side.  Circular cases keep the shifted point at least 2e-3 of the period from the wrap point (wrapping has a test of
its own in test_gpu_parity.py).  A knot row closer than ``2^-30 (xf - x0)`` to its knot would let a shift of the knot by the
``exp_nonpos`` error put kernel and reference into different bins: the builder moves raw width 0 (raw height 0 for a y-knot) of such a feature by
2^-10 and looks again.

Cotangents ``gy`` (B, D), ``gl`` (B,); ``gl = 0`` for the one-element cases (B = D = 1: see ``_inputs``) and for row 3 of the edge rows: on ``x == x0`` / ``x == xf`` the parameter
gradient of the log-derivative jumps between the last bin and the tail, the reference there is one-sided.  The gradients are
those of the FORWARD map (``ops.spline_backward`` is its VJP).

Bounds (``DELTA_S``, ``DELTA_E``; all from the reference, none from a kernel)
---------------------------------------------------------------------------
The kernels form the K + 1 knot slopes in float32 and the softmax exponentials by ``exp_nonpos``; the rest is fp64.

* ``DELTA_S = 2^-20``, the relative error of a slope ``d = softplus(raw + offset) + min_slope`` in float32 with
  ``|z| <= 8``: the rounded add moves z by 2^-24 |z| <= 2^-21, which softplus passes on at most at that relative size; expf
  <= 3 ulp, log1pf <= 2 ulp (the OpenCL full-profile limits: this ROCm installation ships no table of ulp errors of its
  device math library), the final add half an ulp.  Past the threshold (z > 20) d = z + min_slope is two rounded adds; at
  z = -24 the slope is min_slope to 1e-7.
* ``DELTA_E = 2^-33``, 8 x the 1e-11 that ``exp_nonpos`` states for itself.
* values, per element: ``|out - ref| <= 2^-23 |ref| + DELTA_S S_s + DELTA_E S_e`` with ``S_s = sum_j |d out / d d_j| d_j``,
  ``S_e = sum_k |d out / d e_k| e_k`` (over ``ew`` and ``eh``) from autograd on the reference: the store rounds once (2^-24,
  taken twice), and a relative error of an intermediate reaches the output through its sensitivity.
* log-det, per sample: ``sum_i [2^-22 max(1, |ld_i|) + DELTA_S S_s,i + DELTA_E S_e,i] + 2^-24 |ldj|``: per element logf
  (<= 3 ulp of its result) of a float-cast argument (half an ulp of the argument: 2^-24 absolute on its log), the sum in
  fp64, one rounding on the store.  Accumulated onto a start value: ``|start + ldj|`` in the last term.
* gradients: relative L2 per tensor ``<= 2^-22 + 4 M``; ``M`` (``grad_movement``) is how far the reference's own gradient
  moves when every ``d_j`` is scaled by ``1 +- DELTA_S`` and every ``e_k`` by ``1 +- DELTA_E``, signs drawn, the largest of
  4 draws; the factor 4 because drawn signs do not reach the worst case.
* ``GRAD_DROPPED``: the cases whose M exceeds 2^-18 (two at the most; test_spline_cases_host.py holds the list to the
  measurement).
"""
import functools
import math

import numpy as np
import torch

import spline_ref

F32, F64 = torch.float32, torch.float64
DELTA_S, DELTA_E = 2.0 ** -20, 2.0 ** -33
MIN_BIN = MIN_SLOPE = float(np.float32(1e-4))
SLOPE_OFFSET = math.log(math.exp(1.0 - MIN_SLOPE) - 1.0)

TIERS = (1, 8, 9, 16, 17, 32)
WIDTHS = (1, 63, 64, 65, 130)
#: name -> (circular, identity boundary slopes, learnable lower bound, learnable upper bound)
LAYOUTS = {'plain': (False, False, False, False), 'circ': (True, False, False, False), 'ident': (False, True, False, False),
           'circident': (True, True, False, False), 'lower': (False, False, True, False), 'upper': (False, False, False, True),
           'both': (False, False, True, True), 'identboth': (False, True, True, True)}

RANDOM = tuple(f'r_k{K}_d{D}_b{B}' for K in TIERS for D in WIDTHS for B in (1, 5))
LAYOUT = tuple(f'l_{lay}_k{K}' for lay in LAYOUTS for K in (8, 17))
EDGE = tuple(f'e_rows_k{K}' for K in TIERS) + ('e_narrow_k8', 'e_slopes_k8')
#: (bins, circular, identity, learnable lower, learnable upper) of every layout that has a fused epilogue -- the list of
#: tests/test_gpu_torch_ops.py::_FUSED_LAYOUTS and the plain 8-bin layout -- as cases ``s_{flags}_k{K}`` (flags: four digits) with
#: ONE row of parameters for the 5 rows, like the edge cases: what a MAF layer with zero conditioner weights hands every sample
#: (the fused epilogue and the blocked inverse at known parameters; tests/test_spline_cases_host.py holds the list to that one)
FUSED_LAYOUTS = (
    (8, False, False, False, False),
    (4, False, False, False, False), (5, False, False, False, False), (5, True, False, False, False), (8, True, False, False, False),
    (8, False, True, False, False), (8, True, True, False, False), (8, False, True, True, False), (5, False, True, False, False),
    (5, True, True, False, False), (5, False, True, False, True), (5, False, False, True, False), (5, False, False, False, True),
    (5, False, False, True, True), (4, False, True, False, False), (4, False, True, True, False), (4, False, False, False, True),
    (4, False, False, True, True), (8, False, True, True, True), (5, False, True, True, True), (4, False, True, True, True),
    (8, False, False, True, False), (8, False, False, False, True), (8, False, False, True, True))
SHARED = tuple('s_' + ''.join(str(int(f)) for f in lay[1:]) + f'_k{lay[0]}' for lay in FUSED_LAYOUTS)
NAMES = RANDOM + LAYOUT + SHARED + EDGE

#: Cases left out of the gradient comparison: ``grad_movement`` above 2^-18 (none).
GRAD_DROPPED = ()
GRAD_DROP_ABOVE = 2.0 ** -18


def _parse(name):
    p = name.split('_')
    fields = {s[0]: int(s[1:]) for s in p[1:] if s[0] in 'kdb' and s[1:].isdigit()}
    return p[0], p[1], fields


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def flags(c):
    """The keyword arguments of ``spline_ref`` (and of the oracle) of a case."""
    circ, ident, lo, up = c['layout']
    return dict(y0=c['y0'], yf=c['yf'], circular=circ, identity_boundary_slopes=ident, learn_lower_bound=lo,
                learn_upper_bound=up, min_bin_size=MIN_BIN, min_slope=MIN_SLOPE)


def _domain(D, own_y, offset=0.0, length=1.0):
    f = torch.arange(D, dtype=F64)
    x0, xf = offset + length * (-3.0 - 0.01 * (f % 7)), offset + length * (2.5 + 0.02 * (f % 5))
    y0, yf = (-1.5 - 0.01 * (f % 3), 4.0 + 0.03 * (f % 4)) if own_y else (x0, xf)
    return tuple(t.to(F32) for t in (x0, xf, y0, yf))


def _raw(gen, B, K, D, layout, zmax=7.9):
    """(B, P, D) float64 raw parameters of the random recipe."""
    circ, ident, lo, up = layout
    P = spline_ref.n_parameters_per_feature(K, circ, ident, lo, up)
    c = min(1.0, math.log(1.0 / (0.011 * K)) / 3.0)
    p = torch.zeros(B, P, D, dtype=F64)
    p[:, :2 * K] = (torch.rand(B, 2 * K, D, dtype=F64, generator=gen) * 3.0 - 1.5) * c
    n_slopes = K - 1 if ident else (K if circ else K + 1)
    u = torch.rand(B, n_slopes, D, dtype=F64, generator=gen) * 2.0 - 1.0
    p[:, 2 * K:2 * K + n_slopes] = zmax * u ** 3 - SLOPE_OFFSET
    if circ:
        p[:, -1] = torch.rand(B, D, dtype=F64, generator=gen) * 8.0 - 4.0            # the shift: any number
    if lo or up:
        p[:, -1] = torch.rand(B, D, dtype=F64, generator=gen) * 0.6 - 0.3            # log of the domain's scale
    if lo and up:
        p[:, -2] = torch.rand(B, D, dtype=F64, generator=gen) - 0.5                  # the domain's shift
    return p


def _spread(gen, B, lo, hi):
    """Uniform over [lo, hi] and a quarter of its length on either side; (B, D) float64."""
    lo, hi = lo.to(F64), hi.to(F64)
    return lo + (hi - lo) * (torch.rand(B, lo.shape[0], dtype=F64, generator=gen) * 1.5 - 0.25)


def _neighbours(t):
    """The float32 numbers below, nearest to and above a float64 tensor, stacked: (3, ...) float32."""
    mid = t.to(F32)
    return torch.stack([torch.nextafter(mid, torch.full_like(mid, -math.inf)), mid,
                        torch.nextafter(mid, torch.full_like(mid, math.inf))])


def _knots_of(c, par):
    q = spline_ref.intermediates(par.to(F64), c['x0'], c['xf'], c['K'], **flags(c))
    return spline_ref.knots(q)[:2]


def knot_of_feature(K, D):
    """Interior knot of feature f that the edge rows sit on: ``1 + f mod (K - 1)``."""
    return 1 + torch.arange(D) % max(K - 1, 1)


def knot_margin(c):
    return 2.0 ** -30 * (c['xf'].to(F64) - c['x0'].to(F64))


def _edge_rows(c, par):
    """``x`` and ``yin`` of the edge rows, (5, D) float32, for one (P D,) row of float32 parameters."""
    K, D = c['K'], c['D']
    kx, ky = (k[0] for k in _knots_of(c, par[None]))                                # (K + 1, D)
    even = torch.arange(D) % 2 == 0
    far = torch.where(even, torch.full((D,), -1e3, dtype=F32), torch.full((D,), 1e3, dtype=F32))
    # (the inverse's far row: the image of the forward's, so that it stays inside the reference's sentinel knots, which lie
    # 1000 domain widths out in x and only the boundary slope times that in y)
    far_y = spline_ref.spline_forward(far[None].to(F64), par[None].to(F64), c['x0'], c['xf'], K, **flags(c))[0][0].to(F32)
    out = []
    for kn, far_row in ((kx, far), (ky, far_y)):
        lo, hi = kn[0], kn[K]
        target = 0.5 * (lo + hi) if K == 1 else torch.gather(kn, 0, knot_of_feature(K, D)[None])[0]
        ends = torch.where(even, lo, hi).to(F32)
        out.append(torch.cat([_neighbours(target), ends[None], far_row[None]]))
    return out


def _inputs(name):
    kind, what, f = _parse(name)
    K = f['k']
    gen = torch.Generator().manual_seed(_seed(name))
    layout = LAYOUTS[what] if kind == 'l' else (tuple(ch == '1' for ch in what) if kind == 's' else LAYOUTS['plain'])
    B, D = (f['b'], f['d']) if kind == 'r' else (5, 65)
    x0, xf, y0, yf = _domain(D, own_y=kind == 'r', offset=0.0 if kind != 'e' else (0.602 if what == 'narrow' else 4.5),
                             length=0.2 if what == 'narrow' else 1.0)
    c = dict(name=name, K=K, B=B, D=D, layout=layout, x0=x0, xf=xf, y0=y0, yf=yf,
             P=spline_ref.n_parameters_per_feature(K, *layout))
    if kind == 'e':
        p = _raw(gen, 1, K, D, layout, zmax=2.0 if what == 'rows' else 7.9)
        if what == 'narrow':
            p[:, 0] = p[:, K] = -12.0
        if what == 'slopes':
            fe = (torch.arange(D) % 2 == 0)[None, None, :]
            je = (torch.arange(K + 1) % 2 == 0)[None, :, None]
            s = p[:, 2 * K:3 * K + 1]
            p[:, 2 * K:3 * K + 1] = torch.where(fe & je, torch.full_like(s, 25.0), torch.where(~fe & ~je, torch.full_like(s, -25.0), s))
        par = p.reshape(1, -1).to(F32)
        if what == 'rows':
            for _ in range(16):
                x, yin = _edge_rows(c, par[0])
                kx, ky = _knots_of(c, par)
                near = lambda v, kn: ((v[:3, None, :].to(F64) - kn).abs() < knot_margin(c)).any(dim=1).any(dim=0)   # noqa: E731
                bad_x, bad_y = near(x, kx), near(yin, ky)
                if K == 1 or not bool((bad_x | bad_y).any()):
                    break
                par.reshape(c['P'], D)[0, bad_x] += 2.0 ** -10
                par.reshape(c['P'], D)[K, bad_y] += 2.0 ** -10
            else:
                raise RuntimeError(f'{name}: no parameters with every knot row clear of its knot')
        else:
            x, yin = _spread(gen, B, x0, xf), _spread(gen, B, y0, yf)
            kx, ky = (k[0] for k in _knots_of(c, par))
            for v, kn in ((x, kx), (yin, ky)):
                for r, t in enumerate((0.1, 0.5, 0.9) if what == 'narrow' else (0.3, 0.5, 0.7)):
                    # narrow: inside bin 0; slopes: inside bin (f + r) mod K, away from its knots -- next to a knot of slope
                    # 1e-4 the inverse's root formula loses 7 digits to cancellation, in the reference as in any fp64 evaluation
                    j = torch.zeros(D, dtype=torch.long) if what == 'narrow' else (torch.arange(D) + r) % K
                    lo, hi = torch.gather(kn, 0, j[None])[0], torch.gather(kn, 0, j[None] + 1)[0]
                    v[r] = lo + t * (hi - lo)
                if what == 'slopes':
                    length = kn[K] - kn[0]
                    v[3], v[4] = kn[0] - 0.1 * length * (1 + torch.arange(D) % 3), kn[K] + 0.1 * length * (1 + torch.arange(D) % 3)
            x, yin = x.to(F32), yin.to(F32)
        par = par.expand(B, -1).contiguous()
    else:
        par = _raw(gen, 1 if kind == 's' else B, K, D, layout).reshape(-1, c['P'] * D).to(F32).expand(B, -1).contiguous()
        x, yin = _spread(gen, B, x0, xf), _spread(gen, B, y0, yf)
        # the reference (and the oracle) end at two sentinel knots, 1000 domain widths out in x and the boundary slope times
        # that in y: the inverse's input stays inside half of that reach (a boundary slope of 4e-4 reaches 2.2 past the domain)
        q = spline_ref.intermediates(par.to(F64), x0, xf, K, **flags(c))
        kx, ky = spline_ref.knots(q)[:2]
        reach = 500.0 * (kx[:, K] - kx[:, 0])
        yin = torch.minimum(torch.maximum(yin, ky[:, 0] - q['d'][:, 0] * reach), ky[:, K] + q['d'][:, K] * reach)
        if layout[0]:
            # circular: the shifted point u = (x - x0 + shift) mod period in [2e-3, 1 - 2e-3] of the period; the inverse's
            # input inside the domain, moved on where its image would come to lie at the wrap point
            period, shift = (xf - x0).to(F64), par.reshape(B, c['P'], D)[:, -1].to(F64)
            u = (2e-3 + (1 - 4e-3) * torch.rand(B, D, dtype=F64, generator=gen)) * period
            x = (x0.to(F64) + torch.remainder(u - shift, period)).to(F32)
            yin = x0.to(F64) + (0.01 + 0.98 * torch.rand(B, D, dtype=F64, generator=gen)) * period
            for _ in range(16):
                q = spline_ref.intermediates(par.to(F64), x0, xf, K, **flags(c))
                pre = spline_ref.evaluate(yin.to(F32).to(F64), q, inverse=True)[0]
                r = torch.remainder(pre - x0.to(F64) - shift, period) / period
                bad = (r < 2e-3) | (r > 1 - 2e-3)
                if not bool(bad.any()):
                    break
                yin = torch.where(bad, x0.to(F64) + torch.remainder(yin - x0.to(F64) + 0.05 * period, 0.98 * period) + 0.01 * period, yin)
            else:
                raise RuntimeError(f'{name}: the inverse input stays on the wrap point')
        x, yin = x.to(F32), yin.to(F32)
    gy, gl = torch.randn(B, D, dtype=F64, generator=gen).to(F32), torch.randn(B, dtype=F64, generator=gen).to(F32)
    if kind == 'e' and what == 'rows':
        gl[3] = 0.0
    if B * D == 1:
        # one element: a single number per gradient, in which the contributions of the two cotangents can cancel and leave
        # its RELATIVE movement under the error model as large as one likes -- the cotangent of y alone
        gl[0] = 0.0
    c.update(par=par, x=x, yin=yin, gy=gy, gl=gl)
    return c


def _sensitivity(out, q):
    """``(S_s, S_e)`` of every element of ``out`` (B, D): element (b, f) depends on the leaves of (b, :, f) alone, so one
    backward pass of the sum holds every element's own derivatives."""
    g = torch.autograd.grad(out.sum(), [q['d'], q['ew'], q['eh']], retain_graph=True, allow_unused=True)
    gd, gw, gh = (torch.zeros_like(t) if g_ is None else g_ for g_, t in zip(g, (q['d'], q['ew'], q['eh'])))
    return ((gd.abs() * q['d']).sum(dim=1).detach(),
            ((gw.abs() * q['ew']).sum(dim=1) + (gh.abs() * q['eh']).sum(dim=1)).detach())


def _direction(c, key):
    """The reference of one direction with its bounds: dict ``out`` (B, D), ``ld`` (B, D: the log-derivative per element),
    ``ldj`` (B,), ``bins``, ``out_bound`` (B, D) and ``ld_bound`` (B,: the sum over the elements, WITHOUT the rounding of the
    stored total, which depends on what it is accumulated onto -- ``ldj_bound``)."""
    v = c['x' if key == 'fwd' else 'yin'].to(F64)
    fn = spline_ref.forward_elements if key == 'fwd' else spline_ref.inverse_elements
    out, ld, bins, q = fn(v, c['par'].to(F64), c['x0'], c['xf'], c['K'], leaves=True, **flags(c))
    s_s, s_e = _sensitivity(out, q)
    out_bound = 2.0 ** -23 * out.detach().abs() + DELTA_S * s_s + DELTA_E * s_e
    s_s, s_e = _sensitivity(ld, q)
    ld_bound = (2.0 ** -22 * ld.detach().abs().clamp(min=1.0) + DELTA_S * s_s + DELTA_E * s_e).sum(dim=1)
    return dict(out=out.detach(), ld=ld.detach(), ldj=ld.detach().sum(dim=1), bins=bins, out_bound=out_bound, ld_bound=ld_bound)


def ldj_bound(ref, start=None):
    """Bound of the stored log-det per sample; ``start``: the (B,) float64 values it was accumulated onto."""
    total = ref['ldj'] if start is None else start + ref['ldj']
    return ref['ld_bound'] + 2.0 ** -24 * total.abs()


def gradients(c, scale=None):
    """``(grad_x, grad_parameters)`` of ``(y gy).sum() + (log_det_J gl).sum()`` through the forward map, float64."""
    x, par = c['x'].to(F64).requires_grad_(True), c['par'].to(F64).requires_grad_(True)
    y, ldj = spline_ref.spline_forward(x, par, c['x0'], c['xf'], c['K'], scale=scale, **flags(c))
    ((y * c['gy'].to(F64)).sum() + (ldj * c['gl'].to(F64)).sum()).backward()
    return x.grad, par.grad


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: float32 CPU tensors ``x0, xf, y0, yf`` (D,), ``par`` (B, P D), ``x``, ``yin``, ``gy`` (B, D), ``gl`` (B,); ``K, B, D, P,
    layout``; the float64 reference ``fwd`` / ``inv`` (``_direction``) and ``grad`` = (grad_x, grad_parameters) of the forward
    map.  Computed once per name: treat it as read-only."""
    c = _inputs(name)
    c['fwd'], c['inv'] = _direction(c, 'fwd'), _direction(c, 'inv')
    c['grad'] = gradients(c)
    return c


def rel_l2(got, ref):
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    return float((got - ref).norm() / ref.norm().clamp(min=1e-300))


@functools.lru_cache(maxsize=None)
def grad_movement(name):
    """``(M_x, M_parameters)``: the relative L2 by which the reference's gradients move when every slope is scaled by
    ``1 +- DELTA_S`` and every softmax exponential by ``1 +- DELTA_E`` (signs drawn), the largest of 4 draws."""
    c = case(name)
    gen = torch.Generator().manual_seed(_seed(name) + 1)
    B, K, D = c['B'], c['K'], c['D']
    sign = lambda *shape: 2.0 * torch.randint(0, 2, shape, generator=gen).to(F64) - 1.0   # noqa: E731
    moved = [0.0, 0.0]
    for _ in range(4):
        scale = (1.0 + DELTA_S * sign(B, K + 1, D), 1.0 + DELTA_E * sign(B, K, D), 1.0 + DELTA_E * sign(B, K, D))
        g = gradients(c, scale)
        moved = [max(m, rel_l2(a, b)) for m, a, b in zip(moved, g, c['grad'])]
    return tuple(moved)


def grad_bounds(name):
    """Relative L2 bounds of (grad_x, grad_parameters)."""
    return tuple(2.0 ** -22 + 4.0 * m for m in grad_movement(name))


def value_errors(c, key, out, ldj, start=None):
    """``(largest |out - ref| in units of its bound, largest |ldj - ref| in units of its bound)``."""
    ref = c[key]
    out, ldj = out.detach().cpu().to(F64), ldj.detach().cpu().to(F64)
    want = ref['ldj'] if start is None else start + ref['ldj']
    return (float(((out - ref['out']).abs() / ref['out_bound']).max()),
            float(((ldj - want).abs() / ldj_bound(ref, start)).max()))
