"""GPU tests of the float32 rational-quadratic spline kernels, per element, against the float64 restatement
tests/spline_ref.py evaluated at the same float32 numbers (tests/spline_cases.py: the cases and the derivation of every
bound; tests/test_spline_cases_host.py holds cases and restatement to their own conditions):

1. the stand-alone kernels ``spline_kernel<KMAX, INVERSE>`` (``ops.spline``, ``NeuralSplineTransformer``), also accumulating;
2. ``spline_backward_kernel<KMAX>`` (``ops.spline_backward``) in the default and the feature-major parameter layout (LDS-staged
   for K <= 16, unstaged above), the latter also inside a padded wider buffer, strided ``x`` views, a row alone;
3. the fused epilogue (``rq_spline_forward_full``: the ``exact`` and ``split`` paths of a MAF layer) and the blocked inverse
   (``rq_spline_inverse_selects``) at KNOWN parameters: a layer with zero conditioner weights hands every sample its output
   bias;
4. the stand-alone kernels, the default-layout VJP and the super-block kernel of the blocked inverse against the BITS the
   commit before the shared steps of ``csrc/spline.h`` gave (``tests/golden/spline_core_parent.json``, written from that commit
   by tools/dump_spline_digests.py, whose functions the test runs).

Every bound is that of ``spline_cases`` (values per element and log-det per sample: ``value_errors`` returns the error in
units of its bound; gradients: ``grad_bounds``); every test prints the error it saw in those units (bound: 1).
"""
import importlib.util
import os
import sys

import pytest
import torch

import spline_cases as sc

pytestmark = pytest.mark.gpu
F32 = torch.float32


def config(c):
    from tfep_amd import ops
    circ, ident, lo, up = c['layout']
    return ops.SplineConfig(c['x0'].cuda(), c['xf'].cuda(), c['y0'].cuda(), c['yf'].cuda(), c['K'], circ, ident, lo, up,
                            sc.MIN_BIN, sc.MIN_SLOPE)


def transformer(c):
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    circ, ident, lo, up = c['layout']
    return NeuralSplineTransformer(c['x0'].clone(), c['xf'].clone(), c['K'], y0=c['y0'].clone(), yf=c['yf'].clone(), circular=circ,
                                   identity_boundary_slopes=ident, learn_lower_bound=lo, learn_upper_bound=up,
                                   min_bin_size=sc.MIN_BIN, min_slope=sc.MIN_SLOPE).cuda()


def check_values(what, c, key, out, ldj, start=None):
    assert out.dtype == F32 and ldj.dtype == F32 and out.shape == c[key]['out'].shape and ldj.shape == (c['B'],)
    e_out, e_ldj = sc.value_errors(c, key, out, ldj, start)
    print(f'{what} {key}: per element {e_out:.3f}, log-det {e_ldj:.3f} (units of the bound)')
    assert e_out <= 1.0 and e_ldj <= 1.0, (what, key, e_out, e_ldj)
    return e_out, e_ldj


# ------------------------------------------------------------------ 1. the stand-alone kernels

@pytest.mark.parametrize('name', sc.NAMES)
def test_forward_and_inverse_against_float64(name):
    from tfep_amd import ops
    c = sc.case(name)
    cfg, tr, par = config(c), transformer(c), c['par'].cuda()
    assert cfg.n_parameters_per_feature == tr.n_parameters_per_feature == c['P']
    for key, v, fn, inverse in (('fwd', c['x'], tr.forward, False), ('inv', c['yin'], tr.inverse, True)):
        out, ldj = ops.spline(v.cuda(), par, cfg, inverse=inverse)
        check_values(name, c, key, out, ldj)
        with torch.no_grad():
            out_m, ldj_m = fn(v.cuda(), par)
        assert torch.equal(out_m, out) and torch.equal(ldj_m, ldj)


@pytest.mark.parametrize('name', sc.NAMES)
def test_accumulation_onto_a_log_det(name):
    from tfep_amd import ops
    c = sc.case(name)
    cfg, par = config(c), c['par'].cuda()
    start = torch.linspace(-2.0, 3.0, c['B'], dtype=F32)
    for key, v, inverse in (('fwd', c['x'], False), ('inv', c['yin'], True)):
        acc = start.cuda()
        out, ldj = ops.spline(v.cuda(), par, cfg, inverse=inverse, log_det_J=acc)
        assert ldj is acc
        assert torch.equal(out, ops.spline(v.cuda(), par, cfg, inverse=inverse)[0])
        check_values(name + ' accumulated', c, key, out, acc, start=start.double())


# ------------------------------------------------------------------ 2. the VJP

def feature_major(par, P, D, pad=0):
    """(B, P D) in the reference layout (column p D + f) as the (B, D P + pad) buffer of the feature-major layout
    (column f P + p; ``layout = (D P + pad, 1, P)``), the padding filled with a sentinel."""
    B = par.shape[0]
    buf = torch.full((B, D * P + pad), 7.0, dtype=par.dtype, device=par.device)
    buf[:, :D * P] = par.reshape(B, P, D).transpose(1, 2).reshape(B, D * P)
    return buf


def from_feature_major(buf, P, D):
    B = buf.shape[0]
    return buf[:, :D * P].reshape(B, D, P).transpose(1, 2).reshape(B, P * D)


@pytest.mark.parametrize('name', [n for n in sc.NAMES if n not in sc.GRAD_DROPPED])
def test_backward_against_autograd_through_the_restatement(name):
    from tfep_amd import ops
    c = sc.case(name)
    cfg = config(c)
    B, D, P = c['B'], c['D'], c['P']
    x, par, gy, gl = (c[k].cuda() for k in ('x', 'par', 'gy', 'gl'))
    bx, bp = sc.grad_bounds(name)
    gx, gp = ops.spline_backward(x, par, cfg, gy, gl)
    assert gx.dtype == F32 and gp.dtype == F32 and gx.shape == (B, D) and gp.shape == (B, P * D)
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gp).all())
    ex, ep = sc.rel_l2(gx, c['grad'][0]), sc.rel_l2(gp, c['grad'][1])
    print(f'{name}: grad x {ex / bx:.3f}, grad parameters {ep / bp:.3f} (units of the bound: {bx / 2.0 ** -22:.2f}, {bp / 2.0 ** -22:.2f} x 2^-22)')
    assert ex <= bx and ep <= bp, (name, ex, bx, ep, bp)
    # the feature-major layout (K <= 16: through the LDS stage; above: element loads), tight and inside a padded wider buffer
    for pad in (0, 7):
        fm = feature_major(par, P, D, pad)
        gxf, gpf = ops.spline_backward(x, fm, cfg, gy, gl, layout=(D * P + pad, 1, P))
        assert gpf.shape == fm.shape
        assert torch.equal(gxf, gx) and torch.equal(from_feature_major(gpf, P, D), gp), (name, pad)
        assert bool((gpf[:, D * P:] == 0).all())                                  # (fresh zeros: nothing written past the block)
    # x and the cotangent as column slices of wider tensors
    wide_x, wide_g = torch.full((B, D + 5), 9.0, dtype=F32, device='cuda'), torch.full((B, D + 3), -9.0, dtype=F32, device='cuda')
    wide_x[:, 2:D + 2], wide_g[:, 1:D + 1] = x, gy
    for lay, p_ in ((None, par), ((D * P, 1, P), feature_major(par, P, D))):
        gxs, gps = ops.spline_backward(wide_x[:, 2:D + 2], p_, cfg, wide_g[:, 1:D + 1], gl, layout=lay)
        assert torch.equal(gxs, gx) and torch.equal(gps if lay is None else from_feature_major(gps, P, D), gp), (name, lay)


@pytest.mark.parametrize('K', sc.TIERS)
def test_backward_of_a_row_alone_equals_the_row_in_a_batch(K):
    from tfep_amd import ops
    c = sc.case(f'r_k{K}_d130_b5')
    cfg = config(c)
    D, P = c['D'], c['P']
    x, par, gy, gl = (c[k].cuda() for k in ('x', 'par', 'gy', 'gl'))
    for lay, p_ in ((None, par), ((D * P, 1, P), feature_major(par, P, D))):
        gx, gp = ops.spline_backward(x, p_, cfg, gy, gl, layout=lay)
        for r in (0, 3, 4):
            gx1, gp1 = ops.spline_backward(*[t[r:r + 1].clone() for t in (x, p_)], cfg, gy[r:r + 1].clone(), gl[r:r + 1].clone(), layout=lay)
            assert torch.equal(gx1[0], gx[r]) and torch.equal(gp1[0], gp[r]), (K, lay, r)


# ------------------------------------------------------------------ 3. fused epilogue and blocked inverse at known parameters

#: (the cases whose 5 rows share one row of parameters: every layout of tests/test_gpu_torch_ops.py::_FUSED_LAYOUTS -- K = 4,
#: 5 and 8 -- and the plain 8-bin one, then the edge rows at K = 8)
KNOWN = sc.SHARED + ('e_rows_k8', 'e_narrow_k8', 'e_slopes_k8')


def _set_path(maf, path):                                       # (as tests/test_gpu_sos.py::_set_path)
    maf.fused = path != 'generic'
    maf.split_gemm = path == 'split'


def zero_weight_layer(c):
    """A MAF layer whose conditioner has zero weights everywhere and the case's one row of parameters as its output bias:
    every GEMM adds exact zeros to it."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    assert bool((c['par'] == c['par'][:1]).all())
    maf = MAF(generate_degrees(c['D'], 'ascending'), transformer=transformer(c).cpu(), hidden_layers=[72, 80], weight_norm=False,
              initialize_identity=False)
    for n, p in maf._conditioner.named_parameters():
        if n.endswith('weight'):
            p.data.zero_()
    maf._conditioner.set_output(c['par'][0].clone())
    return maf.cuda()


@pytest.mark.parametrize('name', KNOWN)
def test_fused_epilogue_at_known_parameters(name):
    """``generic``, ``exact`` and ``split`` forward of a zero-weight layer: first that the conditioner of each path's
    arithmetic returns the bias bit for bit (the fused kernels keep the parameters in registers: for them the conditioner
    is run with the path's GEMM arithmetic, and the equality below is the check of what their own output GEMM hands the
    epilogue), then ``y`` and the log-det against the bounds, and the fused paths against the stand-alone kernel with
    ``torch.equal`` -- the "bit-identical results" of ``rq_spline_forward_full``."""
    from tfep_amd import ops
    c = sc.case(name)
    maf = zero_weight_layer(c)
    x, par = c['x'].cuda(), c['par'].cuda()
    y0, l0 = ops.spline(x, par, config(c))
    with torch.no_grad():
        for path in ('generic', 'exact', 'split'):
            _set_path(maf, path)
            assert torch.equal(maf.get_transformer_parameters(x), par), (name, path)
            assert (maf._fused_kind() is not None) == (path != 'generic')
            y, l = maf(x)
            check_values(f'{name} {path}', c, 'fwd', y, l)
            assert torch.equal(y, y0), (name, path, float((y - y0).abs().max()))
            assert torch.equal(l, l0), (name, path, float((l - l0).abs().max()))


#: (rows per wave, waves per workgroup, loader wave, split-f16 GEMMs) of the block kernel's row layouts; the last: the
#: (16, paired) layout with the split packs of every layer, which is what lets a layer take the one-launch-per-super-block
#: kernel (``last_inverse_schedule`` says whether it did)
ROW_LAYOUTS = ((64, None, None, None), (16, None, False, None), (16, 4, False, None), (16, None, True, None), (16, None, True, True))


@pytest.mark.parametrize('name', KNOWN)
def test_blocked_inverse_at_known_parameters(name):
    """The block kernel of the blocked inverse in its row layouts against the bounds, and against the pass-per-degree
    inverse (the stand-alone ``rq_spline_element<8, true>`` on the same float32 parameters: first asserted, the conditioner
    of every arithmetic returns the bias bit for bit; the block kernels form the parameters by dots of their own, which
    nothing outside them can read -- the equalities below are their check).

    ``x`` is asserted bit-equal wherever the code claims it: the one-block kernels call ``rq_spline_element<8, true>``
    itself, and ``rq_spline_inverse_selects`` without FAST (the super-block kernel on any layout but the two it specialises)
    states "the same bits".  Only the specialised super-block kernel -- 8 bins, plain or circular: fast fp64 division and
    square root, the quad exchange -- is held to the bounds alone.  The log-det is held to the bounds alone everywhere: the
    block kernel sums a row's terms in fp64 over the whole chain, the pass per degree rounds the sum to float32."""
    c = sc.case(name)
    maf = zero_weight_layer(c)
    yin, par = c['yin'].cuda(), c['par'].cuda()
    specialised = c['K'] == 8 and c['layout'] in (sc.LAYOUTS['plain'], sc.LAYOUTS['circ'])
    with torch.no_grad():
        maf.blocked_inverse = False
        xd, ld = maf.inverse(yin)
        assert maf.last_inverse_route == 'per_degree'
        check_values(f'{name} per degree', c, 'inv', xd, ld)
        x0, l0 = transformer(c).inverse(yin, par)
        assert torch.equal(xd, x0)
        maf.blocked_inverse = True
        assert maf._blocked_plan(yin.device)['fused'] is not None
        for rows, waves, paired, split in ROW_LAYOUTS:
            maf.inverse_rows_per_wave, maf.inverse_waves_per_workgroup, maf.inverse_paired, maf.split_gemm = rows, waves, paired, split
            assert torch.equal(maf.get_transformer_parameters(yin), par), (name, rows, waves, paired, split)
            xb, lb = maf.inverse(yin)
            assert maf.last_inverse_route == 'blocked'
            schedule = maf.last_inverse_schedule
            # the super-block kernel: the paired layout on split packs, where |x| has a bound beforehand (no learnable bound)
            assert (schedule == 'super_kernel') == (bool(split) and not (c['layout'][2] or c['layout'][3])), (name, schedule)
            check_values(f'{name} rows {rows} waves {waves} paired {paired} split {split} ({schedule})', c, 'inv', xb, lb)
            print(f'    the same bits as the pass per degree: x {torch.equal(xb, xd)}, log-det {torch.equal(lb, ld)}')
            if not (schedule == 'super_kernel' and specialised):
                assert torch.equal(xb, xd), (name, rows, waves, paired, split, schedule, float((xb - xd).abs().max()))


# ------------------------------------------------------------------ 4. the bits of the parent commit

def test_the_bits_of_the_parent_commit():
    """SHA-256 of the raw bytes of every output of ``ops.spline`` (both directions), of ``ops.spline_backward`` in the default
    layout and -- on the cases of ``test_blocked_inverse_at_known_parameters`` that take it -- of the super-block kernel, case
    by case, against the digests recorded from the commit before the evaluators were rebuilt from shared steps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('dump_spline_digests', os.path.join(root, 'tools', 'dump_spline_digests.py'))
    dump = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dump)
    want = dump.load()
    assert sorted(want) == sorted(sc.NAMES) and sum('super_x' in d for d in want.values()) == 13
    differ = {}
    for name in sc.NAMES:
        got = dump.case_digests(name, sc, sys.modules[__name__])
        assert sorted(got) == sorted(want[name]), name
        bad = [k for k in sorted(got) if got[k] != want[name][k]]
        if bad:
            differ[name] = bad
    assert differ == {}, f'other bits than the parent commit: {differ}'
