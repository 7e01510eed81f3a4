"""GPU tests of the fused spline epilogue of the split-f16 output GEMM (csrc/split_gemm_kernel.h) with the accumulators of
the later row blocks parked in LDS: the arithmetic is meant to be untouched, so the outputs are compared with the generic
route on the same split GEMMs, with the float64 oracle on inputs outside the domain and on knots, and -- exactly -- with
the outputs the kernel gave before the change (tests/golden/spline_epilogue_parent.npz).

Shapes: one 256-row tile plus a ragged one (B = 300: the last 16-row block of the second tile is partly filled), three
16-feature column tiles (D = 48; D = 40 leaves dead feature slots in the last one)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'spline_epilogue_parent.npz')


def make_layer(D, hidden=96, lo=-5.0, hi=5.0, seed=7, **spline_kw):
    """One MAF layer with an 8-bin RQ spline.  The parameters come from numpy's legacy generator (a fixed stream), so the
    layer is the same wherever it is built -- the stored outputs of the parent commit depend on it."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    maf = MAF(generate_degrees(D, 'ascending'),
              transformer=NeuralSplineTransformer(torch.full((D,), lo), torch.full((D,), hi), 8, **spline_kw),
              hidden_layers=[hidden, hidden], initialize_identity=False)
    rng = np.random.RandomState(seed)
    with torch.no_grad():
        for name, p in maf.named_parameters():
            v = rng.standard_normal(tuple(p.shape)).astype(np.float32)
            if name.endswith('weight_g'):
                v = 0.5 + 0.5 * np.abs(v)
            elif name.endswith('bias'):
                v = 0.2 * v
            p.copy_(torch.from_numpy(v))
    return maf.cuda()


def make_x(B, D, seed=11, scale=1.5):
    return torch.from_numpy((scale * np.random.RandomState(seed).standard_normal((B, D))).astype(np.float32))


def run(maf, x, fused):
    """Forward on the split-f16 GEMMs: the fused output-layer kernel, or three GEMMs and the stand-alone spline kernel."""
    maf.split_gemm, maf.fused = True, fused
    with torch.no_grad():
        y, l = maf(x)
    torch.cuda.synchronize()
    return y, l


def check_fused_against_generic(maf, x):
    yf, lf = run(maf, x, True)
    yg, lg = run(maf, x, False)
    yf2, lf2 = run(maf, x, True)
    rel = float((yf - yg).norm() / yg.norm())
    print(f'fused vs generic: rel L2(y) {rel:.2e}, max |d ldj| {float((lf - lg).abs().max()):.2e}')
    assert bool(torch.isfinite(yf).all()) and bool(torch.isfinite(lf).all())
    # the tolerance of test_forward_paths_agree_on_golden_flows (tests/test_gpu_split_gemm.py)
    assert rel < 1e-6
    assert torch.allclose(lf, lg, rtol=1e-5, atol=2e-5)
    assert torch.equal(yf, yf2) and torch.equal(lf, lf2)
    return yf, lf


@pytest.mark.parametrize('D', [48, 40])
def test_fused_epilogue_matches_the_generic_route(D):
    check_fused_against_generic(make_layer(D), make_x(300, D).cuda())


@pytest.mark.parametrize('flags', [
    dict(circular=True),                                                                    # 25 parameters
    dict(identity_boundary_slopes=True),                                                    # 23
    dict(identity_boundary_slopes=True, circular=True),                                     # 24
    dict(identity_boundary_slopes=True, learn_lower_bound=True),                            # 24
    dict(identity_boundary_slopes=True, learn_lower_bound=True, learn_upper_bound=True),    # 25, an epilogue of its own
    dict(learn_upper_bound=True),                                                           # 26: nothing parked
    dict(learn_lower_bound=True, learn_upper_bound=True),                                   # 27: nothing parked
], ids=lambda f: '+'.join(sorted(f)))
def test_fused_epilogue_flag_combinations(flags):
    lo, hi = (0.0, 2.0) if flags.get('circular') else (-4.0, 4.0)
    D, B = 32, 80
    x = make_x(B, D, scale=1.0)
    if flags.get('circular'):
        x = x.remainder(2.0) * 0.98 + 0.01
    check_fused_against_generic(make_layer(D, lo=lo, hi=hi, **flags), x.cuda())


def test_fused_epilogue_outside_the_domain_and_on_knots_vs_float64_oracle():
    """1.5 randn on [-2, 2] (every tenth element or so lies outside), rows set to x0, to xf, and -- the last feature, which
    no other depends on -- to an interior knot of its own spline.  Tolerances of tests/test_gpu_parity.py, end to end
    through the fp32 GEMMs: rel L2(y) <= 1e-5, log-det error per sample within 1e-5 max(1, |ldj|) or 4 x the float32
    oracle's own error against float64 (floor 2e-5)."""
    from oracle import flows as oflows, made as omade, transformers as otr
    D, B, K, lo, hi = 32, 64, 8, -2.0, 2.0
    maf = make_layer(D, lo=lo, hi=hi)
    x = make_x(B, D).numpy()
    x[0, :], x[1, :] = lo, hi
    x[2, ::2], x[2, 1::2] = lo, hi
    sd = {k: v.cpu().numpy() for k, v in maf.state_dict().items()}

    def olayer(dtype):
        sdd = {k: (v.astype(dtype) if v.dtype == np.float32 else v) for k, v in sd.items()}
        return dict(degrees_in=omade.generate_degrees(D, 'ascending'),
                    transformer=dict(type='spline', x0=np.full(D, lo, dtype), xf=np.full(D, hi, dtype), n_bins=K),
                    embedding=None, made=omade.made_layers_from_state(sdd, prefix='_conditioner.'))
    # rows 3 .. 9: the last feature on interior knot 1 .. 7 of its spline (float64 knot, rounded to float32)
    prm = omade.made_forward(x.astype(np.float64), olayer(np.float64)['made'])
    x0s, _, widths, _, _, _ = otr.spline_get_parameters(prm, np.full(D, lo), np.full(D, hi), K)
    knots = np.asarray(x0s)[..., -1] + np.cumsum(widths[:, :, -1], axis=1)           # (B, K)
    for k in range(1, K):
        x[2 + k, -1] = np.float32(knots[2 + k, k - 1])
    assert (np.abs(x) > hi).mean() > 0.05

    y64, l64 = oflows.sequential_forward(x.astype(np.float64), [olayer(np.float64)])
    y32, l32 = oflows.sequential_forward(x.astype(np.float32), [olayer(np.float32)])
    y, l = run(maf, torch.from_numpy(x).cuda(), True)
    y, l = y.cpu().numpy().astype(np.float64), l.cpu().numpy().astype(np.float64)
    rel = np.linalg.norm(y - y64) / np.linalg.norm(y64)
    noise_l = np.abs(l32.astype(np.float64) - l64).max()
    err_l = np.abs(l - l64)
    tol_l = np.maximum(1e-5 * np.maximum(1.0, np.abs(l64)), max(4.0 * noise_l, 2e-5))
    print(f'vs float64 oracle: rel L2(y) {rel:.2e}, max |d ldj| {err_l.max():.2e} (float32 oracle {noise_l:.2e})')
    assert rel <= 1e-5
    assert bool((err_l <= tol_l).all()), (err_l.max(), tol_l.min())


def parent_case():
    """The case whose outputs were stored on the parent commit: D = 48, B = 300, the fused kernel."""
    return make_layer(48), make_x(300, 48).cuda()


def test_fused_epilogue_gives_the_bits_of_the_parent_commit():
    """y and log|det J| of the fused kernel before its accumulators were parked (stored by running parent_case() on that
    commit): where they are kept until the records are made changes no arithmetic, so not one bit may differ."""
    g = np.load(GOLDEN)
    maf, x = parent_case()
    y, l = run(maf, x, True)
    y, l = y.cpu().numpy(), l.cpu().numpy()
    assert y.dtype == np.float32 and g['y'].dtype == np.float32
    assert np.array_equal(y, g['y']), f'{int((y != g["y"]).sum())} elements of y differ, max {np.abs(y - g["y"]).max():.2e}'
    assert np.array_equal(l, g['log_det_J']), f'{int((l != g["log_det_J"]).sum())} log-dets differ'
