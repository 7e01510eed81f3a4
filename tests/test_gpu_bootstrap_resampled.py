"""GPU tests of the bootstrap with in-kernel resampling and of the float64 bootstrap kernel (csrc/reduce.hip,
csrc/bootstrap_rng.h, tfep_amd.analysis.bootstrap): the stream against its numpy restatement (tests/bootstrap_rng_ref.py), the
table route against the explicit kernel on the same resamples and against torch.logsumexp in float64, the replay of resamples
whose table sum underflows or whose data are not finite, float64 data, and ``bootstrap(..., resampler='kernel')``."""
import functools

import numpy as np
import pytest
import torch

import bootstrap_rng_ref as rr
import golden_util as gu

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
TOL = dict(rtol=1e-9, atol=1e-9)              # the bound of tests/test_gpu_bootstrap.py for this kernel


def _np(t):
    return t.cpu().numpy()


def _formula(work, idx, kT, bias=None):
    """fep_estimator of the resamples ``idx`` with torch.logsumexp in float64."""
    w = work.double()
    if bias is None:
        return -kT * (torch.logsumexp(-w[idx] / kT, dim=1) - np.log(idx.shape[1]))
    b = bias.double()
    return -kT * (torch.logsumexp((-w[idx] + b[idx]) / kT, dim=1) - torch.logsumexp(b[idx] / kT, dim=1))


def _formula_weights(work, wts, kT):
    return -kT * torch.logsumexp(-work.double()[None, :] / kT + torch.log(wts), dim=1)


# ------------------------------------------------------------------ 1. the stream

@pytest.mark.parametrize('high', [1, 7, 600, 2 ** 31 - 1])
@pytest.mark.parametrize('sample_size', [1, 3, 4, 5, 1027])
def test_indices_equal_the_restatement(sample_size, high):
    from tfep_amd.analysis import bootstrap_resample_indices
    rows = {}
    for offset in (0, 3):
        got = bootstrap_resample_indices(5, sample_size, high, seed=2 ** 40 + 17, offset=offset, device='cuda')
        assert got.dtype == torch.int64 and got.shape == (5, sample_size) and got.is_cuda
        rows[offset] = _np(got)
        assert np.array_equal(rows[offset], rr.indices(5, sample_size, high, 2 ** 40 + 17, offset))
        assert rows[offset].min() >= 0 and rows[offset].max() < high
    assert np.array_equal(rows[0][3:], rows[3][:2])


@pytest.mark.parametrize('sample_size', [1, 2, 3, 600])
def test_weights_equal_the_restatement(sample_size):
    from tfep_amd.analysis import bootstrap_resample_weights
    rows = {}
    for offset in (0, 3):
        got = bootstrap_resample_weights(5, sample_size, seed=2 ** 62 + 5, offset=offset, device='cuda')
        assert got.dtype == F64 and got.shape == (5, sample_size)
        rows[offset] = _np(got)
        np.testing.assert_allclose(rows[offset], rr.weights(5, sample_size, 2 ** 62 + 5, offset), rtol=1e-14, atol=0)
        np.testing.assert_allclose(rows[offset].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert np.array_equal(rows[0][3:], rows[3][:2])
    assert bootstrap_resample_weights(0, sample_size, seed=1, device='cuda').shape == (0, sample_size)


# ------------------------------------------------------------------ 2. the table route against the explicit one and torch

@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('seed', range(8))
def test_resampled_against_explicit_kernel_and_torch_logsumexp(seed, dtype):
    from tfep_amd.analysis import (bootstrap_fep, bootstrap_fep_resampled, bootstrap_resample_indices,
                                   bootstrap_resample_weights)
    rng = np.random.default_rng(100 + seed)
    N = int(rng.integers(1, 5000))
    R = int(rng.integers(1, 40))
    S = int(rng.integers(1, 2 * N + 1))
    kT = float(rng.uniform(0.3, 3.0))
    if dtype == F32:
        kT = float(np.float32(kT))                                 # the float32 C ABI takes kT as a float
    gen = torch.Generator().manual_seed(seed)
    work = (torch.randn(N, generator=gen, dtype=dtype) * float(rng.uniform(0.1, 30.0))).cuda()
    bias = torch.randn(N, generator=gen, dtype=dtype).cuda()
    biased = torch.stack([work, bias], dim=1)
    offset, high = int(rng.integers(0, 1000)), int(rng.integers(1, N + 1))
    for hi in (N, high):
        idx = bootstrap_resample_indices(R, S, hi, seed=seed, offset=offset, device='cuda')
        assert int(idx.max()) < hi
        kw = dict(seed=seed, offset=offset, high=hi, kT=kT)
        got = bootstrap_fep_resampled(work, R, S, **kw)
        assert got.dtype == F64 and got.shape == (R,)
        np.testing.assert_allclose(_np(got), _np(bootstrap_fep(work, indices=idx, kT=kT)), **TOL)
        np.testing.assert_allclose(_np(got), _np(_formula(work, idx, kT)), **TOL)
        got = bootstrap_fep_resampled(biased, R, S, **kw)
        np.testing.assert_allclose(_np(got), _np(bootstrap_fep(biased, indices=idx, kT=kT)), **TOL)
        np.testing.assert_allclose(_np(got), _np(_formula(work, idx, kT, bias)), **TOL)
        # the Bayesian mode: one weight per item of data[:hi]
        wts = bootstrap_resample_weights(R, hi, seed=seed, offset=offset, device='cuda')
        got = bootstrap_fep_resampled(work, R, seed=seed, offset=offset, high=hi, bayesian=True, kT=kT)
        np.testing.assert_allclose(_np(got), _np(_formula_weights(work[:hi], wts, kT)), **TOL)
        # the explicit kernel on the same values and the same float64 weights ...
        np.testing.assert_allclose(_np(got), _np(bootstrap_fep(work[:hi].double(), weights=wts, kT=kT)), **TOL)
        if dtype == F32:
            # ... and the float32 one, which rounds each weight to float32: w (1 + d), |d| <= 2^-24, moves the weighted sum
            # by a factor within 1 -+ 2^-24 and so the estimate by at most kT 2^-24 (1 + 2^-25), beyond its own 1e-9
            np.testing.assert_allclose(_np(got), _np(bootstrap_fep(work[:hi], weights=wts, kT=kT)), rtol=1e-9,
                                       atol=1e-9 + kT * 2.0 ** -24 * (1 + 2.0 ** -25))
    # sample_size defaults to high, high to len(data); a batch is a slice of the whole
    whole = bootstrap_fep_resampled(work, R, seed=seed, kT=kT)
    assert torch.equal(whole, bootstrap_fep_resampled(work, R, N, seed=seed, high=N, kT=kT))
    assert torch.equal(whole[R // 2:], bootstrap_fep_resampled(work, R - R // 2, seed=seed, offset=R // 2, kT=kT))
    assert torch.equal(whole, bootstrap_fep_resampled(work, R, seed=seed, kT=kT))       # and reproducible bit for bit


# ------------------------------------------------------------------ 3. the replay

FALLBACK_SEED = 3


def _fallback_indices():
    """(64, 2) draws from 4 items; at least 8 resamples draw item 0 and at least 8 miss it (a miss has probability 9/16)."""
    idx = rr.indices(64, 2, 4, FALLBACK_SEED)
    hits = int((idx == 0).any(axis=1).sum())
    assert 8 <= hits <= 56, hits
    return idx


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('large', [2000.0, 740.0])
def test_underflowing_resamples_are_replayed(large, dtype):
    """exp(-2000) is 0 and exp(-740) is denormal: a sum taken from the table would be -inf, or about 1 % off."""
    from tfep_amd.analysis import bootstrap_fep, bootstrap_fep_resampled, bootstrap_resample_indices
    want_idx = _fallback_indices()
    work = torch.tensor([0.0, large, large, large], dtype=dtype, device='cuda')
    idx = bootstrap_resample_indices(64, 2, 4, seed=FALLBACK_SEED, device='cuda')
    assert np.array_equal(_np(idx), want_idx)
    got = bootstrap_fep_resampled(work, 64, 2, seed=FALLBACK_SEED)
    want = _formula(work, idx, 1.0)
    np.testing.assert_allclose(_np(got), _np(want), **TOL)
    miss = ~(want_idx == 0).any(axis=1)
    assert miss.sum() >= 8 and (~miss).sum() >= 8
    # two misses give `large` exactly; a hit gives log 2 minus the logarithm of its number of zeros, give or take exp(-large)
    zeros = (want_idx == 0).sum(axis=1)
    np.testing.assert_allclose(_np(got)[miss], large, **TOL)
    np.testing.assert_allclose(_np(got)[~miss], np.log(2.0) - np.log(zeros[~miss]), **TOL)
    assert torch.equal(got, bootstrap_fep(work, indices=idx))             # the replay is the explicit kernel's arithmetic
    # with a bias column: the sum of the biases' table underflows where item 0 is missed
    data = torch.stack([torch.zeros(4, dtype=dtype, device='cuda'), -work], dim=1)
    got = bootstrap_fep_resampled(data, 64, 2, seed=FALLBACK_SEED)
    np.testing.assert_allclose(_np(got), _np(_formula(data[:, 0], idx, 1.0, data[:, 1])), **TOL)
    assert torch.equal(got, bootstrap_fep(data, indices=idx))
    # the Bayesian sum always holds the item of the maximum, so it does not underflow; the maximum carries the offset
    from tfep_amd.analysis import bootstrap_resample_weights
    shifted = work + large
    wts = bootstrap_resample_weights(64, 4, seed=FALLBACK_SEED, device='cuda')
    got = bootstrap_fep_resampled(shifted, 64, seed=FALLBACK_SEED, bayesian=True)
    np.testing.assert_allclose(_np(got), _np(_formula_weights(shifted, wts, 1.0)), **TOL)


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('bad', [float('nan'), float('-inf'), float('inf')], ids=['nan', '-inf', '+inf'])
def test_non_finite_work_values_give_what_the_explicit_route_gives(bad, dtype):
    from tfep_amd.analysis import (bootstrap_fep, bootstrap_fep_resampled, bootstrap_resample_indices,
                                   bootstrap_resample_weights)
    gen = torch.Generator().manual_seed(4)
    work = torch.randn(37, generator=gen, dtype=dtype)
    work[5] = bad
    work = work.cuda()
    biased = torch.stack([work, torch.randn(37, generator=gen, dtype=dtype).cuda()], dim=1)
    idx = bootstrap_resample_indices(48, 25, 37, seed=21, device='cuda')
    hit = (idx == 5).any(dim=1)
    assert 8 <= int(hit.sum()) <= 40                                     # resamples with and without the bad item
    for data in (work, biased):
        got, want = bootstrap_fep_resampled(data, 48, 25, seed=21, kT=0.7), bootstrap_fep(data, indices=idx, kT=0.7)
        np.testing.assert_allclose(_np(got), _np(want), equal_nan=True, **TOL)
        assert torch.equal(got.isnan(), want.isnan()) and torch.equal(got.isinf(), want.isinf())
        if bad == float('inf'):                                          # exp(-inf) = 0: the item only counts in log S
            assert bool(got.isfinite().all())
        else:                                                            # NaN; the estimate is -inf where work is -inf
            assert not bool(got[hit].isfinite().any()) and bool(got[~hit].isfinite().all())
    wts = bootstrap_resample_weights(48, 37, seed=21, device='cuda')
    # the same values as float64, so that the explicit kernel takes the weights as they are (float32 data round them)
    got, want = bootstrap_fep_resampled(work, 48, seed=21, bayesian=True), bootstrap_fep(work.double(), weights=wts)
    np.testing.assert_allclose(_np(got), _np(want), equal_nan=True, **TOL)
    assert torch.equal(got.isnan(), want.isnan()) and torch.equal(got.isinf(), want.isinf())


# ------------------------------------------------------------------ 4. float64 data are not cast

def test_float64_data_are_not_cast_to_float32():
    """Work values near 1e5 kT: the float32 spacing there is 7.8e-3, a cast errs by up to 4e-3 per value; rtol = 1e-9 is
    1e-4 absolute."""
    from tfep_amd.analysis import bootstrap_fep, bootstrap_fep_resampled, bootstrap_resample_indices
    work = (1e5 + torch.randn(2000, dtype=F64, generator=torch.Generator().manual_seed(8))).cuda()
    idx = bootstrap_resample_indices(30, 2000, 2000, seed=9, device='cuda')
    want = _formula(work, idx, 1.0)
    np.testing.assert_allclose(_np(bootstrap_fep(work, indices=idx)), _np(want), **TOL)
    np.testing.assert_allclose(_np(bootstrap_fep_resampled(work, 30, seed=9)), _np(want), **TOL)
    wts = torch.distributions.Dirichlet(torch.ones(2000, dtype=F64)).sample((7,)).cuda()
    np.testing.assert_allclose(_np(bootstrap_fep(work, weights=wts)), _np(_formula_weights(work, wts, 1.0)), **TOL)
    # and the bias column
    data = torch.stack([work, 1e3 + torch.randn(2000, dtype=F64, device='cuda')], dim=1)
    np.testing.assert_allclose(_np(bootstrap_fep(data, indices=idx, kT=1.3)), _np(_formula(work, idx, 1.3, data[:, 1])), **TOL)


# ------------------------------------------------------------------ 5. bootstrap(..., resampler='kernel')

KEYS = ('low', 'high', 'standard_deviation', 'mean', 'median')


def _five(res):
    return [res['confidence_interval']['low'], res['confidence_interval']['high'], res['standard_deviation'], res['mean'],
            res['median']]


def _work(dtype=F32):
    return torch.from_numpy(gu.load('bootstrap.npz')['work']).to(dtype).cuda()


@pytest.mark.parametrize('bayesian', [False, True])
def test_batches_change_no_value_and_seeds_do(bayesian):
    from tfep_amd.analysis import bootstrap, bootstrap_fep_resampled, fep_estimator
    work = _work()

    def run(seed, **extra):
        """The Bayesian bootstrap takes no generator: its seed comes from the device's default generator."""
        if not bayesian:
            return _five(bootstrap(work, fep_estimator, n_resamples=250, generator=seed, resampler='kernel', **extra))
        torch.manual_seed(seed)
        return _five(bootstrap(work, fep_estimator, n_resamples=250, bayesian=True, resampler='kernel', **extra))

    whole, batched = run(11), run(11, batch=64)
    for key, a, b in zip(KEYS, whole, batched):
        assert torch.equal(a, b) and a.dtype == work.dtype, key
    assert all(torch.equal(a, b) for a, b in zip(whole, run(11)))
    assert not any(torch.equal(a, b) for a, b in zip(whole, run(12)))
    # the distribution is that of bootstrap_fep_resampled on the same seed
    torch.manual_seed(11)
    stream_seed = int(torch.randint(0, 2 ** 63 - 1, (1,), device='cuda')) if bayesian else 11
    stats = bootstrap_fep_resampled(work, 250, seed=stream_seed, bayesian=bayesian).to(work.dtype)
    assert torch.equal(whole[3], stats.mean()) and torch.equal(whole[4], stats.median())


def test_generators_give_the_seed():
    from tfep_amd.analysis import bootstrap, fep_estimator
    work = _work()
    kw = dict(n_resamples=100, resampler='kernel')
    for make in (lambda: torch.Generator().manual_seed(7), lambda: torch.Generator('cuda').manual_seed(7)):
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=make(), device=make().device))
        a, b = bootstrap(work, fep_estimator, generator=make(), **kw), bootstrap(work, fep_estimator, generator=seed, **kw)
        assert all(torch.equal(x, y) for x, y in zip(_five(a), _five(b)))
    torch.manual_seed(3)
    a = bootstrap(work, fep_estimator, **kw)
    torch.manual_seed(3)
    assert all(torch.equal(x, y) for x, y in zip(_five(a), _five(bootstrap(work, fep_estimator, **kw))))


def test_sample_sizes_take_first_only_float64_basic_and_partial():
    from tfep_amd.analysis import bootstrap, bootstrap_fep_resampled, bootstrap_resample_indices, fep_estimator
    work = _work(F64)
    res = bootstrap(work, fep_estimator, n_resamples=200, bootstrap_sample_size=[50, 300], take_first_only=True, generator=5,
                    resampler='kernel')
    assert isinstance(res, list) and len(res) == 2
    assert all(v.dtype == F64 for r in res for v in _five(r))
    assert int(bootstrap_resample_indices(200, 50, 50, seed=5, device='cuda').max()) < 50
    # the second size takes the next 200 resample numbers, over data[:300]
    for i, size in enumerate((50, 300)):
        stats = bootstrap_fep_resampled(work, 200, size, seed=5, offset=200 * i, high=size)
        assert torch.equal(res[i]['mean'], stats.mean())
    width = [float(r['confidence_interval']['high'] - r['confidence_interval']['low']) for r in res]
    assert width[0] > width[1] > 0
    # without take_first_only the draws range over all the data
    res = bootstrap(work, fep_estimator, n_resamples=200, bootstrap_sample_size=50, generator=5, resampler='kernel')
    assert torch.equal(res['mean'], bootstrap_fep_resampled(work, 200, 50, seed=5).mean())
    # method='basic' reflects the percentile interval about the estimate of the data; a partial fixes kT
    kw = dict(n_resamples=200, generator=5, resampler='kernel')
    half = functools.partial(fep_estimator, kT=2.0)
    perc, basic = bootstrap(work, half, **kw), bootstrap(work, half, method='basic', **kw)
    full = half(work.unsqueeze(0), vectorized=True).reshape(())
    assert torch.equal(basic['confidence_interval']['low'], 2 * full - perc['confidence_interval']['high'])
    assert torch.equal(basic['confidence_interval']['high'], 2 * full - perc['confidence_interval']['low'])
    assert torch.equal(perc['mean'], bootstrap_fep_resampled(work, 200, seed=5, kT=2.0).mean())
    assert not torch.equal(perc['mean'], bootstrap(work, fep_estimator, **kw)['mean'])


@pytest.mark.parametrize('bayesian', [False, True])
def test_fep_estimator_bootstrap_statistics_on_the_kernel_route(bayesian):
    """Work values ~ N(0, 1) give dF ~ -0.5, as tests/test_gpu_bootstrap.py checks on the torch route."""
    from tfep_amd.analysis import bootstrap, fep_estimator
    work = torch.randn(10000, device='cuda', generator=torch.Generator('cuda').manual_seed(1))
    res = bootstrap(work, fep_estimator, n_resamples=2000, batch=500, bayesian=bayesian, method='basic',
                    generator=None if bayesian else 3, resampler='kernel')
    assert abs(float(res['mean']) + 0.5) < 0.1
    assert float(res['confidence_interval']['low']) < float(res['median']) < float(res['confidence_interval']['high'])
    # the spread of the bootstrap distribution is that of the torch route (standard error of the estimator, ~ 0.013)
    ref = bootstrap(work, fep_estimator, n_resamples=2000, bayesian=bayesian, generator=None if bayesian else 3)
    assert 0.8 < float(res['standard_deviation']) / float(ref['standard_deviation']) < 1.25
