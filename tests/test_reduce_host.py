"""The reference of the reduction tests (tests/reduce_ref.py) is tied to the oracle and to the reference's formulas, its
cases meet the conditions the bounds rest on, the bounds can fail, and ``combine_stats`` merges reference statistics.
No GPU: tests/test_gpu_reduce.py holds the kernels to the same reference and the same bounds."""
import numpy as np
import pytest
import torch

import golden_util as gu
import reduce_ref as rr
from oracle import loss as oloss
from tfep_amd.distributed import combine_stats

F64 = torch.float64
KT = rr.KT


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64))


def torch_loss(case, weighted, ignore_nan=False):
    """The reference's loss (loss.py:125-140) in float64 on the CPU."""
    r = _t(case['uB'])
    if case['ldj'] is not None:
        r = r - _t(case['ldj'])
    if case['uA'] is not None:
        r = r - _t(case['uA'])
    if weighted:
        w = torch.softmax(_t(case['lw']), dim=0)
        return float(torch.nansum(w * r) if ignore_nan else torch.sum(w * r))
    return float(torch.nanmean(r) if ignore_nan else torch.mean(r))


def torch_fep(work, bias=None, weights=None, kT=1.0):
    """The reference's estimator (estimator.py:73-86) in float64 on the CPU."""
    work = _t(work)
    if bias is not None:
        log_weights = torch.log_softmax(_t(bias) / kT, dim=-1)
    elif weights is not None:
        log_weights = torch.log(_t(weights))
    else:
        log_weights = -torch.log(torch.tensor(float(work.shape[-1]), dtype=F64))
    return float(-kT * torch.logsumexp(-work / kT + log_weights, dim=-1))


def _close(got, ref, what):
    ratio = rr.scalar_ratio(got, ref)
    assert ratio <= 1.0, (what, got, ref, ratio)


def _both(case, what, ignore_nan=False):
    """Loss (weighted or not) and dF (biased or not) of a float64 case against the torch formulas."""
    stats, _ = rr.stats_ref(**case, kT=KT, ignore_nan=ignore_nan)
    weighted, biased = case['lw'] is not None, case['bias'] is not None
    loss, dF = rr.finalize(stats, weighted=weighted, biased=biased, kT=KT)
    with np.errstate(all='ignore'):
        work = rr.lse_arguments(**case, kT=KT)[0]
    if len(work):
        _close(loss, torch_loss(case, weighted, ignore_nan), (what, 'loss'))
        _close(dF, torch_fep(work, case['bias'], kT=KT), (what, 'dF'))
    else:
        assert np.isnan(loss), what
    return loss, dF


# ------------------------------------------------------------------ the oracle on the golden samples

def test_reference_reproduces_the_oracle_on_the_golden_samples():
    g = gu.load('loss.npz')
    uB, ldj, lw, uA = (g[k].astype(np.float64) for k in ('uB', 'ldj', 'lw', 'uA'))

    def loss(uB, ldj=None, lw=None, uA=None, ignore_nan=False):
        stats, _ = rr.stats_ref(uB, ldj, uA, lw, ignore_nan=ignore_nan)
        return rr.finalize(stats, weighted=lw is not None)[0]

    for what, kw in (('plain', dict(ldj=ldj)), ('ref', dict(ldj=ldj, uA=uA)), ('weighted', dict(ldj=ldj, lw=lw)),
                     ('all', dict(ldj=ldj, lw=lw, uA=uA)), ('noldj', dict())):
        ref = oloss.boltzmann_kl_div_loss(uB, kw.get('ldj'), kw.get('lw'), kw.get('uA'))
        _close(loss(uB, **kw), ref, what)
        _close(loss(uB, **kw), g[f'loss_{what}_f64'], what)
    un = uB.copy()
    un[[3, 77]] = np.nan
    _close(loss(un, ldj, ignore_nan=True), oloss.boltzmann_kl_div_loss(un, ldj, ignore_nan=True), 'nan plain')
    _close(loss(un, ldj, lw, ignore_nan=True), oloss.boltzmann_kl_div_loss(un, ldj, lw, ignore_nan=True), 'nan weighted')
    assert np.isnan(loss(un, ldj)) and np.isnan(loss(un, ldj, lw))
    stats, _ = rr.stats_ref(un, ldj, ignore_nan=True)
    assert np.isnan(stats[5] + np.log(stats[6]))

    def fep(work, bias=None, weights=None, kT=1.0):
        extra = bias if weights is None else np.log(weights) * kT
        stats, _ = rr.stats_ref(work, bias=extra, kT=kT)
        return rr.finalize(stats, biased=bias is not None, bayesian=weights is not None, kT=kT)[1]

    work = uB - ldj - uA
    _close(fep(work), oloss.fep_estimator(work), 'fep plain')
    _close(fep(work * 2.5, kT=2.5), oloss.fep_estimator(work * 2.5, kT=2.5), 'fep kT')
    _close(fep(work, bias=lw), oloss.fep_estimator(np.stack([work, lw], axis=1)), 'fep biased')
    vec, weights, vecb = g['fep_vec_in_f64'], g['fep_bayes_w_f64'], g['fep_vecb_in_f64']
    for got, ref, key in (([fep(v) for v in vec], oloss.fep_estimator(vec, vectorized=True), 'fep_vec_f64'),
                          ([fep(work, weights=w) for w in weights],
                           oloss.fep_estimator(np.broadcast_to(work, (4, work.size)), weights=weights, vectorized=True),
                           'fep_bayes_f64'),
                          ([fep(v[:, 0], bias=v[:, 1]) for v in vecb], oloss.fep_estimator(vecb, vectorized=True),
                           'fep_vecb_f64')):
        for a, b, c in zip(got, ref, g[key]):
            _close(a, b, key)
            _close(a, c, key)


# ------------------------------------------------------------------ the reference's formulas on the cases of the GPU tests

@pytest.mark.parametrize('N', rr.SIZES)
def test_reference_matches_the_torch_formulas_at_every_size(N):
    _both(rr.wide_case(N, 60), N)
    if N == 0:
        stats, _ = rr.stats_ref(**rr.wide_case(0, 60), kT=KT)
        assert np.array_equal(stats, [0, 0, -np.inf, 0, 0, -np.inf, 0, -np.inf, 0])


def test_reference_matches_the_torch_formulas_without_the_optional_inputs():
    for absent in rr.ABSENT:
        some = rr.wide_case(rr.CAP + 1, 60, absent=absent)
        _both(some, absent)
        stats, _ = rr.stats_ref(**some, kT=KT)
        if 'lw' in absent:
            assert stats[2] == -np.inf and stats[3] == 0.0 and stats[4] == 0.0
        if 'bias' in absent:
            assert stats[7] == -np.inf and stats[8] == 0.0


@pytest.mark.parametrize('name', list(rr.ARRANGEMENTS))
def test_reference_matches_the_torch_formulas_over_a_wide_range(name):
    case = rr.wide_case(rr.N_WIDE, 4000, **rr.ARRANGEMENTS[name])
    _both(case, name)
    if name in ('ascending', 'descending'):              # the same values in another order
        step = 1 if name == 'ascending' else -1
        assert np.array_equal(case['lw'][::step], np.sort(rr.wide_case(rr.N_WIDE, 4000)['lw']))
        assert np.all(np.diff(case['lw'][::step]) >= 0) and np.all(np.diff(case['bias'][::step]) >= 0)
    with np.errstate(over='ignore', under='ignore'):      # a naive exp overflows, most terms underflow to zero
        assert np.exp(case['lw'].max()) == np.inf and (np.exp(case['lw'] - case['lw'].max()) == 0.0).mean() > 0.5


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('ignore_nan', [False, True])
def test_reference_follows_the_nan_rules(ignore_nan, weighted):
    case = rr.nan_case()
    case = case if weighted else dict(case, lw=None)
    stats, _ = rr.stats_ref(**case, kT=KT, ignore_nan=ignore_nan)
    clean, _ = rr.stats_ref(**dict(rr.wide_case(rr.N_WIDE, 60), lw=case['lw']), kT=KT)
    loss, dF = rr.finalize(stats, weighted=weighted, biased=True, kT=KT)
    ref = torch_loss(case, weighted, ignore_nan)
    assert np.isnan(dF) and np.isnan(stats[5] + np.log(stats[6]))
    assert stats[3] == clean[3] and stats[2] == clean[2]                 # NaN samples stay in the softmax
    if ignore_nan:
        assert stats[0] == rr.N_WIDE - len(rr.NAN_AT) and np.isfinite(ref)
        _close(loss, ref, 'loss')
    else:
        assert stats[0] == rr.N_WIDE and np.isnan(stats[1]) and np.isnan(loss) and np.isnan(ref)
        assert not weighted or np.isnan(stats[4])


@pytest.mark.parametrize('name', list(rr.INFINITIES))
def test_reference_matches_the_torch_formulas_on_infinities(name):
    loss, dF = _both(rr.infinity_case(name), name)
    if name in ('lw_all_minus_inf', 'lw_plus_inf'):
        assert np.isnan(loss)
    elif name == 'work_plus_inf':
        assert loss == np.inf and np.isfinite(dF)
    elif name.startswith('work_minus_inf'):
        assert loss == -np.inf and dF == -np.inf
    else:
        assert np.isfinite(loss) and np.isfinite(dF)


def test_torch_logsumexp_counts_equal_infinite_maxima():
    assert float(torch.logsumexp(torch.tensor([np.inf, np.inf, 0.0], dtype=F64), 0)) == np.inf
    assert np.isnan(float(torch.softmax(torch.tensor([np.inf, 0.0], dtype=F64), 0)[1]))


# ------------------------------------------------------------------ the conditions the bounds rest on

def _section3_wide_cases():
    for N in rr.SIZES:
        if N >= rr.CONDITIONED_FROM:
            yield f'N={N}', rr.wide_case(N, 60), 60
    for absent in rr.ABSENT:
        yield f'without {absent}', rr.wide_case(rr.CAP + 1, 60, absent=absent), 60
    for name, kw in rr.ARRANGEMENTS.items():
        yield name, rr.wide_case(rr.N_WIDE, 4000, **kw), 4000


def test_every_wide_case_meets_the_conditions_of_the_bounds():
    """Sizes below 1025 hold fewer than 100 terms in reach of the maximum and are there for the launch shapes alone; every
    other case of tests/test_gpu_reduce.py is checked here, in both dtypes."""
    for what, case, spread in _section3_wide_cases():
        for dtype in (np.float64, np.float32):
            cond = rr.assert_conditioned(case, spread, dtype)
            print(what, dtype.__name__, cond)


# ------------------------------------------------------------------ the bounds bite

@pytest.fixture(scope='module')
def widest():
    case = rr.wide_case(rr.N_WIDE, 60)
    return case, {dt: rr.stats_ref(**case, kT=KT, dtype=dt) for dt in (np.float32, np.float64)}


SUMS = ('sum_r', 's_w', 's_wr', 's_e', 's_b')


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_a_reduction_that_stops_after_one_grid_pass_misses_the_bounds(widest, dtype):
    case, ref = widest
    got, _ = rr.stats_ref(**{k: v[:rr.CAP] for k, v in case.items()}, kT=KT, dtype=dtype)
    ratio = rr.ratios(got, *ref[dtype])
    print(ratio)
    assert ratio['count'] == np.inf and all(ratio[k] >= 100.0 for k in SUMS)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_a_float32_accumulator_misses_the_bounds(widest, dtype):
    case, ref = widest
    got, _ = rr.stats_ref(**case, kT=KT, dtype=dtype, acc=np.float32)
    ratio = rr.ratios(got, *ref[dtype])
    print(ratio)
    assert all(ratio[k] >= 100.0 for k in SUMS)


def test_residuals_formed_in_float64_from_float32_inputs_miss_the_bounds(widest):
    case, ref = widest
    as_f32 = {k: v.astype(np.float32).astype(np.float64) for k, v in case.items()}
    got, _ = rr.stats_ref(**as_f32, kT=float(np.float32(KT)), dtype=np.float64)
    ratio = rr.ratios(got, *ref[np.float32])
    print(ratio)
    assert all(ratio[k] >= 100.0 for k in ('sum_r', 's_wr', 's_e'))
    assert ratio['s_w'] <= 1.0 and ratio['s_b'] <= 1.0 and ratio['m_w'] == 0.0       # these do not hold r


def test_one_lost_element_misses_the_bounds(widest):
    case, ref = widest
    got, _ = rr.stats_ref(**{k: v[:-1] for k, v in case.items()}, kT=KT)
    ratio = rr.ratios(got, *ref[np.float64])
    print(ratio)
    assert ratio['count'] == np.inf and max(ratio[k] for k in SUMS) >= 1e4


# ------------------------------------------------------------------ combine_stats on reference statistics

@pytest.mark.parametrize('infinite', [False, True], ids=['finite', 'two_infinite_maxima'])
def test_combine_stats_of_ragged_shards_is_the_statistics_of_the_whole(infinite):
    case = rr.wide_case(rr.CAP + 1, 60)
    if infinite:                                           # work = -inf in the first and in the last shard: m_e = +inf in both
        case = rr.with_values(case, uB={17: -np.inf, 100000: -np.inf})
    whole, scales = rr.stats_ref(**case, kT=KT)
    bounds = (0, 1000, 1000, rr.CAP + 1)                   # the second shard is empty
    shards = [rr.stats_ref(**{k: v[a:b] for k, v in case.items()}, kT=KT)[0] for a, b in zip(bounds, bounds[1:])]
    if infinite:
        assert shards[0][5] == np.inf and shards[2][5] == np.inf and whole[5] == np.inf and whole[6] == 2.0
    assert shards[1][0] == 0 and shards[1][5] == -np.inf
    got = combine_stats(torch.from_numpy(np.stack(shards))).numpy()
    ratio = rr.ratios(got, whole, scales)
    print(ratio)
    assert max(ratio.values()) <= 0.01, ratio
    assert got[0] == rr.CAP + 1 and got[5] == whole[5]
    # a +inf log-weight in two shards: the weight pair stays NaN, as torch.softmax gives
    case = rr.with_values(rr.wide_case(rr.CAP + 1, 60), lw={17: np.inf, 100000: np.inf})
    shards = [rr.stats_ref(**{k: v[a:b] for k, v in case.items()}, kT=KT)[0] for a, b in zip(bounds, bounds[1:])]
    got = combine_stats(torch.from_numpy(np.stack(shards))).numpy()
    assert np.isnan(got[3]) and np.isnan(got[4]) and np.isfinite(got[6])
