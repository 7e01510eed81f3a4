"""Host side of the bootstrap with in-kernel resampling (csrc/bootstrap_rng.h, csrc/reduce.hip, analysis/bootstrap.py): the
numpy restatement of the stream (tests/bootstrap_rng_ref.py) on the known-answer vectors of Philox4x32-10 and on the ranges
its draws must keep, the C ABI tables, and every argument check of the Python entry points, which are made before a library
is loaded or a kernel launched.  No GPU."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import bootstrap_rng_ref as rr
from tfep_amd import _lib
from tfep_amd.analysis import (bootstrap, bootstrap_fep, bootstrap_fep_resampled, bootstrap_resample_indices,
                               bootstrap_resample_weights, fep_estimator)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> number of arguments in include/tfep_hip.h
ARITY = {'tfep_bootstrap_fep': 10, 'tfep_bootstrap_table': 9, 'tfep_bootstrap_fep_resampled': 15,
         'tfep_bootstrap_table_workspace_doubles': 1, 'tfep_bootstrap_resample_indices': 7, 'tfep_bootstrap_resample_weights': 6}
TWINS = {'tfep_bootstrap_fep': 7, 'tfep_bootstrap_table': 3, 'tfep_bootstrap_fep_resampled': 12}     # name -> position of kT

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


# ------------------------------------------------------------------ the stream

@pytest.mark.parametrize('counter,key,want', KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    assert tuple(int(w) for w in rr.philox4x32_10(counter, key)) == want


def test_words_are_the_philox_output_of_the_documented_counter_and_key():
    seed, r = (0x299f31d0 << 32) | 0xa4093822, 0x13198a2e
    w = rr.words(seed, r, 3, rr.STREAM_WEIGHTS)
    assert w.shape == (3, 4)
    for q in range(3):
        assert tuple(int(x) for x in w[q]) == tuple(int(x) for x in rr.philox4x32_10((q, 0, r, 1), (0xa4093822, 0x299f31d0)))
    assert not np.array_equal(w, rr.words(seed, r, 3, rr.STREAM_INDICES))


@pytest.mark.parametrize('high', [1, 7, 600, 2 ** 31 - 1])
def test_index_draws_stay_below_high(high):
    idx = rr.indices(3, 1027, high, seed=5, offset=2 ** 31 - 3)          # up to the last resample number
    assert idx.dtype == np.int64 and idx.shape == (3, 1027)
    assert idx.min() >= 0 and idx.max() < high
    if high > 1:
        assert idx.max() > high // 2 and len(np.unique(idx)) > min(high, 1027) // 2      # and they spread over the range
    # the largest word maps to high - 1
    assert (0xffffffff * high) >> 32 == high - 1


def test_draws_depend_on_seed_resample_and_position_alone():
    a = rr.indices(5, 9, 600, seed=3)
    assert np.array_equal(a[3:], rr.indices(2, 9, 600, seed=3, offset=3))
    assert np.array_equal(a[:, :5], rr.indices(5, 5, 600, seed=3))       # a shorter resample is a prefix
    assert not np.array_equal(a, rr.indices(5, 9, 600, seed=4))
    w = rr.weights(4, 6, seed=3)
    assert np.allclose(w[2:], rr.weights(2, 6, seed=3, offset=2), rtol=0, atol=0)


@pytest.mark.parametrize('sample_size', [1, 2, 3, 600, 4097])
def test_weight_rows_sum_to_one(sample_size):
    u = rr.uniforms(4, sample_size, seed=11)
    assert u.min() > 0.0 and u.max() <= 1.0
    w = rr.weights(4, sample_size, seed=11)
    assert w.shape == (4, sample_size) and w.min() >= 0.0
    assert np.abs(w.sum(axis=1) - 1.0).max() < 1e-12
    if sample_size >= 600:                                               # E_j are standard exponentials: mean 1, variance 1
        e = -np.log(u)
        assert abs(e.mean() - 1.0) < 5.0 / np.sqrt(e.size) and abs(e.var() - 1.0) < 15.0 / np.sqrt(e.size)


# ------------------------------------------------------------------ C ABI

def test_c_abi_tables():
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    sig = _lib._SIGNATURES
    names = list(ARITY) + [n + '_f64' for n in TWINS]
    assert sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith('tfep_bootstrap_')) == sorted(names)
    for name in names:
        declared = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', header)
        assert declared, name
        arity = len(declared.group(1).split(','))
        assert arity == len(sig[name][1]) == ARITY[name.replace('_f64', '')], name
    for name, kT in TWINS.items():
        f32, f64 = sig[name][1], sig[name + '_f64'][1]
        assert f32[kT] is _lib.c_float and f64[kT] is _lib.c_double and f32[:kT] + f32[kT + 1:] == f64[:kT] + f64[kT + 1:], name
    assert sig['tfep_bootstrap_table_workspace_doubles'] == (_lib.c_int64, [_lib.c_int64])
    assert _lib.ABI_VERSION == 8 and re.search(r'#define\s+TFEP_HIP_ABI_VERSION\s+8\b', header)
    assert os.path.exists(os.path.join(ROOT, 'tfep_amd', 'csrc', 'bootstrap_rng.h'))


# ------------------------------------------------------------------ argument checks, before any library or launch

@pytest.fixture
def no_library(monkeypatch):
    """Loading the library, and so any launch, fails the test."""
    def refuse(*args, **kwargs):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', refuse)
    monkeypatch.setattr(_lib, 'call', refuse)


def test_signatures():
    p = inspect.signature(bootstrap_fep_resampled).parameters
    assert list(p) == ['data', 'n_resamples', 'sample_size', 'seed', 'offset', 'high', 'bayesian', 'kT']
    assert p['sample_size'].default is None and p['seed'].default is inspect.Parameter.empty
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('seed', 'offset', 'high', 'bayesian', 'kT'))
    assert (p['offset'].default, p['high'].default, p['bayesian'].default, p['kT'].default) == (0, None, False, 1.0)
    assert list(inspect.signature(bootstrap_resample_indices).parameters) == ['n_resamples', 'sample_size', 'high', 'seed',
                                                                              'offset', 'device']
    assert list(inspect.signature(bootstrap_resample_weights).parameters) == ['n_resamples', 'sample_size', 'seed', 'offset',
                                                                              'device']
    resampler = inspect.signature(bootstrap).parameters['resampler']
    assert resampler.default == 'torch' and resampler.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(bootstrap_fep).parameters) == ['data', 'indices', 'weights', 'kT']


@pytest.mark.parametrize('kwargs,match', [
    (dict(seed=-1), 'seed'),
    (dict(seed=2 ** 63), 'seed'),
    (dict(seed=1.5), 'seed'),
    (dict(seed=1, offset=2 ** 31 - 3), r'2\*\*31'),
    (dict(seed=1, offset=-1), 'offset'),
    (dict(seed=1, high=0), 'high'),
    (dict(seed=1, high=101), 'high'),
    (dict(seed=1, sample_size=0), 'sample_size'),
    (dict(seed=1, sample_size=50, bayesian=True), 'Bayesian'),
    (dict(seed=1, high=50, sample_size=100, bayesian=True), 'Bayesian'),
])
def test_resampled_argument_checks(no_library, kwargs, match):
    data = torch.zeros(100, dtype=torch.float64)
    with pytest.raises(ValueError, match=match):
        bootstrap_fep_resampled(data, 4, **kwargs)


def test_resample_ops_argument_checks(no_library):
    for kwargs in (dict(seed=-1), dict(seed=2 ** 63), dict(seed=0, offset=2 ** 31)):
        with pytest.raises(ValueError):
            bootstrap_resample_indices(1, 4, 10, device='cuda', **kwargs)
        with pytest.raises(ValueError):
            bootstrap_resample_weights(1, 4, device='cuda', **kwargs)
    for high in (0, -3, 2 ** 31):
        with pytest.raises(ValueError, match='high'):
            bootstrap_resample_indices(1, 4, high, seed=0, device='cuda')
    with pytest.raises(ValueError, match='sample_size'):
        bootstrap_resample_indices(1, 0, 10, seed=0, device='cuda')
    with pytest.raises(ValueError, match='sample_size'):
        bootstrap_resample_weights(1, 0, seed=0, device='cuda')
    with pytest.raises(NotImplementedError):                             # as bootstrap_fep with weights
        bootstrap_fep_resampled(torch.zeros(10, 2), 3, seed=0, bayesian=True)


def test_bootstrap_kernel_route_argument_checks(no_library):
    data = torch.zeros(100)

    def mean(x, weights=None, vectorized=True):
        return x.mean(-1)

    with pytest.raises(ValueError, match='resampler'):
        bootstrap(data, fep_estimator, resampler='numpy')
    with pytest.raises(ValueError, match='resampler'):
        bootstrap(data, mean, resampler='numpy')                         # also where the statistic is not the estimator
    for statistic in (mean, functools.partial(fep_estimator, vectorized=True), functools.partial(fep_estimator, data)):
        with pytest.raises(ValueError, match='fep_estimator'):
            bootstrap(data, statistic, resampler='kernel')
    for seed in (-1, 2 ** 63):
        with pytest.raises(ValueError, match='seed'):
            bootstrap(data, fep_estimator, resampler='kernel', generator=seed)
    with pytest.raises(ValueError, match=r'2\*\*31'):
        bootstrap(data, fep_estimator, resampler='kernel', generator=1, n_resamples=2 ** 31 + 1)
    with pytest.raises(ValueError, match=r'2\*\*31'):                    # the sizes take consecutive ranges of resample numbers
        bootstrap(data, fep_estimator, resampler='kernel', generator=1, n_resamples=2 ** 30 + 1, bootstrap_sample_size=[5, 6])
    with pytest.raises(ValueError, match='high'):
        bootstrap(data, fep_estimator, resampler='kernel', generator=1, bootstrap_sample_size=[50, 101], take_first_only=True)
    with pytest.raises(ValueError, match='sample_size'):
        bootstrap(data, fep_estimator, resampler='kernel', generator=1, bootstrap_sample_size=0)
    # the reference's own errors come first, as on the torch route
    with pytest.raises(ValueError, match='generator'):
        bootstrap(data, fep_estimator, resampler='kernel', bayesian=True, generator=1)
    with pytest.raises(ValueError, match='take_first_only'):
        bootstrap(data, fep_estimator, resampler='kernel', bayesian=True, bootstrap_sample_size=[10])
    with pytest.raises(ValueError, match='exactly one'):
        bootstrap_fep(data)


def test_the_seed_of_the_kernel_route():
    from tfep_amd.analysis.bootstrap import _kernel_seed
    assert _kernel_seed(11, torch.device('cpu')) == 11
    want = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=torch.Generator().manual_seed(5)))
    assert _kernel_seed(torch.Generator().manual_seed(5), torch.device('cpu')) == want
    torch.manual_seed(5)
    first = _kernel_seed(None, torch.device('cpu'))
    assert first == want and _kernel_seed(None, torch.device('cpu')) != first        # the default generator moves on
    torch.manual_seed(5)
    assert _kernel_seed(None, torch.device('cpu')) == first


def test_no_cpu_fallback():
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        bootstrap_fep_resampled(torch.zeros(10, dtype=torch.float64), 3, seed=0)
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        bootstrap(torch.zeros(10), fep_estimator, n_resamples=3, resampler='kernel', generator=2)
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        bootstrap_fep(torch.zeros(10, dtype=torch.float64), indices=torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        bootstrap_resample_indices(2, 3, 10, seed=0, device='cpu')
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        bootstrap_resample_weights(2, 3, seed=0, device='cpu')
