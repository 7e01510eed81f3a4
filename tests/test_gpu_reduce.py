"""The loss / estimator reduction (csrc/reduce.hip: tfep_reduce_partial_kernel, tfep_reduce_final_kernel, the bootstrap
kernel) past one pass of its grid, against the plain float64 restatement of tests/reduce_ref.py (tied to the oracle and
to the reference's formulas in tests/test_reduce_host.py, which also shows that the bounds below can fail).

The partial kernel launches min(1024, ceil(N / 256)) blocks and strides over the rest: N > 262 144 takes a second trip,
600 001 three with a ragged last one; the final kernel then merges 1024 partials in 4 trips of 256 threads.

Bounds (``reduce_ref.ratios``), derived, not measured: every sum within 1e-12 of the sum of the magnitudes of its terms,
``count`` and ``m_w`` exact, ``m_e`` / ``m_b`` within 4 ulp; the same for float32 inputs, whose reference starts from
the residuals formed in float32.  A loss or a dF finished from float64 statistics: ``1e-12 max(1, |ref|)``; a float32
loss adds the one rounding of its ``.to(float32)``.  Every figure is printed before it is asserted.
"""
import functools

import numpy as np
import pytest
import torch

import reduce_ref as rr
from tfep_amd.analysis import bootstrap_fep, fep_estimator
from tfep_amd.distributed import combine_stats
from tfep_amd.loss import BoltzmannKLDivLoss, reduce_stats

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NP = {F32: np.float32, F64: np.float64}
DTYPES = pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
KT = rr.KT


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.array(a)).to(device='cuda', dtype=dtype)


def _cpu(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64))


def _inputs(case, dtype):
    return {k: _dev(case[k], dtype) for k in rr.INPUTS}


def _kernel(dev, kT=KT, ignore_nan=False):
    stats = reduce_stats(dev['uB'], dev['ldj'], dev['uA'], dev['lw'], dev['bias'], kT=kT, ignore_nan=ignore_nan)
    assert stats.shape == (9,) and stats.dtype == F64
    return stats


@functools.lru_cache(maxsize=None)
def _case(kind, arg=None):
    """The cases of this module, built once.  The conditions the bounds rest on are asserted on the reference before
    anything is compared (sizes below 1025 are there for the launch shapes alone)."""
    if kind == 'size':
        case, spread = rr.wide_case(arg, 60), 60
    elif kind == 'absent':
        case, spread = rr.wide_case(rr.CAP + 1, 60, absent=arg), 60
    elif kind == 'arrangement':
        case, spread = rr.wide_case(rr.N_WIDE, 4000, **rr.ARRANGEMENTS[arg]), 4000
    elif kind == 'nan':
        return rr.nan_case()
    else:
        return rr.infinity_case(arg)
    if len(case['uB']) >= rr.CONDITIONED_FROM:
        for dtype in NP.values():
            cond = rr.assert_conditioned(case, spread, dtype)
            print(f'{kind} {arg} {dtype.__name__}: (terms >= 1e-6, largest share) per log-sum-exp {cond}')
    return case


@functools.lru_cache(maxsize=None)
def _ref(kind, arg, dtype, ignore_nan=False, weighted=True):
    case = _case(kind, arg)
    case = case if weighted else dict(case, lw=None)
    return rr.stats_ref(**case, kT=KT, ignore_nan=ignore_nan, dtype=NP[dtype])


def _check_stats(what, got, ref, scales):
    ratio = rr.ratios(got, ref, scales)
    print(f'{what}: |got - ref| / bound ' + ', '.join(f'{k} {v:.2e}' for k, v in ratio.items()))
    assert max(ratio.values()) <= 1.0, (what, ratio, got, ref)
    return ratio


def _check_scalar(what, got, ref, dtype=F64):
    """``1e-12 max(1, |ref|)``, plus one float32 rounding for a result that went through ``.to(float32)``."""
    got, ref = float(got), float(ref)
    if not (np.isfinite(ref) and np.isfinite(got)):
        print(f'{what}: {got} (reference {ref})')
        assert (np.isnan(got) and np.isnan(ref)) or got == ref, (what, got, ref)
        return
    bound = rr.REL * max(1.0, abs(ref)) + (2.0 ** -24 * abs(ref) if dtype == F32 else 0.0)
    print(f'{what}: {got!r} (reference {ref!r}), |got - ref| / bound {abs(got - ref) / bound:.2e}')
    assert abs(got - ref) <= bound, (what, got, ref)


def _check_finished(what, dev, got, ref, dtype, ignore_nan=False):
    """The module's loss and the dF finished from the kernel's statistics against the finished reference."""
    weighted, biased = dev['lw'] is not None, dev['bias'] is not None
    ref_loss, ref_dF = rr.finalize(ref, weighted=weighted, biased=biased, kT=KT)
    loss = BoltzmannKLDivLoss(ignore_nan=ignore_nan)(dev['uB'], dev['ldj'], dev['lw'], dev['uA'])
    assert loss.dtype == dtype and loss.shape == ()
    _check_scalar(f'{what} loss', loss, ref_loss, dtype)
    _check_scalar(f'{what} dF', rr.finalize(got, weighted=weighted, biased=biased, kT=KT)[1], ref_dF)


# ------------------------------------------------------------------ (a) sizes

@DTYPES
@pytest.mark.parametrize('N', rr.SIZES)
def test_statistics_at_every_launch_shape(N, dtype):
    dev = _inputs(_case('size', N), dtype)
    got = _kernel(dev).cpu().numpy()
    ref, scales = _ref('size', N, dtype)
    _check_stats(f'N={N} {NP[dtype].__name__}', got, ref, scales)
    _check_finished(f'N={N}', dev, got, ref, dtype)
    if N == 0:
        assert np.array_equal(got, [0, 0, -np.inf, 0, 0, -np.inf, 0, -np.inf, 0])
        assert torch.isnan(BoltzmannKLDivLoss()(dev['uB'], dev['ldj'], dev['lw'], dev['uA']))


# ------------------------------------------------------------------ (b) optional inputs

@pytest.mark.parametrize('absent', rr.ABSENT, ids=['-'.join(a) for a in rr.ABSENT])
def test_statistics_without_the_optional_inputs(absent):
    dev = _inputs(_case('absent', absent), F64)
    assert all(dev[k] is None for k in absent)
    got = _kernel(dev).cpu().numpy()
    ref, scales = _ref('absent', absent, F64)
    _check_stats(f'without {absent}', got, ref, scales)
    _check_finished(f'without {absent}', dev, got, ref, F64)
    if 'lw' in absent:
        assert got[2] == -np.inf and got[3] == 0.0 and got[4] == 0.0
    if 'bias' in absent:
        assert got[7] == -np.inf and got[8] == 0.0


# ------------------------------------------------------------------ (c) range and order

@DTYPES
@pytest.mark.parametrize('name', list(rr.ARRANGEMENTS))
def test_statistics_over_a_range_a_naive_exp_overflows_on(name, dtype):
    dev = _inputs(_case('arrangement', name), dtype)
    got = _kernel(dev).cpu().numpy()
    ref, scales = _ref('arrangement', name, dtype)
    _check_stats(f'{name} {NP[dtype].__name__}', got, ref, scales)
    _check_finished(name, dev, got, ref, dtype)
    assert np.isfinite(got).all()


# ------------------------------------------------------------------ (d) NaN

@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('ignore_nan', [False, True], ids=['propagate', 'ignore'])
def test_nan_samples_in_every_trip_follow_the_reference(ignore_nan, weighted):
    dev = _inputs(_case('nan'), F64)
    if not weighted:
        dev['lw'] = None
    got = _kernel(dev, ignore_nan=ignore_nan).cpu().numpy()
    ref, scales = _ref('nan', None, F64, ignore_nan, weighted)
    ratio = rr.ratios(got, ref, scales)
    shown = ('count', 'sum_r', 'm_w', 's_w', 's_wr', 'm_b', 's_b')
    print(f'ignore_nan={ignore_nan} weighted={weighted}: ' + ', '.join(f'{k} {ratio[k]:.2e}' for k in shown))
    assert max(ratio[k] for k in shown) <= 1.0, (ratio, got, ref)
    assert np.isnan(got[5] + np.log(got[6])), got
    # the module against the reference's nanmean / nansum in float64 on the CPU
    case = _case('nan')
    r = _cpu(case['uB']) - _cpu(case['ldj']) - _cpu(case['uA'])
    if weighted:
        p = torch.softmax(_cpu(case['lw']), dim=0) * r
        want = torch.nansum(p) if ignore_nan else torch.sum(p)
    else:
        want = torch.nanmean(r) if ignore_nan else torch.mean(r)
    loss = BoltzmannKLDivLoss(ignore_nan=ignore_nan)(dev['uB'], dev['ldj'], dev['lw'], dev['uA'])
    _check_scalar('loss', loss, want)
    assert bool(torch.isnan(want)) == (not ignore_nan)


# ------------------------------------------------------------------ (e) infinities

def _torch_reference(case):
    """Loss and dF by the reference's formulas (loss.py:125-140, estimator.py:73-86) in float64 on the CPU."""
    r = _cpu(case['uB']) - _cpu(case['ldj']) - _cpu(case['uA'])
    loss = torch.sum(torch.softmax(_cpu(case['lw']), dim=0) * r)
    log_weights = torch.log_softmax(_cpu(case['bias']) / KT, dim=-1)
    return float(loss), float(-KT * torch.logsumexp(-r / KT + log_weights, dim=-1))


@pytest.mark.parametrize('name', list(rr.INFINITIES))
def test_infinite_inputs_give_what_the_torch_formulas_give(name):
    case = _case('infinity', name)
    dev = _inputs(case, F64)
    got = _kernel(dev).cpu().numpy()
    print(name, dict(zip(rr.NAMES, got)))
    want_loss, want_dF = _torch_reference(case)
    loss = BoltzmannKLDivLoss()(dev['uB'], dev['ldj'], dev['lw'], dev['uA'])
    _check_scalar(f'{name} loss', loss, want_loss)
    _check_scalar(f'{name} dF', rr.finalize(got, weighted=True, biased=True, kT=KT)[1], want_dF)
    work = dev['uB'] - dev['ldj'] - dev['uA']
    _check_scalar(f'{name} fep_estimator', fep_estimator(torch.stack([work, dev['bias']], dim=1), kT=KT), want_dF)
    if name in ('lw_all_minus_inf', 'lw_plus_inf'):
        assert np.isnan(want_loss)
    if name.startswith('work_minus_inf'):
        assert want_dF == -np.inf
    ref, scales = _ref('infinity', name, F64)
    _check_stats(name, got, ref, scales)


def test_a_lone_infinite_log_weight_gives_nan():
    """softmax([+inf]) is NaN; so is the loss of a batch of one, and of one thread that holds two of them."""
    for n, at in ((1, [0]), (rr.CAP + 1, [0, rr.CAP])):
        lw = torch.zeros(n, dtype=F64, device='cuda')
        lw[at] = float('inf')
        loss = BoltzmannKLDivLoss()(torch.ones(n, dtype=F64, device='cuda'), None, lw)
        print(n, float(loss))
        assert torch.isnan(loss)


def test_bootstrap_resample_with_two_infinite_work_values():
    gen = torch.Generator().manual_seed(3)
    work = torch.randn(1000, generator=gen) * 3.0
    work[[10, 700]] = -float('inf')
    finite = [i for i in range(650) if i != 10]
    rows = [finite[:300] + [10, 700] + finite[300:598],         # both, in neighbouring lanes
            [10] + finite[:598] + [10],                          # the same one twice, in different waves
            [700] + finite[:255] + [700] + finite[255:598],      # twice in the stride of thread 0
            finite[:600]]                                        # none
    idx = torch.tensor(rows)
    assert idx.shape == (4, 600)
    kT = float(np.float32(KT))                                   # the C ABI of the bootstrap takes kT as a float
    got = bootstrap_fep(work.cuda(), indices=idx.cuda(), kT=kT).cpu()
    want = -kT * (torch.logsumexp(-work.double()[idx] / kT, dim=1) - np.log(idx.shape[1]))
    print(got.tolist(), want.tolist())
    assert got[:3].tolist() == [-np.inf] * 3 == want[:3].tolist()
    assert abs(float(got[3]) - float(want[3])) <= 1e-9 * max(1.0, abs(float(want[3])))
    data = torch.stack([work, torch.randn(1000, generator=gen)], dim=1)
    got = bootstrap_fep(data.cuda(), indices=idx.cuda(), kT=kT).cpu()
    assert got[:3].tolist() == [-np.inf] * 3 and np.isfinite(float(got[3]))


def test_combine_stats_of_kernel_shards_that_share_an_infinite_maximum():
    case = _case('infinity', 'work_minus_inf_twice_two_blocks')
    cut = 500                                                 # between the two infinite work values
    assert rr.INF_I < cut <= rr.INF_BLOCK
    shards = [_kernel(_inputs({k: v[a:b] for k, v in case.items()}, F64)) for a, b in ((0, cut), (cut, rr.N_INF))]
    assert float(shards[0][5]) == np.inf and float(shards[1][5]) == np.inf
    got = combine_stats(shards).cpu().numpy()
    print(dict(zip(rr.NAMES, got)))
    assert got[5] == np.inf and got[6] == 2.0
    assert rr.finalize(got, weighted=True, biased=True, kT=KT)[1] == -np.inf
    ref, scales = _ref('infinity', 'work_minus_inf_twice_two_blocks', F64)
    _check_stats('combined', got, ref, scales)


# ------------------------------------------------------------------ (f) the estimator in float64

@pytest.fixture(scope='module')
def work_case():
    """4096 work values ~ N(800, 3), a bias, three more rows and Bayesian weights; float64 on the CPU."""
    gen = torch.Generator().manual_seed(11)
    work = 800.0 + 3.0 * torch.randn(4, 4096, dtype=F64, generator=gen)
    bias = torch.randn(4, 4096, dtype=F64, generator=gen)
    weights = torch.distributions.Dirichlet(torch.ones(4096, dtype=F64)).sample((4,))
    return work, bias, weights


def _fep_formula(work, bias=None, weights=None, kT=KT):
    if bias is not None:
        log_weights = torch.log_softmax(bias / kT, dim=-1)
    elif weights is not None:
        log_weights = torch.log(weights)
    else:
        log_weights = -torch.log(torch.tensor(float(work.shape[-1]), dtype=F64))
    return -kT * torch.logsumexp(-work / kT + log_weights, dim=-1)


def test_fep_estimator_keeps_float64_work_in_float64(work_case):
    work, bias, weights = work_case
    w, b, wt = work.cuda(), bias.cuda(), weights.cuda()
    biased = torch.stack([w, b], dim=-1)
    runs = (('plain', fep_estimator(w[0], kT=KT), _fep_formula(work[0])),
            ('biased', fep_estimator(biased[0], kT=KT), _fep_formula(work[0], bias[0])),
            ('vectorized', fep_estimator(w, kT=KT, vectorized=True), _fep_formula(work)),
            ('vectorized biased', fep_estimator(biased, kT=KT, vectorized=True), _fep_formula(work, bias)),
            ('bayesian', fep_estimator(w[0], kT=KT, weights=wt[0]), _fep_formula(work[0], weights=weights[0])),
            ('vectorized bayesian', fep_estimator(w, kT=KT, weights=wt, vectorized=True), _fep_formula(work, weights=weights)))
    for what, got, want in runs:
        assert got.dtype == F64 and got.shape == want.shape and got.is_cuda, what
        for g, r in zip(got.reshape(-1).tolist(), want.reshape(-1).tolist()):
            _check_scalar(what, g, r)


def test_fep_estimator_on_float32_work_is_bit_for_bit_the_float32_reduction(work_case):
    work, bias, weights = work_case
    w, b, wt = work[0].float().cuda(), bias[0].float().cuda(), weights[0].float().cuda()

    def by_hand(extra, biased=False, bayesian=False):
        s = reduce_stats(w, None, None, None, extra, kT=KT)
        lse = s[5] + torch.log(s[6])
        if biased:
            lse = lse - (s[7] + torch.log(s[8]))
        elif not bayesian:
            lse = lse - torch.log(s[0])
        return (-KT * lse).to(F32)

    for what, got, want in (('plain', fep_estimator(w, kT=KT), by_hand(None)),
                            ('biased', fep_estimator(torch.stack([w, b], dim=1), kT=KT), by_hand(b, biased=True)),
                            ('bayesian', fep_estimator(w, kT=KT, weights=wt), by_hand(torch.log(wt) * KT, bayesian=True))):
        print(what, float(got), float(want))
        assert got.dtype == F32 and torch.equal(got, want), what
    # float64 work and its float32 rounding differ by far more than the float64 bound: the two paths are told apart
    assert abs(float(fep_estimator(w, kT=KT)) - float(_fep_formula(work[0]))) > 100 * rr.REL * 800


# ------------------------------------------------------------------ (g) gradients

@DTYPES
@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
def test_loss_gradients_past_one_grid_pass(weighted, dtype):
    """Against CPU float64 autograd of the reference's formula on the residuals as the dtype forms them (the gradient of
    uB is that of r, those of ldj and uA its negative).  Two samples are NaN and ignored.  The reference's own autograd
    gives NaN for every log-weight there (0 * NaN in the backward of ``weights * r``); the module documents zero weight
    for ignored samples, so the log-weight gradient is compared with ``nansum(w * r)`` written as ``sum(w * where(nan,
    0, r))``, the same function."""
    N = rr.CAP + 1
    case = rr.with_values(_case('size', N), uB={9: np.nan, rr.CAP: np.nan})
    dev = {k: v.requires_grad_(True) if k != 'bias' else v for k, v in _inputs(case, dtype).items()}
    loss = BoltzmannKLDivLoss(ignore_nan=True)(dev['uB'], dev['ldj'], dev['lw'] if weighted else None, dev['uA'])
    names = ('uB', 'ldj', 'lw', 'uA') if weighted else ('uB', 'ldj', 'uA')
    got = dict(zip(names, torch.autograd.grad(loss, [dev[k] for k in names])))

    r = torch.from_numpy(rr.lse_arguments(**case, kT=KT, dtype=NP[dtype])[0]).requires_grad_(True)
    if weighted:
        lw = torch.from_numpy(case['lw'].astype(NP[dtype]).astype(np.float64)).requires_grad_(True)
        want_loss = torch.sum(torch.softmax(lw, dim=0) * torch.where(torch.isnan(r), torch.zeros_like(r), r))
        g_r, g_lw = torch.autograd.grad(want_loss, [r, lw])
        literal = torch.autograd.grad(torch.nansum(torch.softmax(lw, dim=0) * r), lw)[0]
        assert torch.isnan(literal).all()
        want = dict(uB=g_r, ldj=-g_r, uA=-g_r, lw=g_lw)
    else:
        want_loss = torch.nanmean(r)
        (g_r,) = torch.autograd.grad(want_loss, r)
        want = dict(uB=g_r, ldj=-g_r, uA=-g_r)
    _check_scalar('loss', loss.detach(), want_loss.detach(), dtype)
    for k in names:
        g, w = got[k].cpu().double(), want[k]
        assert got[k].dtype == dtype and got[k].shape == (N,) and torch.isfinite(g).all(), k
        assert (g[[9, rr.CAP]] == 0).all() or k == 'lw'
        bound = rr.REL * w.abs().max() + (2.0 ** -24 * w.abs() if dtype == F32 else 0.0)
        ratio = float(((g - w).abs() / bound).max())
        print(f'{k}: max |ref| {float(w.abs().max()):.3e}, largest |got - ref| / bound {ratio:.2e}')
        assert ratio <= 1.0, (k, ratio)


# ------------------------------------------------------------------ (h) bits and layout

@DTYPES
def test_bits_do_not_depend_on_the_call_or_the_layout(dtype):
    case = _case('size', rr.N_WIDE)
    dev = _inputs(case, dtype)
    first, again = _kernel(dev), _kernel(dev)
    assert np.array_equal(first.cpu().numpy(), again.cpu().numpy())
    strided = {}
    for k, v in dev.items():
        buf = torch.full((2 * len(v),), 7.0, device='cuda', dtype=dtype)
        buf[::2] = v
        strided[k] = buf[::2]
        assert strided[k].stride(0) == 2 and not strided[k].is_contiguous()
    assert np.array_equal(first.cpu().numpy(), _kernel(strided).cpu().numpy())


@DTYPES
def test_combine_stats_of_three_ragged_kernel_shards(dtype):
    case = _case('size', rr.N_WIDE)
    cuts = (0, 1, rr.CAP + 77, rr.N_WIDE)                     # one element, more than one grid pass, the rest
    shards = [_kernel(_inputs({k: v[a:b] for k, v in case.items()}, dtype)) for a, b in zip(cuts, cuts[1:])]
    got = combine_stats(shards).cpu().numpy()
    ref, scales = _ref('size', rr.N_WIDE, dtype)
    _check_stats(f'3 shards {NP[dtype].__name__}', got, ref, scales)
