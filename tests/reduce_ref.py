"""Plain float64 restatement of the 9 sufficient statistics of csrc/reduce.hip (numpy only), the cases the reduction
tests run and the bounds they hold the kernels to.

The statistics (tfep_hip.h): ``count, sum_r, m_w, s_w, s_wr, m_e, s_e, m_b, s_b`` with ``r = u_B - ldj - u_A`` formed in
the arithmetic of the inputs, ``(m, s)`` pairs ``m = max v``, ``s = sum exp(v - m)`` over the log-weights ``lw``, the
estimator arguments ``-r / kT + bias / kT`` and ``bias / kT``, and ``s_wr = sum exp(lw - m_w) r``.

Bounds (``ratios``).  A sum of N terms through about 30 levels of the kernels' tree errs by at most 30 eps of the sum of
the magnitudes; each term carries an ``exp`` good to a few ulp.  So every sum is held to ``1e-12`` of the sum of the
magnitudes of its terms (the project's float64 tolerance), ``count`` and ``m_w`` are exact, and ``m_e`` / ``m_b``, which
the compiler may contract into a fused multiply-add, are within 4 ulp.
"""
import functools

import numpy as np

NAMES = ('count', 'sum_r', 'm_w', 's_w', 's_wr', 'm_e', 's_e', 'm_b', 's_b')
INPUTS = ('uB', 'ldj', 'uA', 'lw', 'bias')
KT = 0.7
REL = 1e-12            # bound on every sum, relative to the sum of the magnitudes of its terms
MAX_ULP = 4            # bound on m_e and m_b
TERM = 1e-6            # a term of a log-sum-exp counts when exp(v - m) >= TERM
MIN_TERMS = 100        # terms that count in each log-sum-exp of a case with at least CONDITIONED_FROM elements
CONDITIONED_FROM = 1025
CAP = 262144           # elements of one pass of the partial kernel's grid: 1024 blocks of 256 threads

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1025, CAP - 1, CAP, CAP + 1, 600001)
N_WIDE = 600001
SEED = 20250


def _wide(a, dtype):
    return None if a is None else np.asarray(a).astype(dtype).astype(np.float64)


def lse_arguments(uB, ldj=None, uA=None, lw=None, bias=None, kT=1.0, dtype=np.float64):
    """``(r, lw, -r / kT + bias / kT, bias / kT)`` in float64 as the kernel forms them from inputs of ``dtype``; an absent
    input gives None."""
    r = np.asarray(uB).astype(dtype)
    if ldj is not None:
        r = r - np.asarray(ldj).astype(dtype)
    if uA is not None:
        r = r - np.asarray(uA).astype(dtype)
    assert r.dtype == dtype
    r = r.astype(np.float64)
    kT = float(np.float32(kT)) if dtype == np.float32 else float(kT)      # the float32 entry takes kT as a float
    inv_kT = 1.0 / kT
    with np.errstate(invalid='ignore'):
        e = -r * inv_kT
        b = None
        if bias is not None:
            b = _wide(bias, dtype) * inv_kT
            e = e + b
    return r, _wide(lw, dtype), e, b


def _pair(v, acc, softmax=False):
    """``(m, t)``: the maximum and the terms ``exp(v - m)``.  Equal infinite maxima count one each, as in
    ``torch.logsumexp``; for the weights (``softmax``) a ``+inf`` maximum makes every term NaN, as in ``torch.softmax``."""
    if v is None or v.size == 0:
        return -np.inf, np.zeros(0, dtype=acc)
    m = float(np.max(v))
    if np.isnan(m) or (softmax and m == np.inf):
        return m, np.full(v.shape, np.nan, dtype=acc)
    if m == -np.inf:
        return m, np.zeros(v.shape, dtype=acc)
    with np.errstate(invalid='ignore', under='ignore'):
        t = np.exp((v - m).astype(acc))
    return m, np.where(v == m, acc(1.0), t)


def _sum(x, acc):
    """The terms added one after the other into one accumulator of type ``acc``."""
    return np.cumsum(x, dtype=acc)[-1] if x.size else acc(0.0)


def stats_ref(uB, ldj=None, uA=None, lw=None, bias=None, kT=1.0, ignore_nan=False, dtype=np.float64, acc=np.longdouble):
    """``(stats, scales)``: the 9 statistics as float64 and the sums the bounds are scaled by, ``sum |r|`` and
    ``sum exp(lw - m_w) |r|``.  Sums are taken in ``acc``."""
    r, w, e, b = lse_arguments(uB, ldj, uA, lw, bias, kT, dtype)
    nan = np.isnan(r)
    keep = ~nan if ignore_nan else np.ones(r.shape, dtype=bool)
    rk = r[keep].astype(acc)
    with np.errstate(invalid='ignore', over='ignore'):
        count, sum_r, sum_abs_r = float(keep.sum()), _sum(rk, acc), _sum(np.abs(rk), acc)
        m_w, t = _pair(w, acc, softmax=True)
        s_w = _sum(t, acc)
        s_wr = _sum(t[keep] * rk, acc) if w is not None else acc(0.0)
        sum_w_abs_r = _sum(t[keep] * np.abs(rk), acc) if w is not None else acc(0.0)
        if nan.any():                                  # the log-sum-exp of the estimator is NaN, whatever ignore_nan says
            m_e, s_e = np.nan, np.nan
        else:
            m_e, t = _pair(e, acc)
            s_e = _sum(t, acc)
        m_b, t = _pair(b, acc)
        s_b = _sum(t, acc)
    stats = np.array([count, sum_r, m_w, s_w, s_wr, m_e, s_e, m_b, s_b], dtype=np.float64)
    return stats, dict(sum_abs_r=float(sum_abs_r), sum_w_abs_r=float(sum_w_abs_r))


def finalize(stats, weighted=False, biased=False, bayesian=False, kT=1.0):
    """``(loss, dF)`` as tfep_amd/loss.py and tfep_amd/analysis/estimator.py finish the statistics."""
    s = np.asarray(stats, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        loss = s[4] / s[3] if weighted else s[1] / s[0]
        lse = s[5] + np.log(s[6])
        if biased:
            lse = lse - (s[7] + np.log(s[8]))
        elif not bayesian:
            lse = lse - np.log(s[0])
        return float(loss), float(-kT * lse)


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def _ratio(got, ref, bound):
    if not (np.isfinite(ref) and np.isfinite(got)) or bound == 0.0:
        return 0.0 if _same(got, ref) else np.inf
    return abs(got - ref) / bound


def ratios(got, ref, scales):
    """name -> ``|got - ref|`` over its bound; a value that has to be exact gives 0 or inf."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    g, r = dict(zip(NAMES, got)), dict(zip(NAMES, ref))
    out = {'count': 0.0 if _same(g['count'], r['count']) else np.inf,
           'm_w': 0.0 if _same(g['m_w'], r['m_w']) else np.inf,
           'sum_r': _ratio(g['sum_r'], r['sum_r'], REL * scales['sum_abs_r']),
           's_wr': _ratio(g['s_wr'], r['s_wr'], REL * scales['sum_w_abs_r'])}
    for k in ('s_w', 's_e', 's_b'):
        out[k] = _ratio(g[k], r[k], REL * abs(r[k]))
    for k in ('m_e', 'm_b'):
        out[k] = _ratio(g[k], r[k], MAX_ULP * np.spacing(abs(r[k])) if np.isfinite(r[k]) else 0.0)
    return {k: float(out[k]) for k in NAMES}


def scalar_ratio(got, ref):
    """``|got - ref|`` over ``1e-12 max(1, |ref|)``: the bound on a loss or a dF finished from float64 statistics."""
    return _ratio(float(got), float(ref), REL * max(1.0, abs(float(ref))))


# ------------------------------------------------------------------ cases

@functools.lru_cache(maxsize=None)
def wide_case(N, spread, peak=None, seed=SEED, order=None, absent=()):
    """float64 inputs whose three log-sum-exp arguments -- ``lw``, ``-r / kT + bias / kT`` and ``bias / kT`` at kT = KT --
    are each ``-spread / 2 + spread u`` with u uniform in [0, 1), the element at ``peak`` (default N // 3) raised to half a
    unit above the rest.  ``r = -KT (e - b)`` has both signs and reaches ``KT spread``; ``uA`` is uniform in +-300 and
    ``ldj`` in +-20, so ``uB`` is in the hundreds whatever the spread.  ``order`` sorts the three arguments ('ascending',
    'descending') before the inputs are formed from them.  The inputs named in ``absent`` are None and ``uB`` is formed
    from the others, so the arguments keep their form.  The arrays are shared: do not write to them."""
    rng = np.random.default_rng(seed + 7 * N + int(spread))
    peak = N // 3 if peak is None else peak

    def argument():
        a = -spread / 2 + spread * rng.random(N)
        if N:
            a[peak] = a.max() + 0.5
        if order is not None:
            a.sort()
            if order == 'descending':
                a = a[::-1].copy()
        return a
    a_w, a_e, a_b = argument(), argument(), argument()
    ldj, uA = rng.uniform(-20.0, 20.0, N), rng.uniform(-300.0, 300.0, N)
    uB = -KT * (a_e if 'bias' in absent else a_e - a_b)
    for name, v in (('ldj', ldj), ('uA', uA)):
        if name not in absent:
            uB = uB + v
    case = dict(uB=uB, ldj=ldj, uA=uA, lw=a_w, bias=KT * a_b)
    for v in case.values():
        v.setflags(write=False)
    return {k: (None if k in absent else v) for k, v in case.items()}


#: (b) the optional inputs that are absent in turn
ABSENT = (('ldj',), ('uA',), ('lw',), ('bias',), ('ldj', 'uA', 'lw', 'bias'))
#: (c) where the maximum sits and how the arguments are ordered, at N_WIDE and spread 4000
ARRANGEMENTS = {'peak_first': dict(peak=0), 'peak_last': dict(peak=N_WIDE - 1), 'peak_second_trip': dict(peak=CAP + 5),
                'ascending': dict(order='ascending'), 'descending': dict(order='descending')}
#: (d) one NaN per trip of the grid-stride loop
NAN_AT = (7, CAP + 300, 2 * CAP + 70001)
#: (e) N of the infinity cases, an element, its neighbour in the stride of the same thread and one of another block
N_INF, INF_I, INF_STRIDE, INF_BLOCK = CAP + 1, 0, CAP, 1000
INFINITIES = {
    'lw_some_minus_inf': dict(lw={5: -np.inf, 300: -np.inf, CAP: -np.inf}),
    'lw_all_minus_inf': dict(lw={Ellipsis: -np.inf}),
    'lw_plus_inf': dict(lw={300: np.inf}),
    'work_plus_inf': dict(uB={5: np.inf, 300: np.inf}),
    'work_minus_inf_once': dict(uB={INF_BLOCK: -np.inf}),
    'work_minus_inf_twice_one_thread': dict(uB={INF_I: -np.inf, INF_STRIDE: -np.inf}),
    'work_minus_inf_twice_two_blocks': dict(uB={INF_I: -np.inf, INF_BLOCK: -np.inf}),
}


def with_values(case, **changes):
    """A copy of the case with ``changes[name] = {index: value}`` written into its inputs."""
    out = dict(case)
    for name, edits in changes.items():
        a = np.array(case[name])
        for i, v in edits.items():
            a[i] = v
        out[name] = a
    return out


def nan_case():
    """NaN in uB, one per trip.  The log-weights of the two later ones are one unit below the maximum: each is the largest
    its thread has seen, so an ignored sample moves the running maximum that ``s_wr`` is scaled by."""
    case = wide_case(N_WIDE, 60)
    top = case['lw'].max() - 1.0
    assert all(top > case['lw'][i % CAP::CAP][:i // CAP].max() for i in NAN_AT[1:])
    return with_values(case, uB={i: np.nan for i in NAN_AT}, lw={i: top for i in NAN_AT[1:]})


def infinity_case(name):
    return with_values(wide_case(N_INF, 60), **INFINITIES[name])


def conditioning(case, kT=KT, dtype=np.float64):
    """Per log-sum-exp ('w', 'e', 'b') of the inputs present: the number of terms ``exp(v - m) >= TERM`` and the largest
    term's share of ``s``."""
    _, w, e, b = lse_arguments(**case, kT=kT, dtype=dtype)
    out = {}
    for k, v in (('w', w), ('e', e), ('b', b)):
        if v is not None and v.size:
            _, t = _pair(v, np.longdouble)
            out[k] = (int((t >= TERM).sum()), float(t.max() / t.sum()))
    return out


def assert_conditioned(case, spread, dtype=np.float64):
    """What the bounds rest on, for a case of at least CONDITIONED_FROM elements: MIN_TERMS terms that count in every
    log-sum-exp, no term above half of ``s`` at spread 60, and ``sum |r| > 0``.  Returns what it measured."""
    cond = conditioning(case, dtype=dtype)
    _, scales = stats_ref(**case, kT=KT, dtype=dtype)
    for k, (n_terms, share) in cond.items():
        assert n_terms >= MIN_TERMS, (k, n_terms)
        assert spread != 60 or share <= 0.5, (k, share)
    assert scales['sum_abs_r'] > 0.0
    return cond
