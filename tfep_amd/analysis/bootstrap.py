"""Bootstrap analysis of a statistic (reference ``tfep/analysis/bootstrap.py:24-262``).

Same API and results as the reference.  When the statistic is :func:`tfep_amd.analysis.fep_estimator` the whole
bootstrap distribution is computed by one HIP kernel (``tfep_bootstrap_fep``: one workgroup per resample, the
resampled data are never materialised); any other statistic follows the reference's gather-and-call scheme with
torch ops on the data's device.

``bootstrap(..., resampler='kernel')`` also draws the resamples inside the kernel (``bootstrap_fep_resampled``): a
counter-based Philox stream, so that neither an index tensor nor a weight tensor is materialised, over a table of the
``n_samples`` exponentials that exist.  The default, ``resampler='torch'``, draws them with torch as the reference does.
"""
import functools

import torch

from .. import _lib
from .estimator import fep_estimator


def bootstrap(data, statistic, *, confidence_level=0.95, n_resamples=9999, bootstrap_sample_size=None,
              take_first_only=False, batch=None, method='percentile', bayesian=False, generator=None, resampler='torch'):
    """Parameters of the bootstrap distribution of ``statistic`` over ``data`` ``(n_samples,)`` or
    ``(n_samples, data_dimension)``: confidence interval, standard deviation, mean and median; a list of such
    dicts if ``bootstrap_sample_size`` is a list.  Arguments as reference bootstrap.py:24-121.

    ``generator`` may live on the CPU (the resample indices are then drawn exactly as the reference draws them and
    moved to the data's device) or on the device.

    ``resampler='kernel'`` (``statistic`` must be :func:`fep_estimator`, possibly a ``functools.partial`` fixing only
    ``kT``) draws the resamples in the kernel from the stream of :func:`bootstrap_fep_resampled`.  Its seed is an ``int``
    ``generator`` itself, or one ``torch.randint(0, 2**63 - 1, (1,))`` draw from a ``torch.Generator`` or, for ``None``,
    from the default generator of the data's device (``torch.manual_seed`` reproduces a run).  Resample ``k`` of the
    ``i``-th sample size is resample number ``i * n_resamples + k`` of the stream, so ``batch`` changes memory only, never
    a value.  The resamples are not those of ``resampler='torch'`` with the same generator.
    """
    if resampler not in ('torch', 'kernel'):
        raise ValueError("resampler must be 'torch' or 'kernel'")
    n_samples = len(data)
    if bayesian and generator is not None:
        raise ValueError('Bayesian bootstrapping does not support random number generators.')
    if bootstrap_sample_size is None:
        sizes = [n_samples]
    else:
        if bayesian and not take_first_only:
            raise ValueError('With Bayesian bootstrapping, specifying a bootstrap_sample_size '
                             'is supported only when take_first_only is True.')
        sizes = [bootstrap_sample_size] if isinstance(bootstrap_sample_size, int) else list(bootstrap_sample_size)
    single = len(sizes) == 1                  # also a one-element list (reference bootstrap.py: len(...) == 1)
    if method not in ('percentile', 'basic'):
        raise ValueError("method must be 'percentile' or 'basic'")
    kT = _fep_statistic_kT(statistic)
    if resampler == 'kernel':
        if kT is None:
            raise ValueError("resampler='kernel' computes fep_estimator only (or a functools.partial of it fixing kT)")
        seed = _kernel_seed(generator, data.device)
        _check_stream(seed, 0, len(sizes) * n_resamples)
        for sample_size in sizes:
            _check_resample(n_samples, sample_size, sample_size if take_first_only or bayesian else n_samples, bayesian)
    elif isinstance(generator, int):
        generator = torch.Generator(device=data.device).manual_seed(generator)
    if batch is None:
        batch = n_resamples

    results = []
    with torch.no_grad():
        for i_size, sample_size in enumerate(sizes):
            stats = torch.empty(n_resamples, dtype=torch.float64 if kT is not None else data.dtype, device=data.device)
            if resampler == 'kernel':
                high = sample_size if take_first_only or bayesian else n_samples
                table = _FepTable(data[:high], kT)
            for k in range(0, n_resamples, batch):
                nb = min(batch, n_resamples - k)
                if resampler == 'kernel':
                    stats[k:k + nb] = table.resample(nb, sample_size, seed, i_size * n_resamples + k, bayesian)
                elif bayesian:
                    weights = torch.distributions.Dirichlet(
                        torch.ones(sample_size, device=data.device)).sample((nb,))
                    sub = data[:sample_size]
                    if kT is not None:
                        stats[k:k + nb] = bootstrap_fep(sub, weights=weights, kT=kT)
                    else:
                        stats[k:k + nb] = statistic(sub.expand((nb, *sub.shape)), weights=weights, vectorized=True)
                else:
                    high = sample_size if take_first_only else n_samples
                    gen_device = generator.device if generator is not None else data.device
                    idx = torch.randint(low=0, high=high, size=(nb, sample_size), generator=generator,
                                        device=gen_device).to(data.device)
                    if kT is not None:
                        stats[k:k + nb] = bootstrap_fep(data, indices=idx, kT=kT)
                    else:
                        samples = data[idx]                       # (nb, sample_size[, data_dimension])
                        stats[k:k + nb] = statistic(samples, vectorized=True)
            stats = stats.to(data.dtype)
            alpha = (1 - confidence_level) / 2
            ci_l, ci_u = torch.quantile(stats, q=torch.tensor([alpha, 1 - alpha], dtype=stats.dtype, device=stats.device))
            if method == 'basic':
                # the reference calls statistic(data.unsqueeze(0)) (bootstrap.py:170), which its own fep_estimator
                # rejects; the estimator gets the vectorized call it needs, other statistics the reference's call
                full = (statistic(data.unsqueeze(0), vectorized=True) if kT is not None
                        else statistic(data.unsqueeze(0))).reshape(())
                ci_l, ci_u = 2 * full - ci_u, 2 * full - ci_l
            results.append(dict(confidence_interval=dict(low=ci_l, high=ci_u), standard_deviation=torch.std(stats),
                                mean=torch.mean(stats), median=torch.median(stats)))
    return results[0] if single else results


def _fep_statistic_kT(statistic):
    """kT if ``statistic`` is fep_estimator (possibly a functools.partial fixing only kT), else None."""
    if statistic is fep_estimator:
        return 1.0
    if isinstance(statistic, functools.partial) and statistic.func is fep_estimator and not statistic.args \
            and set(statistic.keywords) <= {'kT'}:
        return float(statistic.keywords.get('kT', 1.0))
    return None


def bootstrap_fep(data, indices=None, weights=None, kT=1.0):
    """``fep_estimator`` of every resample in one kernel: ``data`` is ``(n_samples,)`` work values or
    ``(n_samples, 2)`` with the bias in the second column; ``indices`` ``(n_resamples, sample_size)`` int64 picks the
    resamples (standard bootstrap), or ``weights`` ``(n_resamples, n_samples)`` are Bayesian-bootstrap weights.
    float64 ``data`` are read as they are (and the weights as float64); any other dtype is computed from float32 copies.
    Returns ``(n_resamples,)`` float64."""
    if (indices is None) == (weights is None):
        raise ValueError('exactly one of indices and weights must be given')
    work, bias, suffix = _work_and_bias(data)
    _lib.check_device_tensor(work, 'data', work.dtype)
    if indices is not None:
        indices = indices.to(device=work.device, dtype=torch.int64).contiguous()
        R, S = indices.shape
    else:
        if bias is not None:
            raise NotImplementedError('Bayesian bootstrapping is not supported with biased data.')
        weights = weights.to(device=work.device, dtype=work.dtype).contiguous()
        R, S = weights.shape
        if S != work.numel():
            raise ValueError('weights must have one column per sample')
    out = torch.empty(R, dtype=torch.float64, device=work.device)
    _lib.call('tfep_bootstrap_fep' + suffix, _lib.ptr(work), _lib.ptr(bias), _lib.ptr(indices), _lib.ptr(weights), work.numel(),
              R, S, float(kT), _lib.ptr(out), _lib.stream_of(work))
    return out


def _work_and_bias(data):
    """The contiguous work and bias columns of ``data`` and the suffix of their entry points: float64 data stay float64,
    every other dtype is cast to float32."""
    dtype = torch.float64 if data.dtype == torch.float64 else torch.float32
    if data.dim() == 2:
        work, bias = data[:, 0].contiguous().to(dtype), data[:, 1].contiguous().to(dtype)
    else:
        work, bias = data.contiguous().to(dtype), None
    return work, bias, '_f64' if dtype == torch.float64 else ''


def _kernel_seed(generator, device):
    """The seed of the kernel's stream from the ``generator`` argument of :func:`bootstrap`."""
    if isinstance(generator, int):
        return generator
    if generator is None:
        return int(torch.randint(0, 2 ** 63 - 1, (1,), device=device))
    return int(torch.randint(0, 2 ** 63 - 1, (1,), generator=generator, device=generator.device))


def _check_stream(seed, offset, n_resamples):
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 63:
        raise ValueError('seed must be an int in [0, 2**63)')
    if offset < 0 or n_resamples < 0 or offset + n_resamples > 2 ** 31:
        raise ValueError('offset and n_resamples must be >= 0 and offset + n_resamples <= 2**31')


def _check_resample(n_data, sample_size, high, bayesian):
    if not 1 <= high <= min(n_data, 2 ** 31 - 1):
        raise ValueError(f'high must be in [1, min(len(data), 2**31 - 1)], got {high} for {n_data} samples')
    if sample_size < 1:
        raise ValueError('sample_size must be >= 1')
    if bayesian and sample_size != high:
        raise ValueError('Bayesian bootstrapping needs sample_size == high')


class _FepTable:
    """The table ``exp(a_i - max a)`` of ``data`` (``tfep_bootstrap_table``), from which ``resample`` computes batches of
    resamples (``tfep_bootstrap_fep_resampled``)."""

    def __init__(self, data, kT):
        self.work, self.bias, self.suffix = _work_and_bias(data)
        _lib.check_device_tensor(self.work, 'data', self.work.dtype)
        self.kT, n, dev = float(kT), self.work.numel(), self.work.device
        self.table = torch.empty((1 if self.bias is None else 2) * n, dtype=torch.float64, device=dev)
        self.stats = torch.empty(2, dtype=torch.float64, device=dev)
        self.flag = torch.empty(1, dtype=torch.int32, device=dev)
        workspace = torch.empty(_lib.load().tfep_bootstrap_table_workspace_doubles(n), dtype=torch.float64, device=dev)
        _lib.call('tfep_bootstrap_table' + self.suffix, _lib.ptr(self.work), _lib.ptr(self.bias), n, self.kT,
                  _lib.ptr(self.table), _lib.ptr(self.stats), _lib.ptr(self.flag), _lib.ptr(workspace), _lib.stream_of(self.work))

    def resample(self, n_resamples, sample_size, seed, offset, bayesian):
        if bayesian and self.bias is not None:
            raise NotImplementedError('Bayesian bootstrapping is not supported with biased data.')
        out = torch.empty(n_resamples, dtype=torch.float64, device=self.work.device)
        n = self.work.numel()
        _lib.call('tfep_bootstrap_fep_resampled' + self.suffix, _lib.ptr(self.work), _lib.ptr(self.bias), _lib.ptr(self.table),
                  _lib.ptr(self.stats), _lib.ptr(self.flag), n, n_resamples, sample_size, n, seed, offset, int(bayesian), self.kT,
                  _lib.ptr(out), _lib.stream_of(self.work))
        return out


def bootstrap_fep_resampled(data, n_resamples, sample_size=None, *, seed, offset=0, high=None, bayesian=False, kT=1.0):
    """``fep_estimator`` of ``n_resamples`` resamples of ``data[:high]`` drawn inside the kernel: ``data`` as in
    :func:`bootstrap_fep` (float64 read as it is), ``high`` defaults to ``len(data)`` and ``sample_size`` to ``high``.
    Returns ``(n_resamples,)`` float64.

    The resamples come from a counter-based stream (Philox4x32-10 keyed by ``seed`` in ``[0, 2**63)``): row ``k`` is
    resample number ``offset + k`` (``offset + n_resamples <= 2**31``) and depends on ``(seed, offset + k)`` alone, so
    cutting ``n_resamples`` into batches with growing ``offset`` changes no value.  Draw ``j`` of the standard bootstrap is
    the index ``(word_j * high) >> 32`` of a 32-bit word: a multiply-high mapping with a bias of at most ``high / 2**32``,
    which is not the mapping of ``torch.randint``, so the resamples differ from torch's for any generator.  With
    ``bayesian=True`` (``sample_size == high``, no bias column) the weights are ``E_j / sum_j E_j``, ``E_j = -log(u_j)``:
    Dirichlet(1, ..., 1).  :func:`bootstrap_resample_indices` and :func:`bootstrap_resample_weights` return the same
    resamples, which :func:`bootstrap_fep` takes explicitly."""
    n_data = len(data)
    high = n_data if high is None else high
    sample_size = high if sample_size is None else sample_size
    _check_stream(seed, offset, n_resamples)
    _check_resample(n_data, sample_size, high, bayesian)
    if bayesian and data.dim() == 2:
        raise NotImplementedError('Bayesian bootstrapping is not supported with biased data.')
    return _FepTable(data[:high], kT).resample(n_resamples, sample_size, seed, offset, bayesian)


def bootstrap_resample_indices(n_resamples, sample_size, high, *, seed, offset=0, device):
    """The ``(n_resamples, sample_size)`` int64 indices in ``[0, high)`` that :func:`bootstrap_fep_resampled` draws for
    the same ``(seed, offset, high)``."""
    _check_stream(seed, offset, n_resamples)
    if not 1 <= high <= 2 ** 31 - 1:
        raise ValueError('high must be in [1, 2**31 - 1]')
    if sample_size < 1:
        raise ValueError('sample_size must be >= 1')
    out = torch.empty(n_resamples, sample_size, dtype=torch.int64, device=device)
    _lib.check_device_tensor(out, 'device', torch.int64)
    _lib.call('tfep_bootstrap_resample_indices', n_resamples, sample_size, high, seed, offset, _lib.ptr(out), _lib.stream_of(out))
    return out


def bootstrap_resample_weights(n_resamples, sample_size, *, seed, offset=0, device):
    """The ``(n_resamples, sample_size)`` float64 weights, each row summing to 1, that the Bayesian mode of
    :func:`bootstrap_fep_resampled` uses for the same ``(seed, offset)`` and ``sample_size`` samples."""
    _check_stream(seed, offset, n_resamples)
    if sample_size < 1:
        raise ValueError('sample_size must be >= 1')
    out = torch.empty(n_resamples, sample_size, dtype=torch.float64, device=device)
    _lib.check_device_tensor(out, 'device', torch.float64)
    _lib.call('tfep_bootstrap_resample_weights', n_resamples, sample_size, seed, offset, _lib.ptr(out), _lib.stream_of(out))
    return out
