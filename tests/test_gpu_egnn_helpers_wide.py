"""The stand-alone helpers of csrc/egnn.hip past one grid pass.  ``axpy_kernel``, ``radial_kernel``, ``segment_sum_kernel``
and ``fill_kernel`` launch at most 65536 blocks of 256 threads and loop beyond 2^24 elements; every other test stays
below that (the largest, the state of the full-size continuous flow, has 1.26e7).  Here each of them takes a second trip
with a short tail, against float64 / int64 numpy, the elements of the second trip also compared on their own.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PASS = 65536 * 256            # threads of one grid pass: 2^24
U = 2.0 ** -24                # unit round-off of float32


def _report(what, err, bound, tail):
    """Print, then assert, ``err <= bound`` over everything and over the elements past one grid pass."""
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)           # (0 / 0: an exact zero copied exactly)
    print(f'{what}: max error / bound {ratio.max():.3f} over {err.size} elements, {ratio[tail:].max():.3f} over the last '
          f'{err.size - tail}; max error {err.max():.2e}')
    assert np.isfinite(err).all()
    assert np.all(err[tail:] <= bound[tail:])
    assert np.all(err <= bound)


@pytest.fixture(scope='module')
def axpy_data():
    n = PASS + 4099
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(n, generator=gen)
    base = torch.randn(n + 5, generator=gen)                 # the five terms: windows of one array, one element apart
    return n, x, base


@pytest.mark.parametrize('k', [0, 1, 4, 5])
def test_axpy_past_one_grid_pass(axpy_data, k):
    """``x + sum_k a_k v_k`` with 0, 1, 4 and 5 terms (five: two launches).  Per element the float32 result is within
    ``(k + 2) 2^-24 (|x| + sum |a_k v_k|)`` of the float64 one: k additions, each rounding a partial sum no larger than that
    sum of magnitudes, one unit for the roundings of the products together and one for the coefficients rounded to float32
    on their way into the kernel."""
    from tfep_amd.nn.flows.continuous import _axpy_kernel
    n, x, base = axpy_data
    coef = [1.0 / 3.0, -0.375, 0.7, -1.1, 0.05][:k]
    xd, bd = x.cuda(), base.cuda()
    terms = [(a, bd[i:i + n]) for i, a in enumerate(coef)]
    y = _axpy_kernel(xd, terms)
    assert y.shape == xd.shape and y.dtype == torch.float32 and y.data_ptr() != xd.data_ptr()
    assert torch.equal(xd.cpu(), x)                                                    # the input is left alone
    ref = x.numpy().astype(np.float64)
    mag = np.abs(ref)
    for i, a in enumerate(coef):
        t = a * base.numpy()[i:i + n].astype(np.float64)
        ref = ref + t
        mag = mag + np.abs(t)
    got = y.cpu().numpy().astype(np.float64)
    _report(f'axpy, {k} terms', np.abs(got - ref), (k + 2) * U * mag, PASS)
    if k == 0:
        assert torch.equal(y.cpu(), x)


RC = 2.0
N_R = 2 ** 18 + 37
N_BASIS = 64


def _expansions():
    from tfep_amd.nn.embeddings import BehlerParrinelloRadialExpansion, GaussianBasisExpansion
    gb = GaussianBasisExpansion.from_range(n_gaussians=N_BASIS, max_mean=RC, trainable_stds=True)
    bp = BehlerParrinelloRadialExpansion.from_range(r_cutoff=RC, n_gaussians=N_BASIS, max_mean=RC, trainable_stds=True)
    means, stds = GaussianBasisExpansion._get_equidistant_means_and_stds(N_BASIS, RC, 0.0, 3.0)
    bp_nz = BehlerParrinelloRadialExpansion(r_cutoff=RC, means=means, stds=stds, force_zero_after_cutoff=False)
    return dict(gauss=(gb, None, 1e-7), bp=(bp, True, 1e-7), bp_nozero=(bp_nz, False, 2e-7))


@pytest.fixture(scope='module')
def distances():
    r = torch.rand(N_R, generator=torch.Generator().manual_seed(22)) * (1.5 * RC)
    edge = torch.tensor(RC)
    r[:5] = torch.stack([torch.tensor(0.0), edge, torch.nextafter(edge, torch.tensor(4.0)),
                         torch.nextafter(edge, torch.tensor(0.0)), torch.tensor(1.5 * RC)])
    r[-1] = edge                                                # the cutoff itself also in the second trip
    return r


@pytest.mark.parametrize('which', ['gauss', 'bp', 'bp_nozero'])
def test_radial_expansions_past_one_grid_pass(distances, which):
    """2^18 + 37 distances on [0, 1.5 r_cutoff] x 64 functions = 2^24 + 2368 outputs, against float64 numpy on the float32
    distances, means and log-gammas; the bounds of ``test_radial_and_segment_sum_helpers``."""
    module, force_zero, atol = _expansions()[which]
    assert N_R * N_BASIS == PASS + 2368
    r = distances
    out = module.cuda()(r.cuda())
    assert out.shape == (N_R, N_BASIS) and out.dtype == torch.float32
    r64 = r.numpy().astype(np.float64)[:, None]
    mu = module._means.detach().cpu().numpy().astype(np.float64)
    gamma = np.exp(module._log_gammas.detach().cpu().numpy().astype(np.float64))
    ref = np.exp(-gamma * (r64 - mu) ** 2)
    if force_zero is not None:
        sw = 0.5 * np.cos(np.pi / RC * r64) + 0.5
        if force_zero:
            sw = np.where(r64 > RC, 0.0, sw)
        ref = ref * sw
    got = out.cpu().numpy().astype(np.float64).reshape(-1)
    ref = ref.reshape(-1)
    _report(f'radial expansion {which}', np.abs(got - ref), atol + 2e-6 * np.abs(ref), PASS)
    if force_zero:
        beyond = (r64 > RC)[:, 0]
        assert beyond[2] and not beyond[1] and not beyond[-1] and beyond[PASS // N_BASIS:].any()
        assert np.all(got.reshape(N_R, N_BASIS)[beyond] == 0.0)                       # exactly zero past the cutoff
    assert np.abs(ref[PASS:]).max() > 0.1                                             # the second trip is not all tails


def _segment_sum_ref(data, ids, n_segments):
    out = np.zeros((n_segments, data.shape[1]), dtype=np.int64)
    np.add.at(out, ids.numpy(), data.numpy().astype(np.int64))
    return out


def _dirty(shape):
    """Leave a freed block of this shape full of sevens for the allocator to hand to the next ``torch.empty``."""
    t = torch.full(shape, 7.0, device='cuda')
    torch.cuda.synchronize()
    del t


def test_segment_sum_past_one_grid_pass():
    """2^20 + 5 rows x 16 columns (2^24 + 80 elements) into 4099 segments.  The data are integers in [-8, 8]: every partial
    sum is an integer below 2^24, exact in float32 whatever order the atomics take, so the result equals the int64 sum
    bit for bit.  Called twice, the second time into a block that held the first result."""
    from tfep_amd.nn import graph
    n_rows, n_cols, n_seg = 2 ** 20 + 5, 16, 4099
    assert n_rows * n_cols > PASS
    gen = torch.Generator().manual_seed(23)
    data = torch.randint(-8, 9, (n_rows, n_cols), generator=gen).float()
    ids = torch.randint(0, n_seg, (n_rows,), generator=gen)
    ids[-5:] = torch.tensor([0, n_seg - 1, 17, n_seg - 1, 0])           # the rows of the second trip land where they show
    ref = _segment_sum_ref(data, ids, n_seg)
    assert np.abs(ref).max() < 2 ** 24 and np.bincount(ids.numpy(), minlength=n_seg).min() > 0
    tail = _segment_sum_ref(data[PASS // n_cols:], ids[PASS // n_cols:], n_seg)
    assert np.abs(tail).sum() > 0                                       # dropping the second trip would change the result
    d, i = data.cuda(), ids.cuda()
    ref_t = torch.from_numpy(ref).float()
    for trip in range(2):
        _dirty((n_seg, n_cols))
        out = graph.unsorted_segment_sum(d, i, n_seg)
        assert out.shape == (n_seg, n_cols) and out.dtype == torch.float32
        wrong = int((out.cpu() != ref_t).sum())
        print(f'segment sum, call {trip + 1}: {wrong} of {ref_t.numel()} sums differ from the int64 sum')
        assert torch.equal(out.cpu(), ref_t)
        del out


def test_segment_sum_zeroes_an_output_past_one_grid_pass():
    """2^20 + 3 segments x 17 columns: the output alone is more than one grid pass, so the zeroing loops; few rows, the
    last segment among them."""
    from tfep_amd.nn import graph
    n_seg, n_cols, n_rows = 2 ** 20 + 3, 17, 1001
    assert n_seg * n_cols > PASS
    gen = torch.Generator().manual_seed(24)
    data = torch.randint(-8, 9, (n_rows, n_cols), generator=gen).float()
    ids = torch.randint(0, n_seg, (n_rows,), generator=gen)
    ids[:4] = torch.tensor([n_seg - 1, 0, n_seg - 1, PASS // n_cols])
    ref_t = torch.from_numpy(_segment_sum_ref(data, ids, n_seg)).float()
    d, i = data.cuda(), ids.cuda()
    for trip in range(2):
        _dirty((n_seg, n_cols))
        out = graph.unsorted_segment_sum(d, i, n_seg).cpu()
        flat, want = out.reshape(-1), ref_t.reshape(-1)
        print(f'segment sum into {n_seg} x {n_cols}, call {trip + 1}: {int((flat != want).sum())} elements differ, '
              f'{int((flat[PASS:] != want[PASS:]).sum())} of them past one grid pass')
        assert torch.equal(flat[PASS:], want[PASS:])
        assert torch.equal(out, ref_t)
        del out
