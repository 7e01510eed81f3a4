"""The resampling stream of the bootstrap kernels restated with numpy from its definition: Philox4x32-10
words, the multiply-high indices, the uniforms and the Dirichlet(1, ..., 1) weights.  Test infrastructure: the yardstick of
tests/test_bootstrap_resampled_host.py and tests/test_gpu_bootstrap_resampled.py, written without looking at the kernel."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAM_INDICES, STREAM_WEIGHTS = 0, 1


def philox4x32_10(counter, key):
    """Ten rounds on arrays: ``counter`` is four and ``key`` two uint64 arrays (or ints) of 32-bit values that broadcast
    together; returns the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k = [np.asarray(x, dtype=np.uint64) for x in key]
    m0, m1, mask, s32 = np.uint64(M0), np.uint64(M1), np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                              # 32 x 32 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & mask, (p0 >> s32) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return c


def words(seed, r, n_groups, stream):
    """The ``(n_groups, 4)`` words of resample ``r``: group q has the counter (q & 0xffffffff, q >> 32, r, stream) under the key
    (seed & 0xffffffff, seed >> 32)."""
    assert 0 <= seed < 2 ** 63 and 0 <= r < 2 ** 31
    q = np.arange(n_groups, dtype=np.uint64)
    out = philox4x32_10((q & np.uint64(MASK), q >> np.uint64(32), r, stream), (seed & MASK, seed >> 32))
    return np.stack([np.broadcast_to(w, q.shape) for w in out], axis=1)


def indices(n_resamples, sample_size, high, seed, offset=0):
    """``(n_resamples, sample_size)`` int64: draw j of row k is word j % 4 of group j // 4 of resample offset + k, mapped to
    ``(word * high) >> 32``."""
    assert 1 <= high < 2 ** 31
    rows = []
    for k in range(n_resamples):
        w = words(seed, offset + k, -(-sample_size // 4), STREAM_INDICES).reshape(-1)[:sample_size]
        rows.append(((w * np.uint64(high)) >> np.uint64(32)).astype(np.int64))
    return np.stack(rows) if rows else np.empty((0, sample_size), dtype=np.int64)


def uniforms(n_resamples, sample_size, seed, offset=0):
    """``(n_resamples, sample_size)`` float64: draw j takes the word pair (a, b) = (2 (j % 2), 2 (j % 2) + 1) of group j // 2,
    u = (((a >> 5) * 2^26 + (b >> 6)) + 0.5) * 2^-53."""
    rows = []
    for k in range(n_resamples):
        w = words(seed, offset + k, -(-sample_size // 2), STREAM_WEIGHTS).reshape(-1, 2)[:sample_size]
        bits = (w[:, 0] >> np.uint64(5)) * np.uint64(2 ** 26) + (w[:, 1] >> np.uint64(6))
        rows.append((bits.astype(np.float64) + 0.5) * 2.0 ** -53)
    return np.stack(rows) if rows else np.empty((0, sample_size))


def weights(n_resamples, sample_size, seed, offset=0):
    """``(n_resamples, sample_size)`` float64 rows E_j / sum_j E_j with E_j = -log(u_j)."""
    e = -np.log(uniforms(n_resamples, sample_size, seed, offset))
    return e / e.sum(axis=1, keepdims=True)
