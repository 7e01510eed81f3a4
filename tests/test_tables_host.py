"""CPU tests of tfep_amd/_tables.py, the host module that prepares the integer tables of the index, Z-matrix and edge-list
ops: it loads no library, its incidence builder against a brute-force loop, its cache class, and the Z-matrix path leaving
the cache of ``index_tables`` alone.  What the three families build with these pieces is checked in test_geometry_host.py,
test_zmatrix_host.py and test_edge_ops_host.py.  No kernel is launched."""
import itertools
import os
import subprocess
import sys

import pytest
import torch

from tfep_amd import _tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_import_loads_neither_the_binding_nor_ops():
    code = ("import sys; import tfep_amd._tables as t; "
            "assert 'tfep_amd._lib' not in sys.modules and 'tfep_amd.ops' not in sys.modules, sorted(sys.modules); "
            "print(t.incidence.__name__)")
    done = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == 'incidence', done.stdout + done.stderr


@pytest.mark.parametrize('keys, n_bins', [
    ([2, 0, 2, 1, 0, 2, 2], 3),                  # ties: the items of a bin keep their order
    ([4, 1, 1, 4, 0], 6),                        # bins 2, 3 and 5 have no key
    ([], 3),                                     # no key at all
], ids=['ties', 'empty bins', 'no keys'])
def test_incidence_against_a_loop(keys, n_bins):
    start, order = _tables.incidence(torch.tensor(keys, dtype=torch.int64), n_bins)
    assert start.dtype == order.dtype == torch.int64 and start.shape == (n_bins + 1,) and order.shape == (len(keys),)
    assert start.device == order.device == torch.device('cpu')
    by_bin = [[i for i, k in enumerate(keys) if k == b] for b in range(n_bins)]
    assert [order[start[b]:start[b + 1]].tolist() for b in range(n_bins)] == by_bin
    assert int(start[0]) == 0 and int(start[-1]) == len(keys)


def test_integer_and_range_checks():
    for bad in (torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.complex64), torch.zeros(2, 3) > 0, [[0.5]]):
        with pytest.raises(ValueError, match='t must hold integer indices'):
            _tables.integer_table(bad, 't')
    got = _tables.integer_table(torch.tensor([[1, 2]], dtype=torch.int16, requires_grad=False), 't')
    assert got.dtype == torch.int64 and got.device.type == 'cpu' and got.tolist() == [[1, 2]]
    assert _tables.integer_table([[3], [4]], 't').tolist() == [[3], [4]]
    table = torch.tensor([[0, 5], [2, 3]])
    assert _tables.out_of_range(table, 6) is None and _tables.out_of_range(torch.empty(2, 0, dtype=torch.int64), 0) is None
    assert _tables.out_of_range(table, 5) == (0, 5) and _tables.out_of_range(table - 1, 6) == (-1, 4)
    _tables.check_range(table, 't', 6)
    with pytest.raises(ValueError, match=r't has an index outside \[0, 5\): min 0, max 5'):
        _tables.check_range(table, 't', 5)


def test_cache():
    cache = _tables.Cache(size=3)
    tensors = [torch.tensor([i, i + 1]) for i in range(5)]
    values = [object() for _ in tensors]
    key = lambda t: _tables.identity_key((t, None), 7, 'cpu')
    assert cache.get(key(tensors[0]), (tensors[0], None)) is None
    cache.put(key(tensors[0]), (tensors[0], None), values[0])
    assert cache.get(key(tensors[0]), (tensors[0], None)) is values[0]          # a hit: the identical object
    assert cache.get(key(tensors[0])) is values[0]                               # (the key alone, as the edge lists use it)
    assert cache.get(_tables.identity_key((tensors[0], None), 8, 'cpu'), (tensors[0], None)) is None
    assert cache.get(key(tensors[0].clone()), (tensors[0], None)) is None        # an equal tensor is another tensor
    old = key(tensors[0])
    tensors[0][1] = 9                                                            # an in-place write: a new version, a miss
    assert key(tensors[0]) != old and cache.get(key(tensors[0]), (tensors[0], None)) is None
    assert cache.get(old, (tensors[0], None)) is values[0]
    # entry size + 1 evicts the oldest entry only
    for t, v in zip(tensors[1:4], values[1:4]):
        cache.put(key(t), (t, None), v)
    assert cache.get(old, (tensors[0], None)) is None and len(cache.entries) == 3
    assert [cache.get(key(t), (t, None)) for t in tensors[1:4]] == values[1:4]
    # what has no key is not cached: a list, a tensor without a version counter
    assert _tables.identity_key(([0, 1], None), 7, 'cpu') is None
    with torch.inference_mode():
        frozen = torch.tensor([0, 1])
    assert key(frozen) is None
    cache.put(key(frozen), (frozen, None), values[4])
    assert cache.get(key(frozen), (frozen, None)) is None and len(cache.entries) == 3


def test_families_take_a_tensor_without_a_version_counter():
    with torch.inference_mode():
        pairs, z, fixed, edges = (torch.tensor(v) for v in ([[0, 1], [1, 2]], [[3, 0, 1, 2]], [0, 1, 2], [[0, 1], [1, 2]]))
    first = _tables.index_tables(pairs, None, None, 3, 'cpu')
    again = _tables.index_tables(pairs, None, None, 3, 'cpu')
    assert again is not first and all(torch.equal(a, b) for a, b in zip(first, again))
    assert _tables.zmatrix_tables(z, fixed, 4, 'cpu') is not _tables.zmatrix_tables(z, fixed, 4, 'cpu')
    assert _tables.check_edges(edges, 3) is not _tables.check_edges(edges, 3)
    assert _tables.edge_incidence(edges, 3)[1].tolist() == [0, 1, 2, 3]


def test_zmatrix_tables_leave_the_index_table_cache_alone():
    """Nine distinct Z-matrices, one more than the cache of ``index_tables`` holds, do not evict an entry of it: the Z-matrix
    path builds its ``internal_coordinates`` tables with the uncached builder and keeps them in its own cache.  (Before
    tfep_amd/_tables.py it went through the cached ``index_tables`` with three tensors it had just made, so every
    Z-matrix pushed an entry that could never be hit, and this test failed.)"""
    from tfep_amd import ops
    tables = (torch.tensor([[0, 1], [1, 2]]), torch.tensor([[0], [1], [2]]), torch.tensor([[0], [1], [2], [3]]))
    first = ops.index_tables(*tables, n_atoms=4, device='cpu')
    fixed = torch.tensor([0, 1, 2])
    orders = list(itertools.permutations(range(3)))
    z_matrices = [torch.tensor([[3, *orders[i % 6]], [4, 3, *orders[i // 6][:2]]]) for i in range(9)]
    assert len({tuple(z.reshape(-1).tolist()) for z in z_matrices}) == 9
    for z in z_matrices:
        index, fixed_back = ops.zmatrix_index_tables(z, fixed, 5, 'cpu')
        assert index[2].t().tolist() == z.tolist() and fixed_back.tolist() == [0, 1, 2]
        assert ops.zmatrix_tables(z, fixed, 5, 'cpu').rows.shape == (5, 2)
    assert ops.index_tables(*tables, n_atoms=4, device='cpu') is first
