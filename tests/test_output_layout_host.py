"""Host tests of the one definition of the degree-sorted output-row layout (``tfep_amd/_tables.py``: ``stable_order``,
``packed_rows``) against the formulas the fused plan, the backward plan and ``MADE.plan`` each spelled out before, written
out here literally."""
import numpy as np
import pytest
import torch

from tfep_amd import _tables
from tfep_amd.nn.flows import _blocked_f64 as bf

DEGREES = {
    'repeated': [2, 0, 1, 0, 2, 1, 1, 0, 2, 2],
    'single': [0],
    'descending': list(range(16, -1, -1)),                              # n = 17
    'round_robin_17': [i % 5 for i in range(17)],
    'round_robin_33': [(7 * i) % 4 for i in range(33)],
    'ascending_33': list(range(33)),
    'all_equal': [3] * 20,
}


def parent_order(deg):
    """``_fused_plan`` / ``_backward_plan`` / ``MADE.plan`` before the helper."""
    deg = torch.as_tensor(deg)
    order = torch.argsort(deg, stable=True)
    slot_of = torch.empty_like(order)
    slot_of[order] = torch.arange(len(deg), device='cpu')
    return order, slot_of


@pytest.mark.parametrize('name', sorted(DEGREES))
@pytest.mark.parametrize('given', ['list', 'torch', 'torch_int32', 'numpy'])
def test_stable_order_is_the_parents_argsort_and_scatter(name, given):
    deg = DEGREES[name]
    arg = {'list': deg, 'torch': torch.tensor(deg), 'torch_int32': torch.tensor(deg, dtype=torch.int32),
           'numpy': np.asarray(deg)}[given]
    order, position = _tables.stable_order(arg)
    for t in (order, position):
        assert isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.device.type == 'cpu' and t.shape == (len(deg),)
    want_order, want_position = parent_order(deg)
    assert torch.equal(order, want_order) and torch.equal(position, want_position)
    assert torch.equal(position[order], torch.arange(len(deg)))
    # the numpy copy that ``_blocked_f64`` had
    np_order = np.argsort(np.asarray(deg, dtype=np.int64), kind='stable')
    assert order.tolist() == np_order.tolist()
    # stability: equal degrees keep the order of the features
    srt = torch.tensor(deg)[order]
    assert bool((srt[1:] >= srt[:-1]).all())
    assert bool((order[1:] > order[:-1])[srt[1:] == srt[:-1]].all())


def test_blocked_f64_re_exports_the_same_function():
    assert bf.stable_order is _tables.stable_order


#: (P_real, P): affine, the plain shift under the affine tile, 8 bins (25), 8 bins with both bounds learnable (27), SOS of 2
PARAMETERS = [(2, 2), (1, 2), (25, 25), (27, 27), (5, 5)]


@pytest.mark.parametrize('P_real,P', PARAMETERS)
@pytest.mark.parametrize('name', sorted(DEGREES))
def test_packed_rows_without_tiling_is_the_backwards_formula(name, P_real, P):
    n = len(DEGREES[name])
    _, slot_of = parent_order(DEGREES[name])
    p = torch.arange(P_real, device='cpu').repeat_interleave(n)
    want = slot_of.repeat(P_real) * P + p                                # (_backward_plan: row of output o = p*n_tr + t)
    got = _tables.packed_rows(_tables.stable_order(DEGREES[name])[1], P_real, P)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert len(set(got.tolist())) == P_real * n and int(got.min()) >= 0 and int(got.max()) < n * P


@pytest.mark.parametrize('FT', [1, 2, 4])
@pytest.mark.parametrize('P_real,P', PARAMETERS)
@pytest.mark.parametrize('name', sorted(DEGREES))
def test_packed_rows_with_tiling_is_the_fused_plans_formula(name, P_real, P, FT):
    n_g = len(DEGREES[name])
    tile_cols = 16 * P * FT
    _, slot_of = parent_order(DEGREES[name])
    sl = slot_of.repeat(P_real)                                          # (_fused_plan: slot of output row o = p*n_g + t)
    pp = torch.arange(P_real, device='cpu').repeat_interleave(n_g)
    want = (sl // (16 * FT)) * tile_cols + (((sl // 16) % FT) * P + pp) * 16 + (sl % 16)
    got = _tables.packed_rows(_tables.stable_order(DEGREES[name])[1], P_real, P, (FT, tile_cols))
    assert got.dtype == torch.int64 and torch.equal(got, want)
    n_tiles = (n_g + 16 * FT - 1) // (16 * FT)
    assert len(set(got.tolist())) == P_real * n_g
    assert int(got.min()) >= 0 and int(got.max()) < n_tiles * tile_cols


def test_packed_rows_by_hand():
    # three features of degrees (1, 0, 1): slots (1, 0, 2); two parameters each
    _, position = _tables.stable_order([1, 0, 1])
    assert position.tolist() == [1, 0, 2]
    assert _tables.packed_rows(position, 2, 2).tolist() == [2, 0, 4, 3, 1, 5]
    # one 16-feature tile of 2 parameter rows: parameter p of slot s at 16 p + s
    assert _tables.packed_rows(position, 2, 2, (1, 32)).tolist() == [1, 0, 2, 17, 16, 18]
    # the plain shift: only the first of the tile's two parameter rows exists
    assert _tables.packed_rows(position, 1, 2, (1, 32)).tolist() == [1, 0, 2]
    # 17 features on tiles of 2 x 16: slot 16 opens the second 16-feature half of the first tile
    _, position = _tables.stable_order(list(range(17)))
    rows = _tables.packed_rows(position, 2, 2, (2, 64))
    assert rows[16] == 32 and rows[17 + 16] == 48 and rows[17] == 16
