"""The conditions the EGNN shape cases (``egnn_cases.py``) rest on, checked on the host: the cutoffs keep clear of every
pair, the cases land on the tiles, ragged blocks and awkward grids they are meant for, and the float64 oracle that
``test_gpu_egnn_shapes.py`` compares the kernels with is consistent with itself and reachable in float32."""
import numpy as np
import pytest
import torch

import egnn_cases as ec

CASES = pytest.mark.parametrize('name', ec.NAMES)
TILES = ec.TILES
MARGIN = 1e-3                  # of r_cutoff
REL32 = 1e-5                   # the bound of the GPU tests: plain float32 must be able to meet it


@CASES
def test_cutoff_keeps_clear_of_every_pair(name):
    c = ec.case(name)
    margin, share = ec.cutoff_margin_and_share(c['x'], c['n'], c['r_cutoff'])
    layers = ec.layer_margins(name)
    print(f'{name}: r_cutoff {c["r_cutoff"]:.6f}, margin {margin:.2e} x r_cutoff, kept share {share:.3f}, '
          f'margin at the input of every layer {", ".join(f"{m:.1e}" for m in layers)}')
    assert c['r_cutoff'] == float(np.float32(c['r_cutoff']))            # the kernels receive exactly this number
    assert margin >= MARGIN
    assert layers[0] == margin and min(layers) >= MARGIN
    if ec.CASES[name]['cutoff'] == 'inside':
        assert share == 1.0 and c['r_cutoff'] == float(np.float32(2.0 * c['side'] * ec.A))
    else:
        assert 0.05 < share < 0.8
        assert abs(c['r_cutoff'] / (ec.CASES[name]['cutoff'] * ec.A) - 1.0) <= 0.05


@CASES
def test_case_is_deterministic_and_shaped(name):
    c = ec.case(name)
    n, B = c['n'], c['B']
    assert c['x'].shape == c['v'].shape == (B, 3 * n) and c['x'].dtype == c['v'].dtype == torch.float32
    assert c['t'] == 0.37 and c['kwargs']['time_feat_dim'] == c['cfg']['time_feat_dim'] == 4
    assert c['kwargs']['node_types'] == [i % 3 for i in range(n)]
    assert len([k for k in c['sd64'] if k.startswith('graph_layer_') and k.endswith('message_mlp.0.weight')]) == c['layers']
    x0, sd0 = c['x'].clone(), {k: p.clone() for k, p in c['sd64'].items()}
    ec.case.cache_clear()
    again = ec.case(name)
    assert torch.equal(again['x'], x0) and again['r_cutoff'] == c['r_cutoff']
    assert all(torch.equal(again['sd64'][k], p) for k, p in sd0.items())
    # the module the GPU test builds holds the float32 parameters the float64 state dict was widened from
    dyn = ec.dynamics(name)
    assert all(torch.equal(p.double(), again['sd64'][k]) for k, p in dyn.state_dict().items() if p.is_floating_point())


@CASES
def test_tile_and_ragged_blocks(name):
    from tfep_amd import _lib
    c = ec.case(name)
    raw, nt = TILES[name]
    assert ec.raw_tier(c['F'], c['G']) == raw and ec.tile(c['F'], c['G']) == nt
    assert _lib.load().tfep_egnn_tile(c['F'], c['G']) == nt
    assert ec.dynamics(name)._tile() == nt
    n = c['n']
    assert c['n_blk'] == -(-n // 16) > 1 and n % 16 != 0 and n % 8 != 0


def test_table_covers_the_tiers_and_awkward_grids():
    assert {ec.raw_tier(c['F'], c['G']) for c in ec.CASES.values()} == {1, 2, 3}
    assert {raw for raw, _ in TILES.values()} == {1, 2, 3}
    grids = {(c['B'] * -(-c['n'] // 16)) % 8 for c in ec.CASES.values()}
    assert len(grids - {0}) >= 3, grids
    assert any(c['layers'] == 1 for c in ec.CASES.values()) and any(c['layers'] >= 3 for c in ec.CASES.values())
    assert any(c['B'] == 1 for c in ec.CASES.values())
    # tile 2 with and without feature padding, and a tile chosen by G alone
    assert any(max(c['F'], c['G']) == 32 == min(c['F'], c['G']) for c in ec.CASES.values())
    assert any(ec.raw_tier(c['F'], 1) < ec.raw_tier(c['F'], c['G']) for c in ec.CASES.values())


@CASES
def test_float64_oracle_is_self_adjoint_consistent(name):
    """``(J v) . w == v . (w^T J)`` for an independent ``w``: forward mode (double reverse) against one reverse pass."""
    c = ec.case(name)
    ref = ec.reference(name)
    assert ref is ec.reference(name) and not ref['vel'].flags.writeable          # cached, read-only
    w = torch.randn(c['B'], 3 * c['n'], generator=torch.Generator().manual_seed(99), dtype=torch.float64)
    wj = ec.oracle_vjp(name, w)
    v = c['v'].double().numpy()
    for lhs, rhs, terms, what in (((ref['jv'] * w.numpy()).sum(1), (v * wj).sum(1), np.abs(v * wj).sum(1), 'w'),
                                  ((ref['jv'] * v).sum(1), (v * ref['vj']).sum(1), np.abs(v * ref['vj']).sum(1), 'v')):
        err = np.abs(lhs - rhs) / np.maximum(terms, 1.0)
        print(f'{name}: |(J v) . {what} - v . ({what}^T J)| / max(sum |terms|, 1) = {err.max():.2e}')
        assert err.max() <= 1e-10
    assert np.linalg.norm(ref['vel']) > 0.1 and np.linalg.norm(ref['jv']) > 0.1 and np.linalg.norm(ref['vj']) > 0.1
    # the velocity preserves the centre of geometry
    assert np.abs(ref['vel'].reshape(c['B'], c['n'], 3).sum(1)).max() <= 1e-12 * c['n']


@CASES
def test_float32_oracle_meets_the_gpu_bound(name):
    c = ec.case(name)
    r64, r32 = ec.reference(name), ec.reference(name, torch.float32)
    last = 3 * 16 * (c['n_blk'] - 1)
    for k in ('vel', 'jv', 'vj'):
        e, e_last = ec.rel_l2(r32[k], r64[k]), ec.rel_l2(r32[k][:, last:], r64[k][:, last:])
        print(f'{name}: float32 oracle vs float64, {k}: rel L2 {e:.2e}, atoms of the last block {e_last:.2e}')
        assert e <= REL32 and e_last <= REL32
