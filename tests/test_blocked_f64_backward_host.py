"""Host-side planning of the blocked float64 backward through the MAF inverse (tfep_amd/nn/flows/_blocked_f64_backward.py).
No GPU: the plan's schedule (panels + chain, LDS windows, step tables) is emulated in numpy on small MADE-shaped problems and
compared with a dense solve of ``J^T u + K^T c = r``; a count matrix shows that every (row, column) product of every masked
linear is taken exactly once; the LDS formula, ``fit`` and the exported symbols.

The emulation reads what the kernel reads: the panel value from ``G``, the rows ``[start, R)`` from the block's LDS window
(filled by the block itself, and by the ``n_old`` rows loaded at its start), never the global ``ga`` of the current block.
Bound: both sides are float64 evaluations of the same sums in another order on O(1) data with ``|tau_x| >= 0.5``: 1e-12."""
import ctypes

import numpy as np
import pytest
import torch

from tfep_amd.nn.conditioners import generate_degrees
from tfep_amd.nn.flows import MAF
from tfep_amd.nn.flows import _blocked_f64 as bf
from tfep_amd.nn.flows import _blocked_f64_backward as bfb
from tfep_amd.nn.transformers import NeuralSplineTransformer


def emulate(plan, masks, feats, fixed, seed, scale=1.7):
    """Runs the plan's schedule on random data and returns ``(u, u_fixed, dense u, dense u_fixed, count matrices)``.

    ``masks[l]``: boolean (rows, columns) of linear ``l`` in sorted order; ``feats``: (n_slots, 8) records
    ``[_, _, P, prow0, pos, periodic, ..]``; ``fixed``: ``[(pos, periodic)]`` of the inputs no step transforms."""
    rng = np.random.default_rng(seed)
    n_lin = len(masks)
    L = n_lin - 1
    n_rows, n_pad = plan['n_rows'], plan['n_pad']
    n_cols = [m.shape[1] for m in masks]
    assert [m.shape[0] for m in masks] == n_rows
    W = [rng.normal(size=m.shape) * m / np.sqrt(max(m.shape[1], 1)) for m in masks]
    WT = [np.zeros((n_cols[l], n_pad[l])) for l in range(n_lin)]
    for l in range(n_lin):
        WT[l][:, :n_rows[l]] = W[l].T
    elu = [None] + [rng.uniform(0.05, 1.0, size=n_cols[l]) for l in range(1, n_lin)]       # ELU' of the inputs of linear l
    n_slots = len(feats)
    tau = rng.uniform(0.5, 2.0, size=n_slots) * rng.choice([-1.0, 1.0], size=n_slots)
    A, c = rng.normal(size=n_rows[L]), rng.normal(size=n_rows[L])
    r = rng.normal(size=n_slots)
    r_fixed = rng.normal(size=len(fixed))
    trig = rng.uniform(0, 2 * np.pi, size=n_cols[0])                                        # t of a periodic pair, by position

    def embed_T(g0, pos, periodic):
        """s = E^T G_0 of one feature."""
        if not periodic:
            return g0[pos]
        return scale * (-np.sin(trig[pos]) * g0[pos] + np.cos(trig[pos]) * g0[pos + 1])

    # ---- the schedule
    ga = [np.zeros(n_pad[l]) for l in range(n_lin)]
    G = [np.full(n_cols[l], np.nan) for l in range(n_lin)]
    cnt = [np.zeros(m.shape, dtype=int) for m in masks]
    u = np.full(n_slots, np.nan)
    prev_d0 = None
    for b in plan['blocks']:
        assert prev_d0 is None or b['d1'] == prev_d0                                       # descending, contiguous
        prev_d0 = b['d0']
        S, total = [], 0
        for l in range(n_lin):
            (c0, c1), R, row0 = b['cols'][l], b['R'][l], b['row0'][l]
            assert R % bf.ALIGN == 0 and 0 <= R - b['first_final'][l] == b['n_old'][l] < bf.ALIGN and R <= n_pad[l]
            assert b['lds_row0'][l] == total and 0 <= row0 <= b['first_final'][l]
            total += R - row0
            if R < n_pad[l] and c1 > c0:                                                    # panel GEMM
                G[l][c0:c1] = WT[l][c0:c1, R:] @ ga[l][R:]
                cnt[l][R:n_rows[l], c0:c1] += 1
            win = np.full(R - row0, np.nan)                                                 # the LDS window [row0, R)
            win[R - b['n_old'][l] - row0:] = ga[l][R - b['n_old'][l]:R]
            S.append(win)
        assert total == b['lds_rows'] <= plan['lds_rows']
        prev_deg_slots = None
        for st in b['steps']:
            for l in range(L, 0, -1):
                c0, c1, start = st[2 + 3 * l], st[3 + 3 * l], st[4 + 3 * l]
                assert b['cols'][l][0] <= c0 <= c1 <= b['cols'][l][1] and b['row0'][l] <= start <= b['first_final'][l]
                for j in range(c0, c1):
                    g = (G[l][j] if b['R'][l] < n_pad[l] else 0.0) + WT[l][j, start:b['R'][l]] @ S[l][start - b['row0'][l]:]
                    cnt[l][start:min(b['R'][l], n_rows[l]), j] += 1
                    v = g * elu[l][j]
                    assert 0 <= j - b['row0'][l - 1] < len(S[l - 1])                       # lands inside the window of linear l - 1
                    S[l - 1][j - b['row0'][l - 1]] = v
                    ga[l - 1][j] = v
            f0, f1, start = st[0], st[1], st[4]
            assert prev_deg_slots is None or f1 == prev_deg_slots                          # slots walked downwards, none skipped
            prev_deg_slots = f0
            for f in range(f0, f1):
                P, prow0, pos, periodic = feats[f, 2:6]
                g0 = {}
                for p in ((pos, pos + 1) if periodic else (pos,)):
                    assert b['cols'][0][0] <= p < b['cols'][0][1]
                    g0[p] = (G[0][p] if b['R'][0] < n_pad[0] else 0.0) + WT[0][p, start:b['R'][0]] @ S[0][start - b['row0'][0]:]
                    cnt[0][start:min(b['R'][0], n_rows[0]), p] += 1
                u[f] = (r[f] - embed_T(g0, pos, periodic)) / tau[f]
                for p in range(P):
                    row = prow0 + p
                    assert 0 <= row - b['row0'][L] < len(S[L])
                    S[L][row - b['row0'][L]] = ga[L][row] = A[row] * u[f] + c[row]
    n_fixed = plan['n_fixed']
    g0 = WT[0][:n_fixed] @ ga[0]                                                           # the inputs no step transforms
    cnt[0][:, :n_fixed] += 1
    u_fixed = np.array([r_fixed[i] - embed_T(g0, pos, per) for i, (pos, per) in enumerate(fixed)])

    # ---- dense: K = d theta / d x through the linearised conditioner; (diag(tau) + K_tr^T A^T) u = r - K_tr^T c
    def E_col(pos, periodic):
        e = np.zeros(n_cols[0])
        if periodic:
            e[pos], e[pos + 1] = -scale * np.sin(trig[pos]), scale * np.cos(trig[pos])
        else:
            e[pos] = 1.0
        return e
    chain = W[0]
    for l in range(1, n_lin):
        chain = W[l] @ (elu[l][:, None] * chain)
    K_tr = chain @ np.stack([E_col(feats[f, 4], feats[f, 5]) for f in range(n_slots)], axis=1)       # (n_out, n_slots)
    At = np.zeros((n_rows[L], n_slots))
    for f in range(n_slots):
        At[feats[f, 3]:feats[f, 3] + feats[f, 2], f] = A[feats[f, 3]:feats[f, 3] + feats[f, 2]]
    JT = np.diag(tau) + K_tr.T @ At
    u_ref = np.linalg.solve(JT, r - K_tr.T @ c)
    q = At @ u_ref + c
    uf_ref = np.array([r_fixed[i] - E_col(pos, per) @ (chain.T @ q) for i, (pos, per) in enumerate(fixed)])
    return u, u_fixed, u_ref, uf_ref, cnt


def synthetic(n_lin, widths, seed, n_fixed_plain=2, feats_per_degree=(1, 3, 2, 1, 1, 2, 1), P=(2, 3)):
    """Sorted degree vectors, masks, feature records of a small MADE-shaped problem: several features per degree, features
    of degree -1 (one of them periodic), one periodic transformed feature, hidden widths as given."""
    rng = np.random.default_rng(seed)
    deg_feat = np.repeat(np.arange(len(feats_per_degree)), feats_per_degree)
    p_feat = rng.choice(P, size=len(deg_feat))
    periodic = np.zeros(len(deg_feat), dtype=bool)
    periodic[len(deg_feat) // 2] = True
    # inputs in degree order: the fixed ones (plain, then one periodic pair), then the features' positions
    fixed = [(i, False) for i in range(n_fixed_plain)] + [(n_fixed_plain, True)]
    deg_in = [-1] * (n_fixed_plain + 2)
    pos = []
    for d, per in zip(deg_feat, periodic):
        pos.append(len(deg_in))
        deg_in += [d] * (2 if per else 1)
    d_top = int(deg_feat.max())
    deg_cols = [np.asarray(deg_in)] + [np.sort(rng.integers(-1, d_top, size=w)) for w in widths[:n_lin - 1]]
    base = np.concatenate([[0], np.cumsum(p_feat)])
    feats = np.zeros((len(deg_feat), 8), dtype=np.int64)
    feats[:, 2], feats[:, 3], feats[:, 4], feats[:, 5] = p_feat, base[:-1], pos, periodic
    masks = [deg_cols[l + 1][:, None] >= deg_cols[l][None, :] for l in range(n_lin - 1)]
    masks.append(np.repeat(deg_feat, p_feat)[:, None] > deg_cols[-1][None, :])
    return deg_cols, deg_feat, p_feat, masks, feats, fixed


@pytest.mark.parametrize('block', [1, 5, 16, 64])
@pytest.mark.parametrize('n_lin,widths', [(2, [23]), (4, [19, 37, 21])])
def test_schedule_solves_the_transposed_system_and_counts_every_product_once(n_lin, widths, block):
    deg_cols, deg_feat, p_feat, masks, feats, fixed = synthetic(n_lin, widths, seed=block + n_lin)
    assert any(w % 16 for w in widths)
    plan = bfb.plan(deg_cols, deg_feat, p_feat, block)
    assert plan['blocks'][-1]['d0'] == -1 and plan['n_fixed'] == 4
    if block == 64:
        assert len(plan['blocks']) == 1
    u, uf, u_ref, uf_ref, cnt = emulate(plan, masks, feats, fixed, seed=3)
    for l, m in enumerate(masks):
        assert np.array_equal(cnt[l], m.astype(int)), f'linear {l}: a product is not taken exactly once'
    scale = max(1.0, float(np.abs(u_ref).max()))
    assert np.abs(u - u_ref).max() <= 1e-12 * scale and np.abs(uf - uf_ref).max() <= 1e-12 * scale


def _layer_problem(maf):
    """Sorted masks, feature records and fixed inputs of a float64 MAF layer, from its own forward host plan."""
    hp = maf._blocked_f64_host_plan()
    assert hp is not None
    lins = maf._conditioner._linears()
    col_pos = [hp['pos0']] + hp['hidden_pos']
    row_pos = hp['hidden_pos'] + [hp['row_of_out']]
    masks = []
    for l, lin in enumerate(lins):
        m = lin.mask.numpy() != 0
        sm = np.zeros_like(m)
        sm[np.ix_(row_pos[l], col_pos[l])] = m
        masks.append(sm)
    fixed = [(p, False) for _, p in hp['fixed_plain']] + [(p, True) for _, p in hp['fixed_periodic']]
    return hp, masks, hp['feats'].astype(np.int64), fixed


@pytest.mark.parametrize('order', ['ascending', 'descending'])
@pytest.mark.parametrize('block', [1, 5, 16, 64])
def test_layer_plans_ascending_and_descending(order, block):
    from tfep_amd.nn.embeddings import PeriodicEmbedding
    D = 21
    deg = generate_degrees(D, order, conditioning_indices=[3, 10], repeats=2)
    emb = PeriodicEmbedding(D, [0.0, 1.0], periodic_indices=[1, 10, 12])
    maf = MAF(deg, transformer=NeuralSplineTransformer(torch.zeros(D - 2), torch.ones(D - 2), 3), hidden_layers=3,
              embedding=emb).double()
    maf.inverse_block_f64 = block
    hp, masks, feats, fixed = _layer_problem(maf)
    plan = maf._blocked_f64_backward_plan()
    assert plan is not None and maf._blocked_f64_backward_ok()
    # (the three hidden layers and the 190 parameter rows of a whole-range block do not fit the LDS: the block is halved)
    assert plan['block'] <= block and bfb.lds_bytes(plan['lds_rows']) <= bf.LDS_LIMIT and (block > 5 or plan['block'] == block)
    assert sorted(p for p, _ in fixed) == [0, 1] and plan['n_fixed'] == 3               # feature 3 plain, feature 10 a pair
    u, uf, u_ref, uf_ref, cnt = emulate(plan, masks, feats, fixed, seed=11, scale=2 * np.pi)
    for l, m in enumerate(masks):
        assert np.array_equal(cnt[l], m.astype(int)), f'linear {l}'
    scale = max(1.0, float(np.abs(u_ref).max()))
    assert np.abs(u - u_ref).max() <= 1e-12 * scale and np.abs(uf - uf_ref).max() <= 1e-12 * scale


def test_which_layers_take_the_blocked_backward():
    from tfep_amd.nn.transformers import QuaternionProductTransformer
    deg = generate_degrees(8)
    maf = MAF(deg).double()
    assert maf.blocked_inverse_backward is False and maf._blocked_f64_backward_ok()
    assert not MAF(deg)._blocked_f64_backward_ok()                                       # float32
    quat = MAF(generate_degrees(8, repeats=4), transformer=QuaternionProductTransformer()).double()
    quat.blocked_inverse_f64_vectors = True
    assert quat._blocked_f64_ok() and not quat._blocked_f64_backward_ok()               # vector members: pass per degree
    maf.blocked_inverse = False
    assert not maf._blocked_f64_backward_ok()


def test_lds_formula_and_fit_halves_the_block():
    from tfep_amd import _lib
    lib = _lib.load()
    for n in (0, 1, 279, 320):
        assert lib.tfep_inverse_backward_chain_f64_lds_bytes(n) == bfb.lds_bytes(n) == n * 64 * 8
    assert lib.tfep_inverse_backward_chain_f64_lds_bytes(-1) < 0
    assert bfb.lds_bytes(320) == bf.LDS_LIMIT
    deg_cols = [np.arange(64), np.repeat(np.arange(63), 8)]
    args = (deg_cols, np.arange(64), np.full(64, 25))
    # 16 degrees: 128 + <= 15 hidden rows, 400 + <= 15 parameter rows: more than 320 rows of LDS; 8 degrees: 64 + 200 + the old rows
    full = bfb.plan(*args, 16)
    assert full['lds_rows'] > 320
    fitted = bfb.fit(*args, 16)
    assert fitted['block'] == 8 and fitted['lds_rows'] == bfb.plan(*args, 8)['lds_rows'] <= 320
    assert bfb.fit(*args, 16, limit=bfb.lds_bytes(full['lds_rows']))['block'] == 16
    assert bfb.fit(*args, 16, limit=1024) is None
    with pytest.raises(ValueError):
        bfb.plan([np.arange(4)], np.arange(4), np.full(4, 2), 4)
    with pytest.raises(ValueError):
        bfb.plan([np.arange(4)[::-1], np.arange(4)], np.arange(4), np.full(4, 2), 4)


def test_new_symbols_are_exported_and_the_descriptor_mirrors_the_header():
    from tfep_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('tfep_inverse_backward_chain_f64', 'tfep_inverse_backward_chain_f64_lds_bytes'):
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS, name
    # 4 ints, 8 arrays of 5 pointers / int64, 5 arrays of 5 ints + 1, 3 + 3 + 2 + 2 pointers / int64, 1 double
    assert ctypes.sizeof(_lib.InverseBackwardChainF64Desc) == 16 + 8 * 40 + 104 + 10 * 8 + 8
    assert _lib.InverseBackwardChainF64Desc.r.offset == 440 and _lib.InverseBackwardChainF64Desc.emb_scale.offset == 520
