"""Host tests (no GPU) of the blocked float64 backward through the MAF inverse for vector-valued members
(``AutoregressiveFlow.blocked_inverse_backward_vectors``, kernel ``tfep_inverse_backward_chain_vec_f64``): the exported
symbol and its descriptor, which layers take the route, and a numpy emulation of the vector step on the schedule of
``_blocked_f64_backward.plan``.

The emulation walks a small mixed layout (2-vectors, 4-vectors and scalar features with three parameters, interleaved
inside the degrees; slots and links from ``_blocked_f64.feature_slots`` / ``vector_links``) the way the kernel does: a
vector is one unit of work, done at the slot of its component 0; slots of later components are skipped; per component one
chain sum, then ``u_v = T^-T (gx_v - s_v - lx_v)`` and ``q_v = Theta^T u_v + ltheta_v`` with random ``T``, ``Theta`` per
vector.  It is compared with a dense solve of the whole transposed Jacobian; a count matrix shows that every product of every
masked linear is taken exactly once.  Bound: that of tests/test_blocked_f64_backward_host.py -- both sides are float64
evaluations of the same sums in another order on O(1), well-conditioned data: 1e-12 max(1, |u|)."""
import ctypes
import os

import numpy as np
import pytest

from tfep_amd.nn.conditioners import generate_degrees
from tfep_amd.nn.flows import MAF
from tfep_amd.nn.flows import _blocked_f64 as bf
from tfep_amd.nn.flows import _blocked_f64_backward as bfb
from tfep_amd.nn.transformers import MoebiusTransformer, QuaternionProductTransformer, SymmetrizedMoebiusTransformer


# ------------------------------------------------------------------ the C ABI

def test_the_symbol_is_exported_and_the_descriptor_embeds_the_scalar_one():
    from tfep_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    name = 'tfep_inverse_backward_chain_vec_f64'
    assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.load(), name)                                          # bound with its signature
    V, S = _lib.InverseBackwardChainVecF64Desc, _lib.InverseBackwardChainF64Desc
    assert V.chain.offset == 0 and V.chain.size == ctypes.sizeof(S) and ctypes.sizeof(V) >= ctypes.sizeof(S)
    # 2 ints, 2 arrays of 4 ints, 4 doubles, 5 pointers / int64 behind the scalar descriptor
    assert V.n_members.offset == ctypes.sizeof(S) and ctypes.sizeof(V) == ctypes.sizeof(S) + 8 + 32 + 32 + 40
    # the scalar descriptor is what it was
    assert ctypes.sizeof(S) == 528 and S.r.offset == 440 and S.emb_scale.offset == 520
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'tfep_hip.h')) as f:
        header = f.read()
    assert 'int tfep_inverse_backward_chain_vec_f64(const tfep_inverse_backward_chain_vec_f64_desc* desc, void* stream);' in header


# ------------------------------------------------------------------ which layers take the route

FLAGS = ('blocked_inverse_f64_vectors', 'blocked_inverse_backward', 'blocked_inverse_backward_vectors')


def _set(layer, *values):
    for k, v in zip(FLAGS, values):
        setattr(layer, k, v)


def test_the_class_default_is_off():
    from tfep_amd.nn.flows.autoregressive import AutoregressiveFlow
    assert AutoregressiveFlow.blocked_inverse_backward_vectors is False


@pytest.mark.parametrize('make', [QuaternionProductTransformer, lambda: SymmetrizedMoebiusTransformer(4)])
def test_a_vector_layer_takes_the_route_only_with_all_three_flags(make):
    layer = MAF(generate_degrees(8, repeats=4), transformer=make()).double()
    assert not layer._blocked_f64_backward_ok()
    for off in range(3):
        _set(layer, *(i != off for i in range(3)))
        assert not layer._blocked_f64_backward_ok(), FLAGS[off]
    _set(layer, True, True, True)
    assert layer._blocked_f64_ok() and layer._blocked_f64_backward_ok()
    plan = layer._blocked_f64_backward_plan()
    assert plan is not None and layer._blocked_f64_host_plan()['kinds'] in ([2], [3])
    # toggling the new flag on the live layer, plans cached: the answer follows
    layer.blocked_inverse_backward_vectors = False
    assert not layer._blocked_f64_backward_ok() and layer._blocked_f64_backward_plan() is None
    layer.blocked_inverse_backward_vectors = True
    assert layer._blocked_f64_backward_ok() and layer._blocked_f64_backward_plan() is plan


def test_element_wise_layers_do_not_depend_on_the_new_flag():
    layer = MAF(generate_degrees(8)).double()
    for flag in (False, True):
        layer.blocked_inverse_backward_vectors = flag
        assert layer._blocked_f64_backward_ok()                                # (also with blocked_inverse_backward off)


def test_moebius_and_float32_layers_keep_the_pass_per_degree():
    tr = MoebiusTransformer(2)
    tr.float64_kernels = True
    moebius = MAF(generate_degrees(8, repeats=2), transformer=tr, hidden_layers=[20, 20]).double()
    _set(moebius, True, True, True)
    assert moebius._blocked_f64_ok() and moebius._blocked_f64_host_plan()['kinds'] == [5]
    assert not moebius._blocked_f64_backward_ok()
    f32 = MAF(generate_degrees(8, repeats=4), transformer=QuaternionProductTransformer())
    _set(f32, True, True, True)
    assert not f32._blocked_f64_backward_ok()


# ------------------------------------------------------------------ the vector step on the plan's schedule

#: three members on 24 features: 2-vectors, 4-vectors, scalars with three parameters each; ascending degrees
INDICES = [[0, 2, 3, 5, 6, 8, 9, 11], list(range(12, 20)), [1, 4, 7, 10, 20, 21, 22, 23]]
DEGREES = [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 + [4] * 4 + [5] * 4 + [6, 7, 8, 9]
DIMS, PARAMS = [2, 4, 0], [1, 1, 3]


def mixed_layout(widths, seed):
    """Sorted degree vectors, masks and feature records ``[col, member, P, prow0, pos, 0, 1 + component, next slot]``."""
    rng = np.random.default_rng(seed)
    deg_tr = np.asarray(DEGREES)
    n = len(deg_tr)
    member_of, local_of = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for g, ind in enumerate(INDICES):
        member_of[ind], local_of[ind] = g, np.arange(len(ind))
    params_of = np.asarray(PARAMS)[member_of]
    counts = [len(ind) for ind in INDICES]
    offsets = np.concatenate([[0], np.cumsum([p * c for p, c in zip(PARAMS, counts)])])[:-1]
    slot_order, base, _ = bf.feature_slots(deg_tr, params_of, member_of, local_of, offsets, counts)
    links = bf.vector_links(slot_order, deg_tr, member_of, local_of, DIMS)
    assert links is not None
    order0 = np.argsort(deg_tr, kind='stable')
    pos0 = np.empty(n, dtype=np.int64)
    pos0[order0] = np.arange(n)
    feats = np.zeros((n, 8), dtype=np.int64)
    for s, t in enumerate(slot_order):
        feats[s, :6] = (t, member_of[t], params_of[t], base[s], pos0[t], 0)
    feats[:, 6:8] = links
    deg_feat, p_feat = deg_tr[slot_order], params_of[slot_order]
    deg_cols = [deg_tr[order0]] + [np.sort(rng.integers(0, int(deg_tr.max()), size=w)) for w in widths]
    masks = [deg_cols[l + 1][:, None] >= deg_cols[l][None, :] for l in range(len(widths))]
    masks.append(np.repeat(deg_feat, p_feat)[:, None] > deg_cols[-1][None, :])
    return deg_cols, deg_feat, p_feat, masks, feats


def emulate(plan, masks, feats, seed):
    """The schedule with vector steps on random data: ``(u, dense u, count matrices, vectors done)``."""
    rng = np.random.default_rng(seed)
    n_lin = len(masks)
    L = n_lin - 1
    n_rows, n_pad = plan['n_rows'], plan['n_pad']
    n_cols = [m.shape[1] for m in masks]
    W = [rng.normal(size=m.shape) * m / np.sqrt(max(m.shape[1], 1)) for m in masks]
    WT = [np.zeros((n_cols[l], n_pad[l])) for l in range(n_lin)]
    for l in range(n_lin):
        WT[l][:, :n_rows[l]] = W[l].T
    elu = [None] + [rng.uniform(0.05, 1.0, size=n_cols[l]) for l in range(1, n_lin)]
    n_slots = len(feats)
    # the dense blocks: Tb[j, i] = d y_j / d x_i over slots; At[row, j] = d y_j / d theta_row; lx per slot, c per row
    Tb, At = np.zeros((n_slots, n_slots)), np.zeros((n_rows[L], n_slots))
    lx, c = np.zeros(n_slots), rng.normal(size=n_rows[L])
    r = rng.normal(size=n_slots)
    vectors = {}                                             # head slot -> (slots, T, Theta)
    for f in range(n_slots):
        comp, P, prow0 = feats[f, 6], feats[f, 2], feats[f, 3]
        if comp == 0:
            Tb[f, f] = rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0])
            At[prow0:prow0 + P, f] = rng.normal(size=P)
        elif comp == 1:
            slots, s = [], f
            while s >= 0:
                slots.append(s)
                s = feats[s, 7]
            k = len(slots)
            assert k == DIMS[feats[f, 1]] and [feats[s, 6] for s in slots] == list(range(1, k + 1))
            T = 1.5 * np.eye(k) * rng.choice([-1.0, 1.0]) + 0.3 * rng.normal(size=(k, k))
            Theta = rng.normal(size=(k, k))
            rows = feats[slots, 3]
            Tb[np.ix_(slots, slots)] = T
            At[np.ix_(rows, slots)] = Theta.T
            lx[slots] = rng.normal(size=k)
            vectors[f] = (slots, T, Theta)

    ga = [np.zeros(n_pad[l]) for l in range(n_lin)]
    G = [np.full(n_cols[l], np.nan) for l in range(n_lin)]
    cnt = [np.zeros(m.shape, dtype=int) for m in masks]
    u = np.full(n_slots, np.nan)
    done = []
    for b in plan['blocks']:
        S = []
        for l in range(n_lin):
            (c0, c1), R, row0 = b['cols'][l], b['R'][l], b['row0'][l]
            if R < n_pad[l] and c1 > c0:                                                    # panel GEMM
                G[l][c0:c1] = WT[l][c0:c1, R:] @ ga[l][R:]
                cnt[l][R:n_rows[l], c0:c1] += 1
            win = np.full(R - row0, np.nan)                                                 # the LDS window [row0, R)
            win[R - b['n_old'][l] - row0:] = ga[l][R - b['n_old'][l]:R]
            S.append(win)
        for st in b['steps']:
            for l in range(L, 0, -1):
                c0, c1, start = st[2 + 3 * l], st[3 + 3 * l], st[4 + 3 * l]
                for j in range(c0, c1):
                    g = (G[l][j] if b['R'][l] < n_pad[l] else 0.0) + WT[l][j, start:b['R'][l]] @ S[l][start - b['row0'][l]:]
                    cnt[l][start:min(b['R'][l], n_rows[l]), j] += 1
                    S[l - 1][j - b['row0'][l - 1]] = ga[l - 1][j] = g * elu[l][j]
            f0, f1, start = st[0], st[1], st[4]

            def g0_at(pos):
                cnt[0][start:min(b['R'][0], n_rows[0]), pos] += 1
                return (G[0][pos] if b['R'][0] < n_pad[0] else 0.0) + WT[0][pos, start:b['R'][0]] @ S[0][start - b['row0'][0]:]

            def store_q(row, q):
                assert 0 <= row - b['row0'][L] < len(S[L])
                S[L][row - b['row0'][L]] = ga[L][row] = q

            for f in range(f0, f1):
                comp, P, prow0, pos = feats[f, 6], feats[f, 2], feats[f, 3], feats[f, 4]
                if comp > 1:
                    continue                                                                # written with the head of its vector
                if comp == 0:
                    u[f] = (r[f] - g0_at(pos)) / Tb[f, f]
                    for p in range(P):
                        store_q(prow0 + p, At[prow0 + p, f] * u[f] + c[prow0 + p])
                    continue
                slots, s = [], f
                k = DIMS[feats[f, 1]]
                while len(slots) < k and f0 <= s < f1:                                      # a link that leaves the step ends the chain
                    slots.append(s)
                    s = feats[s, 7]
                assert slots == vectors[f][0]
                _, T, Theta = vectors[f]
                g = np.array([r[s] - g0_at(feats[s, 4]) for s in slots])
                uv = np.linalg.solve(T.T, g - lx[slots])
                qv = Theta.T @ uv + c[feats[slots, 3]]
                for i, s in enumerate(slots):
                    assert np.isnan(u[s])
                    u[s] = uv[i]
                    store_q(feats[s, 3], qv[i])
                done.append(f)
    # ---- dense: (Tb^T + K^T At^T ... ) u = r - lx - K^T c with K = d theta / d x through the linearised conditioner
    chain = W[0]
    for l in range(1, n_lin):
        chain = W[l] @ (elu[l][:, None] * chain)
    K = chain[:, feats[:, 4]]                                                               # (n_out, n_slots)
    u_ref = np.linalg.solve(Tb.T + K.T @ At, r - lx - K.T @ c)
    return u, u_ref, cnt, (sorted(done), sorted(vectors))


@pytest.mark.parametrize('block', [1, 2, 3, 16])
@pytest.mark.parametrize('widths', [[23], [19, 37]])
def test_vector_steps_solve_the_transposed_system_and_count_every_product_once(widths, block):
    deg_cols, deg_feat, p_feat, masks, feats = mixed_layout(widths, seed=block + len(widths))
    # slots interleave inside a degree: the first 2-vector sits in slots 0 and 2, a scalar between them
    assert feats[:3, [0, 1, 6, 7]].tolist() == [[0, 0, 1, 2], [1, 2, 0, -1], [2, 0, 2, -1]]
    plan = bfb.plan(deg_cols, deg_feat, p_feat, block)
    assert len(plan['blocks']) == -(-10 // block) and plan['n_fixed'] == 0
    u, u_ref, cnt, (done, heads) = emulate(plan, masks, feats, seed=5)
    assert done == heads and len(heads) == 4 + 2                                # every vector exactly once
    for l, m in enumerate(masks):
        assert np.array_equal(cnt[l], m.astype(int)), f'linear {l}: a product is not taken exactly once'
    assert np.abs(u - u_ref).max() <= 1e-12 * max(1.0, float(np.abs(u_ref).max()))
