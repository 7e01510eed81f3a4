"""Host plan of the vector members of the float64 blocked inverse (``_blocked_f64.vector_links``: the component / next-slot
table of ``tfep_inverse_chain_vec_f64``) and the opt-in route selection (``AutoregressiveFlow.blocked_inverse_f64_vectors``).
No GPU: integer work against hand-written expectations."""
import numpy as np
import torch

from tfep_amd.nn.conditioners import generate_degrees
from tfep_amd.nn.flows import MAF
from tfep_amd.nn.flows import _blocked_f64 as bf
from tfep_amd.nn.transformers import (AffineTransformer, MixedTransformer, NeuralSplineTransformer,
                                      QuaternionProductTransformer, SymmetrizedMoebiusTransformer)


def chains(links):
    """The slot lists of every vector, following the links from each head (component 1)."""
    out = []
    for head in np.nonzero(links[:, 0] == 1)[0]:
        chain, s = [], int(head)
        while s != -1:
            assert links[s, 0] == len(chain) + 1              # components are numbered along the chain
            chain.append(s)
            s = int(links[s, 1])
            assert len(chain) <= len(links)
        out.append(chain)
    return out


def test_adjacent_components_of_a_single_member():
    deg = [0, 0, 0, 1, 1, 1]                                  # two 3-vectors, one per degree
    order, _ = bf.stable_order(deg)
    links = bf.vector_links(order, deg, None, np.arange(6), [3])
    assert links.dtype == np.int32
    assert links.tolist() == [[1, 1], [2, 2], [3, -1], [1, 4], [2, 5], [3, -1]]
    # descending degrees: the second vector takes the first slots
    deg = [1, 1, 0, 0]
    order, _ = bf.stable_order(deg)
    assert order.tolist() == [2, 3, 0, 1]
    assert bf.vector_links(order, deg, None, np.arange(4), [2]).tolist() == [[1, 1], [2, -1], [1, 3], [2, -1]]


def test_components_interleaved_with_another_member_inside_one_degree():
    # features 0, 2: a 2-vector (member 0); feature 1: a scalar feature of member 1; all of degree 0; then the same at degree 1
    deg = [0, 0, 0, 1, 1, 1]
    member = [0, 1, 0, 0, 1, 0]
    local = [0, 0, 1, 2, 1, 3]
    order, _ = bf.stable_order(deg)
    links = bf.vector_links(order, deg, member, local, [2, 0])
    assert links.tolist() == [[1, 2], [0, -1], [2, -1], [1, 5], [0, -1], [2, -1]]
    # the member's own feature order decides the components, not the slot order: local indices swapped in the first vector
    links = bf.vector_links(order, deg, member, [1, 0, 0, 2, 1, 3], [2, 0])
    assert links.tolist() == [[2, -1], [0, -1], [1, 0], [1, 5], [0, -1], [2, -1]]


def test_layers_that_do_not_qualify_give_none():
    order, _ = bf.stable_order([0, 0, 1, 1])
    assert bf.vector_links(order, [0, 0, 1, 1], None, np.arange(4), [2]) is not None
    # a vector that straddles two degrees
    order, _ = bf.stable_order([0, 1, 1, 1])
    assert bf.vector_links(order, [0, 1, 1, 1], None, np.arange(4), [2]) is None
    order, _ = bf.stable_order([0, 1, 2, 3])
    assert bf.vector_links(order, [0, 1, 2, 3], None, np.arange(4), [4]) is None
    # a feature count that is no multiple of the dimension
    order, _ = bf.stable_order([0, 0, 0, 0, 0])
    assert bf.vector_links(order, [0] * 5, None, np.arange(5), [2]) is None
    assert bf.vector_links(order, [0] * 5, [0, 0, 0, 1, 1], [0, 1, 2, 0, 1], [2, 0]) is None
    # a periodic component
    order, _ = bf.stable_order([0, 0, 1, 1])
    assert bf.vector_links(order, [0, 0, 1, 1], None, np.arange(4), [2], [False, False, True, False]) is None
    assert bf.vector_links(order, [0, 0, 1, 1], None, np.arange(4), [2], [False] * 4) is not None
    # (a periodic feature of an element-wise member beside the vectors is fine)
    assert bf.vector_links(order, [0, 0, 1, 1], [0, 0, 1, 1], [0, 1, 0, 1], [2, 0], [False, False, True, True]) is not None


def test_every_chain_has_dim_links_inside_its_step():
    rng = np.random.default_rng(0)
    for dim, n_vec, n_scalar in [(2, 7, 5), (3, 5, 0), (4, 6, 9), (8, 3, 4)]:
        n = dim * n_vec + n_scalar
        perm = rng.permutation(n)                              # where the member's features sit in the layer
        vec_feats, scalar_feats = perm[:dim * n_vec], perm[dim * n_vec:]
        deg = np.zeros(n, dtype=np.int64)
        deg[vec_feats] = np.repeat(rng.integers(0, 4, n_vec), dim)
        deg[scalar_feats] = rng.integers(0, 4, n_scalar)
        member, local = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        member[scalar_feats] = 1
        local[vec_feats], local[scalar_feats] = np.arange(dim * n_vec), np.arange(n_scalar)
        order, _ = bf.stable_order(deg)
        links = bf.vector_links(order, deg, member, local, [dim, 0])
        plan = bf.plan_blocks([np.sort(deg), np.sort(deg)], deg[order], np.ones(n, dtype=np.int64), block=2)
        step_of = {}
        for blk in plan['blocks']:
            for st in blk['steps']:
                for s in range(st[0], st[1]):
                    step_of[s] = (int(st[0]), int(st[1]))
        found = chains(links)
        assert len(found) == n_vec and all(len(c) == dim for c in found)
        for c in found:
            assert all(step_of[s] == step_of[c[0]] for s in c)                 # all inside the head's [slot0, slot1)
            feats = order[c]
            assert (member[feats] == 0).all() and local[feats].tolist() == list(range(local[feats[0]], local[feats[0]] + dim))
            assert local[feats[0]] % dim == 0
        in_chain = np.zeros(n, dtype=bool)
        in_chain[[s for c in found for s in c]] = True
        assert (links[~in_chain] == [0, -1]).all() and (member[order[~in_chain]] == 1).all()


def test_plan_blocks_of_a_scalar_case_is_what_it_was():
    """The numbers of tests/test_blocked_f64_host.py::test_plan_blocks_ascending_by_hand, and feature_slots of a mixed case."""
    plan = bf.plan_blocks([[0, 1, 2, 3], [0, 0, 1, 1, 2, 2]], [0, 1, 2, 3], [2, 2, 2, 2], block=2, align=4)
    assert plan['par_cols'] == 2 and plan['max_feats'] == 1 and plan['max_out_rows'] == 4 and plan['lds_cols'] == 6
    b0, b1 = plan['blocks']
    assert b0['k0'] == [0, 0] and b0['n_old'] == [0, 0] and b0['n_cols'] == [2, 4] and b0['lds_col0'] == [0, 2]
    assert b0['steps'][0, :6].tolist() == [0, 1, 0, 0, 2, 1] and b0['steps'][1, :6].tolist() == [1, 2, 2, 2, 4, 2]
    assert b1['k0'] == [0, 4] and b1['n_old'] == [2, 0] and b1['n_cols'] == [4, 2] and b1['lds_col0'] == [0, 4]
    assert b1['steps'][0, :6].tolist() == [2, 3, 4, 4, 6, 3] and b1['steps'][1, :6].tolist() == [3, 4, 6, 6, 6, 4]
    assert not b0['steps'][:, 6:].any() and not b1['steps'][:, 6:].any()
    order, base, row_of_out = bf.feature_slots([1, 0, 1, 0], [2, 3, 2, 3], [0, 1, 0, 1], [0, 0, 1, 1], [0, 4], [2, 2])
    assert order.tolist() == [1, 3, 0, 2] and base.tolist() == [0, 3, 6, 8, 10]
    assert row_of_out.tolist() == [6, 8, 7, 9, 0, 3, 1, 4, 2, 5]
    fit = bf.fit_block([[0, 1, 2, 3], [0, 0, 1, 1, 2, 2]], [0, 1, 2, 3], [2, 2, 2, 2], 2)
    assert fit['block'] == 2 and len(fit['blocks']) == 2


def _spline(n):
    return NeuralSplineTransformer(torch.full((n,), -4.0), torch.full((n,), 4.0), 8)


def test_the_flag_admits_vector_members_and_nothing_else_changes():
    assert MAF.blocked_inverse_f64_vectors is False
    quat = MAF(generate_degrees(8, repeats=4), transformer=QuaternionProductTransformer()).double()
    sym = MAF(generate_degrees(6, 'descending', repeats=3), transformer=SymmetrizedMoebiusTransformer(3)).double()
    mixed = MAF(torch.tensor([0, 0, 0, 1, 1, 1, 1]),
                transformer=MixedTransformer([SymmetrizedMoebiusTransformer(2), QuaternionProductTransformer(), _spline(1)],
                                             [[0, 2], [3, 4, 5, 6], [1]])).double()
    straddle = MAF(generate_degrees(8), transformer=QuaternionProductTransformer()).double()
    scalar = MAF(generate_degrees(6), transformer=AffineTransformer()).double()
    assert scalar._blocked_f64_ok()
    feats_before = scalar._blocked_f64_host_plan()['feats'].copy()
    for layer in (quat, sym, mixed, straddle):
        assert not layer._blocked_f64_ok()
    for layer in (quat, sym, mixed, straddle, scalar):
        layer.blocked_inverse_f64_vectors = True
    assert quat._blocked_f64_ok() and sym._blocked_f64_ok() and mixed._blocked_f64_ok() and scalar._blocked_f64_ok()
    assert not straddle._blocked_f64_ok()                     # one degree per feature: the pass per degree
    assert np.array_equal(scalar._blocked_f64_host_plan()['feats'], feats_before) and not feats_before[:, 6:].any()
    assert quat._blocked_f64_host_plan()['kinds'] == [3] and sym._blocked_f64_host_plan()['kinds'] == [2]
    hp = mixed._blocked_f64_host_plan()
    assert hp['kinds'] == [2, 3, 1] and hp['par_cols'] == _spline(1).n_parameters_per_feature
    #                          col member        P                   (component, next)
    assert hp['feats'][:, [0, 1]].tolist() == [[0, 0], [1, 2], [2, 0], [3, 1], [4, 1], [5, 1], [6, 1]]
    assert hp['feats'][:, 6:].tolist() == [[1, 2], [0, -1], [2, -1], [1, 4], [2, 5], [3, 6], [4, -1]]
    assert hp['feats'][[0, 2, 3], 2].tolist() == [1, 1, 1]    # one parameter per feature of a vector member
    # a float32 layer and blocked_inverse = False stay out, flag or not
    f32 = MAF(generate_degrees(8, repeats=4), transformer=QuaternionProductTransformer())
    f32.blocked_inverse_f64_vectors = True
    assert not f32._blocked_f64_ok() and f32._blocked_ok()
    quat.blocked_inverse = False
    assert not quat._blocked_f64_ok()
    # the flag is part of the cache key: switching it off again takes the layer out
    sym.blocked_inverse_f64_vectors = False
    assert not sym._blocked_f64_ok()
