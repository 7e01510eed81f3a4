"""Host-side planning of the float64 blocked inverse (``AutoregressiveFlow._inverse_blocked_f64``): pure integer work on
degree vectors, no device needed (tests/test_blocked_f64_host.py).

Every masked linear of the MADE conditioner is packed with its rows AND columns sorted by degree (stable), so that

* the units / inputs / features of a run of consecutive degrees are contiguous ranges, and
* a mask row is a prefix ``[0, cut)`` of the packed columns: ``cut`` = the number of inputs of degree ``<= k`` for a hidden
  row of degree ``k`` (masks ``>=``), of degree ``< k`` for a parameter row of a feature of degree ``k`` (strict ``>``).

The degrees are walked in blocks ``[d0, d1)``.  For linear ``l`` the columns of degree ``< d0`` are final when the block
starts (and so are, from the very start, the inputs of degree -1, which no step transforms); the fp64-MFMA GEMM
multiplies the block's rows with columns ``[0, k0)``, ``k0`` = that count rounded DOWN to the GEMM's k granularity (16),
and the chain kernel (``csrc/inverse_block_f64.hip``) adds columns ``[k0, cut)`` of every row: each product is counted
exactly once.

Vector-valued members (symmetrized Moebius, quaternion product; ``blocked_inverse_f64_vectors``): ``vector_links`` says
which slots are the components of one vector, for ``tfep_inverse_chain_vec_f64``.
"""
import numpy as np

from ..._tables import stable_order    # noqa: F401  (the one definition of the packing order; callers take it from here too)

ALIGN = 16            # k granularity of tfep_masked_linear_gemm_f64
STEP_INTS = 16        # ints per degree in the chain kernel's step table
FEAT_INTS = 8         # ints per feature slot
MAX_LINEARS = 5       # TFEP_INVERSE_F64_MAX_LINEARS
MAX_MEMBERS = 4       # TFEP_INVERSE_F64_MAX_MEMBERS
LDS_LIMIT = 160 * 1024
ROWS = 64             # sample rows per workgroup of the chain kernel


def lds_bytes(n_cols_total, par_cols, max_feats):
    """LDS of one chain launch (``tfep_inverse_chain_f64_lds_bytes``)."""
    return (n_cols_total + par_cols * max_feats + max_feats) * ROWS * 8


def plan_blocks(deg_cols, deg_feat, p_feat, block, align=ALIGN):
    """Blocks of the forward substitution.

    ``deg_cols[l]``: SORTED degrees of the inputs of linear ``l`` (``l = 0``: the conditioner inputs; ``l >= 1``: the units of
    hidden layer ``l - 1``, which are also the rows of linear ``l - 1``); ``deg_feat``: SORTED degrees of the transformed
    features (slot order); ``p_feat``: parameters per feature slot (the rows of the output linear: slot ``s`` owns rows
    ``[base[s], base[s] + p_feat[s])``); ``block``: degrees per block.

    Returns a dict with ``blocks`` -- per block ``d0, d1``, per linear ``k0`` / ``n_old`` / ``n_cols`` / ``lds_col0``, the row
    range ``rows[l]`` of every hidden linear and ``out_rows`` of the output linear, and ``steps`` (one row of ``STEP_INTS`` ints
    per degree: ``[slot0, slot1, cut_out, (row0, row1, cut) per hidden linear]``) -- and the sizes the workspaces need.
    """
    deg_cols = [np.asarray(d, dtype=np.int64) for d in deg_cols]
    deg_feat = np.asarray(deg_feat, dtype=np.int64)
    p_feat = np.asarray(p_feat, dtype=np.int64)
    for d in (*deg_cols, deg_feat):
        if len(d) > 1 and np.any(np.diff(d) < 0):
            raise ValueError('plan_blocks: degrees must be sorted')
    n_lin = len(deg_cols)
    L = n_lin - 1
    if not (2 <= n_lin <= MAX_LINEARS):
        raise ValueError(f'plan_blocks: {n_lin} linears unsupported (2..{MAX_LINEARS})')
    if 3 + 3 * L > STEP_INTS:
        raise ValueError('plan_blocks: step table too small')
    if block < 1:
        raise ValueError('plan_blocks: block must be >= 1')
    base = np.concatenate([[0], np.cumsum(p_feat)])
    d_min = int(min(deg_cols[0].min(), deg_feat.min()))
    d_max = int(deg_feat.max())
    n_fixed = int(np.searchsorted(deg_cols[0], -1, side='right'))    # inputs of degree -1 pass through: never produced by a step

    def lo(a, v):
        return int(np.searchsorted(a, v, side='left'))

    def hi(a, v):
        return int(np.searchsorted(a, v, side='right'))

    blocks = []
    for d0 in range(d_min, d_max + 1, block):
        d1 = min(d0 + block, d_max + 1)
        first = [lo(dc, d0) for dc in deg_cols]                       # columns of degree < d0: final before the block
        first[0] = max(first[0], n_fixed)                             # (and the inputs no step transforms: known from the start)
        k0 = [c // align * align for c in first]
        n_old = [c - k for c, k in zip(first, k0)]
        n_cols = [lo(dc, d1) - k for dc, k in zip(deg_cols, k0)]
        lds_col0 = [int(v) for v in np.concatenate([[0], np.cumsum(n_cols)[:-1]])]
        s0, s1 = lo(deg_feat, d0), lo(deg_feat, d1)
        steps = np.zeros((d1 - d0, STEP_INTS), dtype=np.int32)
        for i, d in enumerate(range(d0, d1)):
            steps[i, 0], steps[i, 1] = lo(deg_feat, d), hi(deg_feat, d)
            steps[i, 2] = lo(deg_cols[L], d)                          # strict '>': inputs of degree < d
            for l in range(L):
                steps[i, 3 + 3 * l] = lo(deg_cols[l + 1], d)
                steps[i, 4 + 3 * l] = hi(deg_cols[l + 1], d)
                steps[i, 5 + 3 * l] = hi(deg_cols[l], d)               # '>=': inputs of degree <= d
        blocks.append(dict(
            d0=d0, d1=d1, k0=k0, n_old=n_old, n_cols=n_cols, lds_col0=lds_col0,
            rows=[(lo(deg_cols[l + 1], d0), lo(deg_cols[l + 1], d1)) for l in range(L)],
            out_rows=(int(base[s0]), int(base[s1])), slots=(s0, s1), steps=steps))
    counts = np.bincount(deg_feat - d_min) if len(deg_feat) else np.zeros(1, dtype=np.int64)
    return dict(blocks=blocks, n_linears=n_lin, base=base,
                par_cols=int(max(int(p_feat.max()), 2)), max_feats=int(max(int(counts.max()), 1)),
                max_out_rows=max(max(b['out_rows'][1] - b['out_rows'][0] for b in blocks), 1),
                lds_cols=max(sum(b['n_cols']) for b in blocks))


def fit_block(deg_cols, deg_feat, p_feat, block, limit=LDS_LIMIT):
    """The plan with the largest block size ``<= block`` (halving) whose state fits the chain kernel's LDS, or None."""
    g = int(block)
    while g >= 1:
        plan = plan_blocks(deg_cols, deg_feat, p_feat, g)
        if lds_bytes(plan['lds_cols'], plan['par_cols'], plan['max_feats']) <= limit:
            plan['block'] = g
            return plan
        g //= 2
    return None


def feature_slots(deg_tr, params_of, member_of=None, local_of=None, member_offset=None, member_count=None):
    """Slot order of the transformed features and the packed row of every conditioner output.

    ``deg_tr``: degree of transformed feature ``t``; ``params_of[t]``: its parameter count.  Plain transformer
    (``member_of`` None): output ``p * n_tr + t`` is parameter ``p`` of feature ``t``.  Mixed transformer: output
    ``member_offset[g] + p * member_count[g] + local_of[t]`` with ``g = member_of[t]`` (parameters grouped by member).

    Returns ``(slot_order, base, row_of_out)``: ``slot_order[s]`` = the feature in slot ``s`` (stable by degree), ``base[s]`` its
    first packed row, ``row_of_out[o]`` the packed row of output ``o``.
    """
    deg_tr = np.asarray(deg_tr, dtype=np.int64)
    params_of = np.asarray(params_of, dtype=np.int64)
    n_tr = len(deg_tr)
    order = stable_order(deg_tr)[0].numpy()
    p_slot = params_of[order]
    base = np.concatenate([[0], np.cumsum(p_slot)])
    row_of_out = np.full(int(params_of.sum()), -1, dtype=np.int64)
    for s, t in enumerate(order):
        p = np.arange(p_slot[s])
        if member_of is None:
            outs = p * n_tr + t
        else:
            g = int(member_of[t])
            outs = member_offset[g] + p * member_count[g] + int(local_of[t])
        row_of_out[outs] = base[s] + p
    if np.any(row_of_out < 0):
        raise ValueError('feature_slots: the conditioner outputs do not match the transformer parameters')
    return order, base, row_of_out


def vector_links(slot_order, deg_tr, member_of, local_of, member_dim, periodic_of=None):
    """The links of the vector members (``tfep_inverse_chain_vec_f64``: ints 6 and 7 of a feature record).

    ``slot_order[s]``: the transformed feature in slot ``s`` (``feature_slots``); ``deg_tr[t]`` / ``member_of[t]`` /
    ``local_of[t]``: degree, member and index inside its member of feature ``t`` (``member_of`` None: one member);
    ``member_dim[g]``: the vector dimension of member ``g``, 0 for an element-wise member; ``periodic_of[t]``: is the feature
    periodic in the conditioner's embedding (None: none is).

    Vector ``v`` of a member is its local features ``[v * dim, (v + 1) * dim)`` -- the reference's ``reshape(B, -1, dim)``
    on the member's own feature order.  Returns the ``(n_slots, 2)`` int32 table ``[1 + component, next slot]`` (component
    0 for an element-wise member, next -1 at the last component and for element-wise members), or None when a member's
    feature count is no multiple of its dimension, a vector spans two degrees, or a component is periodic.  Slots are
    sorted by degree, so all the links of a vector stay inside the slot range of its degree.
    """
    slot_order = np.asarray(slot_order, dtype=np.int64)
    deg_tr = np.asarray(deg_tr, dtype=np.int64)
    local_of = np.asarray(local_of, dtype=np.int64)
    n = len(slot_order)
    member_of = np.zeros(n, dtype=np.int64) if member_of is None else np.asarray(member_of, dtype=np.int64)
    periodic_of = np.zeros(n, dtype=bool) if periodic_of is None else np.asarray(periodic_of, dtype=bool)
    slot_of = np.empty(n, dtype=np.int64)
    slot_of[slot_order] = np.arange(n)
    links = np.zeros((n, 2), dtype=np.int32)
    links[:, 1] = -1
    for g, dim in enumerate(member_dim):
        dim = int(dim)
        if dim == 0:
            continue
        feats = np.nonzero(member_of == g)[0]
        if len(feats) % dim != 0:
            return None
        feats = feats[np.argsort(local_of[feats], kind='stable')]
        if not np.array_equal(local_of[feats], np.arange(len(feats))):
            return None
        for vec in feats.reshape(-1, dim):
            if np.any(deg_tr[vec] != deg_tr[vec[0]]) or np.any(periodic_of[vec]):
                return None
            slots = slot_of[vec]
            links[slots, 0] = 1 + np.arange(dim)
            links[slots[:-1], 1] = slots[1:]
    return links
