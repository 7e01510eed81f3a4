"""Host-side planning of the blocked float64 backward through the MAF inverse (``_backward.BlockedInverseBackwardF64``):
pure integer work on sorted degree vectors, no device needed (tests/test_blocked_f64_backward_host.py).  The mirror of
``_blocked_f64.plan_blocks``; the packing (``stable_order``), the feature slots (``feature_slots``) and the ``feats`` records
are those of the forward plan.

The backward of the inverse is the triangular solve ``J^T u + gl grad_x ldj = gx``.  It walks the degrees
DOWNWARDS: the cotangent of a unit of degree ``d`` collects, through the TRANSPOSED masked linears, the cotangents ``ga`` of
the rows that read it -- rows of degree ``>= d`` of a hidden linear (masks ``>=``), parameter rows of features of degree
``> d`` of the output linear (strict) -- so in the degree-sorted packing a mask COLUMN is a suffix ``[start, n)`` of the packed
rows.

Blocks ``[d0, d1)`` are walked in descending order.  For linear ``l`` the rows of degree ``>= d1`` (parameter rows of features
of degree ``>= d1``) are final when the block starts: ``first_final`` is the first of them.  The fp64-MFMA GEMM multiplies the
block's columns with rows ``[R, n_pad)``, ``R`` = ``first_final`` rounded UP to the GEMM's k granularity (16), and the chain
kernel (``csrc/inverse_backward_f64.hip``) adds rows ``[start, R)`` of every column: each product is counted exactly once.
"""
import numpy as np

from ._blocked_f64 import ALIGN, LDS_LIMIT, MAX_LINEARS, ROWS, feature_slots, stable_order    # noqa: F401  (one definition each)

STEP_INTS = 20        # ints per degree in the backward chain kernel's step table


def lds_bytes(n_rows_total):
    """LDS of one chain launch (``tfep_inverse_backward_chain_f64_lds_bytes``)."""
    return n_rows_total * ROWS * 8


def plan(deg_cols, deg_feat, p_feat, block, align=ALIGN):
    """Blocks of the backward substitution.

    Arguments as ``_blocked_f64.plan_blocks``: ``deg_cols[l]`` the SORTED degrees of the inputs of linear ``l`` (for ``l >= 1``
    also the rows of linear ``l - 1``), ``deg_feat`` the SORTED degrees of the transformed features (slot order), ``p_feat``
    the parameters per slot (slot ``s`` owns rows ``[base[s], base[s] + p_feat[s])`` of the output linear).

    Returns a dict with ``n_rows`` / ``n_pad`` (rows of every linear, and padded to ``align``), ``n_fixed`` (inputs of degree
    -1), and ``blocks`` in the order they run (descending).  Per block: ``d0, d1`` and, per linear, ``cols`` (the block's
    columns; the inputs of degree -1 are not among them), ``first_final``, ``R``, ``row0`` (first row of the block: the LDS
    window is ``[row0, R)``), ``n_old`` (= ``R - first_final``: rows of earlier blocks the panel leaves out), ``lds_row0``
    (running sum of ``R - row0``), and ``steps``: one row of ``STEP_INTS`` ints per degree, DESCENDING,
    ``[slot0, slot1, (col0, col1, start) for l = 0 .. L]`` -- columns ``[col0, col1)`` of linear ``l`` have this degree and
    their mask is the rows ``[start, n)``.
    """
    deg_cols = [np.asarray(d, dtype=np.int64) for d in deg_cols]
    deg_feat = np.asarray(deg_feat, dtype=np.int64)
    p_feat = np.asarray(p_feat, dtype=np.int64)
    for d in (*deg_cols, deg_feat):
        if len(d) > 1 and np.any(np.diff(d) < 0):
            raise ValueError('plan: degrees must be sorted')
    n_lin = len(deg_cols)
    L = n_lin - 1
    if not (2 <= n_lin <= MAX_LINEARS):
        raise ValueError(f'plan: {n_lin} linears unsupported (2..{MAX_LINEARS})')
    if 2 + 3 * n_lin > STEP_INTS:
        raise ValueError('plan: step table too small')
    if block < 1:
        raise ValueError('plan: block must be >= 1')
    base = np.concatenate([[0], np.cumsum(p_feat)])
    d_min = int(min(deg_cols[0].min(), deg_feat.min()))
    d_max = int(deg_feat.max())
    n_fixed = int(np.searchsorted(deg_cols[0], -1, side='right'))
    n_rows = [len(deg_cols[l + 1]) for l in range(L)] + [int(base[-1])]
    n_pad = [(n + align - 1) // align * align for n in n_rows]

    def lo(a, v):
        return int(np.searchsorted(a, v, side='left'))

    def hi(a, v):
        return int(np.searchsorted(a, v, side='right'))

    def row_lo(l, d):
        """First row of linear ``l`` whose unit (feature, for the output linear) has degree >= d."""
        return lo(deg_cols[l + 1], d) if l < L else int(base[lo(deg_feat, d)])

    blocks = []
    for d0 in reversed(range(d_min, d_max + 1, block)):      # the block boundaries of the forward plan, walked downwards
        d1 = min(d0 + block, d_max + 1)
        cols = [(lo(dc, d0), lo(dc, d1)) for dc in deg_cols]
        cols[0] = (max(cols[0][0], n_fixed), max(cols[0][1], n_fixed))      # (no step transforms them: one GEMM at the end)
        first_final = [row_lo(l, d1) for l in range(n_lin)]
        R = [(f + align - 1) // align * align for f in first_final]
        row0 = [row_lo(l, d0) for l in range(n_lin)]
        n_lds = [r - r0 for r, r0 in zip(R, row0)]
        steps = np.zeros((d1 - d0, STEP_INTS), dtype=np.int32)
        for i, d in enumerate(reversed(range(d0, d1))):
            steps[i, 0], steps[i, 1] = lo(deg_feat, d), hi(deg_feat, d)
            for l in range(n_lin):
                steps[i, 2 + 3 * l], steps[i, 3 + 3 * l] = lo(deg_cols[l], d), hi(deg_cols[l], d)
                # hidden rows '>=': units of degree >= d; output rows strict: features of degree > d
                steps[i, 4 + 3 * l] = row_lo(l, d) if l < L else int(base[hi(deg_feat, d)])
        blocks.append(dict(d0=d0, d1=d1, cols=cols, first_final=first_final, R=R, row0=row0,
                           n_old=[r - f for r, f in zip(R, first_final)],
                           lds_row0=[int(v) for v in np.concatenate([[0], np.cumsum(n_lds)[:-1]])],
                           lds_rows=int(sum(n_lds)), steps=steps))
    return dict(blocks=blocks, n_linears=n_lin, base=base, n_rows=n_rows, n_pad=n_pad, n_fixed=n_fixed,
                lds_rows=max(b['lds_rows'] for b in blocks))


def fit(deg_cols, deg_feat, p_feat, block, limit=LDS_LIMIT):
    """The plan with the largest block size ``<= block`` (halving) whose state fits the chain kernel's LDS, or None."""
    g = int(block)
    while g >= 1:
        p = plan(deg_cols, deg_feat, p_feat, g)
        if lds_bytes(p['lds_rows']) <= limit:
            p['block'] = g
            return p
        g //= 2
    return None
