"""GPU tests of the split-precision operands (csrc/split_gemm.hip): conversion, GEMM accuracy against float64
(the exact-fp32 MFMA kernel beside it), masks / k-ranges, ragged shapes and the HIP-graph-safe weight scale."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def unsplit(s, inv, cols):
    """Rebuild fp32 values from split rows (host-side check only)."""
    R = s.shape[0]
    raw = s.view(torch.float16).reshape(R, -1, 2, 8).float()          # (rows, k-groups, hi/lo, 8)
    v = (raw[:, :, 0] + raw[:, :, 1]).reshape(R, -1)[:, :cols]
    return v * (inv.reshape(-1, 1) if inv.numel() == R else inv[0])


def test_split_rows_round_trip_and_scales():
    from tfep_amd import ops
    tk = ops.tile_sizes()[2]
    assert tk == 32
    torch.manual_seed(0)
    x = torch.randn(300, 1000, device='cuda') * torch.logspace(-6, 6, 300, device='cuda')[:, None]
    x[7] = 0.0                                             # all-zero row: scale 1
    xs, inv = ops.split_rows(x, ops.round_up(1000, tk))
    assert xs.shape == (300, 1024) and inv.shape == (300,)
    raw = xs.view(torch.float16).reshape(300, -1, 2, 8)
    assert torch.isfinite(raw.float()).all()
    amax = (raw[:, :, 0].float().abs()).amax(dim=(1, 2))
    live = x.abs().amax(1) > 0
    assert bool(((amax[live] >= 2.0 ** 14 - 8) & (amax[live] <= 2.0 ** 15)).all())      # max |v * s| in [2^14, 2^15)
    assert float(inv[7]) == 1.0 and bool((raw[7] == 0).all())
    lg = torch.log2(inv)
    assert torch.equal(lg, lg.round())                                                  # powers of two
    err = (unsplit(xs, inv, 1000).double() - x.double()).abs() / x.abs().amax(1, keepdim=True).clamp_min(1e-30).double()
    assert float(err.max()) < 2.0 ** -22
    assert bool((xs[:, 1000:] == 0).all())                                              # zero padding
    ws, winv = ops.split_rows(x, 1024, per_tensor=True)
    assert winv.shape == (2,)
    err = (unsplit(ws, winv, 1000).double() - x.double()).abs().max() / x.abs().max()
    assert float(err) < 2.0 ** -22


@pytest.mark.parametrize('B,K,N', [(1000, 1000, 700), (513, 4097, 300), (1, 33, 17), (255, 64, 256), (257, 31, 1)])
@pytest.mark.parametrize('act', [0, 1])
def test_split_gemm_matches_float64(B, K, N, act):
    from tfep_amd import ops
    tm, tn, tk = ops.tile_sizes()
    torch.manual_seed(B + K + N)
    kp, npad = ops.round_up(K, tk), ops.round_up(N, tk)
    a = torch.randn(B, K, device='cuda')
    a = torch.where(a > 0, a, torch.expm1(a))
    w = torch.randn(N, K, device='cuda') / K ** 0.5
    bias = torch.zeros(npad, device='cuda')
    bias[:N] = torch.randn(N, device='cuda')
    ap = ops.pad_columns(a, kp)
    wp = ops.masked_weight_prepare(w, None, None, n_rows_padded=npad, k_padded=kp)
    ref = a.double() @ w.double().T + bias[:N].double()
    if act:
        ref = torch.where(ref > 0, ref, torch.expm1(ref))
    as_, ainv = ops.split_rows(ap, kp)
    ws_, winv = ops.split_rows(wp, kp, per_tensor=True)
    y = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, act=act)
    y32 = ops.masked_linear_packed(ap, wp, bias, N, act=act)
    scale = a.double().abs() @ w.double().abs().T + bias[:N].double().abs()
    e_split = float(((y.double() - ref).abs() / scale).max())
    e_fp32 = float(((y32.double() - ref).abs() / scale).max())
    assert e_split < 1e-6, (e_split, e_fp32)
    assert e_split < 4 * e_fp32 + 2e-7, (e_split, e_fp32)             # fp32-equivalent
    y2 = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, act=act)
    assert torch.equal(y, y2)


def test_split_gemm_rows_spanning_ten_decades_under_a_triangular_mask():
    """MADE's structure at its worst for a per-row scale: activations whose magnitude grows by 10 decades along k and a
    prefix (autoregressive) mask, so that early outputs see ONLY the tiny entries while the row scale is set by the
    largest one.  What the split format promises -- and what is asserted -- is an ABSOLUTE error of ~2^-22 of
    (row maximum) x sum_k |w_jk| per output (fp32-equivalent norm-wise per row); the exact-fp32 MFMA kernel is also
    accurate COMPONENT-wise (error relative to sum_k |a_k w_jk| of the visible entries).  Both are measured and
    printed side by side; the component-wise loss of the split path on the outputs that see only entries below
    ~2^-19 of the row maximum is the documented limit (use ``split_gemm=False`` for such data)."""
    from tfep_amd import ops
    tm, tn, tk = ops.tile_sizes()
    torch.manual_seed(5)
    B, K, N = 256, 1024, 1024
    decades = 10.0 * torch.arange(K, device='cuda') / (K - 1) - 10.0             # 1e-10 ... 1 along k
    a = torch.randn(B, K, device='cuda') * torch.pow(10.0, decades)[None, :]
    w = torch.randn(N, K, device='cuda') / K ** 0.5
    deg_in = torch.arange(K, device='cuda')
    deg_out = torch.sort(torch.randint(1, K + 1, (N,), device='cuda')).values
    mask = (deg_out[:, None] > deg_in[None, :]).float()                          # row j sees the prefix k < deg_out[j]
    npad = ops.round_up(N, tk)
    wp = ops.masked_weight_prepare(w, None, mask, n_rows_padded=npad, k_padded=K)
    bias = torch.zeros(npad, device='cuda')
    wm = (w * mask).double()
    ref = a.double() @ wm.T
    comp = a.double().abs() @ wm.abs().T                                        # sum_k |a_k w_jk| over the visible k
    rowmax = a.double().abs().max(dim=1, keepdim=True).values * wm.abs().sum(dim=1)[None, :]
    as_, ainv = ops.split_rows(a.contiguous(), K)
    ws_, winv = ops.split_rows(wp, K, per_tensor=True)
    y_split = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, act=0).double()
    y_fp32 = ops.masked_linear_packed(a.contiguous(), wp, bias, N, act=0).double()
    seen = comp > 0
    cw_split = float(((y_split - ref).abs() / comp)[seen].max())
    cw_fp32 = float(((y_fp32 - ref).abs() / comp)[seen].max())
    nw_split = float(((y_split - ref).abs() / rowmax)[seen].max())
    nw_fp32 = float(((y_fp32 - ref).abs() / rowmax)[seen].max())
    # outputs whose visible entries are all within 2^-12 of the row maximum keep fp32-like component-wise accuracy
    big = seen & (comp > rowmax * 2.0 ** -12)
    cw_split_big = float(((y_split - ref).abs() / comp)[big].max())
    print(f'10-decade rows, prefix mask: component-wise max error split {cw_split:.2e} / exact-fp32 {cw_fp32:.2e}; '
          f'relative to (row max x sum|w|): split {nw_split:.2e} / exact-fp32 {nw_fp32:.2e}; '
          f'split, outputs within 2^-12 of the row scale: {cw_split_big:.2e}')
    assert cw_fp32 < 2e-6                         # exact fp32 products: accurate component-wise
    assert nw_split < 1e-6                        # split: fp32-equivalent relative to the row scale ...
    assert cw_split_big < 1e-3                    # ... and component-wise wherever the entries are not dwarfed


def test_default_path_is_guarded_against_rows_the_split_format_cannot_carry():
    """The DEFAULT arithmetic is data-aware: a layer large enough for the size rule to pick the
    split-f16 GEMMs checks the scales of the input FEATURES first (``AutoregressiveFlow.split_guard``: the largest magnitude
    of every feature over the batch; a lone small value in a row does not count).  Ordinary data:
    the guard passes, the result IS the split path's, bit for bit.  Rows spanning 10 decades (what the test above shows the
    split format cannot carry component-wise): the call runs on the exact-fp32 kernels, bit for bit the ``split_gemm =
    False`` result, and the first masked linear is accurate COMPONENT-wise on that default path (error relative to
    sum_k |x_k w_jk| over the entries each output sees) -- forced split is not."""
    import warnings
    from tfep_amd import ops
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    torch.manual_seed(11)
    D, B = 200, 512
    layer = MAF(generate_degrees(D, 'ascending'), transformer=NeuralSplineTransformer(torch.full((D,), -5.0), torch.full((D,), 5.0), 8),
                initialize_identity=False).cuda()
    assert layer._conditioner.split_worthwhile(B) and layer.split_gemm is None            # the size rule says split
    x_ok = torch.randn(B, D, device='cuda').clamp_(-4.9, 4.9)
    x_ok[7, 3] = 1e-9                                      # a lone tiny value: not what the guard is about
    decades = 10.0 * torch.arange(D, device='cuda') / (D - 1) - 10.0                     # 1e-10 ... 1 along the features
    x_wide = torch.randn(B, D, device='cuda').clamp_(-4.9, 4.9) * torch.pow(10.0, decades)[None, :]

    def run(x, split):
        layer.split_gemm = split
        with torch.no_grad():
            out = layer(x)
        layer.split_gemm = None
        return out
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        y_d, l_d = run(x_ok, None)
        assert layer.last_split_guard == dict(feature_scales_out_of_range=False, exact=False) and not caught
        y_s, l_s = run(x_ok, True)
        assert torch.equal(y_d, y_s) and torch.equal(l_d, l_s)
        y_d, l_d = run(x_wide, None)
        assert layer.last_split_guard['exact'] and layer.last_split_guard['feature_scales_out_of_range']
        assert any('exact-fp32' in str(w.message) for w in caught)
    y_e, l_e = run(x_wide, False)
    assert torch.equal(y_d, y_e) and torch.equal(l_d, l_e)
    # component-wise accuracy of the first masked linear on the path the default takes for this data
    made = layer._conditioner
    lin = made.layers[0]
    w_eff = (lin.mask * lin.weight_v * (lin.weight_g / lin.weight_v.norm(dim=1, keepdim=True))).double()
    w_eff = torch.where(lin.mask == 0, torch.zeros_like(w_eff), w_eff)
    pre = x_wide.double() @ w_eff.T + lin.bias.double()
    comp = x_wide.double().abs() @ w_eff.abs().T + lin.bias.double().abs()

    def first_layer(split):
        layer.split_gemm = split
        with torch.no_grad(), layer._range_guard(x_wide):
            use = layer._use_split_gemm(B)
            plan = made.plan(x_wide.device)
            h = ops.pad_columns(x_wide, plan['k_pad'][0])
            if use:
                ws, w_inv, b, _ = made._pack_layer_split(plan, 0, lin)
                hs, h_inv = ops.split_rows(h, plan['k_pad'][0])
                out = ops.masked_linear_split(hs, h_inv, ws, w_inv, b, plan['n_pad'][0], k_ranges=plan['k_ranges'][0], act=0,
                                              tile_order=plan['tile_order'][0])
            else:
                w, b = made._pack_layer(plan, 0, lin)
                out = ops.masked_linear_packed(h, w, b, plan['n_pad'][0], k_ranges=plan['k_ranges'][0], act=0,
                                               tile_order=plan['tile_order'][0])
        layer.split_gemm = None
        row_of = plan['row_of_out'][0] if plan.get('row_of_out') is not None else None
        return out, use, row_of
    out_d, used_split, row_of = first_layer(None)
    assert not used_split                                          # the guard sent this data to the exact kernel
    got = out_d[:, row_of.long()].double()                         # packed position of hidden unit u: row_of[u]
    cw_default = float(((got - pre).abs() / comp).max())
    out_s, used_split, _ = first_layer(True)
    assert used_split
    cw_forced_split = float(((out_s[:, row_of.long()].double() - pre).abs() / comp).max())
    print(f'first masked linear, 10-decade rows: component-wise error default path {cw_default:.2e}, forced split {cw_forced_split:.2e}')
    assert cw_default < 2e-6
    # (inside a MADE the exact fp32 bias of every unit dominates sums that see only tiny inputs: forced split is not worse
    # HERE, 2.4e-7 -- the guard is for the product itself, see the test above with zero bias: component-wise error 1.0)
    assert cw_forced_split < 1e-3


def test_inverse_and_graph_replays_are_guarded_too():
    """The range guard of the split-f16 default beyond the eager forward (ADVICE r3 / VERDICT r3 item 9).  ``inverse``: its conditioner
    inputs are its own output, so the feature scales of the x it has produced decide -- ordinary data: the split path's result, bit
    for bit; features spanning 10 decades: the call is repeated on the exact-fp32 kernels, bit for bit the ``split_gemm = False``
    result.  ``GraphedFlow``: the captured call runs the split kernels and computes the flag on the device; a flagged replay is
    repeated eagerly (where the guard picks the exact kernels), an ordinary one is the graph's result."""
    import warnings
    from tfep_amd.graphs import GraphedFlow
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    torch.manual_seed(12)
    D, B = 200, 512
    layer = MAF(generate_degrees(D, 'ascending'), transformer=NeuralSplineTransformer(torch.full((D,), -5.0), torch.full((D,), 5.0), 8),
                initialize_identity=False).cuda()
    assert layer._conditioner.split_worthwhile(B) and layer.split_gemm is None
    x_ok = torch.randn(B, D, device='cuda').clamp_(-4.9, 4.9)
    decades = 10.0 * torch.arange(D, device='cuda') / (D - 1) - 10.0
    x_wide = torch.randn(B, D, device='cuda').clamp_(-4.9, 4.9) * torch.pow(10.0, decades)[None, :]

    def inv(y, split):
        layer.split_gemm = split
        with torch.no_grad():
            out = layer.inverse(y)
        layer.split_gemm = None
        return out
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        y_ok, _ = layer(x_ok)
        y_wide, _ = layer(x_wide)
        # ---- inverse
        xd, ld = inv(y_ok, None)
        assert layer.last_split_guard == dict(feature_scales_out_of_range=False, exact=False, inverse=True)
        xs, ls = inv(y_ok, True)
        assert torch.equal(xd, xs) and torch.equal(ld, ls)
        xd, ld = inv(y_wide, None)
        assert layer.last_split_guard == dict(feature_scales_out_of_range=True, exact=True, inverse=True)
        xe, le = inv(y_wide, False)
        assert torch.equal(xd, xe) and torch.equal(ld, le)
        assert float(((xd - x_wide).abs() / (x_wide.abs() + 1e-6)).max()) < 5e-2       # (and it is the inverse)
        # ---- graph replays
        g = GraphedFlow(layer, B, D)
        assert g.n_guarded_calls == 1
        yg, lg = g(x_ok)
        ye, le = layer(x_ok)
        assert not g.last_call_guarded and torch.equal(yg, ye) and torch.equal(lg, le)
        yg, lg = g(x_wide)
        ye, le = layer(x_wide)
        assert g.last_call_guarded and layer.last_split_guard['exact'] and torch.equal(yg, ye) and torch.equal(lg, le)
        yg, lg = g(x_ok)                                   # the flag is cleared by every replay
        assert not g.last_call_guarded
        gi = GraphedFlow(layer, B, D, inverse=True)
        xg, _ = gi(y_wide)
        assert gi.last_call_guarded and torch.equal(xg, xd)
        xg, _ = gi(y_ok)
        assert not gi.last_call_guarded and torch.equal(xg, xs)


def test_sequence_reads_its_layers_guards_once_and_repeats_from_the_first_flagged_layer():
    """``SequentialFlow.forward`` defers the range guards of its layers (one host synchronisation per flow call):
    the results are those of the layers called one by one, each under its own guard -- bit for bit -- whether no layer, the first
    or a later one is flagged."""
    import warnings
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF, SequentialFlow
    from tfep_amd.nn.flows import autoregressive
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    torch.manual_seed(13)
    D, B = 200, 512

    def maf(order, identity):
        return MAF(generate_degrees(D, order), transformer=NeuralSplineTransformer(torch.full((D,), -5.0), torch.full((D,), 5.0), 8),
                   initialize_identity=identity).cuda()
    x_ok = torch.randn(B, D, device='cuda').clamp_(-4.9, 4.9)
    decades = 10.0 * torch.arange(D, device='cuda') / (D - 1) - 10.0
    x_wide = torch.randn(B, D, device='cuda').clamp_(-4.9, 4.9) * torch.pow(10.0, decades)[None, :]

    def one_by_one(layers, x):
        total, verdicts = None, []
        for layer in layers:
            x, l = layer(x)
            verdicts.append(None if layer.split_gemm is not None else layer.last_split_guard['exact'])
            total = l if total is None else total + l
        return x, total, verdicts
    syncs = []
    real = autoregressive.ops.range_flag
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        # (a) random layers: ordinary data flags nothing; 10-decade data flags the first layer
        flow = SequentialFlow(maf('ascending', False), maf('descending', False), maf('ascending', False))
        for x, expect in ((x_ok, [False, False, False]), (x_wide, [True, False, False])):
            y1, l1, verdicts = one_by_one(list(flow), x)
            assert verdicts == expect
            autoregressive.ops.range_flag = lambda *a, **k: (syncs.append(1), real(*a, **k))[1]
            try:
                del syncs[:]
                y2, l2 = flow(x)
            finally:
                autoregressive.ops.range_flag = real
            assert torch.equal(y1, y2) and torch.equal(l1, l2)
            # the per-layer read-backs happen only in the repeat from the first flagged layer on
            assert len(syncs) == (3 if expect[0] else 0)
        # (b) a pinned identity layer first (no guard of its own): the SECOND layer sees the 10 decades
        first = maf('ascending', True)
        first.split_gemm = False
        flow = SequentialFlow(first, maf('descending', False), maf('ascending', False))
        y1, l1, verdicts = one_by_one(list(flow), x_wide)
        assert verdicts == [None, True, False]
        y2, l2 = flow(x_wide)
        assert torch.equal(y1, y2) and torch.equal(l1, l2)
        assert flow[1].last_split_guard['exact'] and not flow[2].last_split_guard['exact']


def test_split_gemm_with_mask_k_ranges_and_tile_order():
    """Block-triangular mask (sorted MADE degrees): k-ranges in units of 32 skip tiles; results as the dense product."""
    from tfep_amd import ops
    tm, tn, tk = ops.tile_sizes()
    torch.manual_seed(3)
    B, K, N = 300, 640, 700
    deg_in = torch.sort(torch.randint(1, 20, (K,), device='cuda')).values
    deg_out = torch.sort(torch.randint(1, 20, (N,), device='cuda')).values
    mask = (deg_out[:, None] >= deg_in[None, :]).float()
    a = torch.randn(B, K, device='cuda')
    w = torch.randn(N, K, device='cuda')
    npad = ops.round_up(N, tk)
    wp = ops.masked_weight_prepare(w, None, mask, n_rows_padded=npad, k_padded=K)
    n_tiles = (npad + tn - 1) // tn
    kr = ops.mask_k_ranges(mask, tn, n_tiles, K)
    assert bool((kr % tk == 0).all()) and int(kr[0, 1]) < K            # first tile really skips k-tiles
    order = ops.heavy_first_order(kr)
    bias = torch.zeros(npad, device='cuda')
    as_, ainv = ops.split_rows(a, K)
    ws_, winv = ops.split_rows(wp, K, per_tensor=True)
    y = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, k_ranges=kr, tile_order=order)
    ref = a.double() @ (w * mask).double().T
    scale = a.double().abs() @ (w * mask).double().abs().T + 1e-30
    assert float(((y.double() - ref).abs() / scale).max()) < 1e-6


def test_split_operand_validation():
    from tfep_amd import ops
    a = torch.randn(4, 48, device='cuda')
    with pytest.raises(ValueError, match='cols_padded'):
        ops.split_rows(a, 48)                                          # not a multiple of 32
    as_, ainv = ops.split_rows(a, 64)
    assert as_.shape == (4, 64)
    e, einv = ops.split_rows(torch.empty(0, 64, device='cuda'), 64)
    assert e.shape == (0, 64)


def test_forward_paths_agree_on_golden_flows():
    """Every golden flow through the split-f16 and the exact-fp32 GEMM paths: same outputs to fp32 rounding."""
    import golden_util as gu
    g = gu.load('flows.npz')
    for name in ['cfg1', 'rq4', 'cond', 'circ', 'mixflow']:
        flow = gu.build_flow(name, g)
        x = torch.from_numpy(g[f'{name}/x']).cuda()
        with torch.no_grad():
            for layer in flow:
                layer.split_gemm = True
            ys, ls = flow(x)
            for layer in flow:
                layer.split_gemm = False
            yf, lf = flow(x)
        assert float((ys - yf).norm() / yf.norm()) < 1e-6, name
        assert torch.allclose(ls, lf, rtol=1e-5, atol=2e-5), name


def test_split_gemm_non_finite_and_extreme_rows_stay_local():
    """A NaN / inf / huge / tiny activation row must not disturb the other rows (per-row scales)."""
    from tfep_amd import ops
    torch.manual_seed(5)
    B, K, N = 64, 256, 96
    a = torch.randn(B, K, device='cuda')
    w = torch.randn(N, K, device='cuda') / 16
    bias = torch.zeros(N, device='cuda')
    wp = ops.masked_weight_prepare(w, None, None, n_rows_padded=N, k_padded=K)
    ws_, winv = ops.split_rows(wp, K, per_tensor=True)

    def run(a_):
        as_, ainv = ops.split_rows(a_, K)
        return ops.masked_linear_split(as_, ainv, ws_, winv, bias, N)
    clean = run(a)
    a2 = a.clone()
    a2[3, 5] = float('nan')
    a2[7, 9] = float('inf')
    a2[11] *= 1e30
    a2[13] *= 1e-30
    y = run(a2)
    keep = torch.ones(B, dtype=torch.bool, device='cuda')
    keep[[3, 7, 11, 13]] = False
    assert torch.equal(y[keep], clean[keep])
    assert not torch.isfinite(y[3]).any() and not torch.isfinite(y[7]).all()
    ref11 = (a2[11].double() @ w.double().T)
    assert float(((y[11].double() - ref11).abs() / (a2[11].double().abs() @ w.double().abs().T)).max()) < 1e-6
    ref13 = (a2[13].double() @ w.double().T)
    assert float(((y[13].double() - ref13).abs() / (a2[13].double().abs() @ w.double().abs().T)).max()) < 1e-6


@pytest.mark.parametrize('B,K,N', [(300, 640, 704), (1, 64, 32), (257, 96, 288)])
def test_elu_layer_writing_split_rows_directly(B, K, N):
    """Hidden layer with the split-row epilogue (scale from the bound max|x| * max_j sum_k |w_jk| + max|b|): the rows
    it writes decode to ELU(x W^T + b) as accurately as the fp32 output converted afterwards."""
    from tfep_amd import ops
    torch.manual_seed(B + N)
    x = torch.randn(B, K, device='cuda') * torch.logspace(-2, 2, B, device='cuda')[:, None]
    w = torch.randn(N, K, device='cuda') / K ** 0.5
    g = torch.rand(N, 1, device='cuda') + 0.5
    bias = torch.randn(N, device='cuda')
    ws = torch.zeros(N, K, device='cuda')
    w_buf = torch.zeros(4, device='cuda')
    ops.masked_weight_prepare_split(w, g, None, None, None, ws, w_buf)
    w_eff = (g * w / w.norm(dim=1, keepdim=True)).double()
    l1 = float(w_eff.abs().sum(1).max())
    assert abs(float(w_buf[2]) - l1) < 1e-4 * l1                      # row-L1 maximum of the effective weights
    xs, x_inv = ops.split_rows(x, K)
    hs, h_inv = ops.masked_linear_split(xs, x_inv, ws, w_buf, bias, N, act=1, split_out=True)
    assert hs.shape == (B, N) and h_inv.shape == (B,)
    ref = x.double() @ w_eff.T + bias.double()
    ref = torch.where(ref > 0, ref, torch.expm1(ref))
    got = unsplit(hs, h_inv, N).double()
    scale = x.double().abs() @ w_eff.abs().T + bias.double().abs() + 1.0
    assert float(((got - ref).abs() / scale).max()) < 1e-6
    raw = hs.view(torch.float16).reshape(B, -1, 2, 8).float()
    assert torch.isfinite(raw).all() and float(raw.abs().max()) < 2.0 ** 15   # the bound keeps fp16 in range
    fp32 = ops.masked_linear_split(xs, x_inv, ws, w_buf, bias, N, act=1)
    assert float(((got - fp32.double()).abs() / scale).max()) < 5e-7


@pytest.mark.parametrize('B,K,N,S', [(700, 4096, 300, 3), (257, 1000, 90, 2), (64, 2048, 513, 8), (5, 64, 7, 4)])
def test_split_gemm_split_k_slabs_add_up(B, K, N, S):
    """k_split: S slabs of partial sums (bias in slab 0) whose sum is the un-split product -- bit for bit the same
    fp32 partial products, summed in another order -- with a k-range per column tile; deterministic."""
    from tfep_amd import ops
    tm, tn, tk = ops.tile_sizes()
    torch.manual_seed(B + K + N + S)
    kp, npad = ops.round_up(K, tk), ops.round_up(N, tk)
    a = ops.pad_columns(torch.randn(B, K, device='cuda'), kp)
    w = ops.masked_weight_prepare(torch.randn(N, K, device='cuda') / K ** 0.5, None, None, n_rows_padded=npad, k_padded=kp)
    bias = torch.randn(npad, device='cuda')
    n_tiles = (N + tn - 1) // tn
    kr = torch.tensor([[0, kp - tk * min(t, kp // tk - 1)] for t in range(n_tiles)], dtype=torch.int32, device='cuda')
    as_, ainv = ops.split_rows(a, kp)
    ws_, winv = ops.split_rows(w, kp, per_tensor=True)
    full = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, k_ranges=kr)
    slabs = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, k_ranges=kr, k_split=S)
    assert slabs.shape == (S, B, N)
    scale = float(full.abs().max()) + 1.0
    assert float((slabs.sum(0) - full).abs().max()) < 2e-6 * scale
    cols = torch.arange(N, device='cuda')
    ref = torch.zeros(B, N, dtype=torch.float64, device='cuda')
    for t in range(n_tiles):                                   # float64 reference honouring the k-ranges
        c = cols[t * tn:(t + 1) * tn]
        ke = int(kr[t, 1])
        ref[:, c] = a[:, :ke].double() @ w[c, :ke].double().T + bias[c].double()
    assert float((slabs.double().sum(0) - ref).abs().max()) < 2e-6 * scale
    again = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, k_ranges=kr, k_split=S)
    assert torch.equal(slabs, again)


def test_split_columns_with_a_caller_fixed_scale():
    """tfep_split_columns_scaled: a panel filled a few columns at a time ends up as the same split rows as converting it
    whole with the same (bound-based) scale; untouched columns stay untouched; loose bounds keep fp32-level accuracy."""
    from tfep_amd import ops
    torch.manual_seed(3)
    R, C = 300, 200
    x = torch.randn(R, C, device='cuda') * torch.logspace(-3, 3, R, device='cuda')[:, None]
    bound = x.abs().amax(1) * torch.logspace(0, 3, R, device='cuda')          # up to 1000x above the true maximum
    inv = ops.pow2_inv_scale(bound)
    assert torch.equal(torch.log2(inv), torch.log2(inv).round())
    assert bool((bound / inv < 2.0 ** 15).all()) and bool((bound / inv >= 2.0 ** 14 * 0.999).all())
    whole = torch.zeros(R, 224, device='cuda')
    ops.split_columns_scaled(x, 0, C, whole, inv)
    grown = torch.zeros(R, 224, device='cuda')
    panel = torch.zeros(R, C, device='cuda')
    for c0, c1 in ((0, 13), (13, 14), (14, 100), (100, 200)):   # ragged pieces: groups are re-converted from the panel
        panel[:, c0:c1] = x[:, c0:c1]
        g0 = c0 // 8 * 8
        ops.split_columns_scaled(panel, g0, c1 - g0, grown, inv)
    assert torch.equal(whole, grown)
    assert bool((whole[:, 200:] == 0).all())
    back = unsplit(whole, inv, C)
    err = (back.double() - x.double()).abs() / x.abs().amax(1, keepdim=True).double()
    assert float(err.max()) < 2.0 ** -20                      # 1000x loose bound: still far below fp32 rounding of a dot product
    lib_err = None
    try:
        ops.split_columns_scaled(x, 4, 8, whole, inv)
    except ValueError as e:
        lib_err = str(e)
    assert lib_err and 'multiple of 8' in lib_err


def test_abs_reduce_row_maxima_and_infinity_norm():
    from tfep_amd import ops
    torch.manual_seed(5)
    x = torch.randn(301, 1237, device='cuda') * torch.logspace(-4, 4, 301, device='cuda')[:, None]
    assert torch.equal(ops.abs_reduce(x, 'row_max'), x.abs().amax(dim=1))
    got = ops.abs_reduce(x, 'max_row_sum')
    ref = x.double().abs().sum(dim=1).max()
    assert got.shape == (1,) and abs(float(got) - float(ref)) <= 1e-5 * float(ref)
    view = x[:, 100:300]                                         # strided rows
    assert torch.equal(ops.abs_reduce(view, 'row_max'), view.abs().amax(dim=1))
    assert float(ops.abs_reduce(torch.zeros(1, 0, device='cuda'), 'max_row_sum')) == 0.0


@pytest.mark.parametrize('order', ['ascending', 'descending', 'random'])
def test_weight_prepare_without_reading_a_prefix_mask(order):
    """Packed columns are sorted by input degree, so an autoregressive mask row is a prefix of them: the re-pack with
    ``col_cut`` (mask not read) must write exactly the bits of the re-pack that reads the mask; a mask that is not of that
    form is detected and read."""
    import os
    from tfep_amd import ops
    from tfep_amd.nn.conditioners import MADE, generate_degrees
    if os.environ.get('TFEP_MASK_PREFIX', '1') == '0':
        pytest.skip('TFEP_MASK_PREFIX=0: the prefix path is switched off')
    torch.manual_seed(1)
    D = 37
    deg = generate_degrees(D, order)
    made = MADE(deg, degrees_out=deg.repeat(2), hidden_layers=[90, 70]).cuda()
    plan = made.plan(torch.device('cuda'))
    lins = made._linears()
    n_prefix = 0
    for li, lin in enumerate(lins):
        cut = made._mask_prefix_cuts(plan, li, lin)
        n_rows = plan['n_pad'][li]
        with_mask = (torch.zeros(n_rows, plan['k_pad'][li], device='cuda'), torch.zeros(4, device='cuda'))
        ops.masked_weight_prepare_split(lin.weight_v.detach(), lin.weight_g.detach(), lin.mask, plan['row_of_out'][li],
                                        plan['in_of_col'][li], *with_mask)
        if cut is None:
            continue
        n_prefix += 1
        assert cut.dtype == torch.int32 and cut.shape == (lin.out_features,)
        assert torch.equal(cut.long(), lin.mask.sum(dim=1).long())
        no_mask = (torch.zeros(n_rows, plan['k_pad'][li], device='cuda'), torch.zeros(4, device='cuda'))
        ops.masked_weight_prepare_split(lin.weight_v.detach(), lin.weight_g.detach(), lin.mask, plan['row_of_out'][li],
                                        plan['in_of_col'][li], *no_mask, col_cut=cut)
        assert torch.equal(with_mask[0].view(torch.int32), no_mask[0].view(torch.int32))
        assert torch.equal(with_mask[1][0], no_mask[1][0])                       # the matrix scale
        # (row-L1 maximum: the prefix kernel sums a row's |w| in another order -- it only feeds a bound)
        assert torch.allclose(with_mask[1][2], no_mask[1][2], rtol=1e-5)
    assert n_prefix >= 2                                        # every layer fed by degree-sorted hidden units
    # a mask with a hole is not a prefix: detected (per mask version), and the mask is read
    lin = lins[1]
    with torch.no_grad():
        row = int(lin.mask.sum(dim=1).argmax())
        col = int(plan['in_of_col'][1][0])                      # first packed column: set in every non-empty row
        lin.mask[row, col] = 0.0
    assert made._mask_prefix_cuts(plan, 1, lin) is None
    x = torch.randn(5, D, device='cuda')
    with torch.no_grad():
        a = made(x, split=True)
        b = made(x, split=False)
    assert float((a - b).abs().max()) < 1e-5 * (float(b.abs().max()) + 1.0)


def test_elu_of_the_gemm_epilogues_is_fp32_accurate():
    """The ELU of the GEMM epilogues (gemm_common.h: expm1f on the negative branch) against float64:
    through a GEMM with an identity weight, over 30 decades of negative inputs, plus -0, -inf, NaN."""
    from tfep_amd import ops
    tm, tn, tk = ops.tile_sizes()
    n = 256
    xs = torch.cat([-torch.logspace(-30, 2, 4000, dtype=torch.float64), -torch.linspace(0, 20, 4000, dtype=torch.float64),
                    torch.tensor([-0.0, 0.5, 3.0, -float('inf'), float('nan')], dtype=torch.float64)])
    pad = (-len(xs)) % n
    xs = torch.cat([xs, torch.zeros(pad, dtype=torch.float64)])
    a = xs.float().reshape(-1, n).cuda()                                  # each row: n values, identity weight keeps them
    w = ops.masked_weight_prepare(torch.eye(n, device='cuda'), None, None, n_rows_padded=n, k_padded=n)
    bias = torch.zeros(n, device='cuda')
    y32 = ops.masked_linear_packed(a, w, bias, n, act=1)                 # exact-fp32 MFMA kernel, ELU epilogue
    as_, ainv = ops.split_rows(a, n)
    ws_, winv = ops.split_rows(w, n, per_tensor=True)
    ys = ops.masked_linear_split(as_, ainv, ws_, winv, bias, n, act=1)   # split kernel, same epilogue code
    ref = torch.where(a.double() > 0, a.double(), torch.expm1(a.double()))
    for y in (y32, ys):
        finite = torch.isfinite(ref) & torch.isfinite(a)
        rows_ok = torch.isfinite(a).all(dim=1)                           # the NaN / inf row pollutes its own GEMM row only
        m = finite & rows_ok[:, None] & (ref != 0)
        rel = ((y.double() - ref).abs() / ref.abs())[m]
        assert float(rel.max()) < 2.5e-7
        assert bool((y[(ref == 0) & rows_ok[:, None]] == 0).all())
    assert torch.isnan(y32[~rows_ok]).any()                              # NaN in -> NaN out (not -1)


@pytest.mark.parametrize('weight_norm', [True, False])
@pytest.mark.parametrize('K', [8192, 9001, 14998])
def test_fp32_prefix_pack_writes_the_bits_of_the_masked_pack(K, weight_norm):
    """``tfep_masked_weight_prepare_prefix`` (row staged in LDS, mask not read, only the live prefix written) against
    ``tfep_masked_weight_prepare`` reading the mask: identical bits everywhere, for permuted rows and columns, a fully
    masked row, rows whose prefix ends inside a group of 8 and a full row; the masked suffix stays the zeros of the
    allocation; misuse is rejected."""
    import ctypes
    from tfep_amd import _lib, ops
    torch.manual_seed(K)
    N = 77
    g_ = torch.Generator(device='cuda').manual_seed(K + 1)
    v = torch.randn(N, K, device='cuda', generator=g_)
    wg = (torch.rand(N, 1, device='cuda', generator=g_) + 0.5) if weight_norm else None
    in_of_col = torch.randperm(K, device='cuda', generator=g_).to(torch.int32)          # packed column -> input feature
    col_of_in = torch.empty(K, dtype=torch.int32, device='cuda')
    col_of_in[in_of_col.long()] = torch.arange(K, dtype=torch.int32, device='cuda')
    row_of_out = torch.randperm(N + 3, device='cuda', generator=g_)[:N].to(torch.int32)
    cut = torch.randint(0, K + 1, (N,), device='cuda', generator=g_).to(torch.int32)
    cut[0], cut[1], cut[2], cut[3] = 0, K, 13, K - 5
    mask = (col_of_in[None, :].long() < cut[:, None].long()).float()                    # mask[o, i] = packed column of i < cut[o]
    k_pad = ops.round_up(K, ops.tile_sizes()[2])
    ref = ops.masked_weight_prepare(v, wg, mask, row_of_out, col_of_in, N + 3, k_pad)
    out = torch.zeros(N + 3, k_pad, device='cuda')
    got = ops.masked_weight_prepare(v, wg, None, row_of_out, col_of_in, N + 3, k_pad, out=out, col_cut=cut, clear=False,
                                    in_of_col=in_of_col)
    assert got is out and torch.equal(out.view(torch.int32), ref.view(torch.int32))
    again = ops.masked_weight_prepare(v, wg, None, row_of_out, col_of_in, N + 3, k_pad, out=out, col_cut=cut, clear=False,
                                      in_of_col=in_of_col)
    assert torch.equal(again.view(torch.int32), ref.view(torch.int32))
    lib = _lib.load()
    args = (_lib.ptr(v), _lib.ptr(wg), N, K, _lib.ptr(row_of_out), _lib.ptr(in_of_col), _lib.ptr(cut))
    assert lib.tfep_masked_weight_prepare_prefix(*args, _lib.ptr(out), N + 3, k_pad, None) == 0
    assert lib.tfep_masked_weight_prepare_prefix(*args[:6], None, _lib.ptr(out), N + 3, k_pad, None) != 0       # no col_cut
    assert lib.tfep_masked_weight_prepare_prefix(*args, _lib.ptr(out), N - 1, k_pad, None) != 0                 # too few rows
    assert lib.tfep_masked_weight_prepare_prefix(*args, _lib.ptr(out), N + 3, K - 8, None) != 0                 # rows too short
    torch.cuda.synchronize()


def test_transpose_split_equals_split_of_the_transpose():
    """``tfep_transpose_split`` (one pass, the per-tensor scale taken from the split of the matrix itself) writes the bits
    of ``tfep_transpose`` followed by ``tfep_split_rows(per_tensor)``; ragged tiles, a padded row stride; misuse rejected."""
    from tfep_amd import _lib, ops
    torch.manual_seed(4)
    R, C, ld = 224, 333, 352                      # R a multiple of 32 (split rows); C and the strides not multiples of the 64 x 64 tile
    src = torch.zeros(R, ld, device='cuda')
    src[:, :C] = torch.randn(R, C, device='cuda') * torch.logspace(-3, 2, C, device='cuda')
    ws, w_inv = ops.split_rows(src[:, :C], ld, per_tensor=True)
    wt = ops.transpose(src, R, C, torch.zeros(C, R, device='cuda'))
    ref, ref_inv = ops.split_rows(wt, R, per_tensor=True)
    assert float(ref_inv[0]) == float(w_inv[0])
    out = torch.full((C, R), 7.0, device='cuda')
    lib = _lib.load()
    assert lib.tfep_transpose_split(_lib.ptr(src), ld, R, C, _lib.ptr(out), R, R, 0, _lib.ptr(w_inv), None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    # mode 1: the per-tensor scale computed on the way
    out1, inv1 = torch.full((C, R), 7.0, device='cuda'), torch.zeros(2, device='cuda')
    assert lib.tfep_transpose_split(_lib.ptr(src), ld, R, C, _lib.ptr(out1), R, R, 1, None, _lib.ptr(inv1), None) == 0
    assert torch.equal(out1.view(torch.int32), ref.view(torch.int32)) and float(inv1[0]) == float(ref_inv[0])
    # mode 2: one scale per output row from the column maxima of the same pass as the column sums; fewer valid rows than the
    # padded width (rows past R read as zero)
    Rv, Rp = 203, 224
    sums, cmax = torch.zeros(C, device='cuda'), torch.empty(C, device='cuda')
    assert lib.tfep_column_sums_absmax(_lib.ptr(src), ld, Rv, C, _lib.ptr(sums), 1, _lib.ptr(cmax), None) == 0
    assert torch.equal(cmax, src[:Rv, :C].abs().amax(dim=0))
    assert torch.allclose(sums, src[:Rv, :C].double().sum(dim=0).float(), rtol=1e-6, atol=1e-6)
    wt2 = ops.transpose(src, Rv, C, torch.zeros(C, Rp, device='cuda'))
    ref2, ref2_inv = ops.split_rows(wt2, Rp)
    out2, inv2 = torch.full((C, Rp), 7.0, device='cuda'), torch.zeros(C, device='cuda')
    assert lib.tfep_transpose_split(_lib.ptr(src), ld, Rv, C, _lib.ptr(out2), Rp, Rp, 2, _lib.ptr(cmax), _lib.ptr(inv2), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out2.view(torch.int32), ref2.view(torch.int32)) and torch.equal(inv2, ref2_inv)
    # misuse
    assert lib.tfep_transpose_split(_lib.ptr(src), ld, R, C, _lib.ptr(out), R, R - 4, 0, _lib.ptr(w_inv), None, None) != 0   # R_pad < R
    assert lib.tfep_transpose_split(_lib.ptr(src), ld, R, C, _lib.ptr(out), R - 8, R, 0, _lib.ptr(w_inv), None, None) != 0   # rows too short
    assert lib.tfep_transpose_split(_lib.ptr(src), ld, R, C, _lib.ptr(out), R, R, 0, None, None, None) != 0
    assert lib.tfep_transpose_split(_lib.ptr(src), ld, R, C, _lib.ptr(out), R, R, 3, _lib.ptr(w_inv), None, None) != 0


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(1, 1), (7, 5), (513, 1024), (4100, 1030), (33, 4099)])
def test_column_absmax_matches_torch(shape):
    """``tfep_column_absmax`` (the per-feature magnitudes of the split-path guard): equal to torch's, on aligned and
    unaligned rows / row strides; a NaN in a column survives (the guard then routes the batch to the exact kernels)."""
    import torch
    from tfep_amd import ops
    torch.manual_seed(3)
    R, C = shape
    x = torch.randn(R, C, device='cuda') * torch.logspace(-6, 3, C, device='cuda')
    assert torch.equal(ops.column_absmax(x)[0], x.abs().amax(dim=0))
    big = torch.randn(R, C + 3, device='cuda')
    view = big[:, 1:C + 1]                              # row stride C + 3, rows start 4 bytes off the 16-byte grid
    assert torch.equal(ops.column_absmax(view)[0], view.abs().amax(dim=0))
    x[R // 2, C // 2] = float('nan')
    out = ops.column_absmax(x)[0]
    assert bool(torch.isnan(out[C // 2])) and int(torch.isnan(out).sum()) == 1
    assert ops.column_absmax(torch.empty(0, 5, device='cuda')).tolist() == [[0.0] * 5]


def _split_desc(a, w, out, tile_n=0, tile_list=None, tile_live=None, accumulate=0, k_split=1):
    """``tfep_masked_linear_gemm`` on split operands made here (rows of ``a`` per row, ``w`` per tensor)."""
    import ctypes
    from tfep_amd import _lib, ops
    asp, a_inv = ops.split_rows(a, a.shape[1])
    wsp, w_inv = ops.split_rows(w, w.shape[1], per_tensor=True)
    d = _lib.GemmDesc()
    d.split, d.x_inv_scale, d.w_inv_scale = 1, a_inv.data_ptr(), w_inv.data_ptr()
    d.x, d.ldx, d.w, d.ldw = asp.data_ptr(), asp.shape[1], wsp.data_ptr(), wsp.shape[1]
    d.y, d.ldy = out.data_ptr(), out.shape[-1]
    d.B, d.N, d.n_rows_w, d.k_padded, d.act, d.accumulate = a.shape[0], w.shape[0], w.shape[0], w.shape[1], 0, accumulate
    d.tile_n = tile_n
    if tile_list is not None:
        d.tile_list, d.n_tile_list = tile_list.data_ptr(), tile_list.shape[0]
    if tile_live is not None:
        d.tile_live = tile_live.data_ptr()
    if k_split > 1:
        d.k_split, d.slab_stride = k_split, out.shape[-2] * out.shape[-1]
    _lib.call('tfep_masked_linear_gemm', ctypes.byref(d), _lib.stream_of(a))
    return out


@pytest.mark.parametrize('B,K,N', [(700, 1024, 1000), (257, 96, 401), (1, 32, 3), (513, 2048, 400)])
def test_wide_linear_tile_matches_float64_and_the_default_tile(B, K, N):
    """The 400-column tile of the plain linear product (``tile_n = tfep_split_wide_tile_n()``, the training step's GEMMs):
    the same sums as the 256-column tile, so the same bits; fp32-accurate against float64; split-K slabs add up."""
    from tfep_amd import ops
    torch.manual_seed(B + N)
    tw = ops.split_wide_tile_n()
    assert tw == 400
    a = torch.randn(B, K, device='cuda')
    w = torch.randn(N, K, device='cuda') / K ** 0.5
    ref = a.double() @ w.double().T
    y256 = _split_desc(a, w, torch.empty(B, N, device='cuda'))
    y400 = _split_desc(a, w, torch.empty(B, N, device='cuda'), tile_n=tw)
    assert torch.equal(y256, y400)
    assert float((y400.double() - ref).abs().max()) < 2e-6 * float(ref.abs().max()) * max(1.0, K / 1024)
    if K >= 1024:
        slabs = _split_desc(a, w, torch.empty(2, B, N, device='cuda'), tile_n=tw, k_split=2)
        assert float((slabs.sum(dim=0).double() - ref).abs().max()) < 2e-6 * float(ref.abs().max()) * max(1.0, K / 1024)


@pytest.mark.parametrize('tile_n', [0, 400])
def test_tile_list_launches_exactly_the_listed_tiles(tile_n):
    """``tile_list``: the live tiles of a block-sparse product in an order that gives every XCD the same share
    (``ops.xcd_balanced_tile_list``).  Listed tiles hold the product (first pass: written, second pass with ``accumulate``:
    doubled), all other tiles are not touched."""
    from tfep_amd import ops
    torch.manual_seed(7)
    tm = ops.tile_sizes()[0]
    tn = tile_n or ops.tile_sizes()[1]
    B, K, N = 5 * tm + 37, 256, 3 * tn + 11
    M_t, N_t = (B + tm - 1) // tm, (N + tn - 1) // tn
    live = torch.rand(M_t, N_t) < 0.5
    live[0, 0], live[-1, -1] = True, False
    tl = ops.xcd_balanced_tile_list(live)
    listed = tl[tl[:, 0] >= 0]
    assert tl.shape[0] % 256 == 0 and listed.shape[0] == int(live.sum())
    assert {tuple(t) for t in listed.tolist()} == {tuple(t) for t in torch.nonzero(live).tolist()}
    per_xcd = [int((tl[x::8, 0] >= 0).sum()) for x in range(8)]
    assert max(per_xcd) - min(per_xcd) <= 32                    # whole groups of 32, dealt round-robin
    a = torch.randn(B, K, device='cuda')
    w = torch.randn(N, K, device='cuda') / K ** 0.5
    ref = (a.double() @ w.double().T).float()
    out = torch.full((B, N), 123.0, device='cuda')
    _split_desc(a, w, out, tile_n=tile_n, tile_list=tl.cuda())
    mask = live.cuda().repeat_interleave(tm, 0)[:B].repeat_interleave(tn, 1)[:, :N]
    assert bool((out[~mask] == 123.0).all())
    assert float((out[mask] - ref[mask]).abs().max()) < 1e-5
    _split_desc(a, w, out, tile_n=tile_n, tile_list=tl.cuda(), accumulate=1)
    assert bool((out[~mask] == 123.0).all())
    assert float((out[mask] - 2 * ref[mask]).abs().max()) < 2e-5


def test_tile_list_on_the_exact_fp32_kernel():
    """The same launch list drives the exact-fp32 kernel (a guarded training step takes it): listed tiles written, the
    others untouched."""
    import ctypes
    from tfep_amd import _lib, ops
    torch.manual_seed(9)
    tm, tn, tk = ops.tile_sizes()
    B, K, N = 3 * tm + 5, 8 * tk, 2 * tn + 9
    live = torch.tensor([[True, False, True], [False, True, False], [True, True, False], [False, False, True]])
    tl = ops.xcd_balanced_tile_list(live).cuda()
    a = torch.randn(B, K, device='cuda')
    w = torch.randn(N, K, device='cuda') / K ** 0.5
    wp = ops.masked_weight_prepare(w, None, None, n_rows_padded=ops.round_up(N, tk), k_padded=K)
    out = torch.full((B, N), -7.0, device='cuda')
    d = _lib.GemmDesc()
    d.x, d.ldx, d.w, d.ldw = a.data_ptr(), K, wp.data_ptr(), K
    d.y, d.ldy = out.data_ptr(), N
    d.B, d.N, d.n_rows_w, d.k_padded, d.act, d.accumulate = B, N, wp.shape[0], K, 0, 0
    d.tile_list, d.n_tile_list = tl.data_ptr(), tl.shape[0]
    _lib.call('tfep_masked_linear_gemm', ctypes.byref(d), _lib.stream_of(a))
    mask = live.cuda().repeat_interleave(tm, 0)[:B].repeat_interleave(tn, 1)[:, :N]
    ref = (a.double() @ w.double().T).float()
    assert bool((out[~mask] == -7.0).all())
    assert float((out[mask] - ref[mask]).abs().max()) < 1e-4


@pytest.mark.parametrize('R,C', [(64, 64), (8, 32), (200, 96), (1000, 320), (96, 4128)])
def test_transpose_of_split_rows_moves_the_halves(R, C):
    """``tfep_transpose_split_rows``: the transpose of a split matrix with one scale, made from its fp16 halves -- bit for
    bit the split rows of the transposed matrix at that scale."""
    from tfep_amd import _lib, ops
    torch.manual_seed(R + C)
    w = torch.randn(R, C, device='cuda') * torch.logspace(-3, 2, C, device='cuda')
    ws, inv = ops.split_rows(w, C, per_tensor=True)
    out = torch.full((C, R), float('nan'), device='cuda')
    _lib.call('tfep_transpose_split_rows', _lib.ptr(ws), C, R, C, _lib.ptr(out), R, _lib.stream_of(ws))
    ref = torch.empty(C, R, device='cuda')
    _lib.call('tfep_transpose_split', _lib.ptr(w), C, R, C, _lib.ptr(ref), R, R, 0, _lib.ptr(inv), None, _lib.stream_of(w))
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    assert float((unsplit(out, inv, R) - w.t()).abs().max()) <= 2.0 ** -21 * float(w.abs().max())


@pytest.mark.parametrize('layout', ['plain', 'circular', 'learn_both', 'five_bins'])
def test_fused_forward_and_training_step_repeat_bit_for_bit(layout):
    """The same call twice gives the same bits, forward (fused split kernel) and training step (saving forward + backward).
    The matrix-core products of these kernels are inline asm whose result latency the compiler does not know: a spill store or
    a merge copy placed ahead of the hand-written wait once read accumulators before the matrix pipe had written them --
    results off by ~1e-7 on a few rows, different from run to run (tools/scan_hazards.sh scans the listings)."""
    from tfep_amd.loss import BoltzmannKLDivLoss
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    torch.manual_seed(21)
    D, B = 70, 900
    kw = dict(plain={}, circular=dict(circular=True), learn_both=dict(learn_lower_bound=True, learn_upper_bound=True), five_bins={})[layout]
    lo, hi = (0.0, 2.0) if layout == 'circular' else (-4.0, 4.0)
    maf = MAF(generate_degrees(D, 'ascending'), transformer=NeuralSplineTransformer(torch.full((D,), lo), torch.full((D,), hi),
                                                                                   5 if layout == 'five_bins' else 8, **kw),
              hidden_layers=[150, 130], initialize_identity=False).cuda()
    maf.split_gemm, maf.fused = True, True
    x0 = (torch.rand(B, D, device='cuda') * (hi - lo) + lo) * 0.98
    c = torch.linspace(0.1, 0.4, D, device='cuda')
    with torch.no_grad():
        outs = [maf(x0) for _ in range(4)]
    for y, l in outs[1:]:
        assert torch.equal(y, outs[0][0]) and torch.equal(l, outs[0][1])

    def step():
        for p in maf.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        y, l = maf(x)
        BoltzmannKLDivLoss()((c * y ** 2).sum(dim=1), l).backward()
        return [y.detach(), l.detach(), x.grad] + [p.grad.clone() for p in maf.parameters()]
    first = step()
    for _ in range(2):
        for a, b in zip(first, step()):
            assert torch.equal(a, b)


@pytest.mark.parametrize('weight_norm', [True, False])
def test_one_pass_pack_of_both_weight_forms_equals_the_two_packs(weight_norm):
    """``MADE._pack_layer_both`` (``tfep_masked_weight_prepare_split_both``: the blocked inverse's fp32 and split packs of a
    layer from one read of the parameters): bit for bit the packs of ``_pack_layer`` and ``_pack_layer_split``."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import AffineTransformer
    torch.manual_seed(12)
    D = 24
    maf = MAF(generate_degrees(D, 'ascending'), transformer=AffineTransformer(), hidden_layers=[64, 8300], weight_norm=weight_norm,
              initialize_identity=False).cuda()
    made = maf._conditioner
    dev = torch.device('cuda', torch.cuda.current_device())
    plan = made.plan(dev)
    lins = made._linears()
    li, lin = 2, lins[2]                                    # 48 output rows of 8300 weights each
    assert lin.in_features == 8300
    with torch.no_grad():
        w32, b32 = made._pack_layer(plan, li, lin)
        w32, b32 = w32.clone(), b32.clone()
        ws, winv, bs, bmax = made._pack_layer_split(plan, li, lin)
        ws, winv, bs = ws.clone(), winv.clone(), bs.clone()
        made.invalidate_plan()
        plan = made.plan(dev)
        with made.frozen_weights():
            assert made._pack_layer_both(plan, li, lin)
            w32b, b32b = made._pack_layer(plan, li, lin)             # served from what the one pass left
            wsb, winvb, bsb, _ = made._pack_layer_split(plan, li, lin)
            assert torch.equal(w32b, w32) and torch.equal(b32b, b32)
            assert torch.equal(wsb.view(torch.int32), ws.view(torch.int32)) and torch.equal(winvb[0], winv[0]) and torch.equal(bsb, bs)
            assert float(winvb[2]) == float(winv[2])                  # the row-L1 bound of the split pack
        assert made._pack_layer_both(plan, 1, lins[1]) is False      # 64-weight rows: the two methods pack on their own
