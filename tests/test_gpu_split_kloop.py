"""GPU tests of the split GEMM's k-loop schedule (csrc/split_gemm_kernel.h: the slot table that places one companion
instruction -- a B-fragment read or half of an LDS-DMA piece -- after every MFMA).  A wrongly placed wait or DMA does not
fault: it shows as wrong rows, or as rows that differ from run to run.  So every case is checked against float64 computed
from the un-split fp32 operands, with the tolerance of tests/test_gpu_split_gemm.py (1e-6 = 4.2 x 2^-22 of (row maximum)
x sum_k |w_jk| per output), and is run twice with the two results compared bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-6          # tests/test_gpu_split_gemm.py: error <= 1e-6 x (row maximum) x sum_k |w_jk|


def unsplit(s, inv, cols):
    """Rebuild fp32 values from split rows (host-side check only)."""
    R = s.shape[0]
    raw = s.view(torch.float16).reshape(R, -1, 2, 8).float()          # (rows, k-groups, hi/lo, 8)
    v = (raw[:, :, 0] + raw[:, :, 1]).reshape(R, -1)[:, :cols]
    return v * inv.reshape(-1, 1)


def _elu64(v):
    return torch.where(v > 0, v, torch.expm1(v))


def _operands(B, K, N, seed):
    from tfep_amd import ops
    tk = ops.tile_sizes()[2]
    g = torch.Generator(device='cuda').manual_seed(seed)
    kp, npad = ops.round_up(K, tk), ops.round_up(N, tk)
    a = torch.randn(B, K, device='cuda', generator=g)
    w = torch.randn(N, K, device='cuda', generator=g) / K ** 0.5
    bias = torch.zeros(npad, device='cuda')
    bias[:N] = torch.randn(N, device='cuda', generator=g)
    as_, ainv = ops.split_rows(ops.pad_columns(a, kp), kp)
    wp = ops.masked_weight_prepare(w, None, None, n_rows_padded=npad, k_padded=kp)
    ws_, winv = ops.split_rows(wp, kp, per_tensor=True)
    return a, w, bias, as_, ainv, ws_, winv


def _row_scale(a, w):
    """(row maximum of the activations) x sum_k |w_jk|, in float64: what the split format's error is relative to."""
    return a.double().abs().amax(dim=1, keepdim=True) * w.double().abs().sum(dim=1)[None, :]


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('K', [32, 64, 96, 128, 160])
def test_every_k_tile_count_and_stage_parity(K, act):
    """nk = 1 (the last-tile instantiation alone), 2 (one tile with DMA), then both parities of the weight stage with three
    and more tiles; one row, a ragged and a second row tile; one ragged, two, and ragged-last column tiles."""
    from tfep_amd import ops
    for B in (1, 255, 257):
        for N in (17, 272, 400, 416):
            a, w, bias, as_, ainv, ws_, winv = _operands(B, K, N, 1000 * K + 10 * B + N)
            ref = a.double() @ w.double().T + bias[:N].double()
            if act:
                ref = _elu64(ref)
            y = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, act=act)
            y2 = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, act=act)
            err = float(((y.double() - ref).abs() / _row_scale(a, w)).max())
            assert err <= TOL, (B, K, N, act, err)
            assert torch.equal(y, y2), (B, K, N, act)


@pytest.mark.parametrize('K,N', [(96, 288), (64, 32)])
def test_direct_split_output(K, N):
    """``split_out``: the ELU epilogue that writes split rows (what the headline's hidden layers run), un-split here."""
    from tfep_amd import ops
    B = 257
    g = torch.Generator(device='cuda').manual_seed(K + N)
    x = torch.randn(B, K, device='cuda', generator=g) * torch.logspace(-2, 2, B, device='cuda')[:, None]
    w = torch.randn(N, K, device='cuda', generator=g) / K ** 0.5
    wg = torch.rand(N, 1, device='cuda', generator=g) + 0.5
    bias = torch.randn(N, device='cuda', generator=g)
    ws = torch.zeros(N, K, device='cuda')
    w_buf = torch.zeros(4, device='cuda')
    ops.masked_weight_prepare_split(w, wg, None, None, None, ws, w_buf)
    w_eff = (wg * w / w.norm(dim=1, keepdim=True)).double()
    xs, x_inv = ops.split_rows(x, K)
    hs, h_inv = ops.masked_linear_split(xs, x_inv, ws, w_buf, bias, N, act=1, split_out=True)
    hs2, h_inv2 = ops.masked_linear_split(xs, x_inv, ws, w_buf, bias, N, act=1, split_out=True)
    ref = _elu64(x.double() @ w_eff.T + bias.double())
    # the rows leave at a scale set by the bound max(1, row maximum x max_j sum_k |w_jk| + max |b|): test_gpu_split_gemm's scale
    scale = x.double().abs() @ w_eff.abs().T + bias.double().abs() + 1.0
    err = float(((unsplit(hs, h_inv, N).double() - ref).abs() / scale).max())
    assert err <= TOL, err
    assert torch.equal(hs.view(torch.int32), hs2.view(torch.int32)) and torch.equal(h_inv, h_inv2)


def test_k_ranges_empty_single_tile_and_full():
    """Three column tiles in a permuted launch order: an empty k-range (no k-tile: bias only), one k-tile that starts past
    k = 0, and the whole K."""
    from tfep_amd import ops
    tm, tn, tk = ops.tile_sizes()
    B, K, N = 300, 160, 3 * tn
    a, w, bias, as_, ainv, ws_, winv = _operands(B, K, N, 7)
    kr = torch.tensor([[0, 0], [2 * tk, 3 * tk], [0, K]], dtype=torch.int32, device='cuda')
    order = torch.tensor([2, 0, 1], dtype=torch.int32, device='cuda')
    y = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, k_ranges=kr, tile_order=order)
    y2 = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, k_ranges=kr, tile_order=order)
    ref = torch.empty(B, N, dtype=torch.float64, device='cuda')
    for t, (kb, ke) in enumerate(kr.tolist()):
        c = slice(t * tn, (t + 1) * tn)
        ref[:, c] = a[:, kb:ke].double() @ w[c, kb:ke].double().T + bias[c].double()
    err = float(((y.double() - ref).abs() / _row_scale(a, w)).max())
    assert err <= TOL, err
    assert torch.equal(y[:, :tn], bias[:tn].expand(B, tn))            # the empty range: exactly the bias
    assert torch.equal(y, y2)


@pytest.mark.parametrize('S', [2, 3])
def test_split_k_slabs(S):
    """``k_split``: the linear epilogue on the narrow tiles the inverse uses; five k-tiles dealt over 2 or 3 slices."""
    from tfep_amd import ops
    B, K, N = 257, 160, 90
    a, w, bias, as_, ainv, ws_, winv = _operands(B, K, N, 11 + S)
    slabs = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, k_split=S)
    slabs2 = ops.masked_linear_split(as_, ainv, ws_, winv, bias, N, k_split=S)
    assert slabs.shape == (S, B, N)
    ref = a.double() @ w.double().T + bias[:N].double()
    err = float(((slabs.double().sum(0) - ref).abs() / _row_scale(a, w)).max())
    assert err <= TOL, err
    assert torch.equal(slabs, slabs2)


def test_fused_spline_tile_of_25_parameters():
    """One MAF layer with an 8-bin spline (P = 25): D = 40 is three 16-feature column tiles of the fused kernel, the last one
    ragged; two hidden layers of 96; 300 rows.  Split kernels against the exact-fp32 kernels and the float64 oracle, with
    the bounds tests/test_gpu_parity.py applies to layers with identical weights; twice, bit for bit."""
    from oracle import flows as oflows, made as omade
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    D, B = 40, 300
    torch.manual_seed(40)
    layer = MAF(generate_degrees(D, 'ascending'), transformer=NeuralSplineTransformer(torch.full((D,), -5.0), torch.full((D,), 5.0), 8),
                hidden_layers=[96, 96], initialize_identity=False)
    x = torch.randn(B, D, generator=torch.Generator().manual_seed(41)).clamp_(-4.9, 4.9)

    def oracle(dtype):
        sd = {k: (v.numpy().astype(dtype) if v.dtype == torch.float32 else v.numpy()) for k, v in layer.state_dict().items()}
        ol = [dict(degrees_in=omade.generate_degrees(D, 'ascending'),
                   transformer=dict(type='spline', x0=np.full(D, -5.0, dtype), xf=np.full(D, 5.0, dtype), n_bins=8),
                   embedding=None, made=omade.made_layers_from_state(sd, prefix='_conditioner.'))]
        y, l = oflows.sequential_forward(x.numpy().astype(dtype), ol)
        return np.asarray(y, dtype=np.float64), np.asarray(l, dtype=np.float64)
    y64, l64 = oracle(np.float64)
    _, l32 = oracle(np.float32)
    noise_l = float(np.abs(l32 - l64).max())
    layer = layer.cuda()
    xg = x.cuda()
    with torch.no_grad():
        layer.split_gemm, layer.fused = True, True
        assert layer._fused_kind() == 1
        ys, ls = layer(xg)
        ys2, ls2 = layer(xg)
        layer.split_gemm = False
        ye, le = layer(xg)
    assert torch.equal(ys, ys2) and torch.equal(ls, ls2)
    # against the same layer on the exact-fp32 kernels (test_cfg2_four_layer_composition's bounds)
    assert float((ye - ys).norm() / ye.norm()) < 2e-6
    assert float((le - ls).abs().max()) < 1e-5 * max(1.0, float(le.abs().max())) + 2e-4
    # against float64 (the module's tolerances: rel L2 1e-5; log-det 1e-5 max(1, |ldj|), floor 4 x the fp32 oracle's own error)
    rel = np.linalg.norm(ys.cpu().numpy() - y64) / np.linalg.norm(y64)
    assert rel <= 1e-5, rel
    tol_l = np.maximum(1e-5 * np.maximum(1.0, np.abs(l64)), 4.0 * noise_l)
    err_l = np.abs(ls.cpu().numpy().astype(np.float64) - l64)
    assert bool((err_l <= tol_l).all()), (float(err_l.max()), float(tol_l.min()))
