"""GPU tests of the float64 masked linear path: the fp64-MFMA GEMM (``tfep_masked_linear_gemm_f64``) and its helpers,
``masked_linear`` / ``MaskedLinear`` / ``MaskedLinearFunc`` in float64 against the reference's float64 goldens, and the
dtype contract (float64 parameters take float64 inputs; mixed dtypes are a TypeError).

Tolerances: the goldens were computed by the reference in float64 from the stored (float32-rounded) inputs and weights,
and this path differs from it only in summation order, so outputs are pinned at rel L2 <= 1e-12 and gradients within
1e-10 of max |ref| per tensor.  The GEMM unit tests use small integers, whose products and sums are exact in float64:
they are compared exactly (a wrong accumulator-row map would move results to other rows)."""
import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

F64 = torch.float64


def dev(a, dtype=F64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def rel(got, ref):
    return gu.err_stats(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, ref)[0]


def grad_err(got, ref):
    """max |got - ref| over max |ref| (the per-tensor gradient measure)."""
    got = got.detach().cpu().double().numpy()
    ref = np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _ints(*shape, lo=-3, hi=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).double()


def _gemm(x, w, bias=None, k_ranges=None, act=0, accumulate=0, elu_grad_of=None, out=None):
    """Run the fp64 GEMM on host operands: pads, packs and returns the (B, N) result on the host."""
    from tfep_amd import ops
    tk = ops.tile_sizes()[2]
    B, K = x.shape
    N = w.shape[0]
    kp = ops.round_up(K, tk)
    xp = ops.zeros(max(B, 1), kp, dtype=F64, device='cuda')[:B]
    xp[:, :K] = x.cuda()
    wp = ops.zeros(N, kp, dtype=F64, device='cuda')
    wp[:, :K] = w.cuda()
    y = ops.masked_linear_f64(xp, wp, None if bias is None else bias.cuda(), N, k_ranges=k_ranges, act=act,
                              accumulate=accumulate, elu_grad_of=None if elu_grad_of is None else elu_grad_of.cuda(),
                              out=None if out is None else out.cuda())
    torch.cuda.synchronize()
    return y.cpu()


# ------------------------------------------------------------------ 1. the fp64 GEMM

@pytest.mark.parametrize('B', [0, 1, 3, 257])
@pytest.mark.parametrize('K,N', [(5, 7), (33, 129), (130, 300)])
def test_gemm_f64_exact_integers(B, K, N):
    x, w = _ints(B, K, seed=B + K), _ints(N, K, seed=N)
    y = _gemm(x, w)
    assert y.shape == (B, N) and y.dtype == F64
    assert torch.equal(y, x @ w.T)


def test_gemm_f64_exact_integers_every_row_and_column():
    """Distinct values per row and column (x[b, k] = b + 1 on k == 0 only, w[n, 0] = n + 1): y[b, n] = (b + 1)(n + 1)
    tells every output's position apart."""
    B, K, N = 200, 16, 150
    x = torch.zeros(B, K, dtype=F64)
    x[:, 0] = torch.arange(1, B + 1, dtype=F64)
    w = torch.zeros(N, K, dtype=F64)
    w[:, 0] = torch.arange(1, N + 1, dtype=F64)
    y = _gemm(x, w)
    assert torch.equal(y, torch.outer(torch.arange(1, B + 1, dtype=F64), torch.arange(1, N + 1, dtype=F64)))


def test_gemm_f64_masked_weight_k_ranges():
    """A block-triangular mask (degree-sorted MADE rows) with per-256-row k-ranges: the skipped k-tiles hold only zeros,
    the result is the dense product exactly."""
    from tfep_amd import ops
    from tfep_amd.nn.masked import create_autoregressive_mask
    tm, tn, tk = ops.tile_sizes()
    K, N, B = 700, 600, 300
    deg_in = torch.sort(torch.arange(K) % 350).values
    deg_out = torch.sort(torch.arange(N) % 350).values
    mask = create_autoregressive_mask(deg_in, deg_out, strictly_less=False, transpose=True, dtype=F64)     # (N, K)
    assert mask.shape == (N, K)
    x, v = _ints(B, K, seed=11), _ints(N, K, seed=12)
    kp, n_pad = ops.round_up(K, tk), ops.round_up(N, tk)
    n_tiles = (n_pad + tn - 1) // tn
    wp = ops.masked_weight_prepare(v.cuda(), None, mask.cuda(), n_rows_padded=n_pad, k_padded=kp)
    assert wp.dtype == F64
    kr = ops.mask_k_ranges(mask.cuda(), tn, n_tiles, kp)
    kr_h = kr.cpu()
    assert (kr_h[:, 1] - kr_h[:, 0] < kp).any(), 'the test mask should let some column tile skip k-tiles'
    xp = ops.pad_columns(x.cuda(), kp, F64)
    y = ops.masked_linear_f64(xp, wp, None, N, k_ranges=kr)
    assert torch.equal(y.cpu(), x @ (v * mask).T)


def test_masked_linear_module_skips_masked_k_tiles_exactly():
    """MaskedLinear / masked_linear in float64 with a degree-sorted mask: the module path builds the k-range tables of the
    mask and passes them to the GEMM; the result is the dense masked product, exactly on integer data."""
    from tfep_amd.nn import masked
    K, N, B = 700, 600, 65
    deg_in = torch.sort(torch.arange(K) % 350).values
    deg_out = torch.sort(torch.arange(N) % 350).values
    mask = masked.create_autoregressive_mask(deg_in, deg_out, strictly_less=False, transpose=True, dtype=F64)
    lin = masked.MaskedLinear(K, N, mask=mask).double()
    lin.weight.data = _ints(N, K, seed=21) * mask
    lin.bias.data = _ints(N, seed=22)
    x = _ints(B, K, seed=23)
    ref = x @ lin.weight.data.T + lin.bias.data
    lin = lin.cuda()
    assert torch.equal(lin(x.cuda()).cpu(), ref)
    assert torch.equal(masked.masked_linear(x.cuda(), lin.weight, lin.bias, lin.mask).cpu(), ref)


def test_gemm_f64_epilogues():
    """bias + ELU, accumulate and the elu_grad_of factor against float64 torch on the host."""
    g = torch.Generator().manual_seed(5)
    B, K, N = 97, 45, 70
    x, w = torch.randn(B, K, generator=g, dtype=F64), torch.randn(N, K, generator=g, dtype=F64)
    b = torch.randn(N, generator=g, dtype=F64)
    lin = x @ w.T + b
    y = _gemm(x, w, bias=b, act=1)
    assert rel(y, torch.nn.functional.elu(lin).numpy()) <= 1e-14
    y0 = torch.randn(B, N, generator=g, dtype=F64)
    y = _gemm(x, w, bias=b, accumulate=1, out=y0.clone())
    assert rel(y, (y0 + lin).numpy()) <= 1e-14
    h = torch.nn.functional.elu(torch.randn(B, N, generator=g, dtype=F64))
    y = _gemm(x, w, elu_grad_of=h)
    ref = (x @ w.T) * torch.where(h > 0, torch.ones_like(h), h + 1)
    assert rel(y, ref.numpy()) <= 1e-14


def test_gemm_f64_helpers():
    """transpose and column sums in float64 (the weight-norm backward: test_weight_norm_gradients_f64)."""
    from tfep_amd import ops
    g = torch.Generator().manual_seed(6)
    R, C = 70, 45
    a = torch.randn(R, C, generator=g, dtype=F64)
    out = ops.transpose(a.cuda(), R, C, ops.zeros(64, 96, dtype=F64, device='cuda'))
    assert torch.equal(out[:C, :R].cpu(), a.T) and not out[C:].any() and not out[:, R:].any()
    s = ops.column_sums(a.cuda(), R, C)
    assert rel(s, a.sum(0).numpy()) <= 1e-14


# ------------------------------------------------------------------ 2. masked linear goldens

def test_masked_linear_goldens_f64():
    from tfep_amd.nn import masked
    g = gu.load('masked_linear.npz')
    x, w, b, m = dev(g['x']), dev(g['weight']), dev(g['bias']), dev(g['mask'])
    y = masked.masked_linear(x, w, b, m)
    assert y.dtype == F64
    assert rel(y, g['y_f64']) <= 1e-12
    assert rel(masked.masked_linear(x, w, b, None), g['y_nomask_f64']) <= 1e-12
    lin = masked.masked_weight_norm(masked.MaskedLinear(8, 5, mask=torch.from_numpy(g['mask'])))
    lin.load_state_dict({'bias': torch.from_numpy(g['wn_bias']), 'weight_g': torch.from_numpy(g['wn_g']),
                         'weight_v': torch.from_numpy(g['wn_v']), 'mask': torch.from_numpy(g['mask'])})
    lin = lin.double().cuda()
    weff = lin.weight
    assert weff.dtype == F64 and torch.all(torch.isfinite(weff)) and torch.all(weff[2] == 0)
    assert rel(weff, g['wn_weight_f64']) <= 1e-12
    assert rel(lin(x), g['wn_y_f64']) <= 1e-12
    assert lin(x.reshape(2, 3, 8)).shape == (2, 3, 5)
    # back to float32: the float32 path again, as before the round trip
    lin32 = lin.float()
    assert lin32(x.float()).dtype == torch.float32


def test_masked_linear_gradients_f64():
    """grads.npz/ml through the registered autograd formula and through MaskedLinearFunc."""
    from tfep_amd.nn import masked
    g = gu.load('grads.npz')
    for fn in ('op', 'func'):
        x, w, b = (dev(g[f'ml/{k}']).requires_grad_(True) for k in ('x', 'w', 'b'))
        m, gy = dev(g['ml/mask']), dev(g['ml/gy'])
        if fn == 'op':
            y = masked.masked_linear(x, w, b, m)
        else:
            y = masked.MaskedLinearFunc.apply(x, w, b, m)
        (y * gy).sum().backward()
        assert x.grad.dtype == w.grad.dtype == b.grad.dtype == F64
        assert grad_err(x.grad, g['ml/gx']) <= 1e-10, fn
        assert grad_err(w.grad, g['ml/gw']) <= 1e-10, fn
        assert grad_err(b.grad, g['ml/gb']) <= 1e-10, fn


def test_weight_norm_gradients_f64():
    """The masked weight-norm parametrisation: gradients of v, g, bias and x against float64 autograd on the host, with
    the reference's hooks (grad_v = 0 where the mask is 0; grad_g = 0 for a fully-masked row)."""
    from tfep_amd.nn import masked
    g = gu.load('masked_linear.npz')
    mask = torch.from_numpy(g['mask']).double()
    lin = masked.masked_weight_norm(masked.MaskedLinear(8, 5, mask=mask.float()))
    lin.load_state_dict({'bias': torch.from_numpy(g['wn_bias']), 'weight_g': torch.from_numpy(g['wn_g']),
                         'weight_v': torch.from_numpy(g['wn_v']), 'mask': torch.from_numpy(g['mask'])})
    lin = lin.double().cuda()
    gen = torch.Generator().manual_seed(7)
    gy = torch.randn(6, 5, generator=gen, dtype=F64)
    x = dev(g['x']).requires_grad_(True)
    (lin(x) * gy.cuda()).sum().backward()

    v = torch.from_numpy(g['wn_v']).double().requires_grad_(True)
    gg = torch.from_numpy(g['wn_g']).double().requires_grad_(True)
    b = torch.from_numpy(g['wn_bias']).double().requires_grad_(True)
    xr = torch.from_numpy(g['x']).double().requires_grad_(True)
    live = mask.sum(1) > 0
    w = torch.where(live[:, None], mask * gg * v / v.norm(dim=1, keepdim=True), torch.zeros_like(v))
    ((xr @ w.T + b) * gy).sum().backward()
    ref_gv = torch.where(mask != 0, v.grad, torch.zeros_like(v.grad))
    ref_gg = torch.where(live[:, None], gg.grad, torch.zeros_like(gg.grad))
    assert grad_err(lin.weight_v.grad, ref_gv.numpy()) <= 1e-10
    assert grad_err(lin.weight_g.grad, ref_gg.numpy()) <= 1e-10
    assert grad_err(lin.bias.grad, b.grad.numpy()) <= 1e-10
    assert grad_err(x.grad, xr.grad.numpy()) <= 1e-10


def test_default_dtype_float64_module():
    """A MaskedLinear built under torch.set_default_dtype(torch.float64) runs float64 end to end."""
    from tfep_amd.nn import masked
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        torch.manual_seed(3)
        lin = masked.MaskedLinear(40, 300, mask=(torch.rand(300, 40) > 0.5).double()).cuda()
        x = torch.randn(33, 40, device='cuda')
        y = lin(x)
        ref = torch.nn.functional.linear(x.cpu(), (lin.weight * lin.mask).detach().cpu(), lin.bias.detach().cpu())
        assert y.dtype == F64 and rel(y, ref.numpy()) <= 1e-13
    finally:
        torch.set_default_dtype(old)


# ------------------------------------------------------------------ 8. dtype contract

def test_mixed_dtypes_raise():
    from tfep_amd.nn import masked
    lin64 = masked.MaskedLinear(6, 4).double().cuda()
    lin32 = masked.MaskedLinear(6, 4).cuda()
    x32 = torch.randn(3, 6, device='cuda')
    with pytest.raises(TypeError):
        lin64(x32)
    with pytest.raises(TypeError):
        lin32(x32.double())
    w64 = torch.randn(4, 6, device='cuda', dtype=F64)
    with pytest.raises(TypeError):
        masked.masked_linear(x32, w64)
    with pytest.raises(TypeError):
        masked.masked_linear(x32.double(), w64, torch.zeros(4, device='cuda'))        # float32 bias
    with pytest.raises(TypeError):
        masked.MaskedLinearFunc.apply(x32, w64)


def test_opcheck_float64_samples():
    import tfep_amd.torch_ops  # noqa: F401
    g = torch.Generator(device='cuda').manual_seed(0)
    B, D = 7, 6

    def r(*shape, grad=False):
        return torch.randn(*shape, device='cuda', generator=g, dtype=F64).requires_grad_(grad)
    mask = (torch.rand(5, D, device='cuda', generator=g) > 0.4).double()
    mask[2] = 0.0
    for args in ((r(B, D, grad=True), r(5, D, grad=True), r(5, grad=True), mask, r(5, 1, grad=True)),
                 (r(3, B, D, grad=True), r(5, D, grad=True), None, None, None)):
        torch.library.opcheck(torch.ops.tfep.masked_linear.default, args)
    for args in ((r(B, 5), r(B, D), r(5, D), mask, r(5, 1)), (r(B, 5), r(B, D), r(5, D), None, None)):
        torch.library.opcheck(torch.ops.tfep.masked_linear_backward.default, args)
