"""CPU tests of FlipInvariantEmbedding's kernel route: the C ABI declarations and argument checks, the registered ops,
the routing rules of the module (CPU tensors keep the torch code), the size limits, the float64 acceptance rules of a layer,
and the golden file.  No kernel is launched."""
import os
import re

import numpy as np
import pytest
import torch

from tfep_amd.nn.conditioners import generate_degrees
from tfep_amd.nn.embeddings import FlipInvariantEmbedding, MAFEmbedding, MixedEmbedding, PeriodicEmbedding
from tfep_amd.nn.flows import MAF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'flipembed.npz')
SYMBOLS = ('tfep_flip_invariant_embedding', 'tfep_flip_invariant_embedding_f64', 'tfep_flip_invariant_embedding_backward',
           'tfep_flip_invariant_embedding_backward_f64', 'tfep_flip_invariant_embedding_backward_workspace_bytes')
OPS = ('flip_invariant_embedding', 'flip_invariant_embedding_backward')
FAKE = 1 << 12           # a non-NULL pointer that is never dereferenced: the checks below fail before any launch


def test_built_library_exports_the_five_symbols_and_the_header_declares_them():
    from tfep_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    declared = set(re.findall(r'\b(tfep_[a-z0-9_]+)\s*\(', header))
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in declared and s in _lib.EXPORTED_SYMBOLS, s


def _forward_args(n_emb=8, n_non=2, d=4, H=32, E=3, B=5, x=FAKE, params=FAKE, out=FAKE, eidx=FAKE, nidx=FAKE):
    return (x, 10, eidx, n_emb, nidx, n_non, d, H, E, *([params] * 8), out, n_non + n_emb // max(d, 1) * E, B, None)


def _backward_args(n_emb=8, n_non=2, d=4, H=32, E=3, B=5, grads=FAKE, ws=FAKE):
    return (FAKE, 10, FAKE, n_emb, FAKE, n_non, d, H, E, *([FAKE] * 8), FAKE, 16, FAKE, 10, *([grads] * 8), 0, ws, B, None)


def test_entry_points_check_their_arguments_before_any_launch():
    from tfep_amd import _lib
    lib = _lib.load()

    def refused(message, name, args):
        for sfx in ('', '_f64'):
            assert getattr(lib, name + sfx)(*args) == -1, (name + sfx, message)
            assert message in lib.tfep_last_error().decode(), (lib.tfep_last_error().decode(), message)
    fwd, bwd = 'tfep_flip_invariant_embedding', 'tfep_flip_invariant_embedding_backward'
    for name, make in ((fwd, _forward_args), (bwd, _backward_args)):
        refused('vector_dim=9 unsupported', name, make(n_emb=9, d=9))
        refused('vector_dim=0 unsupported', name, make(n_emb=0, d=0))
        refused('hidden=65 unsupported', name, make(H=65))
        refused('emb_dim=33 unsupported', name, make(E=33))
        refused('not a multiple of vector_dim', name, make(n_emb=6))
        refused('negative size', name, make(B=-1))
        for sfx in ('', '_f64'):
            assert getattr(lib, name + sfx)(*make(B=0)) == 0                     # B = 0: nothing to do
            # the limits themselves are accepted (B = 0: no launch)
            assert getattr(lib, name + sfx)(*make(n_emb=16, d=8, H=64, E=32, B=0)) == 0
    refused('x/out must be non-NULL', fwd, _forward_args(x=None))
    refused('x/out must be non-NULL', fwd, _forward_args(out=None))
    refused('embedded_indices is NULL', fwd, _forward_args(eidx=None))
    refused('nonembedded_indices is NULL', fwd, _forward_args(nidx=None))
    refused('a parameter pointer is NULL', fwd, _forward_args(params=None))
    refused('a gradient pointer is NULL', bwd, _backward_args(grads=None))
    refused('workspace is NULL', bwd, _backward_args(ws=None))
    # the workspace: one row of the staged parameter image per workgroup, at most 2048 workgroups; 8 bytes per value
    size = lib.tfep_flip_invariant_embedding_backward_workspace_bytes
    d, H, E = 4, 32, 8
    row = (H * (2 * d + 3 + 8) + 8 + 1) * 8
    assert size(1, 4, d, H, E) == row
    assert size(257, 4, d, H, E) == row                      # 257 items, 4 per lane: one workgroup
    assert size(1025, 4, d, H, E) == 2 * row
    assert size(131072, 256, d, H, E) == 2048 * row
    assert size(0, 4, d, H, E) == row
    assert size(3, 16, 8, 64, 32) == (64 * (2 * 8 + 3 + 32) + 32 + 1) * 8
    assert size(3, 16, 8, 65, 32) < 0 and size(3, 6, 4, 32, 8) < 0 and size(-1, 4, 4, 32, 8) < 0


def test_ops_are_registered_in_their_own_tuple():
    from tfep_amd import torch_ops
    assert torch_ops.FLIP_EMBEDDING_OPS == OPS
    assert torch_ops.OPS == (
        'affine_forward', 'affine_inverse', 'affine_backward', 'spline_forward', 'spline_inverse', 'spline_backward',
        'moebius_forward', 'moebius_inverse', 'moebius_backward', 'masked_linear', 'masked_linear_backward',
        'fused_output_transformer', 'fused_output_transformer_', 'tfep_reduce')
    for name in OPS:
        assert name not in torch_ops.OPS and hasattr(torch.ops.tfep, name), name
    # shapes through the fake implementations (meta tensors: nothing runs)
    def m(*shape, dtype=torch.float32):
        return torch.empty(*shape, device='meta', dtype=dtype)
    params = (m(16, 4), m(16), m(5, 16), m(5), m(16, 4), m(16), m(1, 16), m(1))
    x, eidx, nidx = m(7, 14), m(12, dtype=torch.int32), m(2, dtype=torch.int32)
    out = torch.ops.tfep.flip_invariant_embedding(x, eidx, nidx, 4, *params)
    assert out.shape == (7, 2 + 3 * 5)
    res = torch.ops.tfep.flip_invariant_embedding_backward(x, eidx, nidx, 4, *params, out)
    assert len(res) == 9 and res[0].shape == x.shape and [r.shape for r in res[1:]] == [p.shape for p in params]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_cpu_tensors_keep_the_torch_route_unchanged(dtype):
    torch.manual_seed(1)
    emb = FlipInvariantEmbedding(n_features_in=11, embedding_dimension=3, embedded_indices=[1, 2, 3, 4, 6, 7, 8, 9])
    assert emb.last_route is None
    x = torch.randn(6, 11)
    assert emb.half().takes_kernel_route(x.half()) is False         # (routing only: nothing runs in float16 here)
    emb, x = emb.to(dtype), x.to(dtype)
    assert emb.takes_kernel_route(x) is False
    out = emb(x)
    assert emb.last_route == 'torch' and torch.equal(out, emb.torch_forward(x))
    flipped = x.clone()
    flipped[:, emb._embedded_indices] = -flipped[:, emb._embedded_indices]
    assert torch.equal(emb(flipped), out)                            # the torch route is flip invariant bit for bit
    # constructor, buffers and state_dict keys as before
    assert sorted(emb.state_dict()) == sorted(
        ['_embedded_indices', '_nonembedded_indices'] + [f'{net}.{i}.{p}' for net in ('embedding_layer', 'weight_layer')
                                                          for i in (0, 2) for p in ('weight', 'bias')])
    assert [n for n, _ in emb.named_buffers()] == ['_embedded_indices', '_nonembedded_indices']


def test_limits_predicate_and_parameter_order():
    from tfep_amd import ops
    assert ops.flip_embedding_supported(8, 64, 32) and ops.flip_embedding_supported(1, 1, 1)
    assert not ops.flip_embedding_supported(9, 64, 32)
    assert not ops.flip_embedding_supported(8, 65, 32)
    assert not ops.flip_embedding_supported(8, 64, 33)
    assert not ops.flip_embedding_supported(0, 1, 1)
    assert FlipInvariantEmbedding(8, 3).within_kernel_limits()
    assert FlipInvariantEmbedding(16, 32, vector_dimension=8, hidden_layer_width=64).within_kernel_limits()
    assert not FlipInvariantEmbedding(8, 3, hidden_layer_width=65).within_kernel_limits()
    assert not FlipInvariantEmbedding(8, 33).within_kernel_limits()
    assert not FlipInvariantEmbedding(9, 3, vector_dimension=9).within_kernel_limits()
    emb = FlipInvariantEmbedding(8, 3)
    named = dict(emb.named_parameters())
    order = ['embedding_layer.0.weight', 'embedding_layer.0.bias', 'embedding_layer.2.weight', 'embedding_layer.2.bias',
             'weight_layer.0.weight', 'weight_layer.0.bias', 'weight_layer.2.weight', 'weight_layer.2.bias']
    assert [p is named[k] for p, k in zip(emb.network_parameters(), order)] == [True] * 8
    assert list(named) == order                                     # the order the layer backward hands gradients out in
    # the int32 device tables are cached per device and dropped by .to() / load_state_dict
    a = emb.device_indices('cpu')
    assert a[0].dtype == torch.int32 and emb.device_indices('cpu') is a
    assert torch.equal(a[0].long(), emb._embedded_indices) and torch.equal(a[1].long(), emb._nonembedded_indices)
    emb.double()
    assert emb._i32 == {}
    emb.device_indices('cpu')
    emb.load_state_dict(emb.state_dict())
    assert emb._i32 == {}


def test_float64_layers_accept_the_embeddings_with_float64_kernels():
    """``_check_float64`` up to the device check: a CPU tensor fails there (TfepHipError), which is AFTER the dtype rules;
    the embedding rule itself is ``_float64_embedding``."""
    from tfep_amd.nn.flows.autoregressive import _float64_embedding

    class Identity(MAFEmbedding):
        def forward(self, x):
            return x

        def get_degrees_out(self, degrees_in):
            return degrees_in

    flip = FlipInvariantEmbedding(8, 3)
    per = PeriodicEmbedding(2, [0.0, 1.0])
    assert _float64_embedding(flip) and _float64_embedding(per)
    assert _float64_embedding(MixedEmbedding(10, [per, FlipInvariantEmbedding(8, 3)], [[0, 1], list(range(2, 10))]))
    assert not _float64_embedding(Identity())
    assert not _float64_embedding(MixedEmbedding(10, [per, Identity()], [[0, 1], [2, 3]]))

    class Sub(FlipInvariantEmbedding):       # a subclass may have changed the map: not accepted
        pass
    assert not _float64_embedding(Sub(8, 3))
    # the inverse of a layer with this embedding stays the pass per degree, in both dtypes
    layer = MAF(generate_degrees(8, 'ascending', repeats=4), embedding=FlipInvariantEmbedding(8, 3))
    assert layer._blocked_ok() is False
    layer = layer.double()
    assert layer.is_float64 and layer._blocked_f64_ok() is False


def test_golden_holds_data_only_and_is_small():
    g = np.load(GOLDEN, allow_pickle=False)
    assert os.path.getsize(GOLDEN) < 200 * 1024
    shapes = {'q257': (257, 4, 3), 'strided': (5, 14, 17), 'max': (3, 16, 64), 'min': (1, 3, 3)}
    for name, (B, D, n_out) in shapes.items():
        assert g[f'{name}/x'].shape == (B, D) and g[f'{name}/x'].dtype == np.float32
        assert g[f'{name}/out'].shape == (B, n_out) and g[f'{name}/out'].dtype == np.float64
        assert g[f'{name}/gx'].shape == (B, D)
        assert sum(k.startswith(f'{name}/gp/') for k in g.files) == 8
    for k in g.files:
        assert g[k].dtype.kind in 'fiu', k
        assert g[k].dtype.kind != 'f' or np.isfinite(g[k]).all(), k
    assert g['strided/sd/_nonembedded_indices'].tolist() == [7, 12]
    assert g['q257/sd/_nonembedded_indices'].size == 0
    # the module on the CPU (its torch route, float64) reproduces the reference's output
    emb = FlipInvariantEmbedding(n_features_in=14, embedding_dimension=5, vector_dimension=4, hidden_layer_width=16,
                                 embedded_indices=[2, 3, 4, 5, 8, 9, 10, 11, 13, 0, 1, 6])
    emb.load_state_dict({k[len('strided/sd/'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('strided/sd/')})
    out = emb.double()(torch.from_numpy(g['strided/x']).double())
    np.testing.assert_allclose(out.detach().numpy(), g['strided/out'], rtol=1e-12, atol=1e-14)
