"""Host side of the edge geometry and pruning ops (csrc/edge_ops.hip): the incidence builder on hand-made edge lists, the
validation of edge lists, the registered ops and their fake kernels, the C ABI tables, the default routes of
``compute_edge_distances`` / ``prune_long_edges`` against an inline copy of their torch expressions, the opt-in routes'
refusal of CPU tensors, the plain reference of tests/edge_ops_ref.py against torch's autograd, and the argument checks of the
new entry points in a stand-alone program under the address and undefined-behaviour sanitizers.  No kernel is launched."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import edge_ops_ref as er
import tfep_amd.torch_ops as torch_ops
from tfep_amd import _lib, ops
from tfep_amd.nn import graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
# name -> number of arguments in include/tfep_hip.h
ARITY = {'tfep_edge_geometry': 10, 'tfep_edge_geometry_backward': 14, 'tfep_edge_prune_count': 5, 'tfep_edge_prune_compact': 7,
         'tfep_edge_prune_workspace_int64s': 1, 'tfep_edge_select_edges': 6}
TWINS = ('tfep_edge_geometry', 'tfep_edge_geometry_backward', 'tfep_edge_prune_count', 'tfep_edge_prune_compact')

TRIANGLE = [[0, 1, 1, 2, 2, 0], [1, 0, 2, 1, 0, 2]]
LISTS = {
    'a node with no edge': (4, [[0, 2], [2, 0]]),                                   # nodes 1 and 3 are isolated
    'triangle': (3, TRIANGLE),
    'duplicate edges': (3, [[0, 0, 1, 0], [1, 1, 2, 1]]),
    'pruned ragged list': (6, [[0, 0, 0, 3, 5, 5], [1, 2, 4, 4, 0, 3]]),             # node 0 kept 3 edges, node 1 none as source
    'self-loop': (2, [[0, 1, 1], [1, 1, 0]]),
    'empty': (3, [[], []]),
}


# ------------------------------------------------------------------ incidence lists

@pytest.mark.parametrize('name', list(LISTS))
@pytest.mark.parametrize('kind', ['torch', 'numpy'])
def test_incidence_lists(name, kind):
    n_nodes, edges = LISTS[name]
    edges = np.array(edges, dtype=np.int64).reshape(2, -1)
    E = edges.shape[1]
    node_ptr, incident = ops.incidence_lists(torch.from_numpy(edges) if kind == 'torch' else edges, n_nodes)
    assert node_ptr.dtype == incident.dtype == torch.int64 and node_ptr.shape == (n_nodes + 1,) and incident.shape == (2 * E,)
    node_ptr, incident = node_ptr.numpy(), incident.numpy()
    assert node_ptr[0] == 0 and node_ptr[-1] == 2 * E and (np.diff(node_ptr) >= 0).all()
    for n in range(n_nodes):
        items = incident[node_ptr[n]:node_ptr[n + 1]]
        assert (np.diff(items) > 0).all(), (n, items)                  # ascending edges, the source entry first on a tie
        for item in items:
            assert edges[item & 1, item >> 1] == n
        assert len(items) == (edges == n).sum()
    # every edge exactly once as a source (role 0) and once as a destination (role 1)
    assert sorted(incident.tolist()) == list(range(2 * E))


def test_incidence_lists_by_hand():
    node_ptr, incident = ops.incidence_lists(torch.tensor(TRIANGLE), 3)
    assert node_ptr.tolist() == [0, 4, 8, 12]
    # node 0: source of edge 0, destination of 1, destination of 4, source of 5
    assert incident.tolist() == [0, 3, 9, 10, 1, 2, 4, 7, 5, 6, 8, 11]
    node_ptr, incident = ops.incidence_lists(torch.tensor(LISTS['self-loop'][1]), 2)
    assert node_ptr.tolist() == [0, 2, 6] and incident.tolist() == [0, 5, 1, 2, 3, 4]      # the loop 1 -> 1: item 2 before 3
    isolated = ops.incidence_lists(torch.tensor(LISTS['a node with no edge'][1]), 4)[0]
    assert isolated.tolist() == [0, 2, 2, 4, 4]
    with pytest.raises(ValueError):
        ops.incidence_lists(torch.zeros(3, 4, dtype=torch.int64), 5)


def test_edge_lists_are_validated_on_the_host_and_cached():
    good = torch.tensor(TRIANGLE)
    assert ops.check_edges(good, 3) is ops.check_edges(good, 3)                      # the second call is the cached entry
    assert torch.equal(ops.check_edges(good, 3), good)
    first = graph.edge_incidence(good, 3)
    assert graph.edge_incidence(good, 3) is first                                    # built once
    good[0, 0] = 2                                                                   # an in-place write: a new version
    assert graph.edge_incidence(good, 3) is not first
    assert graph.edge_incidence(good, 3)[1].tolist() == ops.incidence_lists(good, 3)[1].tolist()
    for bad in (torch.tensor([[0, 1], [1, -1]]), torch.tensor([[0, 3], [1, 0]])):
        with pytest.raises(ValueError, match='outside'):
            ops.check_edges(bad, 3)
    for shape in ((3, 4), (2,), (2, 2, 2), (4, 2)):
        with pytest.raises(ValueError, match='shape'):
            ops.check_edges(torch.zeros(shape, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match='integer'):
        ops.check_edges(torch.zeros(2, 4), 3)
    assert ops.check_edges(torch.empty(2, 0), 1).dtype == torch.int64                # get_all_edges(batch, 1): no edge
    strided = torch.tensor(TRIANGLE + TRIANGLE)[::2]                                 # rows 0 and 2 of a (4, 6) table
    assert ops.check_edges(strided, 3).is_contiguous()
    with pytest.raises(ValueError, match='outside'):
        ops.check_edges(good, 2)                                                     # the same tensor over fewer nodes


# ------------------------------------------------------------------ ops, fake kernels, C ABI

def test_ops_are_registered_with_fake_kernels():
    assert torch_ops.EDGE_OPS == ('edge_geometry', 'edge_geometry_backward', 'edge_prune', 'edge_select')
    for name in torch_ops.EDGE_OPS:
        assert hasattr(torch.ops.tfep, name), name
    for dtype in (F32, F64):
        x = torch.empty(7, 3, dtype=dtype, device='meta')
        edges = torch.empty(2, 11, dtype=torch.int64, device='meta')
        distances, directions = torch.ops.tfep.edge_geometry(x, edges, True, False)
        assert distances.shape == (11,) and directions.shape == (11, 3) and distances.dtype == directions.dtype == dtype
        assert distances.device.type == 'meta'
        gx = torch.ops.tfep.edge_geometry_backward(x, edges, distances, None, True, False)
        assert gx.shape == (7, 3) and gx.dtype == dtype
        keep = torch.empty(5, dtype=torch.int64, device='meta')
        picked = torch.ops.tfep.edge_select(torch.empty(11, 4, 2, dtype=dtype, device='meta'), keep)
        assert picked.shape == (5, 4, 2) and picked.dtype == dtype
        assert torch.ops.tfep.edge_select(distances, keep).shape == (5,)
    # the number of kept edges depends on the data: an unbacked size under fake tensors
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import ShapeEnv
    with FakeTensorMode(shape_env=ShapeEnv()):
        keep = torch.ops.tfep.edge_prune(torch.empty(11, device='cuda'), 1.0)
        assert keep.dim() == 1 and keep.dtype == torch.int64 and keep.device.type == 'cuda'


def test_c_abi_tables():
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    sig = _lib._SIGNATURES
    names = list(ARITY) + [n + '_f64' for n in TWINS]
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS, name
        declared = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', header)
        assert declared, name
        arity = len(declared.group(1).split(','))
        assert arity == len(sig[name][1]) == ARITY[name.replace('_f64', '')], name
    for name in TWINS:
        f32, f64 = sig[name][1], sig[name + '_f64'][1]
        if 'prune' in name:                                           # r_cutoff: a float / a double
            assert f32[2] is _lib.c_float and f64[2] is _lib.c_double and f32[:2] + f32[3:] == f64[:2] + f64[3:]
        else:
            assert f32 == f64
    assert sig['tfep_edge_prune_workspace_int64s'] == (_lib.c_int64, [_lib.c_int64])
    from tfep_amd.build import SOURCES
    assert 'edge_ops.hip' in SOURCES and os.path.exists(os.path.join(ROOT, 'tfep_amd', 'csrc', 'edge_ops.hip'))


# ------------------------------------------------------------------ the default routes, the opt-in switches

def _parent_distances(x, edges, normalize_directions=False, inverse_directions=False):
    a, b = (edges[0], edges[1]) if inverse_directions else (edges[1], edges[0])
    directions = x[a] - x[b]
    distances = torch.sqrt(torch.sum(directions ** 2, dim=-1))
    if normalize_directions:
        directions = directions / distances.unsqueeze(-1)
    return distances, directions


def _parent_prune(r_cutoff, edges, distances, *args):
    keep = distances <= r_cutoff
    return (edges[:, keep], distances[keep], *[a[keep] for a in args])


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_default_routes_are_what_they_were(dtype):
    x, edges, _, g_d = er.case(257, 65, dtype)
    x = x.to(dtype)
    for normalize, inverse in er.FLAGS:
        got = graph.compute_edge_distances(x, edges, normalize, inverse)
        want = _parent_distances(x, edges, normalize, inverse)
        assert all(torch.equal(a, b) and a.dtype == dtype for a, b in zip(got, want))
        named = graph.compute_edge_distances(x, edges, normalize_directions=normalize, inverse_directions=inverse,
                                             differentiable=False)
        assert all(torch.equal(a, b) for a, b in zip(named, want))
    distances, directions = _parent_distances(x, edges)
    cutoff = float(distances.median())
    got = graph.prune_long_edges(cutoff, edges, distances, directions, g_d)
    want = _parent_prune(cutoff, edges, distances, directions, g_d)
    assert len(got) == 4 and 0 < got[1].numel() < 257
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
    assert all(torch.equal(a, b) for a, b in zip(graph.prune_long_edges(cutoff, edges, distances, kernel=False), want[:2]))
    # the default route still differentiates through torch
    xg = x.clone().requires_grad_(True)
    graph.compute_edge_distances(xg, edges)[0].sum().backward()
    assert xg.grad is not None


def test_opt_in_switches_default_to_off_and_have_no_cpu_fallback():
    assert inspect.signature(graph.compute_edge_distances).parameters['differentiable'].default is False
    kernel = inspect.signature(graph.prune_long_edges).parameters['kernel']
    assert kernel.default is False and kernel.kind is inspect.Parameter.KEYWORD_ONLY
    x, edges, _, _ = er.case(63, 65, F64)
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        graph.compute_edge_distances(x, edges, differentiable=True)
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        graph.compute_edge_distances(x.float(), edges, True, True, differentiable=True)
    distances, directions = graph.compute_edge_distances(x, edges)
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        graph.prune_long_edges(1.0, edges, distances, directions, kernel=True)
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        ops.edge_prune(distances, 1.0)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.tfep.edge_geometry(x, edges, False, False)             # the dispatcher: no kernel for CPU


# ------------------------------------------------------------------ the yardstick

@pytest.mark.parametrize('normalize,inverse', er.FLAGS)
@pytest.mark.parametrize('n_edges,n_nodes', [(1, 2), (65, 2), (257, 65)])
def test_reference_gradient_matches_autograd(n_edges, n_nodes, normalize, inverse):
    x, edges, g_r, g_d = er.case(n_edges, n_nodes, F64)
    xg = x.clone().requires_grad_(True)
    r, d = er.geometry(xg, edges, normalize, inverse)
    want_r, want_d = _parent_distances(xg, edges, normalize, inverse)
    assert torch.equal(r, want_r) and torch.equal(d, want_d)
    assert float(r.detach().min()) > er.MIN_LENGTH
    for cot_r, cot_d in ((g_r, g_d), (g_r, None), (None, g_d)):
        outputs, cots = zip(*[(o, c) for o, c in ((r, cot_r), (d, cot_d)) if c is not None])
        want, = torch.autograd.grad(outputs, xg, cots, retain_graph=True)
        got = er.geometry_vjp(x, edges, cot_r, cot_d, normalize, inverse)
        rel = er.rel_l2(got.numpy(), want.numpy())
        assert rel <= 1e-14, (rel, cot_r is None, cot_d is None)
    if n_nodes == 65:                                                   # nodes 3 and 64 have no edge
        assert bool((got[[3, 64]] == 0).all()) and int((got != 0).any(1).sum()) == 63
    assert torch.equal(edges[:, -1], edges[:, 0]) and bool((edges[0] != edges[1]).all())
    assert not x.requires_grad                                          # the shared inputs are left as they were


def test_reference_pruning_and_zero_length():
    d = torch.tensor([0.5, 2.0, float('nan'), 1.0, 0.25], dtype=F64)
    assert er.keep_index(d, 1.0).tolist() == [0, 3, 4]                  # <=: the edge at the cutoff stays, the NaN goes
    edges = torch.tensor([[0, 1, 2, 3, 4], [1, 2, 3, 4, 0]])
    kept = er.prune(1.0, edges, d, torch.arange(10.0).reshape(5, 2))
    assert kept[0].tolist() == [[0, 3, 4], [1, 4, 0]] and kept[1].tolist() == [0.5, 1.0, 0.25]
    assert kept[2].tolist() == [[0.0, 1.0], [6.0, 7.0], [8.0, 9.0]]
    # an edge of length 0: distance 0, NaN unit vector, NaN gradient on its two nodes only -- by hand and by autograd
    x = torch.tensor([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0], [1.0, 2.0, 2.0], [0.0, 1.0, 0.0]], dtype=F64, requires_grad=True)
    edges = torch.tensor([[0, 1, 3], [3, 2, 0]])
    r, u = er.geometry(x, edges, True)
    assert r.tolist() == [1.0, 0.0, 1.0] and bool(u[1].isnan().all()) and bool(u[[0, 2]].isfinite().all())
    auto, = torch.autograd.grad(r.sum(), x)
    hand = er.geometry_vjp(x.detach(), edges, torch.ones(3, dtype=F64), None, True)
    for g in (auto, hand):
        assert g.isnan().all(1).tolist() == [False, True, True, False] and bool(g[[0, 3]].isfinite().all())


# ------------------------------------------------------------------ argument checks of the entry points, under sanitizers

def test_entry_point_argument_checks_on_the_host_under_sanitizers(tmp_path):
    """tools/edge_ops_host_check.cpp, built with -fsanitize=address,undefined on its host side, calls the entry points of
    csrc/edge_ops.hip with NULL pointers, negative sizes and empty inputs: each must return its code before any launch."""
    from tfep_amd.build import _hipcc
    try:
        compiler = _hipcc()
        subprocess.run([compiler, '--version'], check=True, capture_output=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError) as e:
        pytest.skip(f'no host compiler: {e}')
    exe = str(tmp_path / 'edge_ops_host_check')
    host = [f for flag in ('-fsanitize=address,undefined', '-fno-sanitize-recover=undefined') for f in ('-Xarch_host', flag)]
    subprocess.run([compiler, '-std=c++17', '--offload-arch=gfx950', '-x', 'hip', '-g', *host,
                    os.path.join(ROOT, 'tools', 'edge_ops_host_check.cpp'), '-o', exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    print(done.stdout, done.stderr)
    assert done.returncode == 0, done.stdout + done.stderr
