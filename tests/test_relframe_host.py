"""CPU tests of the relative-frame layer: the plain reference of tests/relframe_ref.py against the reference's results in
tests/golden/relframe.npz, the conditions the seeds of its cases meet, its own round trip, the host side of
``CartesianToMixedFlow`` (layout, index lists, validation), the normalisation helpers, the C ABI symbols, and the per-row
arithmetic of csrc/relframe.h compiled for the host under the address and undefined-behaviour sanitizers.  No kernel is
launched."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import relframe_ref as rr
import zmatrix_ref as zr
from tfep_amd import _lib
from tfep_amd.nn.flows import CartesianToMixedFlow
from tfep_amd.utils import geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
SYMBOLS = [f'tfep_relative_frame_{name}{sfx}' for name in ('encode', 'encode_backward', 'decode', 'decode_backward')
           for sfx in ('', '_f64')]


class _Identity(torch.nn.Module):
    def forward(self, x):
        return x, torch.zeros(len(x), dtype=x.dtype, device=x.device)

    inverse = forward


# ------------------------------------------------------------------ the reference against the golden file

def test_reference_reproduces_the_golden_file():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'relframe.npz'))
    x, pi_row = torch.from_numpy(g['x']), int(g['pi_row'])
    assert (x[pi_row, -2] - x[pi_row, -3]).tolist() == [-2.0, 0.0, 0.0]
    coords, origin, R, ldj = rr.encode(x, (False, False, False))
    n_o = x.shape[1] - 3
    v = np.concatenate([coords[:, 3:3 + 3 * n_o].reshape(len(x), n_o, 3).numpy(), coords[:, -6:-3].reshape(-1, 1, 3).numpy()], 1)
    a102 = 2.0 * math.pi * coords[:, 2].numpy() - math.pi
    figures = {
        'R': np.abs(R.numpy() - g['R']).max(),
        'v (other atoms, origin)': np.abs(v - g['v'][:, :-2]).max(),
        'd01': np.abs(coords[:, 0].numpy() - g['v'][:, -2, 0]).max(),
        'axis y, z / plane z': max(np.abs(coords[:, -3:-1].numpy() - g['v'][:, -2, 1:]).max(),
                                   np.abs(coords[:, -1].numpy() - g['v'][:, -1, 2]).max()),
        'd02': np.abs(coords[:, 1].numpy() - g['d02']).max(),
        'a102': np.abs(a102 - g['a102']).max(),
        'log_det_J': np.abs(ldj.numpy() + rr.LOG_TWO_PI - g['log_det_polar']).max(),
    }
    x_back, ldj_back = rr.decode(coords, origin, R, (False, False, False))
    figures['x back'] = np.abs(x_back.numpy() - g['x_back']).max()
    figures['log_det_J back'] = np.abs(ldj_back.numpy() - rr.LOG_TWO_PI - g['log_det_polar_back']).max()
    a = 2.0 * math.pi * coords[:, 2] - math.pi
    figures['polar x, y'] = max(np.abs((coords[:, 1] * torch.cos(a)).numpy() - g['polar_x']).max(),
                                np.abs((coords[:, 1] * torch.sin(a)).numpy() - g['polar_y']).max())
    for k, err in figures.items():
        print(f'{k}: max abs {err:.3e}')
        assert err <= 1e-12, k
    assert np.abs(R[pi_row].numpy() - g['R'][pi_row]).max() <= 1e-12 and abs(float(R[pi_row, 0, 0]) + 1.0) <= 4e-16


# ------------------------------------------------------------------ the cases

@pytest.mark.parametrize('name', rr.CASES)
def test_cases_meet_their_conditions(name):
    c = rr.case(name)
    assert c['x_cart'].shape == (rr.B, {'refs_only': 3, 'wide': 70, 'mixed': 9}[name], 3) and rr.B == 6
    one_plus_c, length, d02, a102, c_min = rr.conditions(c['x_cart'])
    print(f"{name}: seed {c['seed']}, min 1 + c = {one_plus_c:.3f}, min |a - o| = {length:.3f}, min d02 = {d02:.3f}, "
          f"max |a102| = {a102:.3f}, min c = {c_min:.3f}")
    assert one_plus_c >= rr.MIN_ONE_PLUS_C == 0.05
    assert length >= rr.MIN_LENGTH == 0.5 and d02 >= 0.5
    assert a102 <= rr.MAX_ABS_A102 == math.pi - 0.1
    assert c_min < rr.SOME_C_BELOW == -0.2
    if name == 'mixed':
        low = zr.min_reference_sine(c['x'], c['z_matrix'])
        print(f'mixed: min sin(x_j, x_k, x_l) = {low:.4f}')
        assert low >= zr.MIN_SINE
        assert torch.equal(c['x'][:, c['ordered']], c['x_cart'])
        # the reference atoms are no prefix of the Cartesian atoms, not next to each other and not in order
        position = [c['cartesian'].tolist().index(i) for i in c['reference'].tolist()]
        assert position == [6, 1, 4] and sorted(c['cartesian'].tolist()) == c['cartesian'].tolist()
        assert sorted(c['cartesian'].tolist() + c['z_matrix'][:, 0].tolist()) == list(range(69))
    many = rr.many_case()
    assert many.shape == (4099, 5, 3)
    pi = rr.pi_case()
    assert torch.equal(pi.to(torch.float32).to(F64), pi)


@pytest.mark.parametrize('remove', rr.REMOVES)
def test_reference_round_trip(remove):
    c = rr.case('mixed')
    coords, origin, R, ldj = rr.encode(c['x_cart'], remove)
    assert coords.shape == (rr.B, rr.width(9, remove))
    x_back, ldj_back = rr.decode(coords, origin, R, remove)
    err, err_l = float((x_back - c['x_cart']).abs().max()), float((ldj + ldj_back).abs().max())
    print(f'{remove}: max |decode(encode(x)) - x| = {err:.3e}, max |log-det sum| = {err_l:.3e}')
    assert err <= 1e-12 and err_l <= 1e-12
    if remove == (True, True, True):
        y, ldj_in, origin, R = rr.to_mixed(c['x'], c['z_matrix'], c['ordered'], remove)
        assert y.shape == (rr.B, 3 * 69 - 6)
        x_back, ldj_out = rr.from_mixed(y, origin, R, c['z_matrix'], c['ordered'], remove)
        err, err_l = float((x_back - c['x']).abs().max()), float((ldj_in + ldj_out).abs().max())
        print(f'whole change: max |x back - x| = {err:.3e}, max |log-det sum| = {err_l:.3e}')
        assert err <= 1e-10 and err_l <= 1e-10
        assert float(y[:, 60:180].min()) >= 0.0 and float(y[:, 60:180].max()) <= 1.0 and 0.0 <= float(y[:, 182].min())


# ------------------------------------------------------------------ the module's host side

# 7 atoms: 2 in internal coordinates (atoms 2 and 5), 5 Cartesian (0, 1, 3, 4, 6); reference atoms origin 4, axis 0, plane 3
Z_MATRIX = [[2, 0, 1, 3], [5, 2, 0, 1]]
CARTESIAN = [0, 1, 3, 4, 6]
REFERENCE = [4, 0, 3]


def _flow(remove, z_matrix=Z_MATRIX, cartesian=CARTESIAN, reference=REFERENCE):
    return CartesianToMixedFlow(_Identity(), cartesian, z_matrix, reference, remove)


def test_layout_and_properties():
    flow = _flow([True, True, True])
    assert flow.cartesian_atom_indices.tolist() == [1, 6, 4, 0, 3]
    assert flow.z_matrix.tolist() == Z_MATRIX and flow.n_ic_atoms == 2
    assert flow.remove_ref_rototranslation.tolist() == [True, True, True]
    assert 'remove_ref_rototranslation' in dict(flow.named_buffers())
    assert flow.n_dofs_out == 3 * 7 - 6 == 15
    assert _flow([False, False, False]).n_dofs_out == 21
    assert isinstance(flow.n_dofs_out, int)


@pytest.mark.parametrize('remove, n_dofs, reference', [
    ([True, False, False], 18, [15, 16, 17]),            # axis y, z and plane z are kept
    ([False, True, False], 19, [15, 16, 17, 18]),        # origin x, y, z and plane z
    ([False, False, True], 20, [15, 16, 17, 18, 19]),    # origin x, y, z and axis y, z
])
def test_dof_indices_by_type(remove, n_dofs, reference):
    """Mixed layout: bonds 0-1, angles 2-3, torsions 4-5, d01 6, d02 7, a102 8, atom 1 at 9-11, atom 6 at 12-14, then the
    kept reference DOFs.  Conditioning atoms: 6 (Cartesian) and 3 (the plane atom: d02 and a102)."""
    flow = _flow(remove)
    assert flow.n_dofs_out == n_dofs
    by_type = flow.get_dof_indices_by_type(conditioning_atom_indices=torch.tensor([6, 3]))
    expected = {'distances': [0, 1, 6, 7], 'angles': [2, 3, 8], 'torsions': [4, 5], 'd01': [6], 'd02': [7], 'a102': [8],
                'cartesians': [9, 10, 11, 12, 13, 14], 'reference': reference, 'conditioning': [7, 8, 12, 13, 14]}
    assert set(by_type) == set(expected)
    for k, v in expected.items():
        assert by_type[k].tolist() == v, k
    none = flow.get_dof_indices_by_type()
    assert none['conditioning'] is None and none['cartesians'].tolist() == expected['cartesians']
    assert flow.get_dof_indices_by_type(torch.tensor([0]))['conditioning'].tolist() == [6]          # the axis atom: d01
    assert flow.get_dof_indices_by_type(torch.tensor([4]))['conditioning'] is None                  # the origin: nothing
    all_removed = _flow([True, True, True]).get_dof_indices_by_type()
    assert all_removed['reference'].tolist() == [] and all_removed['reference'].dtype == torch.int64


@pytest.mark.parametrize('kwargs, match', [
    (dict(reference=[4, 0, 0]), 'three distinct'),
    (dict(reference=[4, 0]), 'three distinct'),
    (dict(reference=[4, 0, 2]), 'must be Cartesian atoms'),
    (dict(cartesian=[0, 1, 3, 4, 7]), 'exactly once'),                           # atom 6 is nowhere
    (dict(cartesian=[0, 1, 2, 3, 4, 6]), 'exactly once'),                        # atom 2 is Cartesian and placed
    (dict(z_matrix=[[2, 0, 1, 3], [5, 2, 0, 0]]), 'distinct'),                   # (ops.check_zmatrix)
    (dict(z_matrix=[[2, 5, 1, 3], [5, 2, 0, 1]]), 'cycle'),
    (dict(remove=[True, True]), '3 flags'),
])
def test_constructor_validation(kwargs, match):
    args = dict(remove=[True, True, True])
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        _flow(**args)


def test_normalisation_helpers():
    torch.manual_seed(0)
    for dtype in (torch.float32, F64):
        a = torch.rand(4, 7, dtype=dtype) * math.pi
        t = (torch.rand(4, 7, dtype=dtype) * 2.0 - 1.0) * math.pi
        for fn, inv, value, ref, log_scale in (
                (geometry.normalize_angles, geometry.unnormalize_angles, a, a / math.pi, -math.log(math.pi)),
                (geometry.normalize_torsions, geometry.unnormalize_torsions, t, (t + math.pi) / (2 * math.pi),
                 -math.log(2 * math.pi))):
            out, ldj = fn(value)
            assert out.dtype == dtype and ldj.dtype == dtype and ldj.shape == (4,)
            assert torch.allclose(out, ref, rtol=0, atol=1e-6 if dtype == torch.float32 else 1e-15)
            assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
            assert torch.allclose(ldj, torch.full((4,), 7 * log_scale, dtype=dtype))
            back, ldj_back = inv(out)
            assert torch.allclose(back, value, rtol=0, atol=1e-5 if dtype == torch.float32 else 1e-14)
            assert torch.allclose(ldj + ldj_back, torch.zeros(4, dtype=dtype), atol=1e-6)
    out, ldj = geometry.normalize_torsions(torch.tensor([[-math.pi, 0.0, math.pi]], dtype=F64))
    assert out.tolist() == [[0.0, 0.5, 1.0]]


def test_public_functions_validate_on_the_host():
    with pytest.raises(ValueError, match='n_c >= 3'):
        geometry.cartesian_to_relative_frame(torch.zeros(2, 2, 3), [True, True, True])
    with pytest.raises(ValueError, match='3 flags'):
        geometry.cartesian_to_relative_frame(torch.zeros(2, 3, 3), [True, True])
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        geometry.cartesian_to_relative_frame(torch.zeros(2, 3, 3), [True, True, True])
    from tfep_amd import ops
    assert [ops.relative_frame_width(5, r) for r in rr.REMOVES] == [rr.width(5, r) for r in rr.REMOVES]
    assert ops.relative_frame_width(3, (True, True, True)) == 3 and ops.relative_frame_width(3, (False, False, False)) == 9


# ------------------------------------------------------------------ the C ABI and the ops

def test_symbols_are_bound_and_declared():
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    declared = set(re.findall(r'\b(tfep_[a-z0-9_]+)\s*\(', header))
    assert len(SYMBOLS) == 8
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(_lib.load(), name), name
    for name in SYMBOLS[::2]:
        assert _lib._SIGNATURES[name] == _lib._SIGNATURES[name + '_f64']
    from tfep_amd.build import SOURCES
    assert 'relframe.hip' in SOURCES


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    fake = 1 << 12                     # a non-NULL pointer that is never dereferenced: every call fails before a launch
    for sfx in ('', '_f64'):
        enc = getattr(lib, 'tfep_relative_frame_encode' + sfx)
        dec = getattr(lib, 'tfep_relative_frame_decode' + sfx)
        assert enc(fake, 15, 5, 1, 1, 1, fake, 9, fake, fake, fake, 0, None) == 0            # B = 0: nothing to do
        for args, message in (((fake, 6, 2, 1, 1, 1, fake, 9, fake, fake, fake, 4, None), 'n_c=2'),
                              ((fake, 14, 5, 1, 1, 1, fake, 9, fake, fake, fake, 4, None), 'row stride'),
                              ((fake, 15, 5, 1, 1, 0, fake, 9, fake, fake, fake, 4, None), 'row stride'),
                              ((fake, 15, 5, 1, 1, 1, fake, 9, None, fake, fake, 4, None), 'non-NULL'),
                              ((fake, 15, 5, 1, 1, 1, fake, 9, fake, fake, fake, -1, None), 'negative')):
            assert enc(*args) == -1 and message in lib.tfep_last_error().decode(), (message, lib.tfep_last_error())
        assert dec(fake, 9, fake, fake, 5, 1, 1, 1, fake, 14, fake, 4, None) == -1
        assert 'row stride' in lib.tfep_last_error().decode()


def test_ops_are_registered_and_their_fakes_keep_the_dtype():
    from tfep_amd import torch_ops
    assert torch_ops.RELATIVE_FRAME_OPS == ('relative_frame_encode', 'relative_frame_decode',
                                            'relative_frame_encode_backward', 'relative_frame_decode_backward')
    t = torch.ops.tfep
    for dtype in (torch.float32, F64):
        m = lambda *shape: torch.empty(*shape, device='meta', dtype=dtype)
        coords, origin, R, ldj = t.relative_frame_encode(m(7, 15), True, False, True)
        assert [tuple(v.shape) for v in (coords, origin, R, ldj)] == [(7, 11), (7, 3), (7, 9), (7,)]
        assert all(v.dtype == dtype for v in (coords, origin, R, ldj))
        x, ldj = t.relative_frame_decode(coords, origin, R, True, False, True)
        assert tuple(x.shape) == (7, 15) and tuple(ldj.shape) == (7,) and x.dtype == dtype
        assert tuple(t.relative_frame_encode_backward(m(7, 15), True, False, True, coords, origin, R, ldj).shape) == (7, 15)
        grads = t.relative_frame_decode_backward(coords, origin, R, True, False, True, x, ldj)
        assert [tuple(g.shape) for g in grads] == [(7, 11), (7, 3), (7, 9)]


# ------------------------------------------------------------------ csrc/relframe.h on the host

def test_row_arithmetic_and_its_vjps_on_the_host_under_sanitizers(tmp_path):
    """csrc/relframe.h is __host__ __device__: tools/relframe_host_check.cpp, built for the host alone with
    -fsanitize=address,undefined, runs the functions the kernels call and checks the hand-written VJPs of encode and decode
    against central differences in fp64, at the bound of tools/frames_host_check.cpp."""
    from tfep_amd.build import _hipcc
    try:
        compiler = _hipcc()
        subprocess.run([compiler, '--version'], check=True, capture_output=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError) as e:
        pytest.skip(f'no host compiler: {e}')
    exe = str(tmp_path / 'relframe_host_check')
    subprocess.run([compiler, '-std=c++17', '--cuda-host-only', '-x', 'hip', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', os.path.join(ROOT, 'tools', 'relframe_host_check.cpp'), '-o', exe],
                   check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    print(done.stdout, done.stderr)
    assert done.returncode == 0, done.stdout + done.stderr
    worst = float(re.search(r'worst \|vjp - central difference\| / \(1 \+ \|vjp\|\) = ([0-9.e+-]+)', done.stdout).group(1))
    assert worst <= 1e-6
