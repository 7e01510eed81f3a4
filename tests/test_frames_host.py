"""Host-side checks of the frame kernels of the Cartesian wrappers (csrc/frames.hip): the C ABI, the argument checks that
run before any launch, the registered ops, and the route table of CenteredCentroidFlow / OrientedFlow.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from tfep_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = ('tfep_centroid_shift', 'tfep_centroid_restore', 'tfep_centroid_shift_backward', 'tfep_centroid_restore_backward',
         'tfep_frame_orient', 'tfep_frame_orient_backward', 'tfep_frame_rotate', 'tfep_frame_rotate_backward')
SYMBOLS = tuple(b + s for b in BASES for s in ('', '_f64'))
FAKE = 1 << 12           # a non-NULL pointer that is never dereferenced: the checks below fail before any launch


class _Identity(torch.nn.Module):
    def forward(self, x):
        return x, torch.zeros(len(x), dtype=x.dtype, device=x.device)

    inverse = forward

    def n_parameters(self):
        return 0


def _ctype(decl):
    decl = decl.strip()
    if '*' in decl:
        return ctypes.c_void_p
    return {'int64_t': ctypes.c_int64, 'int': ctypes.c_int}[decl.rsplit(' ', 1)[0].replace('const ', '').strip()]


def test_symbols_exist_with_the_signatures_of_the_header():
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS, name
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', header)
        assert m, f'{name} is not declared in tfep_hip.h'
        declared = [_ctype(a) for a in m.group(1).split(',')]
        res, bound = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and bound == declared, name
        # the element type of the twin: float pointers in the float32 entry point, double in the other
        assert ('double' in m.group(1)) == name.endswith('_f64') and ('float' in m.group(1)) != name.endswith('_f64'), name


def _shift(x=FAKE, subset=None, n_sub=0, weights=None, origin=FAKE, dim=3, n=5, shift=FAKE, y=FAKE, ld=15, B=4):
    return (x, ld, subset, n_sub, weights, origin, dim, n, shift, y, ld, B, None)


def _restore(y=FAKE, shift=FAKE, subset=None, n_sub=0, origin=FAKE, fixed=0, entry=0, dim=3, n=5, back=1, out=FAKE, ld=15, B=4):
    return (y, ld, shift, subset, n_sub, None, origin, fixed, entry, dim, n, back, out, ld, B, None)


def _shift_bwd(subset=None, n_sub=0, dim=3, n=5, gy=FAKE, gx=FAKE, ld=15, B=4):
    return (subset, n_sub, None, dim, n, gy, ld, FAKE, gx, ld, B, None)


def _restore_bwd(subset=None, n_sub=0, fixed=0, entry=0, dim=3, n=5, g=FAKE, gy=FAKE, gshift=FAKE, ld=15, B=4):
    return (subset, n_sub, None, fixed, entry, dim, n, 1, g, ld, gy, ld, gshift, B, None)


def _orient(x=FAKE, a=0, p=1, axis=0, plane=1, normal=3, y=FAKE, rot=FAKE, n=5, ld=15, B=4):
    return (x, ld, a, p, axis, plane, normal, 1, y, ld, rot, n, B, None)


def _orient_bwd(x=FAKE, a=0, p=1, axis=0, plane=1, normal=3, gy=FAKE, gx=FAKE, n=5, ld=15, B=4):
    return (x, ld, a, p, axis, plane, normal, 1, gy, ld, None, gx, ld, n, B, None)


def _rotate(x=FAKE, rot=FAKE, y=FAKE, n=5, ld=15, B=4):
    return (x, ld, rot, 0, y, ld, n, B, None)


def _rotate_bwd(x=FAKE, rot=FAKE, gy=FAKE, gx=FAKE, grot=FAKE, n=5, ld=15, B=4):
    return (x, ld, rot, 0, gy, ld, gx, ld, grot, n, B, None)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()

    def refused(message, name, args):
        for sfx in ('', '_f64'):
            assert getattr(lib, name + sfx)(*args) == -1, (name + sfx, message)
            assert message in lib.tfep_last_error().decode(), (lib.tfep_last_error().decode(), message)
    makers = {'tfep_centroid_shift': _shift, 'tfep_centroid_restore': _restore, 'tfep_centroid_shift_backward': _shift_bwd,
              'tfep_centroid_restore_backward': _restore_bwd, 'tfep_frame_orient': _orient,
              'tfep_frame_orient_backward': _orient_bwd, 'tfep_frame_rotate': _rotate, 'tfep_frame_rotate_backward': _rotate_bwd}
    for name, make in makers.items():
        refused('negative size', name, make(B=-1))
        refused('a row stride is shorter than the row', name, make(ld=14))
        for sfx in ('', '_f64'):
            assert getattr(lib, name + sfx)(*make(B=0)) == 0                     # B = 0: nothing to do, no launch
    # null pointers
    refused('must be non-NULL', 'tfep_centroid_shift', _shift(x=None))
    refused('must be non-NULL', 'tfep_centroid_shift', _shift(origin=None))
    refused('must be non-NULL', 'tfep_centroid_shift', _shift(shift=None))
    refused('must be non-NULL', 'tfep_centroid_shift', _shift(y=None))
    refused('must be non-NULL', 'tfep_centroid_restore', _restore(y=None))
    refused('must be non-NULL', 'tfep_centroid_restore', _restore(out=None))
    refused('translate_back needs the shift', 'tfep_centroid_restore', _restore(shift=None))
    refused('must be non-NULL', 'tfep_centroid_shift_backward', _shift_bwd(gy=None))
    refused('must be non-NULL', 'tfep_centroid_shift_backward', _shift_bwd(gx=None))
    refused('must be non-NULL', 'tfep_centroid_restore_backward', _restore_bwd(g=None))
    refused('must be non-NULL', 'tfep_centroid_restore_backward', _restore_bwd(gshift=None))
    refused('must be non-NULL', 'tfep_frame_orient', _orient(x=None))
    refused('must be non-NULL', 'tfep_frame_orient', _orient(rot=None))
    refused('must be non-NULL', 'tfep_frame_orient_backward', _orient_bwd(gy=None))
    refused('must be non-NULL', 'tfep_frame_rotate', _rotate(rot=None))
    refused('must be non-NULL', 'tfep_frame_rotate_backward', _rotate_bwd(grot=None))
    # dim outside 1..3
    for name, make in list(makers.items())[:4]:
        refused('dim=0 unsupported', name, make(dim=0))
        refused('dim=4 unsupported', name, make(dim=4, ld=20))
        refused('without a subset', name, make(n_sub=2))
        refused('an empty subset', name, make(subset=FAKE, n_sub=0))
    # the fixed point
    for name, make in (('tfep_centroid_restore', _restore), ('tfep_centroid_restore_backward', _restore_bwd)):
        refused('fixed_point=5 out of range', name, make(fixed=5, entry=5))
        refused('fixed_point=-1 out of range', name, make(fixed=-1))
        refused('fixed_entry=2 out of range', name, make(subset=FAKE, n_sub=2, fixed=3, entry=2))
        refused('fixed_entry must equal fixed_point', name, make(fixed=3, entry=2))
    # the frame
    for name, make in (('tfep_frame_orient', _orient), ('tfep_frame_orient_backward', _orient_bwd)):
        refused('n_points=1', name, make(n=1, a=0, p=0))
        refused('n_points=0', name, make(n=0))
        refused('axis_point=5 out of range', name, make(a=5))
        refused('axis_point=-1 out of range', name, make(a=-1))
        refused('plane_point=7 out of range', name, make(p=7))
        refused('must differ', name, make(a=2, p=2))
        refused('is not a frame', name, make(axis=3))
        refused('is not a frame', name, make(axis=1, plane=1))
        refused('is not a frame', name, make(normal=2))
        refused('is not a frame', name, make(normal=0))
        refused('is not a frame', name, make(normal=4))
        for sfx in ('', '_f64'):                        # either sign of the normal, every pair of axes (B = 0: no launch)
            for axis, plane in ((0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)):
                for sign in (1, -1):
                    assert getattr(lib, name + sfx)(*make(axis=axis, plane=plane, normal=sign * (4 - axis - plane), B=0)) == 0


def test_ops_are_registered_and_their_fakes_keep_the_dtype():
    from tfep_amd import torch_ops
    assert torch_ops.FRAME_OPS[:4] == ('centroid_shift', 'centroid_restore', 'frame_orient', 'frame_rotate')
    for name in torch_ops.FRAME_OPS:
        assert name not in torch_ops.OPS and hasattr(torch.ops.tfep, name), name
    for dtype in (torch.float32, torch.float64):
        def m(*shape, dtype=dtype):
            return torch.empty(*shape, device='meta', dtype=dtype)
        x, sub = m(7, 12), m(2, dtype=torch.int32)
        shift, y = torch.ops.tfep.centroid_shift(x, sub, m(2), m(3), 3)
        assert (shift.shape, y.shape, shift.dtype, y.dtype) == ((7, 3), (7, 12), dtype, dtype)
        out = torch.ops.tfep.centroid_restore(y, shift, sub, None, m(3), 1, 0, 3, True)
        assert out.shape == (7, 12) and out.dtype == dtype
        assert torch.ops.tfep.centroid_shift_backward(y, shift, sub, None, 3).shape == (7, 12)
        gy, gs = torch.ops.tfep.centroid_restore_backward(y, sub, None, 1, 0, 3, True)
        assert (gy.shape, gs.shape, gs.dtype) == ((7, 12), (7, 3), dtype)
        framed, rot = torch.ops.tfep.frame_orient(x, 0, 1, 0, 1, 3, True)
        assert (framed.shape, rot.shape, framed.dtype, rot.dtype) == ((7, 12), (7, 9), dtype, dtype)
        assert torch.ops.tfep.frame_rotate(framed, rot, False).dtype == dtype
        assert torch.ops.tfep.frame_orient_backward(x, framed, rot, 0, 1, 0, 1, 3, True).shape == (7, 12)
        gx, grot = torch.ops.tfep.frame_rotate_backward(x, rot, framed, False)
        assert (gx.shape, grot.shape, grot.dtype) == ((7, 12), (7, 9), dtype)


def test_route_table():
    """frame_kernels None / True / False across float32 / float64 (routing only: CPU tensors, nothing runs)."""
    from tfep_amd.nn.flows import CenteredCentroidFlow, OrientedFlow
    table = {(None, torch.float32): False, (None, torch.float64): True, (True, torch.float32): True,
             (True, torch.float64): True, (False, torch.float32): False, (False, torch.float64): False}
    flows = [CenteredCentroidFlow(_Identity(), space_dimension=3), OrientedFlow(_Identity()),
             CenteredCentroidFlow(_Identity(), space_dimension=2, subset_point_indices=[4, 1], weights=[1.0, 3.0])]
    for flow in flows:
        assert flow.frame_kernels is None and flow.last_route is None
        for (setting, dtype), kernels in table.items():
            flow.frame_kernels = setting
            assert flow.takes_kernel_route(torch.zeros(2, 12, dtype=dtype)) is kernels, (type(flow).__name__, setting, dtype)
    # what the kernels do not take runs on the torch ops whatever the setting: more than 3 dimensions, repeated indices
    for flow in (CenteredCentroidFlow(_Identity(), space_dimension=4),
                 CenteredCentroidFlow(_Identity(), space_dimension=3, subset_point_indices=[1, 2, 1])):
        for setting in (None, True):
            flow.frame_kernels = setting
            assert flow.takes_kernel_route(torch.zeros(2, 12, dtype=torch.float64)) is False
    # the frame of every (axis, plane) pair as the kernels take it: e_axis x e_plane = sign e_normal
    expected = {('x', 'xy'): (0, 1, 3), ('y', 'xy'): (1, 0, -3), ('y', 'yz'): (1, 2, 1), ('z', 'yz'): (2, 1, -1),
                ('x', 'xz'): (0, 2, -2), ('z', 'xz'): (2, 0, 2)}
    for (axis, plane), frame in expected.items():
        assert OrientedFlow(_Identity(), axis=axis, plane=plane)._frame == frame, (axis, plane)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_torch_route_runs_on_cpu_tensors_in_either_dtype(dtype, monkeypatch):
    """``frame_kernels=False`` is the code of before: it runs wherever torch runs, and records its route."""
    from tfep_amd.nn.flows import CenteredCentroidFlow, OrientedFlow
    from tfep_amd.nn.flows.partial import PartialFlow
    # (no device here: the column gather / scatter of PartialFlow is left out, the frame arithmetic is what runs)
    monkeypatch.setattr(PartialFlow, '_pass', lambda self, x, inverse: (x, torch.zeros(len(x), dtype=x.dtype)))
    torch.manual_seed(3)
    x = torch.randn(4, 15, dtype=dtype)
    for flow in (CenteredCentroidFlow(_Identity(), space_dimension=3), OrientedFlow(_Identity())):
        flow.frame_kernels = False
        y, ldj = flow(x)
        assert flow.last_route == 'torch' and y.dtype == dtype and torch.allclose(y, x, atol=1e-5)


def test_frame_rotation_and_its_vjp_on_the_host(tmp_path):
    """csrc/frames.h is __host__ __device__: tools/frames_host_check.cpp, built for the host alone, checks the rotation's
    geometry and frame_rotation_vjp against central differences for all six (axis, plane) pairs."""
    import subprocess
    from tfep_amd.build import _hipcc
    exe = str(tmp_path / 'frames_host_check')
    subprocess.run([_hipcc(), '-std=c++17', '--cuda-host-only', '-x', 'hip', os.path.join(ROOT, 'tools', 'frames_host_check.cpp'),
                    '-o', exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
