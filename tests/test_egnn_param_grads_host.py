"""Host side of the EGNN parameter gradients (csrc/egnn_param_grad.hip, ``EGNNDynamics.vjp_parameters``): the condition
the GPU bounds of ``test_gpu_egnn_param_grads.py`` rest on -- the float32 oracle's own distance from the float64 reference,
per parameter tensor -- and the parts of the interface that need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import egnn_cases as ec
import egnn_param_grad_cases as pc
from tfep_amd import _lib
from tfep_amd.nn.dynamics import EGNNDynamics


@pytest.mark.parametrize('name', ec.NAMES)
def test_oracle_gradients_are_finite_nonzero_and_float32_stays_close(name):
    g64, g32 = pc.oracle_param_grads(name), pc.oracle_param_grads(name, torch.float32)
    unused = pc.unused_names(name)
    assert len(unused) == 4
    assert set(g64) == set(pc.parameter_names(name))
    for k in pc.parameter_names(name):
        if k in unused:
            assert g64[k] is None and g32[k] is None, k
            continue
        assert np.isfinite(g64[k]).all() and np.abs(g64[k]).max() > 0.0, k
        e32 = ec.rel_l2(g32[k], g64[k])
        over = e32 > pc.FLOAT32_ORACLE_REL
        print(f'{name} {k}: float32 oracle rel L2 {e32:.2e}' + (' -- above 2.5e-6: the GPU bound is 4 x this' if over else ''))
        # 1e-5 holds for a tensor exactly while plain float32 arithmetic stays within 2.5e-6 of the reference; beyond that
        # the GPU bound takes its 4 x clause for this tensor (float32 summation order differs between hosts: the figure is
        # a property of the arithmetic, not of the kernels)
        assert pc.bound(name, k) == ((pc.NOISE_MARGIN * e32, e32) if over else (pc.REL, e32)), k


def test_kernel_backward_is_off_by_default():
    assert EGNNDynamics.kernel_backward is False
    assert ec.dynamics('n17_t1').kernel_backward is False


def test_vjp_parameters_has_no_cpu_fallback():
    c = ec.case('n17_t1')
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        ec.dynamics('n17_t1').vjp_parameters(c['t'], c['x'], c['v'])


def test_argument_structs_match_the_header():
    lib = _lib.load()
    structs = (_lib.EgnnEdgeParamGradArgs, _lib.EgnnNodeParamGradArgs, _lib.EgnnParamGradReduceArgs)
    for which, s in enumerate(structs):
        assert ctypes.sizeof(s) == lib.tfep_egnn_param_grad_struct_bytes(which), s.__name__
    assert lib.tfep_egnn_param_grad_struct_bytes(3) == -1
    # the partial sets: three / two / three padded matrices and their vectors; a grid never above the cap or the items
    for nt in (1, 2, 4):
        fp = 16 * nt
        assert [lib.tfep_egnn_param_grad_partial_entries(nt, k) for k in range(3)] == [
            3 * fp * fp + 6 * fp, 2 * fp * fp + fp, 3 * fp * fp + 2 * fp]
    assert lib.tfep_egnn_param_grad_partial_entries(3, 0) == -1 and lib.tfep_egnn_param_grad_partial_entries(1, 3) == -1
    assert lib.tfep_egnn_param_grad_workgroups(9, 2) == 2 and lib.tfep_egnn_param_grad_workgroups(1, 5) == 1
