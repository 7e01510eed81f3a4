"""CPU tests of the float64 flow host side: the float64 transformer / loss entry points are declared, bound and exported,
bad float64 spline descriptors and arguments are refused before any launch, and float64 flows keep the no-CPU-fallback
policy.  No kernel is launched (no GPU here)."""
import ctypes
import os
import re

import pytest
import torch

from tfep_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_SYMBOLS = ('tfep_affine_forward_f64', 'tfep_affine_inverse_f64', 'tfep_affine_backward_f64',
               'tfep_volume_preserving_shift_f64', 'tfep_spline_n_parameters_per_feature_f64', 'tfep_spline_forward_f64',
               'tfep_spline_inverse_f64', 'tfep_spline_backward_f64', 'tfep_periodic_embedding_f64',
               'tfep_periodic_embedding_backward_f64', 'tfep_gather_columns_f64', 'tfep_scatter_columns_f64',
               'tfep_tfep_reduce_f64')
FAKE = ctypes.c_void_p(256)                # never dereferenced: the checks fail first


def test_float64_flow_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    declared = set(re.findall(r'\b(tfep_[a-z0-9_]+)\s*\(', header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in F64_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert 'tfep_spline_desc_f64' not in declared          # a struct, not an entry point
    assert _lib.ABI_VERSION == 8


def _desc(**kw):
    d = dict(x0=FAKE.value, xf=FAKE.value, y0=FAKE.value, yf=FAKE.value, n_bins=8, circular=0, identity_boundary_slopes=0,
             learn_lower_bound=0, learn_upper_bound=0, min_bin_size=1e-4, min_slope=1e-4)
    d.update(kw)
    return _lib.SplineDescF64(*d.values())


@pytest.mark.parametrize('bad, match', [
    (dict(n_bins=0), 'n_bins'), (dict(n_bins=33), 'n_bins'),
    (dict(circular=1, learn_lower_bound=1), 'circular'),
    (dict(min_bin_size=0.0), 'minimum bin size'), (dict(min_slope=1.0), 'minimum slope'),
    (dict(x0=None), 'non-NULL')])
def test_bad_float64_spline_descriptors_raise_before_launch(bad, match):
    d = _desc(**bad)
    lay = _lib.ParamLayout(8, 4, 1)
    for fn in ('tfep_spline_forward_f64', 'tfep_spline_inverse_f64'):
        with pytest.raises(ValueError, match=match):
            _lib.call(fn, FAKE, 4, FAKE, lay, ctypes.byref(d), FAKE, 4, FAKE, 0, 2, 4, None)
    with pytest.raises(ValueError, match=match):
        _lib.call('tfep_spline_backward_f64', FAKE, 4, FAKE, lay, ctypes.byref(d), FAKE, 4, None, FAKE, lay, FAKE, 4, 2, 4,
                  None)
    assert _lib.load().tfep_spline_n_parameters_per_feature_f64(ctypes.byref(d)) == -1


def test_float64_spline_parameter_counts():
    lib = _lib.load()
    for kw, n in ((dict(), 25), (dict(circular=1), 25), (dict(identity_boundary_slopes=1), 23),
                  (dict(identity_boundary_slopes=1, circular=1), 24), (dict(learn_lower_bound=1, learn_upper_bound=1), 27)):
        assert lib.tfep_spline_n_parameters_per_feature_f64(ctypes.byref(_desc(**kw))) == n, kw


def test_float64_argument_errors_before_launch():
    lay = _lib.ParamLayout(8, 4, 1)
    with pytest.raises(ValueError, match='sign'):
        _lib.call('tfep_volume_preserving_shift_f64', FAKE, 4, FAKE, 4, None, 0.0, 1.0, 2, FAKE, 4, 2, 4, None)
    with pytest.raises(ValueError, match='negative size'):
        _lib.call('tfep_affine_forward_f64', FAKE, 4, FAKE, lay, FAKE, 4, FAKE, 0, -1, 4, None)
    with pytest.raises(ValueError, match='non-NULL'):
        _lib.call('tfep_affine_inverse_f64', None, 4, FAKE, lay, FAKE, 4, FAKE, 0, 2, 4, None)
    with pytest.raises(ValueError, match='empty period'):
        _lib.call('tfep_periodic_embedding_f64', FAKE, 4, FAKE, 1, None, 0, 1.0, 1.0, FAKE, 2, 2, None)
    with pytest.raises(ValueError, match='NULL'):
        _lib.call('tfep_gather_columns_f64', None, 4, FAKE, 2, FAKE, 2, 3, None)
    with pytest.raises(ValueError, match='kT'):
        _lib.call('tfep_tfep_reduce_f64', FAKE, None, None, None, None, 0.0, 0, 4, FAKE, FAKE, None)
    # nothing to do: no launch, no pointer read
    lib = _lib.load()
    assert lib.tfep_affine_forward_f64(None, 4, None, lay, None, 4, None, 0, 0, 4, None) == 0
    assert lib.tfep_scatter_columns_f64(None, 4, None, 0, None, 4, 3, None) == 0


@pytest.mark.parametrize('sfx', ['', '_f64'])
def test_float32_and_float64_twins_refuse_the_same_arguments(sfx):
    # the checks the float32 entry points share with their _f64 twins; every call fails before a launch
    def refused(match, fn, *args):
        with pytest.raises(ValueError, match=f'{fn[5:]}{sfx}: {match}'):
            _lib.call(fn + sfx, *args)

    for B, D in ((-1, 4), (2, -4)):
        refused('negative size', 'tfep_volume_preserving_shift', FAKE, 4, FAKE, 4, None, 0.0, 1.0, 1, FAKE, 4, B, D, None)
    for B, n_per, n_non in ((-1, 1, 1), (2, -1, 1), (2, 1, -1)):
        refused('negative size', 'tfep_periodic_embedding', FAKE, 4, FAKE, n_per, FAKE, n_non, 0.0, 1.0, FAKE, 4, B, None)
        refused('negative size', 'tfep_periodic_embedding_backward', FAKE, 4, FAKE, n_per, FAKE, n_non, 0.0, 1.0, FAKE, 4,
                FAKE, 4, B, None)
    refused('empty period', 'tfep_periodic_embedding', FAKE, 4, FAKE, 1, None, 0, 1.0, 1.0, FAKE, 2, 2, None)
    refused('empty period', 'tfep_periodic_embedding_backward', FAKE, 4, FAKE, 1, None, 0, 1.0, 1.0, FAKE, 2, FAKE, 4, 2,
            None)
    refused('periodic_indices is NULL', 'tfep_periodic_embedding_backward', FAKE, 4, None, 1, None, 0, 0.0, 1.0, FAKE, 2,
            FAKE, 4, 2, None)
    refused('nonperiodic_indices is NULL', 'tfep_periodic_embedding_backward', FAKE, 4, None, 0, None, 1, 0.0, 1.0, FAKE, 2,
            FAKE, 4, 2, None)
    for fn in ('tfep_gather_columns', 'tfep_scatter_columns'):
        for B, n_idx in ((-1, 2), (3, -2)):
            refused('negative size', fn, FAKE, 4, FAKE, n_idx, FAKE, 4, B, None)


def test_float64_spline_config_validates_on_the_host():
    x0 = torch.zeros(3, dtype=torch.float64)
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        ops.SplineConfig(x0, x0, x0, x0, 4, dtype=torch.float64)


def test_float64_flow_on_cpu_has_no_fallback():
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF, SequentialFlow
    from tfep_amd.nn.transformers import NeuralSplineTransformer
    flow = SequentialFlow(MAF(generate_degrees(4), transformer=NeuralSplineTransformer(torch.full((4,), -2.0),
                                                                                      torch.full((4,), 2.0), 4))).double()
    x = torch.zeros(3, 4, dtype=torch.float64)
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        flow(x)
    with pytest.raises(_lib.TfepHipError, match='no CPU fallback'):
        flow.inverse(x)
    assert flow[0].is_float64 and not flow[0].float().is_float64


def test_float64_moebius_refused_on_the_host():
    from tfep_amd.nn.transformers import MoebiusTransformer
    with pytest.raises(TypeError, match='float64 is not supported'):
        MoebiusTransformer(2)(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64))
