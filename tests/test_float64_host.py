"""CPU tests of the float64 masked-linear host side: the new C-ABI entry points are declared, bound and exported, and
float64 argument errors are raised before any launch.  No kernel is launched (no GPU here)."""
import ctypes
import os
import re

import pytest
import torch

from tfep_amd import _lib, ops
from tfep_amd.nn import masked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_SYMBOLS = ('tfep_masked_weight_prepare_f64', 'tfep_mask_k_ranges_f64', 'tfep_masked_linear_gemm_f64',
               'tfep_transpose_f64', 'tfep_column_sums_f64', 'tfep_weight_norm_backward_f64', 'tfep_diag_mfma_f64_peak')


def test_float64_entry_points_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'tfep_hip.h')).read()
    declared = set(re.findall(r'\b(tfep_[a-z0-9_]+)\s*\(', header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in F64_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 8


def test_float64_gemm_argument_errors_before_launch():
    """The library rejects bad float64 GEMM arguments itself (status -1 -> ValueError) without touching a pointer."""
    lib = _lib.load()
    fake = ctypes.c_void_p(256)                  # never dereferenced: the checks fail first
    with pytest.raises(ValueError, match='k_padded'):
        _lib.call('tfep_masked_linear_gemm_f64', fake, 24, fake, 24, None, None, 256, fake, 8, 4, 8, 8, 24, 0, 0, None, 0, None)
    with pytest.raises(ValueError, match='act'):
        _lib.call('tfep_masked_linear_gemm_f64', fake, 32, fake, 32, None, None, 256, fake, 8, 4, 8, 8, 32, 2, 0, None, 0, None)
    with pytest.raises(ValueError, match='16-byte'):
        _lib.call('tfep_masked_linear_gemm_f64', fake, 33, fake, 32, None, None, 256, fake, 8, 4, 8, 8, 32, 0, 0, None, 0, None)
    with pytest.raises(ValueError, match='kr_tile_n'):             # a k-range table must be of whole kernel tiles
        _lib.call('tfep_masked_linear_gemm_f64', fake, 32, fake, 32, None, fake, 32, fake, 8, 4, 8, 8, 32, 0, 0, None, 0, None)
    assert lib.tfep_masked_linear_gemm_f64(None, 32, None, 32, None, None, 256, None, 8, 0, 8, 8, 32, 0, 0, None, 0, None) == 0


def test_float64_prefix_pack_is_float32_only():
    v = torch.zeros(4, 8, dtype=torch.float64)
    with pytest.raises(ValueError, match='float32-only'):
        ops.masked_weight_prepare(v, col_cut=torch.zeros(4, dtype=torch.int32))


def test_float64_module_keeps_reference_state_dict():
    lin = masked.masked_weight_norm(masked.MaskedLinear(8, 5, mask=torch.ones(5, 8))).double()
    sd = lin.state_dict()
    assert set(sd) == {'bias', 'mask', 'weight_g', 'weight_v'}
    assert all(t.dtype == torch.float64 for t in sd.values())
    assert masked._input_dtype(lin.weight_v) == torch.float64
    assert masked._input_dtype(lin.weight_v.float()) == torch.float32


def test_float64_gemm_rejects_k_ranges_of_another_tile_width():
    """A k-range table built for another tile width (e.g. the 32-column narrow tile) is refused before any launch."""
    x = torch.zeros(4, 32, dtype=torch.float64)
    w = torch.zeros(300, 32, dtype=torch.float64)
    kr = torch.zeros(10, 2, dtype=torch.int32)                   # ceil(300 / 32) tiles: not the 256-row tables
    with pytest.raises(ValueError, match='k_ranges has shape'):
        ops.masked_linear_f64(x, w, None, 300, k_ranges=kr)
