"""Host-side tests of the ``dtype`` keyword of ``tfep_amd.graphs`` (no GPU): the dtype inference on CPU modules, the
ValueError for a dtype the kernels do not run in, and the signatures (the keyword is last and defaults to None, so existing
positional calls mean what they meant).  The float64 capture added no C-ABI symbol, so there is no new declaration to check
against ``include/tfep_hip.h``."""
import inspect

import pytest
import torch

from tfep_amd import graphs


class _Scale(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.register_buffer('count', torch.zeros(2, dtype=torch.long))
        self.index = torch.nn.Parameter(torch.zeros(2, dtype=torch.long), requires_grad=False)     # not floating: passed over
        if dtype is not None:
            self.scale = torch.nn.Parameter(torch.ones(3, dtype=dtype))


@pytest.mark.parametrize('dtype, expected', [(torch.float64, torch.float64), (torch.float32, torch.float32),
                                             (None, torch.float32), (torch.float16, torch.float16)])
def test_flow_dtype_is_that_of_the_floating_parameters(dtype, expected):
    assert graphs.flow_dtype(_Scale(dtype)) is expected


def test_flow_dtype_of_a_module_without_parameters_is_float32():
    assert graphs.flow_dtype(torch.nn.Identity()) is torch.float32
    assert graphs.flow_dtype(torch.nn.Linear(2, 2).double()) is torch.float64


def test_resolve_dtype():
    f64, f32 = _Scale(torch.float64), _Scale(torch.float32)
    assert graphs._resolve_dtype(f64, None, 'GraphedFlow') is torch.float64
    assert graphs._resolve_dtype(f32, None, 'GraphedFlow') is torch.float32
    assert graphs._resolve_dtype(_Scale(None), None, 'GraphedFlow') is torch.float32
    # an explicit float32 / float64 overrides what the parameters say
    assert graphs._resolve_dtype(f64, torch.float32, 'GraphedFlow') is torch.float32
    assert graphs._resolve_dtype(f32, torch.float64, 'GraphedFlow') is torch.float64


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.int32, torch.int64, torch.bool, torch.complex64])
@pytest.mark.parametrize('cls', [graphs.GraphedFlow, graphs.GraphedTrainingStep])
def test_other_dtypes_are_value_errors_at_construction(cls, dtype):
    """Raised before anything touches a device: this runs without one."""
    flow = _Scale(torch.float64)
    with pytest.raises(ValueError, match=cls.__name__):
        if cls is graphs.GraphedFlow:
            cls(flow, 3, 4, dtype=dtype)
        else:
            cls(flow, lambda y, ldj: ldj.mean(), torch.optim.SGD(flow.parameters(), lr=0.1), 3, 4, dtype=dtype)


def test_half_parameters_without_an_override_are_a_value_error():
    with pytest.raises(ValueError, match='float16'):
        graphs.GraphedFlow(_Scale(torch.float16), 3, 4)


@pytest.mark.parametrize('cls, before', [
    (graphs.GraphedFlow, ['flow', 'batch_size', 'n_features', 'inverse', 'device', 'warmup', 'check_range']),
    (graphs.GraphedTrainingStep, ['flow', 'loss_fn', 'optimizer', 'batch_size', 'n_features', 'device', 'warmup', 'sample_input']),
])
def test_dtype_is_the_last_keyword_and_defaults_to_none(cls, before):
    params = list(inspect.signature(cls.__init__).parameters.values())[1:]          # (without self)
    assert [p.name for p in params] == before + ['dtype']
    assert params[-1].default is None
    assert params[-1].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


def test_input_dtype_check():
    """A float64 graph refuses inputs of another dtype; a float32 graph converts, as it always has."""
    s64, s32 = torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 3)
    graphs._check_input_dtype(torch.zeros(2, 3, dtype=torch.float64), s64, 'GraphedFlow')
    for other in (torch.float32, torch.float16, torch.int64):
        with pytest.raises(TypeError, match='GraphedFlow'):
            graphs._check_input_dtype(torch.zeros(2, 3, dtype=other), s64, 'GraphedFlow')
    for any_dtype in (torch.float32, torch.float64, torch.int64):
        graphs._check_input_dtype(torch.zeros(2, 3, dtype=any_dtype), s32, 'GraphedFlow')


def test_volume_preserving_shift_mask_is_made_once():
    """The periodic mask and limits of the shift transformer are cached (a host -> device copy per call cannot be captured)
    and follow the two attributes when they are replaced or written."""
    from tfep_amd.nn.transformers import VolumePreservingShiftTransformer
    t = VolumePreservingShiftTransformer(torch.tensor([1]), torch.tensor([-4.0, 4.0]))
    x = torch.zeros(2, 3)
    m0, lim0 = t._mask(x)
    m1, lim1 = t._mask(x)
    assert m1 is m0 and m0.tolist() == [0, 1, 0] and lim0 == lim1 == (-4.0, 4.0)
    assert t._mask(torch.zeros(2, 4))[0].tolist() == [0, 1, 0, 0]
    t.periodic_indices = [0, 2]
    assert t._mask(x)[0].tolist() == [1, 0, 1]
    t.periodic_limits.mul_(0.5)
    assert t._mask(x)[1] == (-2.0, 2.0)
    assert VolumePreservingShiftTransformer()._mask(x) == (None, (0.0, 1.0))

