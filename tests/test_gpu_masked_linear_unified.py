"""GPU test of the single masked linear layer behind ``MaskedLinearFunc``, ``torch.ops.tfep.masked_linear`` and ``MADE``: what
every route computes, forward and backward, in float32 and float64, is bit for bit what the commit before the routes were
folded into ``ops.masked_linear_layer`` / ``ops.masked_linear_layer_backward`` computed
(``tests/golden/masked_linear_before_unify.npz``, written from that commit by tools/dump_masked_linear_outputs.py, whose
functions this test runs; that commit gave the same bits on two runs for every output)."""
import functools
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('dump_masked_linear_outputs',
                                               os.path.join(ROOT, 'tools', 'dump_masked_linear_outputs.py'))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)


@functools.lru_cache(maxsize=None)
def before():
    return dump.load(os.path.join(ROOT, 'tests', 'golden', 'masked_linear_before_unify.npz'))


@pytest.mark.parametrize('route', dump.ROUTES)
def test_route_equals_the_outputs_from_before_the_unification_bit_for_bit(route):
    """Every output of the route (``y`` and the gradients of input, weight, bias and weight norm of each case of
    ``dump.cases()``; the MADE forward) equals the fixture: ``torch.equal`` on the stored array or, for an output of more than
    ``dump.FULL_BELOW`` elements, the SHA-256 of its bytes."""
    got = dump.route_outputs(route)
    expected = {n: v for n, v in before().items() if n.startswith(route + '/')}
    assert sorted(got) == sorted(expected)
    assert [n for n in sorted(got) if not dump.matches(got[n], expected[n])] == []


def test_fully_masked_row_has_an_exactly_zero_weight_norm_gradient():
    """The cases with mask and weight norm have a fully masked first row: that entry of ``grad_g`` is exactly 0, and the
    masked entries of ``grad_v`` are (reference masked.py:401-402, :429)."""
    for name, shape, dtype, m, g, b in dump.cases():
        if m and g and b:
            tensors = dump.inputs(shape, dtype, m, g, b)
            for outputs in (dump.op_outputs, dump.func_outputs):
                out = outputs(tensors)
                assert out['gg'][0, 0] == 0 and out['gg'][1, 0] != 0, name
                assert not out['gw'][tensors[3].numpy() == 0].any(), name


def test_function_backward_returns_none_for_what_is_not_wanted():
    """``MaskedLinearFunc.backward`` with ``requires_grad`` on the input alone, and on the weight (and its norm) alone: None
    for everything else, and what it does return are the bits of the full backward."""
    expected = before()
    for name, shape, dtype, m, g, b in dump.cases():
        tensors = dump.inputs(shape, dtype, m, g, b)
        gi, gw, gb, gm, gg = dump.func_backward_alone(tensors, 'input')
        assert gw is None and gb is None and gm is None and gg is None, name
        assert gi.shape == tensors[0].shape and dump.matches(gi.cpu().numpy(), expected[f'func/{name}/gi']), name
        gi, gw, gb, gm, gg = dump.func_backward_alone(tensors, 'weight')
        assert gi is None and gb is None and gm is None and (gg is None) == (not g), name
        assert dump.matches(gw.cpu().numpy(), expected[f'func/{name}/gw']), name
        if g:
            assert dump.matches(gg.cpu().numpy(), expected[f'func/{name}/gg']), name
