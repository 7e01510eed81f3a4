"""GPU test of the output-row layout of a MAF layer: every integer table of the fused plan, the backward plan and the fused
saving plan, and one training step on kept activations, are bit for bit what the commit before the layout was given one
definition (``_tables.stable_order`` / ``_tables.packed_rows``) produced (``tests/golden/output_layout_parent.npz``, written
from that commit by tools/dump_output_layout.py, whose functions this test runs; that commit gave the same bits on two runs
for every output)."""
import functools
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('dump_output_layout', os.path.join(ROOT, 'tools', 'dump_output_layout.py'))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)


@functools.lru_cache(maxsize=None)
def parent():
    return dump.load(os.path.join(ROOT, 'tests', 'golden', 'output_layout_parent.npz'))


def differing(got, prefix):
    expected = {n: v for n, v in parent().items() if n.startswith(prefix)}
    assert sorted(got) == sorted(expected)
    return [n for n in sorted(got) if not dump.matches(got[n], expected[n])]


@pytest.mark.parametrize('case', dump.CASES)
def test_plan_tables_equal_the_parents(case):
    """``row_of_out``, ``feat_index``, ``feat_tr``, ``k_ranges``, ``tile_order``, ``base``, ``n_rows`` of the fused plan; ``order``,
    ``row_of_out``, ``k_ranges``, ``dx_ranges``, ``live`` and the wide ``k_ranges_out`` of the backward plan; ``k_ranges`` and
    ``tile_order`` of the fused saving plan, or that there is none: ``torch.equal`` with the fixture."""
    got = dump.plan_tables(case, dump.build(case))
    assert differing(got, case + '/') == []


@pytest.mark.parametrize('case', dump.SAVING_CASES)
def test_plain_spline_layers_have_a_fused_saving_plan(case):
    """The fused plan and the backward plan take their slot order from one place, so a plain RQ-spline layer in a fused
    layout always gets the one-launch saving forward (this once depended on a runtime comparison of two separate sorts)."""
    from tfep_amd.nn.flows import _backward as bw
    maf = dump.build(case)
    dev = torch.device('cuda', torch.cuda.current_device())
    fs = bw._fused_saving_plan(maf, dev)
    assert fs is not None
    grp = maf._fused_plan(dev, maf._fused_kind(), maf._tables(dev))['groups'][0]
    assert fs['grp'] is grp
    n_tr = maf._tables(dev)['n_tr']
    assert torch.equal(grp['feat_tr'][:n_tr], bw._backward_plan(maf, dev)['order'])


@pytest.mark.parametrize('split', [True, False])
def test_training_step_on_kept_activations_equals_the_parents(split):
    """``forward_saving`` + ``layer_backward`` of the 40-feature spline layer with ``split_gemm`` pinned and the range guard
    off: ``y``, ``log_det_J``, the input gradient and every parameter gradient bit-equal to the fixture.  On split operands the
    forward is the one launch of the fused saving kernel."""
    maf = dump.build(dump.TRAIN_CASE)
    got = dump.training_outputs(maf, split)
    fused_saving = maf._dev.get(('fused_saving', str(torch.device('cuda', torch.cuda.current_device()))))
    assert (fused_saving is not None) == split
    assert differing(got, f'train/split{int(split)}/') == []
