#!/usr/bin/env python
"""Write the integer tables that lay out the MADE output layer of a MAF layer, and one training step on them:

  <case>/fused/...     ``AutoregressiveFlow._fused_plan``: ``row_of_out``, ``n_rows`` and, per group ``g<i>``, ``feat_index``,
                       ``feat_tr``, ``k_ranges``, ``tile_order``, ``base``, ``n_rows``
  <case>/bwd/...       ``_backward._backward_plan``: ``sorted_out``, ``order`` and ``row_of_out`` (where the output rows are
                       degree sorted), every ``k_ranges[l]``, ``dx_ranges[l]``, ``live[l]`` and ``wide/k_ranges_out``
  <case>/saving/...    ``_backward._fused_saving_plan``: ``is_none`` and, where there is one, ``k_ranges``, ``tile_order``
  train/split<s>/...   case ``spline``: ``forward_saving`` + ``layer_backward`` on kept activations with ``split_gemm`` pinned to
                       ``s`` and the range guard off: ``y``, ``log_det_J``, the input gradient ``gx`` and every parameter
                       gradient ``g<i>`` (``trainable_tensors`` order)

for the layers of ``CASES``.  Weights and inputs come from fixed seeds on the CPU.

``tests/golden/output_layout_parent.npz`` is this tool's output on an MI355X from the commit before the degree-sorted row
layout was given one definition (``_tables.stable_order`` / ``_tables.packed_rows``): ``tests/test_gpu_output_layout.py``
holds every later tree to those tables and bits.  The tool uses nothing that commit lacks.  Run on an MI355X:

    python tools/dump_output_layout.py OUT.npz

Integer tables are kept whole; of a floating-point array of more than ``FULL_BELOW`` elements only the SHA-256 of its bytes
is kept: ``load`` gives ``name -> array or digest``, ``matches`` compares an output with either.
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tfep_amd.nn.conditioners import generate_degrees  # noqa: E402
from tfep_amd.nn.flows import MAF, _backward as bw  # noqa: E402
from tfep_amd.nn.transformers import (AffineTransformer, MixedTransformer, NeuralSplineTransformer,  # noqa: E402
                                      SOSPolynomialTransformer, VolumePreservingShiftTransformer)

FULL_BELOW = 1024
TRAIN_CASE, TRAIN_BATCH = 'spline', 512          # 512 rows x 1000 parameters: above the MiB from which activations are kept
CASES = ('spline', 'spline_fixed', 'affine16', 'sos2', 'mixed', 'spline_descending')
#: the cases whose training forward is the one-launch fused saving kernel
SAVING_CASES = ('spline', 'spline_fixed', 'spline_descending')


def _spline(n, **kwargs):
    return NeuralSplineTransformer(torch.full((n,), -4.0), torch.full((n,), 4.0), 8, **kwargs)


def build(case):
    """The layer of ``case`` on the GPU, weights from a fixed seed."""
    torch.manual_seed(11 + CASES.index(case))
    hidden = [70, 90]
    if case == 'spline':                 # 40 features on 13 degrees: repeated degrees, 40 slots are no multiple of 16
        maf = MAF(generate_degrees(40, 'ascending', max_value=12), transformer=_spline(40), hidden_layers=hidden,
                  initialize_identity=False)
    elif case == 'spline_fixed':
        maf = MAF(generate_degrees(40, 'ascending', max_value=12, conditioning_indices=[3, 17, 29]), transformer=_spline(37),
                  hidden_layers=hidden, initialize_identity=False)
    elif case == 'affine16':
        maf = MAF(generate_degrees(16, 'ascending'), transformer=AffineTransformer(), hidden_layers=hidden,
                  initialize_identity=False)
    elif case == 'sos2':
        maf = MAF(generate_degrees(21, 'ascending', max_value=6), transformer=SOSPolynomialTransformer(2), hidden_layers=hidden,
                  initialize_identity=False)
    elif case == 'mixed':                # 19 spline, 10 affine and 4 plain-shift features, interleaved
        idx = list(range(33))
        shift = idx[5::8]
        affine = [i for i in idx[1::3] if i not in shift][:10]
        spline = [i for i in idx if i not in shift and i not in affine]
        mixed = MixedTransformer([_spline(len(spline)), AffineTransformer(), VolumePreservingShiftTransformer()],
                                 [spline, affine, shift])
        maf = MAF(generate_degrees(33, 'descending', max_value=9), transformer=mixed, hidden_layers=hidden,
                  initialize_identity=False)
    else:                                # the slot order is the reverse of the feature order
        maf = MAF(generate_degrees(40, 'descending'), transformer=_spline(40), hidden_layers=hidden, initialize_identity=False)
    maf = maf.cuda()
    maf.split_guard = False
    return maf


def _np(t):
    return t.detach().cpu().numpy()


def plan_tables(case, maf):
    """``name -> array`` of every integer table of the three plans of the layer."""
    dev = torch.device('cuda', torch.cuda.current_device())
    maf._sync_conditioner()
    out = {}
    kind = maf._fused_kind()
    assert kind is not None, case
    fp = maf._fused_plan(dev, kind, maf._tables(dev))
    out['fused/row_of_out'], out['fused/n_rows'] = _np(fp['row_of_out']), np.int64(fp['n_rows'])
    out['fused/n_groups'] = np.int64(len(fp['groups']))
    for i, grp in enumerate(fp['groups']):
        for k in ('feat_index', 'feat_tr', 'k_ranges', 'tile_order'):
            out[f'fused/g{i}/{k}'] = _np(grp[k])
        for k in ('base', 'n_rows'):
            out[f'fused/g{i}/{k}'] = np.int64(grp[k])
    bp = bw._backward_plan(maf, dev)
    out['bwd/sorted_out'] = np.int64(bp['sorted_out'])
    if bp['sorted_out']:
        out['bwd/order'], out['bwd/row_of_out'] = _np(bp['order']), _np(bp['row_of_out'])
    for k in ('k_ranges', 'dx_ranges', 'live'):
        for l, t in enumerate(bp[k]):
            out[f'bwd/{k}/{l}'] = _np(t)
    out['bwd/has_wide'] = np.int64(bp['wide'] is not None)
    if bp['wide'] is not None:
        out['bwd/wide/k_ranges_out'] = _np(bp['wide']['k_ranges_out'])
    fs = bw._fused_saving_plan(maf, dev)
    out['saving/is_none'] = np.int64(fs is None)
    if fs is not None:
        out['saving/k_ranges'], out['saving/tile_order'] = _np(fs['k_ranges']), _np(fs['tile_order'])
    return {f'{case}/{k}': np.asarray(v) for k, v in out.items()}


def training_outputs(maf, split):
    """``name -> array`` of one forward on kept activations and its backward, ``split_gemm`` pinned to ``split``."""
    maf.split_gemm = bool(split)
    D = maf._inverse_masks.shape[1]
    gen = torch.Generator().manual_seed(23)
    x = (torch.randn(TRAIN_BATCH, D, generator=gen) * 1.3).clamp(-3.9, 3.9).cuda()
    gy, gl = torch.randn(TRAIN_BATCH, D, generator=gen).cuda(), torch.randn(TRAIN_BATCH, generator=gen).cuda()
    assert bw.saves_activations(maf, x)
    maf._sync_conditioner()
    with torch.no_grad():
        y, ldj, saved = bw.forward_saving(maf, x)
        gx, grads = bw.layer_backward(maf, x, gy, gl, saved=saved)
    out = {'y': y, 'log_det_J': ldj, 'gx': gx, **{f'g{i}': g for i, g in enumerate(grads)}}
    return {f'train/split{int(split)}/{k}': _np(v) for k, v in out.items()}


def all_outputs():
    out = {}
    for case in CASES:
        maf = build(case)
        out.update(plan_tables(case, maf))
        if case == TRAIN_CASE:
            for split in (True, False):
                out.update(training_outputs(maf, split))
    return out


def digest(a):
    a = np.ascontiguousarray(a)
    return np.frombuffer(hashlib.sha256(str((a.dtype, a.shape)).encode() + a.tobytes()).digest(), dtype=np.uint8)


def _by_digest(a):
    return a.dtype.kind == 'f' and a.size > FULL_BELOW


def matches(got, expected):
    """Whether the array ``got`` is what ``load`` returned for it: the stored array element for element, or of the stored
    digest (for an array stored by digest this is bitwise equality)."""
    got = np.asarray(got)
    if _by_digest(got):
        return expected.dtype == np.uint8 and bool((digest(got) == expected).all())
    return got.dtype == expected.dtype and got.shape == expected.shape and \
        torch.equal(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(expected)))


def save(path, out):
    np.savez_compressed(path, **{k.replace('/', '|'): (digest(v) if _by_digest(v) else v) for k, v in out.items()})


def load(path):
    with np.load(path) as z:
        return {k.replace('|', '/'): z[k] for k in z.files}


if __name__ == '__main__':
    out = all_outputs()
    again = all_outputs()                    # the fixture is only worth keeping if this tree gives the same bits twice
    differ = [k for k in out if not matches(again[k], digest(out[k]) if _by_digest(out[k]) else out[k])]
    save(sys.argv[1], out)
    print(sys.argv[1], len(out), 'arrays; differ between two runs:', differ)
    sys.exit(1 if differ else 0)
