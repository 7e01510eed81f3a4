#!/usr/bin/env python
"""SHA-256 digests of the raw output bytes of the float32 rational-quadratic spline kernels over the cases of
tests/spline_cases.py, per case:

  fwd_y, fwd_ldj, inv_x, inv_ldj    the stand-alone ``spline_kernel<KMAX, INVERSE>`` (``ops.spline``) in both directions
  grad_x, grad_par                  ``spline_backward_kernel<KMAX>`` (``ops.spline_backward``) in the default layout
  super_x, super_ldj                the one-launch-per-super-block kernel of the blocked inverse, on the cases that
                                    tests/test_gpu_spline_f32.py routes to it through a zero-weight MAF layer (``SUPER``): the
                                    one kernel that no ``torch.equal`` of that module ties to another

``tests/golden/spline_core_parent.json`` is this tool's output on an MI355X from the commit before the float32 spline was
rebuilt from the shared steps of ``csrc/spline.h``; ``test_the_bits_of_the_parent_commit`` holds every later tree to those
bits.  The tool uses nothing that commit lacks (the case builders are those of the test module).  Run on an MI355X:

    python tools/dump_spline_digests.py --dump OUT.json
"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(str((t.dtype, tuple(t.shape))).encode() + t.numpy().tobytes()).hexdigest()


def super_cases(sc):
    """The cases of the blocked-inverse test that have no learnable bound: those the super-block kernel takes."""
    known = sc.SHARED + ('e_rows_k8', 'e_narrow_k8', 'e_slopes_k8')
    return tuple(n for n in known if not (sc.case(n)['layout'][2] or sc.case(n)['layout'][3]))


def case_digests(name, sc, builders):
    """``output -> digest`` of one case; ``builders``: ``config`` and ``zero_weight_layer`` of the test module."""
    from tfep_amd import ops
    c = sc.case(name)
    cfg, par = builders.config(c), c['par'].cuda()
    out = {}
    out['fwd_y'], out['fwd_ldj'] = map(sha, ops.spline(c['x'].cuda(), par, cfg))
    out['inv_x'], out['inv_ldj'] = map(sha, ops.spline(c['yin'].cuda(), par, cfg, inverse=True))
    out['grad_x'], out['grad_par'] = map(sha, ops.spline_backward(c['x'].cuda(), par, cfg, c['gy'].cuda(), c['gl'].cuda()))
    if name in super_cases(sc):
        maf = builders.zero_weight_layer(c)
        maf.blocked_inverse = True
        maf.inverse_rows_per_wave, maf.inverse_waves_per_workgroup, maf.inverse_paired, maf.split_gemm = 16, None, True, True
        with torch.no_grad():
            x, ldj = maf.inverse(c['yin'].cuda())
        assert maf.last_inverse_route == 'blocked' and maf.last_inverse_schedule == 'super_kernel', name
        out['super_x'], out['super_ldj'] = sha(x), sha(ldj)
    return out


def all_digests(sc, builders):
    return {name: case_digests(name, sc, builders) for name in sc.NAMES}


def load(path=os.path.join(ROOT, 'tests', 'golden', 'spline_core_parent.json')):
    with open(path) as f:
        return json.load(f)


if __name__ == '__main__':
    if len(sys.argv) != 3 or sys.argv[1] != '--dump':
        sys.exit(__doc__)
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    import spline_cases
    import test_gpu_spline_f32
    out = all_digests(spline_cases, test_gpu_spline_f32)
    again = all_digests(spline_cases, test_gpu_spline_f32)      # a fixture is only worth keeping if the tree gives the same bits twice
    differ = [n for n in out if out[n] != again[n]]
    with open(sys.argv[2], 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print(sys.argv[2], len(out), 'cases,', sum(map(len, out.values())), 'digests; differ between two runs:', differ)
    sys.exit(1 if differ else 0)
