#!/usr/bin/env python
"""Check a flow's own log-det against the Jacobian autograd gives: ``batch_autograd_log_abs_det_J`` of its output with
respect to its input, the check the reference's tests apply to every flow.  ``log_det_mismatch`` is the function (the
geometry tests use it); run as a script it checks a 2-layer float64 affine MAF on the GPU:

    python tools/check_flow_log_det.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfep_amd.utils.math import batch_autograd_log_abs_det_J  # noqa: E402


def log_det_mismatch(flow, x):
    """max |log_det_J of the flow - log |det dy/dx| by autograd| over the batch ``x`` (batch_size, D)."""
    x = x.detach().requires_grad_(True)
    y, log_det_J = flow(x)
    return float((log_det_J - batch_autograd_log_abs_det_J(x, y)).detach().abs().max())


def small_maf(D=6, dtype=torch.float64, device='cuda', seed=0):
    """A 2-layer affine MAF with random (not identity) weights."""
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF, SequentialFlow
    from tfep_amd.nn.transformers import AffineTransformer
    torch.manual_seed(seed)
    return SequentialFlow(*[MAF(generate_degrees(D, order), transformer=AffineTransformer(), initialize_identity=False)
                            for order in ('ascending', 'descending')]).to(dtype).to(device)


if __name__ == '__main__':
    x = torch.randn(5, 6, dtype=torch.float64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    err = log_det_mismatch(small_maf(), x)
    print(f'max |log_det_J - autograd| = {err:.3e}')
    assert err < 1e-9
