#!/usr/bin/env python
"""Write what the float32 wrapped flows of ``golden_util.wrapper_configs()`` compute on the inputs of
``tests/golden/wrappers.npz`` with nothing set on them (the default route), forward and -- where the fixture has an inverse
input -- inverse, as an ``.npz`` of float32 arrays ``<name>/{y,ldj,xinv,ldjinv}``.

``tests/golden/wrappers_f32_before_frames.npz`` is this tool's output on an MI355X from the commit before the frame kernels
(``csrc/frames.hip``) existed: ``tests/test_gpu_frames.py`` holds the float32 default of every later tree to those bits.
The tool uses nothing that commit lacks.  Run on an MI355X:

    python tools/dump_wrapper_outputs.py OUT.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import golden_util as gu  # noqa: E402
import tfep_amd.nn.flows as flows  # noqa: E402
from oracle.made import generate_degrees  # noqa: E402
from tfep_amd.nn.flows import MAF  # noqa: E402
from tfep_amd.nn.transformers import AffineTransformer, NeuralSplineTransformer  # noqa: E402


def build(name, g):
    cfg = gu.wrapper_configs()[name]
    n_in = gu.wrapper_n_inner(cfg)
    if cfg.get('spline'):
        tr = NeuralSplineTransformer(x0=torch.full((n_in,), -8.0), xf=torch.full((n_in,), 8.0), n_bins=6)
    else:
        tr = AffineTransformer()
    inner = MAF(degrees_in=torch.as_tensor(generate_degrees(n_in, 'ascending')), transformer=tr, initialize_identity=False)
    flow = gu.build_wrapped(cfg, inner, flows)
    sd = flow.state_dict()
    for k, v in gu.sub(g, f'{name}/sd/').items():
        sd[k] = torch.from_numpy(np.asarray(v))
    flow.load_state_dict(sd, strict=True)
    return flow.cuda(), cfg


def outputs(name, g):
    flow, cfg = build(name, g)
    out = {}
    with torch.no_grad():
        y, ldj = flow(torch.from_numpy(g[f'{name}/x']).cuda())
        out[f'{name}/y'], out[f'{name}/ldj'] = y.cpu().numpy(), ldj.cpu().numpy()
        if cfg['inverse']:
            x, ldji = flow.inverse(torch.from_numpy(g[f'{name}/inv_in']).cuda())
            out[f'{name}/xinv'], out[f'{name}/ldjinv'] = x.cpu().numpy(), ldji.cpu().numpy()
    return out


if __name__ == '__main__':
    g = gu.load('wrappers.npz')
    out = {}
    for name in gu.wrapper_configs():
        out.update(outputs(name, g))
    np.savez_compressed(sys.argv[1], **out)
    print(sys.argv[1], len(out), 'arrays')
