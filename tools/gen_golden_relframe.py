"""Generate tests/golden/relframe.npz from the reference's ``tfep.utils.geometry``: the pieces of the relative frame of
``_CartesianToMixedFlow`` (``app/mixedmaf.py:1216-1271, 1321-1375``) as the reference computes them.

Dev-container only (needs the reference, through ``tools/ref_shim.py``; see ``tools/gen_golden.py``).  Everything is
computed by the reference on the CPU in float64.  The file holds the inputs ``x`` (N_ROWS, N_ATOMS, 3) whose last three
atoms are the origin, axis and plane atoms; the reference's ``R`` from ``reference_frame_rotation_matrix(...,
project_on_positive_axis=True)``; the rotated positions ``v``; ``cartesian_to_polar`` of the plane atom and
``polar_to_cartesian`` back, with their log-dets.  Row ``PI_ROW`` has the axis vector exactly (-2, 0, 0): the rotation
by pi.

    python tools/gen_golden_relframe.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402,F401
from tfep.utils import geometry as rg  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'relframe.npz')
N_ROWS, N_ATOMS, PI_ROW, SEED = 9, 6, 4, 11


def main():
    # (the reference compares against torch.zeros(1) in the DEFAULT dtype: float64 inputs need a float64 default)
    torch.set_default_dtype(torch.float64)
    gen = torch.Generator().manual_seed(SEED)
    x = 1.5 * torch.randn(N_ROWS, N_ATOMS, 3, dtype=torch.float64, generator=gen)
    x[PI_ROW, -3] = torch.tensor([0.5, -0.25, 1.0], dtype=torch.float64)
    x[PI_ROW, -2] = torch.tensor([-1.5, -0.25, 1.0], dtype=torch.float64)
    origin = x[:, -3]
    centered = x - origin.unsqueeze(1)
    R = rg.reference_frame_rotation_matrix(
        axis_atom_positions=centered[:, -2].clone(), plane_atom_positions=centered[:, -1].clone(),
        axis=rg.get_axis_from_name('x').to(x), plane_axis=rg.get_axis_from_name('y').to(x), project_on_positive_axis=True)
    v = rg.batchwise_rotate(centered, R)
    d02, a102, log_det_polar = rg.cartesian_to_polar(v[:, -1, 0], v[:, -1, 1], return_log_det_J=True)
    px, py, log_det_back = rg.polar_to_cartesian(d02, a102, return_log_det_J=True)
    back = rg.batchwise_rotate(v, R, inverse=True) + origin.unsqueeze(1)
    out = {'x': x, 'R': R, 'v': v, 'd02': d02, 'a102': a102, 'log_det_polar': log_det_polar, 'polar_x': px, 'polar_y': py,
           'log_det_polar_back': log_det_back, 'x_back': back}
    out = {k: t.numpy() for k, t in out.items()}
    out.update(pi_row=np.array(PI_ROW), seed=np.array(SEED))
    assert (centered[PI_ROW, -2]).tolist() == [-2.0, 0.0, 0.0]
    assert bool(torch.isfinite(R).all()) and abs(float(v[PI_ROW, -2, 0]) - 2.0) < 1e-12
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
