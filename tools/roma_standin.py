"""Stand-in for the third-party ``roma`` package, for ``tools/gen_golden.py`` only.

The reference's ``QuaternionProductTransformer`` (``tfep/nn/transformers/quatprod.py``) imports ``roma`` for four functions;
the package is not installed where the goldens are generated.  This module states those four in plain torch, in roma's
convention: a quaternion is the last axis of length 4 with the scalar LAST, ``(x, y, z, w)``, multiplied with the Hamilton
product.  ``install()`` registers it as ``sys.modules['roma']``.  It is never imported by ``tfep_amd``, and
``tests/test_quatprod_host.py`` pins what it produced against a product written out independently in numpy and against
``scipy.spatial.transform.Rotation``.
"""
import sys

import torch


def quat_normalize(quat):
    return quat / torch.norm(quat, dim=-1, keepdim=True)


def quat_conjugation(quat):
    return torch.cat((-quat[..., :3], quat[..., 3:]), dim=-1)


def quat_product(p, q):
    pv, pw = p[..., :3], p[..., 3:]
    qv, qw = q[..., :3], q[..., 3:]
    vector = pw * qv + qw * pv + torch.linalg.cross(pv, qv, dim=-1)
    scalar = pw * qw - torch.sum(pv * qv, dim=-1, keepdim=True)
    return torch.cat((vector, scalar), dim=-1)


def identity_quat(size=tuple(), dtype=None, device=None):
    size = (size,) if isinstance(size, int) else tuple(size)
    quat = torch.zeros(size + (4,), dtype=dtype, device=device)
    quat[..., 3] = 1.0
    return quat


def install():
    sys.modules.setdefault('roma', sys.modules[__name__])
