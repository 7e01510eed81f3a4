#!/usr/bin/env python
"""Eager against HIP-graph replay of float64 flows, for README / DESIGN section 4b.  Run on an MI355X:

    python tools/measure_f64_graphs.py                  # every case, each in a fresh process, one after the other
    python tools/measure_f64_graphs.py inverse_d300     # one case, in this process

Cases: ``forward_d66`` / ``inverse_d66`` (cfg1's shape: 2 MAF layers + affine on 66 features, batch 1024),
``forward_d300`` / ``inverse_d300`` (2 MAF layers + RQ-8 spline on 300 features, batch 8192; the inverse is the float64
blocked forward substitution in both), ``train_d66`` (forward + TFEP loss + backward + AdamW with ``capturable=True`` at
cfg1's shape).  One graph per process.  One JSON line per case: the eager and the replayed time (host clock around calls
that end in a device synchronisation, alternating windows of the two, the median window of each), the number of C-ABI
kernel launches of one eager call (torch's own element-wise kernels come on top) and the git revision.  The outputs of the
two sides are compared bit for bit before anything is timed."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('forward_d66', 'inverse_d66', 'forward_d300', 'inverse_d300', 'train_d66')


def revision():
    try:
        return subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:  # noqa: BLE001  (a copy of the tree without its history)
        return os.environ.get('TFEP_REVISION', 'unknown')


def run_case(case):
    import torch
    sys.path.insert(0, ROOT)
    from tfep_amd import _lib, ops
    from tfep_amd.graphs import GraphedFlow, GraphedTrainingStep
    from tfep_amd.loss import BoltzmannKLDivLoss
    from tfep_amd.nn.conditioners import generate_degrees
    from tfep_amd.nn.flows import MAF, SequentialFlow
    from tfep_amd.nn.transformers import NeuralSplineTransformer

    kind, size = case.split('_')
    D, B = (66, 1024) if size == 'd66' else (300, 8192)
    dev = torch.device('cuda')
    F64 = torch.float64
    torch.manual_seed(0)
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        def transformer():
            return None if size == 'd66' else NeuralSplineTransformer(torch.full((D,), -5.0), torch.full((D,), 5.0), 8)
        flow = SequentialFlow(*[MAF(generate_degrees(D, o), transformer=transformer(), initialize_identity=False)
                                for o in ('ascending', 'descending')]).to(dev)
    finally:
        torch.set_default_dtype(old)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = 4.0 * (2.0 * torch.rand(B, D, device=dev, dtype=F64, generator=gen) - 1.0)

    # the C-ABI launches of one call (every entry point goes through ``_lib.call``; ``ops`` holds a second name for it)
    count = [0]
    real = _lib.call

    def counting(name, *args):
        count[0] += 1
        return real(name, *args)

    def launches(fn):
        _lib.call = ops.call = counting
        try:
            count[0] = 0
            fn()
            return count[0]
        finally:
            _lib.call = ops.call = real

    if kind == 'train':
        import copy
        loss_mod = BoltzmannKLDivLoss()

        def loss_fn(y, ldj):
            return loss_mod(0.5 * (y ** 2).sum(dim=1), ldj)
        kw = dict(lr=1e-6, capturable=True)
        twin = copy.deepcopy(flow)
        opt, opt_twin = torch.optim.AdamW(flow.parameters(), **kw), torch.optim.AdamW(twin.parameters(), **kw)

        def eager():
            opt_twin.zero_grad(set_to_none=True)
            loss = loss_fn(*twin(x))
            loss.backward()
            opt_twin.step()
            return loss.detach()
        graphed = GraphedTrainingStep(flow, loss_fn, opt, B, D)
        same = float(graphed(x)) == float(eager())
        replay = lambda: graphed(x)                                                        # noqa: E731
        route = None
    else:
        inverse = kind == 'inverse'
        with torch.no_grad():
            data = flow(x)[0] if inverse else x
            fn = flow.inverse if inverse else flow.forward

            def eager():
                with torch.no_grad():
                    return fn(data)
            graphed = GraphedFlow(flow, B, D, inverse=inverse)
            want, got = eager(), graphed(data)
        same = torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
        replay = lambda: graphed(data)                                                     # noqa: E731
        route = [layer.last_inverse_route for layer in flow] if inverse else None
    n_launches = launches(eager)

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for fn in (eager, replay):                        # warm both
        window(fn, 3)
    n = max(5, min(200, int(300.0 / max(window(eager, 3), 1e-3))))          # ~0.3 s of eager calls per window
    eager_ms, replay_ms = [], []
    for _ in range(5):                                # alternating windows
        eager_ms.append(window(eager, n))
        replay_ms.append(window(replay, n))
    e, r = statistics.median(eager_ms), statistics.median(replay_ms)
    print(json.dumps(dict(case=case, dtype='float64', D=D, batch=B, layers=len(flow), eager_ms=round(e, 4), replay_ms=round(r, 4),
                          ratio=round(e / r, 2), eager_c_abi_launches=n_launches, calls_per_window=n,
                          eager_windows_ms=[round(v, 4) for v in eager_ms], replay_windows_ms=[round(v, 4) for v in replay_ms],
                          bitwise_equal=bool(same), inverse_route=route, revision=revision(),
                          device=torch.cuda.get_device_name(0))), flush=True)
    return 0 if same else 1


def main(argv):
    cases = argv or list(CASES)
    unknown = [c for c in cases if c not in CASES]
    if unknown:
        print(f'unknown case(s) {unknown}; known: {", ".join(CASES)}', file=sys.stderr)
        return 2
    if len(cases) == 1:
        return run_case(cases[0])
    for case in cases:                                # one graph per process: a fresh child for every case, none concurrently
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), case]).returncode
        if rc != 0:
            print(f'{case} ended with status {rc}: stopping', file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
