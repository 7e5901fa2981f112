"""Timing probe of the non-neural downscalers at production shapes (needs an
MI355X): ``SurfaceSpatialMetModel`` at the trhp forward-pass chunk, (48, 75,
75, 9) -> 15x -> (48, 1125, 1125, 9) fp32 (2.19 GB out), and
``LinearInterp`` at (8, 100, 100, 48, 2) -> 3x / 4x (1.1 GB out).

Prints one JSON object per model: device time per call (events, inputs and
output on the device), the whole ``generate`` call (upload, device, copy
back), the host restatement tests/interp_ref.py (timed on ``--host-obs``
observations and scaled to the batch) and the fraction of 8 TB/s with the
algorithmic bytes: the high-res field written once plus the low-res and
topography reads.  ``--trace-only``: only a few device calls (for a
``rocprofv3 --kernel-trace --stats`` run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRHP = ['temperature_2m', 'temperature_10m', 'temperature_100m',
        'relativehumidity_2m', 'relativehumidity_10m',
        'relativehumidity_100m', 'pressure_0m', 'pressure_100m',
        'pressure_200m']
PEAK = 8e12


def _events(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts))


def surface(args):
    from sup3r_amd import SurfaceSpatialMetModel
    from sup3r_amd.engine import Device
    from tests.test_interp_gpu import _surface_inputs
    dev = Device.get()
    n, h, w, s = args.n, 75, 75, 15
    low, topo_lr, topo_hr = _surface_inputs(n, h, w, s, TRHP)
    model = SurfaceSpatialMetModel(TRHP, s)
    xd, tl, th = (dev.to_device(a) for a in (low, topo_lr, topo_hr))
    med, best = _events(lambda: model.downscale_device(xd, tl, th),
                        3 if args.trace_only else args.reps)
    out_b = n * h * s * w * s * len(TRHP) * 4
    alg = out_b + low.nbytes + (h * s * w * s + h * w) * 4
    res = {'model': 'SurfaceSpatialMetModel', 'shape': [n, h, w, 9], 's': s,
           'device_ms': med, 'device_ms_best': best,
           'algorithmic_GB': alg / 1e9,
           'frac_8TBs': alg / (med * 1e-3) / PEAK}
    if not args.trace_only:
        exo = {'topography': {'steps': [{'data': topo_lr},
                                        {'data': topo_hr}]}}
        model.generate(low, exogenous_data=exo)
        t0 = time.perf_counter()
        y = model.generate(low, exogenous_data=exo)
        res['generate_ms'] = (time.perf_counter() - t0) * 1e3
        from tests import interp_ref as R
        k = args.host_obs
        t0 = time.perf_counter()
        ref = R.surface_generate(low[:k], topo_lr, topo_hr, TRHP, s)
        res['host_restatement_ms_scaled'] = \
            (time.perf_counter() - t0) * 1e3 * n / k
        res['host_obs_timed'] = k
        res['max_rel_err_vs_restatement'] = max(
            float(np.abs(y[:k, ..., i] - ref[..., i]).max() /
                  np.abs(ref[..., i]).max()) for i in range(len(TRHP)))
    return res


def linear(args):
    from sup3r_amd import LinearInterp
    from sup3r_amd.engine import Device
    dev = Device.get()
    shape, s, t = (8, 100, 100, 48, 2), 3, 4
    x = np.random.default_rng(0).standard_normal(shape).astype(np.float32)
    model = LinearInterp(['u_100m', 'v_100m'], s, t)
    xd = dev.to_device(x)
    med, best = _events(lambda: model.generate_device(xd),
                        3 if args.trace_only else args.reps)
    alg = x.nbytes * (1 + s * s * t)
    res = {'model': 'LinearInterp', 'shape': list(shape), 's': s, 't': t,
           'device_ms': med, 'device_ms_best': best,
           'algorithmic_GB': alg / 1e9,
           'frac_8TBs': alg / (med * 1e-3) / PEAK}
    if not args.trace_only:
        model.generate(x)
        t0 = time.perf_counter()
        y = model.generate(x)
        res['generate_ms'] = (time.perf_counter() - t0) * 1e3
        from tests import interp_ref as R
        t0 = time.perf_counter()
        ref = R.st_interp(x[0, ..., 0], s, t)
        res['host_restatement_ms_scaled'] = \
            (time.perf_counter() - t0) * 1e3 * shape[0] * shape[-1]
        res['max_rel_err_vs_restatement'] = float(
            np.abs(y[0, ..., 0] - ref).max() / np.abs(x).max())
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--n', type=int, default=48, help='time steps per chunk')
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--host-obs', type=int, default=2)
    p.add_argument('--trace-only', action='store_true')
    p.add_argument('--out', default=None, help='also write the JSON here')
    args = p.parse_args()
    rows = [surface(args), linear(args)]
    for r in rows:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
