"""Times the bias calculators (``sup3r_amd.bias_calc``) on a production-like
shape and prints one JSON line:

    python tools/bias_calc_probe.py [--grid 40 80] [--years 40]
        [--base-years 5] [--sites 9] [--repeats 3] [--ref-pixels 64]

  * a 40 x 80 bias grid with 40 years of daily data (14 610 steps, under the
    sort's LDS limit) and 9 base sites per pixel, hourly for 5 years (one
    entry of ``base_data`` per year);
  * a whole ``run()`` of ``MonthlyLinearCorrection``,
    ``QuantileDeltaMappingCorrection`` (12 windows, 50 quantiles) and
    ``PresRat``: wall time, and every ``s3_bc_*`` call between two device
    events on the context's stream — warm, the median of ``--repeats`` runs;
  * per kernel the bytes it has to read (series and base data once) against
    8 TB/s, and a device copy of the bias series as the yardstick of the sort
    kernels;
  * the per-pixel loop of ``tests/bias_calc_ref.py`` in float32 on this host
    for ``--ref-pixels`` pixels, scaled to the grid."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8e12


def make_inputs(grid, years, base_years, sites, seed=0):
    rng = np.random.default_rng(seed)
    s1, s2 = grid
    lat, lon = np.meshgrid(50.0 - np.arange(s1), -120.0 + np.arange(s2),
                           indexing='ij')
    bias_lat_lon = np.stack([lat, lon], axis=-1)
    bias_ti = pd.date_range('1980-01-01', periods=int(365.25 * years),
                            freq='D')
    fut_ti = pd.date_range('2050-01-01', periods=len(bias_ti), freq='D')
    shape = (s1, s2, len(bias_ti))
    bias = np.maximum(0, rng.standard_normal(shape, np.float32) + 0.6)
    fut = np.maximum(0, rng.standard_normal(shape, np.float32) + 0.8)
    # the sites of a pixel lie around it, and next to each other in memory
    off = rng.uniform(-0.4, 0.4, (s1 * s2, sites, 2))
    base_lat_lon = (bias_lat_lon.reshape(-1, 1, 2) + off).reshape(-1, 2)
    entries = []
    for y in range(base_years):
        ti = pd.date_range(f'{2001 + y}-01-01', f'{2001 + y}-12-31 23:00',
                           freq='h')
        arr = rng.standard_normal((len(ti), len(base_lat_lon)), np.float32)
        np.maximum(arr + 0.2, 0, out=arr)
        entries.append((arr, ti))
    return dict(base_data=entries, bias_data=bias, base_dset='pr_obs',
                bias_feature='pr', base_lat_lon=base_lat_lon,
                bias_lat_lon=bias_lat_lon, bias_time_index=bias_ti,
                bias_fut_data=fut, bias_fut_time_index=fut_ti)


def timed_backend():
    import torch
    from sup3r_amd.bias_calc import DeviceBackend

    class Timed(DeviceBackend):
        """every kernel call between two events on the context's stream"""
        events = []

        def _call(self, name, *args):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            super()._call(name, *args)
            b.record()
            self.events.append((name, a, b))

        def drain(self):
            torch.cuda.synchronize()
            out = {}
            for name, a, b in self.events:
                out[name] = out.get(name, 0.0) + a.elapsed_time(b)
            self.events.clear()
            return out
    return Timed()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, nargs=2, default=(40, 80))
    ap.add_argument('--years', type=float, default=40)
    ap.add_argument('--base-years', type=int, default=5)
    ap.add_argument('--sites', type=int, default=9)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--ref-pixels', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import sup3r_amd
    from tests import bias_calc_ref as R

    inp = make_inputs(args.grid, args.years, args.base_years, args.sites)
    n_pix = args.grid[0] * args.grid[1]
    n_b = len(inp['bias_time_index'])
    base_bytes = sum(a.nbytes for a, _ in inp['base_data'])
    n_days = sum(len(ti) for _, ti in inp['base_data']) // 24
    qdm_kw = dict(n_quantiles=50, n_time_steps=12, window_size=60)
    be = timed_backend()
    cases = {
        'MonthlyLinearCorrection': ({}, {}),
        'QuantileDeltaMappingCorrection': (qdm_kw, {}),
        'PresRat': (qdm_kw, dict(zero_rate_threshold=0.05)),
    }
    res = {'shape': dict(grid=list(args.grid), bias_steps=n_b,
                         base_steps=n_days * 24,
                         base_sites=len(inp['base_lat_lon']),
                         base_gib=round(base_bytes / 2 ** 30, 2)),
           'device': torch.cuda.get_device_name(0), 'classes': {}}
    # what each kernel has to read, once
    series = n_pix * n_b * 4
    need = {
        's3_bc_base_series': base_bytes,
        's3_bc_moments': series + n_pix * n_days * 4,
        's3_bc_window_quantiles': 2 * series * 60 * 12 / 365
        + n_pix * n_days * 4 * 60 * 12 / 365,
        's3_bc_presrat': 2 * series + n_pix * n_days * 4,
    }
    for kind, (kw, run_kw) in cases.items():
        full = dict(inp, **kw)
        if not kw:
            full.pop('bias_fut_data')
            full.pop('bias_fut_time_index')
        calc = getattr(sup3r_amd, kind)(backend=be, **full)
        walls, kernels = [], []
        for rep in range(args.repeats + 1):
            be.drain()
            t0 = time.perf_counter()
            calc.run(**run_kw)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            k = be.drain()
            if rep:                                   # the first run warms
                walls.append(wall)
                kernels.append(k)
        med = {n: float(np.median([k[n] for k in kernels]))
               for n in kernels[0]}
        res['classes'][kind] = {
            'run_wall_s': float(np.median(walls)),
            'kernel_ms': med,
            'read_gb': {n: round(need[n] / 1e9, 3) for n in med},
            'share_of_8TBps': {n: round(need[n] / HBM / (med[n] * 1e-3), 4)
                               for n in med},
        }
        t0 = time.perf_counter()
        sub = dict(full)
        R.run(kind, sub, np.float32, only=range(args.ref_pixels),
              fill_extend=False, **run_kw)
        host = time.perf_counter() - t0
        res['classes'][kind]['host_loop_s_scaled'] = host / args.ref_pixels \
            * n_pix
        res['classes'][kind]['host_loop_pixels'] = args.ref_pixels
    # the yardstick of the sort kernels: a device copy of the bias series
    x = be.upload(inp['bias_data'].reshape(n_pix, -1))
    times = []
    for _ in range(6):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        y = x.clone()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
        del y
    res['copy_of_bias_series_ms'] = float(np.median(times[1:]))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
