"""Times ``SkillAssessment`` (``sup3r_amd.bias_calc``) on the shape of
``tools/bias_calc_probe.py`` and prints one JSON line:

    python tools/skill_probe.py [--grid 40 80] [--years 40] [--base-years 5]
        [--sites 9] [--repeats 3] [--ref-pixels 32] [--out FILE]

  * ``s3_bc_skill`` alone on the run's two device series (daily base series
    of 5 years, 40 years of daily bias data per pixel), between two events on
    the context's stream — warm, the median of ``--repeats`` launches — and
    the bytes it has to read once (both series) against 8 TB/s;
  * a device ``copy_`` of the two series' bytes as the yardstick;
  * a whole ``run()``: wall time, the time inside the ``s3_bc_*`` calls, and
    the host time spent on the KS p-values (``ks_seconds``), with the number
    of distinct p-values that were computed;
  * the reference's per-pixel arithmetic (``tests/skill_ref.run_single_skill``
    on the device's base series) in one host process for ``--ref-pixels``
    pixels, scaled to the grid — an extrapolation, and stated as one."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HBM = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, nargs=2, default=(40, 80))
    ap.add_argument('--years', type=float, default=40)
    ap.add_argument('--base-years', type=int, default=5)
    ap.add_argument('--sites', type=int, default=9)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--ref-pixels', type=int, default=32)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import sup3r_amd
    from sup3r_amd import bias_calc as B
    from bias_calc_probe import make_inputs, timed_backend
    from tests import bias_calc_ref as R
    from tests import skill_ref as S

    inp = make_inputs(args.grid, args.years, args.base_years, args.sites)
    inp.pop('bias_fut_data')
    inp.pop('bias_fut_time_index')
    n_pix = args.grid[0] * args.grid[1]
    be = timed_backend()
    calc = sup3r_amd.SkillAssessment(backend=be, **inp)
    memo_sizes = []
    plain = B.ks_from_counts

    def counted(n1, n2, counts, memo=None):
        memo = {}
        out = plain(n1, n2, counts, memo)
        memo_sizes.append(len(memo))
        return out
    B.ks_from_counts = counted
    walls, kernels, hosts = [], [], []
    for rep in range(args.repeats + 1):
        be.drain()
        t0 = time.perf_counter()
        calc.run()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        k = be.drain()
        if rep:                                       # the first run warms
            walls.append(wall)
            kernels.append(k)
            hosts.append(calc.ks_seconds)
    B.ks_from_counts = plain
    med = {n: float(np.median([k[n] for k in kernels])) for n in kernels[0]}
    # the kernel alone, on the run's own series
    base, base_ti = calc._base_series('avg')
    bias = calc._bias_series(calc.bias_data)
    n_d, n_t = int(base.shape[1]), int(bias.shape[1])
    need = (n_d + n_t) * n_pix * 4
    be.drain()
    alone = []
    for _ in range(args.repeats + 1):
        be.skill(base, bias, True)
        alone.append(be.drain()['s3_bc_skill'])
    skill_ms = float(np.median(alone[1:]))
    both = torch.cat([base.reshape(-1), bias.reshape(-1)])
    dst = torch.empty_like(both)
    times = []
    for _ in range(6):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(both)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    # the reference's arithmetic per pixel, on the same series
    h_base, h_bias = be.to_host(base), be.to_host(bias)
    good = np.where(np.diff(calc.site_ptr) > 0)[0][:args.ref_pixels]
    t0 = time.perf_counter()
    with R.quiet():
        for p in good:
            S.run_single_skill(h_bias[p], h_base[p], base_ti, calc.bias_ti,
                               'pr', 'pr_obs')
    host = time.perf_counter() - t0
    res = {
        'shape': dict(grid=list(args.grid), base_steps=n_d, bias_steps=n_t),
        'device': torch.cuda.get_device_name(0),
        'skill_kernel_ms': skill_ms,
        'skill_read_gb': round(need / 1e9, 4),
        'skill_share_of_8TBps': round(need / HBM / (skill_ms * 1e-3), 4),
        'copy_of_both_series_ms': float(np.median(times[1:])),
        'run_wall_s': float(np.median(walls)),
        'run_kernel_ms': med,
        'run_ks_pvalue_host_s': float(np.median(hosts)),
        'distinct_p_values': int(np.median(memo_sizes)),
        'host_loop_pixels': int(len(good)),
        'host_loop_s_scaled': host / max(len(good), 1) * n_pix,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
