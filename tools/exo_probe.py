"""Times of exogenous rasterisation on the device (profiles/exo/NOTES.md).

Shapes: 4 000 000 source points (a 2000 x 2000 raster) onto a (500, 500)
target, the same sources onto (50, 50) (the long-list regime), and T = 24 on
the first.  Per shape: ``s3_exo_nearest`` and ``s3_exo_group_mean`` (device
events around repeated calls, after warm-up), next to a ``copy_`` of the bytes
each must read and write, as a fraction of 8 TB/s; then a whole
``ExoDataHandler`` for a two-step chain (2x, 5x over a (50, 50) low-res grid)
by the host clock around a device synchronise; with ``--host`` the host route
(KD-tree query and pandas group mean of tests/exo_ref.py) on the first shape.

    python tools/exo_probe.py [--small] [--host] [--json PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PEAK = 8e12          # bytes / s


def grid(h, w, lat0=45.0, lon0=-110.0, extent=10.0):
    lats = lat0 - extent * (np.arange(h) + 0.5) / h
    lons = lon0 + extent * (np.arange(w) + 0.5) / w
    return np.dstack(np.meshgrid(lats, lons, indexing='ij')).astype(
        np.float32)


def timed(fn, sync, warm=3, reps=10):
    """median / min / max of ``reps`` timed calls, ms, by device events"""
    import torch
    for _ in range(warm):
        fn()
    sync()
    out = []
    for _ in range(reps):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(min(out)), float(max(out))


def copy_ms(n_bytes, sync):
    """a ``copy_`` that reads and writes ``n_bytes`` in all"""
    import torch
    half = max(int(n_bytes) // 8, 1)
    a = torch.empty(half, dtype=torch.float32, device='cuda')
    b = torch.empty(half, dtype=torch.float32, device='cuda')
    a.fill_(1.0)
    return timed(lambda: b.copy_(a), sync)


def probe_shape(name, n_side, tgt_shape, t, rows):
    import torch
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    dev, L = Device.get(), _lib.lib()
    rng = np.random.default_rng(0)
    src = grid(n_side, n_side, 45.2, -110.2, 10.4).reshape(-1, 2)
    tgt = grid(*tgt_shape).reshape(-1, 2)
    n, m = len(src), len(tgt)
    r = float(np.abs(np.median(np.diff(grid(*tgt_shape), axis=0),
                               axis=0)).max())
    vals = rng.uniform(0, 4000, (n, t)).astype(np.float32)
    to = lambda a: torch.from_numpy(a).to(dev.torch_device)   # noqa: E731
    s, g, v = to(src), to(tgt), to(vals)
    nn = torch.empty(n, dtype=torch.int32, device=dev.torch_device)
    out = torch.empty((m, t), dtype=torch.float32, device=dev.torch_device)
    count = torch.empty(1, dtype=torch.int64, device=dev.torch_device)
    wb = max(int(L.s3_exo_nearest_work_bytes(m)),
             int(L.s3_exo_group_mean_work_bytes(m, t)))
    work = torch.empty(wb // 8 + 1, dtype=torch.int64, device=dev.torch_device)
    p = lambda x: C.c_void_p(x.data_ptr())                    # noqa: E731
    col = np.arange(t, dtype=np.int32)

    def nearest():
        rc = L.s3_exo_nearest(dev.ctx, p(s), n, p(g), m, r, p(work), wb,
                              p(nn), None)
        assert rc == 0, _lib.last_error(dev.ctx)

    def mean():
        rc = L.s3_exo_group_mean(
            dev.ctx, p(nn), p(v), n, m, t, t,
            col.ctypes.data_as(C.POINTER(C.c_int32)), 1.0, p(work), wb,
            p(out), p(count))
        assert rc == 0, _lib.last_error(dev.ctx)

    for what, fn, n_bytes in (
            ('nearest', nearest, 8 * n + 8 * m + 4 * n),
            ('group_mean', mean, 4 * n + 4 * n * t + 4 * m * t)):
        ms, lo, hi = timed(fn, dev.sync)
        cp, _, _ = copy_ms(n_bytes, dev.sync)
        rows.append(dict(shape=name, kernel=what, n_src=n, n_tgt=m, t=t,
                         ms=ms, ms_min=lo, ms_max=hi, bytes=n_bytes,
                         frac_of_8TBs=n_bytes / (ms * 1e-3) / PEAK,
                         copy_ms=cp, copy_frac_of_8TBs=n_bytes / (
                             cp * 1e-3) / PEAK, times_a_copy=ms / cp))
        print(json.dumps(rows[-1]), flush=True)
    hits = int((nn != m).sum().item())
    print(f'# {name}: {hits} of {n} sources within r = {r:.5f}; '
          f'{int(count.item())} NaN cells', flush=True)
    return src, tgt, r, vals


def probe_handler(n_side, rows):
    import pandas as pd
    import warnings
    from sup3r_amd import exo
    from sup3r_amd.engine import Device
    from test_exo_cpu import FakeModel, FakeMultiStep
    dev = Device.get()
    model = FakeMultiStep([
        FakeModel(['u', 'topography'], ['topography'], ['u'], s_enhance=2),
        FakeModel(['u', 'topography'], ['topography'], ['u'], s_enhance=5)])
    lr = grid(50, 50)
    ti = pd.date_range('2020-01-01', periods=4, freq='h')
    ll = grid(n_side, n_side, 45.2, -110.2, 10.4)
    vals = np.random.default_rng(1).uniform(0, 4000, ll.shape[:2]).astype(
        np.float32)
    src = exo.ExoSource(ll, topography=vals)
    times = []
    for _ in range(4):
        dev.sync()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            h = exo.ExoDataHandler('topography', exo.ExoInput(lr, ti),
                                   model=model, source_files=src)
        dev.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    shapes = [s.shape for s in h.data['topography']['steps']]
    rows.append(dict(shape='handler 2x, 5x over (50, 50)', kernel='whole',
                     n_src=n_side * n_side, steps=str(shapes),
                     ms_first=times[0], ms=float(np.median(times[1:]))))
    print(json.dumps(rows[-1]), flush=True)


def probe_host(src, tgt, r, vals, rows):
    import exo_ref
    t0 = time.perf_counter()
    dists, nn = exo_ref.query_tree(tgt.astype(np.float64), src, r)
    t1 = time.perf_counter()
    exo_ref.get_data_2d('x', vals[:, :1], nn, (len(tgt), 1, 1))
    t2 = time.perf_counter()
    rows.append(dict(shape='host route, first shape', kernel='KDTree.query',
                     ms=(t1 - t0) * 1e3))
    rows.append(dict(shape='host route, first shape',
                     kernel='pandas group mean', ms=(t2 - t1) * 1e3))
    print(json.dumps(rows[-2]), flush=True)
    print(json.dumps(rows[-1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true',
                    help='a 200 x 200 source: a rehearsal, not a measurement')
    ap.add_argument('--host', action='store_true')
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('exo_probe needs a GPU: nothing is timed without one')
    side = 200 if args.small else 2000
    big, small = ((50, 50), (5, 5)) if args.small else ((500, 500), (50, 50))
    rows = []
    first = probe_shape(f'{side * side} -> {big}', side, big, 1, rows)
    probe_shape(f'{side * side} -> {small}', side, small, 1, rows)
    probe_shape(f'{side * side} -> {big}, T = 24', side, big, 24, rows)
    probe_handler(side, rows)
    if args.host:
        probe_host(*first, rows)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
