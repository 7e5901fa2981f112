"""Cost of the two regridding kernels, in ONE process, at two shapes:

(a) an ERA5 region: 60 x 60 sources -> 100 x 100 targets, T = 8760, 2
    features;
(b) a large one: 721 x 1440 sources (the global 0.25-degree grid, hence the
    latitude-band mode) -> 250 x 250 targets, T = 744, 1 feature.

Per shape: ``s3_regrid_knn`` (device events around back-to-back calls; every
call builds the cell grid and waits once for the 64-byte read-back of the
boxes, so this is a host-visible time as well), ``s3_regrid_apply`` with the
tables on the device, a ``copy_`` of the OUTPUT bytes, and the host's
``BallTree`` build and query (host clock).

Algorithmic bytes of the apply: the output written once and k = 4 source rows
read per output row (4 x the output bytes) at most; neighbouring targets share
source rows, so the unique source bytes are far fewer: the table prints both
the rate over (1 + 4) x the output bytes and the time against ``copy_``, which
moves the output bytes twice (read and write).
Usage: python tools/regrid_probe.py [--small]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
import torch  # noqa: E402
from sup3r_amd.derive import DeviceBackend  # noqa: E402

small = '--small' in sys.argv
HBM_PEAK = 8.0e12                                # bytes / s, the data sheet's
be = DeviceBackend()
cuda = be.dev.torch_device


def device_ms(fn, window_s=0.3):
    """ms per call: events around enough back-to-back calls to fill
    ``window_s``, after a warm-up"""
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    reps = 3
    while True:
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= window_s * 1e3 or reps >= 2000:
            return ms / reps, reps
        reps = min(2000, max(reps * 2,
                             int(reps * window_s * 1.2e3 / max(ms, 1e-3))))


def grid(n1, n2, lat, lon, dlat, dlon):
    i, j = np.meshgrid(np.arange(n1), np.arange(n2), indexing='ij')
    return np.stack([lat - dlat * i, lon + dlon * j], -1).astype(
        np.float32).reshape(-1, 2)


def probe(label, src, tgt, t, n_feat):
    n, m = len(src), len(tgt)
    planes = [torch.randn((n, t), dtype=torch.float32, device=cuda)
              for _ in range(n_feat)]
    handle = be.regrid_knn(src, tgt, 4)
    outs, counts = be.regrid_apply(handle, planes, t)
    torch.cuda.synchronize()
    # the result first: against the BallTree, whose build and query are timed
    from sklearn.neighbors import BallTree
    t0 = time.perf_counter()
    tree = BallTree(np.deg2rad(src.astype(np.float64)), leaf_size=4,
                    metric='haversine')
    t_build = time.perf_counter() - t0
    dist, ind = tree.query(np.deg2rad(tgt.astype(np.float64)), k=4)
    t_query = time.perf_counter() - t0 - t_build
    idx = handle['idx'].cpu().numpy()
    agree = (idx == ind).all(axis=1).mean()
    d_err = np.abs(handle['dist'].cpu().numpy() - dist).max()
    out_bytes = n_feat * m * t * 4
    spare = [torch.empty_like(o) for o in outs]

    def knn():
        be.regrid_knn(src, tgt, 4)

    def apply():
        be.regrid_apply(handle, planes, t)

    def copy():
        for dst, o in zip(spare, outs):
            dst.copy_(o)

    ms = {k: [] for k in ('knn', 'apply', 'copy')}
    for _ in range(2):                           # alternating: drift shows
        ms['knn'].append(device_ms(knn))
        ms['apply'].append(device_ms(apply))
        ms['copy'].append(device_ms(copy))
    best = {k: min(v for v, _ in r) for k, r in ms.items()}
    print(f'{label}: {n} sources -> {m} targets, T = {t}, {n_feat} '
          f'feature(s), output {out_bytes / 1e6:.1f} MB; ids equal to the '
          f"BallTree's for {100 * agree:.2f} % of the targets, distances "
          f'within {d_err:.1e} rad')
    print('| pass | ms (two passes) | calls | bytes | TB/s | of 8 TB/s | '
          'time / copy_ |')
    print('|---|---|---|---|---|---|---|')
    rows = [('s3_regrid_apply, output + 4 rows per row', 'apply',
             5 * out_bytes),
            ('copy_ of the output bytes (read + write)', 'copy',
             2 * out_bytes)]
    for name, key, nb in rows:
        rate = nb / (best[key] * 1e-3)
        print(f'| {name} | {ms[key][0][0]:.4f} / {ms[key][1][0]:.4f} | '
              f'{ms[key][1][1]} | {nb / 1e6:.1f} MB | {rate / 1e12:.2f} | '
              f'{100 * rate / HBM_PEAK:.0f} % | '
              f'{best[key] / best["copy"]:.2f} |')
    print(f'| s3_regrid_knn (uploads, grid, query, one wait) | '
          f'{ms["knn"][0][0]:.4f} / {ms["knn"][1][0]:.4f} | '
          f'{ms["knn"][1][1]} | | | | |')
    print(f'host BallTree: build {t_build * 1e3:.1f} ms, query '
          f'{t_query * 1e3:.1f} ms; s3_regrid_knn {best["knn"]:.3f} ms')
    del planes, outs, spare
    torch.cuda.empty_cache()


if small:
    probe('(a) small', grid(12, 12, 42.0, -108.0, 0.25, 0.25),
          grid(20, 20, 41.0, -107.0, 0.09, 0.09), 96, 2)
    probe('(b) small, bands', grid(73, 144, 90.0, 0.0, 2.5, 2.5),
          grid(25, 25, 41.0, 253.0, 0.09, 0.09), 24, 1)
else:
    # 15 x 15 degrees of ERA5 around a 9 x 9 degree target region
    probe('(a) ERA5 region', grid(60, 60, 47.0, -112.0, 0.25, 0.25),
          grid(100, 100, 44.0, -109.0, 0.09, 0.09), 8760, 2)
    # the global grid, 0 .. 359.75 east: a longitude span above 180 degrees
    probe('(b) global ERA5', grid(721, 1440, 90.0, 0.0, 0.25, 0.25),
          grid(250, 250, 50.0, 240.0, 0.08, 0.08), 744, 1)
