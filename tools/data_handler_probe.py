"""Cost of the two data-handler kernels that carry the bytes, in ONE process:

(a) ``s3_daily_reduce``: three months of hourly data on (300, 300) pixels, 4
    features -> 7 daily planes (mean / max / min of one, mean of another, two
    sums and their ratio) in one launch, against ``copy_`` of the 4 planes;
(b) ``s3_raster_gather`` of a flat ``(T = 8760, 2 10^6 sites)`` plane onto a
    (300, 300) raster, once with neighbouring sites along the raster's rows
    and once with scattered sites, against ``copy_`` of the raster;
(c) the host route of (a) for ONE feature (download, ``np.nanmean`` /
    ``nanmax`` / ``nanmin`` over the float64 windows, upload), and of (b) for
    a TENTH of the steps (numpy fancy indexing of a host array), host clock.

Algorithmic bytes: every source byte read once and every output byte written
once ((b): the raster's bytes read and written; the cache lines a scattered
gather drags along are not counted).  ``copy_`` moves its bytes twice, read and
write.  (a) and (b) are timed with device events around back-to-back calls
after a warm-up, two alternating passes each.  The flat source of (b) is
allocated uninitialised (70 GB): the gather copies bits.
Usage: python tools/data_handler_probe.py [--small]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
import torch  # noqa: E402
from sup3r_amd import _lib  # noqa: E402
from sup3r_amd.derive import DeviceBackend  # noqa: E402

small = '--small' in sys.argv
S = 30 if small else 300
DAYS = 9 if small else 90
T_FLAT, N_SITES = (96, 20000) if small else (8760, 2_000_000)
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


def table(rows, best, ms, nbytes):
    print('| pass | ms (two passes) | calls | bytes moved | TB/s | of 8 TB/s | '
          'time / copy_ |')
    print('|---|---|---|---|---|---|---|')
    for label, key, base in rows:
        rate = nbytes[key] / (best[key] * 1e-3)
        ratio = '' if base is None else f'{best[key] / best[base]:.2f}'
        print(f'| {label} | {ms[key][0][0]:.4f} / {ms[key][1][0]:.4f} | '
              f'{ms[key][1][1]} | {nbytes[key] / 1e6:.1f} MB | '
              f'{rate / 1e12:.2f} | {100 * rate / HBM_PEAK:.0f} % | {ratio} |')


# ------------------------------------------------------------ (a) the days
T = 24 * DAYS
planes = [torch.randn((S, S, T), dtype=torch.float32, device=cuda) * 5 + m
          for m in (280., 300., 400., 6.)]
planes[0][::7, ::5, ::3] = float('nan')
outputs = [(0, None, 'mean'), (0, None, 'max'), (0, None, 'min'),
           (3, None, 'mean'), (1, None, 'sum'), (2, None, 'sum'),
           (1, 2, 'ratio')]
spare = [torch.empty_like(p) for p in planes]
plane_bytes = planes[0].numel() * 4
nbytes = {'daily': 4 * plane_bytes + len(outputs) * plane_bytes // 24,
          'copy4': 8 * plane_bytes}


def daily():
    return be.daily_reduce(planes, 24, outputs)


def copy4():
    for dst, src in zip(spare, planes):
        dst.copy_(src)


# the result first, against the host route of feature 0, which is timed here
got = [g.cpu().numpy() for g in daily()[:3]]
torch.cuda.synchronize()
t0 = time.perf_counter()
host = planes[0].cpu().numpy()
t_down = time.perf_counter() - t0
win = host.astype(np.float64).reshape(S, S, DAYS, 24)
import warnings  # noqa: E402
with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    ref = [np.nanmean(win, -1), np.nanmax(win, -1), np.nanmin(win, -1)]
t_np = time.perf_counter() - t0 - t_down
up = [be.asarray(r.astype(np.float32)) for r in ref]
torch.cuda.synchronize()
t_host = time.perf_counter() - t0
assert np.allclose(got[0], ref[0], rtol=2e-7, atol=0, equal_nan=True)
assert np.array_equal(got[1], ref[1].astype(np.float32), equal_nan=True)
assert np.array_equal(got[2], ref[2].astype(np.float32), equal_nan=True)
del host, win, ref, up

ms = {k: [] for k in ('daily', 'copy4')}
for _ in range(2):                               # alternating: drift shows
    ms['daily'].append(device_ms(daily))
    ms['copy4'].append(device_ms(copy4))
best = {k: min(m for m, _ in v) for k, v in ms.items()}
print(f'(a) 4 planes {(S, S, T)} fp32, {4 * plane_bytes / 1e6:.1f} MB -> '
      f'{len(outputs)} planes {(S, S, DAYS)}; mean within 2e-7 relative of '
      'float64 numpy, max / min equal')
table([('s3_daily_reduce', 'daily', 'copy4'),
       ('copy_ of the 4 planes', 'copy4', None)], best, ms, nbytes)
print(f'host route, ONE feature (mean, max, min): {t_host * 1e3:.0f} ms '
      f'(download {t_down * 1e3:.0f}, numpy {t_np * 1e3:.0f}, upload the '
      f'rest); the launch for all four: {best["daily"]:.3f} ms')
del planes, spare
torch.cuda.empty_cache()

# ------------------------------------------------------------ (b) the raster
flat = torch.empty((T_FLAT, N_SITES), dtype=torch.float32, device=cuda)
rng = np.random.default_rng(0)
rows_of_sites = (rng.choice(N_SITES // S - 1, size=S, replace=False)[:, None]
                 * S + np.arange(S)[None, :])    # S neighbours per raster row
scattered = rng.choice(N_SITES, size=(S, S), replace=False)
raster_bytes = S * S * T_FLAT * 4
spare = torch.empty((S, S, T_FLAT), dtype=torch.float32, device=cuda)
spare2 = torch.empty_like(spare)
tables = {'near': be.to_index(rows_of_sites.reshape(-1)),
          'far': be.to_index(scattered.reshape(-1))}


def gather(which):
    """the launch alone: the site table is on the device already"""
    return lambda: be._gather(_lib.RG_FLAT, [flat], (S, S, T_FLAT), T_FLAT, 1,
                              (1, N_SITES, T_FLAT), 0, 0, 0, 1, tables[which])


def copy1():
    spare2.copy_(spare)


# bits: a tenth of the steps against numpy fancy indexing, which is timed
t_sub = max(T_FLAT // 10, 1)
flat[:t_sub].copy_(torch.randn((t_sub, N_SITES), device=cuda))
got = be.raster_gather([flat], t0=0, step=1, n_k=t_sub,
                       site=scattered)[0].cpu().numpy()
host = flat[:t_sub].cpu().numpy()
t0 = time.perf_counter()
want = np.ascontiguousarray(np.moveaxis(host[:, scattered], 0, -1))
t_np = time.perf_counter() - t0
assert np.array_equal(got.view(np.int32), want.view(np.int32))
del host, want, got

ms = {k: [] for k in ('near', 'far', 'copy1')}
for _ in range(2):
    ms['near'].append(device_ms(gather('near')))
    ms['far'].append(device_ms(gather('far')))
    ms['copy1'].append(device_ms(copy1))
best = {k: min(m for m, _ in v) for k, v in ms.items()}
nbytes = {k: 2 * raster_bytes for k in ms}
print(f'(b) flat {(T_FLAT, N_SITES)} fp32 -> raster {(S, S, T_FLAT)}, '
      f'{raster_bytes / 1e6:.1f} MB; a tenth of the steps bit-equal to numpy')
table([('s3_raster_gather, neighbouring sites', 'near', 'copy1'),
       ('s3_raster_gather, scattered sites', 'far', 'copy1'),
       ('copy_ of the raster', 'copy1', None)], best, ms, nbytes)
print(f'host route, a TENTH of the steps (numpy fancy indexing of a host '
      f'array, no transfer): {t_np * 1e3:.0f} ms')
