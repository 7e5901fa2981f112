"""Cost of the statistics stage on one production-like cube, in ONE process:

(a) ``s3_channel_moments`` (both kernels, without the read-back) against
    ``torch.sum`` over the same tensor: a read-only pass over the same bytes;
(b) ``s3_normalize_channels`` against an in-place ``mul_``: one read and one
    write of the same bytes;
(c) the host route they replace: download, ``np.nanmean`` / ``np.nanstd`` on
    the float64-widened cube, float32 normalisation, upload.

(a) and (b) are timed with device events around back-to-back calls after a
warm-up, two alternating passes each; (c) with the host clock, once, ending in
a device synchronise.  The cube is larger than the 256 MiB Infinity Cache, so
every pass streams from HBM.  The normalisation is timed with mean 0 and std 1
(and ``mul_`` with 1): the same instructions, and the data stay as they are.
Usage: python tools/stats_probe.py [--small]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
import torch  # noqa: E402
from sup3r_amd import _lib  # noqa: E402
from sup3r_amd.engine import Device  # noqa: E402
from sup3r_amd.samplers import channel_moments, normalize_channels  # noqa: E402

small = '--small' in sys.argv
# three months of hourly data, 100 x 100 pixels, 6 features: 530 MB
SHAPE = (20, 20, 200, 6) if small else (100, 100, 2208, 6)
HBM_PEAK = 8.0e12                                # bytes / s, the data sheet's
dev = Device.get()


def device_ms(fn, window_s=0.3):
    """ms per call: events around enough back-to-back calls to fill
    ``window_s``, after a warm-up"""
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    reps = 5
    while True:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= window_s * 1e3 or reps >= 5000:
            return ms / reps, reps
        reps = min(5000, max(reps * 2,
                             int(reps * window_s * 1.2e3 / max(ms, 1e-3))))


feats = [f'f{i}' for i in range(SHAPE[3])]
c = SHAPE[3]
loc = torch.tensor([0., 5., 9.5e4, 280., 0.5, -3.], device=dev.torch_device)
cube = torch.randn(SHAPE, dtype=torch.float32, device=dev.torch_device) \
    * 3 + loc[:c]
cube[::7, ::5, ::3, 4] = float('nan')
nbytes = cube.numel() * 4
out = torch.empty((c, 3), dtype=torch.float64, device=dev.torch_device)
L = _lib.lib()
zeros, ones = np.zeros(c, np.float32), np.ones(c, np.float32)
flags = np.ones(c, np.uint8)


def moments():
    rc = L.s3_channel_moments(dev.ctx, C.c_void_p(cube.data_ptr()),
                              cube.numel() // c, c, C.c_void_p(out.data_ptr()))
    assert rc == 0


def torch_sum():
    torch.sum(cube)


def normalize():
    normalize_channels(dev, cube, zeros, ones, flags)


def mul():
    cube.mul_(1.0)


# the results first: device against the host route, which is timed here
torch.cuda.synchronize()
t0 = time.perf_counter()
host = cube.cpu().numpy()
t_down = time.perf_counter() - t0
wide = host.reshape(-1, c).astype(np.float64)
mean, std = np.nanmean(wide, axis=0), np.nanstd(wide, axis=0)
t_stats = time.perf_counter() - t0 - t_down
del wide
m32, s32 = mean.astype(np.float32), std.astype(np.float32)
host_norm = (host - m32) / s32
t_norm = time.perf_counter() - t0 - t_down - t_stats
up = dev.to_device(host_norm)
torch.cuda.synchronize()
t_host = time.perf_counter() - t0
got = channel_moments(dev, cube)
got_std = np.sqrt(got[:, 2] / got[:, 0])
assert np.array_equal(got[:, 1].astype(np.float32), m32) or \
    np.allclose(got[:, 1], mean, rtol=2e-7, atol=0), (got[:, 1], mean)
assert np.allclose(got_std, std, rtol=2e-7, atol=0), (got_std, std)
check = cube.clone()
normalize_channels(dev, check, m32, s32, flags)
same = torch.equal(torch.nan_to_num(check, nan=0.0),
                   torch.nan_to_num(up, nan=0.0))
assert same, 'device normalisation differs from numpy float32'
del check, up, host, host_norm
torch.cuda.empty_cache()

ms = {k: [] for k in ('moments', 'sum', 'normalize', 'mul')}
for _ in range(2):                               # alternating: drift shows
    ms['moments'].append(device_ms(moments))
    ms['sum'].append(device_ms(torch_sum))
for _ in range(2):
    ms['normalize'].append(device_ms(normalize))
    ms['mul'].append(device_ms(mul))
best = {k: min(m for m, _ in v) for k, v in ms.items()}

print(f'cube {SHAPE} fp32, {nbytes / 1e6:.1f} MB; device results equal the '
      'host route (mean / std within 2e-7 relative, normalised cube bit-equal)')
print('| pass | ms (two passes) | calls | bytes moved | TB/s | of 8 TB/s | '
      'ratio to baseline |')
print('|---|---|---|---|---|---|---|')
rows = [('s3_channel_moments', 'moments', 1, 'sum'),
        ('torch.sum', 'sum', 1, None),
        ('s3_normalize_channels', 'normalize', 2, 'mul'),
        ('in-place mul_', 'mul', 2, None)]
for label, key, passes, base in rows:
    rate = passes * nbytes / (best[key] * 1e-3)
    ratio = '' if base is None else f'{best[key] / best[base]:.2f}'
    print(f'| {label} | {ms[key][0][0]:.4f} / {ms[key][1][0]:.4f} | '
          f'{ms[key][1][1]} | {passes * nbytes / 1e6:.1f} MB | '
          f'{rate / 1e12:.2f} | {100 * rate / HBM_PEAK:.0f} % | {ratio} |')
print(f'host route: {t_host * 1e3:.0f} ms (download {t_down * 1e3:.0f}, '
      f'nanmean + nanstd {t_stats * 1e3:.0f}, normalise {t_norm * 1e3:.0f}, '
      f'upload the rest) = {t_host * 1e3 / (best["moments"] + best["normalize"]):.0f}'
      ' x the two device passes')
