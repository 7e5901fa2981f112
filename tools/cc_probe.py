"""Cost of one ``next(DeviceDualSamplerCC)`` at the production batch of the
solar climate-change models, ``(16, 20, 20, 72, 3)`` at ``t_enhance = 24`` and
``(16, 20, 20, 12, 3)`` at ``t_enhance = 3``, in ONE process, against

(a) the host route it replaces: download of the raw ``24 * lr_t``-hour batch,
    the numpy helpers of ``sup3r_amd.samplers_cc`` (middle days, daylight
    window) and ``scipy.ndimage.distance_transform_edt`` as in the reference's
    ``nn_fill_array``, upload;
(b) a ``torch`` device-to-device ``copy_`` of as many bytes as the hi-res
    batch has.

The device side is timed with events around back-to-back calls after a
warm-up, two alternating passes, over pre-drawn sets of origins; its stages
(the low-res gather, the hi-res gather with or without the night mask, the
fill) are timed the same way, the fill as ``gather + fill`` minus ``gather``
(it works in place: a second fill of the same batch would find nothing to do).
(a) is timed with the host clock around calls that end in a device
synchronise.  Per-kernel times come from a ``rocprofv3 --kernel-trace
--stats`` run of ``python tools/cc_probe.py --once``.
Usage: python tools/cc_probe.py [--small] [--once]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
import torch  # noqa: E402
from sup3r_amd.engine import Device  # noqa: E402
from sup3r_amd.samplers_cc import DeviceDualSamplerCC  # noqa: E402

small, once = '--small' in sys.argv, '--once' in sys.argv
FEATS = ['clearsky_ratio', 'temperature_2m', 'relativehumidity_2m']
# name, raster, days, sample shape, t_enhance, batch size
SHAPES = [('t_enhance 24', 60, 365, (20, 20, 72), 24, 16),
          ('t_enhance 3', 60, 365, (20, 20, 12), 3, 16)]
if small:
    SHAPES = [('t_enhance 24 (small)', 12, 40, (8, 8, 48), 24, 4),
              ('t_enhance 3 (small)', 12, 40, (8, 8, 12), 3, 4)]
N_SETS = 16
dev = Device.get()


def device_ms(fn, window_s=0.3):
    """ms per call: events around enough back-to-back calls to fill
    ``window_s``, after a warm-up"""
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    reps = 20
    while True:
        for i in range(5):
            fn(i)
        torch.cuda.synchronize()
        a.record()
        for i in range(reps):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= window_s * 1e3 or reps >= 20000:
            return ms / reps
        reps = min(20000, max(reps * 2,
                              int(reps * window_s * 1.2e3 / max(ms, 1e-3))))


def host_ms(fn, reps):
    fn(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def solar_cubes(S, days, seed=0):
    """daily / hourly cubes whose clearsky ratio is NaN at night; the night
    moves by an hour every 20 columns"""
    rng = np.random.default_rng(seed)
    hourly = rng.uniform(0.05, 1.0, (S, S, 24 * days, 3)).astype(np.float32)
    hour = np.arange(24 * days) % 24
    for j in range(S):
        shift = j // 20
        hourly[:, j, (hour < 6 + shift) | (hour >= 18 + shift), 0] = np.nan
    daily = np.nanmean(hourly.reshape(S, S, days, 24, 3), axis=3).astype(
        np.float32)
    return daily, hourly


try:
    from scipy import ndimage
except ImportError:
    ndimage = None

print('| shape | hi-res batch MB | next(sampler) ms | low-res gather ms | '
      'hi-res gather ms | fill ms | (b) copy ms | (a) host route ms | '
      'fill share of 8 TB/s |')
print('|---|---|---|---|---|---|---|---|---|')
for name, S, days, box, te, batch in SHAPES:
    daily, hourly = solar_cubes(S, days)
    smp = DeviceDualSamplerCC(daily, hourly, FEATS, FEATS, box,
                              batch_size=batch, t_enhance=te, seed=0)
    s1, s2, t = box
    lt = t // te
    sets = []
    for _ in range(N_SETS):
        ix = smp._batch_indices()
        sets.append((smp._origins([i[0] for i in ix], lt, batch),
                     smp._origins([i[1] for i in ix], 24 * lt, batch)))
    channels = smp._hr.channels(smp.hr_features)
    start, hours = smp._middle(24 * lt)
    shift = np.array([0, 0, start], dtype=np.int32)

    def low_gather(i):
        return smp._lr.gather(sets[i % N_SETS][0], smp.lr_sample_shape,
                              smp._lr.channels(smp.lr_features))

    def high_gather(i):
        org = sets[i % N_SETS][1] + shift
        if t >= hours:
            return smp._hr.gather(org, (s1, s2, hours), channels)
        return smp._daylight_gather(org, box, channels, channels[0])

    def gather_and_fill(i):
        high = high_gather(i)
        smp._nn_fill(high, 0)
        return high

    def host_route(i):
        org = sets[i % N_SETS][1]
        raw = smp._hr.gather(org, (s1, s2, 24 * lt), channels).cpu().numpy()
        raw = smp.reduce_high_res_sub_daily(raw, csr_ind=0, clamp=True)
        raw = np.ascontiguousarray(raw)
        holes = np.isnan(raw[..., 0])
        idx = ndimage.distance_transform_edt(holes, return_distances=False,
                                             return_indices=True)
        raw[..., 0] = raw[..., 0][tuple(idx)]
        return dev.to_device(raw)

    got = gather_and_fill(3)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (batch, s1, s2, t, 3), got.shape
    assert not torch.isnan(got[..., 0]).any()
    if ndimage is not None:
        want = host_route(3)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), name
    if once:
        for i in range(20):
            next(smp)
        torch.cuda.synchronize()
        print(f'| {name} | 20 batches drawn for the kernel trace |')
        continue
    out_bytes = got.numel() * 4
    pairs = [(torch.randn(got.numel(), device=dev.torch_device),
              torch.empty(got.numel(), device=dev.torch_device))
             for _ in range(8)]

    def copy(i):
        src, dst = pairs[i % 8]
        dst.copy_(src)

    ms = {k: [] for k in ('next', 'low', 'high', 'both', 'copy')}
    for _ in range(2):                           # alternating: drift shows
        ms['next'].append(device_ms(lambda i: next(smp)))
        ms['low'].append(device_ms(low_gather))
        ms['high'].append(device_ms(high_gather))
        ms['both'].append(device_ms(gather_and_fill))
        ms['copy'].append(device_ms(copy))
    best = {k: min(v) for k, v in ms.items()}
    fill = best['both'] - best['high']
    ms_host = host_ms(host_route, 5) if ndimage is not None else float('nan')
    # what a fill has to move at the least: the batch read and written once
    share = 2 * out_bytes / (fill * 1e-3) / 8e12
    both = ' / '.join(f'{v:.4f}' for v in ms['next'])
    print(f'| {name}: {batch} x {box} x 3 | {out_bytes / 1e6:.3f} | {both} | '
          f'{best["low"]:.4f} | {best["high"]:.4f} | {fill:.4f} | '
          f'{best["copy"]:.4f} | {ms_host:.2f} | {share:.4f} |')
    print(f'{name}: next(sampler) back to back, host clock, synchronised at '
          f'the end: {host_ms(lambda i: next(smp), 200):.4f} ms per batch; '
          f'NaNs found in the last batch: '
          f'{int(smp.cc_status.cpu()[3])} of {got.numel() // 3}')
    del smp, pairs, got
    torch.cuda.empty_cache()
