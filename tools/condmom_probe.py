"""Device time of ``s3_condmom_target`` (the conditional-moment batch targets)
against ``s3_coarsen`` on the same hi-res batch and against the numpy / scipy
host path it replaces (tests/condmom_ref.py).  All timings in ONE process
(call-to-call spread).
Usage: python tools/condmom_probe.py [--small] [--no-host]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
import torch  # noqa: E402
from sup3r_amd import _lib  # noqa: E402
from sup3r_amd.engine import Device  # noqa: E402
from tests import condmom_ref as R  # noqa: E402

PEAK = 8e12                                      # HBM3E bytes / s
small = '--small' in sys.argv
shape, s, te = ((4, 24, 24, 16, 2) if small else (32, 96, 96, 96, 2)), 3, 4
lr_shape = (shape[0], shape[1] // s, shape[2] // s, shape[3] // te, shape[4])
rng = np.random.default_rng(0)
hr = rng.standard_normal(shape).astype(np.float32)
dev, L = Device.get(), _lib.lib()
hr_d = dev.to_device(hr)
lr_d, m_d, out_d, mask_d = (dev.empty(sh) for sh in
                            (lr_shape, shape, shape, shape))
m_d.normal_()


def ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def coarsen():
    _lib.check(L.s3_coarsen(dev.ctx, ptr(hr_d), *shape, s, te,
                            _lib.TC_METHODS['average'], ptr(lr_d)),
               dev.ctx, 's3_coarsen')


def target(flags, with_mask):
    cmap = (C.c_int32 * 2)(0, 1)

    def run():
        _lib.check(L.s3_condmom_target(
            dev.ctx, ptr(hr_d), ptr(lr_d), ptr(m_d), *shape, shape[4],
            shape[4], cmap, s, te, flags, 1, 1, shape[3] - 1, ptr(out_d),
            ptr(mask_d) if with_mask else None), dev.ctx, 's3_condmom_target')
    return run


def device_ms(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


coarsen()
nb, lb = hr.nbytes, hr.nbytes / (s * s * te)
rows = [('s3_coarsen (average)', coarsen, nb + lb)]
SF, LIN, M1, SQ = (_lib.CM_SUBFILTER, _lib.CM_LINEAR, _lib.CM_MOM1,
                   _lib.CM_SQUARE)
for name, flags, n_in in (('Mom1SF constant', SF, 1),
                          ('Mom1SF linear', SF | LIN, 1),
                          ('Mom2SF', SF | M1 | SQ, 2)):
    for with_mask in (False, True):
        rows.append((f'{name}{" + mask" if with_mask else ""}',
                     target(flags, with_mask),
                     nb * (n_in + 1 + with_mask) + lb))
# two passes over the rows, alternating, so that drift shows
ms = {name: [] for name, _, _ in rows}
for _ in range(2):
    for name, fn, _ in rows:
        ms[name].append(device_ms(fn))
print(f'hr {shape}, {s}x / {te}x, {nb / 1e6:.0f} MB per hi-res tensor')
print('| call | device ms (two passes) | algorithmic MB | TB/s | of 8 TB/s |')
print('|---|---|---|---|---|')
rate = {}
for name, _, moved in rows:
    best = min(ms[name])
    rate[name] = moved / best / 1e9
    print(f'| {name} | {ms[name][0]:.4f} / {ms[name][1]:.4f} | '
          f'{moved / 1e6:.0f} | {rate[name]:.2f} | '
          f'{moved / best / 1e-3 / PEAK:.1%} |')
base = rate['s3_coarsen (average)']
for name in list(rate)[1:]:
    print(f'{name}: {rate[name] / base:.2f} x the bytes/s of s3_coarsen')

if '--no-host' not in sys.argv:
    lr = lr_d.cpu().numpy()
    mom1 = m_d.cpu().numpy()
    for kind, mode in (('Mom1SF', 'constant'), ('Mom1SF', 'linear'),
                       ('Mom2SF', 'constant')):
        t0 = time.perf_counter()
        R.make_output(kind, lr, hr, s, te, mode, [0, 1], mom1=mom1)
        R.make_mask(shape, 1, 1, False, te)
        print(f'host numpy / scipy {kind} {mode}: '
              f'{(time.perf_counter() - t0) * 1e3:.0f} ms')
