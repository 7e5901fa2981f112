"""Cost of the QA stage on one production-like output, in ONE process: a
three-month hourly 3x / 4x output ``(300, 300, 2208, 2)`` against its
``(100, 100, 552)`` source.

(a) ``s3_qa_recoarsen`` with synthetic, error and summary, on the cube (both
    features in one launch) and on one time-first field;
(b) a whole ``direct_dist`` and a whole ``gradient_dist`` of one
    high-resolution feature (percentile select, statistics, histogram and
    their read-backs);
(c) one ``frequency_spectrum`` of a source feature (the hi-res time axis is
    beyond ``s3_dft_axis``);
each against a ``copy_`` of the bytes it has to read and against the host
route: download plus the reference's numpy lines (tests/qa_ref.py).

(a) is timed with device events around back-to-back calls after a warm-up;
(b), (c) and the host route with the host clock around synchronised calls.
Results are checked against the host route before anything is timed.
Usage: python tools/qa_probe.py [--small]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
import torch  # noqa: E402
from sup3r_amd import _lib, qa  # noqa: E402
from tests import qa_ref as R  # noqa: E402

small = '--small' in sys.argv
S, TE = 3, 4
LR = (10, 10, 24) if small else (100, 100, 552)
HR = (LR[0] * S, LR[1] * S, LR[2] * TE)
HBM_PEAK = 8.0e12
be = qa.QaDeviceBackend()
dev = be.dev


def say(*a):
    print(*a, flush=True)


def device_ms(fn, window_s=0.3):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    reps = 3
    while True:
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


def host_ms(fn, reps=3):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def row(label, ms, nbytes, note=''):
    rate = nbytes / (ms * 1e-3)
    say(f'| {label} | {ms:.3f} | {nbytes / 1e6:.1f} MB | {rate / 1e12:.2f} | '
        f'{100 * rate / HBM_PEAK:.0f} % | {note} |')


g = torch.Generator(device=dev.torch_device).manual_seed(0)
true = [torch.randn(LR, generator=g, device=dev.torch_device) * 5
        for _ in range(2)]
cube = torch.stack([t.repeat_interleave(S, 0).repeat_interleave(S, 1)
                    .repeat_interleave(TE, 2) for t in true], -1).contiguous()
cube += torch.randn(cube.shape, generator=g, device=dev.torch_device)
tfirst = cube[..., 0].permute(2, 0, 1).contiguous()
plane = cube[..., 0].contiguous()
methods = ['average', 'subsample']
n_cube, n_plane = cube.numel() * 4, plane.numel() * 4
say(f'output {tuple(cube.shape)} fp32 = {n_cube / 1e6:.1f} MB, source {LR}')

# ---- results first, and the host route timed on the way
t0 = time.perf_counter()
host_cube = cube.cpu().numpy()
t_down = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
host_err = []
for f in range(2):
    tf = np.transpose(host_cube[..., f], (2, 0, 1))       # the file's order
    host_err.append(R.numpy_path(tf, S, TE, methods[f])
                    - true[f].cpu().numpy())
t_host_rc = (time.perf_counter() - t0) * 1e3
out = be.recoarsen(cube, 'cube', [0, 1], methods, S, TE, true=true)
for f in range(2):
    # (the cube's feature plane is not a time-first file: numpy's order on it
    # is the fixed order only within the counted bound, see NOTES.md)
    d = np.abs(out[f][1].cpu().numpy() - host_err[f]).max()
    assert d <= (S * S + TE) * 2.0 ** -24 * np.abs(host_cube).max(), d
(o_tf,) = be.recoarsen(tfirst, 'tfirst', [0], ['average'], S, TE,
                       true=true[:1])
assert torch.equal(o_tf[1], out[0][1]), 'layouts differ'
host_plane = host_cube[..., 0]
t_host_dd, want_dd = host_ms(lambda: R.direct_dist(host_plane), reps=1)
t_host_gd, want_gd = host_ms(lambda: R.gradient_dist(host_plane), reps=1)
for name, want in (('direct_dist', want_dd), ('gradient_dist', want_gd)):
    got = getattr(qa, name)(plane)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert abs(got[2] - want[2]) <= 3e-6 * want[2], (got[2], want[2])
src0 = true[0].cpu().numpy()
t_host_fs, want_fs = host_ms(lambda: R.frequency_spectrum(
    src0.astype(np.float64)), reps=1)
got_fs = qa.frequency_spectrum(true[0])
assert np.abs(got_fs[1] - want_fs[1]).max() <= 1e-5 * want_fs[1].max()
del host_cube, host_plane
say('device results agree with the host route')

# ---- timings
scratch = torch.empty_like(cube)
syn = [torch.empty_like(t) for t in true]
err = [torch.empty_like(t) for t in true]
words = torch.empty((2, 5), dtype=torch.float64, device=dev.torch_device)
codes = [_lib.TC_METHODS[m] for m in methods]


def launch(hr, layout, n):
    be.launch_recoarsen(hr, layout, [0, 1][:n], codes[:n], S, TE, true[:n],
                        syn[:n], err[:n], words)


sp = torch.empty_like(tfirst)
sl = torch.empty_like(true[0])
say('| pass | ms | bytes read | TB/s | of 8 TB/s | note |')
say('|---|---|---|---|---|---|')
ms, _ = device_ms(lambda: launch(cube, 'cube', 2))
row('s3_qa_recoarsen cube, 2 features', ms, n_cube, 'syn + err + summary')
ms_c, _ = device_ms(lambda: scratch.copy_(cube))
row('copy_ of the cube', ms_c, n_cube, 'reads and writes these bytes')
ms, _ = device_ms(lambda: launch(tfirst, 'tfirst', 1))
row('s3_qa_recoarsen time-first, 1 feature', ms, n_plane,
    'syn + err + summary')
ms_p, _ = device_ms(lambda: sp.copy_(tfirst))
row('copy_ of the field', ms_p, n_plane, 'reads and writes these bytes')
ms_dd, _ = host_ms(lambda: qa.direct_dist(plane))
row('direct_dist, whole', ms_dd / 6, n_plane,
    f'{ms_dd:.3f} ms for 6 reads of the field, 3 read-backs')
ms_gd, _ = host_ms(lambda: qa.gradient_dist(plane))
row('gradient_dist, whole', ms_gd / 6, 2 * n_plane,
    f'{ms_gd:.3f} ms for 6 passes, two loads per value')
ms_fs, _ = host_ms(lambda: qa.frequency_spectrum(true[0]))
ms_l, _ = device_ms(lambda: sl.copy_(true[0]))
row('frequency_spectrum of a source feature', ms_fs, true[0].numel() * 4,
    f'copy_ of it {ms_l:.4f} ms')
say(f'host route: download of the cube {t_down:.0f} ms; re-coarsen + error '
    f'of 2 features {t_host_rc:.0f} ms; direct_dist {t_host_dd:.0f} ms; '
    f'gradient_dist {t_host_gd:.0f} ms; frequency_spectrum (float64) '
    f'{t_host_fs:.0f} ms')
