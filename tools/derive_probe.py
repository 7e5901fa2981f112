"""What deriving features costs on one MI355X (``sup3r_amd.derive``).

``s3_level_interp`` at a month of hourly data on a (60, 60, 744) grid with 37
levels, in two cases — u and v to three heights (one launch, six planes), and
one variable to one height — against
  * ``copy_`` of the same input + output bytes: the yardstick for a share of
    the memory bandwidth (a copy reads half of them and writes half);
  * a lane-per-column kernel with a single target (tools/probes/
    derive_naive.hip, for this probe only): what the staging through LDS buys;
  * the host route for the same request: ``NumpyBackend`` (vectorised numpy),
    and for the single request ``tests/derive_ref.py`` (the reference's masked
    passes restated).
Then the pointwise, flag and stack kernels at (60, 60, 744), C = 6.

Device events around back-to-back calls after a warm-up, ``--reps`` windows
each; the median and the spread (min .. max) are printed, and one JSON line
at the end.  The bytes are the algorithm's, from the shapes: every input
element once, every output once.

Usage: python tools/derive_probe.py [--small] [--reps N] [--no-host]"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import torch  # noqa: E402
from sup3r_amd import derive as D  # noqa: E402
from tests import derive_ref as R  # noqa: E402

PEAK = 8e12                                      # HBM3E bytes / s
small = '--small' in sys.argv
host = '--no-host' not in sys.argv
reps = int(sys.argv[sys.argv.index('--reps') + 1]) if '--reps' in sys.argv \
    else 5
SHAPE, L = ((12, 12, 48), 37) if small else ((60, 60, 744), 37)
HEIGHTS = [40.0, 100.0, 160.0]


def windows(fn, n=20, warm=3):
    """ms per call: ``reps`` windows of n calls between device events"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / n)
    return out


def report(name, ms, nbytes=None):
    med = float(np.median(ms))
    row = {'name': name, 'ms': med, 'ms_min': float(min(ms)),
           'ms_max': float(max(ms))}
    text = f'{name:44s} {med:8.3f} ms  ({min(ms):.3f} .. {max(ms):.3f})'
    if nbytes:
        row['bytes'] = int(nbytes)
        row['tb_s'] = nbytes / med / 1e9
        text += (f'  {nbytes / 1e6:8.1f} MB  {row["tb_s"]:.2f} TB/s '
                 f'({100 * nbytes / med / 1e-3 / PEAK:.0f} % of 8 TB/s)')
    print(text, flush=True)
    return row


def naive_lib():
    so = os.path.join(HERE, 'probes', 'derive_naive.so')
    src = os.path.join(HERE, 'probes', 'derive_naive.hip')
    if not os.path.exists(so):
        subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'),
                        '--offload-arch=gfx950', '-O3', '-shared', '-fPIC',
                        src, '-o', so], check=True)
    lib = C.CDLL(so)
    lib.naive_level_interp.restype = C.c_int
    lib.naive_level_interp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int64, C.c_int, C.c_float,
                                       C.c_void_p, C.c_int]
    return lib


def main():
    be = D.DeviceBackend()
    dev = be.dev.torch_device
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator(device=dev).manual_seed(0)
    s1, s2, t = SHAPE
    P = s1 * s2 * t
    topo = torch.rand((s1, s2), generator=g, device=dev) * 50
    hgt = torch.sort(torch.rand((s1, s2, t, L), generator=g, device=dev)
                     * 3000 + 12, dim=-1).values
    zg = (hgt + topo[..., None, None]).contiguous()
    del hgt
    u = torch.randn((s1, s2, t, L), generator=g, device=dev) * 8
    v = torch.randn((s1, s2, t, L), generator=g, device=dev) * 8
    rows = []
    plane, col = 4 * P, 4 * P * L

    # ---- s3_level_interp
    out6 = [[be.dev.empty(SHAPE) for _ in HEIGHTS] for _ in range(2)]
    out1 = [[be.dev.empty(SHAPE)]]
    lev = ('column', zg, topo)
    cases = [('level_interp u, v -> 3 heights', [u, v], HEIGHTS, out6),
             ('level_interp u -> 1 height', [u], HEIGHTS[:1], out1)]
    for name, vs, hs, out in cases:
        nbytes = col * (1 + len(vs)) + plane * len(vs) * len(hs) + 4 * s1 * s2
        rows.append(report(name, windows(
            lambda: be.level_interp(lev, vs, [], [], hs, out=out)), nbytes))
        n = nbytes // 8
        src = torch.empty(n, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        rows.append(report(f'  copy_ of {nbytes / 1e6:.0f} MB read + written',
                           windows(lambda: dst.copy_(src)), 8 * n))
        del src, dst
    # the lane-per-column shape, one target, no topography (its levels: zg)
    lib = naive_lib()
    stream = torch.cuda.current_stream().cuda_stream
    naive_out = be.dev.empty(SHAPE)
    grid = min((P + 255) // 256, num_cu * 8)
    rc = []

    def naive():
        rc.append(lib.naive_level_interp(
            C.c_void_p(stream), C.c_void_p(zg.data_ptr()),
            C.c_void_p(u.data_ptr()), P, L, HEIGHTS[0] + 25,
            C.c_void_p(naive_out.data_ptr()), grid))
    rows.append(report('  lane per column, u -> 1 height', windows(naive),
                       2 * col + plane))
    assert not any(rc)
    staged = be.level_interp(('column', zg, None), [u], [], [],
                             [HEIGHTS[0] + 25])[0][0]
    same = bool(torch.equal(staged, naive_out))
    print(f'  lane per column == staged kernel, bitwise: {same}')
    assert same

    # ---- the host route for the same requests
    if host:
        nb = D.NumpyBackend()
        h = {k: x.cpu().numpy() for k, x in
             (('zg', zg), ('topo', topo), ('u', u), ('v', v))}
        for name, vs, hs in (('u, v -> 3 heights', ['u', 'v'], HEIGHTS),
                             ('u -> 1 height', ['u'], HEIGHTS[:1])):
            t0 = time.perf_counter()
            got = nb.level_interp(('column', h['zg'], h['topo']),
                                  [h[k] for k in vs], [], [], hs)
            ms = 1e3 * (time.perf_counter() - t0)
            rows.append(report(f'  host NumpyBackend {name}', [ms]))
        assert np.array_equal(got[0][0], out1[0][0].cpu().numpy())
        t0 = time.perf_counter()
        ref = R.interp_to_level(h['zg'] - h['topo'][..., None, None], h['u'],
                                np.float32(HEIGHTS[0]))
        ms = 1e3 * (time.perf_counter() - t0)
        rows.append(report('  host derive_ref (masked passes) u -> 1 height',
                           [ms]))
        assert np.array_equal(ref, got[0][0])
        del h, got, ref

    # ---- pointwise, flags, stack at (60, 60, 744), C = 6
    del zg, u, v
    ll = R.grid(s1, s2)
    theta = be._theta(ll)
    a = torch.rand(SHAPE, generator=g, device=dev) * 20
    b = torch.rand(SHAPE, generator=g, device=dev) * 360
    flags = torch.zeros(t, dtype=torch.int32, device=dev)
    from sup3r_amd import _lib
    pw = [('uv_from_wswd', _lib.DP_UV_FROM_WSWD, 2, 2),
          ('wswd_from_uv', _lib.DP_WSWD_FROM_UV, 2, 2),
          ('surface_rh', _lib.DP_SURFACE_RH, 2, 1),
          ('ratio_masked', _lib.DP_RATIO_MASKED, 2, 1),
          ('scale', _lib.DP_SCALE, 1, 1)]
    for name, op, n_in, n_out in pw:
        rows.append(report(f'pointwise {name}', windows(
            lambda: be.pointwise(op, SHAPE, a, b if n_in > 1 else None,
                                 theta=theta, flags=flags, p0=1.5,
                                 n_out=n_out)), plane * (n_in + n_out)))
    rows.append(report('time_flags le, one plane', windows(
        lambda: be.time_flags(a, 'le', 1.0)), plane))
    planes = [torch.rand(SHAPE, generator=g, device=dev) for _ in range(6)]
    rows.append(report('stack_features C = 6, roll 5', windows(
        lambda: be.stack(planes, 5)), 12 * plane))
    cube = be.stack(planes, 5)
    rows.append(report('time_flags nan, cube C = 6', windows(
        lambda: be.time_flags(cube, 'nan')), 6 * plane))
    print(json.dumps({'derive_probe': rows, 'shape': list(SHAPE), 'L': L,
                      'num_cu': num_cu, 'reps': reps}))


if __name__ == '__main__':
    main()
