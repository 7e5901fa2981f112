"""Cost of one ``SolarMultiStepGan.generate`` on a production-like chunk —
daily low-res ``(T = 5, 40 x 40)`` with (clearsky_ratio, U_200m, V_200m), the
shipped 2x spatial specs and the shipped ``gen_solar_1x_8x_1f`` temporal spec —
by the device route and by the host route of the same commit, and the device
time of the two kernels of the device route beside the bytes they move.

Two steps, each its own process (run each under its own ``timeout``):

    python tools/solar_probe.py generate
    python tools/solar_probe.py kernels

``generate``: host clock around calls (either route ends in the download of
the result), a warm-up, then the two routes in turn; medians.  ``kernels``:
device events around back-to-back calls after a warm-up, cycling through
several buffer sets so that no call finds its source in a cache; median of
five windows; at the chunk's own shape (a few hundred KB: launch bound) and at
a shape large enough to show the rate."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(__file__), '..')
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from sup3r_amd import MultiStepGan, SolarMultiStepGan, Sup3rGan  # noqa: E402
from sup3r_amd import _lib  # noqa: E402
from sup3r_amd.engine import Device  # noqa: E402

CFG = os.path.join(ROOT, 'sup3r_amd', 'configs')
CSR, WIND = ['clearsky_ratio'], ['U_200m', 'V_200m']
MEANS = {'clearsky_ratio': 0.7, 'U_200m': 4.2, 'V_200m': 5.6}
STDS = {'clearsky_ratio': 0.04, 'U_200m': 1.1, 'V_200m': 1.3}
T, S = 5, 40
HBM = 8e12                                              # bytes / s
PF = C.POINTER(C.c_float)


def gan(gen, disc, lr, out, s, t, lr_shape, seed):
    Sup3rGan.seed(seed)
    feats = set(lr) | set(out)
    m = Sup3rGan(os.path.join(CFG, 'sup3r', gen), os.path.join(CFG, disc),
                 means={f: np.float32(MEANS[f]) for f in feats},
                 stdevs={f: np.float32(STDS[f]) for f in feats})
    m.set_model_params(lr_features=lr, hr_out_features=out, s_enhance=s,
                       t_enhance=t)
    hr = (lr_shape[0],) + tuple(
        d * (s if i < 2 else t) for i, d in enumerate(lr_shape[1:-1])) + (
        len(out),)
    m.init_weights(lr_shape, hr)
    return m


def step_generate():
    ms = SolarMultiStepGan(
        MultiStepGan([gan('spatial/gen_2x_1f.json', 'test_disc_s_same.json',
                          CSR, CSR, 2, 1, (T, S, S, 1), 1)]),
        MultiStepGan([gan('spatial/gen_2x_2f.json', 'test_disc_s_same.json',
                          WIND, WIND, 2, 1, (T, S, S, 2), 2)]),
        MultiStepGan([gan('sup3rcc/gen_solar_1x_8x_1f.json',
                          'test_disc_st_same.json', CSR + WIND, CSR, 1, 8,
                          (1, 2 * S, 2 * S, T, 3), 3)]))
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((T, S, S, 3)).astype(np.float32) *
         np.array([0.04, 1.1, 1.3], np.float32) +
         np.array([0.7, 4.2, 5.6], np.float32))
    assert ms._device_blocker(x, None, None) is None
    a, b = ms.generate(x, device=True), ms.generate(x, device=False)
    assert a.shape == (1, 2 * S, 2 * S, 8 * T, 1) and np.array_equal(a, b)
    for _ in range(3):
        ms.generate(x, device=True)
        ms.generate(x, device=False)
    ms_dev, ms_host = [], []
    for _ in range(15):
        for route, sink in ((True, ms_dev), (False, ms_host)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ms.generate(x, device=route)
            sink.append((time.perf_counter() - t0) * 1e3)
    res = {'step': 'generate', 'chunk': [T, S, S, 3],
           'out': list(a.shape), 'calls': len(ms_dev),
           'device_ms_median': statistics.median(ms_dev),
           'device_ms_min': min(ms_dev), 'device_ms_max': max(ms_dev),
           'host_ms_median': statistics.median(ms_host),
           'host_ms_min': min(ms_host), 'host_ms_max': max(ms_host)}
    res['host_over_device'] = res['host_ms_median'] / res['device_ms_median']
    print(json.dumps(res))


def device_us(fn, window_s=0.1, windows=5):
    """median over ``windows`` of the us per call inside a window of
    back-to-back calls bracketed by device events, after a warm-up"""
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    for i in range(10):
        fn(i)
    torch.cuda.synchronize()
    reps, out = 50, []
    while len(out) < windows:
        a.record()
        for i in range(reps):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms < window_s * 1e3 and reps < 20000:
            reps = min(20000, reps * 4)
            continue
        out.append(ms * 1e3 / reps)
    return statistics.median(out), reps


def step_kernels():
    dev, L = Device.get(), _lib.lib()
    f32 = np.float32
    sc1, sh1 = np.array([0.04], f32), np.array([0.7], f32)
    sc2, sh2 = np.array([1.1, 1.3], f32), np.array([4.2, 5.6], f32)
    mu, sd = np.array([0.7, 4.2, 5.6], f32), np.array([0.04, 1.1, 1.3], f32)

    def ptr(a):
        return a.ctypes.data_as(PF)

    def vp(t):
        return C.c_void_p(t.data_ptr())
    one, two = (C.c_int32 * 1)(0), (C.c_int32 * 2)(0, 1)
    for name, (t, h, w), t_out, pad in (
            ('the chunk', (T, 2 * S, 2 * S), 8 * T, 0),
            ('the chunk, t_enhance 10', (T, 2 * S, 2 * S), 8 * T, 5),
            ('large', (24, 400, 400), 192, 0)):
        n_join = t * h * w * 3 * 4                      # bytes either way
        n_sets = int(min(8, max(2, -(-600e6 // (2 * n_join)))))
        sets = [(torch.randn((t, h, w, 1), device=dev.torch_device),
                 torch.randn((t, h, w, 2), device=dev.torch_device),
                 dev.empty((1, h, w, t, 3))) for _ in range(n_sets)]

        def join(i):
            ya, yb, x = sets[i % n_sets]
            rc = L.s3_branch_join(
                dev.ctx, vp(ya), 1, one, 1, ptr(sc1), ptr(sh1), vp(yb), 2,
                two, 2, ptr(sc2), ptr(sh2), t, h, w, ptr(mu), ptr(sd), vp(x))
            assert rc == 0
        us, reps = device_us(join)
        print(json.dumps({
            'step': 'kernels', 'kernel': 's3_branch_join', 'case': name,
            'thw': [t, h, w], 'channels': '1 + 2 -> 3',
            'bytes_read_written': 2 * n_join, 'us': us, 'calls': reps,
            'buffer_sets': n_sets, 'GBps': 2 * n_join / us / 1e3,
            'fraction_of_8TBps': 2 * n_join / (us * 1e-6) / HBM}))
        del sets
        outer = h * w
        n_rd, n_wr = outer * t_out * 4, outer * (t_out + 2 * pad) * 4
        n_sets = int(min(8, max(2, -(-600e6 // (n_rd + n_wr)))))
        sets = [(torch.randn((outer, t_out, 1), device=dev.torch_device),
                 dev.empty((outer, t_out + 2 * pad, 1)))
                for _ in range(n_sets)]

        def padk(i):
            y, out = sets[i % n_sets]
            rc = L.s3_time_pad_reflect(dev.ctx, vp(y), outer, t_out, 1, pad,
                                       ptr(sc1), ptr(sh1), vp(out))
            assert rc == 0
        us, reps = device_us(padk)
        print(json.dumps({
            'step': 'kernels', 'kernel': 's3_time_pad_reflect', 'case': name,
            'outer_t_c_pad': [outer, t_out, 1, pad],
            'bytes_read_written': n_rd + n_wr, 'us': us, 'calls': reps,
            'buffer_sets': n_sets, 'GBps': (n_rd + n_wr) / us / 1e3,
            'fraction_of_8TBps': (n_rd + n_wr) / (us * 1e-6) / HBM}))
        del sets
        torch.cuda.empty_cache()


if __name__ == '__main__':
    step = sys.argv[1] if len(sys.argv) > 1 else ''
    if step == 'generate':
        step_generate()
    elif step == 'kernels':
        step_kernels()
    else:
        sys.exit(__doc__)
