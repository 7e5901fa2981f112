"""Device bias correction at the two production forward-pass shapes
(examples/sup3rwind/run_configs/wind/config_fwp_spatial.json: chunk (75, 75,
48) x 14 features, monthly_local_linear_bc; examples/sup3rcc/run_configs/
nearsurf/config_fwp_step1.json: chunk (54, 54, 43) x 10 features,
local_qdm_bc, Q = 101, 24 windows).  Three measurements, all in ONE process:

1. kernel time of ``s3_bias_correct`` on a batch of 8 padded chunks (device
   events around the bare C-ABI call, descriptors prepared once; the
   wrapper's host preparation is printed next to it; run it alone under
   ``rocprofv3 --kernel-trace --stats -- python tools/bias_probe.py
   --kernel-only`` for the trace), with the algorithmic
   bytes — the batch read and written once plus every touched table row once —
   as a share of 8 TB/s;
2. the host cost it replaces: ``tests/bias_ref.py`` per chunk (vectorised
   numpy; the reference's QDM is a Python loop over sites in ``rex`` and far
   slower, so this understates the gain);
3. end-to-end chunks/s of the executor, alternating and repeated: (a) device
   correction, (b) the same executor fed chunks corrected on the host by the
   restatement, (c) no correction.  The generator is two small convolutions,
   so that the input stage is visible.

Usage: python tools/bias_probe.py [--small] [--kernel-only] [--reps N]"""
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
import pandas as pd  # noqa: E402
import torch  # noqa: E402
from sup3r_amd import ForwardPass, Sup3rGan  # noqa: E402
from sup3r_amd import _lib  # noqa: E402
from sup3r_amd import bias as B  # noqa: E402
from sup3r_amd.configs.author_configs import pcc  # noqa: E402
from sup3r_amd.forward_pass import register_model  # noqa: E402
from sup3r_amd.strategy import ArrayStrategy  # noqa: E402
from tests import bias_ref as R  # noqa: E402

PEAK = 8e12                                      # HBM3E bytes / s
small = '--small' in sys.argv
kernel_only = '--kernel-only' in sys.argv
reps = int(sys.argv[sys.argv.index('--reps') + 1]) if '--reps' in sys.argv \
    else 3
CFG = os.path.join(os.path.dirname(__file__), '..', 'sup3r_amd', 'configs')
rng = np.random.default_rng(0)


def shapes(name):
    """(chunk shape, features, chunks of the domain along s1, s2, t)"""
    if name == 'linear':
        return ((12, 12, 8) if small else (75, 75, 48)), 14, (2, 2, 4)
    return ((10, 10, 7) if small else (54, 54, 43)), 10, (2, 2, 4)


def setup(name):
    chunk, n_f, grid = shapes(name)
    dom = tuple(c * g for c, g in zip(chunk, grid))
    feats = [f'f{i}' for i in range(n_f)]
    if name == 'linear':
        # hourly: 192 steps from Jan 29 straddle the month boundary
        ti = pd.date_range('2015-01-29', periods=dom[2], freq='1h')
        fp = {}
        for f in feats:
            fp.update(R.seeded_linear_tables(rng, dom[:2], feature=f))
        kw = {f: dict(bias_fp=fp, temporal_avg=True) for f in feats}
        method = 'monthly_local_linear_bc'
        data = rng.standard_normal(dom + (n_f,)).astype(np.float32)
    else:
        # daily: the 24 windows are 15.2 days wide, a 43 + 2 day chunk spans
        # two or three of them
        ti = pd.date_range('2015-01-01', periods=dom[2], freq='1D')
        W, Q = (4, 21) if small else (24, 101)
        tabs = [np.cumsum(rng.uniform(0.05, 1.0, dom[:2] + (W, Q)),
                          axis=-1).astype(np.float32) + off
                for off in (1.0, 1.5, 2.0)]
        fp = {'time_window_center': (np.arange(W) + 0.5) * 365.0 / W}
        for f in feats:
            # (one host copy for all features; each gets its own device copy)
            fp[f'base_{f}_obs_params'], fp[f'bias_{f}_params'], \
                fp[f'bias_fut_{f}_params'] = tabs
        kw = {f: dict(bias_fp=fp, base_dset=f'{f}_obs', relative=True)
              for f in feats}
        method = 'local_qdm_bc'
        data = rng.uniform(2.0, 50.0, dom + (n_f,)).astype(np.float32)
    return chunk, feats, dom, ti, method, kw, data


def device_ms(fn, n=30, warm=3):
    for _ in range(warm):
        fn()
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def kernel(name):
    chunk, feats, dom, ti, method, kw, data = setup(name)
    bc = B.DeviceBiasCorrection(method, kw, feats)
    pad = ((1, 0), (1, 0), (1, 1))
    n = 8
    # 8 padded chunks: the 2 x 2 spatial windows of two time chunks
    wins, xs = [], []
    for k in range(n):
        a, b, c = k % 2, (k // 2) % 2, k // 4
        sl = tuple(slice(i * e, (i + 1) * e) for i, e in zip((a, b, c),
                                                             chunk))
        wins.append(B.ChunkWindow(sl[:2], pad, ti[sl[2]]))
        xs.append(np.pad(data[sl], pad + ((0, 0),), mode='reflect'))
    x = bc.dev.to_device(np.stack(xs))
    out = bc.dev.empty(x.shape)
    mean = np.linspace(0.1, 1.0, len(feats)).astype(np.float32)
    std = np.linspace(1.0, 2.0, len(feats)).astype(np.float32)

    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        # descriptors, index buffers and geometry once: the events bracket
        # nothing but back-to-back s3_bias_correct calls
        hold = []
        calls, _, counts = bc.prepare(x, wins, out=out, mean=mean, std=std,
                                      keep=hold)
        L, ctx = _lib.lib(), bc.dev.ctx

        def run():
            for args in calls:
                _lib.check(L.s3_bias_correct(ctx, *args), ctx,
                           's3_bias_correct')
        ms = [device_ms(run) for _ in range(2)]
        # the wrapper's host cost per batch (planning + the small upload),
        # a figure of its own
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            bc.prepare(x, wins, out=out, mean=mean, std=std, counts=counts)
        host_prep = (time.perf_counter() - t0) / 20 * 1e3
    assert not counts.cpu().numpy().any()
    npix = n * x.shape[1] * x.shape[2]
    chunk_bytes = 2 * x.numel() * 4
    if name == 'linear':
        rows = npix * len(feats) * 2 * 2 * 4       # 2 tables x 2 months x 4 B
        what = 'scalar + adder of the 2 touched months per pixel and feature'
    else:
        Q = bc.features[0].n_q
        pix = x.shape[1] * x.shape[2]
        touched = [len(set(B.window_index(w.time_index,
                                          bc.features[0].centers)))
                   for w in wins]
        rows = pix * sum(touched) * len(feats) * 3 * Q * 4
        what = (f'3 rows of {Q * 4} B per touched window, pixel and feature; '
                f'windows touched per chunk {touched}')
    best = min(ms)
    print(f'[kernel] {name}: batch {tuple(x.shape)}, s3_bias_correct device '
          f'ms (events, two passes) {ms[0]:.4f} / {ms[1]:.4f}; host '
          f'preparation of a batch {host_prep:.3f} ms')
    print(f'[kernel] {name}: algorithmic bytes = batch read + written '
          f'{chunk_bytes / 1e6:.1f} MB + table rows {rows / 1e6:.1f} MB '
          f'({what}) -> {(chunk_bytes + rows) / best / 1e9:.3f} TB/s = '
          f'{(chunk_bytes + rows) / best / 1e-3 / PEAK:.1%} of 8 TB/s; '
          f'{best / n:.4f} ms per chunk')


def end_to_end(name):
    chunk, feats, dom, ti, method, kw, data = setup(name)
    Sup3rGan.seed(0)
    means = {f: np.float32(0.1 * i) for i, f in enumerate(feats)}
    stds = {f: np.float32(1.0 + 0.1 * i) for i, f in enumerate(feats)}
    m = Sup3rGan(pcc(3, 16) + pcc(3, 2, act=False),
                 os.path.join(CFG, 'disc_st.json'), means=means, stdevs=stds,
                 precision='bf16')
    m.set_model_params(lr_features=feats, hr_out_features=feats[:2],
                       s_enhance=1, t_enhance=1)
    key = {'model_dir': f'bias-probe-{name}'}
    register_model('Sup3rGan', key, m)
    args = dict(fwp_chunk_shape=chunk, spatial_pad=1, temporal_pad=1, model=m)

    def strategy(corrected):
        extra = dict(bias_correct_method=method, bias_correct_kwargs=kw,
                     input_time_index=ti) if corrected else {}
        return ArrayStrategy(data, key, **args, **extra)

    # (2) host cost of the restatement per chunk
    st = strategy(False)
    t0 = time.perf_counter()
    n_host = min(4, st.n_chunks)
    for i in range(n_host):
        R.correct_chunk(st.init_chunk(i), method, kw, feats, ti)
    host_ms = (time.perf_counter() - t0) / n_host * 1e3
    print(f'[host] {name}: tests/bias_ref.py {host_ms:.1f} ms per chunk '
          f'{chunk} x {len(feats)} features (vectorised numpy; understates '
          'the reference, whose QDM loops over sites in Python)')

    def route_device():
        return ForwardPass.run(strategy(True), 0, batch=8)

    def route_none():
        return ForwardPass.run(strategy(False), 0, batch=8)

    def route_host():
        s0 = strategy(False)
        fwp = ForwardPass(s0, 0)

        def chunks():
            for i in range(s0.n_chunks):
                c = s0.init_chunk(i)
                c.input_data = R.correct_chunk(c, method, kw, feats, ti)
                c.input_data, c.exo_data = fwp.pad_source_data(
                    c.input_data, c.pad_width, c.exo_data)
                yield c
        return sum(1 for _ in ForwardPass.iter_chunks(
            chunks(), m, batch=8, return_data=False))
    routes = (('(a) device correction', route_device),
              ('(b) host restatement', route_host),
              ('(c) no correction', route_none))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for _, fn in routes:                      # warm-up: plans, tables
            fn()
        rate = {r: [] for r, _ in routes}
        for _ in range(reps):
            for r, fn in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = fn()
                torch.cuda.synchronize()
                rate[r].append(n / (time.perf_counter() - t0))
    for r, _ in routes:
        print(f'[e2e] {name} {r}: chunks/s ' +
              ' / '.join(f'{v:.1f}' for v in rate[r]) +
              f' (median {np.median(rate[r]):.1f})')


for which in ('linear', 'qdm'):
    kernel(which)
    if not kernel_only:
        end_to_end(which)
