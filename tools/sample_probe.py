"""Cost of drawing one raw training batch, at the C2 and the C1 training shape,
three ways in ONE process:

(a) ``s3_sample_gather`` out of the resident cube (sup3r_amd/samplers.py);
(b) a ``torch`` device-to-device ``copy_`` of as many bytes as (a) writes;
(c) the host route it replaces: numpy slices of the cube, ``np.stack``,
    ``Device.to_device``.

(a) and (b) are timed with device events around back-to-back calls after a
warm-up, two alternating passes; (c) with the host clock around calls that end
in a device synchronise.  (a) cycles through pre-drawn sets of origins and (b)
through several buffer pairs, so that no call finds its source in a cache.
Usage: python tools/sample_probe.py [--small]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))
import torch  # noqa: E402
from sup3r_amd.engine import Device  # noqa: E402
from sup3r_amd.samplers import DeviceSampler, sample_gather  # noqa: E402

small = '--small' in sys.argv
# name, cube, box, batch size, channels kept
SHAPES = [('C2', (120, 120, 8760, 4), (80, 80, 288), 8, [0, 1]),
          ('C1', (100, 100, 8760, 2), (10, 10, 1), 15, [0, 1])]
if small:
    SHAPES = [('C2 (small)', (30, 30, 400, 4), (20, 20, 48), 8, [0, 1]),
              ('C1 (small)', (20, 20, 400, 2), (10, 10, 1), 15, [0, 1])]
N_SETS = 16                                      # pre-drawn batches of origins
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
            return ms / reps, reps
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


print('| shape | batch | out MB | (a) gather ms | (b) copy ms | (c) host route'
      ' ms | (a) / (b) | (c) / (a) | (a) GB/s read + written |')
print('|---|---|---|---|---|---|---|---|---|')
for name, cube_shape, box, batch, channels in SHAPES:
    feats = [f'f{i}' for i in range(cube_shape[3])]
    cube_d = torch.randn(cube_shape, dtype=torch.float32,
                         device=dev.torch_device)
    cube_h = cube_d.cpu().numpy()
    smp = DeviceSampler(cube_d, feats, box, batch_size=batch, seed=0,
                        feature_sets={'features': [feats[c] for c in channels]})
    del cube_d
    cube_d = smp.data
    sets = []
    for _ in range(N_SETS):
        sets.append(smp._origins(smp._batch_indices(), box[2], batch))
    s1, s2, t = box

    def gather(i):
        return sample_gather(dev, cube_d, sets[i % N_SETS], box, channels)

    def host_route(i):
        org = sets[i % N_SETS]
        raw = np.stack([cube_h[a:a + s1, b:b + s2, k:k + t][..., channels]
                        for a, b, k in org])
        return dev.to_device(raw)

    got, want = gather(3), host_route(3)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), name
    out_bytes = got.numel() * 4
    read_bytes = batch * s1 * s2 * t * cube_shape[3] * 4    # whole runs
    # enough source / destination pairs that a copy does not find its source
    # in the 256 MiB Infinity Cache either
    n_pairs = int(min(8, max(1, -(-600e6 // (2 * out_bytes)))))
    pairs = [(torch.randn(got.numel(), dtype=torch.float32,
                          device=dev.torch_device),
              torch.empty(got.numel(), dtype=torch.float32,
                          device=dev.torch_device)) for _ in range(n_pairs)]

    def copy(i):
        src, dst = pairs[i % n_pairs]
        dst.copy_(src)

    ms_a, ms_b = [], []
    for _ in range(2):                           # alternating: drift shows
        ms_a.append(device_ms(gather))
        ms_b.append(device_ms(copy))
    ms_c = host_ms(host_route, 3 if not small and name == 'C2' else 20)
    # index arithmetic + launch as the queue pays them: next(sampler)
    ms_next = host_ms(lambda i: next(smp), 200)
    a, b = min(m for m, _ in ms_a), min(m for m, _ in ms_b)
    print(f'| {name} {cube_shape} | {batch} x {box} x {len(channels)} | '
          f'{out_bytes / 1e6:.3f} | '
          f'{ms_a[0][0]:.4f} / {ms_a[1][0]:.4f} ({ms_a[1][1]} calls) | '
          f'{ms_b[0][0]:.4f} / {ms_b[1][0]:.4f} ({ms_b[1][1]} calls) | '
          f'{ms_c:.3f} | {a / b:.2f} | {ms_c / a:.0f} | '
          f'{(read_bytes + out_bytes) / a / 1e6:.0f} |')
    print(f'{name}: next(sampler) back to back, host clock, synchronised at '
          f'the end: {ms_next:.4f} ms per batch; the gather reads '
          f'{read_bytes / 1e6:.3f} MB (whole runs of {cube_shape[3]} channels)'
          f' and writes {out_bytes / 1e6:.3f} MB, the copy reads and writes '
          f'{out_bytes / 1e6:.3f} MB ({n_pairs} buffer pairs in turn)')
    del cube_d, cube_h, smp, pairs, got, want
    torch.cuda.empty_cache()
