"""GPU tests (``-m gpu``) of the device-resident samplers: ``s3_sample_gather``
against numpy slicing of the same cube, bit for bit (every comparison is made
on ``uint32`` views: the cubes are random BIT PATTERNS, NaNs of every kind
included); the batch queues over device samplers against the same queues over
host samplers that replay the draws; ``Sup3rGanDC`` trained from a
``DeviceBatchHandlerDC``."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), '..', 'sup3r_amd', 'configs')
EINVAL = -1
PAD = 64                       # sentinel floats in front of and behind `out`
SENTINEL = 0x5A5AC3C3
# quiet NaN with a payload, signalling NaN, negative NaN, +inf, -inf, -0.0
SPECIALS = np.array([0x7FC00001, 0x7F800001, 0xFFC12345, 0x7F800000,
                     0xFF800000, 0x80000000], dtype=np.uint32)


def bit_cube(shape, seed):
    """random 32-bit patterns with the special values planted at the front of
    the first pixel and at the very end of the last"""
    cube = np.random.default_rng(seed).integers(
        0, 2 ** 32, size=shape, dtype=np.uint32)
    flat = cube.reshape(-1)
    flat[:len(SPECIALS)] = SPECIALS
    flat[-len(SPECIALS):] = SPECIALS
    return cube


def on_device(bits):
    """uint32 array -> fp32 device tensor with those bits"""
    import torch
    return torch.from_numpy(bits.view(np.int32)).to('cuda').view(torch.float32)


def raw_gather(cube_d, cube_shape, origins, box, channels, pad=PAD, n=None):
    """one ``s3_sample_gather`` call into a sentinel-filled buffer; returns
    (rc, the whole buffer as uint32, elements of out)"""
    import torch
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    dev, L = Device.get(), _lib.lib()
    org = np.ascontiguousarray(origins, dtype=np.int32).reshape(-1, 3)
    n = len(org) if n is None else n
    ch = np.ascontiguousarray(channels, dtype=np.int32)
    numel = max(n, 1) * int(np.prod(box)) * max(len(ch), 1)
    buf = torch.full((pad + numel + PAD,), SENTINEL, dtype=torch.int32,
                     device=cube_d.device)
    ip = C.POINTER(C.c_int32)
    S1, S2, T, Cc = cube_shape
    rc = L.s3_sample_gather(
        dev.ctx, C.c_void_p(cube_d.data_ptr()), S1, S2, T, Cc,
        org.ctypes.data_as(ip), n, box[0], box[1], box[2],
        ch.ctypes.data_as(ip), len(ch),
        C.c_void_p(buf.data_ptr() + 4 * pad))
    dev.sync()
    return rc, buf.cpu().numpy().view(np.uint32), numel


def np_gather(cube, origins, box, channels):
    s1, s2, t = box
    return np.stack([cube[i:i + s1, j:j + s2, k:k + t][..., channels]
                     for i, j, k in origins])


def check_gather(cube, origins, box, channels, pad=PAD, cube_d=None):
    cube_d = on_device(cube) if cube_d is None else cube_d
    rc, buf, numel = raw_gather(cube_d, cube.shape, origins, box, channels,
                                pad=pad)
    assert rc == 0
    want = np_gather(cube, origins, box, channels)
    assert want.size == numel
    np.testing.assert_array_equal(buf[pad:pad + numel], want.reshape(-1))
    assert (buf[:pad] == SENTINEL).all() and (buf[pad + numel:] == SENTINEL).all()


CHANNEL_MAPS = [[0, 1, 2], [2, 0], [1]]
ORIGINS5 = [(0, 0, 0), (3, 4, 44), (1, 2, 7), (2, 0, 13), (0, 3, 21)]


@pytest.mark.parametrize('channels', CHANNEL_MAPS, ids=str)
@pytest.mark.parametrize('t', [6, 1])
def test_gather_short_runs(t, channels):
    """runs of 18 and of 3 floats: the lane-per-four-outputs kernel; the far
    corner, an odd k0, every channel map"""
    cube = bit_cube((7, 9, 50, 3), seed=t)
    origins = [(i, j, min(k, 50 - t)) for i, j, k in ORIGINS5]
    check_gather(cube, origins, (4, 5, t), channels)


@pytest.mark.parametrize('t', [6, 1])
def test_gather_single_channel_cube(t):
    cube = bit_cube((7, 9, 50, 1), seed=3)
    check_gather(cube, ORIGINS5[:2] + [(1, 2, 7)], (4, 5, t), [0])
    check_gather(cube, [(3, 4, 44)], (4, 5, t), [0, 0, 0])   # one channel thrice


@pytest.mark.parametrize('channels', CHANNEL_MAPS, ids=str)
def test_gather_long_runs_with_misaligned_head_and_tail(channels):
    """runs of 270 floats from k0 = 1 and k0 = 3 (source offsets of 3 and 9
    floats: 12 and 4 bytes past a 16-byte line): the wave-per-pixel kernel,
    more than one 16-byte pass of a wave, peeled head and tail on both sides"""
    cube = bit_cube((3, 3, 400, 3), seed=5)
    check_gather(cube, [(0, 0, 1), (1, 1, 3), (1, 0, 310), (0, 1, 2)],
                 (2, 2, 90), channels)


@pytest.mark.parametrize('shape,box,origins,channels', [
    # a run of 2100 floats: two staged passes (2046 + 54)
    ((2, 3, 800, 3), (2, 2, 700), [(0, 0, 1), (0, 1, 100)], [0, 1, 2]),
    ((2, 3, 800, 3), (2, 2, 700), [(0, 1, 99)], [2, 1]),
    # 128 floats: the shortest run of the wave-per-pixel kernel; 126: the
    # longest of the other
    ((3, 4, 70, 2), (2, 3, 64), [(0, 0, 0), (1, 1, 5), (1, 0, 6)], [0, 1]),
    ((3, 4, 70, 2), (2, 3, 63), [(0, 0, 0), (1, 1, 5), (1, 0, 7)], [1, 0]),
    # 256 channels: passes of 8 time steps; 257: the other kernel again
    ((2, 3, 12, 256), (2, 2, 10), [(0, 0, 1), (0, 1, 2)], [255, 0, 17]),
    ((2, 2, 3, 257), (1, 2, 2), [(0, 0, 1), (1, 0, 0)], [256, 0, 100]),
], ids=['2100', '2100sel', '128', '126', 'c256', 'c257'])
def test_gather_at_the_kernel_thresholds(shape, box, origins, channels):
    check_gather(bit_cube(shape, seed=11), origins, box, channels)


@pytest.mark.parametrize('shape,box', [((7, 9, 50, 3), (2, 2, 3)),
                                       ((3, 3, 400, 3), (1, 2, 50))],
                         ids=['short', 'long'])
@pytest.mark.parametrize('over', [1, 67])
def test_gather_more_origins_than_one_launch_carries(shape, box, over):
    from sup3r_amd import _lib
    n = _lib.SAMPLE_MAX_ORIGINS + over           # 65: 64 + 1; 131: 64 + 64 + 3
    rng = np.random.default_rng(over)
    origins = np.stack([rng.integers(0, d - b + 1, size=n)
                        for d, b in zip(shape[:3], box)], axis=1)
    check_gather(bit_cube(shape, seed=13), origins, box, [2, 1])
    check_gather(bit_cube(shape, seed=13), origins, box, [0, 1, 2])


@pytest.mark.parametrize('shape,box', [((7, 9, 50, 3), (4, 5, 6)),
                                       ((3, 3, 400, 3), (2, 2, 90))],
                         ids=['short', 'long'])
@pytest.mark.parametrize('pad', [65, 66, 67])
def test_gather_into_a_destination_off_the_16_byte_grid(shape, box, pad):
    cube = bit_cube(shape, seed=17)
    origins = [(0, 0, 1), (shape[0] - box[0], shape[1] - box[1],
                           shape[2] - box[2])]
    check_gather(cube, origins, box, [0, 1, 2], pad=pad)
    check_gather(cube, origins, box, [1], pad=pad)


def test_gather_refuses_bad_arguments_before_any_launch():
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    shape, box = (7, 9, 50, 3), (4, 5, 6)
    cube = bit_cube(shape, seed=19)
    cube_d = on_device(cube)
    good = [(0, 0, 0), (3, 4, 44)]
    bad_calls = [
        dict(origins=good + [(4, 4, 44)]),           # one past the edge: rows
        dict(origins=good + [(3, 5, 44)]),           # ... columns
        dict(origins=good + [(3, 4, 45)]),           # ... time
        dict(origins=[(-1, 0, 0)]),
        dict(origins=good, channels=[0, 3]),         # channel == C
        dict(origins=good, channels=[-1]),
        dict(origins=good, n=0),
        dict(origins=good, channels=list(range(3)) * 11),   # 33 channels kept
        dict(origins=good, box=(8, 5, 6)),           # larger than the cube
        dict(origins=good, box=(4, 5, 0)),
    ]
    for call in bad_calls:
        kw = dict(box=box, channels=[0, 1, 2])
        kw.update(call)
        rc, buf, _ = raw_gather(cube_d, shape, kw.pop('origins'), **kw)
        assert rc == EINVAL, call
        assert (buf == SENTINEL).all(), call
        assert _lib.last_error(Device.get().ctx).startswith('sample_gather')
    check_gather(cube, good, box, [0, 1, 2], cube_d=cube_d)   # still in order


def test_gather_offsets_are_64_bit():
    """a box at the far corner of a cube of 2^31 + 2^20 floats (8.6 GB, never
    initialised as a whole): its last pixel lies beyond 2^31 elements"""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < 12 * 2 ** 30:
        pytest.skip(f'needs 12 GB of free device memory, {free / 2 ** 30:.1f}'
                    ' GB are free')
    S1, S2, C_ = 16, 16, 4
    T = (2 ** 31 + 2 ** 20) // (S1 * S2 * C_)
    assert S1 * S2 * T * C_ == 2 ** 31 + 2 ** 20
    big = torch.empty((S1, S2, T, C_), dtype=torch.float32, device='cuda')
    box = (2, 2, 8)
    known = np.random.default_rng(23).integers(
        0, 2 ** 32, size=box + (C_,), dtype=np.uint32)
    # (written through int32 views: no float ever touches the patterns)
    bits = big.view(torch.int32)
    bits[-2:, -2:, -8:, :] = torch.from_numpy(known.view(np.int32)).to('cuda')
    # ... and the same pixels at time 0: the same code below 2^31 elements
    known_low = known[::-1].copy()
    bits[-2:, -2:, :8, :] = torch.from_numpy(
        known_low.view(np.int32)).to('cuda')
    origins = [(S1 - 2, S2 - 2, T - 8), (S1 - 2, S2 - 2, 0)]
    assert ((S1 * S2 - 1) * T + T - 8) * C_ > 2 ** 31
    for channels in ([0, 1, 2, 3], [3, 1]):
        rc, buf, numel = raw_gather(big, (S1, S2, T, C_), origins, box,
                                    channels)
        assert rc == 0
        want = np.stack([known, known_low])[..., channels]
        np.testing.assert_array_equal(buf[PAD:PAD + numel], want.reshape(-1))
        assert (buf[:PAD] == SENTINEL).all()
        assert (buf[PAD + numel:] == SENTINEL).all()
    del big
    torch.cuda.empty_cache()


# ------------------------------------------------------------------- queues
class ReplaySampler:
    """host sampler: numpy slices of a copy of the cube at the origins that the
    documented draws of seed ``seed`` give (fast batches)"""

    def __init__(self, cube, features, sample_shape, batch_size, seed,
                 hr_features_ind):
        self.data, self.features = cube, list(features)
        self.sample_shape = tuple(sample_shape) + (1,) * (3 - len(sample_shape))
        self.batch_size, self.size = batch_size, cube.size
        self.rng = np.random.default_rng(seed)
        self.lr_features = self.features
        self.hr_features_ind = list(hr_features_ind)
        self.hr_features = [self.features[i] for i in self.hr_features_ind]

    def __next__(self):
        (S1, S2, T, _), (s1, s2, t), B = self.data.shape, self.sample_shape, \
            self.batch_size
        i0 = self.rng.integers(0, S1 - s1 + 1)
        j0 = self.rng.integers(0, S2 - s2 + 1)
        k0 = self.rng.integers(0, T - B * t + 1)
        return np.stack([self.data[i0:i0 + s1, j0:j0 + s2,
                                   k0 + m * t:k0 + (m + 1) * t]
                         for m in range(B)])


@pytest.mark.parametrize('sample_shape,t_enhance', [((12, 10, 8), 4),
                                                    ((12, 10), 1)],
                         ids=['5d', '4d'])
def test_queue_over_device_sampler_equals_queue_over_host_sampler(
        sample_shape, t_enhance):
    import torch
    from sup3r_amd import DeviceBatchQueue, DeviceSampler
    feats = ['u_10m', 'v_10m', 'topography']
    cube = np.random.default_rng(29).standard_normal(
        (20, 17, 45, 3)).astype(np.float32)
    kw = dict(batch_size=4, n_batches=3, s_enhance=2, t_enhance=t_enhance,
              seed=0, transform_kwargs={
                  'smoothing': 0.7, 'smoothing_ignore': ['topography'],
                  'temporal_coarsening_method': 'average'})
    dev_smp = DeviceSampler(cube, feats, sample_shape, batch_size=4, seed=31,
                            feature_sets={'lr_only_features': ['topo*']})
    assert list(dev_smp.hr_features_ind) == [0, 1]
    host_smp = ReplaySampler(cube.copy(), feats, sample_shape, 4, 31, [0, 1])
    dev_q = DeviceBatchQueue([dev_smp], **kw)
    host_q = DeviceBatchQueue([host_smp], **kw)
    assert dev_q.device_resident and not host_q.device_resident
    got, want = list(dev_q), list(host_q)
    host_q.stop()
    assert not dev_q.queue_thread.is_alive()
    assert dev_q.queue_thread.ident is None      # never started
    assert len(got) == len(want) == 3
    nd = len(sample_shape) + 2
    for a, b in zip(got, want):
        for name in ('low_res', 'high_res'):
            x, y = getattr(a, name), getattr(b, name)
            assert isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == nd
            np.testing.assert_array_equal(
                x.cpu().numpy().view(np.uint32),
                y.cpu().numpy().view(np.uint32))
        assert a.high_res.shape[-1] == 2 and a.low_res.shape[-1] == 3


def test_dual_queue_members_are_the_numpy_slices():
    import torch
    from sup3r_amd import DeviceDualBatchQueue, DeviceDualSampler
    rng = np.random.default_rng(37)
    s, te, box, B = 2, 3, (4, 6, 6), 3
    lr = rng.standard_normal((6, 7, 20, 3)).astype(np.float32)
    hr = rng.standard_normal((12, 14, 60, 3)).astype(np.float32)
    obs = hr.copy()
    obs[rng.random(obs.shape) < 0.7] = np.nan
    smp = DeviceDualSampler(
        lr, hr, ['u', 'v', 'cape'], ['topo', 'v', 'u'], box, batch_size=B,
        s_enhance=s, t_enhance=te, obs=obs, seed=41,
        feature_sets={'lr_only_features': ['cape'],
                      'hr_exo_features': ['topo']})
    assert smp.hr_features == ['u', 'v', 'topo']
    q = DeviceDualBatchQueue([smp], batch_size=B, n_batches=4, s_enhance=s,
                             t_enhance=te, seed=0)
    replay = np.random.default_rng(41)
    n = 0
    for batch in q:
        i0, j0 = replay.integers(0, 6 - 2 + 1), replay.integers(0, 7 - 3 + 1)
        k0 = replay.integers(0, 20 - B * 2 + 1)
        for m in range(B):
            k = k0 + 2 * m
            want = {
                'low_res': lr[i0:i0 + 2, j0:j0 + 3, k:k + 2],
                'high_res': hr[2 * i0:2 * i0 + 4, 2 * j0:2 * j0 + 6,
                               3 * k:3 * k + 6][..., [2, 1, 0]],
                'obs': obs[2 * i0:2 * i0 + 4, 2 * j0:2 * j0 + 6,
                           3 * k:3 * k + 6][..., [2, 1]]}
            for name, w in want.items():
                x = getattr(batch, name)
                assert isinstance(x, torch.Tensor) and x.is_cuda
                np.testing.assert_array_equal(
                    x[m].cpu().numpy().view(np.uint32),
                    np.ascontiguousarray(w).view(np.uint32))
        assert np.isnan(batch.obs.cpu().numpy()).any()
        n += 1
    assert n == 4 and not q.queue_thread.is_alive()


def test_dual_queue_smooths_4d_low_res_like_the_single_source_queue():
    """4-D dual batches: low_res goes through s3_gaussian_smooth — the same
    call, hence the same bits, as DeviceBatchTransform with s_enhance 1"""
    from sup3r_amd import DeviceDualBatchQueue, DeviceDualSampler
    from sup3r_amd.batch_transform import DeviceBatchTransform
    rng = np.random.default_rng(43)
    lr = rng.standard_normal((9, 8, 12, 2)).astype(np.float32)
    hr = rng.standard_normal((18, 16, 12, 2)).astype(np.float32)
    smp = DeviceDualSampler(lr, hr, ['u', 'v'], ['u', 'v'], (8, 8),
                            batch_size=5, s_enhance=2, t_enhance=1, seed=47)
    kw = {'smoothing': 0.9, 'smoothing_ignore': ['v']}
    q = DeviceDualBatchQueue([smp], batch_size=5, n_batches=1, s_enhance=2,
                             t_enhance=1, transform_kwargs=kw, seed=0)
    (batch,) = list(q)
    assert batch.low_res.shape == (5, 4, 4, 2)
    raw = np.stack([lr[i:i + 4, j:j + 4, k]
                    for i, j, k in smp.last_lr_origins])
    want, _ = DeviceBatchTransform(1, 1, ['u', 'v']).transform(raw, **kw)
    np.testing.assert_array_equal(
        batch.low_res.cpu().numpy().view(np.uint32),
        want.cpu().numpy().view(np.uint32))
    assert (batch.low_res.cpu().numpy()[..., 1] == raw[..., 1]).all()
    assert (batch.low_res.cpu().numpy()[..., 0] != raw[..., 0]).any()


def test_sup3r_gan_dc_trains_from_a_device_batch_handler_dc():
    from sup3r_amd import DeviceBatchHandlerDC, DeviceSamplerDC, Sup3rGanDC
    feats = ['u_10m', 'v_10m', 'topography']

    def smp(shape, seed):
        cube = np.random.default_rng(seed).standard_normal(
            shape + (3,)).astype(np.float32)
        return DeviceSamplerDC(cube, feats, (10, 12, 16), batch_size=4,
                               seed=seed,
                               feature_sets={'lr_only_features': ['topo*']})
    train = [smp((24, 26, 80), 1), smp((20, 30, 70), 2)]
    val = [smp((20, 22, 70), 3)]
    bh = DeviceBatchHandlerDC(train, val, n_space_bins=2, n_time_bins=2,
                              batch_size=4, n_batches=3, s_enhance=2,
                              t_enhance=4, seed=0)
    assert bh.shapes == ((4, 5, 6, 4, 3), (4, 10, 12, 16, 2))
    assert len(bh.val_data) == 4
    Sup3rGanDC.seed(0)
    model = Sup3rGanDC(os.path.join(CFG, 'test_gen_st_2x_4x_2f.json'),
                       os.path.join(CFG, 'test_disc_st_same.json'),
                       learning_rate=1e-4, loss='MeanAbsoluteError')
    model.train(bh, input_resolution={'spatial': '8km', 'temporal': '60min'},
                n_epoch=2, weight_gen_advers=1e-3, checkpoint_int=None)
    assert len(model.history) == 2
    assert not bh.queue_thread.is_alive()
    assert not bh.val_data.queue_thread.is_alive()
    ws, wt = np.asarray(bh.spatial_weights), np.asarray(bh.temporal_weights)
    assert ws.shape == wt.shape == (2,)
    assert np.isfinite(ws).all() and np.isfinite(wt).all()
    # v / v.sum() in float32: each quotient is off by at most half an ulp of a
    # number below 1 (2^-25), their float64 sum by no more than 2 * 2^-25
    for w in (ws, wt):
        assert w.dtype == np.float32
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 2.0 ** -24
    assert not (np.all(ws == 0.5) and np.all(wt == 0.5))
    bh.sample_batch()
    drawn = train[bh.container_index]
    assert drawn.spatial_weights is bh.spatial_weights
    assert drawn.temporal_weights is bh.temporal_weights
