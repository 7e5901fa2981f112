"""GPU tests (``-m gpu``) of ``DualSamplerCC`` on the device: ``s3_nn_fill``,
``s3_cc_night_mask`` and ``s3_cc_window_gather`` through the C-ABI into
sentinel-filled buffers with red zones, ``DeviceDualSamplerCC`` and
``DeviceBatchHandlerCC`` end to end.  Every comparison is bit-exact (``uint32``
views) against the numpy restatement ``tests/cc_ref.py``, which
``test_samplers_cc_cpu.py`` holds against scipy."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import cc_ref  # noqa: E402
from test_samplers_cc_cpu import (CSR, FEATS, WINDOW_CASES,  # noqa: E402
                                  holes_night, night_of, solar_cubes)

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), '..', 'sup3r_amd', 'configs')
EINVAL = -1
PAD = 64                       # sentinel words in front of and behind a buffer
SENTINEL = 0x5A5AC3C3
NANS = np.array([0x7FC00000, 0x7FC00001, 0x7F800001, 0xFFC12345],
                dtype=np.uint32)             # quiet, payload, signalling, negative
# -0.0, +inf, -inf, the smallest denormal, the largest
ODD_VALUES = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x00000001,
                       0x007FFFFF], dtype=np.uint32)


def padded(words, device):
    """int32 device buffer of ``words`` words between two red zones"""
    import torch
    return torch.full((PAD + words + PAD,), SENTINEL, dtype=torch.int32,
                      device=device)


def zones_intact(buf, words):
    host = buf.cpu().numpy().view(np.uint32)
    return bool((host[:PAD] == SENTINEL).all()
                and (host[PAD + words:] == SENTINEL).all())


def payload(buf, words):
    return buf.cpu().numpy().view(np.uint32)[PAD:PAD + words].copy()


def block_bits(shape, holes, channel, seed):
    """``(n, s1, s2, t, C)`` uint32: distinct finite values everywhere, the odd
    values planted among them, NaNs of every kind in the ``holes`` of
    ``channel`` — and NaNs with other payloads sprinkled over the OTHER
    channels, which the fill must not touch"""
    rng = np.random.default_rng(seed)
    bits = rng.standard_normal(shape).astype(np.float32).view(np.uint32).copy()
    flat = bits.reshape(-1)
    spots = rng.choice(flat.size, size=min(len(ODD_VALUES), flat.size),
                       replace=False)
    flat[spots] = ODD_VALUES[:len(spots)]
    for q in range(shape[4]):
        if q != channel:
            other = rng.random(shape[:4]) < 0.3
            bits[..., q][other] = 0x7FC0BEEF + q
    plane = bits[..., channel]
    plane[holes] = NANS[rng.integers(0, len(NANS), size=int(holes.sum()))]
    return bits


def run_fill(bits, channel):
    """``s3_nn_fill`` on a copy of ``bits`` on the device; returns (rc, block
    after the call, count word); asserts that nothing around the block, the
    workspace and the count word was written"""
    import torch
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    dev, L = Device.get(), _lib.lib()
    n, s1, s2, t, c = bits.shape
    keys = n * s1 * s2 * t
    x = padded(bits.size, dev.torch_device)
    x[PAD:PAD + bits.size] = torch.from_numpy(
        bits.reshape(-1).view(np.int32)).to(dev.torch_device)
    work = padded(2 * keys, dev.torch_device)
    count = padded(1, dev.torch_device)
    assert (work.data_ptr() + 4 * PAD) % 8 == 0
    rc = L.s3_nn_fill(dev.ctx, C.c_void_p(x.data_ptr() + 4 * PAD), n, s1, s2,
                      t, c, channel, C.c_void_p(work.data_ptr() + 4 * PAD),
                      C.c_void_p(count.data_ptr() + 4 * PAD))
    dev.sync()
    assert zones_intact(x, bits.size) and zones_intact(work, 2 * keys)
    assert zones_intact(count, 1)
    return rc, payload(x, bits.size).reshape(bits.shape), int(
        payload(count, 1).view(np.int32)[0])


def check_fill(shape, holes, channels=1, channel=0, seed=0):
    bits = block_bits(shape + (channels,), holes, channel, seed)
    want, found = cc_ref.nn_fill(bits.view(np.float32), channel)
    rc, got, count = run_fill(bits, channel)
    assert rc == 0
    np.testing.assert_array_equal(got, want.view(np.uint32))
    assert count == found == int(holes.sum())
    return got


FILL_SHAPES = [(1, 1, 1, 2), (2, 3, 1, 5), (3, 4, 5, 6),
               # one axis of 65 to cross a wave, a long and the longest time
               # axis of the reference's tests
               (65, 1, 1, 2), (1, 65, 1, 2), (1, 1, 65, 2), (1, 2, 2, 72),
               (1, 1, 2, 216)]


@pytest.mark.parametrize('p', [0.2, 0.6, 0.95])
@pytest.mark.parametrize('shape', FILL_SHAPES, ids=str)
def test_fill_uniform_masks(shape, p):
    rng = np.random.default_rng(int(p * 100) + sum(shape))
    holes = rng.random(shape) < p
    if holes.all():
        holes[tuple(rng.integers(0, d) for d in shape)] = False
    check_fill(shape, holes, seed=sum(shape))


@pytest.mark.parametrize('extra', [0.0, 0.05])
def test_fill_night_bands(extra):
    shape = (5, 6, 6, 24)
    holes = holes_night(np.random.default_rng(3), shape, extra)
    got = check_fill(shape, holes, channels=2, channel=1, seed=7)
    assert not np.isnan(got.view(np.float32)[..., 1]).any()


def test_fill_from_a_single_source():
    shape = (3, 4, 5, 6)
    holes = np.ones(shape, dtype=bool)
    holes[2, 1, 3, 4] = False
    got = check_fill(shape, holes, seed=11)
    assert (got == got[2, 1, 3, 4, 0]).all()


def test_fill_without_nan_changes_nothing():
    """-0.0, the infinities and the denormals among the values; count 0"""
    shape = (3, 4, 5, 6)
    bits = block_bits(shape + (1,), np.zeros(shape, dtype=bool), 0, seed=13)
    assert all(v in bits for v in ODD_VALUES)
    rc, got, count = run_fill(bits, 0)
    assert rc == 0 and count == 0
    np.testing.assert_array_equal(got, bits)


def test_fill_all_nan_stays_nan():
    shape = (2, 3, 2, 5)
    bits = block_bits(shape + (2,), np.ones(shape, dtype=bool), 0, seed=17)
    rc, got, count = run_fill(bits, 0)
    assert rc == 0 and count == 2 * 3 * 2 * 5
    np.testing.assert_array_equal(got, bits)


@pytest.mark.parametrize('channels,channel', [(1, 0), (3, 0), (3, 1), (3, 2)])
def test_fill_touches_one_channel(channels, channel):
    shape = (2, 3, 4, 7)
    holes = np.random.default_rng(channel).random(shape) < 0.6
    bits = block_bits(shape + (channels,), holes, channel, seed=19)
    rc, got, _ = run_fill(bits, channel)
    assert rc == 0
    want, _ = cc_ref.nn_fill(bits.view(np.float32), channel)
    np.testing.assert_array_equal(got, want.view(np.uint32))
    others = [q for q in range(channels) if q != channel]
    np.testing.assert_array_equal(got[..., others], bits[..., others])
    if others:
        assert np.isnan(got.view(np.float32)[..., others]).any()
    assert not np.isnan(got.view(np.float32)[..., channel]).any()


def test_fill_refuses_what_is_over_its_limits():
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    dev, L = Device.get(), _lib.lib()
    x = padded(16, dev.torch_device)
    work = padded(32, dev.torch_device)
    count = padded(1, dev.torch_device)
    big = _lib.NN_FILL_MAX_AXIS + 1

    def call(n, s1, s2, t, c=1, channel=0, w=work):
        return L.s3_nn_fill(
            dev.ctx, C.c_void_p(x.data_ptr() + 4 * PAD), n, s1, s2, t, c,
            channel, C.c_void_p(w.data_ptr() + 4 * PAD) if w is not None
            else None, C.c_void_p(count.data_ptr() + 4 * PAD))
    cases = [((big, 1, 1, 2), 'S3_NN_FILL_MAX_AXIS'),
             ((1, big, 1, 2), 'S3_NN_FILL_MAX_AXIS'),
             ((1, 1, big, 2), 'S3_NN_FILL_MAX_AXIS'),
             ((1, 1, 2, big), 'S3_NN_FILL_MAX_AXIS'),
             ((2048, 2048, 512, 1), '2^31'),      # 2^31 elements exactly
             ((2, 2, 2, 0), 'empty block')]
    for dims, text in cases:
        assert call(*dims) == EINVAL, dims
        msg = _lib.last_error(dev.ctx)
        assert msg.startswith('s3_nn_fill') and text in msg, (dims, msg)
    assert call(2, 2, 2, 2, c=2, channel=2) == EINVAL
    assert 'channel' in _lib.last_error(dev.ctx)
    assert call(2, 2, 2, 2, w=None) == EINVAL
    assert _lib.last_error(dev.ctx).startswith('s3_nn_fill')
    dev.sync()
    for buf in (x, work, count):
        assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all()


# --------------------------------------------- night mask and shifted gather
def window_cube(day, n, single=False):
    """(6, 6, 96, 2) cube (hour counter, clearsky ratio) and ``n`` 2 x 2 boxes
    on separate pixels whose 24-hour windows start at different hours; every
    night hour of the windows is NaN in ONE pixel of ONE box (``single``: all
    of them in the same pixel of the last box)"""
    cube = np.random.default_rng(len(list(day))).uniform(
        0.1, 1.0, (6, 6, 96, 2)).astype(np.float32)
    cube[..., 0] += np.arange(96, dtype=np.float32) * 4      # hours tell apart
    origins = [(0, 0, 36), (2, 3, 24), (4, 1, 60)][:n]
    for k in np.flatnonzero(night_of(day)):
        m = n - 1 if single else k % n
        i0, j0, k0 = origins[m]
        a, b = (1, 0) if single else ((k // n) % 2, (k // (2 * n)) % 2)
        cube[i0 + a, j0 + b, k0 + k, 1] = np.nan
    return cube, np.array(origins, dtype=np.int32)


def run_window(cube, origins, box, csr_channel, channels):
    """night mask + window gather through the C-ABI; returns (out, status)"""
    import torch
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    dev, L = Device.get(), _lib.lib()
    cube_d = torch.from_numpy(cube).to(dev.torch_device)
    S1, S2, T, Cc = cube.shape
    s1, s2, t = box
    org = np.ascontiguousarray(origins, dtype=np.int32)
    ch = np.ascontiguousarray(channels, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    words = len(org) * s1 * s2 * t * len(ch)
    out = padded(words, dev.torch_device)
    status = padded(_lib.CC_STATUS_WORDS, dev.torch_device)
    sp = C.c_void_p(status.data_ptr() + 4 * PAD)
    rc = L.s3_cc_night_mask(dev.ctx, C.c_void_p(cube_d.data_ptr()), S1, S2, T,
                            Cc, org.ctypes.data_as(ip), len(org), s1, s2,
                            csr_channel, sp)
    assert rc == 0, _lib.last_error(dev.ctx)
    rc = L.s3_cc_window_gather(
        dev.ctx, C.c_void_p(cube_d.data_ptr()), S1, S2, T, Cc,
        org.ctypes.data_as(ip), len(org), s1, s2, t, ch.ctypes.data_as(ip),
        len(ch), sp, C.c_void_p(out.data_ptr() + 4 * PAD))
    assert rc == 0, _lib.last_error(dev.ctx)
    dev.sync()
    assert zones_intact(out, words) and zones_intact(
        status, _lib.CC_STATUS_WORDS)
    return (payload(out, words).reshape(len(org), s1, s2, t, len(ch)),
            payload(status, _lib.CC_STATUS_WORDS).view(np.int32))


@pytest.mark.parametrize('channels', [[0, 1], [1]], ids=str)
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('day,start,raw', WINDOW_CASES,
                         ids=[str(i) for i in range(len(WINDOW_CASES))])
def test_night_mask_and_window_gather(day, start, raw, n, channels):
    t = 12
    cube, origins = window_cube(day, n)
    got, status = run_window(cube, origins, (2, 2, t), 1, channels)
    night = night_of(day)
    assert cc_ref.window_start(night, t) == (raw, start)
    assert list(status) == [cc_ref.mask_word(night), raw, start, 0]
    want = np.stack([cube[i:i + 2, j:j + 2, k + start:k + start + t]
                     [..., channels] for i, j, k in origins])
    np.testing.assert_array_equal(got, want.view(np.uint32))


def test_one_dark_pixel_in_one_box_darkens_the_hour_for_all():
    t = 12
    day = range(7, 18)
    cube, origins = window_cube(day, 3, single=True)
    got, status = run_window(cube, origins, (2, 2, t), 1, [0, 1])
    assert list(status) == [cc_ref.mask_word(night_of(day)), 6, 6, 0]
    # without that pixel the first two boxes have no night at all
    assert not np.isnan(cube[:4, :, :, 1]).any()
    first_two = cc_ref.night_mask(np.stack(
        [cube[i:i + 2, j:j + 2, k:k + 24, 1] for i, j, k in origins[:2]]))
    assert not first_two.any()
    want = np.stack([cube[i:i + 2, j:j + 2, k + 6:k + 18]
                     for i, j, k in origins])
    np.testing.assert_array_equal(got, want.view(np.uint32))


def test_more_windows_than_one_launch_carries():
    """70 boxes: two launches of the mask kernel and of the gather; the night
    (hours 0-5 and 19-23) is NaN only in a pixel that no box before the 70th
    covers, so the second mask launch has to reach every workgroup of both
    gather launches"""
    from sup3r_amd import _lib
    n, t = _lib.SAMPLE_MAX_ORIGINS + 6, 12
    rng = np.random.default_rng(70)
    cube = rng.uniform(0.1, 1.0, (6, 6, 96, 2)).astype(np.float32)
    origins = np.stack([rng.integers(0, 3, n), rng.integers(0, 5, n),
                        24 * rng.integers(0, 4, n)], axis=1).astype(np.int32)
    origins[-1] = (4, 2, 48)                     # rows 4-5: only this box
    day = range(6, 19)
    for k in np.flatnonzero(night_of(day)):
        cube[5, 3, 48 + k, 1] = np.nan
    got, status = run_window(cube, origins, (2, 2, t), 1, [1, 0])
    raw, start = cc_ref.window_start(night_of(day), t)
    assert (raw, start) == (6, 6)                # 13 hours of daylight: 6 - ceil(-1 / 2)
    assert list(status) == [cc_ref.mask_word(night_of(day)), raw, start, 0]
    want = np.stack([cube[i:i + 2, j:j + 2, k + start:k + start + t]
                     [..., [1, 0]] for i, j, k in origins])
    np.testing.assert_array_equal(got, want.view(np.uint32))


def test_window_entry_points_refuse_bad_arguments():
    import torch
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    dev, L = Device.get(), _lib.lib()
    cube, origins = window_cube(range(7, 18), 1)
    cube_d = torch.from_numpy(cube).to(dev.torch_device)
    ip = C.POINTER(C.c_int32)
    ch = np.array([0, 1], dtype=np.int32)
    out = padded(2 * 2 * 24 * 2, dev.torch_device)
    status = padded(_lib.CC_STATUS_WORDS, dev.torch_device)
    sp = C.c_void_p(status.data_ptr() + 4 * PAD)

    def mask(org, channel=1):
        org = np.array(org, dtype=np.int32)
        return L.s3_cc_night_mask(dev.ctx, C.c_void_p(cube_d.data_ptr()), 6, 6,
                                  96, 2, org.ctypes.data_as(ip), 1, 2, 2,
                                  channel, sp)

    def gather(org, t):
        org = np.array(org, dtype=np.int32)
        return L.s3_cc_window_gather(
            dev.ctx, C.c_void_p(cube_d.data_ptr()), 6, 6, 96, 2,
            org.ctypes.data_as(ip), 1, 2, 2, t, ch.ctypes.data_as(ip), 2, sp,
            C.c_void_p(out.data_ptr() + 4 * PAD))
    # the 24-hour window, not the t hours kept, must fit the cube
    for rc in (mask([[0, 0, 73]]), mask([[5, 0, 0]]), mask([[0, 0, 0]], 2)):
        assert rc == EINVAL
        assert _lib.last_error(dev.ctx).startswith('s3_cc_night_mask')
    for rc in (gather([[0, 0, 73]], 12), gather([[0, 0, 0]], 24),
               gather([[0, 5, 0]], 12)):
        assert rc == EINVAL
        assert _lib.last_error(dev.ctx).startswith('s3_cc_window_gather')
    dev.sync()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all()
    assert (status.cpu().numpy().view(np.uint32) == SENTINEL).all()


# ------------------------------------------------------------- the sampler
def device_sampler(daily, hourly, sample_shape, t_enhance, batch_size,
                   s_enhance=1, seed=5, **kw):
    import warnings
    from sup3r_amd import DeviceDualSamplerCC
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # the slow-batch warning
        return DeviceDualSamplerCC(
            daily, hourly, FEATS, FEATS, sample_shape, batch_size=batch_size,
            s_enhance=s_enhance, t_enhance=t_enhance, seed=seed, **kw)


@pytest.mark.parametrize('s_enhance', [1, 2])
@pytest.mark.parametrize('slow', [False, True], ids=['fast', 'slow'])
@pytest.mark.parametrize('t,t_enhance', [(24, 24), (48, 24), (24, 8), (12, 3)])
def test_sampler_end_to_end(t, t_enhance, slow, s_enhance):
    from sup3r_amd.samplers_cc import coarsen_daily
    days = 6
    daily, hourly = solar_cubes(days=days)       # the night moves with the column
    lt = t // t_enhance
    batch = days // lt + (1 if slow else 0)
    smp = device_sampler(daily, hourly, (4, 6, t), t_enhance, batch,
                         s_enhance=s_enhance)
    assert smp._fast_batch_possible() == (not slow)
    low_res = daily if s_enhance == 1 else coarsen_daily(daily, s_enhance)
    lr_box = (4 // s_enhance, 6 // s_enhance, lt)
    for _ in range(2):
        low, high = next(smp)
        status = smp.cc_status.cpu().numpy()
        low, high = low.cpu().numpy(), high.cpu().numpy()
        lr_org, hr_org = smp.last_lr_origins, smp.last_origins
        np.testing.assert_array_equal(
            hr_org, lr_org * [s_enhance, s_enhance, 24])
        want_low, want_high, info = cc_ref.cc_next(
            low_res, hourly, lr_org, hr_org, lr_box, (4, 6, t), t_enhance,
            [0, 1], [0, 1], 0)
        assert high.shape == (batch, 4, 6, t, 2)
        np.testing.assert_array_equal(high.view(np.uint32),
                                      want_high.view(np.uint32))
        np.testing.assert_array_equal(low.view(np.uint32),
                                      want_low.view(np.uint32))
        assert not np.isnan(high[..., 0]).any() and info['filled'] > 0
        assert status[3] == info['filled']
        if t < 24:
            assert list(status[:3]) == [info['mask'], info['start_raw'],
                                        info['start']]
        else:
            assert list(status[:3]) == [0, 0, 0]
        # the low-res batch is the daily slice of the same days
        for m, (i, j, k) in enumerate(lr_org):
            np.testing.assert_array_equal(
                low[m], low_res[i:i + lr_box[0], j:j + lr_box[1], k:k + lt])


def test_sampler_without_clearsky_output_is_the_raw_gather():
    daily, hourly = solar_cubes(days=6)
    smp = device_sampler(daily, hourly, (4, 6, 12), 3, 1,
                         feature_sets={'lr_only_features': [CSR]})
    low, high = next(smp)
    assert tuple(high.shape) == (1, 4, 6, 96, 1)
    (i, j, k), = smp.last_origins
    np.testing.assert_array_equal(
        high.cpu().numpy()[0].view(np.uint32),
        hourly[i:i + 4, j:j + 6, k:k + 96][..., [1]].view(np.uint32))
    assert (smp.cc_status.cpu().numpy() == 0).all()


# ------------------------------------------------------- the batch handler
def test_batch_handler_cc_and_solar_cc():
    import torch
    from sup3r_amd import (BatchHandlerCC, DeviceBatchHandlerCC,
                           DeviceDualBatchQueue, SolarCC)
    assert BatchHandlerCC is DeviceBatchHandlerCC
    s, te, B = 2, 4, 2
    daily, hourly = solar_cubes(days=12, S=16)
    train = device_sampler(daily, hourly, (8, 8, 24), te, B, s_enhance=s, seed=1)
    val = device_sampler(daily, hourly, (8, 8, 24), te, B, s_enhance=s, seed=2)
    with pytest.raises(AssertionError, match='t_enhance'):
        DeviceBatchHandlerCC([train], [val], batch_size=B, n_batches=2,
                             s_enhance=s, t_enhance=24)
    with pytest.raises(AssertionError, match='s_enhance'):
        DeviceBatchHandlerCC([train], [val], batch_size=B, n_batches=2,
                             s_enhance=1, t_enhance=te)
    bh = DeviceBatchHandlerCC([train], [val], batch_size=B, n_batches=2,
                              s_enhance=s, t_enhance=te, seed=0)
    assert bh.device_resident and isinstance(bh.val_data, DeviceDualBatchQueue)
    assert bh.BATCH_MEMBERS == ('low_res', 'high_res')
    assert bh.queue_shape == [(B, 4, 4, 6, 2), (B, 8, 8, 24, 2)]
    assert bh.shapes == ((B, 4, 4, 6, 2), (B, 8, 8, 24, 2))
    batches, vals = list(bh), list(bh.val_data)
    assert len(batches) == 2 and len(vals) == 2
    assert not bh.queue_thread.is_alive()
    for b in batches + vals:
        assert isinstance(b.high_res, torch.Tensor) and b.high_res.is_cuda
        assert tuple(b.low_res.shape) == (B, 4, 4, 6, 2)
        assert tuple(b.high_res.shape) == (B, 8, 8, 24, 2)
        assert not torch.isnan(b.high_res).any()
    # the smallest spec of tests/test_solar_cc.py: 2 x in space, 4 x in time
    SolarCC.seed(0)
    model = SolarCC(os.path.join(CFG, 'test_gen_st_2x_4x_2f.json'),
                    os.path.join(CFG, 'test_disc_st_same.json'),
                    learning_rate=1e-4, loss='MeanAbsoluteError')
    low = batches[0].low_res.cpu().numpy()
    true = batches[0].high_res.cpu().numpy()
    model.init_weights(low.shape, true.shape)
    gen = model.generate(low, norm_in=False, un_norm_out=False)
    assert gen.shape == true.shape
    loss, details = model.calc_loss(true, gen, weight_gen_advers=0.0)
    assert np.isfinite(float(loss))
    for k, v in details.items():
        assert np.isfinite(float(v)), (k, v)
