"""GPU tests (``-m gpu``) of the statistics stage: ``s3_channel_moments``
against float64 numpy (one float32 ulp on mean and std, exact counts, two runs
bit-equal), ``s3_normalize_channels`` against numpy's float32 arithmetic bit
for bit, and ``from_containers`` end to end for five handlers.

Why one ulp: the device accumulates shifted sums in float64, whose error is
many orders below a float32 ulp; so is numpy's float64 pairwise error.  Both
values are rounded to float32 once: only a value within ~1e-9 ulp of a
rounding boundary can come out one ulp apart.

The slab sizes below are those of a 256-CU device: the moments walk takes
1024 workgroups (4 per CU), the normalisation 2048 (8 per CU), of 256 lanes
with 4 floats each per slab."""
import ctypes as C
import itertools
import warnings

import numpy as np
import pytest

from tests import stats_ref as R

pytestmark = pytest.mark.gpu

EINVAL = -1
PAD = 64
SENTINEL = 0x5A5AC3C3
CHANNELS = [1, 3, 4, 5, 16, 17, 64]           # 64 = S3_STATS_MAX_CHANNELS
POSITIONS = [1, 63, 64, 65, 4097]
MOMENTS_SLAB = 1024 * 256 * 4                 # floats
NORMALIZE_SLAB = 2048 * 256 * 4


def device():
    from sup3r_amd.engine import Device
    return Device.get()


def upload(x, offset=0):
    """``x`` as a device tensor ``offset`` floats past a 16-byte line, with
    sentinel floats around it; returns (view, whole buffer)"""
    import torch
    flat = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    buf = torch.full((PAD + offset + flat.size + PAD,), SENTINEL,
                     dtype=torch.int32, device='cuda').view(torch.float32)
    view = buf[PAD + offset:PAD + offset + flat.size]
    view.copy_(torch.from_numpy(flat))
    return view.view(*x.shape), buf


def raw_moments(x_d, n_pos, c):
    import torch
    from sup3r_amd import _lib
    dev = device()
    out = torch.full((max(c, 1), 3), -7.0, dtype=torch.float64, device='cuda')
    rc = _lib.lib().s3_channel_moments(
        dev.ctx, C.c_void_p(x_d.data_ptr()), n_pos, c,
        C.c_void_p(out.data_ptr()))
    dev.sync()
    return rc, out.cpu().numpy()


def check_moments(x, offset=0, x_d=None):
    """counts exact, mean and std within one float32 ulp of float64 numpy,
    a second run bit-equal, the cube untouched"""
    n_pos, c = x.shape
    if x_d is None:
        x_d, buf = upload(x, offset)
    rc, got = raw_moments(x_d, n_pos, c)
    assert rc == 0
    rc, again = raw_moments(x_d, n_pos, c)
    assert rc == 0
    np.testing.assert_array_equal(got.view(np.uint64), again.view(np.uint64))
    count, mean, std = R.nan_moments(x)
    np.testing.assert_array_equal(got[:, 0], count)
    with np.errstate(all='ignore'):
        got_std = np.sqrt(got[:, 2] / got[:, 0])
    for q in range(c):
        if count[q] == 0:
            assert got[q, 1] == 0 and got[q, 2] == 0
            continue
        d_mean = R.ulp_distance(got[q, 1], mean[q])
        d_std = R.ulp_distance(got_std[q], std[q])
        print(f'C={c} n_pos={n_pos} channel {q}: mean {got[q, 1]!r} vs '
              f'{mean[q]!r} ({d_mean} ulp), std {got_std[q]!r} vs {std[q]!r} '
              f'({d_std} ulp)')
        assert d_mean <= 1 and d_std <= 1, (q, got[q], mean[q], std[q])
    return got


def data(n_pos, c, seed):
    """every channel with a location and a scale of its own"""
    rng = np.random.default_rng(seed)
    loc = rng.uniform(-300, 300, c)
    scale = rng.uniform(0.5, 20, c)
    return (rng.standard_normal((n_pos, c)) * scale + loc).astype(np.float32)


# ------------------------------------------------------------------- moments
@pytest.mark.parametrize('c', CHANNELS)
def test_moments_every_channel_count_and_length(c):
    for n_pos in POSITIONS:
        for offset in ((0, 1, 3) if n_pos in (1, 65) else (0,)):
            x = data(n_pos, c, seed=c * 10007 + n_pos)
            x_d, buf = upload(x, offset)
            check_moments(x, x_d=x_d)
            whole = buf.cpu().numpy()
            np.testing.assert_array_equal(
                whole[PAD + offset:PAD + offset + x.size], x.reshape(-1))


def test_moments_above_the_maximum_is_einval():
    from sup3r_amd import _lib
    c = _lib.STATS_MAX_CHANNELS + 1
    x_d, _ = upload(data(8, c, 0))
    rc, out = raw_moments(x_d, 8, c)
    assert rc == EINVAL and (out == -7.0).all()
    assert _lib.last_error(device().ctx).startswith('s3_channel_moments')
    rc, out = raw_moments(x_d, 0, 4)
    assert rc == EINVAL and (out == -7.0).all()


NAN_PATTERNS = ['none', 'first_last', 'channel', 'waves', 'alternate']


def plant_nans(x, pattern):
    flat = x.reshape(-1)
    if pattern == 'first_last':
        flat[0] = flat[-1] = np.nan
    elif pattern == 'channel':
        x[:, x.shape[1] // 2] = np.nan
    elif pattern == 'waves':              # a wave loads 256 consecutive floats
        flat[300:300 + 3 * 256 + 17] = np.nan
    elif pattern == 'alternate':
        flat[::2] = np.nan
    return x


@pytest.mark.parametrize('pattern', NAN_PATTERNS)
@pytest.mark.parametrize('n_pos,c', [(4097, 5), (65, 16), (4097, 1)])
def test_moments_nan_patterns(n_pos, c, pattern):
    x = plant_nans(data(n_pos, c, seed=n_pos + c), pattern)
    got = check_moments(x)
    if pattern == 'channel':
        assert got[c // 2, 0] == 0
    if pattern == 'alternate' and c == 16:      # even channels hold nothing
        assert (got[::2, 0] == 0).all() and (got[1::2, 0] == n_pos).all()


@pytest.mark.parametrize('c,offset', [(3, 0), (5, 1), (17, 2), (64, 0)])
def test_moments_more_than_one_slab_per_workgroup(c, offset):
    """2.3 slabs: the grid is cut to a multiple of the odd part of C, every
    lane walks two or three float4 of fixed channels, the end is ragged"""
    n_pos = (2 * MOMENTS_SLAB + 300001) // c + 1
    x = data(n_pos, c, seed=c)
    rng = np.random.default_rng(c + 1)
    x.reshape(-1)[rng.integers(0, x.size, x.size // 20)] = np.nan
    check_moments(x, offset)


def test_moments_infinities_propagate_as_in_numpy():
    x = data(4097, 4, seed=3)
    x[100, 1] = np.inf
    x[7, 2], x[4000, 2] = np.inf, -np.inf
    x[0, 3] = -np.inf                      # the first value a lane meets
    x_d, _ = upload(x)
    rc, got = raw_moments(x_d, *x.shape)
    assert rc == 0
    _, mean, std = R.nan_moments(x)
    assert list(got[:, 0]) == [4097] * 4
    assert got[1, 1] == np.inf == mean[1] and np.isnan(got[1, 2])
    assert np.isnan(got[2, 1]) and np.isnan(mean[2]) and np.isnan(got[2, 2])
    assert got[3, 1] == -np.inf == mean[3] and np.isnan(got[3, 2])
    assert np.isnan(std[1:]).all()
    assert R.ulp_distance(got[0, 1], mean[0]) <= 1          # and the finite one
    assert R.ulp_distance(np.sqrt(got[0, 2] / 4097), std[0]) <= 1


def test_moments_offset_case():
    """values far from 0 with a small spread: what sum(x^2) cannot do
    (tests/test_stats_cpu.py shows that it misses the bound on these data)"""
    rng = np.random.default_rng(11)
    n = 65 * 4097
    x = np.stack([1e5 + 0.1 * rng.standard_normal(n),
                  -3e4 + 1e-2 * rng.standard_normal(n)],
                 axis=1).astype(np.float32)
    check_moments(x)


def test_moments_past_two_to_the_31_elements():
    """a cube of just over 2^31 floats, filled on the device with a constant
    per channel, three values planted in the last positions: the expectation
    is analytic.  32-bit offsets would miss the planted values."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip('less than 16 GiB of device memory free')
    c = 6
    n_pos = 2 ** 31 // c + 1000
    assert n_pos * c > 2 ** 31
    const = np.array([1.5, -2.0, 300.25, 0.0, 1e5, -7.75], dtype=np.float32)
    delta = np.array([2.0 ** 20, 3.0, -2.0 ** 12, 1.0, 64.0, 2.0 ** 16],
                     dtype=np.float32)
    x = torch.empty((n_pos, c), dtype=torch.float32, device='cuda')
    x[:] = torch.from_numpy(const).to('cuda')
    planted = np.stack([const + delta, const - 2 * delta, const + 4 * delta])
    x[-3:] = torch.from_numpy(planted).to('cuda')
    rc, got = raw_moments(x, n_pos, c)
    del x
    assert rc == 0
    d = planted.astype(np.float64) - const.astype(np.float64)    # exact
    mean = const + d.sum(axis=0) / n_pos
    m2 = (d * d).sum(axis=0) - d.sum(axis=0) ** 2 / n_pos
    std = np.sqrt(m2 / n_pos)
    assert (got[:, 0] == n_pos).all()
    for q in range(c):
        assert R.ulp_distance(got[q, 1], mean[q]) <= 1, (q, got[q], mean[q])
        assert R.ulp_distance(np.sqrt(got[q, 2] / n_pos), std[q]) <= 1, \
            (q, got[q], std[q])
    assert np.float32(got[0, 1]) != const[0]     # the planted values counted


# ----------------------------------------------------------------- normalise
def raw_normalize(x_d, n_pos, c, m, s, flags):
    from sup3r_amd import _lib
    dev = device()
    m = np.ascontiguousarray(m, dtype=np.float32)
    s = np.ascontiguousarray(s, dtype=np.float32)
    f = np.ascontiguousarray(flags, dtype=np.uint8)
    pf = C.POINTER(C.c_float)
    rc = _lib.lib().s3_normalize_channels(
        dev.ctx, C.c_void_p(x_d.data_ptr()), n_pos, c, m.ctypes.data_as(pf),
        s.ctypes.data_as(pf), f.ctypes.data_as(C.POINTER(C.c_ubyte)))
    dev.sync()
    return rc


def norm_case(n_pos, c, seed):
    """data, means, stds with |x - m| / s far inside the normal range (an
    exact 0 apart); NaNs of two kinds and an infinity planted; unflagged
    channels carry raw bit patterns"""
    rng = np.random.default_rng(seed)
    x = data(n_pos, c, seed)
    m = (x.mean(axis=0) + rng.uniform(-1, 1, c)).astype(np.float32)
    s = rng.uniform(0.3, 30, c).astype(np.float32)
    flat = x.view(np.uint32).reshape(-1)
    where = rng.integers(0, x.size, 1 + x.size // 50)
    flat[where] = rng.choice(np.array([0x7FC00001, 0xFFC12345, 0x7F800000],
                                      dtype=np.uint32), len(where))
    flat[0], flat[-1] = 0x7FC00000, 0xFFC00000
    return x, m, s


def check_normalize(x, m, s, flags, offset=0):
    n_pos, c = x.shape
    x_d, buf = upload(x, offset)
    assert raw_normalize(x_d, n_pos, c, m, s, flags) == 0
    whole = buf.cpu().numpy().view(np.uint32)
    got = whole[PAD + offset:PAD + offset + x.size].reshape(x.shape)
    want = R.normalize(x, m, s, flags)
    np.testing.assert_array_equal(np.isnan(got.view(np.float32)), np.isnan(x))
    for q in range(c):
        if flags[q]:
            a, b = got[:, q].view(np.float32), want[:, q]
            ok = ~np.isnan(b)
            np.testing.assert_array_equal(a[ok].view(np.uint32),
                                          b[ok].view(np.uint32))
        else:                            # every bit, NaN payloads included
            np.testing.assert_array_equal(got[:, q],
                                          x[:, q].view(np.uint32))
    assert (whole[:PAD + offset] == SENTINEL).all()
    assert (whole[PAD + offset + x.size:] == SENTINEL).all()


@pytest.mark.parametrize('c', CHANNELS)
def test_normalize_is_numpy_float32_bit_for_bit(c):
    for n_pos in POSITIONS:
        x, m, s = norm_case(n_pos, c, seed=c * 31 + n_pos)
        every_other = [(q + n_pos) % 2 for q in range(c)]
        for offset in ((0, 1, 3) if n_pos in (1, 65) else (0,)):
            check_normalize(x, m, s, [1] * c, offset)
            check_normalize(x, m, s, every_other, offset)


@pytest.mark.parametrize('c,offset', [(5, 1), (17, 0), (64, 3)])
def test_normalize_more_than_one_slab_per_workgroup(c, offset):
    n_pos = (2 * NORMALIZE_SLAB + 300001) // c + 1
    x, m, s = norm_case(n_pos, c, seed=c)
    check_normalize(x, m, s, [q % 3 != 1 for q in range(c)], offset)


def test_normalize_refuses_bad_arguments_and_skips_no_flags():
    from sup3r_amd import _lib
    x, m, s = norm_case(65, 3, 0)
    x_d, buf = upload(x)
    big = _lib.STATS_MAX_CHANNELS + 1
    assert raw_normalize(x_d, 1, big, [0] * big, [1] * big, [1] * big) \
        == EINVAL
    assert _lib.last_error(device().ctx).startswith('s3_normalize_channels')
    assert raw_normalize(x_d, 65, 3, m, s, [0, 0, 0]) == 0
    whole = buf.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(whole[PAD:PAD + x.size],
                                  x.view(np.uint32).reshape(-1))


# ---------------------------------------------------------------- end to end
def near(v):
    """the float32 values within one ulp of the float64 ``v``"""
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v,
            np.nextafter(v, np.float32(np.inf))]


def check_stats(handler, per_feature):
    """``per_feature``: ``{name: [cube channel per training container]}``.
    The handler's mean / std must be the reference's combination of
    per-container statistics that lie within one ulp of float64 numpy's."""
    sizes = [s.size for s in handler.containers]
    w = R.container_weights(sizes)
    assert list(handler.means) == list(per_feature) == list(handler.stds)
    for f, columns in per_feature.items():
        per = [R.nan_moments(col.reshape(-1, 1)) for col in columns]
        means = {R.combine_means(pick, w) for pick in
                 itertools.product(*[near(p[1][0]) for p in per])}
        stds = {R.combine_stds(pick, w) for pick in
                itertools.product(*[near(p[2][0]) for p in per])}
        print(f'{f}: mean {handler.means[f]!r} of {sorted(means)}, '
              f'std {handler.stds[f]!r} of {sorted(stds)}')
        assert type(handler.means[f]) is np.float32
        assert handler.means[f] in means and handler.stds[f] in stds


def np_gather(cube, origins, box, channels):
    s1, s2, t = box
    return np.stack([cube[i:i + s1, j:j + s2, k:k + t][..., channels]
                     for i, j, k in origins])


def check_batch(sampler, raw_cube, features, handler):
    """the next batch of ``sampler`` is the gather of the numpy-normalised
    cube, bit for bit"""
    m = [handler.means[f] for f in features]
    s = [handler.stds[f] for f in features]
    want_cube = R.normalize(raw_cube, m, s)
    batch = next(sampler).cpu().numpy()
    want = np_gather(want_cube, sampler.last_origins, sampler.sample_shape,
                     list(range(len(features))))
    np.testing.assert_array_equal(batch.view(np.uint32), want.view(np.uint32))


FEATS = ['u_100m', 'v_100m', 'pressure']


def plain_cubes():
    rng = np.random.default_rng(5)
    a = (rng.standard_normal((9, 8, 30, 3)) * [3, 2, 400]
         + [1, -2, 9.5e4]).astype(np.float32)
    b = (rng.standard_normal((7, 7, 22, 3)) * [4, 1, 300]
         + [0, 3, 9.9e4]).astype(np.float32)
    v = (rng.standard_normal((6, 6, 20, 3)) * [3, 2, 400]
         + [1, -2, 9.7e4]).astype(np.float32)
    a[2, 3, 4:9, 1] = np.nan
    return a, b, v


def test_from_containers_plain_handler():
    from sup3r_amd import DeviceBatchHandler
    a, b, v = plain_cubes()
    bh = DeviceBatchHandler.from_containers(
        [{'data': a, 'features': FEATS}, {'data': b, 'features': FEATS}],
        [{'data': v, 'features': FEATS}], sample_shape=(4, 4, 6),
        batch_size=3, n_batches=2, s_enhance=2, t_enhance=2, seed=3)
    check_stats(bh, {f: [a[..., q], b[..., q]] for q, f in enumerate(FEATS)})
    check_batch(bh.containers[0], a, FEATS, bh)
    check_batch(bh.containers[1], b, FEATS, bh)
    check_batch(bh.val_data.containers[0], v, FEATS, bh)
    batch = next(iter(bh))
    assert tuple(batch.low_res.shape) == (3, 2, 2, 3, 3)
    assert tuple(batch.high_res.shape) == (3, 4, 4, 6, 3)
    bh.stop()


def test_from_containers_normalizes_a_device_tensor_in_the_callers_memory():
    import torch
    from sup3r_amd import DeviceBatchHandler
    a, _, _ = plain_cubes()
    a_d = torch.from_numpy(a).to('cuda')
    bh = DeviceBatchHandler.from_containers(
        [{'data': a_d, 'features': FEATS}], sample_shape=(4, 4, 6),
        batch_size=3, n_batches=2)
    want = R.normalize(a, [bh.means[f] for f in FEATS],
                       [bh.stds[f] for f in FEATS])
    assert bh.containers[0].data.data_ptr() == a_d.data_ptr()
    np.testing.assert_array_equal(a_d.cpu().numpy().view(np.uint32),
                                  want.view(np.uint32))


def test_from_containers_data_centric_handler():
    from sup3r_amd import DeviceBatchHandlerDC
    a, b, v = plain_cubes()
    bh = DeviceBatchHandlerDC.from_containers(
        [{'data': a, 'features': FEATS}], [{'data': v, 'features': FEATS}],
        sample_shape=(4, 4, 6), batch_size=2, n_batches=2, n_space_bins=2,
        n_time_bins=3, seed=1)
    assert type(bh.containers[0]).__name__ == 'DeviceSamplerDC'
    assert bh.val_data.n_batches == 6
    check_stats(bh, {f: [a[..., q]] for q, f in enumerate(FEATS)})
    check_batch(bh.containers[0], a, FEATS, bh)
    check_batch(bh.val_data.containers[0], v, FEATS, bh)


def test_from_containers_moment_handler():
    from sup3r_amd import DeviceBatchHandlerMom1SF
    a, b, v = plain_cubes()
    bh = DeviceBatchHandlerMom1SF.from_containers(
        [{'data': a, 'features': FEATS}, {'data': b, 'features': FEATS}],
        sample_shape=(4, 4, 6), batch_size=2, n_batches=2, s_enhance=2,
        t_enhance=2, time_enhance_mode='constant', s_padding=1, seed=2)
    assert bh.s_padding == 1 and bh.val_data == []
    check_stats(bh, {f: [a[..., q], b[..., q]] for q, f in enumerate(FEATS)})
    check_batch(bh.containers[1], b, FEATS, bh)
    batch = next(iter(bh))
    assert tuple(batch.output.shape) == (2, 4, 4, 6, 3)
    bh.stop()


def test_from_containers_dual_handler_with_obs():
    from sup3r_amd import DeviceDualBatchHandler
    rng = np.random.default_rng(8)
    lr = (rng.standard_normal((5, 5, 12, 2)) * [3, 9] + [1, 280]).astype(
        np.float32)
    hr = (rng.standard_normal((10, 10, 24, 2)) * [5, 200] + [2, 900]).astype(
        np.float32)
    obs = hr.copy()
    obs[rng.random(obs.shape) < 0.6] = np.nan
    lr_f, hr_f = ['u', 'temperature'], ['u', 'topography']
    bh = DeviceDualBatchHandler.from_containers(
        [{'low_res': lr, 'high_res': hr, 'lr_features': lr_f,
          'hr_features': hr_f, 'obs': obs}],
        sample_shape=(4, 4, 4), batch_size=2, n_batches=2, s_enhance=2,
        t_enhance=2, seed=6,
        feature_sets={'hr_exo_features': ['topography'],
                      'lr_only_features': ['temperature']})
    # u from high_res although low_res carries it too; obs is never asked
    check_stats(bh, {'u': [hr[..., 0]], 'temperature': [lr[..., 1]],
                     'topography': [hr[..., 1]]})
    smp = bh.containers[0]
    m, s = bh.means, bh.stds
    want_lr = R.normalize(lr, [m[f] for f in lr_f], [s[f] for f in lr_f])
    want_hr = R.normalize(hr, [m[f] for f in hr_f], [s[f] for f in hr_f])
    want_obs = R.normalize(obs, [m[f] for f in hr_f], [s[f] for f in hr_f])
    low, high, ob = (x.cpu().numpy() for x in next(smp))
    np.testing.assert_array_equal(
        low.view(np.uint32),
        np_gather(want_lr, smp.last_lr_origins, (2, 2, 2),
                  [0, 1]).view(np.uint32))
    np.testing.assert_array_equal(
        high.view(np.uint32),
        np_gather(want_hr, smp.last_origins, (4, 4, 4),
                  [0, 1]).view(np.uint32))
    want_ob = np_gather(want_obs, smp.last_origins, (4, 4, 4), [0])
    np.testing.assert_array_equal(np.isnan(ob), np.isnan(want_ob))
    ok = ~np.isnan(want_ob)
    np.testing.assert_array_equal(ob[ok].view(np.uint32),
                                  want_ob[ok].view(np.uint32))
    assert ok.any() and not ok.all()
    batch = next(iter(bh))
    assert batch.dset_names == ['low_res', 'high_res', 'obs']


def test_from_containers_cc_handler_with_nan_nights():
    from sup3r_amd import DeviceBatchHandlerCC
    days, S = 6, 8
    rng = np.random.default_rng(0)
    hourly = rng.uniform(0.1, 1.0, (S, S, 24 * days, 2)).astype(np.float32)
    hourly[..., 1] = hourly[..., 1] * 30 + 270
    hour = np.arange(24 * days) % 24
    for j in range(S):
        dark = (hour < 6 + j % 5) | (hour >= 17 + j % 5)
        hourly[:, j, dark, 0] = np.nan
    daily = np.nanmean(hourly.reshape(S, S, days, 24, 2), axis=3).astype(
        np.float32)
    feats = ['clearsky_ratio', 'temperature']
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # the slow-batch warning
        bh = DeviceBatchHandlerCC.from_containers(
            [{'daily': daily, 'hourly': hourly, 'lr_features': feats,
              'hr_features': feats}],
            sample_shape=(4, 6, 24), batch_size=2, n_batches=2, s_enhance=1,
            t_enhance=24, seed=5)
    # both features are high_res features: the hourly cube, nights skipped
    check_stats(bh, {f: [hourly[..., q]] for q, f in enumerate(feats)})
    smp = bh.containers[0]
    m = [bh.means[f] for f in feats]
    s = [bh.stds[f] for f in feats]
    want_daily, want_hourly = R.normalize(daily, m, s), \
        R.normalize(hourly, m, s)
    low, high = (x.cpu().numpy() for x in next(smp))
    np.testing.assert_array_equal(
        low.view(np.uint32),
        np_gather(want_daily, smp.last_lr_origins, (4, 6, 1),
                  [0, 1]).view(np.uint32))
    want_high = np_gather(want_hourly, smp.last_origins, (4, 6, 24), [0, 1])
    day = ~np.isnan(want_high)                  # the nights are filled
    assert day[..., 1].all() and not day[..., 0].all()
    np.testing.assert_array_equal(high[day].view(np.uint32),
                                  want_high[day].view(np.uint32))
    assert not np.isnan(high).any()
