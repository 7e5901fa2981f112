"""GPU tests (``-m gpu``) of csrc/kernels_data_handler.hip and of the handlers of
sup3r_amd/data_handlers.py on ``DeviceBackend``, against
tests/data_handler_ref.py.

Tolerances.  Gathers, maxima, minima, the scaling and the ratios are compared
bit for bit.  Means and sums are compared with the float64 reference over the
same window within ``ulp32(ref) + 2^-45 sum|x|``: the device and numpy both add
in float64, each erring by at most ``w 2^-53 sum|x|`` (``w <= 256``), and the
one float32 rounding behind either can fall on different sides of a rounding
boundary.  RATIO is numpy's float32 quotient of the device's own two totals.
"""
import warnings

import numpy as np
import pandas as pd
import pytest

from tests import data_handler_ref as R

pytestmark = pytest.mark.gpu


def backend():
    from sup3r_amd.derive import DeviceBackend
    return DeviceBackend()


def bits(rng, shape):
    """float32 of random bit patterns: NaN payloads, infinities, denormals,
    and some -0.0"""
    x = rng.integers(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64).astype(
        np.int32)
    x.reshape(-1)[::11] = np.int32(-2 ** 31)              # -0.0
    return x.view(np.float32)


def up(x, offset=0):
    """``x`` on the device, ``offset`` floats past a 16-byte line"""
    import torch
    x = np.ascontiguousarray(x, dtype=np.float32)
    buf = torch.empty(x.size + 8, dtype=torch.float32, device='cuda')
    view = buf[offset:offset + x.size].view(*x.shape)
    view.copy_(torch.from_numpy(x))
    return view


def down(t):
    return t.detach().cpu().numpy()


def same_bits(got, want, what='', payload=False):
    """bit for bit; NaN matches NaN of any sign and payload unless ``payload``
    (0 / 0 is -NaN on the host)"""
    got = np.ascontiguousarray(down(got) if hasattr(got, 'cpu') else got)
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(np.int32), want.view(np.int32)
    if not payload:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        g, w = g[~nan], w[~nan]
    assert np.array_equal(g, w), what


# ------------------------------------------------------------ raster gather
@pytest.mark.parametrize('rows, cols, t0, step, n_k', [
    (slice(2, 3), slice(4, 5), 6, 1, 1),
    (slice(1, 4), slice(2, 7), 3, 1, 7),
    (slice(0, 6), slice(0, 9), 0, 1, 40),                # whole rows
    (slice(3, 6), slice(5, 9), 5, 2, 17),                # t0 > 0, step 2
    (slice(0, 5), slice(1, 8), 1, 3, 13),
])
def test_gridded_windows_are_bit_equal(rows, cols, t0, step, n_k):
    rng = np.random.default_rng(n_k)
    be = backend()
    planes = [bits(rng, (6, 9, 40)), bits(rng, (6, 9, 40)),
              bits(rng, (6, 9, 40, 5)), bits(rng, (6, 9))]
    got = be.raster_gather([up(p) for p in planes], rows=rows, cols=cols,
                           t0=t0, step=step, n_k=n_k)
    steps = slice(t0, t0 + (n_k - 1) * step + 1, step)
    for g, p in zip(got, planes):
        want = p[rows, cols] if p.ndim == 2 else p[rows, cols, steps]
        same_bits(g, want, f'{p.shape} {rows} {cols} {steps}', payload=True)


@pytest.mark.parametrize('shape', [(7, 9), (8, 8), (5, 13), (13, 10)])
@pytest.mark.parametrize('n_k', [63, 64, 65, 130])
def test_flat_tiles_are_bit_equal(shape, n_k):
    rng = np.random.default_rng(n_k + shape[0])
    be = backend()
    n_sites, t0, step = 301, 3, 2
    t_src = t0 + (n_k - 1) * step + 1 + 2
    src = bits(rng, (t_src, n_sites))
    flat1d = bits(rng, (n_sites,))
    site = rng.integers(0, n_sites, size=shape)          # unordered, repeats
    site[0, :3] = site[0, 0]
    a, b = be.raster_gather([up(src), up(flat1d)], t0=t0, step=step, n_k=n_k,
                            site=site)
    same_bits(a, R.rasterize_flat(src, site, slice(t0, t0 + n_k * step, step)),
              payload=True)
    same_bits(b, flat1d[site], payload=True)
    # neighbouring sites, every step
    site = (np.arange(shape[0] * shape[1]) + 17).reshape(shape)
    a, = be.raster_gather([up(src)], t0=0, step=1, n_k=t_src, site=site)
    same_bits(a, R.rasterize_flat(src, site, slice(None)), payload=True)


def test_gather_refuses_what_leaves_the_source():
    be = backend()
    src = up(np.zeros((4, 5, 6), np.float32))
    with pytest.raises(ValueError, match='time steps leave the source'):
        be.raster_gather([src], rows=slice(0, 4), cols=slice(0, 5), t0=2,
                         step=1, n_k=5)
    flat = up(np.zeros((6, 20), np.float32))
    with pytest.raises(IndexError):
        be.raster_gather([flat], t0=0, step=1, n_k=6,
                         site=np.array([[0, 20]]))
    with pytest.raises(ValueError, match='time steps leave the source'):
        be.raster_gather([flat], t0=0, step=2, n_k=4, site=np.array([[0, 1]]))


def test_flat_source_past_2_to_31_elements():
    """offsets are 64-bit: the rows read lie behind element 2^31 of an
    uninitialised source; only they are written"""
    import torch
    be = backend()
    n_sites, t_src = 2 ** 20 + 3, 2300
    assert (t_src - 140) * n_sites > 2 ** 31
    src = torch.empty((t_src, n_sites), dtype=torch.float32, device='cuda')
    rng = np.random.default_rng(5)
    cols = np.sort(rng.choice(n_sites, size=100, replace=False))
    cols[-1] = n_sites - 1
    rows = 131
    planted = bits(rng, (rows, len(cols)))
    src[t_src - rows:, torch.from_numpy(cols).cuda()] = torch.from_numpy(
        planted).cuda()
    pick = rng.integers(0, len(cols), size=(13, 10))
    pick[-1, -1] = len(cols) - 1
    got, = be.raster_gather([src], t0=t_src - rows, step=2, n_k=66,
                            site=cols[pick])
    same_bits(got, np.moveaxis(planted[::2][:, pick], 0, -1), payload=True)
    del src
    torch.cuda.empty_cache()


# ------------------------------------------------------------- daily reduce
DAILY_SHAPES = [(1, 2, 24), (15, 3, 24), (195, 2, 24), (7, 367, 24),
                (4, 2, 18), (5, 3, 8), (3, 4, 48), (2, 5, 1)]


def planted(rng, n_pix, days, w, scale=100.0):
    """mixed-sign windows with a NaN at the first and at the last hour, an
    all-NaN window, +inf, -inf and both"""
    x = (rng.standard_normal((n_pix * days, w)) * scale).astype(np.float32)
    n = len(x)
    x[0, 0] = np.nan
    x[1 % n, -1] = np.nan
    if n >= 3:
        x[2] = np.nan
    if n >= 4:
        x[3, w // 2] = np.inf
    if n >= 5:
        x[4, 0] = -np.inf
    if n >= 6 and w >= 2:
        x[5, 0], x[5, -1] = np.inf, -np.inf
    if n >= 8:
        x[7, :] = np.nan
        x[7, w // 2] = np.float32(-3.25)                 # one value among NaN
    return x.reshape(n_pix, 1, days * w)


def check_outputs(sources, w, outputs, got):
    got = [down(g) for g in got]
    for (i, j, op), g in zip(outputs, got):
        assert g.shape == (*sources[i].shape[:2], sources[i].shape[2] // w)
        if op == 'ratio':
            tot = {k: got[outputs.index((k, None, 'sum'))] for k in (i, j)}
            with np.errstate(all='ignore'):
                same_bits(g, tot[i] / tot[j], 'ratio')
            continue
        ref, sum_abs = R.reduce64(sources[i], w, op)
        if op in ('max', 'min'):
            same_bits(g, ref.astype(np.float32), op)
        else:
            R.assert_close_sum(g, ref, sum_abs, f'{op} w={w}')
    return got


@pytest.mark.parametrize('offset', [0, 1, 3])
@pytest.mark.parametrize('n_pix, days, w', DAILY_SHAPES)
def test_daily_reduce(n_pix, days, w, offset):
    rng = np.random.default_rng(n_pix * 1000 + days + w)
    be = backend()
    a = planted(rng, n_pix, days, w)
    b = planted(rng, n_pix, days, w, scale=3.0)
    a_d, b_d = up(a, offset), up(b, (offset + 2) % 4)
    one = [(0, None, 'mean')]
    check_outputs([a], w, one, be.daily_reduce([a_d], w, one))
    eight = [(0, None, op) for op in ('mean', 'max', 'min', 'sum')] * 2
    got = check_outputs([a], w, eight, be.daily_reduce([a_d], w, eight))
    for first, second in zip(got[:4], got[4:]):
        same_bits(first, second)
    two = [(0, None, 'sum'), (1, None, 'sum'), (0, 1, 'ratio'),
           (1, 0, 'ratio'), (0, None, 'mean'), (1, None, 'max'),
           (1, None, 'min')]
    got = check_outputs([a, b], w, two, be.daily_reduce([a_d, b_d], w, two))
    again = be.daily_reduce([a_d, b_d], w, two)          # the same bits
    for g, h in zip(got, again):
        same_bits(h, g)
    same_bits(a_d, a)                                    # sources untouched
    same_bits(b_d, b)


def test_daily_reduce_all_nan_window_and_table_limits():
    from sup3r_amd import _lib
    be = backend()
    x = np.full((2, 1, 48), np.nan, np.float32)
    x[1, 0, 30] = 2.5
    outs = [(0, None, op) for op in ('mean', 'max', 'min', 'sum')] + [
        (0, 0, 'ratio')]
    mean, mx, mn, total, ratio = (down(g)[:, 0] for g in be.daily_reduce(
        [up(x)], 24, outs))
    for g in (mean, mx, mn, ratio):
        assert np.isnan(g[0]).all() and np.isnan(g[1, 0])
    assert (total[0] == 0).all() and total[1, 0] == 0 and total[1, 1] == 2.5
    assert mean[1, 1] == mx[1, 1] == mn[1, 1] == 2.5 and ratio[1, 1] == 1.0
    # more sources and outputs than one launch's tables hold
    rng = np.random.default_rng(0)
    srcs = [rng.standard_normal((3, 2, 48)).astype(np.float32)
            for _ in range(_lib.DAILY_MAX_SRC + 3)]
    outs = [(i, None, op) for i in range(len(srcs)) for op in ('mean', 'max')]
    assert len(outs) > _lib.DAILY_MAX_OUT
    check_outputs(srcs, 24, outs,
                  be.daily_reduce([up(s) for s in srcs], 24, outs))


# ------------------------------------------------------------ site day mean
@pytest.mark.parametrize('k', [1, 4, 9])
@pytest.mark.parametrize('m', [24, 48])
def test_site_day_mean(k, m):
    rng = np.random.default_rng(k * m)
    be = backend()
    n_sites, src_days, t_lo, n_pix = 37, 6, 5, 11
    src = (rng.standard_normal((t_lo + src_days * m + 3, n_sites)) * 50
           ).astype(np.float32)
    src[:, 4] = np.nan                                   # a site that is out
    src[t_lo + m:t_lo + 2 * m, 9] = np.nan               # ... for a day
    src[t_lo + 7, 11] = np.nan
    idx = np.stack([rng.choice(n_sites, size=k, replace=False)
                    for _ in range(n_pix)])
    idx[0, 0] = 4                                        # with k = 1: all NaN
    idx[1, :] = np.resize([9, 11, 4], k)
    day_map = np.array([0, 1, -1, 5, 2, 2, 3, 4, -1], np.int32)
    got = down(be.site_day_mean(up(src), idx, t_lo, m, day_map))
    days = src[t_lo:t_lo + src_days * m].astype(np.float64).reshape(
        src_days, m, n_sites)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        site_mean = np.nanmean(days[:, :, idx], axis=-1)        # (d, m, p)
        ref = np.nanmean(site_mean, axis=1)                     # (d, p)
    sum_abs = np.nan_to_num(np.abs(days[:, :, idx])).sum(axis=(1, 3))
    want = np.where(day_map[None, :] < 0, np.nan, ref[day_map].T)
    assert got.shape == (n_pix, len(day_map))
    assert np.isnan(got[:, day_map < 0]).all()
    if k == 1:
        assert np.isnan(got[0]).all()
    assert np.isnan(want).sum() < want.size / 2
    R.assert_close_sum(got, want, sum_abs[day_map].T, f'k={k} m={m}')


# --------------------------------------------------------- scale to time max
@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 4, 63), (2, 5, 365),
                                   (9, 7, 64)])
def test_scale_to_time_max(shape):
    rng = np.random.default_rng(shape[2])
    be = backend()
    a = rng.uniform(0, 400, shape).astype(np.float32)
    b = rng.uniform(0, 900, shape).astype(np.float32)
    if shape[2] > 1:
        a[0, 0, 0] = b[0, 0, -1] = np.nan
        a[-1, -1, :] = np.nan                            # an all-NaN pixel
        b[0, -1, :] = np.nan
        b[-1, 0, :] = 0.0                                # x / 0
    a_d, b_d = up(a), up(b)
    scaled, scale = be.scale_to_time_max(a_d, b_d)
    want_scaled, want_scale = R.scale_clearsky_ghi(a, b)
    same_bits(scale, want_scale, 'scale')
    same_bits(scaled, want_scaled, 'scaled')
    assert scaled.data_ptr() == b_d.data_ptr()           # in place
    same_bits(a_d, a, 'a')


# --------------------------------------------------------------- end to end
def grid_source(s1=8, s2=10, t=96, seed=0):
    from sup3r_amd.derive import DeriveData
    rng = np.random.default_rng(seed)
    arrays = {
        'windspeed_10m': rng.uniform(1, 9, (s1, s2, t)).astype(np.float32),
        'temperature_2m': rng.normal(280, 5, (s1, s2, t)).astype(np.float32),
        'u': rng.normal(0, 3, (s1, s2, t, 3)).astype(np.float32),
        'topography': rng.uniform(0, 900, (s1, s2)).astype(np.float32)}
    return lambda: DeriveData(
        dict(arrays), R.grid_lat_lon(s1, s2),
        pd.date_range('2020-01-01', periods=t, freq='h'),
        level=[1000., 900., 800.])


def both(make, **kwargs):
    """the same construction on the device and on numpy"""
    from sup3r_amd.derive import NumpyBackend
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return make(backend=backend(), **kwargs), make(backend=NumpyBackend(),
                                                       **kwargs)


def test_rasterizer_and_data_handler_match_numpy():
    from sup3r_amd import data_handlers as H
    source = grid_source()
    kw = dict(target=source().lat_lon[6, 1], shape=(4, 5),
              time_slice=[2, 90, 2])
    dev, ref = both(lambda **k: H.DeviceRasterizer(source(), **k), **kw)
    assert dev.features == ref.features and dev.raster_index == ref.raster_index
    for f in ref.features:
        same_bits(dev[f], ref[f], f)
    rng = np.random.default_rng(3)
    flat = {'ghi': rng.uniform(0, 900, (50, 200)).astype(np.float32),
            'elevation': rng.uniform(0, 2000, 200).astype(np.float32)}
    meta = rng.uniform(30, 40, (200, 2))
    index = rng.integers(0, 200, (9, 8))
    dev, ref = both(lambda **k: H.DeviceRasterizer(H.FlatData(
        dict(flat), meta, pd.date_range('2019-06-01', periods=50, freq='h')),
        **k), raster_index=index, time_slice=slice(1, 49, 3))
    for f in ('ghi', 'elevation'):
        same_bits(dev[f], ref[f], f)
    feats = ['temperature_2m', 'windspeed_10m']
    dev, ref = both(lambda **k: H.DataHandler(source(), feats, **k),
                    time_roll=3, nan_method_kwargs={'method': 'mask'}, **kw)
    assert dev.shape == ref.shape == (4, 5, 44, 2)
    assert dev.time_step == 7200.0 and dev.time_index.equals(ref.time_index)
    same_bits(dev.as_array(), ref.as_array())


def check_daily(handler, ops):
    """the daily planes of a device handler against float64 reductions of its
    own hourly planes"""
    for f, op in ops.items():
        hourly = down(handler.data.hourly[f])
        ref, sum_abs = R.reduce64(hourly, 24, op)
        got = down(handler.data.daily[f])
        if op in ('max', 'min'):
            same_bits(got, ref.astype(np.float32), f)
        else:
            R.assert_close_sum(got, ref, sum_abs, f)
    feats = handler.requested_features
    same_bits(handler.daily, np.stack(
        [down(handler.data.daily[f]) for f in feats], axis=-1))
    same_bits(handler.hourly, np.stack(
        [down(handler.data.hourly[f]) for f in feats], axis=-1))


def test_daily_handlers_match_numpy():
    from sup3r_amd import data_handlers as H
    source = grid_source()
    feats = ['temperature_2m', 'temperature_max_2m', 'temperature_min_2m']
    for cls in (H.DailyDataHandler, H.DataHandlerH5WindCC):
        registry = ({'FeatureRegistry': H.RegistryH5WindCC}
                    if cls is H.DailyDataHandler else {})
        dev, ref = both(lambda **k: cls(source(), feats, **k),
                        shape=(5, 6), target=source().lat_lon[7, 2],
                        **registry)
        assert dev.daily.shape == ref.daily.shape == (5, 6, 4, 3)
        same_bits(dev.hourly, ref.hourly)
        for f in feats[1:]:
            same_bits(dev.data.daily[f], ref.data.daily[f], f)
        check_daily(dev, dict(zip(feats, ('mean', 'max', 'min'))))
        assert dev.daily_time_index.equals(ref.daily_time_index)


def solar_source(s1=6, s2=6, days=8):
    from sup3r_amd.derive import DeriveData
    planes = R.solar_planes(s1, s2, days)
    return lambda: DeriveData(
        dict(planes), R.grid_lat_lon(s1, s2),
        pd.date_range('2018-03-01', periods=24 * days, freq='h'))


def test_solar_cc_handler_matches_numpy_and_feeds_the_batch_handler():
    import torch
    from sup3r_amd import DeviceBatchHandlerCC
    from sup3r_amd import data_handlers as H
    source = solar_source()
    feats = ['clearsky_ratio', 'temperature_2m']
    dev, ref = both(lambda **k: H.DataHandlerH5SolarCC(source(), feats, **k))
    same_bits(dev.hourly, ref.hourly)          # the ratio: one fp32 division
    check_daily(dev, {'temperature_2m': 'mean'})
    tot = {k: down(v) for k, v in dev.totals.items()}
    for name, src in (('total_ghi', 'ghi'),
                      ('total_clearsky_ghi', 'clearsky_ghi')):
        ref64, sum_abs = R.reduce64(source()[src], 24, 'sum')
        R.assert_close_sum(tot[name], ref64, sum_abs, name)
    same_bits(dev.data.daily['clearsky_ratio'],
              tot['total_ghi'] / tot['total_clearsky_ghi'])
    assert not torch.isnan(dev.daily).any()
    bh = DeviceBatchHandlerCC.from_containers(
        [dev], sample_shape=(4, 4, 72), batch_size=2, n_batches=2,
        s_enhance=2, t_enhance=24, seed=1)
    batch = next(iter(bh))
    bh.stop()
    assert tuple(batch.low_res.shape) == (2, 2, 2, 3, 2)
    assert tuple(batch.high_res.shape)[:3] == (2, 4, 4)
    assert tuple(batch.high_res.shape)[4] == 2
    assert not torch.isnan(batch.low_res).any()
    assert set(bh.means) == set(feats)


def test_nc_cc_handlers_match_the_reference():
    from sup3r_amd import data_handlers as H
    from sup3r_amd.derive import DeriveData
    rng = np.random.default_rng(2)
    days, s1, s2 = 40, 3, 4
    ti = pd.date_range('2019-02-10 12:00', periods=days, freq='D')
    arrays = {'rsds': rng.uniform(50, 400, (s1, s2, days)).astype(np.float32),
              'uas': rng.normal(0, 4, (s1, s2, days)).astype(np.float32)}
    arrays['rsds'][1, 2, :] = np.nan
    lat_lon = R.grid_lat_lon(s1, s2, d=1.0)
    ti_ns = pd.date_range('2019-01-01', '2020-01-01', freq='30min',
                          inclusive='left')
    hour = np.asarray(ti_ns.hour + ti_ns.minute / 60)
    sun = np.clip(np.sin((hour - 6) / 12 * np.pi), 0, None)
    cs = (1000 * sun[:, None] * rng.uniform(0.7, 1, (1, 60))).astype(
        np.float32)
    cs[3000:3100, 7] = np.nan
    meta = np.stack([rng.uniform(36, 43, 60), rng.uniform(-106, -101, 60)], -1)
    ns = H.FlatData({'clearsky_ghi': cs}, meta, ti_ns)

    def make(features, cls=H.DataHandlerNCforCC, **k):
        return cls(DeriveData(dict(arrays), lat_lon, ti), features,
                   nsrdb_source_fp=ns, nsrdb_agg=4, **k)
    be = backend()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        off = make(['clearsky_ghi'], scale_clearsky_ghi=False, backend=be)
        on = make(['clearsky_ratio', 'clearsky_ghi'], backend=be)
        law = make(['u_100m'], cls=H.DataHandlerNCforCCwithPowerLaw,
                   backend=be)
    want, sum_abs, _ = R.get_clearsky_ghi(lat_lon, ti, meta, ti_ns, cs, 4)
    off_cs = down(off['clearsky_ghi'])
    R.assert_close_sum(off_cs, want, sum_abs, 'clearsky_ghi')
    scaled, scale = R.scale_clearsky_ghi(arrays['rsds'], off_cs)
    same_bits(on._cs_ghi_scale, scale)
    same_bits(on['clearsky_ghi'], scaled)
    with np.errstate(all='ignore'):
        ratio = np.maximum(np.minimum(arrays['rsds'] / scaled, 1), 0)
    same_bits(on['clearsky_ratio'], ratio)
    same_bits(law['u_100m'], arrays['uas'] * np.float32((100 / 10) ** 0.2))
