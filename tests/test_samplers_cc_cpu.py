"""CPU tests of ``sup3r_amd.samplers_cc``: the numpy restatement
``tests/cc_ref.py`` against scipy's distance transform (the tie rule the device
fill is built on), the first hour of the daylight window, the middle days on
the reference's own cases, and ``DeviceDualSamplerCC``'s index logic over
stand-in gathers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import cc_ref  # noqa: E402

CSR = 'clearsky_ratio'


# ---------------------------------------------------------------- the fill
def holes_uniform(rng, shape, p):
    return rng.random(shape) < p


def holes_night(rng, shape, extra):
    """night bands: every pixel has its own sunrise and sunset hour; ``extra``:
    share of further holes sprinkled over the day"""
    n, s1, s2, t = shape
    rise = rng.integers(4, 9, size=(n, s1, s2, 1))
    sset = rng.integers(16, 21, size=(n, s1, s2, 1))
    hour = np.arange(t).reshape(1, 1, 1, t) % 24
    holes = (hour < rise) | (hour >= sset)
    if extra:
        holes = holes | (rng.random(shape) < extra)
    return holes


MASK_KINDS = [lambda r, s: holes_uniform(r, s, 0.2),
              lambda r, s: holes_uniform(r, s, 0.6),
              lambda r, s: holes_uniform(r, s, 0.95),
              lambda r, s: holes_night(r, s, 0.0),
              lambda r, s: holes_night(r, s, 0.05)]


def test_cc_ref_fill_picks_the_sources_scipy_picks():
    """indices equal element for element, over enough filled elements and
    enough TIED ones (the same pixel an hour earlier and the neighbouring pixel
    in the same hour are both at distance 1) that the tie rule is what is
    tested"""
    nd = pytest.importorskip('scipy.ndimage')
    filled = tied = 0
    for seed in range(40):
        rng = np.random.default_rng(seed)
        shape = tuple(int(v) for v in rng.integers(1, 8, size=3)) + (
            int(rng.integers(2, 30)),)
        holes = MASK_KINDS[seed % len(MASK_KINDS)](rng, shape)
        if holes.all():
            holes[tuple(rng.integers(0, d) for d in shape)] = False
        want = nd.distance_transform_edt(holes, return_distances=False,
                                         return_indices=True)
        got = cc_ref.nn_fill_indices(holes)
        np.testing.assert_array_equal(got, want, err_msg=f'{seed} {shape}')
        filled += int(holes.sum())
        tied += cc_ref.tied_fills(holes)
    assert filled >= 10000, filled
    assert 3 * tied >= filled, (tied, filled)


def test_cc_ref_fill_moves_bit_patterns_and_leaves_the_rest():
    block = np.random.default_rng(1).standard_normal(
        (2, 3, 2, 5, 3)).astype(np.float32)
    block[..., 1][np.random.default_rng(2).random((2, 3, 2, 5)) < 0.5] = np.nan
    block[0, 0, 0, 0, 0] = np.nan                # another channel's NaN stays
    block[1, 2, 1, 4, 1] = -0.0
    out, found = cc_ref.nn_fill(block, 1)
    assert found == int(np.isnan(block[..., 1]).sum()) > 0
    assert not np.isnan(out[..., 1]).any()
    assert np.isnan(out[0, 0, 0, 0, 0])
    keep = ~np.isnan(block)
    np.testing.assert_array_equal(out.view(np.uint32)[keep],
                                  block.view(np.uint32)[keep])
    all_nan = np.full((1, 2, 2, 3, 1), np.nan, dtype=np.float32)
    out, found = cc_ref.nn_fill(all_nan, 0)
    assert found == 12 and np.isnan(out).all()


# ------------------------------------------------------- the daylight window
def night_of(day_hours):
    night = np.ones(24, dtype=bool)
    night[list(day_hours)] = False
    return night


# daylight hours, clamped start, unclamped start
WINDOW_CASES = [
    (range(7, 18), 6, 6),
    (range(5, 19), 6, 6),        # padding -2: ceil(-1) = -1
    (range(4, 19), 5, 5),        # fifteen hours: padding -3, ceil(-1.5) = -1
    (range(0, 8), 0, -2),
    (range(16, 24), 12, 14),
    ([0, 1, 2, 3, 20, 21, 22, 23], 0, -2),   # split daylight: first 0, n_day 8
    ([], 6, 6),                  # all night: the centred window
]


def reference_slice(data, shape, csr_ind):
    """the slicing of nsrdb_reduce_daily_data on a numpy array, with the
    reference's own steps: hours with any NaN are night, the day hours are
    listed, half of the padding (rounded up) is taken off the first"""
    dark = np.isnan(data[:, :, :, :, csr_ind]).any(axis=(0, 1, 2))
    lit = np.where(~dark)[0]
    half_pad = int(np.ceil((shape - len(lit)) / 2))
    first = lit[0] - half_pad
    return data[..., slice(first, first + shape), :]


@pytest.mark.parametrize('day,start,raw', WINDOW_CASES,
                         ids=[str(i) for i in range(len(WINDOW_CASES))])
def test_window_start(day, start, raw):
    from sup3r_amd.samplers_cc import nsrdb_reduce_daily_data
    t = 12
    night = night_of(day)
    assert cc_ref.window_start(night, t) == (raw, start)
    # a batch whose second channel is the clearsky ratio: NaN at night in ONE
    # pixel of one sample each hour; the first channel counts the hours
    data = np.zeros((2, 2, 3, 24, 2), dtype=np.float32)
    data[..., 0] = np.arange(24)
    for k in np.flatnonzero(night):
        data[k % 2, (k // 2) % 2, k % 3, k, 1] = np.nan
    got = nsrdb_reduce_daily_data(data, t, csr_ind=1, clamp=True)
    assert got.shape == (2, 2, 3, t, 2)
    np.testing.assert_array_equal(got[0, 0, 0, :, 0], np.arange(start, start + t))
    if len(list(day)) and 0 <= raw <= 24 - t:
        want = reference_slice(data, t, 1)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        ref = nsrdb_reduce_daily_data(data, t, csr_ind=1)       # as the reference
        np.testing.assert_array_equal(ref.view(np.uint32), want.view(np.uint32))
    elif not len(list(day)):
        # the reference hands the 24 hours back
        assert nsrdb_reduce_daily_data(data, t, csr_ind=1).shape[3] == 24


@pytest.mark.parametrize('t,t_enhance,raw,lo,hi,reduced', [
    (72, 24, 72, 0, 72, False), (72, 8, 216, 72, 144, False),
    (24, 8, 72, 24, 48, False), (12, 3, 96, 36, 60, True),
    (33, 3, 264, 116, 149, False)])
def test_get_middle_days_on_the_reference_cases(t, t_enhance, raw, lo, hi,
                                                reduced):
    from sup3r_amd.samplers_cc import DeviceDualSamplerCC
    assert raw == 24 * (t // t_enhance)
    hours = np.arange(raw, dtype=np.float32).reshape(1, 1, 1, raw, 1)
    if t_enhance == 24:
        got = hours                   # the reference does not cut at all
        assert cc_ref.middle_days(raw, t) in ((lo, hi - lo), (0, raw))
    else:
        got = DeviceDualSamplerCC.get_middle_days(hours, (4, 4, t))
        assert cc_ref.middle_days(raw, t) == (lo, hi - lo)
    np.testing.assert_array_equal(got[0, 0, 0, :, 0], np.arange(lo, hi))
    assert (t < got.shape[3]) == reduced


# -------------------------------------------------- the sampler, stand-ins
class StandIns:
    """numpy gathers over host cubes that record what they were asked for"""

    def __init__(self, daily, hourly, lr_box, hr_box):
        self.cubes = {'low_res': daily, 'high_res': hourly}
        self.boxes = {'low_res': lr_box, 'high_res': hr_box}
        self.calls, self.fills = [], 0

    def gather(self, name):
        def run(origins, channels):
            b1, b2, bt = self.boxes[name]
            self.calls.append((name, origins.copy(), list(channels)))
            return np.stack([self.cubes[name][i:i + b1, j:j + b2, k:k + bt]
                             [..., channels] for i, j, k in origins])
        return run

    def fill(self, high, channel):
        self.fills += 1
        return cc_ref.nn_fill(high, channel)[0]

    def as_dict(self, with_fill=True):
        d = {n: self.gather(n) for n in self.cubes}
        if with_fill:
            d['nn_fill'] = self.fill
        return d


def solar_cubes(days, S=8, seed=0, offset_per_column=1):
    """daily (S, S, days, 2) and hourly (S, S, 24 days, 2) with channels
    (clearsky_ratio, temperature): the ratio is NaN at night, the night starts
    at a different hour in every column"""
    rng = np.random.default_rng(seed)
    hourly = rng.uniform(0.1, 1.0, (S, S, 24 * days, 2)).astype(np.float32)
    hour = np.arange(24 * days) % 24
    for j in range(S):
        shift = (j * offset_per_column) % 5
        dark = (hour < 6 + shift) | (hour >= 17 + shift)
        hourly[:, j, dark, 0] = np.nan
    daily = np.nanmean(hourly.reshape(S, S, days, 24, 2), axis=3).astype(
        np.float32)
    return daily, hourly


FEATS = [CSR, 'temperature']


def make_sampler(daily, hourly, sample_shape, t_enhance, batch_size=3,
                 s_enhance=1, seed=5, feature_sets=None, with_fill=True,
                 hr_features=FEATS):
    from sup3r_amd.samplers_cc import DeviceDualSamplerCC
    s1, s2, t = sample_shape
    lt = t // t_enhance
    raw = lt * (1 if t_enhance == 1 else 24)
    lr_src = daily
    if s_enhance > 1:
        from sup3r_amd.samplers_cc import coarsen_daily
        lr_src = coarsen_daily(daily, s_enhance)
    hr_src = daily if t_enhance == 1 else hourly
    stand = StandIns(lr_src, hr_src, (s1 // s_enhance, s2 // s_enhance, lt),
                     (s1, s2, raw))
    smp = DeviceDualSamplerCC(
        daily, hourly, FEATS, hr_features, sample_shape,
        batch_size=batch_size, s_enhance=s_enhance, t_enhance=t_enhance,
        feature_sets=feature_sets, seed=seed,
        gather=stand.as_dict(with_fill))
    return smp, stand


def test_sampler_draws_replay_and_the_hourly_slice_is_24_times_the_daily():
    daily, hourly = solar_cubes(days=20)
    smp, stand = make_sampler(daily, hourly, (4, 4, 12), t_enhance=3)
    assert smp.lr_sample_shape == (4, 4, 4)
    assert smp._fast_batch_possible()            # 24 * 4 * 3 <= 480
    rng = np.random.default_rng(5)
    for _ in range(3):
        lr_ix, hr_ix = smp.get_sample_index()
        i0, j0 = rng.integers(0, 8 - 4 + 1), rng.integers(0, 8 - 4 + 1)
        k0 = rng.integers(0, 20 - 4 * 3 + 1)
        assert lr_ix[:3] == (slice(i0, i0 + 4), slice(j0, j0 + 4),
                             slice(k0, k0 + 12))
        assert hr_ix[:3] == (slice(i0, i0 + 4), slice(j0, j0 + 4),
                             slice(24 * k0, 24 * (k0 + 12)))
        assert hr_ix[3] == [CSR, 'temperature']
    twin, _ = make_sampler(daily, hourly, (4, 4, 12), t_enhance=3)
    for _ in range(3):
        twin.get_sample_index()
    a, b = next(smp), next(twin)
    np.testing.assert_array_equal(smp.last_origins, twin.last_origins)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize('days', [20, 6])      # 6 days: slow but for one day a sample
@pytest.mark.parametrize('t,t_enhance', [(12, 3), (24, 8), (24, 24), (48, 24)])
def test_sampler_batches_are_cc_ref(t, t_enhance, days):
    daily, hourly = solar_cubes(days=days)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # the slow-batch warning
        smp, stand = make_sampler(daily, hourly, (4, 6, t), t_enhance,
                                  batch_size=4)
    lt = t // t_enhance
    fast = 24 * lt * 4 <= 24 * days
    assert smp._fast_batch_possible() == fast
    assert fast == (days == 20 or lt == 1)
    low, high = next(smp)
    lr_org, hr_org = smp.last_lr_origins, smp.last_origins
    np.testing.assert_array_equal(hr_org, lr_org * [1, 1, 24])
    if fast:
        np.testing.assert_array_equal(np.diff(lr_org[:, 2]), lt)
        assert (lr_org[:, :2] == lr_org[0, :2]).all()
    want_low, want_high, info = cc_ref.cc_next(
        daily, hourly, lr_org, hr_org, (4, 6, lt), (4, 6, t), t_enhance,
        [0, 1], [0, 1], 0)
    assert high.shape == (4, 4, 6, t, 2) and low.shape == (4, 4, 6, lt, 2)
    np.testing.assert_array_equal(low.view(np.uint32), want_low.view(np.uint32))
    np.testing.assert_array_equal(high.view(np.uint32),
                                  want_high.view(np.uint32))
    assert not np.isnan(high[..., 0]).any() and stand.fills == 1
    assert (info['start'] is not None) == (t < 24)
    # the low-res batch is the daily slice of the same days
    for m, (i, j, k) in enumerate(lr_org):
        np.testing.assert_array_equal(low[m], daily[i:i + 4, j:j + 6, k:k + lt])


def test_sampler_t_enhance_1_pairs_daily_with_itself():
    daily, hourly = solar_cubes(days=12)
    smp, stand = make_sampler(daily, hourly, (4, 4, 1), t_enhance=1,
                              s_enhance=2)
    assert smp._hr.shape == daily.shape and smp._lr.shape == (4, 4, 12, 2)
    low, high = next(smp)
    assert low.shape == (3, 2, 2, 1, 2) and high.shape == (3, 4, 4, 1, 2)
    assert stand.fills == 0
    for m, (i, j, k) in enumerate(smp.last_origins):
        np.testing.assert_array_equal(high[m], daily[i:i + 4, j:j + 4, k:k + 1])
    np.testing.assert_array_equal(smp.last_origins, smp.last_lr_origins * [2, 2, 1])


def test_sampler_s_enhance_coarsens_daily_by_block_means():
    from sup3r_amd.samplers_cc import coarsen_daily
    daily, hourly = solar_cubes(days=6)
    coarse = coarsen_daily(daily, 2)
    assert coarse.shape == (4, 4, 6, 2) and coarse.dtype == np.float32
    want = np.mean([daily[a::2, b::2].astype(np.float64)
                    for a in (0, 1) for b in (0, 1)], axis=0)
    # four float32 values summed and divided by four: a few ulps of values < 1
    assert np.abs(coarse - want).max() <= 4 * 2.0 ** -24
    with pytest.warns(UserWarning):              # 24 * 1 * 8 > 24 * 6: slow
        smp, _ = make_sampler(daily, hourly, (4, 4, 24), t_enhance=24,
                              s_enhance=2, batch_size=8)
    low, high = next(smp)
    assert low.shape == (8, 2, 2, 1, 2) and high.shape == (8, 4, 4, 24, 2)
    for m, (i, j, k) in enumerate(smp.last_lr_origins):
        np.testing.assert_array_equal(low[m], coarse[i:i + 2, j:j + 2, k:k + 1])
    with pytest.raises(AssertionError, match='no multiple'):
        coarsen_daily(daily[:7], 2)


def test_sampler_shape_assertion_fires():
    daily, hourly = solar_cubes(days=6)
    with pytest.raises(AssertionError, match='not compatible'):
        make_sampler(daily, hourly[:, :, :-24], (4, 4, 24), t_enhance=24)
    with pytest.raises(AssertionError, match='not compatible'):
        # t_enhance = 3 still wants 24 hourly steps per daily step
        make_sampler(daily, hourly[:, :, :18], (4, 4, 3), t_enhance=3)


def test_sampler_without_clearsky_output_reduces_and_fills_nothing():
    daily, hourly = solar_cubes(days=20)
    smp, stand = make_sampler(
        daily, hourly, (4, 4, 12), t_enhance=3,
        feature_sets={'lr_only_features': [CSR]})
    assert smp.hr_out_features == ['temperature'] and smp.csr_index is None
    low, high = next(smp)
    # the parent's batch on the 24 x slice: all 96 raw hours
    assert high.shape == (3, 4, 4, 96, 1) and stand.fills == 0
    for m, (i, j, k) in enumerate(smp.last_origins):
        np.testing.assert_array_equal(
            high[m], hourly[i:i + 4, j:j + 4, k:k + 96][..., [1]])
    # clearsky ratio as an exogenous feature is no output either
    smp, stand = make_sampler(
        daily, hourly, (4, 4, 12), t_enhance=3,
        hr_features=['temperature', CSR],
        feature_sets={'hr_exo_features': [CSR]})
    assert smp.csr_index is None
    assert next(smp)[1].shape == (3, 4, 4, 96, 2) and stand.fills == 0


def test_names_are_exported():
    import sup3r_amd
    for name in ('DeviceDualSamplerCC', 'DualSamplerCC', 'DeviceBatchHandlerCC',
                 'BatchHandlerCC'):
        assert name in sup3r_amd.__all__ and hasattr(sup3r_amd, name)
    assert sup3r_amd.DualSamplerCC is sup3r_amd.DeviceDualSamplerCC
    assert sup3r_amd.BatchHandlerCC is sup3r_amd.DeviceBatchHandlerCC
    assert issubclass(sup3r_amd.BatchHandlerCC, sup3r_amd.DeviceDualBatchHandler)


def test_header_declares_the_cc_entry_points():
    import re
    from sup3r_amd import _lib
    root = os.path.join(os.path.dirname(__file__), '..')
    with open(os.path.join(root, 'include', 'sup3r_hip.h')) as f:
        header = f.read()
    for name in ('s3_nn_fill', 's3_cc_night_mask', 's3_cc_window_gather'):
        assert re.search(rf'\bint\s+{name}\s*\(', header)
        assert name in _lib.EXPORTS
    for name, value in (('S3_NN_FILL_MAX_AXIS', _lib.NN_FILL_MAX_AXIS),
                        ('S3_CC_STATUS_WORDS', _lib.CC_STATUS_WORDS),
                        ('S3_CC_NIGHT_MASK', _lib.CC_NIGHT_MASK),
                        ('S3_CC_START_RAW', _lib.CC_START_RAW),
                        ('S3_CC_START', _lib.CC_START),
                        ('S3_CC_FILLED', _lib.CC_FILLED)):
        assert re.search(rf'#define {name} {value}\b', header)
