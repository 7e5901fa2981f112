"""CPU checks of the bias-correction feature: the host planning of
``sup3r_amd.bias`` (indices, weights, mirrored table rows, grid matching,
errors and warnings), the strategy's record and the new ABI symbol.  No kernel
runs here.  (The restatement's own properties: tests/test_bias_ref_cpu.py.)"""
import os
import re
import warnings

import numpy as np
import pandas as pd
import pytest

from tests import bias_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ti(start, periods, freq='6h'):
    return pd.date_range(start, periods=periods, freq=freq)


# ----------------------------------------------------------- host planning
def test_month_and_window_indices_mirrored_along_time():
    from sup3r_amd import bias as B
    ti = _ti('2015-01-30', 12)                       # Jan 30 .. Feb 1
    months = ti.month.values - 1
    for pad in ((0, 0), (2, 0), (0, 3), (2, 3)):
        want = np.pad(months, pad, mode='reflect')
        np.testing.assert_array_equal(B.month_index(ti, pad), want)
        assert B.month_index(ti, pad).dtype == np.int32
    w, distinct = B.month_weights(ti)
    assert distinct == 2 and w.shape == (12,) and w.sum() == 1.0
    np.testing.assert_array_equal(w[:2], [8 / 12, 4 / 12])
    # weights stand for the mean over the gathered months
    tab = np.random.default_rng(0).uniform(0.5, 2, (3, 2, 12))
    np.testing.assert_allclose((tab * w).sum(-1), tab[..., months].mean(-1),
                               rtol=1e-14)
    # windows: argmin |doy - center|, the FIRST minimum on a tie
    centers = np.array([10.0, 20.0, 30.0])
    days = pd.DatetimeIndex(['2015-01-14', '2015-01-15', '2015-01-16',
                             '2015-01-25', '2015-12-31'])
    idx = B.window_index(days, centers)
    np.testing.assert_array_equal(idx, [0, 0, 1, 1, 2])     # doy 15: tie -> 0
    np.testing.assert_array_equal(idx, R.closest_time_idx(days, centers))
    np.testing.assert_array_equal(B.window_index(days, centers, (2, 1)),
                                  np.pad(idx, (2, 1), mode='reflect'))


def test_mirrored_rows_equal_np_pad_reflect_for_every_edge_pad():
    from sup3r_amd import bias as B
    rng = np.random.default_rng(1)
    for extent in (1, 2, 3, 7):
        row = rng.standard_normal(extent)
        for lo in range(0, 4):
            for hi in range(0, 4):
                if extent == 1 and (lo or hi):
                    continue              # np.pad cannot reflect one cell
                if max(lo, hi) > extent - 1 and extent < 3:
                    continue
                m = B.mirror_index(lo + extent + hi, lo, extent)
                np.testing.assert_array_equal(
                    row[m], np.pad(row, (lo, hi), mode='reflect'))
    # two chunks of one padded shape with different (lo, hi), through the
    # plan's geometry: table window (origin + mirror) == padded factor window
    table = rng.standard_normal((9, 8))
    plan = B.BiasPlan('local_linear_bc',
                      {'u': dict(bias_fp={'u_scalar': table,
                                          'u_adder': table})}, ['u'])
    wins = [B.ChunkWindow((slice(0, 5), slice(2, 8)), ((1, 0), (0, 1))),
            B.ChunkWindow((slice(4, 9), slice(1, 7)), ((0, 1), (1, 0)))]
    geo = plan.geometry(wins, (6, 7))
    np.testing.assert_array_equal(geo, [[0, 2, 1, 0, 5, 6],
                                        [4, 1, 0, 1, 5, 6]])
    for g, w in zip(geo, wins):
        o1, o2, lo1, lo2, e1, e2 = (int(v) for v in g)
        rows = o1 + B.mirror_index(6, lo1, e1)
        cols = o2 + B.mirror_index(7, lo2, e2)
        np.testing.assert_array_equal(
            table[np.ix_(rows, cols)],
            np.pad(table[w.lr_pad_slice], w.pad_width[:2], mode='reflect'))
    with pytest.raises(ValueError, match='do not match lr_pad_slice'):
        plan.geometry(wins, (7, 7))


def _grid(n1, n2):
    lat = np.linspace(45, 40, n1)[:, None] + np.zeros((1, n2))
    lon = np.linspace(-110, -104, n2)[None] + np.zeros((n1, 1))
    return lat, lon


def test_grid_window_lookup_and_threshold():
    from sup3r_amd import bias as B
    lat, lon = _grid(11, 13)
    tab = np.arange(11 * 13, dtype=np.float32).reshape(11, 13)
    params = B.BiasParams.load({'u_scalar': tab, 'u_adder': tab,
                                'latitude': lat, 'longitude': lon})
    dom = np.stack([lat[3:8, 2:9], lon[3:8, 2:9]], -1)
    assert B.grid_window(params, dom) == (3, 2)
    assert B.grid_window(params, None) is None
    f = B._Feature('local_linear_bc', 'u', dict(bias_fp=params), dom)
    np.testing.assert_array_equal(f.tables['scalar'][..., 0], tab[3:8, 2:9])
    with pytest.raises(RuntimeError, match='threshold'):
        B.grid_window(params, dom + 0.2, threshold=0.1)
    assert B.grid_window(params, dom + 0.04, threshold=0.1) == (3, 2)
    # a 6-row window whose lower-left corner sits on grid row 2
    far = np.zeros((6, 3, 2))
    far[-1, 0] = lat[2, 0], lon[2, 0]
    with pytest.raises(RuntimeError, match='leaves'):
        B.grid_window(params, far)
    # without coordinates the tables must already have the domain's shape
    with pytest.raises(ValueError, match='no latitude'):
        B._Feature('local_linear_bc', 'u',
                   dict(bias_fp={'u_scalar': tab, 'u_adder': tab}), dom)
    with pytest.raises(AssertionError, match='Missing v_scalar'):
        B._Feature('local_linear_bc', 'v', dict(bias_fp=params), dom)


def test_npz_source_and_attributes(tmp_path):
    from sup3r_amd import bias as B
    fp = R.seeded_qdm_tables(np.random.default_rng(2), (3, 2), 2, 11,
                             presrat=True)
    path = os.path.join(str(tmp_path), 'bc.npz')
    np.savez(path, **fp)
    f = B._Feature('local_presrat_bc', 'rsds',
                   dict(bias_fp=path, base_dset='ghi', k_range=(0.9, 1.1)))
    assert f.kind == B._lib.BC_QDM and (f.n_t, f.n_q) == (2, 11)
    assert f.flags & B._lib.BC_PRESRAT and f.flags & B._lib.BC_RELATIVE
    # delta_denom_min defaults to the source's zero_rate_threshold
    assert f.flags & B._lib.BC_DENOM_MIN
    assert f.limits['denom_min'] == pytest.approx(1.182033e-5)
    assert f.tables['kfac'].min() >= np.float32(0.9) and \
        f.tables['kfac'].max() <= np.float32(1.1)
    assert f.tables['tau'].shape == (3, 2)
    with pytest.raises(ValueError, match='npz'):
        B.BiasParams.load('factors.h5')


def test_unsupported_options_and_warnings():
    from sup3r_amd import bias as B
    rng = np.random.default_rng(7)
    fp = R.seeded_qdm_tables(rng, (3, 2), 2, 11)
    kw = dict(base_dset='ghi')
    with pytest.raises(KeyError, match='dist="weibull_min"'):
        B._Feature('local_qdm_bc', 'rsds',
                   dict(kw, bias_fp=dict(fp, dist='weibull_min')))
    for sampling in ('log', 'invlog'):
        with pytest.raises(KeyError, match=f'sampling="{sampling}"'):
            B._Feature('local_qdm_bc', 'rsds',
                       dict(kw, bias_fp=dict(fp, sampling=sampling)))
    with pytest.raises(KeyError, match='unknown bias correction method'):
        B._Feature('cubic_bc', 'rsds', {})
    lin = R.seeded_linear_tables(rng, (4, 3))
    # a missing temporal_avg keyword (bias/utilities.py:272-284)
    with pytest.warns(UserWarning, match='"temporal_avg" was not provided'):
        plan = B.BiasPlan('monthly_local_linear_bc',
                          {'u_10m': dict(bias_fp=lin)}, ['u_10m', 'v_10m'])
    assert plan.features[1] is None and plan.features[0].month_mode == \
        'weights'
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        plan = B.BiasPlan('monthly_local_linear_bc',
                          {'u_10m': dict(bias_fp=lin, temporal_avg=True)},
                          ['u_10m'])
        # two months: no warning
        plan.time_plan([B.ChunkWindow((slice(0, 4), slice(0, 3)), None,
                                      _ti('2015-01-29', 20))], 20)
    # more than two months averaged (bias_transforms.py:449-455)
    with pytest.warns(UserWarning, match='>2 months'):
        plan.time_plan([B.ChunkWindow((slice(0, 4), slice(0, 3)), None,
                                      _ti('2015-01-29', 300))], 300)
    # NaN in the factors of the chunk's window — once per window
    bad = {k: v.copy() for k, v in lin.items()}
    bad['u_10m_scalar'][3, 2, 4] = np.nan
    plan = B.BiasPlan('monthly_local_linear_bc',
                      {'u_10m': dict(bias_fp=bad, temporal_avg=False)},
                      ['u_10m'])
    geo = plan.geometry([B.ChunkWindow((slice(0, 2), slice(0, 3)))], (2, 3))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        plan._warn_nan(geo)                                   # NaN not inside
    geo = plan.geometry([B.ChunkWindow((slice(2, 4), slice(0, 3)))], (2, 3))
    with pytest.warns(UserWarning, match='had NaNs for "u_10m"'):
        plan._warn_nan(geo)
    # planning errors
    with pytest.raises(ValueError, match='low-res time index'):
        plan.time_plan([B.ChunkWindow((slice(0, 2), slice(0, 3)))], 4)
    with pytest.raises(AssertionError, match='Time should align'):
        plan.time_plan([B.ChunkWindow((slice(0, 2), slice(0, 3)), None,
                                      _ti('2015-01-01', 5))], 4)
    with pytest.raises(ValueError, match='names \\[\'w\'\\]'):
        B.BiasPlan('local_linear_bc', {'w': dict(bias_fp=lin)}, ['u_10m'])
    with pytest.raises(TypeError, match='unexpected keyword'):
        B._Feature('local_linear_bc', 'u_10m', dict(bias_fp=lin, k_range=1))
    with pytest.raises(AssertionError, match='needs 3D scalars'):
        B._Feature('monthly_local_linear_bc', 'u_10m', dict(
            bias_fp={k: v[..., 0] for k, v in lin.items()}))


def test_array_strategy_defaults_attach_no_record():
    from sup3r_amd.strategy import ArrayStrategy
    rng = np.random.default_rng(8)
    domain = rng.standard_normal((10, 8, 9, 2)).astype(np.float32)
    kw = dict(s_enhance=2, t_enhance=1)
    st = ArrayStrategy(domain, {}, (5, 4, 4), **kw)
    for i in range(st.n_chunks):
        assert st.init_chunk(i).bias_correct is None
    lin = R.seeded_linear_tables(rng, (10, 8))
    bc = {'u_10m': dict(bias_fp=lin, temporal_avg=True)}
    with pytest.raises(ValueError, match='input_time_index'):
        ArrayStrategy(domain, {}, (5, 4, 4), bias_correct_method=
                      'monthly_local_linear_bc', bias_correct_kwargs=bc, **kw)
    with pytest.raises(KeyError, match='unknown bias_correct_method'):
        ArrayStrategy(domain, {}, (5, 4, 4), bias_correct_method='nope',
                      bias_correct_kwargs=bc, **kw)
    ti = _ti('2015-01-30', 9)
    st = ArrayStrategy(domain, {}, (5, 4, 4), spatial_pad=1, temporal_pad=1,
                       bias_correct_method='monthly_local_linear_bc',
                       bias_correct_kwargs=bc, input_time_index=ti, **kw)
    c = st.init_chunk(st.n_chunks - 1)
    rec = c.bias_correct
    assert rec.method == 'monthly_local_linear_bc' and rec.kwargs is bc
    assert rec.lr_pad_slice == c.lr_pad_slice
    assert list(rec.time_index) == list(ti[c.lr_pad_slice[2]])
    # input_data stays raw
    np.testing.assert_array_equal(c.input_data, domain[c.lr_pad_slice])
    assert st.init_chunk(0).bias_correct.shared is rec.shared
    # local_linear_bc needs no time index
    st = ArrayStrategy(domain, {}, (5, 4, 4), bias_correct_method=
                       'local_linear_bc', bias_correct_kwargs=bc, **kw)
    assert st.init_chunk(0).bias_correct.time_index is None


def test_bias_symbol_is_declared_exported_and_bound():
    from sup3r_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'sup3r_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'\bint\s+s3_bias_correct\s*\(', header)
    assert 's3_bias_correct' in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsup3r_hip.so not built (run __graft_entry__.build())')
    fn = _lib.lib().s3_bias_correct
    assert len(fn.argtypes) == 19
    # the descriptor's ctypes layout is the C struct's: 4 ints, 7 pointers,
    # 10 floats
    import ctypes as C
    assert C.sizeof(_lib.BiasChannel) == 4 * 4 + 7 * 8 + 10 * 4
    for name, value in re.findall(r'#define S3_BC_([A-Z_]+) (\d+)u?', header):
        assert getattr(_lib, f'BC_{name}') == int(value), name


def test_tables_must_have_the_domain_shape_without_coordinates():
    from sup3r_amd import bias as B
    rng = np.random.default_rng(9)
    lin = R.seeded_linear_tables(rng, (10, 8))
    kw = {'u_10m': dict(bias_fp=lin, temporal_avg=True)}
    plan = B.BiasPlan('monthly_local_linear_bc', kw, ['u_10m'],
                      domain_shape=(10, 8))
    assert plan.grid == (10, 8)
    # larger (or smaller) tables are refused, not read from their corner
    for shape in ((9, 8), (12, 8), (10, 7)):
        with pytest.raises(ValueError, match='low-res domain is'):
            B.BiasPlan('monthly_local_linear_bc', kw, ['u_10m'],
                       domain_shape=shape)
    # the strategy hands the domain's shape over with every record
    from sup3r_amd.strategy import ArrayStrategy
    domain = rng.standard_normal((9, 8, 6, 1)).astype(np.float32)
    st = ArrayStrategy(domain, {}, (5, 4, 4), s_enhance=2, t_enhance=1,
                       bias_correct_method='monthly_local_linear_bc',
                       bias_correct_kwargs=kw,
                       input_time_index=_ti('2015-01-30', 6))
    assert st.init_chunk(0).bias_correct.domain_shape == (9, 8)
