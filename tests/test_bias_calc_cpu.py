"""CPU tests of ``sup3r_amd.bias_calc``: the host planning and the classes'
plumbing, with ``tests/bias_calc_ref.py``'s numpy ``Backend`` injected where
the device's kernels would be called (as ``test_samplers_cpu.py`` injects a
numpy gather).  What the kernels compute is tested in
``test_bias_calc_gpu.py``."""
import numpy as np
import pandas as pd
import pytest

from tests import bias_calc_ref as R

KINDS = R.LINEAR + ('QuantileDeltaMappingCorrection', 'PresRat')
QDM_KW = dict(n_quantiles=11, n_time_steps=6, window_size=90)


def _kwargs(kind, inp, **extra):
    kw = dict(inp)
    if kind in R.LINEAR:
        kw.pop('bias_fut_data')
        kw.pop('bias_fut_time_index')
    else:
        kw.update(QDM_KW)
    kw.update(extra)
    return kw


def _make(kind, inp, **extra):
    import sup3r_amd
    return getattr(sup3r_amd, kind)(backend=R.Backend(),
                                    **_kwargs(kind, inp, **extra))


@pytest.fixture(scope='module')
def inputs():
    return {layout: R.seeded_inputs(layout, years=('2020',))
            for layout in ('sites', 'raster')}


# ------------------------------------------------------------ window lists
@pytest.mark.parametrize('d0, size, want', [
    (60, 3, [59, 60, 61]), (60, 4, [59, 60, 61]), (1, 3, [1, 2, 365]),
    (365, 3, [1, 364, 365])])
def test_member_lists_are_the_reference_window_masks(d0, size, want):
    """the four cases of the reference's test_window_mask*"""
    from sup3r_amd import bias_calc as B
    d = np.arange(1, 366)
    assert np.allclose(want, d[B.window_mask(d, d0, size)])
    ptr, member = B.window_members(d, [d0], size)
    assert ptr.dtype == member.dtype == np.int32
    assert list(ptr) == [0, len(want)]
    assert list(d[member]) == want


@pytest.mark.parametrize('n_t, size', [(24, 120), (12, None), (4, 200),
                                       (1, 365), (3, 30)])
def test_member_lists_of_wrapping_and_overlapping_windows(n_t, size):
    """windows that wrap the year and overlap, unsorted days over leap years;
    with the default size day 365 and 366 are in no window"""
    from sup3r_amd import bias_calc as B
    rng = np.random.default_rng(n_t)
    ti = pd.date_range('2019-01-01', '2021-12-31', freq='D')
    doy = ti.day_of_year.values[rng.permutation(len(ti))]
    centers = B.window_center(n_t)
    assert np.array_equal(centers, R.window_center(n_t))
    w = size or 365 / n_t
    ptr, member = B.window_members(doy, centers, w)
    assert len(ptr) == n_t + 1 and ptr[0] == 0 and ptr[-1] == len(member)
    covered = np.zeros(len(doy), bool)
    for k, d0 in enumerate(centers):
        want = np.where(R.window_mask(doy, d0, w))[0]
        assert np.array_equal(member[ptr[k]:ptr[k + 1]], want)
        covered[want] = True
    last = B.last_window(len(doy), ptr, member)
    assert np.array_equal(last >= 0, covered)
    for t in np.where(covered)[0][:50]:
        held = [k for k, d0 in enumerate(centers)
                if R.window_mask(doy[t:t + 1], d0, w)[0]]
        assert last[t] == held[-1]
    if size is None:
        assert not covered[doy >= 365].any() and covered[doy < 365].all()


def test_a_different_number_of_centres_is_refused(inputs):
    """365 / 367 * 367 steps pass 366: the reference indexes past its
    template there"""
    from sup3r_amd import bias_calc as B
    n = next(n for n in range(2, 2000) if len(B.window_center(n)) != n)
    with pytest.raises(ValueError, match='window centres'):
        _make('QuantileDeltaMappingCorrection', inputs['sites'],
              n_time_steps=n)


# ----------------------------------------------------------------- mapping
def test_kdtree_mapping_and_default_bound(inputs):
    from sup3r_amd import bias_calc as B
    for layout, inp in inputs.items():
        bound = R.distance_upper_bound(inp['bias_lat_lon'])
        assert bound == 1.0
        _, nn = R.nn_query(inp['bias_lat_lon'], inp['base_lat_lon'])
        ptr, idx, nn_ind, b = B.site_mapping(inp['bias_lat_lon'],
                                             inp['base_lat_lon'])
        assert b == bound and np.array_equal(nn_ind, nn)
        assert ptr.dtype == idx.dtype == np.int32 and len(ptr) == 13
        for gid in range(12):
            assert np.array_equal(idx[ptr[gid]:ptr[gid + 1]],
                                  np.where(nn == gid)[0])
        # the last column of the grid has no site
        assert [g for g in range(12) if ptr[g] == ptr[g + 1]] == [3, 7, 11]
    # a tight bound drops sites: they map to no pixel (index P)
    inp = inputs['sites']
    ptr, idx, nn_ind, _ = B.site_mapping(inp['bias_lat_lon'],
                                         inp['base_lat_lon'], 0.2)
    _, nn = R.nn_query(inp['bias_lat_lon'], inp['base_lat_lon'], 0.2)
    assert np.array_equal(nn_ind, nn) and (nn == 12).any()
    assert ptr[-1] == (nn < 12).sum() == len(idx)


def test_day_plan_ranks_the_dates_and_refuses_a_split_day():
    from sup3r_amd import bias_calc as B
    a = pd.date_range('2020-02-27', '2020-03-01 23:00', freq='6h')
    b = pd.date_range('2020-03-02', '2020-03-03 23:00', freq='h')
    perm = np.random.default_rng(0).permutation(len(a))
    plans, ti = B.day_plan([(None, a[perm]), (None, b)], reduce=True)
    assert list(ti) == list(pd.date_range('2020-02-27', '2020-03-03'))
    (ptr, idx, off), (ptr_b, _, off_b) = plans
    assert off == 0 and off_b == 4 and list(np.diff(ptr_b)) == [24, 24]
    for d in range(4):
        days = a[perm][idx[ptr[d]:ptr[d + 1]]].normalize()
        assert len(days) == 4 and (days == ti[d]).all()
    plans, ti = B.day_plan([(None, a), (None, b)], reduce=False)
    assert len(ti) == len(a) + len(b) and plans[1][2] == len(a)
    c = pd.date_range('2020-03-01 12:00', '2020-03-02 23:00', freq='h')
    with pytest.raises(ValueError, match='spans two entries'):
        B.day_plan([(None, a), (None, c)], reduce=True)


# ------------------------------------------------------------ whole classes
@pytest.mark.parametrize('layout', ['sites', 'raster'])
@pytest.mark.parametrize('kind', KINDS)
def test_keys_shapes_and_dtypes_of_out(inputs, kind, layout):
    """``_init_out`` of the three reference files; the values are those of the
    per-pixel loop when the backend computes like it"""
    calc = _make(kind, inputs[layout])
    out = calc.run(max_workers=3)
    want = R.run(kind, _kwargs(kind, inputs[layout]), np.float32)
    assert list(out) == list(want)
    for k, v in out.items():
        assert v.dtype == np.float32 and v.shape == want[k].shape, k
        assert np.array_equal(np.isnan(v), np.isnan(want[k])), k
        ok = ~np.isnan(v)
        assert np.allclose(v[ok], want[k][ok], rtol=2e-5, atol=1e-6), k
    nt = {'LinearCorrection': 1, 'ScalarCorrection': 1}.get(kind, 12)
    if kind in R.LINEAR:
        assert out['pr_scalar'].shape == (3, 4, nt)
        assert calc.bad_bias_gids == [3, 7, 11]
    else:
        assert out['base_pr_obs_params'].shape == (3, 4, 6, 11)
    if kind == 'PresRat':
        assert out['pr_tau_fut'].shape == (3, 4, 1)
        assert out['pr_obs_zero_rate'].shape == (3, 4, 1)
        assert out['pr_k_factor'].shape == (3, 4, 6)
    if 'Scalar' in kind:
        assert np.isnan(out['bias_pr_std']).all()
        assert (out['pr_adder'] == 0).all()


def test_bad_pixels_stay_nan_without_the_fill(inputs):
    out = _make('MonthlyLinearCorrection', inputs['sites']).run(
        fill_extend=False)
    for k, v in out.items():
        assert np.isnan(v[:, 3]).all() and not np.isnan(v[:, :3]).any(), k


@pytest.mark.parametrize('where', ['corner', 'interior'])
@pytest.mark.parametrize('kw', [
    dict(), dict(fill_extend=False, smooth_extend=1.5),
    dict(smooth_extend=2), dict(smooth_interior=1),
    dict(smooth_extend=1, smooth_interior=0.5)])
def test_fill_and_smooth_is_the_restatement(where, kw):
    from sup3r_amd import bias_calc as B
    rng = np.random.default_rng(5)
    out = {'a': rng.normal(size=(6, 7, 3)).astype(np.float32),
           'b': rng.normal(size=(6, 7, 2, 4)).astype(np.float32)}
    for v in out.values():
        if where == 'corner':
            v[:2, :3] = np.nan
        else:
            v[2:4, 3] = np.nan
            v[4, 5] = np.nan
    want = R.fill_and_smooth({k: v.copy() for k, v in out.items()}, **kw)
    got = B.fill_and_smooth({k: v.copy() for k, v in out.items()}, **kw)
    for k in out:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
        filled = kw.get('fill_extend', True)
        assert np.isnan(got[k]).any() != filled


# ------------------------------------------------------------------ files
def test_npz_feeds_the_five_transforms(inputs, tmp_path, monkeypatch):
    """run(fp_out) -> BiasParams.load -> every feature set-up of bias.py"""
    from sup3r_amd import bias as B
    inp = inputs['sites']
    lat_lon = inp['bias_lat_lon']
    for kind, method, extra in [
            ('LinearCorrection', 'local_linear_bc', {}),
            ('MonthlyScalarCorrection', 'monthly_local_linear_bc',
             dict(temporal_avg=False)),
            ('QuantileDeltaMappingCorrection', 'local_qdm_bc',
             dict(base_dset='pr_obs')),
            ('PresRat', 'local_presrat_bc', dict(base_dset='pr_obs'))]:
        fp = str(tmp_path / f'{kind}.npz')
        calc = _make(kind, inp)
        out = calc.run(fp_out=fp) if kind != 'PresRat' else calc.run(
            fp_out=fp, zero_rate_threshold=0.05)
        params = B.BiasParams.load(fp)
        for k, v in out.items():
            assert np.array_equal(params.datasets[k.lower()], v,
                                  equal_nan=True)
        assert np.array_equal(params.datasets['latitude'], lat_lon[..., 0])
        assert np.array_equal(params.datasets['longitude'], lat_lon[..., 1])
        if kind in R.LINEAR:
            assert params.attrs == {}
        else:
            assert params.attrs['dist'] == 'empirical'
            assert params.attrs['sampling'] == 'linear'
            assert params.attrs['log_base'] == 10
            assert np.array_equal(params.attrs['time_window_center'],
                                  R.window_center(6))
            assert ('zero_rate_threshold' in params.attrs) == (
                kind == 'PresRat')
        if kind == 'PresRat':
            assert params.attrs['zero_rate_threshold'] == 0.05
        # the transform's own planning accepts the file
        plan = B.BiasPlan(method, {'pr': dict(
            feature_name='pr', bias_fp=fp, **extra)}, ['pr'],
            lat_lon=lat_lon)
        f = plan.features[0]
        assert f is not None and tuple(plan.grid) == (3, 4)
        assert plan.needs_time == (method != 'local_linear_bc')
    with pytest.raises(ValueError, match='.npz'):
        _make('LinearCorrection', inp).run(fp_out=str(tmp_path / 'x.h5'))


# ----------------------------------------------------------------- errors
def test_value_and_key_errors(inputs):
    inp = inputs['sites']
    with pytest.raises(KeyError, match='empirical'):
        _make('QuantileDeltaMappingCorrection', inp, dist='norm')
    for sampling in ('log', 'invlog', 'cubic'):
        with pytest.raises(KeyError, match='sampling'):
            _make('PresRat', inp, sampling=sampling)
    with pytest.raises(ValueError, match='daily_reduction'):
        _make('LinearCorrection', inp).run(daily_reduction='median')
    with pytest.raises(ValueError, match='clearsky_ratio'):
        _make('LinearCorrection', inp, base_dset='clearsky_ratio').run()
    # a day in two entries of base_data
    (a, ta), (b, tb) = inp['base_data'][0], inp['base_data'][0]
    two = [(a[:100], ta[:100]), (b[100:200], tb[100:200])]
    with pytest.raises(ValueError, match='spans two entries'):
        _make('LinearCorrection', inp, base_data=two).run()
    # non-finite bias values with match_zero_rate
    bad = inp['bias_data'].copy()
    bad[1, 1, 7] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        _make('LinearCorrection', inp, bias_data=bad,
              match_zero_rate=True).run()
    # PresRat keeps the reference's assertion
    with pytest.raises(AssertionError, match='Unexpected invalid values'):
        _make('PresRat', inp, bias_data=bad).run()
    # shapes that do not belong together
    with pytest.raises(ValueError, match='bias_lat_lon'):
        _make('LinearCorrection', inp,
              bias_lat_lon=inp['bias_lat_lon'][:2])
    with pytest.raises(ValueError, match='base_lat_lon'):
        _make('LinearCorrection', inp,
              base_lat_lon=inp['base_lat_lon'][:5])
    # longer than the sort's LDS
    from sup3r_amd import _lib
    n = _lib.BCC_MAX_SORT + 1
    long_ti = pd.date_range('1900-01-01', periods=n, freq='D')
    with pytest.raises(ValueError, match='BCC_MAX_SORT'):
        _make('LinearCorrection', inp, match_zero_rate=True,
              bias_data=np.zeros((3, 4, n), np.float32),
              bias_time_index=long_ti).run()


def test_names_are_exported_and_the_header_declares_the_kernels():
    import os
    import re
    import sup3r_amd
    from sup3r_amd import _lib, bias_calc
    for name in KINDS:
        assert name in sup3r_amd.__all__ and name in bias_calc.__all__
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include',
                               'sup3r_hip.h')).read()
    for fn in ('s3_bc_base_series', 's3_bc_moments',
               's3_bc_window_quantiles', 's3_bc_match_zero_rate',
               's3_bc_presrat'):
        assert re.search(r'\bint\s+' + fn + r'\s*\(', header)
        assert fn in _lib.EXPORTS
    assert f'#define S3_BCC_MAX_SORT {_lib.BCC_MAX_SORT}' in header
