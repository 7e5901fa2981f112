"""GPU tests (``-m gpu``) of feature derivation on the device: the five
kernels of ``csrc/kernels_derive.hip`` through
``sup3r_amd.derive.DeviceBackend`` (thin ctypes wrappers) against
``tests/derive_ref.py`` (the reference restated with ``numpy.ma``, unverified
against dask), and ``DeviceDeriver`` against the same deriver on
``NumpyBackend`` and into ``DeviceSampler`` / ``ForwardPass``.

Exact means: the same float32 bits wherever the reference gives a number, NaN
wherever it gives NaN (the sign and payload of a NaN are nobody's promise).

Bounds of what is not exact, counted, none fitted to the device's output.
``u = 2**-24`` is the unit roundoff of float32; HIP's math API documents
``logf``, ``expf``, ``sinf``, ``cosf``, ``atan2f`` and ``hypotf`` within 1 ulp,
a relative error of at most ``2 u``.  Every yardstick is the float64
evaluation of the reference's expression on the test's float32 inputs; second
order terms are covered by a factor 1.01 on each bound.

  log interpolation, ``out = coeff log(|level - h0| + 1) + v0`` with ``coeff =
  (v1 - v0) / log(h1 - h0 + 1)``, the inputs keep ``h1 - h0`` at 0 (then
  ``coeff = 0`` and ``out = v0`` exactly) or >= 1:
    * ``A = h1 - h0 + 1`` carries two roundings, ``|dA| <= 2 u A``, so ``log A``
      is off by ``2 u`` absolutely before ``logf`` adds ``2 u log A``: relative
      ``2 u / log A + 2 u`` — the first log's error amplified by ``1 / log(h1 -
      h0 + 1)``;
    * ``v1 - v0`` and the division: ``u`` each, so ``coeff`` is off by ``r_c =
      4 u + 2 u / log A`` relatively;
    * ``B = |level - h0| + 1`` likewise, ``log B`` off by ``2 u + 2 u log B``
      absolutely;
    * the product and the sum round once each, relative to ``|coeff log B|``
      and to ``|coeff log B| + |v0|``;
    bound = ``|coeff log B| (r_c + 2 u + 2 u) + |coeff| 2 u + u |v0|``.

  u / v from speed and direction, relative to ``W = |ws| (|cos t| + |sin t|)``
  with the float32 tables as given: the radians ``wd k`` carry the rounding
  of ``k`` and of the product, ``|d| <= 2 u |wd k|``, which moves ``sin`` and
  ``cos`` by as much; ``sinf`` / ``cosf`` add ``2 u``; two products and one
  sum round at ``u`` each: bound = ``W u (5 + 2 |wd k|)``.

  speed / direction from u / v: each rotated component is two products and a
  sum, ``ur = cos t u - sin t v`` off by at most ``e_u = 3 u (|cos t u| + |sin
  t v|)`` and ``vr = sin t u + cos t v`` by ``e_v = 3 u (|sin t u| + |cos t
  v|)``; ``hypot`` is 1-Lipschitz in each argument and ``hypotf`` adds ``2 u
  ws``: bound_ws = ``e_u + e_v + 2 u ws``.  ``atan2`` moves by at most ``(e_u +
  e_v) / ws`` radians, ``atan2f`` adds ``2 u |angle|``, the degrees' constant
  and product ``2 u |deg|``, the sum with 360 ``u (|deg| + 360)``, ``fmod`` is
  exact: bound_wd = ``((e_u + e_v) / ws) 180 / pi + 4 u |deg| + u (|deg| +
  360)``, compared on the circle.

  relative humidity, relative to the result: ``z = 17.1 x / (235 + x)``
  carries the constant's rounding, a product, a sum and a quotient, ``|dz| <=
  4 u |z|``, which ``exp`` turns into a relative ``4 u |z|``; ``expf`` adds ``2
  u``, the constant 6.1078 and its product ``2 u``; the factor 100 and the
  quotient ``u`` each: bound = ``u (4 |z_d| + 4 |z_t| + 10)``.

Each case prints its figures (``profiles/derive/NOTES.md`` records them)."""
import functools
import os

import numpy as np
import pandas as pd
import pytest

from sup3r_amd import derive as D
from tests import derive_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CAP = 64                      # S3_LI_MAX_LEVELS
SENTINEL = np.float32(-7.0e33)
CFG = os.path.join(os.path.dirname(__file__), '..', 'sup3r_amd', 'configs')


@functools.lru_cache(None)
def _be():
    return D.DeviceBackend()


@functools.lru_cache(None)
def _num_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _np(x):
    return x.detach().cpu().numpy()


def _exact(dev, ref, what=''):
    dev, ref = np.asarray(dev), np.asarray(ref)
    assert dev.dtype == np.float32 and dev.shape == ref.shape, what
    ref = ref.astype(np.float32)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(dev), nan), what
    assert np.array_equal(dev[~nan].view(np.int32),
                          ref[~nan].view(np.int32)), what


def _within(name, dev, r64, bound):
    """|dev - r64| <= 1.01 bound wherever r64 is finite, the same class of
    value elsewhere; prints the worst error / bound"""
    dev, r64 = np.asarray(dev, np.float64), np.asarray(r64, np.float64)
    ok = np.isfinite(r64)
    assert np.array_equal(np.isnan(dev), np.isnan(r64)), name
    assert np.array_equal(dev[~ok], r64[~ok], equal_nan=True), name
    err, bound = np.abs(dev - r64)[ok], 1.01 * np.asarray(bound)[ok]
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print(f'[derive bound] {name}: max err {float(err.max()):.3e}, '
          f'worst err / bound {ratio:.3f}')
    assert (err <= bound).all(), (name, ratio)
    return ratio


# ------------------------------------------------------------ s3_level_interp
def _columns(shape, L_ml, n_sl, n_var, source, seed, topo=None, special=True):
    """a level-interpolation case: the backend's arguments (host arrays) and
    the reference's ``(P, L)`` level / variable arrays"""
    rng = np.random.default_rng(seed)
    s1, s2, t = shape
    P = s1 * s2 * t
    case = {'shape': shape, 'lev': None, 'var_ml': [], 'var_sl': [],
            'sl_levels': []}
    cols = []
    if L_ml:
        if source == 'vector':
            vec = (rng.integers(0, 40, L_ml) * 10).astype(np.float32)
            case['lev'] = ('vector', vec)
            cols.append(np.broadcast_to(vec, (P, L_ml)))
        else:
            # multiples of 10: duplicates and exact hits are common
            zg = (rng.integers(0, 40, (*shape, L_ml)) * 10).astype(np.float32)
            if special:
                zg[rng.random(zg.shape) < 0.08] = np.nan
                flat = zg.reshape(P, L_ml)
                flat[rng.random(P) < 0.1, 0] = np.nan        # NaN at index 0
                flat[rng.random(P) < 0.05] = np.nan          # all-NaN columns
                flat[::7, -1] = flat[::7, 0] + np.float32(5e-4)   # |diff| < 1e-3
            tp = None
            if topo == '2d':
                tp = rng.integers(0, 4, (s1, s2)).astype(np.float32) * 10
                full = np.broadcast_to(tp[..., None], shape)
            elif topo == '3d':
                tp = rng.integers(0, 4, shape).astype(np.float32) * 10
                full = tp
            case['lev'] = ('column', zg, tp)
            cols.append(zg.reshape(P, L_ml) if tp is None else
                        zg.reshape(P, L_ml) - full.reshape(P, 1))
    if n_sl:
        sl = (rng.choice(np.arange(1, 40), n_sl, replace=False) * 10
              + 5).astype(np.float32)
        case['sl_levels'] = list(sl)
        cols.append(np.broadcast_to(sl, (P, n_sl)))
    case['levs'] = np.concatenate(cols, axis=-1).astype(np.float32)
    case['vars'] = []
    for _ in range(n_var):
        parts = []
        if L_ml:
            ml = rng.normal(0, 8, (*shape, L_ml)).astype(np.float32)
            if special:
                ml[rng.random(ml.shape) < 0.02] = np.nan
            case['var_ml'].append(ml)
            parts.append(ml.reshape(P, L_ml))
        planes = [rng.normal(0, 8, shape).astype(np.float32)
                  for _ in range(n_sl)]
        case['var_sl'].append(planes)
        parts += [p.reshape(P, 1) for p in planes]
        case['vars'].append(np.concatenate(parts, axis=-1))
    if not n_sl:
        case['var_sl'] = []
    return case


def _offset_by_one_float(a):
    """the array on the device, 4 bytes past a 16-byte boundary"""
    a = np.ascontiguousarray(a, np.float32)
    buf = _be().asarray(np.concatenate([[0], a.reshape(-1)]))
    t = buf[1:].view(a.shape)
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _run(case, targets, method='linear', out=None, misalign=False):
    be = _be()
    up = _offset_by_one_float if misalign else be.asarray
    lev = case['lev']
    if lev is not None and lev[0] == 'column':
        lev = ('column', up(lev[1]),
               None if lev[2] is None else be.asarray(lev[2]))
    return be.level_interp(
        lev, [up(a) for a in case['var_ml']],
        [[be.asarray(p) for p in planes] for planes in case['var_sl']],
        case['sl_levels'], targets, method, out=out)


def _check_linear(case, targets, what):
    got = _run(case, targets)
    assert len(got) == len(case['vars'])
    for v, var in enumerate(case['vars']):
        assert len(got[v]) == len(targets)
        for k, tg in enumerate(targets):
            ref = R.interp_to_level(case['levs'], var, np.float32(tg))
            _exact(_np(got[v][k]).reshape(-1), ref, (what, v, tg))


TARGETS3 = [-15.0, 200.0, 1000.0]     # below all, equal to / between, above all


@pytest.mark.parametrize('n_sl', [0, 1, 2])
@pytest.mark.parametrize('L_ml', [1, 2, 3, 37, 'cap'])
def test_level_interp_linear_level_counts(L_ml, n_sl):
    L_ml = CAP - n_sl if L_ml == 'cap' else L_ml
    case = _columns((13, 1, 5), L_ml, n_sl, 1, 'column', 100 * L_ml + n_sl,
                    topo='2d')
    _check_linear(case, TARGETS3, f'L_ml={L_ml} n_sl={n_sl}')


@pytest.mark.parametrize('shape', [(1, 1, 1), (7, 3, 3), (4, 4, 4),
                                   (13, 5, 1), 'above the grid cap'])
def test_level_interp_linear_column_counts(shape):
    if isinstance(shape, str):
        # grid_for caps the launch at 8 workgroups of 256 columns per CU
        shape = (_num_cu() * 8 + 1, 16, 16)
        assert shape[0] * 256 > _num_cu() * 8 * 256
    case = _columns(shape, 3, 1, 1, 'column', 7, topo='2d')
    _check_linear(case, [35.0], f'shape={shape}')


@pytest.mark.parametrize('source,topo', [('column', None), ('column', '2d'),
                                         ('column', '3d'), ('vector', None)])
def test_level_interp_linear_level_sources(source, topo):
    case = _columns((5, 4, 6), 6, 2, 2, source, 11, topo=topo)
    _check_linear(case, [10.0, 215.0], f'{source} {topo}')


@pytest.mark.parametrize('n_var,n_out', [(1, 1), (3, 3), (8, 16), (1, 16),
                                         (8, 1)])
def test_level_interp_linear_variables_and_targets(n_var, n_out):
    case = _columns((9, 2, 4), 5, 1, n_var, 'column', 13 + n_var, topo='3d')
    targets = list(np.linspace(-20, 420, n_out).astype(np.float32))
    _check_linear(case, targets, f'n_var={n_var} n_out={n_out}')


@pytest.mark.parametrize('L_ml', [3, 37])
def test_level_interp_linear_misaligned_arrays(L_ml):
    """multi-level arrays that do not start on a 16-byte boundary: the runs
    are staged float by float instead of 16 bytes per lane"""
    case = _columns((13, 5, 3), L_ml, 1, 2, 'column', 71 + L_ml, topo='2d')
    got = _run(case, TARGETS3, misalign=True)
    for v, var in enumerate(case['vars']):
        for k, tg in enumerate(TARGETS3):
            _exact(_np(got[v][k]).reshape(-1),
                   R.interp_to_level(case['levs'], var, np.float32(tg)),
                   (L_ml, v, tg))


@pytest.mark.parametrize('topo', ['2d', '3d'])
def test_level_stats(topo):
    """the figures behind ``run_level_check``: the device's counts and
    extrema are the numpy backend's"""
    case = _columns((9, 7, 11), 5, 0, 1, 'column', 73, topo=topo)
    zg, tp = case['lev'][1], case['lev'][2]
    zg[..., 0][zg[..., 0] == 0] = -30           # a negative first level too
    be = _be()
    for lo, hi in ((-50.0, 1000.0), (35.0, 200.0), (1000.0, -50.0)):
        got = be.level_stats(be.asarray(zg), be.asarray(tp), lo, hi)
        want = D.NumpyBackend().level_stats(zg, tp, lo, hi)
        assert want['nan'] > 0 and want['all_nan'] > 0
        assert got == want, (lo, hi)
    # no topography: the figures of the array itself
    got = be.level_stats(be.asarray(zg), None, 35.0, 200.0)
    assert got == D.NumpyBackend().level_stats(zg, None, 35.0, 200.0)
    allnan = np.full((2, 3, 4, 5), np.nan, np.float32)
    got = be.level_stats(be.asarray(allnan), be.asarray(
        np.zeros((2, 3), np.float32)), 0.0, 1.0)
    assert got['all_nan'] == got['columns'] == 24 and got['nan'] == 120
    assert got['bad_min'] == got['bad_max'] == 0
    assert np.isnan(got['first']).all() and np.isnan(got['last']).all()


def test_level_check_warns_from_the_device_statistics():
    arrays, ll, ti = R.era5_like(83, (6, 5, 4), 4)
    arrays['zg'][0, 0, 0, 1] = np.nan
    for height, text in ((1, 'were greater than the minimum requested'),
                         (5000, 'were lower than the maximum requested')):
        with pytest.warns(UserWarning) as rec:
            D.DeviceDeriver(D.DeriveData(dict(arrays), ll, ti),
                            [f'v_{height}m'],
                            interp_kwargs={'run_level_check': True})
        msgs = [str(w.message) for w in rec]
        assert any(text in m for m in msgs), msgs
        # one NaN among 6 * 5 * 4 * 4 levels
        assert any('Approximately 0.21% of the vertical level' in m
                   for m in msgs), msgs


def test_level_interp_linear_single_levels_only():
    case = _columns((6, 5, 4), 0, 2, 2, 'column', 17)
    _check_linear(case, [30.0, 500.0], 'single levels only')


def test_level_interp_linear_chosen_columns():
    """target equal to a level, midway between two pairs of equal levels
    (ties to the lowest index), |diff| < 1e-3, a NaN level in the middle and
    at index 0, an all-NaN column, a NaN variable"""
    nan = np.nan
    levs = np.array([[10, 50, 50, 90], [30, 30, 70, 70], [50, 50.0005, 80, 90],
                     [10, nan, 60, 90], [nan, 20, 60, 90], [nan, nan, nan, nan],
                     [90, 60, 20, 10], [50, 50, 50, 50]], np.float32)
    var = np.arange(32, dtype=np.float32).reshape(8, 4) * 1.25 - 7
    var_nan = var.copy()
    var_nan[0, 1] = nan
    var_nan[3, 2] = nan
    case = {'lev': ('column', levs.reshape(8, 1, 1, 4), None),
            'var_ml': [var.reshape(8, 1, 1, 4), var_nan.reshape(8, 1, 1, 4)],
            'var_sl': [], 'sl_levels': [], 'levs': levs,
            'vars': [var, var_nan]}
    _check_linear(case, [50.0, 50.0002, 5.0, 95.0, 60.0], 'chosen columns')
    got = _np(_run(case, [50.0])[0][0]).reshape(-1)
    assert got[0] == var[0, 1]            # the first of the two levels at 50
    assert np.isnan(got[5])               # all-NaN levels: NaN out


def _guarded(n_planes, P, pad=96):
    """one buffer [pad | plane | pad | plane | ... | pad] of sentinels and the
    planes as views of it"""
    import torch
    be = _be()
    total = pad + n_planes * (P + pad)
    buf = be.asarray(np.full(total, SENTINEL, np.float32))
    planes = [buf[pad + i * (P + pad): pad + i * (P + pad) + P]
              for i in range(n_planes)]
    assert all(isinstance(p, torch.Tensor) for p in planes)
    return buf, planes, pad


def test_level_interp_writes_exactly_its_planes():
    shape, n_var, targets = (5, 3, 7), 3, [35.0, 120.0]
    P = int(np.prod(shape))
    case = _columns(shape, 4, 1, n_var, 'column', 19, topo='2d',
                    special=False)
    buf, planes, pad = _guarded(n_var * len(targets), P)
    out = [[planes[v * len(targets) + k].view(shape)
            for k in range(len(targets))] for v in range(n_var)]
    _run(case, targets, out=out)
    host = _np(buf)
    for i in range(len(planes) + 1):
        lo = i * (P + pad)
        assert (host[lo:lo + pad] == SENTINEL).all(), f'guard {i} written'
    for v in range(n_var):
        for k, tg in enumerate(targets):
            got = _np(out[v][k]).reshape(-1)
            assert not (got == SENTINEL).any()
            _exact(got, R.interp_to_level(case['levs'], case['vars'][v],
                                          np.float32(tg)), (v, tg))


@pytest.mark.parametrize('what', ['levels', 'single', 'vars', 'targets'])
def test_level_interp_refuses_past_its_limits(what):
    """the first refused value of each limit: S3_EINVAL (a ValueError), and
    nothing written"""
    L_ml, n_sl, n_var, n_out = 4, 1, 1, 1
    if what == 'levels':
        L_ml = CAP                        # 64 + 1 single level = 65
    elif what == 'single':
        n_sl = 9
    elif what == 'vars':
        n_var = 9
    else:
        n_out = 17
    shape = (3, 2, 2)
    case = _columns(shape, L_ml, n_sl, n_var, 'column', 23, special=False)
    buf, planes, _ = _guarded(n_var * n_out, 12)
    out = [[planes[v * n_out + k].view(shape) for k in range(n_out)]
           for v in range(n_var)]
    with pytest.raises(ValueError, match='level_interp'):
        _run(case, list(np.arange(n_out, dtype=np.float32) * 30), out=out)
    _be().dev.sync()
    assert (_np(buf) == SENTINEL).all()


@pytest.mark.parametrize('n_sl', [0, 2])
def test_level_interp_log(n_sl):
    """against float64 with the counted bound of the module docstring; the
    levels are whole numbers, so ``h1 - h0`` is 0 or >= 1; every element is
    compared"""
    case = _columns((11, 3, 5), 5, n_sl, 2, 'column', 29 + n_sl, topo='2d',
                    special=False)
    targets = [-15.0, 33.0, 200.0, 1000.0]
    got = _run(case, targets, method='log')
    levs = case['levs']
    worst = 0.0
    for v, var in enumerate(case['vars']):
        for k, tg in enumerate(targets):
            r64 = R.interp_to_level(levs, var, np.float32(tg), method='log',
                                    dtype=np.float64)
            i1, i2 = D._select_levels(levs, np.float32(tg))
            pick = lambda a, i: np.take_along_axis(        # noqa: E731
                a, i[:, None], -1)[:, 0].astype(np.float64)
            l1, l2, v1, v2 = pick(levs, i1), pick(levs, i2), pick(var, i1), \
                pick(var, i2)
            m = l1 < l2
            h0, h1 = np.where(m, l1, l2), np.where(m, l2, l1)
            w0, w1 = np.where(m, v1, v2), np.where(m, v2, v1)
            gap = h1 - h0
            assert ((gap == 0) | (gap >= 1)).all()
            log_a = np.log(np.maximum(gap, 1) + 1)
            coeff = np.where(gap == 0, 0.0, (w1 - w0) / log_a)
            log_b = np.log(np.abs(tg - h0) + 1)
            r_c = 4 * U + 2 * U / log_a
            bound = (np.abs(coeff * log_b) * (r_c + 4 * U)
                     + np.abs(coeff) * 2 * U + U * np.abs(w0))
            assert np.allclose(coeff * log_b * np.where(tg < h0, -1, 1) + w0,
                               r64, rtol=1e-12, atol=0)
            worst = max(worst, _within(f'log n_sl={n_sl} var {v} target {tg}',
                                       _np(got[v][k]).reshape(-1), r64, bound))
    print(f'[derive bound] log n_sl={n_sl}: worst err / bound {worst:.3f}')


# -------------------------------------------------------- s3_derive_pointwise
def _sizes():
    return [(1, 1, 1), (5, 3, 17), (257, 1, 1), (_num_cu() * 16 + 1, 16, 16)]


def _specials(rng, shape, lo=-50, hi=50):
    x = rng.uniform(lo, hi, shape).astype(np.float32)
    flat = x.reshape(-1)
    vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    if flat.size >= 64:
        idx = rng.choice(flat.size, 25, replace=False)
        flat[idx] = np.tile(vals, 5)
    return x


@pytest.mark.parametrize('i_size', range(4))
def test_pointwise_exact_ops(i_size):
    shape = _sizes()[i_size]
    s1, s2, t = shape
    rng = np.random.default_rng(31 + i_size)
    be = _be()
    a, b = _specials(rng, shape), _specials(rng, shape)
    cs = rng.integers(0, 3, shape).astype(np.float32)     # clearsky in {0, 1, 2}
    cs2 = np.where(rng.random(shape) < 0.5, cs, cs + 2).astype(np.float32)
    da, db, dcs, dcs2 = (be.asarray(x) for x in (a, b, cs, cs2))
    with np.errstate(all='ignore'):
        _exact(_np(be.add(da, db)), a + b, 'add')
        f = (80.0 / 10) ** 0.2
        _exact(_np(be.scale(da, f)), R.power_law(a, 80), 'scale')
        _exact(_np(be.offset(da, -273.15)), R.to_celsius(a), 'offset')
        got = _np(be.ratio_clip01(da, dcs2))
        _exact(got, R.clearsky_ratio_cc(a, cs2), 'ratio_clip01')
        # a ratio that is not positive comes out as +0, never as -0
        assert not np.signbit(got[got == 0]).any()
    # flags: computed by s3_time_flags on clearsky_ghi <= 1, and chosen ones
    night = be.time_flags(dcs, 'le', 1.0)
    assert np.array_equal(_np(night), (cs <= 1).any(axis=(0, 1)))
    for flags in ((cs <= 1).any(axis=(0, 1)),
                  np.arange(t) % (t - 1 if t > 1 else 1) == 0):   # first, last
        import torch
        dflags = torch.from_numpy(flags.astype(np.int32)).to(da.device)
        with np.errstate(all='ignore'):
            want = (a / cs2).astype(np.float32)
            want[..., flags] = np.nan
            _exact(_np(be.ratio_masked(da, dcs2, dflags)), want, 'ratio')
            want = (a < cs2).astype(np.float32)
            want[..., flags] = np.nan
            _exact(_np(be.cloud_mask(da, dcs2, dflags)), want, 'cloud_mask')
    plane = _specials(rng, (s1, s2))
    _exact(_np(be.broadcast_pixel(plane, t)),
           np.repeat(plane[..., None], t, axis=-1), 'broadcast_pixel')
    ti = pd.date_range('2021-12-31 21:17:05', periods=t, freq='2003s')
    vec = R.time_encoding(ti, 'soy')
    _exact(_np(be.broadcast_time(vec, s1, s2)),
           np.broadcast_to(vec, shape), 'broadcast_time')


def _tables(ll):
    from sup3r_amd.output_transform import grid_theta
    theta = grid_theta(ll)
    return (np.cos(theta).astype(np.float32).astype(np.float64)[..., None],
            np.sin(theta).astype(np.float32).astype(np.float64)[..., None])


def _uv_bound(ws, wd, ct, st):
    w = np.abs(ws) * (np.abs(ct) + np.abs(st))
    return w * U * (5 + 2 * np.abs(np.radians(wd)))


def _uv64(ws, wd, ct, st):
    ws, wd = ws.astype(np.float64), np.radians(wd.astype(np.float64))
    return (ct * ws * np.sin(wd) + st * ws * np.cos(wd),
            -st * ws * np.sin(wd) + ct * ws * np.cos(wd))


def _wswd_check(name, ws_d, wd_d, u, v, ct, st):
    """``wd_d`` None: the speed alone"""
    u, v = u.astype(np.float64), v.astype(np.float64)
    ur, vr = ct * u - st * v, st * u + ct * v
    ws = np.hypot(ur, vr)
    deg = np.degrees(np.arctan2(ur, vr))
    e = 3 * U * (np.abs(ct * u) + np.abs(st * v)
                 + np.abs(st * u) + np.abs(ct * v))       # e_u + e_v
    r1 = _within(f'{name} windspeed', ws_d, ws, e + 2 * U * ws)
    if wd_d is None:
        return r1
    bound = (e / ws) * 180 / np.pi + 4 * U * np.abs(deg) \
        + U * (np.abs(deg) + 360)
    diff = np.abs(np.asarray(wd_d, np.float64) - (deg + 360) % 360)
    diff = np.minimum(diff, 360 - diff)                  # on the circle
    assert (np.asarray(wd_d) >= 0).all() and (np.asarray(wd_d) <= 360).all()
    r2 = float((diff / (1.01 * bound)).max())
    print(f'[derive bound] {name} winddirection: max err {diff.max():.3e}, '
          f'worst err / bound {r2:.3f}')
    assert r2 <= 1, name
    return max(r1, r2)


@pytest.mark.parametrize('grid', ['descending', 'ascending', 'one row',
                                  'above the cap'])
def test_pointwise_wind_transforms(grid):
    rng = np.random.default_rng(37)
    shape = {'one row': (1, 9, 5), 'above the cap':
             (_num_cu() * 16 + 1, 16, 16)}.get(grid, (6, 7, 9))
    ll = R.grid(shape[0], shape[1], flip=grid == 'ascending')
    if grid == 'one row':
        assert len(ll) == 1
    ws = rng.uniform(0, 30, shape).astype(np.float32)
    wd = rng.uniform(0, 360, shape).astype(np.float32)
    wd.reshape(-1)[:5] = [0, 90, 180, 270, 360]
    be = _be()
    u_d, v_d = be.uv_from_wswd(be.asarray(ws), be.asarray(wd), ll)
    ct, st = _tables(ll)
    u64, v64 = _uv64(ws, wd, ct, st)
    bound = _uv_bound(ws, wd, ct, st)
    _within(f'{grid} u', _np(u_d), u64, bound)
    _within(f'{grid} v', _np(v_d), v64, bound)
    # the rotation is the reference's, row flip included
    u_r, v_r = R.transform_rotate_wind(ws, wd, ll)
    assert np.allclose(_np(u_d), u_r, atol=1e-3)
    assert np.allclose(_np(v_d), v_r, atol=1e-3)
    u = rng.normal(0, 8, shape).astype(np.float32)
    v = rng.normal(0, 8, shape).astype(np.float32)
    ws_d, wd_d = be.wswd_from_uv(be.asarray(u), be.asarray(v), ll)
    _wswd_check(grid, _np(ws_d), _np(wd_d), u, v, ct, st)
    ws_r, wd_r = R.invert_uv(u, v, ll)
    assert np.allclose(_np(ws_d), ws_r, atol=1e-3)


def _rh_check(name, got, d2m, t2m):
    d, tc = d2m.astype(np.float64), t2m.astype(np.float64)
    r64 = R.surface_rh(d, tc)
    z_d, z_t = 17.1 * d / (235 + d), 17.1 * tc / (235 + tc)
    bound = np.abs(r64) * U * (4 * np.abs(z_d) + 4 * np.abs(z_t) + 10)
    return _within(name, got, r64, bound)


@pytest.mark.parametrize('i_size', range(4))
def test_pointwise_surface_rh(i_size):
    shape = _sizes()[i_size]
    rng = np.random.default_rng(41 + i_size)
    t2m = rng.uniform(-40, 45, shape).astype(np.float32)
    d2m = (t2m - rng.uniform(0, 20, shape)).astype(np.float32)
    be = _be()
    _rh_check(f'surface_rh {shape}',
              _np(be.surface_rh(be.asarray(d2m), be.asarray(t2m))), d2m, t2m)


# --------------------------------------------- s3_time_flags, s3_stack_features
@pytest.mark.parametrize('t', [1, 2, 24])
@pytest.mark.parametrize('c', [1, 3, 32])
def test_stack_and_flags(t, c):
    rng = np.random.default_rng(43 + t + c)
    s1, s2 = 5, 13
    planes = [rng.normal(size=(s1, s2, t)).astype(np.float32)
              for _ in range(c)]
    be = _be()
    dplanes = [be.asarray(p) for p in planes]
    for roll in (0, 1, t - 1, -1, t + 3):
        got = _np(be.stack(dplanes, roll))
        _exact(got, np.roll(np.stack(planes, axis=-1), roll, axis=2),
               f'roll {roll}')
    cube = np.stack(planes, axis=-1)
    assert not _np(be.time_flags(be.asarray(cube), 'nan')).any()
    for pix, step in [((0, 0), 0), ((s1 - 1, s2 - 1), 0), ((0, 0), t - 1),
                      ((s1 - 1, s2 - 1), t - 1)]:
        bad = cube.copy()
        bad[pix[0], pix[1], step, c - 1] = np.nan
        want = np.zeros(t, np.int32)
        want[step] = 1
        assert np.array_equal(_np(be.time_flags(be.asarray(bad), 'nan')), want)
    le = _np(be.time_flags(dplanes[0], 'le', -1.5))
    assert np.array_equal(le, (planes[0] <= np.float32(-1.5)).any(axis=(0, 1)))


def test_stack_refuses_33_planes():
    be = _be()
    planes = [be.asarray(np.zeros((2, 2, 2), np.float32))] * 33
    with pytest.raises(ValueError, match='stack_features'):
        be.stack(planes, 0)


# ------------------------------------------------------------------ class level
def _both(arrays, ll, ti, feats, **kw):
    dd = {k: kw.pop(k) for k in ('attrs',) if k in kw}
    host = D.DeviceDeriver(D.DeriveData(dict(arrays), ll, ti, **dd), feats,
                           backend=D.NumpyBackend(), **kw)
    dev = D.DeviceDeriver(D.DeriveData(dict(arrays), ll, ti, **dd), feats,
                          **kw)
    assert dev.features == host.features
    assert [(g.variables, g.targets, g.companions) for g in dev.launch_plan] \
        == [(g.variables, g.targets, g.companions) for g in host.launch_plan]
    return dev, host


def test_deriver_era5_like():
    arrays, ll, ti = R.era5_like(47, (9, 7, 12), 10)
    feats = ['u_40m', 'v_40m', 'u_100m', 'windspeed_100m', 'sod_encoding']
    dev, host = _both(arrays, ll, ti, feats)
    assert len(dev.launch_plan) == 2          # u with u_10m; v without
    for f in ('u_40m', 'v_40m', 'u_100m', 'sod_encoding'):
        _exact(_np(dev[f]), host[f], f)
    # windspeed_100m from the interpolated pair (the device's u_100m is the
    # host's, bit for bit; v_100m was derived on the way, as an input)
    ct, st = _tables(ll)
    u100 = np.asarray(host['u_100m'])
    v100 = R.interp_to_level(R.height_array(arrays), arrays['v'],
                             np.float32(100))
    _exact(_np(dev.backend.level_interp(
        ('column', dev.backend.asarray(arrays['zg']),
         dev.backend.asarray(arrays['topography'])),
        [dev.backend.asarray(arrays['v'])], [], [], [100.0])[0][0]), v100,
        'v_100m')
    _wswd_check('era5 windspeed_100m', _np(dev['windspeed_100m']), None, u100,
                v100, ct, st)
    cube = _np(dev.as_array())
    assert cube.shape == (9, 7, 12, 5) and cube.dtype == np.float32
    for i, f in enumerate(feats):
        assert np.array_equal(cube[..., i], _np(dev[f]), equal_nan=True)


def test_deriver_gcm_power_law():
    rng = np.random.default_rng(53)
    shape = (8, 6, 10)
    arrays = {'uas': rng.normal(0, 5, shape), 'vas': rng.normal(0, 5, shape),
              'tas': rng.uniform(250, 310, shape),
              'rsds': rng.uniform(-5, 400, shape),
              'clearsky_ghi': rng.uniform(0, 350, shape),
              'hurs': rng.uniform(0, 100, shape)}
    arrays = {k: v.astype(np.float32) for k, v in arrays.items()}
    ti = pd.date_range('2050-01-01', periods=10, freq='D')
    feats = ['u_100m', 'v_100m', 'temperature_2m', 'clearsky_ratio',
             'relativehumidity_2m']
    dev, host = _both(arrays, R.grid(8, 6), ti, feats,
                      FeatureRegistry=D.RegistryNCforCCwithPowerLaw)
    for f in feats:
        _exact(_np(dev[f]), host[f], f)
    assert dev.data.attrs['tas']['units'] == 'C'
    _exact(_np(dev.as_array()), host.as_array(), 'cube')


def test_deriver_nsrdb():
    rng = np.random.default_rng(59)
    shape = (7, 5, 24)
    cs = np.clip(400 * np.sin(np.linspace(-1, 4, 24)), 0, None)
    cs = np.round(np.broadcast_to(cs, shape) * rng.uniform(
        0.9, 1, shape)).astype(np.float32)
    arrays = {'ghi': (cs * rng.uniform(0, 1, shape)).astype(np.float32),
              'clearsky_ghi': cs,
              'wind_speed': rng.uniform(0, 10, shape).astype(np.float32),
              'wind_direction': rng.uniform(0, 360, shape).astype(np.float32),
              'air_temperature': rng.normal(size=shape).astype(np.float32)}
    ll = R.grid(7, 5)
    ti = pd.date_range('2018-01-01', periods=24, freq='h')
    feats = ['clearsky_ratio', 'u', 'v', 'air_temperature']
    dev, host = _both(arrays, ll, ti, feats,
                      FeatureRegistry=D.RegistryH5SolarCC,
                      nan_method_kwargs={'method': 'mask'}, time_roll=2)
    assert dev.time_index.equals(host.time_index)
    assert 0 < len(dev.time_index) < 24
    for f in ('clearsky_ratio', 'air_temperature'):
        _exact(_np(dev[f]), host[f], f)
    plain = D.DeviceDeriver(D.DeriveData(dict(arrays), ll, ti), ['u', 'v'],
                            FeatureRegistry=D.RegistryH5SolarCC)
    ct, st = _tables(ll)
    ws, wd = arrays['wind_speed'], arrays['wind_direction']
    u64, v64 = _uv64(ws, wd, ct, st)
    _within('nsrdb u', _np(plain['u']), u64, _uv_bound(ws, wd, ct, st))
    _within('nsrdb v', _np(plain['v']), v64, _uv_bound(ws, wd, ct, st))


def test_deriver_coarsens_on_the_device():
    """``hr_spatial_coarsen=2`` on an odd grid: trimmed, block-meaned by
    ``s3_coarsen``.  Its sum of four and the numpy backend's may associate
    differently: both within ``4 u mean|x|`` of the float64 mean (three
    additions and the product with 1 / 4, ``u`` each)"""
    rng = np.random.default_rng(79)
    shape = (11, 9, 6)
    arrays = {'uas': rng.normal(0, 6, shape).astype(np.float32),
              'vas': rng.normal(0, 6, shape).astype(np.float32)}
    ll = R.grid(11, 9)
    ti = pd.date_range('2050-01-01', periods=6, freq='D')
    feats = ['u_100m', 'v_100m']
    dev, host = _both(arrays, ll, ti, feats, hr_spatial_coarsen=2,
                      FeatureRegistry=D.RegistryNCforCCwithPowerLaw)
    assert dev.shape == host.shape == (5, 4, 6, 2)
    assert np.array_equal(dev.lat_lon, host.lat_lon)
    assert dev.lat_lon.shape == (5, 4, 2)
    for f, src in zip(feats, ('uas', 'vas')):
        x = R.power_law(arrays[src], 100)[:10, :8].astype(np.float64)
        blocks = x.reshape(5, 2, 4, 2, 6)
        mean = blocks.mean(axis=(1, 3))
        bound = 4 * U * np.abs(blocks).mean(axis=(1, 3))
        _within(f'coarsen {f} device', _np(dev[f]), mean, bound)
        _within(f'coarsen {f} numpy backend', host[f], mean, bound)
    assert np.array_equal(_np(dev.as_array())[..., 1], _np(dev['v_100m']))


def test_cube_feeds_the_sampler():
    from sup3r_amd import DeviceSampler
    arrays, ll, ti = R.era5_like(61, (12, 11, 20), 4)
    feats = ['u_40m', 'v_40m', 'u_100m']
    dev = D.DeviceDeriver(D.DeriveData(arrays, ll, ti), feats)
    cube = dev.as_array()
    from_dev = DeviceSampler(cube, feats, (6, 5, 8), batch_size=4, seed=3)
    from_host = DeviceSampler(_np(cube), feats, (6, 5, 8), batch_size=4,
                              seed=3)
    for _ in range(3):
        a, b = next(from_dev), next(from_host)
        a = a[0] if isinstance(a, (tuple, list)) else a
        b = b[0] if isinstance(b, (tuple, list)) else b
        assert np.array_equal(_np(a) if hasattr(a, 'detach') else a,
                              _np(b) if hasattr(b, 'detach') else b)


def test_cube_feeds_the_forward_pass():
    from sup3r_amd import ForwardPass, Sup3rGan
    from sup3r_amd.forward_pass import register_model
    from sup3r_amd.strategy import ArrayStrategy
    feats = ['u_10m', 'v_10m']
    Sup3rGan.seed(9)
    m = Sup3rGan(os.path.join(CFG, 'test_gen_s_2x_2f.json'),
                 os.path.join(CFG, 'test_disc_s_same.json'),
                 means={f: np.float32(0.3) for f in feats},
                 stdevs={f: np.float32(1.5) for f in feats}, precision='f32')
    m.set_model_params(lr_features=feats, hr_out_features=feats, s_enhance=2,
                       t_enhance=1)
    m.init_weights((1, 16, 16, 2), (1, 32, 32, 2))
    key = {'model_dir': 'derive-fwp'}
    register_model('Sup3rGan', key, m)
    rng = np.random.default_rng(67)
    shape = (24, 20, 4)
    arrays = {'uas': rng.normal(0, 6, shape).astype(np.float32),
              'vas': rng.normal(0, 6, shape).astype(np.float32)}
    ti = pd.date_range('2020-01-01', periods=4, freq='h')
    dev = D.DeviceDeriver(D.DeriveData(dict(arrays), R.grid(24, 20), ti),
                          ['u_100m', 'v_100m'],
                          FeatureRegistry=D.RegistryNCforCCwithPowerLaw)
    domain = _np(dev.as_array())
    # the hand-built domain: numpy alone, nothing of the deriver's
    by_hand = np.stack([R.power_law(arrays['uas'], 100),
                        R.power_law(arrays['vas'], 100)], axis=-1)
    assert by_hand.dtype == np.float32 and not np.array_equal(
        by_hand[..., 0], arrays['uas'])

    def run(dom):
        st = ArrayStrategy(dom, key, (12, 10, 4), model=m, spatial_pad=2,
                           temporal_pad=0)
        done, kept = ForwardPass.run(st, 0, return_data=True)
        assert done == st.n_chunks
        return dict(kept)

    got, want = run(domain), run(by_hand)
    assert sorted(got) == sorted(want) and len(got) == 4
    for k in want:
        assert np.array_equal(got[k], want[k])
