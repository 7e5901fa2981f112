"""GPU tests (``-m gpu``) of ``SolarMultiStepGan``
(sup3r/models/multi_step.py:484-911): the two kernels of its device route
against ``tests/solar_ref.py`` bit for bit, the reference's own test
(tests/forward_pass/test_multi_step.py:234-288), device route == host route,
the fall-back, and the chunk executor."""
import ctypes as C
import json
import os
import tempfile

import numpy as np
import pytest

from . import solar_ref

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), '..', 'sup3r_amd', 'configs')
PF = C.POINTER(C.c_float)
#: tile of branch_join_kernel (csrc/kernels_join.hip: kTileW columns x kTileT
#: time steps of one image row)
TILE_W, TILE_T = 32, 16
CSR, WIND = ['clearsky_ratio'], ['U_200m', 'V_200m']


def _f(a):
    return None if a is None else a.ctypes.data_as(PF)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _imap(m):
    return (C.c_int32 * max(len(m), 1))(*m)


def _join(ya, map_a, aff_a, yb, map_b, aff_b, stats, thw):
    """s3_branch_join -> (return code, x as numpy or None)"""
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    dev, L = Device.get(), _lib.lib()
    t, h, w = thw
    yad = dev.to_device(ya) if ya is not None and ya.size else None
    ybd = dev.to_device(yb) if yb is not None and yb.size else None
    nc = len(map_a) + len(map_b)
    x = dev.empty((1, h, w, t, max(nc, 1)))
    rc = L.s3_branch_join(
        dev.ctx, _p(yad), 0 if ya is None else ya.shape[-1], _imap(map_a),
        len(map_a), _f(aff_a[0]), _f(aff_a[1]), _p(ybd),
        0 if yb is None else yb.shape[-1], _imap(map_b), len(map_b),
        _f(aff_b[0]), _f(aff_b[1]), t, h, w, _f(stats[0]), _f(stats[1]),
        _p(x))
    return rc, (x.cpu().numpy() if rc == 0 else None)


def _join_case(rng, thw, ca, map_a, cb, map_b, un_a=True, un_b=True,
               nrm=True, poke=()):
    t, h, w = thw
    ya = (rng.standard_normal((t, h, w, ca)) * 3).astype(np.float32)
    yb = (rng.standard_normal((t, h, w, cb)) * 3).astype(np.float32)
    for which, pos, val in poke:
        (ya, yb)[which][pos] = val
    aff_a = ((0.5 + rng.random(ca)).astype(np.float32),
             rng.standard_normal(ca).astype(np.float32)) if un_a \
        else (None, None)
    aff_b = ((0.5 + rng.random(cb)).astype(np.float32),
             rng.standard_normal(cb).astype(np.float32)) if un_b \
        else (None, None)
    nc = len(map_a) + len(map_b)
    stats = (rng.standard_normal(nc).astype(np.float32),
             (0.5 + rng.random(nc)).astype(np.float32)) if nrm \
        else (None, None)
    want = solar_ref.branch_join(ya, map_a, *aff_a, yb, map_b, *aff_b, *stats)
    rc, got = _join(ya if ca else None, map_a, aff_a, yb if cb else None,
                    map_b, aff_b, stats, thw)
    assert rc == 0
    assert got.shape == (1, h, w, t, nc) == want.shape
    np.testing.assert_array_equal(got, want)
    return got


#: (ca, map_a, cb, map_b)
CHANNELS = [(1, [0], 2, [0, 1]), (1, [0], 6, [5, 4]),
            (16, list(range(16)), 0, []), (0, [], 3, [0, 1, 2]),
            (8, list(range(8)), 8, list(range(8)))]
#: one element; odd, below the tile; one past the tile in t and in w (two
#: tiles along either, three image rows); one short of it
SHAPES = [(1, 1, 1), (3, 5, 7), (TILE_T + 1, 3, TILE_W + 1),
          (TILE_T - 1, 2, TILE_W - 1)]


@pytest.mark.parametrize('thw', SHAPES)
@pytest.mark.parametrize('ca, map_a, cb, map_b', CHANNELS)
def test_branch_join_kernel_vs_numpy(thw, ca, map_a, cb, map_b):
    rng = np.random.default_rng(sum(thw) + 100 * ca + cb)
    _join_case(rng, thw, ca, map_a, cb, map_b)


@pytest.mark.parametrize('un_a, un_b, nrm', [
    (False, False, True), (True, True, False), (False, False, False),
    (True, False, True)])
def test_branch_join_null_statistics(un_a, un_b, nrm):
    """NULL scale / shift: no un-normalisation of that source; NULL mean /
    std: no normalisation; all NULL: a pure transpose-concat"""
    rng = np.random.default_rng(17)
    for thw in ((3, 5, 7), (TILE_T + 1, 3, TILE_W + 1)):
        _join_case(rng, thw, 1, [0], 6, [5, 4], un_a, un_b, nrm)


def test_branch_join_carries_nan_and_inf_in_place():
    rng = np.random.default_rng(23)
    thw = (TILE_T + 1, 3, TILE_W + 1)
    poke = [(0, (0, 0, 0, 0), np.nan), (0, (16, 2, 32, 0), np.inf),
            (1, (5, 1, 31, 1), -np.inf), (1, (16, 2, 32, 0), np.nan),
            (1, (3, 0, 7, 1), np.nan)]
    got = _join_case(rng, thw, 1, [0], 2, [0, 1], poke=poke)
    assert np.isnan(got[0, 0, 0, 0, 0]) and np.isposinf(got[0, 2, 32, 16, 0])
    assert np.isneginf(got[0, 1, 31, 5, 2]) and np.isnan(got[0, 2, 32, 16, 1])
    assert np.isnan(got[0, 0, 7, 3, 2])
    assert np.isnan(got).sum() == 3 and np.isinf(got).sum() == 2
    # a pure transpose-concat moves the bits themselves
    got = _join_case(rng, thw, 1, [0], 2, [0, 1], False, False, False,
                     poke=poke)
    assert np.isnan(got).sum() == 3 and np.isinf(got).sum() == 2


def test_branch_join_argument_checks():
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    none = (None, None)
    y17 = np.zeros((2, 2, 2, 17), np.float32)
    y2 = np.zeros((2, 2, 2, 2), np.float32)
    rc, _ = _join(y17, [0], none, y2, [0], none, none, (2, 2, 2))
    assert rc != 0 and '16' in _lib.last_error(Device.get().ctx)
    rc, _ = _join(y2, [0], none, y17, [0], none, none, (2, 2, 2))
    assert rc != 0
    y9 = np.zeros((2, 2, 2, 9), np.float32)
    rc, _ = _join(y9, list(range(9)), none, y9, list(range(8)), none, none,
                  (2, 2, 2))
    assert rc != 0                                    # 17 at the destination
    rc, _ = _join(y2, [], none, y2, [], none, none, (2, 2, 2))
    assert rc != 0                                    # na + nb = 0
    rc, _ = _join(y2, [2], none, y2, [0], none, none, (2, 2, 2))
    assert rc != 0 and 'map' in _lib.last_error(Device.get().ctx)


@pytest.mark.parametrize('outer, t, c, pad', [
    (1, 24, 1, 3), (35, 4, 3, 7), (7, 2, 16, 5), (3, 5, 2, 0), (4, 1, 2, 2)])
@pytest.mark.parametrize('affine', [True, False])
def test_time_pad_reflect_kernel_vs_numpy(outer, t, c, pad, affine):
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    dev, L = Device.get(), _lib.lib()
    rng = np.random.default_rng(outer + t + c + pad)
    y = (rng.standard_normal((outer, t, c)) * 3).astype(np.float32)
    scale = (0.5 + rng.random(c)).astype(np.float32) if affine else None
    shift = rng.standard_normal(c).astype(np.float32) if affine else None
    want = solar_ref.time_pad_reflect(y, pad, scale, shift)
    yd = dev.to_device(y)
    out = dev.empty((outer, t + 2 * pad, c))
    rc = L.s3_time_pad_reflect(dev.ctx, _p(yd), outer, t, c, pad, _f(scale),
                               _f(shift), _p(out))
    _lib.check(rc, dev.ctx, 's3_time_pad_reflect')
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    if not affine:
        np.testing.assert_array_equal(
            out.cpu().numpy(),
            np.pad(y, ((0, 0), (pad, pad), (0, 0)), mode='reflect'))
    rc = L.s3_time_pad_reflect(dev.ctx, _p(yd), outer, t, 17, pad, None,
                               None, _p(out))
    assert rc != 0


# -- models -----------------------------------------------------------------
MEANS = {'clearsky_ratio': 0.7, 'U_200m': 4.2, 'V_200m': 5.6, 'U_10m': 1.5,
         'topography': 100.2}
STDS = {'clearsky_ratio': 0.04, 'U_200m': 1.1, 'V_200m': 1.3, 'U_10m': 0.9,
        'topography': 50.3}


def _spec(name, filters=None, topo=False):
    """a shipped generator spec; ``filters``: another number of output
    channels; ``topo``: a Sup3rConcat of hi-res topography behind the
    expansion's activation"""
    spec = json.load(open(os.path.join(CFG, 'sup3r', name)))
    layers = spec['hidden_layers']
    if filters is not None:
        last = [la for la in layers if 'filters' in la][-1]
        last['filters'] = filters
    if topo:
        k = [la.get('class') for la in layers].index('Activation')
        layers.insert(k + 1, {'class': 'Sup3rConcat', 'name': 'topography'})
    return spec


def _gan(gen, disc, lr, out, s, t, lr_shape, seed, exo=()):
    from sup3r_amd import Sup3rGan
    Sup3rGan.seed(seed)
    feats = set(lr) | set(out) | set(exo)
    m = Sup3rGan(gen, os.path.join(CFG, disc),
                 means={f: np.float32(MEANS[f]) for f in feats},
                 stdevs={f: np.float32(STDS[f]) for f in feats})
    m.set_model_params(lr_features=list(lr), hr_out_features=list(out),
                       hr_exo_features=list(exo), s_enhance=s, t_enhance=t)
    hr = (lr_shape[0],) + tuple(
        d * (s if i < 2 else t) for i, d in enumerate(lr_shape[1:-1])) + (
        len(out) + len(exo),)
    m.init_weights(lr_shape, hr)
    return m


@pytest.fixture(scope='module')
def steps():
    """the three models of the reference's test from the shipped specs, and
    variants of the wind step: with topography ('input' + 'layer' exo), with
    three outputs in another order, and a second 1x step"""
    s_disc, st_disc = 'test_disc_s_same.json', 'test_disc_st_same.json'
    out = {
        'solar': _gan(_spec('spatial/gen_2x_1f.json'), s_disc, CSR, CSR, 2, 1,
                      (3, 10, 9, 1), 1),
        'wind': _gan(_spec('spatial/gen_2x_2f.json'), s_disc, WIND, WIND, 2,
                     1, (3, 10, 9, 2), 2),
        'temporal': _gan(_spec('sup3rcc/gen_solar_1x_8x_1f.json'), st_disc,
                         CSR + WIND, CSR, 1, 8, (1, 20, 18, 3, 3), 3),
        'wind_topo': _gan(_spec('spatial/gen_2x_2f.json', topo=True), s_disc,
                          WIND + ['topography'], WIND, 2, 1, (3, 10, 9, 3), 4,
                          exo=['topography']),
        'wind_3': _gan(_spec('spatial/gen_2x_2f.json', filters=3), s_disc,
                       WIND, ['V_200m', 'U_10m', 'U_200m'], 2, 1,
                       (3, 10, 9, 2), 5),
    }
    # a second wind step, 1x: the expansion of the 2x spec taken out
    spec = _spec('spatial/gen_2x_2f.json', filters=3)
    layers = spec['hidden_layers']
    k = [la.get('class') for la in layers].index('SpatialExpansion')
    del layers[k]
    out['wind_1x'] = _gan(spec, s_disc, ['U_200m', 'U_10m', 'V_200m'],
                          ['V_200m', 'U_10m', 'U_200m'], 1, 1, (3, 20, 18, 3),
                          6)
    return out


def _solar(steps, wind=('wind',), t_enhance=None):
    from sup3r_amd import MultiStepGan, SolarMultiStepGan
    steps['temporal'].meta['t_enhance'] = 8
    return SolarMultiStepGan(
        MultiStepGan([steps['solar']]),
        MultiStepGan([steps[k] for k in wind]),
        MultiStepGan([steps['temporal']]), t_enhance=t_enhance)


def _input(n_feat=3, seed=41):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((3, 10, 9, n_feat)).astype(np.float32)
    mu = np.array([0.7, 4.2, 5.6], np.float32)[:n_feat]
    sd = np.array([0.04, 1.1, 1.3], np.float32)[:n_feat]
    return x * sd + mu


def _both_routes(ms, x, exo=None, **kw):
    assert ms._device_blocker(
        x, *(ms_exo for ms_exo in _split(ms, exo))) is None
    host = ms.generate(x, exogenous_data=exo, device=False, **kw)
    dev = ms.generate(x, exogenous_data=exo, device=True, **kw)
    auto = ms.generate(x, exogenous_data=exo, **kw)
    assert host.dtype == dev.dtype == np.float32
    assert np.isfinite(host).all() and host.std() > 0
    np.testing.assert_array_equal(dev, host)
    np.testing.assert_array_equal(auto, host)
    return host


def _split(ms, exo):
    from sup3r_amd.utilities import ExoData
    if exo is None:
        return None, None
    return ExoData(exo).split([len(ms.spatial_wind_models)])


def test_reference_solar_multistep_test():
    """tests/forward_pass/test_multi_step.py:234-288 on the shipped specs with
    the reference test's statistics: save, load, swapped directories,
    generate(np.ones((3, 10, 10, 3))) -> (1, 20, 20, 24, 1)"""
    from sup3r_amd import SolarMultiStepGan, Sup3rGan

    def model(gen, disc, lr, out, lr_shape, res):
        m = Sup3rGan(os.path.join(CFG, 'sup3r', gen),
                     os.path.join(CFG, 'sup3r', disc))
        _ = m.generate(np.ones(lr_shape))
        m.set_norm_stats({f: MEANS[f] for f in lr}, {f: STDS[f] for f in lr})
        m.meta['input_resolution'] = {'spatial': res, 'temporal': '40min'}
        m.set_model_params(lr_features=lr, hr_out_features=out)
        return m
    Sup3rGan.seed(0)
    m1 = model('spatial/gen_2x_1f.json', 'spatial/disc.json', CSR, CSR,
               (4, 10, 10, 1), '8km')
    m2 = model('spatial/gen_2x_2f.json', 'spatial/disc.json', WIND, WIND,
               (4, 10, 10, 2), '4km')
    m3 = model('sup3rcc/gen_solar_1x_8x_1f.json', 'spatiotemporal/disc.json',
               CSR + WIND, CSR, (4, 10, 10, 3, 3), '2km')
    with tempfile.TemporaryDirectory() as td:
        fp1, fp2, fp3 = (os.path.join(td, f'model{i}') for i in (1, 2, 3))
        m1.save(fp1)
        m2.save(fp2)
        m3.save(fp3)
        with pytest.raises(AssertionError):
            SolarMultiStepGan.load(fp2, fp1, fp3)
        ms = SolarMultiStepGan.load(fp1, fp2, fp3)
        assert ms.s_enhance == 2 and ms.t_enhance == 8 and len(ms.meta) == 3
        x = np.ones((3, 10, 10, 3))
        out = ms.generate(x)
        assert out.shape == (1, 20, 20, 24, 1)
        # (a float64 array is normalised in float64 by numpy: the host route;
        # the same numbers in float32 stay on the device)
        assert 'float32' in ms._device_blocker(x, None, None)
        x32 = x.astype(np.float32)
        assert ms._device_blocker(x32, None, None) is None
        np.testing.assert_array_equal(ms.generate(x32, device=True),
                                      ms.generate(x32, device=False))
        # the pipeline's loader reaches ``load`` through the three keywords
        from sup3r_amd.forward_pass import get_model
        kw = {'spatial_solar_model_dirs': fp1, 'spatial_wind_model_dirs': fp2,
              'temporal_solar_model_dirs': [fp3], 't_enhance': 8}
        via = get_model('SolarMultiStepGan', kw)
        assert isinstance(via, SolarMultiStepGan)
        np.testing.assert_array_equal(via.generate(x32), ms.generate(x32))


@pytest.mark.parametrize('norm_in', [True, False])
@pytest.mark.parametrize('un_norm_out', [True, False])
def test_device_route_equals_host_route(steps, norm_in, un_norm_out):
    ms = _solar(steps)
    x = _input() if norm_in else \
        np.random.default_rng(43).standard_normal((3, 10, 9, 3)).astype(
            np.float32)
    y = _both_routes(ms, x, norm_in=norm_in, un_norm_out=un_norm_out)
    assert y.shape == (1, 20, 18, 24, 1)


def test_device_route_with_topography_exo(steps):
    """the wind branch takes lo-res topography at its input and hi-res
    topography mid-network (tests/forward_pass/test_forward_pass_exo.py:
    1030-1125); the exo data is not changed by a call"""
    ms = _solar(steps, wind=('wind_topo',))
    assert ms.lr_features == CSR + WIND + ['topography']
    rng = np.random.default_rng(47)
    lo = (100 + 50 * rng.standard_normal((3, 10, 9, 1))).astype(np.float32)
    hi = (100 + 50 * rng.standard_normal((3, 20, 18, 1))).astype(np.float32)
    exo = {'topography': {'steps': [
        {'model': 0, 'combine_type': 'input', 'data': lo},
        {'model': 0, 'combine_type': 'layer', 'data': hi}]}}
    y = _both_routes(ms, _input(), exo)
    assert y.shape == (1, 20, 18, 24, 1)
    assert [s['model'] for s in exo['topography']['steps']] == [0, 0]
    # ... and the topography is used
    exo2 = {'topography': {'steps': [
        {'model': 0, 'combine_type': 'input', 'data': lo + 25},
        {'model': 0, 'combine_type': 'layer', 'data': hi}]}}
    assert not np.array_equal(ms.generate(_input(), exogenous_data=exo2), y)
    # 'input' exo in float64 is normalised in float64 by numpy: host route
    exo['topography']['steps'][0]['data'] = lo.astype(np.float64)
    with pytest.raises(RuntimeError, match='not float32'):
        ms.generate(_input(), exogenous_data=exo, device=True)
    assert ms.generate(_input(), exogenous_data=exo).shape == y.shape


def test_device_route_with_two_wind_steps_and_another_output_order(steps):
    """a s3_step_handover inside the wind branch (2x with three outputs, then
    1x taking them in another order), and a wind output order (V_200m,
    U_10m, U_200m) that differs from the temporal model's input order
    (clearsky_ratio, U_200m, V_200m)"""
    ms = _solar(steps, wind=('wind_3',))
    assert list(ms.idf_wind_out) == [2, 0]
    one = _both_routes(ms, _input())
    ms2 = _solar(steps, wind=('wind_3', 'wind_1x'))
    assert len(ms2) == 3 and ms2.s_enhance == 2 and ms2.t_enhance == 8
    two = _both_routes(ms2, _input())
    assert one.shape == two.shape == (1, 20, 18, 24, 1)
    assert not np.array_equal(one, two)


def test_device_route_pads_in_time(steps):
    """the padding arrives through a ``t_enhance`` override: 10 instead of the
    layers' 8 makes pad = (3 * 10 - 24) / 2 = 3 on either side of the 24
    generated hours (the constructor writes the temporal model's meta itself,
    past ``set_model_params``' enhancement checks; the shipped temporal spec
    has no Cropping3D on time)"""
    ms = _solar(steps, t_enhance=10)
    assert ms.t_enhance == 10
    for un_norm_out in (True, False):
        y = _both_routes(ms, _input(), un_norm_out=un_norm_out)
        assert y.shape == (1, 20, 18, 30, 1)
        np.testing.assert_array_equal(y[..., :3, :], y[..., 6:3:-1, :])
        np.testing.assert_array_equal(y[..., 27:, :], y[..., 25:22:-1, :])
    core = _solar(steps).generate(_input())
    assert core.shape == (1, 20, 18, 24, 1)
    padded = _solar(steps, t_enhance=10).generate(_input())
    np.testing.assert_array_equal(padded[..., 3:27, :], core)


def test_fallback_when_a_step_brings_its_own_normalisation(steps):
    from sup3r_amd import MultiStepGan, SolarMultiStepGan, Sup3rGan

    class OwnNorm(Sup3rGan):
        def norm_input(self, low_res):
            return super().norm_input(low_res) * np.float32(0.5)
    wind = steps['wind']
    own = OwnNorm.__new__(OwnNorm)
    own.__dict__.update(wind.__dict__)
    ms = SolarMultiStepGan(MultiStepGan([steps['solar']]),
                           MultiStepGan([own]),
                           MultiStepGan([steps['temporal']]))
    x = _input()
    assert 'overrides' in ms._device_blocker(x, None, None)
    with pytest.raises(RuntimeError, match='overrides norm_input'):
        ms.generate(x, device=True)
    y = ms.generate(x)
    np.testing.assert_array_equal(y, ms.generate(x, device=False))
    assert not np.array_equal(y, _solar(steps).generate(x))


@pytest.mark.parametrize('batch', [1, 3])
def test_executor_runs_the_class_chunk_by_chunk(steps, batch):
    """``iter_chunks`` over a (20, 18, 6, 3) domain in chunks of (10, 9, 3)
    with spatial and temporal padding of 1: every chunk is ``generate`` on
    that chunk's input followed by the chunk's crop; no chunk fails"""
    from sup3r_amd import ForwardPass
    from sup3r_amd.forward_pass import register_model
    from sup3r_amd.strategy import ArrayStrategy
    ms = _solar(steps)
    kw = {'spatial_solar_model_dirs': 's', 'spatial_wind_model_dirs': 'w',
          'temporal_solar_model_dirs': 't'}
    register_model('SolarMultiStepGan', kw, ms)
    rng = np.random.default_rng(53)
    domain = (rng.standard_normal((20, 18, 6, 3)).astype(np.float32) *
              np.array([0.04, 1.1, 1.3], np.float32) +
              np.array([0.7, 4.2, 5.6], np.float32))
    stg = ArrayStrategy(domain, kw, (10, 9, 3), spatial_pad=1,
                        temporal_pad=1, model_class='SolarMultiStepGan',
                        max_nodes=1, model=ms)
    fwp = ForwardPass(stg, 0)
    ids = [int(i) for i in stg.node_chunks[0]]
    assert len(ids) == 8
    assert not ForwardPass._device_path(ms, fwp.get_input_chunk(ids[0]))
    got = {}
    for c, failed, data in ForwardPass.iter_chunks(
            (fwp.get_input_chunk(i) for i in ids), ms, batch=batch):
        assert not failed
        got[c.index] = np.array(data)
    assert sorted(got) == sorted(ids)
    for i in ids:
        c = fwp.get_input_chunk(i)
        assert c.input_data.dtype == np.float32
        want = ms.generate(np.transpose(c.input_data, (2, 0, 1, 3)))[0][
            tuple(c.hr_crop_slice)]
        assert got[i].shape == want.shape and got[i].shape[-1] == 1
        np.testing.assert_array_equal(got[i], want)
    # the reference's per-chunk entry point loads the class by name
    failed, data = ForwardPass.run_chunk(
        fwp.get_input_chunk(ids[0]), kw, 'SolarMultiStepGan', False)
    assert not failed
    np.testing.assert_array_equal(data, got[ids[0]])
