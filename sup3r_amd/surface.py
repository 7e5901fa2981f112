"""``SurfaceSpatialMetModel`` — the reference's non-neural spatial downscaler
of near-surface temperature, relative humidity and pressure
(sup3r/models/surface.py) on the MI355X.

The reference resizes one 2-D slice at a time with ``PIL.Image.resize`` on
the host (2 to 5 resizes per feature and slice, counting the bias fix).  Here
the whole batch goes through ``s3_surface_downscale`` (kernels_interp.hip):
Pillow's separable resize in mode 'F' restated with its own coefficients
(``pillow_coeffs``, float64 on the host, uploaded once per (length, s,
method)), the lapse-rate / scale-height / humidity-regression terms and the
bias fix ``hr -= R(C(hr) - lr)`` fused, the high-res field written once.

Semantics kept from the reference, quirks included:

* ``load`` is ``LinearInterp.load``: only the meta keys that are ``__init__``
  argument names come back, so ``temp_lapse_rate``, ``weight_for_delta_*``
  and ``pressure_*`` of a saved model are NOT reloaded (the defaults apply);
* the humidity -> temperature pairing is ``_get_temp_rh_ind`` literally,
  ``endswith`` match included (``relativehumidity_2m`` pairs with a
  ``temperature_12m`` listed first);
* a pressure field that is (or becomes) negative raises ``ValueError``;
  the high-res check is one device min-reduction and a 4-byte read-back.

Not kept: the noise of ``noise_adders`` is uniform on [0, stdev) as in the
reference, but drawn on the device (Philox4x32-10 keyed by ``seed()`` and a
per-call counter), so it does not reproduce numpy's draws.
"""
import ctypes as C
import logging
import math
from fnmatch import fnmatch
from warnings import warn

import numpy as np

from . import _lib
from .linear import LinearInterp, _device, _ptr

logger = logging.getLogger(__name__)


class Resampling:
    """The names and values of ``PIL.Image.Resampling``: an unknown name
    raises ``AttributeError``, as ``getattr(Image.Resampling, name)`` does."""
    NEAREST = 0
    LANCZOS = 1
    BILINEAR = 2
    BICUBIC = 3
    BOX = 4
    HAMMING = 5


_SUPPORT = {Resampling.BOX: 0.5, Resampling.BILINEAR: 1.0,
            Resampling.HAMMING: 1.0, Resampling.BICUBIC: 2.0,
            Resampling.LANCZOS: 3.0}
# Pillow's Hamming window is written with float literals
_F054, _F046 = float(np.float32(0.54)), float(np.float32(0.46))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (_F054 + _F046 * math.cos(x))


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_FILTERS = {Resampling.BOX: _box, Resampling.BILINEAR: _bilinear,
            Resampling.HAMMING: _hamming, Resampling.BICUBIC: _bicubic,
            Resampling.LANCZOS: _lanczos}


def pillow_coeffs(in_size, out_size, method):
    """Pillow's ``precompute_coeffs`` (libImaging/Resample.c) for one axis in
    float64: ``(lo, cnt, w[out_size, K])``, output ``o`` = sum over ``k <
    cnt[o]`` of ``w[o, k] * in[lo[o] + k]``.  An unchanged size is Pillow's
    copy and NEAREST its affine transform (source ``floor((o + 0.5) in /
    out)``): one tap of weight 1."""
    scale = in_size / out_size
    if in_size == out_size or method == Resampling.NEAREST:
        lo = np.floor((np.arange(out_size) + 0.5) * scale).astype(np.int32)
        return lo, np.ones(out_size, np.int32), np.ones((out_size, 1))
    filt = _FILTERS[method]
    filterscale = max(scale, 1.0)
    support = _SUPPORT[method] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    lo = np.zeros(out_size, np.int32)
    cnt = np.zeros(out_size, np.int32)
    w = np.zeros((out_size, ksize))
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)      # C truncation
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        lo[xx], cnt[xx] = xmin, xmax
        w[xx, :xmax] = k
    return lo, cnt, w


_TABLES = {}


def _table(dev, in_size, s, method):
    """(device table, host lo, host cnt, taps) of one axis, built once per
    (device, length, s, method)"""
    key = (dev.index, int(in_size), int(s), int(method))
    if key not in _TABLES:
        import torch
        lo, cnt, w = pillow_coeffs(int(in_size), int(in_size) * int(s),
                                   int(method))
        if np.any(np.diff(lo) < 0) or np.any(np.diff(lo + cnt) < 0):
            raise RuntimeError('resize coefficients are not monotonic')
        buf = np.concatenate([lo, cnt, w.astype(np.float32).view(np.int32)
                              .ravel()]).astype(np.int32)
        _TABLES[key] = (torch.from_numpy(buf).to(dev.torch_device),
                        np.ascontiguousarray(lo), np.ascontiguousarray(cnt),
                        w.shape[1])
    return _TABLES[key]


def _iptr(a):
    return C.c_void_p(a.ctypes.data)


def resize2d(x, s_enhance, method='LANCZOS', dev=None):
    """``PIL.Image.resize`` in mode 'F' of every (n, :, :, c) plane of ``x``
    (n, h, w, c), c <= 32, upscaled ``s_enhance`` times: ``s3_resize2d``,
    the result stays on the device (fp32 tensor)."""
    dev = dev or _device()
    m = getattr(Resampling, method) if isinstance(method, str) else int(method)
    s = int(s_enhance)
    xd = dev.to_device(x)
    n, h, w, c = (int(v) for v in xd.shape)
    y = dev.empty((n, h * s, w * s, c))
    planes = dev.empty(((3 * c + 1) * n * h * w,))
    tab_h, lo_h, cnt_h, k = _table(dev, h, s, m)
    tab_w = _table(dev, w, s, m)[0]
    rc = _lib.lib().s3_resize2d(dev.ctx, _ptr(xd), n, h, w, c, s, _ptr(tab_h),
                                _ptr(tab_w), _iptr(lo_h), _iptr(cnt_h), k,
                                _ptr(planes), _ptr(y))
    _lib.check(rc, dev.ctx, 's3_resize2d')
    return y


class LstsqRegression:
    """What ``sklearn.linear_model.LinearRegression(fit_intercept=False)``
    provides to ``train``'s callers — ``coef_``, ``intercept_`` (0.0),
    ``predict`` — from ``numpy.linalg.lstsq``."""
    intercept_ = 0.0

    def fit(self, x, y):
        self.coef_ = np.linalg.lstsq(np.asarray(x, np.float64),
                                     np.asarray(y, np.float64), rcond=None)[0]
        return self

    def predict(self, x):
        return np.asarray(x, np.float64) @ self.coef_


# the device noise generator: the k-th call after seed(s) draws from (s, k)
_NOISE = {'seed': 0, 'calls': 0}


class SurfaceSpatialMetModel(LinearInterp):
    """Spatial downscaling of daily near-surface temperature, relative
    humidity and pressure with lapse-rate, scale-height and regression
    corrections against topography (sup3r/models/surface.py:18-827)."""

    TEMP_LAPSE = 6.5 / 1000
    PRES_DIV = 44307.69231
    PRES_EXP = 5.25328
    W_DELTA_TEMP = -3.99242830
    W_DELTA_TOPO = -0.01736911

    def __init__(self, lr_features, s_enhance, noise_adders=None,
                 temp_lapse=None, w_delta_temp=None, w_delta_topo=None,
                 pres_div=None, pres_exp=None, interp_method='LANCZOS',
                 input_resolution=None, fix_bias=True):
        self._lr_features = lr_features
        self._s_enhance = s_enhance
        self._t_enhance = 1
        self._t_centered = False
        self._noise_adders = noise_adders
        self._temp_lapse = temp_lapse or self.TEMP_LAPSE
        self._w_delta_temp = w_delta_temp or self.W_DELTA_TEMP
        self._w_delta_topo = w_delta_topo or self.W_DELTA_TOPO
        self._pres_div = pres_div or self.PRES_DIV
        self._pres_exp = pres_exp or self.PRES_EXP
        self._fix_bias = fix_bias
        self._input_resolution = input_resolution
        self._interp_name = interp_method
        self._interp_method = getattr(Resampling, interp_method)
        if isinstance(self._noise_adders, (int, float)):
            self._noise_adders = [self._noise_adders] * len(self._lr_features)

    def __len__(self):
        return 1

    @staticmethod
    def seed(s=0):
        """Reset the device noise generator: the noise of the k-th
        ``generate`` after ``seed(s)`` is a function of (s, k) alone."""
        _NOISE['seed'], _NOISE['calls'] = int(s), 0

    input_dims = property(lambda self: 4)

    @staticmethod
    def _get_s_enhance(topo_lr, topo_hr):
        """surface.py:136-164"""
        assert len(topo_lr.shape) == 2, 'topo_lr must be 2D'
        assert len(topo_hr.shape) == 2, 'topo_hr must be 2D'
        se0 = topo_hr.shape[0] / topo_lr.shape[0]
        se1 = topo_hr.shape[1] / topo_lr.shape[1]
        assert se0 % 1 == 0, f'Bad calculated s_enhance on axis 0: {se0}'
        assert se1 % 1 == 0, f'Bad calculated s_enhance on axis 1: {se1}'
        assert se0 == se1, 'Calculated s_enhance does not match along axis'
        return int(se0)

    def _inds(self, pattern):
        return [i for i, name in enumerate(self._lr_features)
                if fnmatch(name, pattern)]

    feature_inds_temp = property(lambda self: self._inds('temperature_*'))
    feature_inds_pres = property(lambda self: self._inds('pressure_*'))
    feature_inds_rh = property(lambda self: self._inds('relativehumidity_*'))

    @property
    def feature_inds_other(self):
        tprh = (self.feature_inds_temp + self.feature_inds_pres +
                self.feature_inds_rh)
        return [i for i in range(len(self._lr_features)) if i not in tprh]

    def _get_temp_rh_ind(self, idf_rh):
        """surface.py:212-248: the first temperature feature whose name ends
        with the humidity feature's height suffix, both or neither of them
        ``_min_`` / ``_max_``; ``KeyError`` if there is none"""
        name_rh = self._lr_features[idf_rh]
        hh_suffix = name_rh.split('_')[-1]
        for i in self.feature_inds_temp:
            name = self._lr_features[i]
            same_hh = name.endswith(hh_suffix)
            not_minmax = not any(mm in name_rh for mm in ('_min_', '_max_'))
            both_mins = '_min_' in name_rh and '_min_' in name
            both_maxs = '_max_' in name_rh and '_max_' in name
            if same_hh and (not_minmax or both_mins or both_maxs):
                return i
        msg = ('Could not find temperature feature corresponding to '
               '"{}" in feature list: {}'.format(name_rh, self._lr_features))
        logger.error(msg)
        raise KeyError(msg)

    def _channel_plan(self):
        """(kinds, pairs) int32 arrays of s3_surface_downscale"""
        c = len(self._lr_features)
        kinds = np.full(c, _lib.SURF_OTHER, np.int32)
        pair = np.full(c, -1, np.int32)
        for i in self.feature_inds_temp:
            kinds[i] = _lib.SURF_TEMP
        for i in self.feature_inds_pres:
            kinds[i] = _lib.SURF_PRES
        for i in self.feature_inds_rh:
            kinds[i] = _lib.SURF_RH
            pair[i] = self._get_temp_rh_ind(i)
        return kinds, pair

    @property
    def meta(self):
        return {'temp_lapse_rate': self._temp_lapse,
                's_enhance': self._s_enhance,
                't_enhance': 1,
                'noise_adders': self._noise_adders,
                'input_resolution': self._input_resolution,
                'weight_for_delta_temp': self._w_delta_temp,
                'weight_for_delta_topo': self._w_delta_topo,
                'pressure_divisor': self._pres_div,
                'pressure_exponent': self._pres_exp,
                'lr_features': self.lr_features,
                'hr_out_features': self.hr_out_features,
                'interp_method': self._interp_name,
                'fix_bias': self._fix_bias,
                'class': self.__class__.__name__}

    def _get_topo_from_exo(self, exogenous_data):
        """surface.py:532-575: ``exogenous_data['topography']['steps']`` =
        [lr, hr], each 2-D or 4-D (then ``[0, :, :, 0]``); a plain dict
        without ``combine_type`` is accepted"""
        exo_data = [step['data']
                    for step in exogenous_data['topography']['steps']]
        msg = 'exogenous_data is of a bad type {}!'.format(type(exo_data))
        assert isinstance(exo_data, (list, tuple)), msg
        msg = 'exogenous_data is of a bad length {}!'.format(len(exo_data))
        assert len(exo_data) == 2, msg
        lr_topo, hr_topo = exo_data
        if len(lr_topo.shape) == 4:
            lr_topo = lr_topo[0, :, :, 0]
        if len(hr_topo.shape) == 4:
            hr_topo = hr_topo[0, :, :, 0]
        return lr_topo, hr_topo

    def _check_pressure_lr(self, low_res, lr_topo):
        """surface.py:471-495 on the low-res fields (host: they are small)"""
        const = 101325 * (1 - (1 - lr_topo / self._pres_div) **
                          self._pres_exp)
        for idf in self.feature_inds_pres:
            for iobs in range(len(low_res)):
                p = low_res[iobs, :, :, idf]
                if np.max(p) < 10000:
                    msg = ('Pressure data appears to not be in Pa with '
                           'min/mean/max: {:.1f}/{:.1f}/{:.1f}'.format(
                               p.min(), p.mean(), p.max()))
                    logger.warning(msg)
                    warn(msg)
                if np.min(p.copy() + const) < 0.0:
                    msg = ('Spatial interpolation of surface pressure '
                           'resulted in negative values. Incorrectly '
                           'scaled/unscaled values or incorrect units are '
                           'the most likely causes. All pressure data should '
                           'be in Pascals.')
                    logger.error(msg)
                    raise ValueError(msg)

    # pylint: disable=unused-argument
    def generate(self, low_res, norm_in=False, un_norm_out=False,
                 exogenous_data=None):
        """(n_obs, s1, s2, features) -> (n_obs, s1 s, s2 s, features)
        float32 (surface.py:578-713); ``norm_in`` / ``un_norm_out`` do
        nothing, as in the reference"""
        low_res = np.asarray(low_res)
        lr_topo, hr_topo = self._get_topo_from_exo(exogenous_data)
        lr_topo = np.asarray(lr_topo)
        hr_topo = np.asarray(hr_topo)
        msg = f'topo_lr needs to be 2d but has shape {lr_topo.shape}'
        assert len(lr_topo.shape) == 2, msg
        msg = f'topo_hr needs to be 2d but has shape {hr_topo.shape}'
        assert len(hr_topo.shape) == 2, msg
        msg = ('lr_topo.shape needs to match lr_res.shape[:2] but received '
               f'{lr_topo.shape} and {low_res.shape}')
        assert lr_topo.shape[0] == low_res.shape[1], msg
        assert lr_topo.shape[1] == low_res.shape[2], msg
        s_enhance = self._get_s_enhance(lr_topo, hr_topo)
        msg = ('Topo shapes of {} and {} did not match desired spatial '
               'enhancement of {}'.format(lr_topo.shape, hr_topo.shape,
                                          self._s_enhance))
        assert self._s_enhance == s_enhance, msg
        self._check_pressure_lr(low_res, lr_topo)
        return self.downscale_device(low_res, lr_topo, hr_topo).cpu().numpy()

    def downscale_device(self, low_res, lr_topo, hr_topo):
        """The device half of ``generate`` — numpy or device inputs, the
        (n, s1 s, s2 s, features) fp32 result left on the device; raises
        ``ValueError`` when a final pressure value is negative."""
        dev = _device()
        xd = dev.to_device(low_res)
        n, h, w, c = (int(v) for v in xd.shape)
        if c != len(self._lr_features):
            raise ValueError(f'{c} features in, the model has '
                             f'{len(self._lr_features)}')
        if c > 32:
            raise ValueError('SurfaceSpatialMetModel runs at most 32 '
                             'features per call')
        kinds, pair = self._channel_plan()
        noise = np.zeros(c, np.float32)
        for idf, stdev in enumerate(self._noise_adders or []):
            if stdev is not None:
                if idf >= c:
                    raise IndexError(f'noise_adders has {idf + 1} entries, '
                                     f'the data {c} features')
                noise[idf] = stdev
        s = int(self._s_enhance)
        m = self._interp_method
        tl, th = dev.to_device(lr_topo), dev.to_device(hr_topo)
        y = dev.empty((n, h * s, w * s, c))
        planes = dev.empty(((3 * c + 1) * n * h * w,))
        any_pres = bool(self.feature_inds_pres)
        g_hr = dev.empty((h * s * w * s,)) if any_pres else None
        tab_h, lo_h, cnt_h, k = _table(dev, h, s, m)
        tab_w = _table(dev, w, s, m)[0]
        consts = np.array([self._temp_lapse, self._w_delta_temp,
                           self._w_delta_topo, self._pres_div,
                           self._pres_exp], np.float32)
        pmin = np.full(1, np.inf, np.float32)
        call = _NOISE['calls'] & 0xFFFFFFFF
        _NOISE['calls'] += 1
        rc = _lib.lib().s3_surface_downscale(
            dev.ctx, _ptr(xd), n, h, w, c, s, _ptr(tab_h), _ptr(tab_w),
            _iptr(lo_h), _iptr(cnt_h), k, _iptr(kinds), _iptr(pair),
            _iptr(consts), int(bool(self._fix_bias)),
            _iptr(noise) if noise.any() else None,
            _NOISE['seed'] & 0xFFFFFFFFFFFFFFFF, call, _ptr(tl), _ptr(th),
            _ptr(planes), None if g_hr is None else _ptr(g_hr), _ptr(y),
            _iptr(pmin) if any_pres else None)
        _lib.check(rc, dev.ctx, 's3_surface_downscale')
        if any_pres and pmin[0] < 0.0:
            msg = ('Spatial interpolation of surface pressure '
                   'resulted in negative values. Incorrectly '
                   'scaled/unscaled values or incorrect units are '
                   'the most likely causes.')
            logger.error(msg)
            raise ValueError(msg)
        return y

    def train(self, true_hr_temp, true_hr_rh, true_hr_topo, input_resolution):
        """surface.py:735-827: fit the humidity regression on true high-res
        (lat, lon, n_days) temperature / humidity and (lat, lon) topography;
        the coarsening (``s3_coarsen``) and the LANCZOS resizes
        (``s3_resize2d``) run on the device.  Returns ``(w_delta_temp,
        w_delta_topo, regr, x, y)``; ``regr`` is an ``LstsqRegression``."""
        self._input_resolution = input_resolution
        assert len(true_hr_temp.shape) == 3, 'Bad true_hr_temp shape'
        assert len(true_hr_rh.shape) == 3, 'Bad true_hr_rh shape'
        assert len(true_hr_topo.shape) == 2, 'Bad true_hr_topo shape'
        s = int(self._s_enhance)
        true_hr_topo = np.repeat(np.expand_dims(true_hr_topo, axis=-1),
                                 true_hr_temp.shape[-1], axis=-1)
        lat, lon, nd = true_hr_temp.shape
        if lat % s or lon % s:
            raise ValueError('s_enhance must evenly divide grid size. '
                             f'Received s_enhance: {s} with data shape: '
                             f'{true_hr_temp.shape}')
        stack = np.stack([true_hr_temp, true_hr_rh, true_hr_topo], axis=-1)
        dev = _device()
        hr = dev.to_device(np.transpose(stack, (2, 0, 1, 3)))
        lr = dev.empty((nd, lat // s, lon // s, 3))
        rc = _lib.lib().s3_coarsen(dev.ctx, _ptr(hr), nd, lat, lon, 1, 3, s,
                                   1, _lib.TC_METHODS['subsample'], _ptr(lr))
        _lib.check(rc, dev.ctx, 's3_coarsen')
        interp = np.transpose(resize2d(lr, s, 'LANCZOS', dev).cpu().numpy(),
                              (1, 2, 0, 3))
        x1 = true_hr_temp - interp[..., 0]
        x2 = true_hr_topo - interp[..., 2]
        x = np.vstack((x1.flatten(), x2.flatten())).T
        y = (true_hr_rh - interp[..., 1]).flatten()
        regr = LstsqRegression().fit(x, y)
        return regr.coef_[0], regr.coef_[1], regr, x, y

