"""``LinearInterp`` — the reference's baseline model (sup3r/models/linear.py):
trilinear interpolation of every (obs, feature) field of a 5-D batch with
linear extrapolation at the borders (``st_interp``,
sup3r/models/utilities.py:161-212), one ``s3_st_interp`` launch per
``generate`` on the MI355X.

In index space, output index ``j`` of an axis enhanced ``e`` times samples the
source at ``(j + 0.5) / e - 0.5`` (the spatial axes, and time with
``t_centered``) or at ``j / e`` (time otherwise): the reference's cell-centred
(0, 10) meshes reduced to indices.  Every spatial and time axis needs length
>= 2 (``AssertionError``, as in the reference).

Reference quirk NOT copied: the reference builds its meshes with
``np.arange(0, 10, 10 / n)``, which has n + 1 points for 154 lengths below
5000 (61, 77, 122, 154, 211, ...), and its ``generate`` then fails on a shape
mismatch.  Here those lengths follow the formula and return the right shape.
"""
import ctypes as C
import json
import logging
import os
from inspect import signature

import numpy as np

from . import _lib

logger = logging.getLogger(__name__)

_AXES = {}


def _device():
    from .engine import Device
    return Device.get()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _plain(obj):
    """json ``default`` for numpy scalars / arrays in a meta dict"""
    if isinstance(obj, np.generic):
        return obj.item()
    if isinstance(obj, np.ndarray):
        return obj.tolist()
    return str(obj)


def interp_axis(n_in, enhance, centered):
    """(i0, f) of every output index of one axis from float64 positions: the
    value is ``a[i0] + f (a[i0 + 1] - a[i0])``, the edge intervals
    extrapolated"""
    j = np.arange(n_in * enhance, dtype=np.float64)
    p = (j + 0.5) / enhance - 0.5 if centered else j / enhance
    i0 = np.clip(np.floor(p), 0, n_in - 2)
    return i0.astype(np.int32), (p - i0).astype(np.float32)


def _axes_table(dev, s1, s2, t, s, te, t_centered):
    """the s3_st_interp axis table on the device, built once per shape"""
    key = (dev.index, s1, s2, t, s, te, bool(t_centered))
    if key not in _AXES:
        import torch
        parts = [interp_axis(s1, s, True), interp_axis(s2, s, True),
                 interp_axis(t, te, t_centered)]
        buf = np.concatenate([p[0] for p in parts] +
                             [p[1].view(np.int32) for p in parts])
        _AXES[key] = torch.from_numpy(buf).to(dev.torch_device)
    return _AXES[key]


class LinearInterp:
    """Linear interpolation along the spatial and temporal axes
    (sup3r/models/linear.py:15-171)."""

    def __init__(self, lr_features, s_enhance, t_enhance, t_centered=False,
                 input_resolution=None):
        self._lr_features = lr_features
        self._s_enhance = s_enhance
        self._t_enhance = t_enhance
        self._t_centered = t_centered
        self._input_resolution = input_resolution

    @classmethod
    def load(cls, model_dir, verbose=False):
        """linear.py:48-81: ``cls(**meta)`` from ``model_params.json``,
        keeping only the meta keys that are ``__init__`` argument names"""
        fp_params = os.path.join(model_dir, 'model_params.json')
        assert os.path.exists(fp_params), f'Could not find: {fp_params}'
        with open(fp_params) as f:
            params = json.load(f)
        meta = params['meta']
        args = signature(cls.__init__).parameters
        model = cls(**{k: v for k, v in meta.items() if k in args})
        if verbose:
            logger.info('Loading %s with meta data: %s', cls.__name__,
                        model.meta)
        return model

    @property
    def meta(self):
        return {'input_resolution': self._input_resolution,
                'lr_features': self._lr_features,
                's_enhance': self._s_enhance,
                't_enhance': self._t_enhance,
                't_centered': self._t_centered,
                'hr_out_features': self.hr_out_features,
                'class': self.__class__.__name__}

    model_params = property(lambda self: {'meta': self.meta})
    lr_features = property(lambda self: self._lr_features)
    hr_out_features = property(lambda self: self._lr_features)
    hr_exo_features = property(lambda self: [])
    # no normalisation statistics (what MultiStepGan's properties read)
    means = property(lambda self: None)
    stdevs = property(lambda self: None)
    s_enhance = property(lambda self: int(self._s_enhance))
    t_enhance = property(lambda self: int(self._t_enhance))
    s_enhancements = property(lambda self: [self.s_enhance])
    t_enhancements = property(lambda self: [self.t_enhance])
    input_dims = property(lambda self: 5)
    is_5d = property(lambda self: self.input_dims == 5)
    is_4d = property(lambda self: self.input_dims == 4)

    @property
    def input_resolution(self):
        res = self.meta.get('input_resolution')
        assert res is not None, \
            'model.input_resolution is None. This needs to be set.'
        return res

    def save(self, out_dir):
        """writes ``model_params.json`` (interface.py:501-517)"""
        self.save_params(out_dir)

    def save_params(self, out_dir):
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, 'model_params.json'), 'w') as f:
            json.dump(self.model_params, f, sort_keys=True, indent=2,
                      default=_plain)

    # pylint: disable=unused-argument
    def generate(self, low_res, norm_in=False, un_norm_out=False,
                 exogenous_data=None):
        """(n, s1, s2, t, f) -> (n, s1 s, s2 s, t t_enhance, f) float32;
        ``norm_in``, ``un_norm_out`` and ``exogenous_data`` are ignored, as in
        the reference"""
        return self.generate_device(low_res).cpu().numpy()

    def generate_device(self, low_res):
        """``generate`` with the output left on the device (fp32 tensor);
        ``low_res`` may already be a device tensor"""
        if not hasattr(low_res, 'shape'):
            low_res = np.asarray(low_res)
        shape = tuple(int(v) for v in low_res.shape)
        if len(shape) != 5:
            raise ValueError('LinearInterp takes (n, s1, s2, t, features) '
                             f'arrays, got {shape}')
        assert not any(v <= 1 for v in shape[1:4]), \
            'Input to st_interp cannot include axes with length 1'
        if shape[4] != len(self.hr_out_features):
            raise ValueError(f'{shape[4]} features in, the model has '
                             f'{len(self.hr_out_features)}')
        n, s1, s2, t, c = shape
        s, te = self.s_enhance, self.t_enhance
        dev = _device()
        x = dev.to_device(low_res)
        y = dev.empty((n, s1 * s, s2 * s, t * te, c))
        axes = _axes_table(dev, s1, s2, t, s, te, self._t_centered)
        rc = _lib.lib().s3_st_interp(dev.ctx, _ptr(x), n, s1, s2, t, c, s, te,
                                     _ptr(axes), _ptr(y))
        _lib.check(rc, dev.ctx, 's3_st_interp')
        return y
