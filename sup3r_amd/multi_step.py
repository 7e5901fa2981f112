"""``MultiStepGan`` — several trained single-step models run back to back
(what ``sup3r/models/multi_step.py:23-330`` provides: the
constructor / ``load`` / ``generate`` surface, the re-interpretation of the
array between spatial-only (4-D) and spatiotemporal (5-D) steps, the feature
selection between steps and the normalise-first / un-normalise-last rule).
Each step's conv stack runs on the MI355X through that model's ``generate``.
"""
import json
import logging
import os

import numpy as np

from .utilities import ExoData

logger = logging.getLogger(__name__)


def _as_model_rank(model, arr):
    """Present ``arr`` in the rank ``model`` consumes.  A stack of spatial
    fields ``(n, s1, s2, f)`` handed to a 5-D model is ONE sample whose time
    axis is the stack; a one-sample 5-D array handed to a 4-D model is a stack
    of its time steps."""
    if arr.ndim == model.input_dims:
        return arr
    if model.is_5d and arr.ndim == 4:
        return np.moveaxis(arr, 0, 2)[None]
    if model.is_4d and arr.ndim == 5:
        if arr.shape[0] != 1:
            raise AssertionError(
                f'a 4-D step can only take ONE 5-D sample, got {arr.shape}')
        return np.moveaxis(arr[0], 2, 0)
    raise AssertionError(f'{arr.shape} does not fit a {model.input_dims}-D '
                         'model')


class MultiStepGan:
    """Ordered tuple of trained single-step models."""

    def __init__(self, models):
        self._models = tuple(models)

    def __len__(self):
        return len(self._models)

    @classmethod
    def load(cls, model_dirs, model_kwargs=None, verbose=True):
        """One saved model directory per step; each step's class is the
        ``meta.class`` of its ``model_params.json`` (``Sup3rGan`` if absent)."""
        import sup3r_amd
        dirs = [model_dirs] if isinstance(model_dirs, str) else list(model_dirs)
        if model_kwargs is None:
            model_kwargs = [{}] * len(dirs)
        elif isinstance(model_kwargs, dict):
            model_kwargs = [model_kwargs]
        steps = []
        for d, kw in zip(dirs, model_kwargs):
            fp = os.path.join(d, 'model_params.json')
            if not os.path.exists(fp):
                raise AssertionError(f'{fp} does not exist')
            with open(fp) as f:
                meta = json.load(f).get('meta') or {}
            klass = getattr(sup3r_amd, meta.get('class', 'Sup3rGan'))
            steps.append(klass.load(d, verbose=verbose, **kw))
        return cls(steps)

    models = property(lambda self: self._models)
    means = property(lambda self: tuple(m.means for m in self._models))
    stdevs = property(lambda self: tuple(m.stdevs for m in self._models))
    meta = property(lambda self: tuple(m.meta for m in self._models))
    model_params = property(
        lambda self: tuple(m.model_params for m in self._models))
    lr_features = property(lambda self: self._models[0].lr_features)
    hr_out_features = property(lambda self: self._models[-1].hr_out_features)
    hr_exo_features = property(
        lambda self: [m.hr_exo_features for m in self._models])
    input_dims = property(lambda self: self._models[0].input_dims)
    is_5d = property(lambda self: self.input_dims == 5)
    is_4d = property(lambda self: self.input_dims == 4)

    @property
    def s_enhancements(self):
        return [e for m in self._models for e in m.s_enhancements]

    @property
    def t_enhancements(self):
        return [e for m in self._models for e in m.t_enhancements]

    s_enhance = property(lambda self: int(np.prod(self.s_enhancements)))
    t_enhance = property(lambda self: int(np.prod(self.t_enhancements)))

    @staticmethod
    def seed(s=0):
        from .gan import Sup3rGan
        Sup3rGan.seed(s=s)

    # kept under the reference's names for callers that reach for them
    @staticmethod
    def _transpose_model_input(model, hi_res):
        return _as_model_rank(model, hi_res)

    def _match_model_input(self, model_step, hi_res, exo_data):
        """Channels step ``model_step`` reads out of the previous step's
        output (its lo-res features minus what arrives as exogenous data), in
        the order it lists them."""
        if model_step == 0:
            return hi_res
        produced = self._models[model_step - 1].hr_out_features
        wanted = [f for f in self._models[model_step].lr_features
                  if f not in (exo_data or {})]
        missing = [f for f in wanted if f not in produced]
        if missing:
            raise ValueError(
                f'step {model_step} needs {missing}, step {model_step - 1} '
                f'only produces {produced}')
        return hi_res[..., [produced.index(f) for f in wanted]]

    def generate(self, low_res, norm_in=True, un_norm_out=True,
                 exogenous_data=None):
        """Run the chain.  Only the first step may skip normalising its input
        and only the last may skip un-normalising its output; every hand-over
        in between is in physical units."""
        if isinstance(exogenous_data, dict) and \
                not isinstance(exogenous_data, ExoData):
            exogenous_data = ExoData(exogenous_data)
        last = len(self._models) - 1
        arr = np.array(low_res, copy=True)
        for i, model in enumerate(self._models):
            step_exo = None if exogenous_data is None else \
                exogenous_data.get_model_step_exo(i)
            try:
                arr = self._match_model_input(
                    i, _as_model_rank(model, arr), step_exo)
                arr = model.generate(arr, norm_in=norm_in or i > 0,
                                     un_norm_out=un_norm_out or i < last,
                                     exogenous_data=step_exo)
            except Exception as e:
                raise RuntimeError(
                    f'step {i + 1} of {last + 1} ({type(model).__name__}) '
                    f'failed on an array of shape {arr.shape}') from e
        return arr


class MultiStepSurfaceMetGan(MultiStepGan):
    """A spatial-only surface step (``SurfaceSpatialMetModel``) on a 4-D stack
    of near-surface fields, then a (spatio)temporal model on the 5-D sample
    whose time axis is that stack (sup3r/models/multi_step.py:340-482).  The
    hand-over is ``_as_model_rank``'s (n, s1, s2, f) -> (1, s1, s2, n, f)."""

    def generate(self, low_res, norm_in=True, un_norm_out=True,
                 exogenous_data=None):
        """``MultiStepGan.generate`` after checking that ``exogenous_data``
        carries the two topography steps (low-res, high-res) of the surface
        step: a bare ``AssertionError`` otherwise, before any step runs."""
        msg = ('MultiStepSurfaceMetGan needs exogenous_data with two '
               'topography steps, for low and high res topography inputs.')
        exo_check = (exogenous_data is not None and
                     len(exogenous_data['topography']['steps']) == 2)
        assert exo_check, msg
        return super().generate(low_res, norm_in, un_norm_out, exogenous_data)

    @classmethod
    def load(cls, surface_model_class='SurfaceSpatialMetModel',
             temporal_model_class='MultiStepGan', surface_model_kwargs=None,
             temporal_model_kwargs=None, verbose=True):
        """the two models by class name from this package,
        ``Class.load(verbose=verbose, **kwargs)`` each, chained"""
        import sup3r_amd
        s_models = getattr(sup3r_amd, surface_model_class).load(
            verbose=verbose, **(surface_model_kwargs or {}))
        t_models = getattr(sup3r_amd, temporal_model_class).load(
            verbose=verbose, **(temporal_model_kwargs or {}))
        s_models = getattr(s_models, 'models', [s_models])
        t_models = getattr(t_models, 'models', [t_models])
        return cls([*s_models, *t_models])


class SolarMultiStepGan(MultiStepGan):
    """Two spatial chains side by side — solar only (``clearsky_ratio`` ->
    ``clearsky_ratio``) and wind (u / v (+ topography) -> u / v) — whose
    outputs are joined into one ``(clearsky_ratio, u_200m, v_200m)`` sample for
    a (spatio)temporal solar chain; the result is reflect-padded in time up to
    ``low_res.shape[0] * t_enhance`` (sup3r/models/multi_step.py:484-911).

    ``generate`` has two routes with the same bits: through the three
    sub-chains' ``generate`` and host numpy, as the reference does it, and
    device resident — one upload of ``low_res``, one download of the result,
    the join (s3_branch_join) and the pad (s3_time_pad_reflect) on the GPU."""

    def __init__(self, spatial_solar_models, spatial_wind_models,
                 temporal_solar_models, t_enhance=None):
        # ``models`` is what the aggregate enhancement factors come from:
        # counting both spatial branches would square the spatial one
        super().__init__([*spatial_wind_models.models,
                          *temporal_solar_models.models])
        self._spatial_solar_models = spatial_solar_models
        self._spatial_wind_models = spatial_wind_models
        self._temporal_solar_models = temporal_solar_models
        self._t_enhance = t_enhance
        self.preflight()
        if self._t_enhance is not None:
            msg = ('Can only update t_enhance for a '
                   'single temporal solar model.')
            assert len(self.temporal_solar_models) == 1, msg
            self.temporal_solar_models.models[0].meta['t_enhance'] = \
                self._t_enhance

    def preflight(self):
        """the loaded models can work together (multi_step.py:552-597)"""
        s_enh = self.spatial_solar_models.s_enhancements
        w_enh = self.spatial_wind_models.s_enhancements
        msg = ('Solar and wind spatial enhancements must be equivalent but '
               'received models that do spatial enhancements of '
               '{} (solar) and {} (wind)'.format(s_enh, w_enh))
        assert np.prod(s_enh) == np.prod(w_enh), msg
        s_t_feat = self.spatial_solar_models.lr_features
        s_o_feat = self.spatial_solar_models.hr_out_features
        msg = ('Solar spatial enhancement models need to take '
               '"clearsky_ratio" as the only input and output feature but '
               'received models that need {} and output {}'.format(
                   s_t_feat, s_o_feat))
        assert s_t_feat == ['clearsky_ratio'], msg
        assert s_o_feat == ['clearsky_ratio'], msg
        temp_solar_feats = self.temporal_solar_models.lr_features
        msg = ('Input feature 0 for the temporal_solar_models should be '
               '"clearsky_ratio" but received: {}'.format(temp_solar_feats))
        assert temp_solar_feats[0] == 'clearsky_ratio', msg
        spatial_out_features = (self.spatial_wind_models.hr_out_features +
                                self.spatial_solar_models.hr_out_features)
        missing = [fn for fn in temp_solar_feats
                   if fn not in spatial_out_features]
        msg = ('Solar temporal model needs features {} that were not '
               'found in the solar + wind model output feature list {}'.format(
                   missing, spatial_out_features))
        assert not any(missing), msg

    spatial_solar_models = property(lambda self: self._spatial_solar_models)
    spatial_wind_models = property(lambda self: self._spatial_wind_models)
    temporal_solar_models = property(
        lambda self: self._temporal_solar_models)
    meta = property(lambda self: (self.spatial_solar_models.meta +
                                  self.spatial_wind_models.meta +
                                  self.temporal_solar_models.meta))
    lr_features = property(
        lambda self: (self.spatial_solar_models.lr_features +
                      self.spatial_wind_models.lr_features))
    hr_out_features = property(
        lambda self: self.temporal_solar_models.hr_out_features)

    @property
    def idf_wind(self):
        """indices into ``lr_features`` of what the wind chain takes from the
        input array (topography arrives as exogenous data)"""
        return np.array([self.lr_features.index(fn)
                         for fn in self.spatial_wind_models.lr_features
                         if fn != 'topography'])

    @property
    def idf_wind_out(self):
        """indices into the wind chain's output of what the temporal chain
        takes after ``clearsky_ratio``, in the temporal chain's order"""
        return np.array([self.spatial_wind_models.hr_out_features.index(fn)
                         for fn in self.temporal_solar_models.lr_features[1:]])

    @property
    def idf_solar(self):
        return np.array([self.lr_features.index(fn)
                         for fn in self.spatial_solar_models.lr_features
                         if fn != 'topography'])

    def generate(self, low_res, norm_in=True, un_norm_out=True,
                 exogenous_data=None, *, device=None):
        """``low_res``: (temporal, spatial_1, spatial_2, features) with all of
        ``lr_features`` (minus topography supplied through
        ``exogenous_data``); returns (1, spatial_1, spatial_2, temporal,
        features) numpy (multi_step.py:694-822).  ``device``: None takes the
        device route where its conditions hold and the host route otherwise,
        False the host route, True the device route or a ``RuntimeError``
        naming the condition that does not hold."""
        if isinstance(exogenous_data, dict) and \
                not isinstance(exogenous_data, ExoData):
            exogenous_data = ExoData(exogenous_data)
        if exogenous_data is not None:
            s_exo, t_exo = exogenous_data.split(
                split_steps=[len(self.spatial_wind_models)])
        else:
            s_exo = t_exo = None
        if device is not False:
            why = self._device_blocker(low_res, s_exo, t_exo)
            if why is None:
                return self._generate_device(low_res, norm_in, un_norm_out,
                                             s_exo, t_exo)
            if device:
                raise RuntimeError(
                    'SolarMultiStepGan.generate(device=True): ' + why)
            logger.debug('SolarMultiStepGan takes the host route: %s', why)
        return self._generate_host(low_res, norm_in, un_norm_out, s_exo,
                                   t_exo)

    def _generate_host(self, low_res, norm_in, un_norm_out, s_exo, t_exo):
        """multi_step.py:751-822 over the three sub-chains and numpy"""
        try:
            hi_res_wind = self.spatial_wind_models.generate(
                low_res[..., self.idf_wind], norm_in=norm_in,
                un_norm_out=True, exogenous_data=s_exo)
        except Exception as e:
            msg = ('Could not run the 1st step spatial-wind-only GAN on '
                   'input shape {}'.format(low_res.shape))
            logger.exception(msg)
            raise RuntimeError(msg) from e
        try:
            hi_res_solar = self.spatial_solar_models.generate(
                low_res[..., self.idf_solar], norm_in=norm_in,
                un_norm_out=True)
        except Exception as e:
            msg = ('Could not run the 1st step spatial-solar-only GAN on '
                   'input shape {}'.format(low_res.shape))
            logger.exception(msg)
            raise RuntimeError(msg) from e
        hi_res = (hi_res_solar, hi_res_wind[..., self.idf_wind_out])
        hi_res = np.concatenate(hi_res, axis=3)
        hi_res = np.transpose(hi_res, axes=(1, 2, 0, 3))
        hi_res = np.expand_dims(hi_res, axis=0)
        try:
            hi_res = self.temporal_solar_models.generate(
                hi_res, norm_in=True, un_norm_out=un_norm_out,
                exogenous_data=t_exo)
        except Exception as e:
            msg = ('Could not run the 2nd step (spatio)temporal solar GAN on '
                   'input shape {}'.format(low_res.shape))
            logger.exception(msg)
            raise RuntimeError(msg) from e
        return self.temporal_pad(low_res, hi_res)

    def temporal_pad(self, low_res, hi_res, mode='reflect'):
        """pad the time axis of the 5-D ``hi_res`` on both sides up to
        ``low_res.shape[0] * t_enhance`` (multi_step.py:824-852)"""
        t_shape = low_res.shape[0] * self.t_enhance
        t_pad = int((t_shape - hi_res.shape[-2]) / 2)
        pad_width = ((0, 0), (0, 0), (0, 0), (t_pad, t_pad), (0, 0))
        return np.pad(hi_res, pad_width, mode=mode)

    @classmethod
    def load(cls, spatial_solar_model_dirs, spatial_wind_model_dirs,
             temporal_solar_model_dirs, t_enhance=None, verbose=True):
        """one or more saved model directories per chain
        (multi_step.py:854-911)"""
        ssm = MultiStepGan.load(spatial_solar_model_dirs, verbose=verbose)
        swm = MultiStepGan.load(spatial_wind_model_dirs, verbose=verbose)
        tsm = MultiStepGan.load(temporal_solar_model_dirs, verbose=verbose)
        return cls(ssm, swm, tsm, t_enhance=t_enhance)

    # -- the device route ---------------------------------------------------
    def _device_blocker(self, low_res, s_exo, t_exo):
        """None where ``generate`` can stay on the device, else the reason it
        cannot — the conditions ``ForwardPass._device_chain`` applies per
        step: this package's engine on one device, the base class's
        normalisation and input combination, fp32 statistics, at most 16
        channels at every hand-over, no 'output' exo; and what the hand-over
        kernels assume on top: fp32 input and 'input' exo (numpy would
        normalise anything wider in float64), exo fields in the rank of the
        step that takes them, 2-D branches in front of a 3-D temporal chain
        and no 'input' exo at the join (s3_branch_join has two sources)"""
        from .forward_pass import _is_base_method
        solar = list(self.spatial_solar_models.models)
        wind = list(self.spatial_wind_models.models)
        temporal = list(self.temporal_solar_models.models)
        if not (isinstance(low_res, np.ndarray) and low_res.ndim == 4 and
                low_res.dtype == np.float32):
            return 'the input is not a 4-D float32 numpy array'
        if low_res.shape[-1] > 16:
            return 'more than 16 input channels'
        first = getattr(wind[0], '_gen', None)
        if first is None:
            return 'the wind steps do not run on the HIP engine'
        for chain, rank in ((solar, 4), (wind, 4), (temporal, 5)):
            for m in chain:
                name = type(m).__name__
                if getattr(m, '_gen', None) is None or hasattr(m, 'models') \
                        or not getattr(m, 'supports_device_chunks', False):
                    return f'a {name} step does not run on the HIP engine'
                if not all(_is_base_method(m, fn) for fn in (
                        'norm_input', 'un_norm_output', 'generate',
                        '_combine_fwp_input')):
                    return (f'a {name} step overrides norm_input / '
                            'un_norm_output / generate / _combine_fwp_input')
                if m.input_dims != rank:
                    return f'a {name} step is {m.input_dims}-D, not {rank}-D'
                if m._gen.dev is not first.dev:
                    return 'the steps live on different devices'
                if len(m.lr_features) > 16 or len(m.hr_out_features) > 16:
                    return 'more than 16 channels at a hand-over'
                if m._means is not None:
                    for feats in (m.lr_features, m.hr_out_features):
                        mu, sd = m._stats_for(feats)
                        if mu.dtype != np.float32 or sd.dtype != np.float32:
                            return 'statistics that are not float32'
        for exo, chain in ((s_exo, wind), (t_exo, temporal)):
            for entry in (exo or {}).values():
                for st in entry['steps']:
                    kind = st['combine_type'].lower()
                    if kind == 'output':
                        return "'output' exogenous data"
                    k = st.get('model', 0)
                    if k >= len(chain) or \
                            np.ndim(st['data']) != chain[k].input_dims:
                        return ('an exogenous field that is not in the rank '
                                'of the step that takes it')
                    if kind == 'input' and \
                            np.asarray(st['data']).dtype != np.float32:
                        return "'input' exogenous data that is not float32"
                    if kind == 'input' and chain is temporal and k == 0:
                        return "'input' exogenous data at the join"
        return None

    @staticmethod
    def _exo_field(dev, step, data, keep, prep):
        """one exo field, given in ``step``'s own layout, on the device in
        that layout (``ForwardPass._exo_to_device`` takes a chunk's
        ``(s1, s2, t, c)`` view: a field that is constant in time crosses
        PCIe once)"""
        from .forward_pass import ForwardPass
        data = np.asarray(data)
        rank4 = step.input_dims == 4
        view = np.transpose(data, (1, 2, 0, 3)) if rank4 else data[0]
        return ForwardPass._exo_to_device(dev, [view], rank4, keep, prep)

    @classmethod
    def _step_input(cls, dev, y, cmap, affine, nxt, nxt_exo, norm, keep):
        """s3_step_handover: channels ``cmap`` of ``y`` un-normalised with
        ``affine`` = (scale, shift) (None, None: as they are), ``nxt``'s
        'input' exo channels appended, normalised with ``nxt``'s statistics
        when ``norm`` — the input of step ``nxt``"""
        from . import _lib
        from .forward_pass import _fptr, _nonzero_std, _vp
        import ctypes as C
        ysh = tuple(int(v) for v in y.shape)
        extra = len(nxt.lr_features) - len(cmap)
        names = list(nxt.lr_features[-extra:]) if extra > 0 else []
        absent = [f for f in names if f not in (nxt_exo or {})]
        assert not absent, (f'exogenous_data lacks {absent} '
                            '(combine_type "input")')
        exo_t = None
        if names:
            cols = [np.asarray(nxt_exo.get_combine_type_data(f, 'input'))
                    for f in names]
            exo_t = cls._exo_field(
                dev, nxt, cols[0] if len(cols) == 1 else
                np.concatenate(cols, axis=-1), keep, lambda a: a)
            if tuple(exo_t.shape[:-1]) != ysh[:-1]:
                raise RuntimeError(
                    f'"input" exo of shape {tuple(exo_t.shape)} for data '
                    f'of shape {ysh}')
        mu = sd = None
        if norm and nxt._means is not None:
            mu, sd = nxt._stats_for(nxt.lr_features)
            sd = np.ascontiguousarray(_nonzero_std(sd), dtype=np.float32)
            mu = np.ascontiguousarray(mu, dtype=np.float32)
        scale, shift = affine
        x = dev.empty(ysh[:-1] + (len(cmap) + len(names),))
        rc = _lib.lib().s3_step_handover(
            dev.ctx, _vp(y), int(np.prod(ysh[:-1], dtype=np.int64)), ysh[-1],
            (C.c_int32 * len(cmap))(*[int(v) for v in cmap]), len(cmap),
            _fptr(scale), _fptr(shift),
            _vp(exo_t) if exo_t is not None else None, len(names), _fptr(mu),
            _fptr(sd), _vp(x))
        _lib.check(rc, dev.ctx, 's3_step_handover')
        return x

    @classmethod
    def _layer_exo(cls, dev, m, ph, step_exo, norm, keep):
        """the 'layer' exo fields ``m``'s generator consumes mid-network,
        normalised as ``Sup3rGan.generate`` does, in the plan's shapes"""
        out = {}
        for name in ph.input_names:
            if name == 'x':
                continue
            assert step_exo is not None and name in step_exo, \
                f'the generator needs exogenous feature "{name}"'
            t = cls._exo_field(
                dev, m, step_exo.get_combine_type_data(name, 'layer'), keep,
                lambda a, name=name: m._reshape_norm_exo(
                    tuple(a.shape), a, name, norm_in=norm))
            # (the plan of a 2-D model carries a time axis of one)
            want = tuple(int(v) for v in ph.in_shapes[name])
            if tuple(v for v in t.shape if v != 1) != \
                    tuple(v for v in want if v != 1):
                raise RuntimeError(
                    f'exogenous "{name}" of shape {tuple(t.shape)} cannot '
                    f'be laid over hi-res {want}')
            out[name] = t.reshape(want)
        return out

    @classmethod
    def _walk(cls, dev, steps, x, exo, norm_first, keep):
        """a chain on the device from its first step's input ``x`` to its
        last generator's NORMALISED output: plan forward, s3_step_handover"""
        from .forward_pass import _unnorm_affine
        for i, m in enumerate(steps):
            e_i = None if exo is None else exo.get_model_step_exo(i)
            ph = m._gen.plan(tuple(int(v) for v in x.shape), training=False)
            y = ph.forward(x, cls._layer_exo(dev, m, ph, e_i,
                                             norm_first or i > 0, keep))
            if i + 1 == len(steps):
                return y
            nxt = steps[i + 1]
            e_n = None if exo is None else exo.get_model_step_exo(i + 1)
            produced = list(m.hr_out_features)
            wanted = [f for f in nxt.lr_features if f not in (e_n or {})]
            missing = [f for f in wanted if f not in produced]
            if missing:
                raise ValueError(f'step {i + 1} needs {missing}, step {i} '
                                 f'only produces {produced}')
            x = cls._step_input(dev, y, [produced.index(f) for f in wanted],
                                _unnorm_affine(m), nxt, e_n, True, keep)

    def _generate_device(self, low_res, norm_in, un_norm_out, s_exo, t_exo):
        """one upload, both branches and the temporal chain on the context's
        stream, the join and the pad as kernels, one download"""
        from . import _lib
        from .forward_pass import _fptr, _nonzero_std, _unnorm_affine, _vp
        import ctypes as C
        solar = list(self.spatial_solar_models.models)
        wind = list(self.spatial_wind_models.models)
        temporal = list(self.temporal_solar_models.models)
        dev, keep, L = wind[0]._gen.dev, [], _lib.lib()
        try:
            xd = dev.to_device(low_res)
            ys = []
            for steps, idf, exo in ((solar, self.idf_solar, None),
                                    (wind, self.idf_wind, s_exo)):
                e_0 = None if exo is None else exo.get_model_step_exo(0)
                x = self._step_input(dev, xd, idf, (None, None), steps[0],
                                     e_0, norm_in, keep)
                ys.append(self._walk(dev, steps, x, exo, norm_in, keep))
            ya, yb = ys
            nt, h, w, ca = (int(v) for v in ya.shape)
            if tuple(yb.shape[:3]) != (nt, h, w):
                raise RuntimeError(
                    f'the solar branch produced {tuple(ya.shape)}, the wind '
                    f'branch {tuple(yb.shape)}')
            first = temporal[0]
            map_b = [int(v) for v in self.idf_wind_out]
            mu, sd = first._stats_for(first.lr_features) \
                if first._means is not None else (None, None)
            if mu is not None:
                sd = np.ascontiguousarray(_nonzero_std(sd), dtype=np.float32)
                mu = np.ascontiguousarray(mu, dtype=np.float32)
            sc_a, sh_a = _unnorm_affine(solar[-1])
            sc_b, sh_b = _unnorm_affine(wind[-1])
            x = dev.empty((1, h, w, nt, ca + len(map_b)))
            rc = L.s3_branch_join(
                dev.ctx, _vp(ya), ca, (C.c_int32 * ca)(*range(ca)), ca,
                _fptr(sc_a), _fptr(sh_a), _vp(yb), int(yb.shape[-1]),
                (C.c_int32 * max(len(map_b), 1))(*map_b), len(map_b),
                _fptr(sc_b), _fptr(sh_b), nt, h, w, _fptr(mu), _fptr(sd),
                _vp(x))
            _lib.check(rc, dev.ctx, 's3_branch_join')
            y = self._walk(dev, temporal, x, t_exo, True, keep)
            _, y1, y2, t_out, n_out = (int(v) for v in y.shape)
            pad = int((low_res.shape[0] * self.t_enhance - t_out) / 2)
            scale, shift = _unnorm_affine(temporal[-1]) if un_norm_out \
                else (None, None)
            out = dev.empty((1, y1, y2, t_out + 2 * pad, n_out))
            rc = L.s3_time_pad_reflect(
                dev.ctx, _vp(y), y1 * y2, t_out, n_out, pad, _fptr(scale),
                _fptr(shift), _vp(out))
            _lib.check(rc, dev.ctx, 's3_time_pad_reflect')
            return out.cpu().numpy()
        except Exception as e:
            msg = ('Could not run the SolarMultiStepGan chains on the '
                   'device on input shape {}'.format(low_res.shape))
            logger.exception(msg)
            raise RuntimeError(msg) from e
        finally:
            keep.clear()
