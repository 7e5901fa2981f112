"""Samplers whose data lives on the device.

The reference's samplers (sup3r/preprocessing/samplers/base.py, dc.py,
dual.py) cut every batch out of their container with numpy on the host and
the batch queue uploads it.  The samplers here upload their ``(S1, S2, T, C)``
cube ONCE, in the constructor, and ``next(sampler)`` is index arithmetic on the
host (microseconds) plus one ``s3_sample_gather`` launch (include/sup3r_hip.h)
whose box origins and channel map travel in the kernel arguments: what comes
out is a device tensor ``(batch_size, s1, s2, t, C')`` and nothing crosses
PCIe.  A :class:`~sup3r_amd.batch_queue.DeviceBatchQueue` over such samplers
starts no feeder thread (``device_resident``).

* :class:`DeviceSampler` — ``Sampler``: uniform boxes; a "fast" batch is one
  box of ``batch_size * t`` consecutive steps cut into ``batch_size`` samples,
  a "slow" one ``batch_size`` independent boxes (when the cube is too short);
* :class:`DeviceSamplerDC` — ``SamplerDC``: box and time starts drawn with the
  bin weights of the data-centric handler (:func:`start_probabilities`);
* :class:`DeviceDualSampler` — ``DualSampler``: paired low-res / high-res cubes
  (and optionally observations with NaN holes), drawn on the low-res grid.

Draws come from one ``numpy.random.default_rng(seed)`` per sampler, in the
reference's order: row ``integers(0, S1 - s1 + 1)``, column ``integers(0, S2 -
s2 + 1)``, time ``integers(0, T - n_obs * t + 1)`` (the weighted samplers:
``choice(starts, p=...)`` for the box, then for the time).  A generator of the
same seed replays them.

``gather=`` stands in for the device: a callable ``(origins, channels) ->
batch`` (for the dual sampler a dict of them by member name), so the index
logic runs without a GPU — the counterpart of ``DeviceBatchQueue(transform=)``.

Multi-GPU: every rank holds its own copy of the cube (the samplers are built
per process, on ``Device.get()`` of that rank) and draws with its own seed.

``DualSamplerCC`` (daily / hourly pairs, daylight reduction and ``nn_fill`` of
the clearsky ratio) is in samplers_cc.py.  Not here: reading containers from
files.

Statistics: ``sampler.channel_moments(names)`` (one ``s3_channel_moments`` pass
per cube, cached) and ``sampler.normalize(means, stds)`` (``s3_normalize_
channels``, in place) are what :class:`~sup3r_amd.stats.DeviceStatsCollection`
drives — the stage the reference runs between building its samplers and
starting its queues.
"""
import ctypes as C
import logging
from fnmatch import fnmatch
from warnings import warn

import numpy as np

logger = logging.getLogger(__name__)


def _lowered(names):
    return [str(n).lower() for n in names]


def sample_gather(dev, cube, origins, box, channels):
    """``out[m, i, j, k, q] = cube[i0[m] + i, j0[m] + j, k0[m] + k,
    channels[q]]`` for the ``(n, 3)`` host ``origins`` and the ``box`` ``(s1,
    s2, t)``: one asynchronous ``s3_sample_gather`` on the device's stream."""
    from . import _lib
    org = np.ascontiguousarray(origins, dtype=np.int32).reshape(-1, 3)
    ch = np.ascontiguousarray(channels, dtype=np.int32)
    n, (s1, s2, t) = len(org), (int(v) for v in box)
    S1, S2, T, Cc = (int(v) for v in cube.shape)
    out = dev.empty((n, s1, s2, t, len(ch)))
    ip = C.POINTER(C.c_int32)
    rc = _lib.lib().s3_sample_gather(
        dev.ctx, C.c_void_p(cube.data_ptr()), S1, S2, T, Cc,
        org.ctypes.data_as(ip), n, s1, s2, t, ch.ctypes.data_as(ip), len(ch),
        C.c_void_p(out.data_ptr()))
    _lib.check(rc, dev.ctx, 's3_sample_gather')
    return out


def channel_moments(dev, cube):
    """``(C, 3)`` float64 — count of non-NaN values, their mean, their sum of
    squared deviations from it — per channel of the channels-last fp32 device
    tensor ``cube``: one ``s3_channel_moments`` pass and one read-back."""
    import torch
    from . import _lib
    c = int(cube.shape[-1])
    out = torch.empty((c, 3), dtype=torch.float64, device=cube.device)
    rc = _lib.lib().s3_channel_moments(
        dev.ctx, C.c_void_p(cube.data_ptr()), cube.numel() // c, c,
        C.c_void_p(out.data_ptr()))
    _lib.check(rc, dev.ctx, 's3_channel_moments')
    return out.cpu().numpy()


def normalize_channels(dev, cube, means, stds, flags):
    """``cube[..., q] = (cube[..., q] - means[q]) / stds[q]`` in place where
    ``flags[q]``: one asynchronous ``s3_normalize_channels`` (float32, two
    correctly rounded operations)."""
    from . import _lib
    c = int(cube.shape[-1])
    m = np.ascontiguousarray(means, dtype=np.float32)
    s = np.ascontiguousarray(stds, dtype=np.float32)
    f = np.ascontiguousarray(flags, dtype=np.uint8)
    assert len(m) == len(s) == len(f) == c, (len(m), len(s), len(f), c)
    pf = C.POINTER(C.c_float)
    rc = _lib.lib().s3_normalize_channels(
        dev.ctx, C.c_void_p(cube.data_ptr()), cube.numel() // c, c,
        m.ctypes.data_as(pf), s.ctypes.data_as(pf),
        f.ctypes.data_as(C.POINTER(C.c_ubyte)))
    _lib.check(rc, dev.ctx, 's3_normalize_channels')


class _ResidentCube:
    """one ``(S1, S2, T, C)`` cube and the names of its channels: on the device
    (fp32, contiguous, uploaded here once), or — with a stand-in gather — just
    its shape.  ``Device.to_device`` does not copy a contiguous fp32 device
    tensor: a cube handed in as one is normalised in the caller's memory."""

    def __init__(self, data, features, device, gather, what):
        self.features = list(features)
        shape = tuple(int(v) for v in data.shape)
        assert len(shape) == 4 and shape[3] == len(self.features), (
            f'{what} data must be (S1, S2, T, C) with one channel per feature:'
            f' shape {shape}, features {self.features}')
        self.shape = shape
        self._index = {f.lower(): i for i, f in enumerate(self.features)}
        self.dev, self.tensor, self._gather = device, None, gather
        self._moments = None
        if gather is None:
            from . import _lib
            from .engine import Device
            self.dev = device or Device.get()
            self.tensor = self.dev.to_device(data)
            self.max_channels = _lib.SAMPLE_MAX_CHANNELS

    def channels(self, names):
        missing = [f for f in names if f.lower() not in self._index]
        if missing:
            raise KeyError(f'features {missing} are not in the data: '
                           f'{self.features}')
        return [self._index[f.lower()] for f in names]

    def gather(self, origins, box, channels):
        if self._gather is not None:
            return self._gather(np.asarray(origins), list(channels))
        if len(channels) > self.max_channels:
            raise ValueError(f'a sample carries at most {self.max_channels} '
                             f'features, {len(channels)} were asked for')
        return sample_gather(self.dev, self.tensor, origins, box, channels)

    def _need_tensor(self, what):
        if self.tensor is None:
            raise RuntimeError(f'{what} needs the cube on the device; this '
                               'one stands in for it with a gather callable')

    def moments(self, names):
        """``{name: (count, mean, std)}`` over all of space and time, NaN
        skipped, ddof 0 (xarray's ``.mean(skipna=True)`` / ``.std(skipna=
        True)``): one ``s3_channel_moments`` pass over the whole cube and one
        read-back of ``3 C`` doubles, kept until :meth:`normalize` changes the
        data.  A feature without a value is NaN, with a warning."""
        idx = self.channels(names)
        if self._moments is None:
            self._need_tensor('moments()')
            self._moments = channel_moments(self.dev, self.tensor)
        out = {}
        for name, i in zip(names, idx):
            n, mean, m2 = self._moments[i]
            if n == 0:
                msg = (f'feature "{name}" holds no value (all NaN): its mean '
                       'and standard deviation are NaN')
                logger.warning(msg)
                warn(msg)
                out[name] = (0, np.float64('nan'), np.float64('nan'))
            else:
                with np.errstate(invalid='ignore'):
                    out[name] = (int(n), np.float64(mean),
                                 np.sqrt(np.float64(m2) / np.float64(n)))
        return out

    def normalize(self, means, stds):
        """``x = (x - float32(mean)) / float32(std)`` IN PLACE for the
        features present in both dicts (``Sup3rX.normalize``,
        accessor.py:356-361; names compared in lower case): one
        ``s3_normalize_channels`` pass, bit for bit numpy's float32 result."""
        lo_m = {str(k).lower(): v for k, v in means.items()}
        lo_s = {str(k).lower(): v for k, v in stds.items()}
        c = len(self.features)
        m, s = np.zeros(c, np.float32), np.ones(c, np.float32)
        flag = np.zeros(c, np.uint8)
        for i, f in enumerate(self.features):
            if f.lower() in lo_m and f.lower() in lo_s:
                m[i], s[i], flag[i] = lo_m[f.lower()], lo_s[f.lower()], 1
        if not flag.any():
            return
        self._need_tensor('normalize()')
        normalize_channels(self.dev, self.tensor, m, s, flag)
        self._moments = None


class DeviceSampler:
    """``Sampler`` (samplers/base.py) over a cube resident on the device.

    ``data``: numpy array or tensor ``(S1, S2, T, C)``; ``features``: the names
    of its channels.  ``feature_sets``: ``features`` (the channels to sample,
    default all), ``lr_only_features``, ``hr_exo_features`` (names or
    patt*erns).  ``next(sampler)`` returns ``(batch_size, s1, s2, t,
    len(features))`` on the device; ``last_origins`` are the ``(batch_size,
    3)`` box origins it used."""

    device_resident = True

    def __init__(self, data, features, sample_shape=None, batch_size=16,
                 feature_sets=None, seed=None, device=None, gather=None):
        self._cube = _ResidentCube(data, features, device, gather,
                                   type(self).__name__)
        feature_sets = feature_sets or {}
        self.features = list(feature_sets.get('features', features))
        self._channels = self._cube.channels(self.features)
        self._lr_only_features = feature_sets.get('lr_only_features', [])
        self._hr_exo_features = feature_sets.get('hr_exo_features', [])
        self.sample_shape = sample_shape or (10, 10, 1)
        self.batch_size = int(batch_size)
        self.lr_features = self.features
        self.rng = np.random.default_rng(seed)
        self.last_origins = None
        self.preflight()

    # ------------------------------------------------------------ container
    @property
    def data(self):
        """the resident cube (None with a stand-in gather)"""
        return self._cube.tensor

    @property
    def shape(self):
        return self._cube.shape

    @property
    def size(self):
        """elements of the cube: the sampler's weight in a queue"""
        return int(np.prod(self.shape))

    def compute(self):
        """nothing to load: the data is already on the device"""
        return self

    # ----------------------------------------------------------- statistics
    def channel_moments(self, names):
        """``{name: (count, mean, std)}`` of the named features over the whole
        cube (NaN skipped, ddof 0, float64): what ``StatsCollection`` asks of
        a container.  One pass and one read-back per cube, cached."""
        return self._cube.moments(list(names))

    def normalize(self, means, stds):
        """normalise the cube IN PLACE with the features found in both dicts.
        A cube handed to the constructor as a contiguous fp32 device tensor
        was not copied: it is the caller's memory that is normalised, as the
        reference normalises its containers' datasets."""
        self._cube.normalize(means, stds)

    @property
    def sample_shape(self):
        return self._sample_shape

    @sample_shape.setter
    def sample_shape(self, sample_shape):
        shape = tuple(int(v) for v in sample_shape)
        if len(shape) == 2:
            logger.info('2-D sample shape %s: adding a time axis of 1', shape)
            shape = (*shape, 1)
        self._sample_shape = shape

    @property
    def hr_sample_shape(self):
        return self._sample_shape

    @hr_sample_shape.setter
    def hr_sample_shape(self, hr_sample_shape):
        self.sample_shape = hr_sample_shape

    def preflight(self):
        """the box must fit the raster and the time axis; a cube too short for
        ``batch_size`` consecutive samples only warns (slow batches)"""
        s1, s2, t = self.sample_shape
        assert s1 <= self.shape[0] and s2 <= self.shape[1], (
            f'spatial_sample_shape {(s1, s2)} is larger than the raster size '
            f'{self.shape[:2]}')
        assert self.shape[2] >= t, (
            f'sample_shape[2] ({t}) cannot be larger than the number of time '
            f'steps in the raw data ({self.shape[2]}).')
        if not self._fast_batch_possible():
            msg = (f'sample_shape[2] * batch_size ({t} * {self.batch_size}) is'
                   ' larger than the number of time steps in the raw data '
                   f'({self.shape[2]}): batches are built from batch_size '
                   'independent boxes instead of one box of batch_size * '
                   'sample_shape[2] consecutive steps.')
            logger.warning(msg)
            warn(msg)

    # ------------------------------------------------------------- features
    def _parse_features(self, unparsed):
        """names as a lower-cased list; with a ``*`` among them: every sampled
        feature that matches one of the patterns"""
        if isinstance(unparsed, str):
            parsed = [unparsed]
        elif unparsed is None:
            parsed = []
        else:
            parsed = list(unparsed)
        if any('*' in p for p in parsed):
            parsed = [f for f in self.features
                      if any(fnmatch(f.lower(), p.lower()) for p in parsed)]
        return _lowered(parsed)

    @property
    def lr_only_features(self):
        """features that only the low-res input carries"""
        return self._parse_features(self._lr_only_features)

    @property
    def hr_exo_features(self):
        """hi-res features fed to the model mid-network but not produced by
        it; they must close the feature list"""
        exo = self._parse_features(self._hr_exo_features)
        if exo:
            assert exo == _lowered(self.features[-len(exo):]), (
                f'High-res train-only features "{exo}" do not come at the end '
                f'of the full high-res feature set: {self.features}')
        return exo

    @property
    def hr_out_features(self):
        """features the generator outputs: neither low-res only nor exo"""
        lr_only, exo = self.lr_only_features, self.hr_exo_features
        out = [f for f in self.features
               if not any(fnmatch(f.lower(), p) for p in lr_only)
               and f.lower() not in exo]
        if not out:
            msg = (f'It appears that all handler features "{self.features}" '
                   'were specified as `hr_exo_features` or `lr_only_features` '
                   'and therefore there are no output features!')
            logger.error(msg)
            raise RuntimeError(msg)
        return _lowered(out)

    @property
    def hr_features_ind(self):
        """channels of a sample that make up the hi-res truth"""
        keep = self.hr_out_features + self.hr_exo_features
        return [i for i, f in enumerate(self.features) if f.lower() in keep]

    @property
    def hr_features(self):
        return [self.features[i].lower() for i in self.hr_features_ind]

    # ---------------------------------------------------------------- draws
    def _draw_box(self, shape, box):
        """row, then column"""
        return (int(self.rng.integers(0, shape[0] - box[0] + 1)),
                int(self.rng.integers(0, shape[1] - box[1] + 1)))

    def _draw_time(self, shape, steps):
        return int(self.rng.integers(0, shape[2] - steps + 1))

    def get_sample_index(self, n_obs=None):
        """``(rows, columns, steps, features)``: a random box with ``n_obs *
        t`` consecutive time steps (``n_obs`` default ``batch_size``)"""
        n_obs = n_obs or self.batch_size
        s1, s2, t = self.sample_shape
        i0, j0 = self._draw_box(self.shape, (s1, s2))
        k0 = self._draw_time(self.shape, t * n_obs)
        return (slice(i0, i0 + s1), slice(j0, j0 + s2),
                slice(k0, k0 + t * n_obs), self.features)

    def _fast_batch_possible(self):
        return self.batch_size * self.sample_shape[2] <= self.shape[2]

    def _batch_indices(self):
        """the sample indices of one batch: one of ``batch_size`` samples'
        worth of steps (fast) or ``batch_size`` of one sample each (slow)"""
        if self._fast_batch_possible():
            return [self.get_sample_index(n_obs=self.batch_size)]
        return [self.get_sample_index(n_obs=1) for _ in range(self.batch_size)]

    @staticmethod
    def _origins(indices, t, batch_size):
        """(batch_size, 3) box origins: sample m of a fast batch starts ``m *
        t`` steps into the slice"""
        if len(indices) == 1:
            i, j, k = indices[0][:3]
            return np.array([(i.start, j.start, k.start + m * t)
                             for m in range(batch_size)], dtype=np.int32)
        return np.array([(i.start, j.start, k.start)
                         for i, j, k, *_ in indices], dtype=np.int32)

    def __next__(self):
        origins = self._origins(self._batch_indices(), self.sample_shape[2],
                                self.batch_size)
        self.last_origins = origins
        return self._cube.gather(origins, self.sample_shape, self._channels)


def start_probabilities(n_starts, weights):
    """probability of each of ``n_starts`` consecutive start indices under bin
    ``weights`` (samplers/utilities.py:81-86, :128-134): the starts are split
    with ``np.array_split`` into ``len(weights)`` consecutive chunks, a start
    in chunk b weighs ``weights[b]``, the whole is normalised."""
    weights = np.asarray(weights, dtype=np.float64).ravel()
    chunks = np.array_split(np.arange(int(n_starts)), len(weights))
    p = np.concatenate([np.full(len(c), w) for c, w in zip(chunks, weights)])
    total = p.sum()
    if not (np.isfinite(total) and total > 0 and (p >= 0).all()):
        raise ValueError(
            f'the weights {weights.tolist()} leave none of the {n_starts} '
            'starts a probability (bins without a start get no weight)')
    return p / total


class DeviceSamplerDC(DeviceSampler):
    """``SamplerDC`` (samplers/dc.py): the box start and the time start are
    drawn with bin weights that the data-centric handler updates from the
    validation loss.  A "space bin" is a band of the row-major flattened box
    starts, as in the reference — not a rectangle of the domain."""

    def __init__(self, data, features, sample_shape=None, batch_size=16,
                 feature_sets=None, spatial_weights=None,
                 temporal_weights=None, **kwargs):
        self.spatial_weights = [1] if spatial_weights is None \
            else spatial_weights
        self.temporal_weights = [1] if temporal_weights is None \
            else temporal_weights
        super().__init__(data, features, sample_shape=sample_shape,
                         batch_size=batch_size, feature_sets=feature_sets,
                         **kwargs)

    start_probabilities = staticmethod(start_probabilities)

    def update_weights(self, spatial_weights, temporal_weights):
        self.spatial_weights = spatial_weights
        self.temporal_weights = temporal_weights

    def _draw_box(self, shape, box):
        n_rows, n_cols = shape[0] - box[0] + 1, shape[1] - box[1] + 1
        starts = np.arange(n_rows * n_cols)
        start = int(self.rng.choice(starts, p=start_probabilities(
            len(starts), self.spatial_weights)))
        return start // n_cols, start % n_cols

    def _draw_time(self, shape, steps):
        starts = np.arange(shape[2] - steps + 1)
        return int(self.rng.choice(starts, p=start_probabilities(
            len(starts), self.temporal_weights)))


class DeviceDualSampler(DeviceSampler):
    """``DualSampler`` (samplers/dual.py): paired cubes, ``low_res`` ``(L1, L2,
    TL, C_lr)`` and ``high_res`` ``(L1 s, L2 s, TL t_enhance, C_hr)``, optionally
    ``obs`` on the hi-res grid, with the channels of ``high_res`` and NaN
    where nothing was observed (they arrive untouched: the gather is a copy).
    ``lr_features`` / ``hr_features`` name the cubes' channels;
    ``sample_shape`` is the hi-res one.  ``next(sampler)`` is the
    tuple ``(low_res, high_res[, obs])`` with the sampler's ``lr_features``,
    ``hr_features`` and ``hr_out_features``."""

    def __init__(self, low_res, high_res, lr_features, hr_features,
                 sample_shape=None, batch_size=16, s_enhance=1, t_enhance=1,
                 feature_sets=None, obs=None, seed=None, device=None,
                 gather=None):
        gather = gather or {}
        who = type(self).__name__
        self._lr = _ResidentCube(low_res, lr_features, device,
                                 gather.get('low_res'), who + ' low_res')
        self._hr = self._cube = _ResidentCube(
            high_res, hr_features, device, gather.get('high_res'),
            who + ' high_res')
        self._obs = None if obs is None else _ResidentCube(
            obs, hr_features, device, gather.get('obs'), who + ' obs')
        self.dset_names = ['low_res', 'high_res', 'obs'][:2 + (obs is not None)]
        self.s_enhance, self.t_enhance = int(s_enhance), int(t_enhance)
        feature_sets = feature_sets or {}
        self._lr_only_features = feature_sets.get('lr_only_features', [])
        self._hr_exo_features = feature_sets.get('hr_exo_features', [])
        self.features = self.get_features(feature_sets)
        lr_names = _lowered(self._lr.features)
        self.lr_features = [f for f in self.features if f.lower() in lr_names]
        self.sample_shape = sample_shape or (10, 10, 1)
        self.batch_size = int(batch_size)
        s1, s2, t = self.hr_sample_shape
        self.lr_sample_shape = (s1 // self.s_enhance, s2 // self.s_enhance,
                                t // self.t_enhance)
        self.rng = np.random.default_rng(seed)
        self.last_origins = self.last_lr_origins = None
        self.check_for_consistent_shapes()
        self.preflight()

    def get_features(self, feature_sets):
        """low-res features, then the hi-res ones not among them, the exo
        features last — unless ``feature_sets['features']`` says otherwise"""
        exo = _lowered(self._hr_exo_features)
        feats = []
        for f in [*self._lr.features, *self._hr.features]:
            if f not in feats and f.lower() not in exo:
                feats.append(f)
        return list(feature_sets.get('features', feats + exo))

    def check_for_consistent_shapes(self):
        enhanced = (self._lr.shape[0] * self.s_enhance,
                    self._lr.shape[1] * self.s_enhance,
                    self._lr.shape[2] * self.t_enhance)
        assert self._hr.shape[:3] == enhanced, (
            f'hr_data.shape {self._hr.shape[:3]} and enhanced lr_data.shape '
            f'{enhanced} are not compatible with the given enhancement '
            'factors')
        if self._obs is not None:
            assert self._obs.shape[:3] == self._hr.shape[:3], (
                f'obs.shape {self._obs.shape[:3]} is not the hi-res grid '
                f'{self._hr.shape[:3]}')

    @property
    def low_res(self):
        return self._lr.tensor

    @property
    def high_res(self):
        return self._hr.tensor

    @property
    def obs(self):
        return None if self._obs is None else self._obs.tensor

    def _members(self):
        return [c for c in (self._lr, self._hr, self._obs) if c is not None]

    def channel_moments(self, names):
        """the split of ``StatsCollection._get_stat`` (collections/stats.py:
        51-74): features that ``high_res`` carries come from ``high_res``, the
        remaining ones from ``low_res``; ``obs`` is never asked"""
        names = list(names)
        hr_names = _lowered(self._hr.features)
        hr = [f for f in names if f.lower() in hr_names]
        out = self._hr.moments(hr) if hr else {}
        lr = [f for f in names if f.lower() not in hr_names]
        if lr:
            out.update(self._lr.moments(lr))
        return {f: out[f] for f in names}

    def normalize(self, means, stds):
        """every member — ``low_res``, ``high_res`` and ``obs`` — IN PLACE,
        each for its features found in both dicts (``Sup3rX.normalize`` per
        member).  Members that are one and the same device tensor (handed in
        twice, not copied) are normalised once.  As for
        :meth:`DeviceSampler.normalize`, cubes handed in as contiguous fp32
        device tensors are the caller's memory."""
        done = set()
        for cube in self._members():
            tensor = getattr(cube, 'tensor', None)
            key = id(cube) if tensor is None else tensor.data_ptr()
            if key not in done:
                cube.normalize(means, stds)
                done.add(key)
            cube._moments = None

    def get_sample_index(self, n_obs=None):
        """``(lr_index, hr_index[, obs_index])``: drawn on the low-res grid,
        the hi-res box is that box times the enhancement factors"""
        n_obs = n_obs or self.batch_size
        l1, l2, tl = self.lr_sample_shape
        i0, j0 = self._draw_box(self._lr.shape, (l1, l2))
        k0 = self._draw_time(self._lr.shape, tl * n_obs)
        lr = (slice(i0, i0 + l1), slice(j0, j0 + l2),
              slice(k0, k0 + tl * n_obs))
        s, te = self.s_enhance, self.t_enhance
        hr = tuple(slice(a.start * f, a.stop * f)
                   for a, f in zip(lr, (s, s, te)))
        index = ((*lr, self.lr_features), (*hr, self.hr_features),
                 (*hr, self.hr_out_features))
        return index[:len(self.dset_names)]

    def __next__(self):
        indices = self._batch_indices()
        n = self.batch_size
        lr_org = self._origins([ix[0] for ix in indices],
                               self.lr_sample_shape[2], n)
        hr_org = self._origins([ix[1] for ix in indices],
                               self.hr_sample_shape[2], n)
        self.last_lr_origins, self.last_origins = lr_org, hr_org
        out = [self._lr.gather(lr_org, self.lr_sample_shape,
                               self._lr.channels(self.lr_features)),
               self._hr.gather(hr_org, self.hr_sample_shape,
                               self._hr.channels(self.hr_features))]
        if self._obs is not None:
            out.append(self._obs.gather(
                hr_org, self.hr_sample_shape,
                self._obs.channels(self.hr_out_features)))
        return tuple(out)


# the reference's names
Sampler, SamplerDC, DualSampler = DeviceSampler, DeviceSamplerDC, \
    DeviceDualSampler

__all__ = ['DeviceSampler', 'DeviceSamplerDC', 'DeviceDualSampler',
           'start_probabilities', 'sample_gather', 'channel_moments',
           'normalize_channels', 'Sampler', 'SamplerDC', 'DualSampler']
