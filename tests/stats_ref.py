"""numpy restatement of the statistics stage, for the tests of sup3r_amd/stats.py.

* per-container statistics: ``np.nanmean`` / ``np.nanstd`` (ddof 0) over all of
  space and time on the data WIDENED TO FLOAT64, one value per channel;
* the combination across containers as ``StatsCollection.get_means`` /
  ``get_stds`` write it (sup3r/preprocessing/collections/stats.py:103-136):
  float32 per-container statistics times float32 container weights, summed in
  float32, the std as the square root of the weighted mean of variances;
* ``Sup3rX.normalize`` (accessor.py:356-361) in float32;
* numpy containers that answer ``channel_moments`` / ``normalize`` the way the
  device samplers do, to drive ``DeviceStatsCollection`` without a GPU.

UNVERIFIED AGAINST XARRAY: xarray is not installed where these tests run.  The
reference reduces float32 data in float32 (numpy's pairwise sums), so the last
bits of its per-container means and stds can differ from the correctly rounded
float64 values used here — and from the device's, which are float64 too.
"""
import warnings

import numpy as np


def nan_moments(data):
    """``(count, mean, std)`` per channel of ``(..., C)``: float64 numpy over
    the widened data; NaN skipped; all-NaN -> (0, nan, nan); +-inf as numpy
    has it (mean +-inf or nan, std nan)"""
    x = np.asarray(data, dtype=np.float64).reshape(-1, np.shape(data)[-1])
    count = (~np.isnan(x)).sum(axis=0)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)
        return count, np.nanmean(x, axis=0), np.nanstd(x, axis=0)


def sumsq_moments(data):
    """the scheme that is NOT acceptable: float64 ``sum(x)`` and ``sum(x^2)``
    in one pass, ``var = sum(x^2) / n - mean^2``"""
    x = np.asarray(data, dtype=np.float64).reshape(-1, np.shape(data)[-1])
    n = x.shape[0]
    mean = x.sum(axis=0) / n
    var = (x * x).sum(axis=0) / n - mean * mean
    return mean, np.sqrt(np.maximum(var, 0.0))


def ulp_distance(a, b):
    """distance in float32 units in the last place between two float32 values
    (0 for equal values and for two NaNs; huge for NaN against a number)"""
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if np.isnan(a) and np.isnan(b) else 2 ** 32

    def key(v):                       # monotone integer image of a float32
        i = int(np.array(v, np.float32).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))


def container_weights(sizes):
    weights = list(sizes) / np.sum(sizes)
    return weights.astype(np.float32)


def combine_means(cmeans, weights):
    """``np.float32(np.sum([cm * w ...]))`` with float32 ``cm``"""
    return np.float32(np.sum([np.float32(m) * w
                              for m, w in zip(cmeans, weights)]))


def combine_stds(cstds, weights):
    """``np.float32(np.sqrt(np.sum([w * cs ** 2 ...])))`` with float32 ``cs``"""
    return np.float32(np.sqrt(np.sum([w * np.float32(s) ** 2
                                      for s, w in zip(cstds, weights)])))


def collection_stats(cubes, sizes=None):
    """(means, stds) float32 arrays per channel over the list of ``(..., C)``
    cubes with the same channels: the reference route"""
    sizes = [np.size(c) for c in cubes] if sizes is None else sizes
    w = container_weights(sizes)
    per = [nan_moments(c) for c in cubes]
    n_c = np.shape(cubes[0])[-1]
    means = np.array([combine_means([p[1][q] for p in per], w)
                      for q in range(n_c)], dtype=np.float32)
    stds = np.array([combine_stds([p[2][q] for p in per], w)
                     for q in range(n_c)], dtype=np.float32)
    return means, stds


def normalize(data, means, stds, flags=None):
    """float32 ``(x - float32(m)) / float32(s)`` per channel where flagged"""
    out = np.array(data, dtype=np.float32, copy=True)
    for q in range(out.shape[-1]):
        if flags is None or flags[q]:
            with np.errstate(all='ignore'):
                out[..., q] = ((out[..., q] - np.float32(means[q]))
                               / np.float32(stds[q]))
    return out


class NumpyCube:
    """a ``(..., C)`` float32 array with named channels that answers
    ``moments`` / ``normalize`` like ``samplers._ResidentCube``"""

    tensor = None

    def __init__(self, data, features):
        self.data = np.array(data, dtype=np.float32, copy=True)
        self.features = list(features)
        self._moments = None
        self.reads = 0                # passes over the data

    @property
    def shape(self):
        return self.data.shape

    def channels(self, names):
        low = [f.lower() for f in self.features]
        missing = [f for f in names if f.lower() not in low]
        if missing:
            raise KeyError(f'features {missing} are not in the data: '
                           f'{self.features}')
        return [low.index(f.lower()) for f in names]

    def moments(self, names):
        idx = self.channels(names)
        if self._moments is None:
            self._moments = nan_moments(self.data)
            self.reads += 1
        n, mean, std = self._moments
        out = {}
        for name, i in zip(names, idx):
            if n[i] == 0:
                warnings.warn(f'feature "{name}" holds no value (all NaN)')
            out[name] = (int(n[i]), mean[i], std[i])
        return out

    def normalize(self, means, stds):
        lo_m = {k.lower(): v for k, v in means.items()}
        lo_s = {k.lower(): v for k, v in stds.items()}
        flags = [f.lower() in lo_m and f.lower() in lo_s
                 for f in self.features]
        m = [lo_m.get(f.lower(), 0) for f in self.features]
        s = [lo_s.get(f.lower(), 1) for f in self.features]
        self.data = normalize(self.data, m, s, flags)
        self._moments = None


class NumpySampler:
    """the container surface ``DeviceStatsCollection`` uses, over one numpy
    cube; constructor keywords of ``DeviceSampler`` so that it can stand in
    as a handler's ``SAMPLER``"""

    device_resident = True

    def __init__(self, data, features, sample_shape=None, batch_size=16,
                 feature_sets=None, seed=None):
        self._cube = NumpyCube(data, features)
        self.features = list((feature_sets or {}).get('features', features))
        self.sample_shape = tuple(sample_shape or (2, 2, 1))
        self.batch_size, self.seed = batch_size, seed

    @property
    def data(self):
        return self._cube.data

    @property
    def size(self):
        return int(self._cube.data.size)

    @property
    def shape(self):
        return self._cube.data.shape

    def channel_moments(self, names):
        return self._cube.moments(list(names))

    def normalize(self, means, stds):
        self._cube.normalize(means, stds)

    def __next__(self):
        s1, s2, t = self.sample_shape
        return np.stack([self._cube.data[:s1, :s2, :t]] * self.batch_size)
