"""``StatsCollection`` over containers whose data lives on the device.

The reference builds a ``StatsCollection`` (sup3r/preprocessing/collections/
stats.py) in ``BatchHandlerFactory.__init__`` between building its samplers and
starting its queues: per-feature ``nanmean`` / ``nanstd`` of every training
container, combined across containers with the container weights, then every
container normalised in place.  :class:`DeviceStatsCollection` is that object
— same constructor, same methods, same control flow — over containers that
answer two calls:

* ``container.channel_moments(names)`` -> ``{name: (count, mean, std)}`` over
  all of space and time, NaN skipped, ddof 0, float64;
* ``container.normalize(means, stds)``: in place, for the features found in
  both dicts.

The device samplers (samplers.py) answer them with one ``s3_channel_moments``
pass per cube — one read serves ``get_means`` and ``get_stds`` — and one
``s3_normalize_channels`` pass; a numpy stand-in answers them in the tests.
Containers also need ``features`` and ``size``, as in the reference.

The arithmetic across containers follows the reference line by line: the
per-container statistic is a float32 (xarray reduces float32 data to float32),
multiplied by the float32 weight, summed in float32:

    means[f] = float32(sum_c  w_c * mean_c[f])
    stds[f]  = float32(sqrt(sum_c  w_c * std_c[f] ** 2))

The std formula is the reference's and is kept: it pools the containers'
variances and ignores the spread of their means, so containers with different
means get a smaller std than the std of their union.

Deviations: the per-container mean / std is the float64 device result rounded
to float32 once; xarray sums float32 pairwise, so its last bit can differ.
``_get_stat`` returns the statistics of the asked features only (the reference
computes the std of every feature and then reads the needed ones).  Feature
names are matched in lower case.  JSON is written with the ``json`` module
(values as Python floats, as ``safe_serialize`` writes them).
"""
import json
import logging
import os
import pprint
from warnings import warn

import numpy as np

logger = logging.getLogger(__name__)


class DeviceStatsCollection:
    """``StatsCollection(containers, means=None, stds=None)``: computes the
    missing means / stds, saves them if file paths were given, normalises the
    containers.  ``means`` / ``stds``: a dict (used as it is for the features
    it has), the path of a JSON file (read if it exists, written otherwise or
    when features were added), or None."""

    def __init__(self, containers, means=None, stds=None):
        self.containers = list(containers)
        self.data = tuple(getattr(c, 'data', None) for c in self.containers)
        self._features = []
        self._moments = {}            # container index -> {feature: (n, m, s)}
        self.means = self.get_means(means)
        self.stds = self.get_stds(stds)
        self.save_stats(stds=stds, means=means)
        self.normalize(self.containers)

    @property
    def features(self):
        """the union of the containers' features, in first-seen order"""
        if not self._features:
            for c in self.containers:
                for f in c.features:
                    if f not in self._features:
                        self._features.append(f)
        return self._features

    @property
    def container_weights(self):
        """the containers' shares of the data (collections/base.py:52-58)"""
        sizes = [c.size for c in self.containers]
        weights = sizes / np.sum(sizes)
        return weights.astype(np.float32)

    def _get_stat(self, stat_type, needed_features='all'):
        """``[{feature: float32 statistic}]``, one dict per container.  Every
        container is asked once for everything the collection needs, so one
        read of a cube serves the means and the stds."""
        all_feats = (self.features if needed_features == 'all'
                     else list(needed_features))
        which = {'mean': 1, 'std': 2}[stat_type]
        cstats = []
        for i, c in enumerate(self.containers):
            have = self._moments.setdefault(i, {})
            ask = [f for f in all_feats if f not in have]
            if ask:
                have.update(c.channel_moments(ask))
            cstats.append({f: np.float32(have[f][which]) for f in all_feats})
        return cstats

    def _init_stats_dict(self, stats):
        """a dict as it is, an existing file's content, or an empty dict; any
        other type is an error.  A dict that lacks features only warns."""
        if isinstance(stats, str) and os.path.exists(stats):
            with open(stats) as f:
                stats = json.load(f)
        elif stats is None or isinstance(stats, str):
            stats = {}
        else:
            msg = (f'Received incompatible type {type(stats)}. Need a file '
                   'path or dictionary')
            assert isinstance(stats, dict), msg
        if stats != {} and any(f not in stats for f in self.features):
            msg = (f'Not all features ({self.features}) are found in the given '
                   f'stats dictionary {stats}. This is obviously from a prior '
                   'run so you better be sure these stats carry over.')
            logger.warning(msg)
            warn(msg)
        return stats

    def _needed(self, stats):
        return [f for f in self.features if f not in stats]

    def get_means(self, means):
        """``{feature: mean}`` over all containers; only the features that
        ``means`` lacks are computed"""
        means = self._init_stats_dict(means)
        needed = self._needed(means)
        if needed:
            logger.info('Getting means for %s.', needed)
            weights = self.container_weights
            cmeans = [{f: cm[f] * w for f in needed} for cm, w in
                      zip(self._get_stat('mean', needed), weights)]
            for f in needed:
                means[f] = np.float32(np.sum([cm[f] for cm in cmeans]))
        return means

    def get_stds(self, stds):
        """``{feature: std}``: the square root of the weighted mean of the
        containers' variances (the reference's formula, see the module
        docstring); only the features that ``stds`` lacks are computed"""
        stds = self._init_stats_dict(stds)
        needed = self._needed(stds)
        if needed:
            logger.info('Getting stds for %s.', needed)
            weights = self.container_weights
            cstds = [{f: w * cs[f] ** 2 for f in needed} for cs, w in
                     zip(self._get_stat('std', needed), weights)]
            for f in needed:
                stds[f] = np.float32(np.sqrt(np.sum([cs[f] for cs in cstds])))
        return stds

    @staticmethod
    def _added_stats(fp, stat_dict):
        """does ``stat_dict`` hold features the file lacks"""
        with open(fp) as f:
            on_file = json.load(f)
        return any(f not in on_file for f in stat_dict)

    @staticmethod
    def _write(fp, stat_dict):
        with open(fp, 'w') as f:
            json.dump({k: float(v) for k, v in stat_dict.items()}, f)

    def save_stats(self, stds, means):
        """write the dicts to the given paths: new files, and files that
        features were added to"""
        if isinstance(stds, str) and (
                not os.path.exists(stds) or self._added_stats(stds, self.stds)):
            self._write(stds, self.stds)
            logger.info('Saved standard deviations %s to %s.', self.stds, stds)
        if isinstance(means, str) and (
                not os.path.exists(means)
                or self._added_stats(means, self.means)):
            self._write(means, self.means)
            logger.info('Saved means %s to %s.', self.means, means)

    def normalize(self, containers):
        """normalise ``containers`` (in place) with this collection's stats"""
        logger.debug('Normalizing containers with:\nmeans: %s\nstds: %s',
                     pprint.pformat(self.means, indent=2),
                     pprint.pformat(self.stds, indent=2))
        for i, c in enumerate(containers):
            logger.info('Normalizing container %s', i + 1)
            c.normalize(means=self.means, stds=self.stds)


# the reference's name
StatsCollection = DeviceStatsCollection

__all__ = ['DeviceStatsCollection', 'StatsCollection']
