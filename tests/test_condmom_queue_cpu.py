"""Conditional-moment batch queues without a device: the numpy / scipy
restatement's own invariants (tests/condmom_ref.py), then the queue and handler
logic of ``sup3r_amd.batch_queue_conditional`` with the oracle transform and
the restatement injected, over the 16 parametrisations of the reference's
tests/training/test_train_conditional.py."""
import itertools
import threading

import numpy as np
import pytest

from tests import condmom_ref as R
from tests.test_batch_queue import DummySampler

FEATURES = ['u_100m', 'v_100m']
ST, S = (12, 12, 16), (12, 12, 1)
# (end_t_padding, time_enhance_mode, kind, sample_shape, s_enhance, t_enhance)
PARAMS = [(False, 'constant', 'Mom1'), (True, 'constant', 'Mom1'),
          (False, 'constant', 'Mom1SF'), (False, 'linear', 'Mom1SF'),
          (False, 'constant', 'Mom2'), (False, 'constant', 'Mom2SF'),
          (False, 'constant', 'Mom2Sep'), (False, 'constant', 'Mom2SepSF')]
PARAMS = [p + (ST, 3, 4) for p in PARAMS] + [p + (S, 2, 1) for p in PARAMS]
IDS = [f'{"st" if p[3] == ST else "s"}-{p[2]}-{p[1]}-{"endpad" if p[0] else "nopad"}'
       for p in PARAMS]


# ------------------------------------------------- the restatement itself
@pytest.mark.parametrize('s', [2, 3, 5, 7])
def test_zoom_order0_is_repeat(s):
    rng = np.random.default_rng(s)
    x5 = rng.standard_normal((2, 3, 4, 5, 2)).astype(np.float32)
    x4 = x5[:, :, :, 0]
    for x in (x4, x5):
        want = np.repeat(np.repeat(x, s, axis=1), s, axis=2)
        np.testing.assert_array_equal(R.enhance_space(x, s), want)
    np.testing.assert_array_equal(R.enhance_time(x5, 4, 'constant'),
                                  np.repeat(x5, 4, axis=3))
    assert R.enhance_time(x5, 1, 'linear') is x5
    with pytest.raises(ValueError, match='must be 5D'):
        R.enhance_time(x4, 4)


def test_linear_time_mode_is_the_line_through_neighbours():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 2, 2, 3, 1)).astype(np.float32)
    y = R.enhance_time(x, 4, 'linear')
    assert y.shape == (1, 2, 2, 12, 1) and y.dtype == np.float32
    # (scipy evaluates lo + slope * dx at the landmarks too: an ulp may move)
    np.testing.assert_allclose(y[:, :, :, ::4], x, rtol=0, atol=1e-6)
    x64 = x.astype(np.float64)
    # inside the first segment, and extrapolated past the last landmark
    np.testing.assert_allclose(y[:, :, :, 1], x64[:, :, :, 0] + 0.25 * (
        x64[:, :, :, 1] - x64[:, :, :, 0]), rtol=0, atol=1e-6)
    np.testing.assert_allclose(y[:, :, :, 11], x64[:, :, :, 1] + 1.75 * (
        x64[:, :, :, 2] - x64[:, :, :, 1]), rtol=0, atol=1e-6)


@pytest.mark.parametrize('shape', [(2, 12, 12, 16, 2), (2, 12, 12, 2)])
def test_mask_box_for_every_padding_combination(shape):
    """the restatement's slices and the product's (s_pad, t_lo, t_hi) box
    describe the same set of cells, counted by hand"""
    from sup3r_amd.batch_queue_conditional import mask_box
    t_enhance = 4 if len(shape) == 5 else 1
    for s_pad, t_pad, end in itertools.product((0, 1, 2), (0, 1, 3),
                                               (False, True)):
        mask = R.make_mask(shape, s_pad, t_pad, end, t_enhance)
        side = shape[1] - 2 * s_pad
        if len(shape) == 5:
            steps = shape[3] - 2 * t_pad - (t_enhance - 1 if end else 0)
        else:
            steps = 1
        assert mask.sum() == shape[0] * side * side * steps * shape[-1]
        assert set(np.unique(mask)) <= {0.0, 1.0}
        box = mask_box(shape, s_pad, t_pad, end, t_enhance)
        assert box[0] == s_pad
        assert box[2] - box[1] == steps
        inner = mask[0, s_pad, s_pad]
        if len(shape) == 5:
            assert inner[box[1]:box[2]].all() and inner.sum() == \
                steps * shape[-1]
        _, again = R.target(3, t_enhance, [0, 1])(
            np.zeros(shape, np.float32), box=box, output=False)
        np.testing.assert_array_equal(again, mask)


# ------------------------------------------------------------ queue logic
def _oracle_transform(s_enhance, t_enhance, features):
    from oracle.transform import transform

    def f(samples, smoothing=None, smoothing_ignore=None,
          temporal_coarsening_method='subsample'):
        lr, hr = transform(np.asarray(samples, np.float64), s_enhance,
                           t_enhance, features, list(range(len(features))),
                           smoothing, smoothing_ignore,
                           temporal_coarsening_method)
        return lr.astype(np.float32), hr.astype(np.float32)
    return f


class HostMom1:
    """stands for a first-moment ``Sup3rCondMom``: a fixed function of the
    low-res batch, and a note of the thread it ran on"""

    hr_exo_features = []

    def __init__(self, s_enhance, t_enhance):
        self.s, self.t = s_enhance, t_enhance
        self.threads = []

    def get_hr_exo_input(self, hi_res_true):
        return {}

    def generate(self, lr):
        y = np.repeat(np.repeat(np.asarray(lr, np.float32), self.s, 1),
                      self.s, 2)
        if y.ndim == 5:
            y = np.repeat(y, self.t, 3)
        return (np.float32(0.5) * y + np.float32(0.125)).astype(np.float32)

    def _tf_generate(self, low_res, hi_res_exo=None):
        assert hi_res_exo == {}
        self.threads.append(threading.current_thread())
        return self.generate(low_res)


def _samplers(sample_shape, seeds=(1, 2)):
    return [DummySampler(sample_shape, (14, 14, 24), 2, FEATURES, seed=s)
            for s in seeds]


def _raw_of(batch, samplers, squeeze):
    """the raw batch of a sampler's record that became ``batch``"""
    for smp in samplers:
        for raw in smp.drawn:
            raw = raw[..., 0, :] if squeeze else raw
            if np.array_equal(raw, batch.high_res):
                return raw
    raise AssertionError('batch does not stem from a recorded draw')


@pytest.mark.parametrize(
    'end_t_padding, mode, kind, sample_shape, s_enhance, t_enhance', PARAMS,
    ids=IDS)
def test_conditional_handler_batches(end_t_padding, mode, kind, sample_shape,
                                     s_enhance, t_enhance):
    import sup3r_amd
    from sup3r_amd import batch_queue_conditional as Q
    handler_cls = getattr(Q, 'BatchHandler' + kind)
    queue_cls = getattr(Q, 'Queue' + kind)
    assert handler_cls is getattr(sup3r_amd, 'DeviceBatchHandler' + kind)
    assert queue_cls is getattr(sup3r_amd, 'DeviceQueue' + kind)
    assert issubclass(handler_cls, queue_cls)
    assert issubclass(queue_cls, Q.ConditionalBatchQueue)
    lower = HostMom1(s_enhance, t_enhance)
    train, val = _samplers(sample_shape), _samplers(sample_shape, (3,))
    bh = handler_cls(
        train, val, batch_size=2, n_batches=3, s_enhance=s_enhance,
        t_enhance=t_enhance, queue_cap=2, lower_models={1: lower},
        end_t_padding=end_t_padding, time_enhance_mode=mode, s_padding=1,
        t_padding=1, seed=0,
        transform=_oracle_transform(s_enhance, t_enhance, FEATURES),
        target=R.target(s_enhance, t_enhance, [0, 1]))
    assert type(bh.val_data) is queue_cls
    assert bh.val_data.lower_models is bh.lower_models
    assert bh.val_data.time_enhance_mode == mode
    assert bh.val_data.end_t_padding == end_t_padding
    assert set(bh.means) == set(FEATURES) and set(bh.stds) == set(FEATURES)
    squeeze = sample_shape[2] == 1
    hr_shape = (2,) + (sample_shape[:2] if squeeze else sample_shape) + (2,)
    lr_shape = (2, sample_shape[0] // s_enhance, sample_shape[1] // s_enhance
                ) + (() if squeeze else (sample_shape[2] // t_enhance,)) + (2,)
    transform = _oracle_transform(s_enhance, t_enhance, FEATURES)
    for queue, samplers in ((bh, train), (bh.val_data, val)):
        batches = list(queue)
        assert len(batches) == 3
        masks = set()
        for b in batches:
            assert b.dset_names == ['low_res', 'high_res', 'output', 'mask']
            assert b.low_res.shape == lr_shape
            for member in (b.high_res, b.output, b.mask):
                assert member.shape == hr_shape
            raw = _raw_of(b, samplers, squeeze)
            lr, hr = transform(raw)
            np.testing.assert_array_equal(b.low_res, lr)
            want = R.make_output(kind, lr, hr, s_enhance, t_enhance, mode,
                                 [0, 1], mom1=lower.generate(lr))
            assert b.output.dtype == np.float32
            np.testing.assert_array_equal(b.output, want)
            np.testing.assert_array_equal(b.mask, R.make_mask(
                hr_shape, 1, 1, end_t_padding, t_enhance))
            assert (b.output is b.high_res) == (kind == 'Mom1')
            masks.add(id(b.mask))
        assert len(masks) == 1           # one mask tensor per batch shape
    bh.stop()
    assert not bh.queue_thread.is_alive()
    assert not bh.val_data.queue_thread.is_alive()
    if kind in ('Mom2', 'Mom2SF'):
        # the first-moment model ran where get_batch was called, never on a
        # feeder thread
        assert len(lower.threads) == 6
        assert set(lower.threads) == {threading.current_thread()}
    else:
        assert lower.threads == []


def test_plain_handler_is_unchanged():
    from sup3r_amd.batch_queue import DeviceBatchHandler, DeviceBatchQueue
    bh = DeviceBatchHandler(_samplers(ST), _samplers(ST, (3,)), batch_size=2,
                            n_batches=2, s_enhance=3, t_enhance=4,
                            transform=_oracle_transform(3, 4, FEATURES))
    assert type(bh.val_data) is DeviceBatchQueue
    assert DeviceBatchHandler.VAL_QUEUE is DeviceBatchQueue
    b = next(iter(bh))
    assert b.dset_names == ['low_res', 'high_res']
    bh.stop()
    with pytest.raises(TypeError):       # conditional arguments are not its
        DeviceBatchHandler(_samplers(ST), batch_size=2, s_enhance=3,
                           t_enhance=4, s_padding=1)


# ----------------------------------------------------------------- errors
def _queue(kind, sample_shape=ST, s_enhance=3, t_enhance=4, **kw):
    from sup3r_amd import batch_queue_conditional as Q
    return getattr(Q, 'Queue' + kind)(
        _samplers(sample_shape), batch_size=2, n_batches=2,
        s_enhance=s_enhance, t_enhance=t_enhance,
        transform=_oracle_transform(s_enhance, t_enhance, FEATURES),
        target=R.target(s_enhance, t_enhance, [0, 1]), **kw)


@pytest.mark.parametrize('kind', ['Mom1SF', 'Mom2SF', 'Mom2SepSF'])
def test_4d_data_cannot_be_enhanced_in_time(kind):
    q = _queue(kind, lower_models={1: HostMom1(3, 4)})
    lr = np.zeros((2, 4, 4, 2), np.float32)
    hr = np.zeros((2, 12, 12, 2), np.float32)
    with pytest.raises(ValueError, match='Data must be 5D to do temporal '
                                         'enhancing'):
        q.make_output((lr, hr))


def test_linear_mode_needs_two_low_res_time_steps():
    """(scipy's interp1d returns NaN for a single landmark; here it is an
    error, at construction and for a batch that arrives with one)"""
    with pytest.raises(ValueError, match='two low-res time steps'):
        _queue('Mom1SF', sample_shape=(12, 12, 4),
               time_enhance_mode='linear')
    q = _queue('Mom1SF', time_enhance_mode='linear')
    with pytest.raises(ValueError, match='two low-res time steps'):
        q.make_output((np.zeros((2, 4, 4, 1, 2), np.float32),
                       np.zeros((2, 12, 12, 4, 2), np.float32)))
    # one step is fine where nothing is interpolated
    _queue('Mom1SF', sample_shape=(12, 12, 4), time_enhance_mode='constant')
    _queue('Mom1', sample_shape=(12, 12, 4), time_enhance_mode='linear')
    with pytest.raises(ValueError, match='time_enhance_mode'):
        _queue('Mom1SF', time_enhance_mode='cubic')


@pytest.mark.parametrize('kind', ['Mom2', 'Mom2SF'])
@pytest.mark.parametrize('lower', [None, {}, {2: HostMom1(3, 4)}])
def test_second_moment_needs_the_first_moment_model(kind, lower):
    with pytest.raises((KeyError, AssertionError)):
        _queue(kind, lower_models=lower)


def test_lib_declares_the_kernel():
    from sup3r_amd import _lib
    assert 's3_condmom_target' in _lib.EXPORTS
    assert (_lib.CM_SUBFILTER, _lib.CM_LINEAR, _lib.CM_MOM1,
            _lib.CM_SQUARE) == (1, 2, 4, 8)
