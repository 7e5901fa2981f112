"""numpy / scipy restatement of the reference's conditional-moment batch
targets, for the tests of ``sup3r_amd.batch_queue_conditional`` (the product
never imports it):

* ``make_mask``: the box of ones of ``ConditionalBatchQueue.make_mask``
  (sup3r/preprocessing/batch_queues/conditional.py:79-127), by the same
  negative-index slices;
* ``enhance_space`` / ``enhance_time``: the two "simple enhancing" functions
  (batch_queues/utilities.py:12-54, :106-173) through the same
  ``scipy.ndimage.zoom`` and ``scipy.interpolate.interp1d`` calls;
* ``make_output``: the six ``QueueMom*.make_output`` rules (:169-288), given
  the first-moment model's output where a rule needs it.

Everything is computed in float32, as the reference does on float32 batches;
the linear time mode goes through ``interp1d`` in float64 and is cast to
float32 afterwards, as the reference casts it."""
import numpy as np
from scipy.interpolate import interp1d
from scipy.ndimage import zoom

KINDS = ('Mom1', 'Mom1SF', 'Mom2', 'Mom2Sep', 'Mom2SF', 'Mom2SepSF')
# what each rule is made of: (subtract enhanced low-res, subtract the first
# moment, square)
PARTS = {'Mom1': (False, False, False), 'Mom1SF': (True, False, False),
         'Mom2': (False, True, True), 'Mom2Sep': (False, False, True),
         'Mom2SF': (True, True, True), 'Mom2SepSF': (True, False, True)}


def make_mask(shape, s_padding=0, t_padding=0, end_t_padding=False,
              t_enhance=1, dtype=np.float32):
    mask = np.zeros(shape, dtype=dtype)
    s_stop = -s_padding if s_padding else None
    t_stop = -t_padding if t_padding else None
    if end_t_padding and t_enhance > 1:
        t_stop = 1 - t_enhance if t_stop is None \
            else 1 - t_enhance - t_padding
    if len(shape) == 4:
        mask[:, s_padding:s_stop, s_padding:s_stop, :] = 1.0
    elif len(shape) == 5:
        mask[:, s_padding:s_stop, s_padding:s_stop, t_padding:t_stop, :] = 1.0
    return mask


def enhance_space(data, s_enhance):
    """nearest-neighbour blow-up of the two spatial axes of a 4-D / 5-D batch"""
    if s_enhance in (None, 1):
        return data
    if data.ndim not in (4, 5):
        raise ValueError('Data must be 3D, 4D, or 5D to do spatial enhancing, '
                         f'but received: {data.shape}')
    factors = [1, s_enhance, s_enhance] + [1] * (data.ndim - 3)
    return zoom(data, factors, order=0, mode='nearest', grid_mode=True)


def enhance_time(data, t_enhance, mode='constant'):
    """blow-up of the time axis of a 5-D batch: a repeat ('constant') or the
    line through neighbouring time steps, continued past the last ('linear')"""
    if t_enhance in (None, 1):
        return data
    if data.ndim != 5:
        raise ValueError('Data must be 5D to do temporal enhancing, but '
                         f'received: {data.shape}')
    if mode == 'constant':
        return zoom(data, [1, 1, 1, t_enhance, 1], order=0, mode='nearest',
                    grid_mode=True)
    assert mode == 'linear', mode
    t_hr = np.arange(data.shape[3] * t_enhance)
    f = interp1d(t_hr[::t_enhance], data, axis=3, fill_value='extrapolate')
    return np.array(f(t_hr), dtype=np.float32)


def enhanced_lr(lr, s_enhance, t_enhance, mode, hr_features_ind):
    out = enhance_time(enhance_space(lr, s_enhance), t_enhance, mode)
    return out[..., list(hr_features_ind)]


def combine(hr, gen):
    """the generator's output with the truth's trailing channels behind it
    (``_combine_loss_input``)"""
    extra = hr.shape[-1] - gen.shape[-1]
    if extra <= 0:
        return gen
    return np.concatenate([gen, hr[..., -extra:]], axis=-1)


def make_output(kind, lr, hr, s_enhance, t_enhance, mode='constant',
                hr_features_ind=None, mom1=None):
    """``Queue<kind>.make_output((lr, hr))``; ``mom1`` = the first-moment
    model's output for the rules that use it"""
    lr, hr = np.asarray(lr, np.float32), np.asarray(hr, np.float32)
    ind = list(range(hr.shape[-1])) if hr_features_ind is None \
        else hr_features_ind

    def sf():
        return hr - enhanced_lr(lr, s_enhance, t_enhance, mode, ind)
    if kind == 'Mom1':
        return hr
    if kind == 'Mom1SF':
        return sf()
    if kind == 'Mom2Sep':
        return hr ** 2
    if kind == 'Mom2SepSF':
        return sf() ** 2
    first = combine(hr, np.asarray(mom1, np.float32))
    if kind == 'Mom2':
        return (hr - first) ** 2
    if kind == 'Mom2SF':
        return (sf() - first) ** 2
    raise KeyError(kind)


def target(s_enhance, t_enhance, hr_features_ind):
    """a host stand-in for ``DeviceCondMomTarget`` (same call signature), made
    of the functions above: what the CPU tests inject as ``target=``"""
    def f(hr, lr=None, mom1=None, subfilter=False, square=False,
          mode='constant', box=None, output=True):
        hr = np.asarray(hr, np.float32)
        out = mask = None
        if output:
            out = hr
            if subfilter:
                te = t_enhance if hr.ndim == 5 else 1
                out = out - enhanced_lr(np.asarray(lr, np.float32), s_enhance,
                                        te, mode, hr_features_ind)
            if mom1 is not None:
                out = out - combine(hr, np.asarray(mom1, np.float32))
            if square:
                out = out ** 2
        if box is not None:
            s_pad, t_lo, t_hi = box
            mask = np.zeros(hr.shape, np.float32)
            sl = slice(s_pad, hr.shape[1] - s_pad), \
                slice(s_pad, hr.shape[2] - s_pad)
            if hr.ndim == 4:
                mask[:, sl[0], sl[1], :] = 1.0
            else:
                mask[:, sl[0], sl[1], t_lo:t_hi, :] = 1.0
        return out, mask
    return f
