"""Conditional-moment batch queues on the device: ``s3_condmom_target``
against the numpy / scipy restatement (tests/condmom_ref.py), the 2nd-moment
queues with a real first-moment model, and the reference's training procedure
(tests/training/test_train_conditional.py) over its 16 parametrisations."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import condmom_ref as R
from tests.test_batch_queue import DummySampler
from tests.test_condmom_queue_cpu import IDS, PARAMS

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), '..', 'sup3r_amd', 'configs')
ST_GEN = os.path.join(CFG, 'gen_3x_4x_2f.json')
S_GEN = os.path.join(CFG, 'gen_2x_2f.json')
TOPO_GEN = os.path.join(CFG, 'test_gen_st_3x_4x_2f_topo.json')
FEATURES = ['u_100m', 'v_100m']

# hr shape, lr channels, lr channel of each hr channel, s_enhance, t_enhance
CASES = {'st_map': ((3, 9, 15, 12, 2), 3, [0, 2], 3, 4),
         's_2x': ((5, 10, 14, 1), 1, [0], 2, 1),
         's_5x_tail': ((2, 35, 35, 3), 3, [0, 1, 2], 5, 1)}


def _lr_shape(hr_shape, c_lr, s, te):
    mid = (hr_shape[3] // te,) if len(hr_shape) == 5 else ()
    return (hr_shape[0], hr_shape[1] // s, hr_shape[2] // s) + mid + (c_lr,)


def _kernel(hr, lr, mom1, ind, s, te, kind, mode, box):
    """one ``s3_condmom_target`` call into NaN-filled tensors"""
    import torch
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    dev, L = Device.get(), _lib.lib()
    sub, first, square = R.PARTS[kind]
    flags = (_lib.CM_SUBFILTER * sub | _lib.CM_MOM1 * first
             | _lib.CM_SQUARE * square
             | _lib.CM_LINEAR * (sub and mode == 'linear'))
    hr_d, lr_d = dev.to_device(hr), dev.to_device(lr)
    m_d = dev.to_device(mom1) if first else None
    out = torch.full(hr.shape, float('nan'), dtype=torch.float32,
                     device=hr_d.device)
    mask = torch.full_like(out, float('nan')) if box is not None else None
    is_5d = hr.ndim == 5
    t = hr.shape[3] if is_5d else 1

    def ptr(x):
        return None if x is None else C.c_void_p(x.data_ptr())
    s_pad, t_lo, t_hi = box if box is not None else (0, 0, t)
    rc = L.s3_condmom_target(
        dev.ctx, ptr(hr_d), ptr(lr_d), ptr(m_d), hr.shape[0], hr.shape[1],
        hr.shape[2], t, hr.shape[-1], lr.shape[-1],
        mom1.shape[-1] if first else 0, (C.c_int32 * len(ind))(*ind), s,
        te if is_5d else 1, flags, s_pad, t_lo, t_hi, ptr(out), ptr(mask))
    _lib.check(rc, dev.ctx, 's3_condmom_target')
    dev.sync()
    return out.cpu().numpy(), None if mask is None else mask.cpu().numpy()


@pytest.mark.parametrize('with_mask', [False, True], ids=['out', 'out+mask'])
@pytest.mark.parametrize('mode', ['constant', 'linear'])
@pytest.mark.parametrize('kind', R.KINDS[1:])
@pytest.mark.parametrize('case', list(CASES))
def test_kernel_matches_the_restatement(case, kind, mode, with_mask):
    from sup3r_amd.batch_queue_conditional import mask_box
    hr_shape, c_lr, ind, s, te = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case + kind + mode)))
    hr = rng.standard_normal(hr_shape).astype(np.float32)
    lr = (3 * rng.standard_normal(_lr_shape(hr_shape, c_lr, s, te))
          ).astype(np.float32)
    # the first moment with all the hi-res channels, or (where there are
    # several) without the last: that one then comes from the truth
    c_m = hr_shape[-1] - (1 if hr_shape[-1] > 1 and with_mask else 0)
    mom1 = rng.standard_normal(hr_shape[:-1] + (c_m,)).astype(np.float32)
    box = mask_box(hr_shape, 1, 2, True, te) if with_mask else None
    out, mask = _kernel(hr, lr, mom1, ind, s, te, kind, mode, box)
    assert not np.isnan(out).any()
    want = R.make_output(kind, lr, hr, s, te, mode, ind, mom1=mom1)
    sub, first, square = R.PARTS[kind]
    if with_mask:
        assert not np.isnan(mask).any()
        np.testing.assert_array_equal(
            mask, R.make_mask(hr_shape, 1, 2, True, te))
    if first and c_m < hr_shape[-1]:
        # hr - hr on the channel the truth stands in for
        base = hr[..., -1] - R.enhanced_lr(lr, s, te, mode, ind)[..., -1] \
            if sub else hr[..., -1]
        np.testing.assert_array_equal(want[..., -1], (base - hr[..., -1]) ** 2)
    if not (sub and mode == 'linear' and te > 1):
        np.testing.assert_array_equal(out, want)
        return
    # linear mode: fp32 lo + (hi - lo) * frac on the device against scipy's
    # float64 evaluation cast to fp32: three fp32 roundings of magnitudes
    # <= 4 max|lr| in extrapolation plus scipy's cast
    delta = 16 * 2.0 ** -24 * float(np.abs(lr).max())
    if not square:
        err, bound = np.abs(out - want).max(), delta
    else:
        unsq = R.make_output('Mom1SF', lr, hr, s, te, mode, ind)
        if first:
            unsq = unsq - R.combine(hr, mom1)
        bound = 2 * float(np.abs(unsq).max()) * delta + delta ** 2
        err = np.abs(out - want).max()
    print(f'{case} {kind} linear: max err {err:.3e}, bound {bound:.3e}')
    assert err <= bound


def test_mask_only_call_and_target_wrapper():
    """``output=False``: only the mask is written; the wrapper's tensors are
    device tensors"""
    import torch
    from sup3r_amd.batch_queue_conditional import (DeviceCondMomTarget,
                                                   mask_box)
    hr = np.random.default_rng(0).standard_normal(
        (2, 6, 9, 8, 3)).astype(np.float32)
    tgt = DeviceCondMomTarget(3, 4, [0, 1, 2])
    for pads in ((0, 0, False), (1, 1, False), (2, 3, True), (3, 0, True)):
        out, mask = tgt(hr, box=mask_box(hr.shape, *pads, 4), output=False)
        assert out is None and isinstance(mask, torch.Tensor) and mask.is_cuda
        np.testing.assert_array_equal(mask.cpu().numpy(),
                                      R.make_mask(hr.shape, *pads, 4))
    out, mask = tgt(hr, square=True)
    assert mask is None
    np.testing.assert_array_equal(out.cpu().numpy(), hr ** 2)


def test_kernel_refuses_bad_arguments():
    hr = np.zeros((2, 6, 6, 8, 2), np.float32)
    lr = np.zeros((2, 2, 2, 2, 2), np.float32)

    def call(hr=hr, lr=lr, mom1=hr, ind=(0, 1), s=3, te=4, kind='Mom2SF',
             mode='constant'):
        return _kernel(hr, lr, mom1, list(ind), s, te, kind, mode, None)
    call()
    with pytest.raises(RuntimeError, match='s_enhance must evenly divide'):
        call(s=4)
    with pytest.raises(RuntimeError, match='t_enhance must evenly divide'):
        call(te=3)
    with pytest.raises(RuntimeError, match='more channels'):
        call(mom1=np.zeros((2, 6, 6, 8, 3), np.float32))
    with pytest.raises(RuntimeError, match='channel map'):
        call(ind=(0, 2))
    with pytest.raises(RuntimeError, match='channel map'):
        call(ind=(-1, 0))
    with pytest.raises(RuntimeError, match='two low-res time steps'):
        call(hr=np.zeros((2, 6, 6, 4, 2), np.float32),
             lr=np.zeros((2, 2, 2, 1, 2), np.float32),
             mom1=np.zeros((2, 6, 6, 4, 2), np.float32), mode='linear')


# ------------------------------------------- queues with a real lower model
def _model(fp_gen, seed=0):
    from sup3r_amd import Sup3rCondMom
    Sup3rCondMom.seed(seed)
    return Sup3rCondMom(fp_gen, learning_rate=1e-4)


@pytest.mark.parametrize('kind', ['Mom2', 'Mom2SF'])
@pytest.mark.parametrize('fp_gen, sample_shape, s, te', [
    (ST_GEN, (12, 12, 16), 3, 4), (S_GEN, (12, 12, 1), 2, 1)],
    ids=['st', 's'])
def test_second_moment_queue_with_a_real_first_moment_model(
        kind, fp_gen, sample_shape, s, te):
    import torch
    from sup3r_amd import batch_queue_conditional as Q
    mom1 = _model(fp_gen)
    samplers = [DummySampler(sample_shape, (20, 20, 30), 2, FEATURES, seed=4)]
    q = getattr(Q, 'Queue' + kind)(
        samplers, batch_size=2, n_batches=3, s_enhance=s, t_enhance=te,
        queue_cap=2, lower_models={1: mom1}, s_padding=1, seed=0)
    got = list(q)
    q.stop()
    assert not q.queue_thread.is_alive()
    assert len(got) == 3
    squeeze = sample_shape[2] == 1
    for b, raw in zip(got, samplers[0].drawn):
        raw = raw[..., 0, :] if squeeze else raw
        for member in b:
            assert isinstance(member, torch.Tensor) and member.is_cuda
        np.testing.assert_array_equal(b.high_res.cpu().numpy(), raw)
        gen = mom1._tf_generate(b.low_res, mom1.get_hr_exo_input(b.high_res))
        assert tuple(gen.shape) == raw.shape
        want = R.make_output(kind, b.low_res.cpu().numpy(), raw, s, te,
                             'constant', [0, 1], mom1=gen.cpu().numpy())
        np.testing.assert_array_equal(b.output.cpu().numpy(), want)
        assert float(np.abs(want).max()) > 0
        np.testing.assert_array_equal(
            b.mask.cpu().numpy(), R.make_mask(raw.shape, 1, 0, False, te))
        assert b.mask is got[0].mask


@pytest.mark.parametrize('kind', ['Mom2', 'Mom2SF'])
def test_second_moment_queue_with_a_hi_res_exo_channel(kind):
    """the arrangement of tests/training/test_train_conditional_exo.py:
    topography is a low-res input AND, at hi-res, the trailing channel of the
    truth that feeds the generator's Sup3rConcat layer; the first-moment model
    writes (u, v) only, so on the topography channel the first moment is the
    truth itself"""
    from sup3r_amd import batch_queue_conditional as Q
    feats = FEATURES + ['topography']
    mom1 = _model(TOPO_GEN)
    assert mom1.hr_exo_features == ['topography']

    class Smp(DummySampler):
        lr_features = feats
        hr_features = feats
        hr_out_features = feats[:2]
        hr_exo_features = feats[2:]
        hr_features_ind = [0, 1, 2]

    samplers = [Smp((12, 12, 16), (20, 20, 30), 2, feats, seed=6)]
    q = getattr(Q, 'Queue' + kind)(
        samplers, batch_size=2, n_batches=2, s_enhance=3, t_enhance=4,
        queue_cap=2, lower_models={1: mom1}, seed=0)
    got = list(q)
    q.stop()
    for b, raw in zip(got, samplers[0].drawn):
        exo = mom1.get_hr_exo_input(b.high_res)
        assert list(exo) == ['topography']
        np.testing.assert_array_equal(exo['topography'].cpu().numpy(),
                                      raw[..., 2:])
        gen = mom1._tf_generate(b.low_res, exo)
        assert tuple(gen.shape) == raw.shape[:-1] + (2,)
        joined = mom1._combine_loss_input(b.high_res, gen).cpu().numpy()
        np.testing.assert_array_equal(joined, R.combine(raw, gen.cpu().numpy()))
        lr = b.low_res.cpu().numpy()
        want = R.make_output(kind, lr, raw, 3, 4, 'constant', [0, 1, 2],
                             mom1=gen.cpu().numpy())
        out = b.output.cpu().numpy()
        np.testing.assert_array_equal(out, want)
        sf = raw[..., 2] - np.repeat(np.repeat(np.repeat(
            lr[..., 2], 3, 1), 3, 2), 4, 3) if kind == 'Mom2SF' else raw[..., 2]
        np.testing.assert_array_equal(out[..., 2], (sf - raw[..., 2]) ** 2)


# ------------------------------------------ the reference's training procedure
@pytest.mark.parametrize(
    'end_t_padding, mode, kind, sample_shape, s_enhance, t_enhance', PARAMS,
    ids=IDS)
def test_train_conditional(tmp_path, end_t_padding, mode, kind, sample_shape,
                           s_enhance, t_enhance):
    from sup3r_amd import Sup3rCondMom
    from sup3r_amd import batch_queue_conditional as Q
    fp_gen = ST_GEN if sample_shape[2] > 1 else S_GEN
    Sup3rCondMom.seed()
    model = Sup3rCondMom(fp_gen, learning_rate=1e-4)
    model_mom1 = Sup3rCondMom(fp_gen, learning_rate=1e-4)
    train = [DummySampler(sample_shape, (20, 20, 40), 2, FEATURES, seed=1)]
    val = [DummySampler(sample_shape, (20, 20, 40), 2, FEATURES, seed=2)]
    bh = getattr(Q, 'BatchHandler' + kind)(
        train, val, batch_size=2, s_enhance=s_enhance, t_enhance=t_enhance,
        n_batches=2, lower_models={1: model_mom1},
        end_t_padding=end_t_padding, time_enhance_mode=mode, seed=0)
    out_dir = os.path.join(str(tmp_path), 'test_{epoch}')
    model.train(bh, input_resolution={'spatial': '12km', 'temporal': '60min'},
                n_epoch=2, checkpoint_int=2, out_dir=out_dir)
    assert not bh.queue_thread.is_alive()
    assert not bh.val_data.queue_thread.is_alive()
    h = model.history
    assert len(h) == 2
    for col in ('train_loss_gen', 'val_loss_gen'):
        assert np.isfinite(np.asarray(h[col], dtype=np.float64)).all()
    # (epochs count from 0: the checkpoint of the last one)
    assert sorted(os.listdir(str(tmp_path))) == ['test_0', 'test_1']
    loaded = Sup3rCondMom.load(out_dir.format(epoch=1))
    lr_shape = (2, sample_shape[0] // s_enhance, sample_shape[1] // s_enhance
                ) + ((sample_shape[2] // t_enhance,)
                     if sample_shape[2] > 1 else ()) + (2,)
    x = np.random.default_rng(0).standard_normal(lr_shape).astype(np.float32)
    np.testing.assert_array_equal(loaded.generate(x), model.generate(x))
