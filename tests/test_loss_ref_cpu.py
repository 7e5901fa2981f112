"""Pins tests/loss_ref.py (the float64 restatement the GPU cases of
tests/test_loss_kernels_gpu.py compare with) on the CPU, three ways: against
oracle/losses.py by composing map -> MAE / MSE -> value, by
``<F x, y> = <x, F^T y>`` for the linear maps, and against torch autograd /
central differences for the rest.  The last tests evaluate, with numpy normal
draws standing in for the device's directions, the two conditions that keep
the sliced-Wasserstein GPU cases from hiding a failure."""
import numpy as np
import pytest

from oracle import losses as OL
from tests import loss_ref as R

SHAPE = (2, 5, 4, 6, 3)


def _x(seed, shape=SHAPE):
    return np.random.default_rng(seed).standard_normal(shape)


# ------------------------------------------------------------ against the oracle
@pytest.mark.parametrize('kind,name', [(R.DERIV_S, 'SpatialDerivativeLoss'),
                                       (R.DERIV_T, 'TemporalDerivativeLoss'),
                                       (R.MATERIAL, 'MaterialDerivativeLoss'),
                                       (R.MEAN_S, 'CoarseMseLoss'),
                                       (R.EXT_S, 'SpatialExtremesLoss'),
                                       (R.EXT_T, 'TemporalExtremesLoss')])
def test_maps_compose_to_the_oracle_losses(kind, name):
    a, b = _x(1), _x(2)
    cu = 2
    fa, fb = R.lossmap_fwd(kind, a, cu), R.lossmap_fwd(kind, b, cu)
    if kind == R.MEAN_S:
        val = OL.mse(fa, fb)
    elif kind in (R.EXT_S, R.EXT_T):
        val = (OL.mae(fa[0], fb[0]) + OL.mae(fa[1], fb[1])) / 2
    else:
        val = OL.mae(fa, fb)
    assert np.isclose(val, OL.LOSSES[name](a[..., :cu], b[..., :cu]), rtol=1e-13)


def test_deriv_s_on_a_4d_batch_is_the_oracle():
    a, b = _x(3, (2, 5, 4, 1, 3)), _x(4, (2, 5, 4, 1, 3))
    val = OL.mae(R.lossmap_fwd(R.DERIV_S, a, 3), R.lossmap_fwd(R.DERIV_S, b, 3))
    assert np.isclose(val, OL.spatial_derivative_loss(a[:, :, :, 0], b[:, :, :, 0]), rtol=1e-13)


@pytest.mark.parametrize('s,te,method', [(1, 2, 'average'), (2, 1, 'average'), (2, 3, 'subsample'),
                                         (2, 3, 'average')])
def test_coarsen_composes_to_the_low_res_loss(s, te, method):
    a, b = _x(5, (2, 4, 6, 6, 3)), _x(6, (2, 4, 6, 6, 3))
    m = R.TC_AVERAGE if method == 'average' else R.TC_SUBSAMPLE
    val = OL.mse(R.coarsen(a, s, te, m), R.coarsen(b, s, te, m))
    assert np.isclose(val, OL.low_res_loss(a, b, s_enhance=s, t_enhance=te, t_method=method), rtol=1e-13)


def test_mmd_value_is_the_oracle():
    a, b = _x(7), _x(8)
    for sigma in (0.5, 1.0, 3.0):
        val, _ = R.mmd(a.reshape(2, -1, 3), b.reshape(2, -1, 3), 3, sigma, 1.0)
        assert np.isclose(val, OL.mmd_loss(a, b, sigma), rtol=1e-12)


def test_sliced_wasserstein_value_is_the_oracle():
    a, b = _x(9), _x(10)
    dirs = np.random.default_rng(11).standard_normal((17, 5 * 4 * 6))
    val, _ = R.sliced_wasserstein(a.reshape(2, -1, 3), b.reshape(2, -1, 3), dirs, 3, 1.0)
    assert np.isclose(val, OL.sliced_wasserstein_loss(a, b, dirs), rtol=1e-12)


@pytest.mark.parametrize('mode3d', [0, 1])
def test_dft_and_specmap_compose_to_the_fft_losses(mode3d):
    shape = (2, 5, 4, 6, 3) if mode3d else (2, 5, 4, 1, 3)
    a, b = _x(12, shape), _x(13, shape)
    n, s1, s2, t, c = shape

    def fmap(x):
        z = x.astype(np.complex128)
        for outer, ln, inner in [(n, s1, s2 * t * c), (n * s1, s2, t * c)] + ([(n * s1 * s2, t, c)] if mode3d else []):
            z = R.dft_axis(z.real, z.imag, outer, ln, inner, -1)
        z = z.reshape(shape)
        return R.specmap_fwd(z.real, z.imag, mode3d)
    if mode3d:
        want = OL.spatiotemporal_fft_loss(a, b)
    else:
        want = OL.spatial_fft_loss(a[:, :, :, 0], b[:, :, :, 0])
    assert np.isclose(OL.mae(fmap(a), fmap(b)), want, rtol=1e-11)


def test_dft_axis_is_numpy_fft():
    z = _x(14, (3, 37, 5)) + 1j * _x(15, (3, 37, 5))
    assert np.allclose(R.dft_axis(z.real, z.imag, 3, 37, 5, -1), np.fft.fft(z, axis=1), atol=1e-12)
    assert np.allclose(R.dft_axis(z.real, z.imag, 3, 37, 5, +1), np.fft.ifft(z, axis=1) * 37, atol=1e-12)
    assert np.allclose(R.dft_axis(z.real, None, 3, 37, 5, -1), np.fft.fft(z.real, axis=1), atol=1e-12)


def test_time_windows_are_slices():
    full = _x(16, (7, 9, 3))
    assert np.array_equal(R.time_window(full, 2, 4), full[:, 2:6])
    assert np.allclose(R.time_mean(full, 2, 4), full[:, 2:6].mean(axis=1), rtol=1e-15)


# ------------------------------------------------------------ <F x, y> = <x, F^T y>
@pytest.mark.parametrize('shape', [(2, 2, 3, 2, 3), (1, 3, 2, 3, 2), (2, 5, 4, 6, 3)])
@pytest.mark.parametrize('kind', [R.DERIV_S, R.DERIV_T, R.MEAN_S])
def test_linear_maps_and_their_adjoints(kind, shape):
    cu = shape[-1] - 1
    x = _x(20, shape)
    fx = R.lossmap_fwd(kind, x, cu)
    y = _x(21, fx.shape)
    adj = R.lossmap_adjoint(kind, x, y, cu)
    assert np.all(adj[..., cu:] == 0)
    assert np.isclose((fx * y).sum(), (x * adj).sum(), rtol=1e-12)


@pytest.mark.parametrize('s,te,method', [(1, 2, R.TC_AVERAGE), (2, 1, R.TC_SUBSAMPLE), (2, 3, R.TC_SUBSAMPLE),
                                         (2, 3, R.TC_AVERAGE), (4, 2, R.TC_AVERAGE)])
def test_coarsen_and_its_adjoint(s, te, method):
    x = _x(22, (2, 4, 8, 6, 3))
    fx = R.coarsen(x, s, te, method)
    y = _x(23, fx.shape)
    adj = R.lossmap_adjoint(R.COARSEN, x, y, 2, (s, te, method))
    assert np.all(adj[..., 2:] == 0)
    assert np.isclose((fx * y)[..., :2].sum(), (x * adj).sum(), rtol=1e-12)


def test_time_windows_and_their_adjoints():
    full = _x(24, (7, 9, 3))
    for t0, ln in [(0, 1), (0, 9), (2, 4), (5, 4)]:
        w, m = R.time_window(full, t0, ln), R.time_mean(full, t0, ln)
        yw, ym = _x(25, w.shape), _x(26, m.shape)
        assert np.isclose(0.5 * (w * yw).sum(), (full * R.time_window_adjoint(yw, 9, t0, ln, 0.5)).sum(), rtol=1e-12)
        assert np.isclose(0.5 * (m * ym).sum(), (full * R.time_mean_adjoint(ym, 9, t0, ln, 0.5)).sum(), rtol=1e-12)


def test_dft_adjoint_is_the_other_sign():
    x = _x(27, (3, 37, 5)) + 1j * _x(28, (3, 37, 5))
    y = _x(29, (3, 37, 5)) + 1j * _x(30, (3, 37, 5))
    fx = R.dft_axis(x.real, x.imag, 3, 37, 5, -1)
    fy = R.dft_axis(y.real, y.imag, 3, 37, 5, +1)
    assert np.isclose(np.vdot(y, fx), np.vdot(fy, x), rtol=1e-12)


def test_derivative_matrix_rows():
    assert np.array_equal(R.derivative_matrix(2), [[-1, 1], [-1, 1]])
    assert np.array_equal(R.derivative_matrix(3), [[-1, 1, 0], [-.5, 0, .5], [0, -1, 1]])
    x = _x(31, (7, 3))
    assert np.allclose(R.derivative_rows(x), np.gradient(x, axis=0), rtol=1e-14)


# ------------------------------------------------------------ autograd / differences
def _central(f, x, d, h=1e-6):
    return (f(x + h * d) - f(x - h * d)) / (2 * h)


@pytest.mark.parametrize('kind', [R.MATERIAL, R.EXT_S, R.EXT_T])
def test_nonlinear_adjoints_against_central_differences(kind):
    cu = 3 if kind == R.MATERIAL else 2      # material: channel 2 has no partner and stays out
    x = _x(40)
    g = _x(41, R.lossmap_fwd(kind, x, cu).shape)
    adj = R.lossmap_adjoint(kind, x, g, cu)
    assert np.all(adj[..., cu:] == 0)
    if kind == R.MATERIAL:
        assert np.all(adj[..., 2] == 0)
    for seed in (42, 43, 44):
        d = _x(seed)
        num = _central(lambda v: (R.lossmap_fwd(kind, v, cu) * g).sum(), x, d)
        assert np.isclose(num, (adj * d).sum(), rtol=1e-6, atol=1e-8)


def test_extremes_share_a_tie_equally():
    x = np.zeros((1, 2, 3, 4, 2))
    x[0, 0, 0, 1, 0] = x[0, 1, 2, 1, 0] = -1.0         # two-way minimum of (n 0, t 1, ch 0)
    g = np.arange(2 * 1 * 4 * 2, dtype=np.float64).reshape(2, 1, 4, 2) + 1
    adj = R.lossmap_adjoint(R.EXT_S, x, g, 2)
    assert adj[0, 0, 0, 1, 0] == adj[0, 1, 2, 1, 0] == g[0, 0, 1, 0] / 2
    assert np.allclose(adj[0, :, :, 1, 0].sum(), g[0, 0, 1, 0] + g[1, 0, 1, 0])
    # a constant slice: all six share both gradients
    assert np.allclose(adj[0, :, :, 0, 1], (g[0, 0, 0, 1] + g[1, 0, 0, 1]) / 6)
    cnt = R.extremes_counts(x, 2, True)
    assert cnt[0, 0, 1, 0] == 2 and cnt[1, 0, 1, 0] == 4 and cnt[0, 0, 0, 1] == 6
    xt = np.zeros((1, 1, 2, 1, 1))
    adj = R.lossmap_adjoint(R.EXT_T, xt, np.array([3.0, 4.0, 5.0, 6.0]).reshape(2, 1, 1, 2, 1), 1)
    assert np.array_equal(adj.ravel(), [8.0, 10.0])     # t = 1: min and max at once


@pytest.mark.parametrize('mode3d', [0, 1])
def test_specmap_gradient_is_the_closed_form(mode3d):
    re, im = _x(50), _x(51)
    re[0, 2, 2, 3, 1] = im[0, 2, 2, 3, 1] = 0.0          # |X| = 0: gradient 0, not NaN
    g = _x(52)
    gr, gi = R.specmap_bwd(re, im, g, mode3d)
    w = R.spec_weights(5, 4, 6, mode3d)
    mag = np.hypot(re, im)
    with np.errstate(invalid='ignore', divide='ignore'):
        f = np.where(mag > 0, g * w / ((1 + w * mag) * mag), 0.0)
    assert np.allclose(gr, f * re, rtol=1e-12, atol=0) and np.allclose(gi, f * im, rtol=1e-12, atol=0)
    assert gr[0, 2, 2, 3, 1] == 0 and gi[0, 2, 2, 3, 1] == 0
    assert np.all(gr[:, 0] == 0) and np.all(gr[:, :, 0] == 0)       # w = 0 rows
    assert np.all(R.specmap_fwd_bound(re, im, mode3d) >= 0)


def test_mmd_terms_sum_to_the_autograd_gradient():
    rng = np.random.default_rng(60)
    a, b = rng.standard_normal((5, 7, 4)), rng.standard_normal((5, 7, 5))
    for sigma in (0.5, 3.0):
        val, d = R.mmd(a, b, 3, sigma, 0.75)
        _, (t1, t2), _ = R.mmd_terms(a, b, 3, sigma, 0.75)
        assert np.allclose((t1 + t2).sum(axis=1), d[..., :3], rtol=1e-11, atol=1e-15)
        assert np.all(d[..., 3:] == 0)
        vb, gb = R.mmd_bounds(a, b, 3, sigma, 0.75, np.ones_like(a), 300)
        assert 0 < vb < 1e-4 and gb.shape == a.shape and np.all(gb > 0)
    val, d = R.mmd(a, a[..., :4], 3, 1.0, 1.0)
    assert abs(val) < 1e-15 and np.abs(d).max() < 1e-16


def test_sw_bound_reference_is_the_autograd_gradient():
    rng = np.random.default_rng(61)
    a, b = rng.standard_normal((3, 29, 4)), rng.standard_normal((3, 29, 4))
    dirs = rng.standard_normal((17, 29))
    for bb in (b, np.zeros_like(b)):
        val, d = R.sliced_wasserstein(a, bb, dirs, 3, 0.5)
        vb, gb, full = R.sw_bounds(a, bb, dirs, 3, 0.5, np.zeros_like(a))
        assert np.allclose(full, d, rtol=1e-10, atol=1e-15)
        assert np.all(gb[..., :3] > 0) and vb > 0


# ------------------------------------------------------------ the two SW conditions
@pytest.mark.parametrize('case', R.SW_ZERO_TRUTH[1:], ids=lambda c: f'{c[0]}x{c[1]}x{c[2] * c[3]}')
def test_sw_zero_truth_bound_stays_below_a_dropped_projection(case):
    """largest bound of the case < RMS of its reference gradient / (4 sqrt(n_proj))"""
    n_proj, n_pos, n, cu, nnz = case
    a = R.sw_zero_truth_field(n_pos, n, nnz, cu)
    dirs = np.random.default_rng(71).standard_normal((n_proj, n_pos)).astype(np.float32)
    _, gb, ref = R.sw_bounds(a, np.zeros_like(a), dirs, cu, 1.0, np.zeros_like(a))
    rms = np.sqrt((ref ** 2).mean())
    print('largest bound / RMS', gb.max() / rms, 'limit', 1 / (4 * np.sqrt(n_proj)))
    assert gb.max() / rms < 1 / (4 * np.sqrt(n_proj))


def test_sw_general_truth_gap_condition_can_hold():
    """(17, 61, 33): for most draws the smallest gap between adjacent sorted
    projections exceeds the two error bounds; the GPU case asserts it for the
    device's own directions"""
    ok = 0
    for seed in range(4):
        rng = np.random.default_rng(80 + seed)
        a, b = rng.standard_normal((11, 61, 4)), rng.standard_normal((11, 61, 4))
        dirs = rng.standard_normal((17, 61)).astype(np.float32)
        ratio = min(R.sw_min_gap_ratio(a, dirs, 3), R.sw_min_gap_ratio(b, dirs, 3))
        print('seed', seed, 'gap / error bounds', ratio)
        ok += ratio > 1
    assert ok >= 2
