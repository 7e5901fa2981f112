"""The structured content-loss kernels (sup3r_amd/csrc/kernels_loss.hip,
kernels_loss_sw.hip, kernels_time_window.hip and ``s3_coarsen``) element by
element, through the C ABI, at the edges of their loops — each against the
float64 restatement of the same call (tests/loss_ref.py, pinned on the CPU by
tests/test_loss_ref_cpu.py).

Exact cases: every input is k / 4 with |k| <= 32 and every ``g_out`` an integer
in [-4, 4], so no fp32 sum or product can round and the comparison is
``assert_array_equal``; each case asserts that proof (largest sum of absolute
terms in units of the granularity below 2^24).  Cases with one or two
roundings compare at 2^-22 of the sum of the absolute terms.  Bounded cases
use a per-element bound computed in float64 from the reference's own sums of
absolute terms (``loss_ref.*_bound``) and print the worst error / bound.

Every ``d_x`` is pre-filled with a non-zero dyadic pattern: the adjoints add,
and channels >= c_used keep their bits.  Grid-cap shapes come from the device's
CU count inside the test: collecting the file touches no device.  See
profiles/losses/NOTES.md."""
import ctypes as C

import numpy as np
import pytest

from tests import loss_ref as R

pytestmark = pytest.mark.gpu

EINVAL = -1
TOL2 = 2.0 ** -22            # one or two fp32 roundings, and the add into d_x


# ------------------------------------------------------------------ helpers
def _dev():
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    return Device.get(), _lib.lib(), _lib


def _cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _lds():
    """LDS a workgroup may declare: the property s3_ctx_create reads"""
    import torch
    return int(torch.cuda.get_device_properties(0).shared_memory_per_block)


def _up(a):
    return _dev()[0].to_device(np.ascontiguousarray(a, dtype=np.float32))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _ok(rc, what):
    dev, _, lib = _dev()
    lib.check(rc, dev.ctx, what)


def _q(rng, shape, amp=32):
    """k / 4, |k| <= amp"""
    return rng.integers(-amp, amp + 1, size=shape).astype(np.float64) / 4


def _g(rng, shape):
    return rng.integers(-4, 5, size=shape).astype(np.float64)


def _d0(shape, like=1.0):
    """non-zero dyadic pre-fill of a gradient buffer: multiples of 1 / 4, times
    the power of two nearest ``like`` (the size of the gradient to be added,
    so that the pre-fill does not swamp it)"""
    v = (np.arange(int(np.prod(shape))) % 7 - 3) / 4.0
    v[v == 0] = 1.25
    return v.reshape(shape) * 2.0 ** np.round(np.log2(like))


def _fits(abs_sum, gran):
    """the no-rounding proof: sums of absolute terms, in units of the terms'
    granularity, stay below 2^24"""
    assert np.max(abs_sum) / gran < 2 ** 24, 'an fp32 sum could round'


def _odd_pair(target):
    """(a, b), both odd, a * b >= target and as little above it as that allows"""
    a = int(np.ceil(np.sqrt(target))) | 1
    b = int(-(-target // a)) | 1
    return a, b


def _shape(case):
    return case(_cu()) if callable(case) else case


def _close2(got, ref, abs_terms, what):
    """within 2^-22 of the sum of the absolute terms, element by element"""
    err, tol = np.abs(got - ref), TOL2 * abs_terms
    print(f'{what}: worst error / (2^-22 sum |terms|) = {np.max(err / np.maximum(tol, 1e-300)):.3f}')
    assert np.all(err <= tol), what


def _lossmap_fwd(kind, x, cu, out_size, work_size=0):
    dev, L, _ = _dev()
    n, s1, s2, t, c = x.shape
    xd, out = _up(x), dev.empty((out_size,))
    work = _up(np.full(work_size, 1e30)) if work_size else None
    _ok(L.s3_lossmap_fwd(dev.ctx, kind, _p(xd), n, s1, s2, t, c, cu, 0, 0, 0, _p(out), _p(work)), 'lossmap_fwd')
    return _np(out), out


def _lossmap_bwd(kind, x, g, cu, fx=None, p=(0, 0, 0), work_size=0):
    """-> (d_x after the call, the pre-fill)"""
    dev, L, _ = _dev()
    n, s1, s2, t, c = x.shape
    d0 = _d0(x.shape)
    xd, gd, dx = _up(x), _up(np.ravel(g)), _up(d0)
    work = _up(np.full(work_size, 1e30)) if work_size else None
    _ok(L.s3_lossmap_bwd(dev.ctx, kind, _p(xd), _p(fx), _p(gd), n, s1, s2, t, c, cu, *p, _p(dx), _p(work)),
        'lossmap_bwd')
    return _np(dx), d0


# ================================================================ derivatives
def _cap(t, cu, c, extra=0):
    """(n, s1, s2, t, c, cu) with n s1 s2 t cu just above the 8 CU 256 elements
    one sweep of the capped grid covers; odd extents"""
    def make(ncu):
        a, b = _odd_pair(-(-(8 * ncu * 256 + 1) // (t * cu)) + extra)
        return (1, a, b, t, c, cu)
    return make


DERIV = [
    ('s_len2', R.DERIV_S, (2, 2, 2, 3, 3, 3)),
    ('s_len3', R.DERIV_S, (1, 3, 3, 2, 2, 2)),
    ('s_len5', R.DERIV_S, (2, 5, 5, 3, 3, 3)),
    ('s_len2x3', R.DERIV_S, (2, 2, 3, 5, 2, 2)),
    ('s_c5_used2', R.DERIV_S, (2, 3, 5, 2, 5, 2)),
    ('s_4d', R.DERIV_S, (3, 5, 4, 1, 3, 3)),
    ('s_above_cap', R.DERIV_S, _cap(3, 2, 3)),
    ('t_len2', R.DERIV_T, (2, 3, 2, 2, 3, 3)),
    ('t_len3', R.DERIV_T, (1, 2, 3, 3, 2, 2)),
    ('t_len5', R.DERIV_T, (2, 3, 3, 5, 3, 3)),
    ('t_c5_used2', R.DERIV_T, (2, 3, 2, 5, 5, 2)),
    ('t_above_cap', R.DERIV_T, _cap(3, 2, 3)),
]


@pytest.mark.parametrize('kind,case', [d[1:] for d in DERIV], ids=[d[0] for d in DERIV])
def test_derivative_maps_exact(kind, case):
    """DERIV_S / DERIV_T forward and adjoint: one-sided rows at both ends
    (length 2: nothing else), one central row (3), c_used < c, 4-D, and the
    grid-stride second pass"""
    *shape, cu = _shape(case)
    rng = np.random.default_rng(1)
    x = _q(rng, shape)
    ref = R.lossmap_fwd(kind, x, cu)
    _fits(4 * np.abs(x).max(), 0.125)                    # two stencils of two terms, halves of k / 4
    got, _ = _lossmap_fwd(kind, x, cu, ref.size)
    np.testing.assert_array_equal(got, ref.ravel())
    g = _g(rng, ref.shape)
    dx, d0 = _lossmap_bwd(kind, x, g, cu)
    _fits(np.abs(d0).max() + 4 * np.abs(g).max(), 0.125)    # at most four coefficients of size <= 1 each
    np.testing.assert_array_equal(dx, d0 + R.lossmap_adjoint(kind, x, g, cu))


# ================================================================ material derivative
MATERIAL = [
    ('s1_2', (2, 2, 3, 4, 2, 2)), ('s2_2', (2, 3, 2, 4, 2, 2)), ('t_2', (2, 3, 4, 2, 2, 2)),
    ('all_2', (1, 2, 2, 2, 2, 2)),
    ('c5_used2', (2, 3, 4, 3, 5, 2)), ('c5_used3', (2, 3, 4, 3, 5, 3)), ('c5_used4', (2, 3, 4, 3, 5, 4)),
    ('above_cap', _cap(3, 1, 3)),            # counted in (u, v) pairs: n s1 s2 t hub just above the cap
]


@pytest.mark.parametrize('case', [m[1] for m in MATERIAL], ids=[m[0] for m in MATERIAL])
def test_material_derivative_exact(case):
    """MATERIAL forward and adjoint; an odd c_used leaves its last channel
    alone, channels >= c_used keep their bits"""
    *shape, cu = _shape(case)
    if cu == 1:                     # the cap helper counted pairs: two channels per output element
        cu = 2
    hub = cu // 2
    rng = np.random.default_rng(2)
    x = _q(rng, shape, amp=16)
    ref = R.lossmap_fwd(R.MATERIAL, x, cu)
    assert ref.shape[-1] == hub
    xm = np.abs(x).max()
    _fits(2 * xm + 2 * xm * 2 * xm, 1 / 32)             # du/dt + u du/ds1 + v du/ds2: (k/4) (k/8)
    got, _ = _lossmap_fwd(R.MATERIAL, x, cu, ref.size)
    np.testing.assert_array_equal(got, ref.ravel())
    g = _g(rng, ref.shape)
    dx, d0 = _lossmap_bwd(R.MATERIAL, x, g, cu)
    gm = np.abs(g).max()
    _fits(np.abs(d0).max() + gm * (2 * xm + 2 + 4 * xm), 0.125)
    want = d0 + R.lossmap_adjoint(R.MATERIAL, x, g, cu)
    np.testing.assert_array_equal(dx, want)
    np.testing.assert_array_equal(dx[..., 2 * hub:], d0[..., 2 * hub:])


# ================================================================ spatial / temporal reductions
def _tied_field(rng, shape, cu, spatial, counts, amp=24):
    """k / 4 field whose minimum (-amp - 8) / 4 and maximum (amp + 8) / 4 are
    taken ``counts[i]`` times in column i (cyclic): the first and the last
    position of the reduced axis among the ties — of the minimum in even
    columns, of the maximum in odd ones — so that a two-way tie sits in two
    different slabs.  Channels >= cu hold the minimum everywhere: a kernel that read them would count them."""
    n, s1, s2, t, c = shape
    x = _q(rng, shape, amp)
    lo, hi = -(amp + 8) / 4, (amp + 8) / 4
    xu = x[..., :cu]
    v = (xu.transpose(0, 3, 4, 1, 2).reshape(-1, s1 * s2) if spatial
         else xu.transpose(0, 1, 2, 4, 3).reshape(-1, t)).copy()
    P = v.shape[1]
    cols = range(v.shape[0]) if v.shape[0] <= 4096 else list(range(512)) + list(range(v.shape[0] - 512, v.shape[0]))
    for i in cols:
        m_lo = min(counts[i % len(counts)], P // 2)
        m_hi = min(counts[(i // len(counts) + i) % len(counts)], P // 2)
        if P < 2:
            continue
        pool = [0, P - 1] + list(rng.permutation(np.arange(1, P - 1)))
        a_pos, b_pos = pool[:m_lo], pool[m_lo:m_lo + m_hi]
        if i % 2:
            a_pos, b_pos, m_lo, m_hi = b_pos, a_pos, m_hi, m_lo
        v[i, a_pos] = lo
        v[i, b_pos] = hi
    if spatial:
        xu = v.reshape(n, t, cu, s1, s2).transpose(0, 3, 4, 1, 2)
    else:
        xu = v.reshape(n, s1, s2, cu, t).transpose(0, 1, 2, 4, 3)
    x[..., :cu] = xu
    x[..., cu:] = lo
    return x


def _ext_sizes(shape, cu, spatial):
    n, s1, s2, t, c = shape
    ne = n * t * cu if spatial else n * s1 * s2 * cu
    return ne, (n * 64 * t * cu if spatial else 0)


def _extremes_case(shape, cu, spatial, x, exact):
    kind = R.EXT_S if spatial else R.EXT_T
    rng = np.random.default_rng(4)
    ne, slab = _ext_sizes(shape, cu, spatial)
    ref = R.lossmap_fwd(kind, x, cu)
    got, fx = _lossmap_fwd(kind, x, cu, 2 * ne, slab)
    np.testing.assert_array_equal(got, ref.ravel())                 # min / max never round
    g = _g(rng, ref.shape)
    g[g == 0] = 3
    dx, d0 = _lossmap_bwd(kind, x, g, cu, fx=fx, work_size=2 * ne + slab)
    adj = R.lossmap_adjoint(kind, x, g, cu)
    cnt = R.extremes_counts(x, cu, spatial)
    if exact:
        assert set(np.unique(cnt)) <= {1, 2, 4, 8, 16, 32, 64}, 'a tie count that is no power of two'
        _fits(np.abs(d0).max() + 2 * np.abs(g).max(), 1 / 64)
        np.testing.assert_array_equal(dx, d0 + adj)
    else:
        ax = (1, 2) if spatial else (3,)
        xu = x[..., :cu]
        terms = sum(np.where(xu == f(xu, axis=ax, keepdims=True), np.expand_dims(np.abs(g[q]) / cnt[q], ax), 0)
                    for q, f in ((0, np.min), (1, np.max)))
        full = np.abs(d0)
        full[..., :cu] += terms
        _close2(dx, d0 + adj, full, 'extremes adjoint')
        np.testing.assert_array_equal(dx[..., cu:], d0[..., cu:])
    return cnt


REDUCE_S = [   # (n, s1, s2, t, c, cu): s1 s2 in {1, 15, 64, 65}, t cu in {1, 260}, n in {1, 3}
    ('p1_tc1_n1', (1, 1, 1, 1, 2, 1)),
    ('p15_n3', (3, 3, 5, 2, 3, 2)),
    ('p64_n1', (1, 8, 8, 3, 2, 2)),
    ('p65_n3', (3, 5, 13, 2, 3, 3)),
    ('p15_tc260_n3', (3, 3, 5, 52, 6, 5)),
    ('p65_tc260_n1', (1, 13, 5, 65, 4, 4)),
    ('p1_tc260', (2, 1, 1, 65, 4, 4)),
]


@pytest.mark.parametrize('case', [r[1] for r in REDUCE_S], ids=[r[0] for r in REDUCE_S])
def test_spatial_extremes_exact(case):
    """EXT_S: empty slabs (s1 s2 < 64), a last slab of two (65), the j loop of
    reduce_s_stage1 (t c_used = 260); tie counts 1, 2, 4, the tied members in
    the first and the last slab"""
    *shape, cu = case
    x = _tied_field(np.random.default_rng(3), shape, cu, True, (1, 2, 4))
    cnt = _extremes_case(shape, cu, True, x, exact=True)
    if shape[1] * shape[2] >= 8:
        assert set(np.unique(cnt)) == {1, 2, 4}


@pytest.mark.parametrize('case', [(3, 3, 5, 2, 3, 2), (1, 13, 5, 3, 2, 2)], ids=['p15', 'p65'])
def test_spatial_extremes_tie_counts_3_and_5(case):
    *shape, cu = case
    x = _tied_field(np.random.default_rng(5), shape, cu, True, (3, 5))
    cnt = _extremes_case(shape, cu, True, x, exact=False)
    assert set(np.unique(cnt)) == {3, 5}


REDUCE_T = [
    ('t1_one_element', (1, 1, 1, 1, 2, 1)),
    ('t1', (3, 3, 5, 1, 3, 2)),            # every element is min and max at once and takes both gradients
    ('t5', (2, 3, 4, 5, 3, 2)),
    ('t8_n3', (3, 5, 3, 8, 4, 4)),
    ('above_cap', lambda ncu: (1,) + _odd_pair(8 * ncu * 256 // 2 + 1) + (2, 3, 2)),
]


@pytest.mark.parametrize('case', [r[1] for r in REDUCE_T], ids=[r[0] for r in REDUCE_T])
def test_temporal_extremes_exact(case):
    *shape, cu = _shape(case)
    counts = (1, 2, 4) if shape[3] >= 8 else (1, 2)
    x = _tied_field(np.random.default_rng(6), shape, cu, False, counts)
    _extremes_case(shape, cu, False, x, exact=True)


def test_temporal_extremes_tie_counts_3_and_5():
    shape, cu = (2, 3, 4, 11, 3), 2
    x = _tied_field(np.random.default_rng(7), shape, cu, False, (3, 5))
    cnt = _extremes_case(shape, cu, False, x, exact=False)
    assert set(np.unique(cnt)) == {3, 5}


@pytest.mark.parametrize('spatial', [True, False], ids=['spatial', 'temporal'])
def test_extremes_of_a_constant_field(spatial):
    """every element is tied at both extremes: 64 (4) share each gradient"""
    shape, cu = ((2, 8, 8, 2, 3), 2) if spatial else ((2, 3, 3, 4, 3), 2)
    x = np.full(shape, 0.75)
    cnt = _extremes_case(shape, cu, spatial, x, exact=True)
    assert np.all(cnt == (64 if spatial else 4))


@pytest.mark.parametrize('case', [r[1] for r in REDUCE_S] + [lambda ncu: (1,) + _odd_pair(8 * ncu * 256 + 1) + (1, 2, 1)],
                         ids=[r[0] for r in REDUCE_S] + ['above_cap'])
def test_spatial_mean(case):
    """MEAN_S forward and adjoint: the sum is exact, 1 / (s1 s2) and the
    product round unless s1 s2 is a power of two; then the add into d_x"""
    *shape, cu = _shape(case)
    n, s1, s2, t, c = shape
    rng = np.random.default_rng(8)
    x = _q(rng, shape, amp=8)
    ref = R.lossmap_fwd(R.MEAN_S, x, cu)
    _fits(np.abs(x[..., :cu]).sum(axis=(1, 2)), 0.25)
    got, _ = _lossmap_fwd(R.MEAN_S, x, cu, ref.size, n * 64 * t * cu)
    g = _g(rng, ref.shape)
    dx, d0 = _lossmap_bwd(R.MEAN_S, x, g, cu)
    want = d0 + R.lossmap_adjoint(R.MEAN_S, x, g, cu)
    pow2 = (s1 * s2) & (s1 * s2 - 1) == 0
    if pow2:
        np.testing.assert_array_equal(got, ref.ravel())
        np.testing.assert_array_equal(dx, want)
    else:
        _close2(got, ref.ravel(), np.abs(ref).ravel(), 'mean forward')
        _close2(dx, want, np.abs(d0) + np.abs(want - d0), 'mean adjoint')
    np.testing.assert_array_equal(dx[..., cu:], d0[..., cu:])


# ================================================================ coarsening
COARSEN = [(s, te, m) for s, te in ((1, 2), (2, 1), (2, 4), (4, 2)) for m in (R.TC_AVERAGE, R.TC_SUBSAMPLE)]


def _coarsen_case(shape, cu, s, te, method, exact):
    dev, L, _ = _dev()
    n, s1, s2, t, c = shape
    rng = np.random.default_rng(9)
    x = _q(rng, shape)
    ref = R.coarsen(x, s, te, method)
    xd, lr = _up(x), dev.empty((ref.size,))
    _ok(L.s3_coarsen(dev.ctx, _p(xd), n, s1, s2, t, c, s, te, method, _p(lr)), 's3_coarsen')
    g = _g(rng, ref.shape)                               # all c channels; those >= c_used must not arrive
    dx, d0 = _lossmap_bwd(R.COARSEN, x, g, cu, p=(s, te, method))
    want = d0 + R.lossmap_adjoint(R.COARSEN, x, g, cu, (s, te, method))
    if exact:
        _fits(s * s * max(te, 1) * np.abs(x).max(), 0.25 / (s * s * max(te, 1)))
        _fits(np.abs(d0).max() + np.abs(g).max(), 1.0 / (4 * s * s * max(te, 1)))
        np.testing.assert_array_equal(_np(lr), ref.ravel())
        np.testing.assert_array_equal(dx, want)
    else:
        _close2(_np(lr), ref.ravel(), R.coarsen(np.abs(x), s, te, method).ravel(), 'coarsen forward')
        _close2(dx, want, np.abs(d0) + np.abs(want - d0), 'coarsen adjoint')
    np.testing.assert_array_equal(dx[..., cu:], d0[..., cu:])


@pytest.mark.parametrize('s,te,method', COARSEN)
def test_coarsen_and_its_adjoint_exact(s, te, method):
    _coarsen_case((2, 4, 8, 4, 3), 2, s, te, method, exact=True)


def test_coarsen_4d_exact():
    _coarsen_case((3, 4, 6, 1, 3), 2, 2, 1, R.TC_AVERAGE, exact=True)


@pytest.mark.parametrize('method', [R.TC_AVERAGE, R.TC_SUBSAMPLE])
def test_coarsen_by_three(method):
    """s = 3, t_enhance = 3: 1 / 9 and 1 / 3 round"""
    _coarsen_case((2, 6, 3, 6, 3), 2, 3, 3, method, exact=False)


# ================================================================ time windows
WINDOWS = [   # outer, t, c, t0, len
    ('t0_0', (5, 8, 3, 0, 3)), ('to_the_end', (5, 8, 3, 5, 3)), ('len1_c1', (5, 8, 1, 4, 1)),
    ('whole_axis', (5, 8, 3, 0, 8)), ('len4_c1', (7, 8, 1, 2, 4)), ('len2', (3, 5, 3, 1, 2)),
    ('len5', (3, 7, 3, 1, 5)),
]


@pytest.mark.parametrize('case', [w[1] for w in WINDOWS] + [lambda ncu: (16 * ncu * 256 // 2 + 3, 3, 1, 1, 2)],
                         ids=[w[0] for w in WINDOWS] + ['above_cap'])
def test_time_window_exact(case):
    dev, L, _ = _dev()
    outer, t, c, t0, ln = _shape(case)
    rng = np.random.default_rng(10)
    full = _q(rng, (outer, t, c))
    fd, wd = _up(full), dev.empty((outer, ln, c))
    _ok(L.s3_time_window(dev.ctx, _p(fd), outer, t, c, t0, ln, _p(wd), 0, 0.5), 'time_window')
    np.testing.assert_array_equal(_np(wd), R.time_window(full, t0, ln))
    np.testing.assert_array_equal(_np(fd), full)
    g, d0 = _g(rng, (outer, ln, c)), _d0((outer, t, c))
    gd, dd = _up(g), _up(d0)
    _ok(L.s3_time_window(dev.ctx, _p(dd), outer, t, c, t0, ln, _p(gd), 1, 0.5), 'time_window adjoint')
    _fits(np.abs(d0).max() + 0.5 * np.abs(g).max(), 0.25)
    np.testing.assert_array_equal(_np(dd), d0 + R.time_window_adjoint(g, t, t0, ln, 0.5))


@pytest.mark.parametrize('case', [w[1] for w in WINDOWS] + [lambda ncu: (16 * ncu * 256 + 3, 3, 1, 1, 2)],
                         ids=[w[0] for w in WINDOWS] + ['above_cap'])
def test_time_mean(case):
    """exact when len is a power of two; else 1 / len and the product round"""
    dev, L, _ = _dev()
    outer, t, c, t0, ln = _shape(case)
    rng = np.random.default_rng(11)
    full = _q(rng, (outer, t, c))
    fd, md = _up(full), dev.empty((outer, c))
    _ok(L.s3_time_mean(dev.ctx, _p(fd), outer, t, c, t0, ln, _p(md), 0, 0.5), 'time_mean')
    ref = R.time_mean(full, t0, ln)
    _fits(ln * np.abs(full).max(), 0.25)
    g, d0 = _g(rng, (outer, c)), _d0((outer, t, c))
    gd, dd = _up(g), _up(d0)
    _ok(L.s3_time_mean(dev.ctx, _p(dd), outer, t, c, t0, ln, _p(gd), 1, 0.5), 'time_mean adjoint')
    want = d0 + R.time_mean_adjoint(g, t, t0, ln, 0.5)
    if ln & (ln - 1) == 0:
        _fits(np.abs(d0).max() + np.abs(g).max(), 0.5 / ln)
        np.testing.assert_array_equal(_np(md), ref)
        np.testing.assert_array_equal(_np(dd), want)
    else:
        _close2(_np(md), ref, np.abs(ref), 'time mean')
        _close2(_np(dd), want, np.abs(d0) + np.abs(want - d0), 'time mean adjoint')
    np.testing.assert_array_equal(_np(dd)[:, :t0], d0[:, :t0])
    np.testing.assert_array_equal(_np(dd)[:, t0 + ln:], d0[:, t0 + ln:])


# ================================================================ DFT
DFT_L = [1, 2, 37, 248, 249, 288, 'longest']
DFT_VIEWS = [(1, 1), (33, 1), (3, 20)]          # outer, inner: 1, 33 and 60 columns, panels of 32


def _dft_len(L):
    return _lds() // 264 if L == 'longest' else L


def _dft(re, im, outer, L, inner, sign):
    dev, lib, _ = _dev()
    rd, idv = _up(re), (_up(im) if im is not None else None)
    ore, oim = _up(np.full(re.shape, 7.0)), _up(np.full(re.shape, 7.0))
    _ok(lib.s3_dft_axis(dev.ctx, _p(rd), _p(idv), _p(ore), _p(oim), outer, L, inner, sign), 's3_dft_axis')
    return _np(ore) + 1j * _np(oim)


@pytest.mark.parametrize('L', DFT_L)
def test_dft_axis_unit_impulses(L):
    """one 1.0 at index j of every column (a different j per column), real then
    imaginary: the output is the twiddle row of j, every other term an exact
    zero — within 4 2^-24 absolute; pins the j k mod L walk, the ragged last
    panel, the > 64 KB LDS path (L >= 249) and the longest axis accepted"""
    L = _dft_len(L)
    worst = 0.0
    for outer, inner in DFT_VIEWS:
        col = np.arange(outer * inner).reshape(outer, inner)
        j = (7 * col + 3) % L
        x = np.zeros((outer, L, inner))
        np.put_along_axis(x, j[:, None, :], 1.0, axis=1)
        for sign in (-1, 1):
            w = R.twiddles(L, sign)                                        # [k, j]
            row = np.moveaxis(w[:, j], 0, 1)                               # (outer, L, inner)
            for part in ('re', 'im'):
                got = _dft(x, None, outer, L, inner, sign) if part == 're' else \
                    _dft(np.zeros_like(x), x, outer, L, inner, sign)
                ref = row if part == 're' else 1j * row
                worst = max(worst, np.abs(got.real - ref.real).max(), np.abs(got.imag - ref.imag).max())
    print(f'dft impulses L={L}: worst error / (4 2^-24) = {worst / (4 * 2.0 ** -24):.3f}')
    assert worst <= 4 * 2.0 ** -24


@pytest.mark.parametrize('L', DFT_L)
def test_dft_axis_random_input(L):
    """random complex input, both signs, real-only input too: every output
    within (L + 8) 2^-23 sum_j |x_j| of its column"""
    L = _dft_len(L)
    rng = np.random.default_rng(12)
    worst = 0.0
    for outer, inner in DFT_VIEWS:
        re = rng.standard_normal((outer, L, inner)).astype(np.float32)
        im = rng.standard_normal((outer, L, inner)).astype(np.float32)
        for sign in (-1, 1):
            for imag in (im, None):
                got = _dft(re, imag, outer, L, inner, sign)
                ref = R.dft_axis(re, imag, outer, L, inner, sign)
                bound = R.dft_bound(re, imag, outer, L, inner)
                worst = max(worst, (np.abs(got.real - ref.real) / bound).max(),
                            (np.abs(got.imag - ref.imag) / bound).max())
    print(f'RATIO dft L={L}: worst error / bound = {worst:.4f}')
    assert worst <= 1


def test_dft_axis_refuses_the_first_length_that_cannot_fit():
    """host-side argument check: 264 L bytes of LDS per workgroup; nothing is launched"""
    dev, lib, mod = _dev()
    L = _lds() // 264 + 1
    buf = dev.empty((4,))
    rc = lib.s3_dft_axis(dev.ctx, _p(buf), None, _p(buf), _p(buf), 1, L, 1, -1)
    assert rc == EINVAL
    assert 'LDS' in mod.last_error(dev.ctx) and str(L) in mod.last_error(dev.ctx)
    assert lib.s3_dft_axis(dev.ctx, _p(buf), None, _p(buf), _p(buf), 1, 0, 1, -1) == EINVAL


# ================================================================ specmap
SPEC = [   # shape, mode3d
    ('2d', (2, 5, 4, 1, 3), 0), ('3d', (2, 5, 4, 6, 3), 1), ('3d_read_as_2d', (2, 5, 4, 6, 3), 0),
    ('2d_w_above_2p24', (1, 70, 70, 1, 2), 0), ('3d_w_above_2p24', (1, 30, 30, 24, 1), 1),
]


@pytest.mark.parametrize('shape,mode3d', [s[1:] for s in SPEC], ids=[s[0] for s in SPEC])
def test_specmap_forward_and_backward(shape, mode3d):
    """log(1 + w |X|) and its gradient: the w = 0 rows, a column with |X| = 0
    (gradient 0, not NaN), weights beyond 2^24"""
    dev, lib, _ = _dev()
    n, s1, s2, t, c = shape
    rng = np.random.default_rng(13)
    re = (rng.standard_normal(shape) * 3).astype(np.float32)
    im = (rng.standard_normal(shape) * 3).astype(np.float32)
    re[0, s1 - 1, s2 - 1, :, 0] = 0
    im[0, s1 - 1, s2 - 1, :, 0] = 0
    gy = rng.standard_normal(shape).astype(np.float32)
    w = R.spec_weights(s1, s2, t, mode3d)
    if s1 >= 30:
        assert w.max() > 2 ** 24
    rd, idv, gd = _up(re), _up(im), _up(gy)
    y = dev.empty(shape)
    _ok(lib.s3_specmap(dev.ctx, 0, _p(rd), _p(idv), None, n, s1, s2, t, c, mode3d, _p(y), None), 'specmap')
    ref, bound = R.specmap_fwd(re, im, mode3d), R.specmap_fwd_bound(re, im, mode3d)
    err = np.abs(_np(y) - ref)
    assert np.all(_np(y)[:, 0] == 0) and np.all(_np(y)[:, :, 0] == 0)
    ratio_f = (err[bound > 0] / bound[bound > 0]).max()
    assert np.all(err <= bound)
    g0, g1 = _up(np.full(shape, 7.0)), _up(np.full(shape, 7.0))
    _ok(lib.s3_specmap(dev.ctx, 1, _p(rd), _p(idv), _p(gd), n, s1, s2, t, c, mode3d, _p(g0), _p(g1)), 'specmap bwd')
    rr, ri = R.specmap_bwd(re, im, gy, mode3d)
    ratio_b = 0.0
    for got, want in ((_np(g0), rr), (_np(g1), ri)):
        assert np.all(np.isfinite(got))
        b = R.specmap_bwd_bound(want, mode3d)
        e = np.abs(got - want)
        assert np.all(got[0, s1 - 1, s2 - 1, :, 0] == 0) and np.all(got[:, 0] == 0) and np.all(got[:, :, 0] == 0)
        ratio_b = max(ratio_b, (e[b > 0] / b[b > 0]).max())
        assert np.all(e <= b)
    print(f'RATIO specmap {shape} mode3d={mode3d}: forward {ratio_f:.4f}, backward {ratio_b:.4f}')


# ================================================================ MMD
MMD = [   # n, n_pos, c_a, c_b, c_used, sigma
    ('n1_p255_c1', (1, 255, 2, 3, 1, 1.0)),
    ('n2_p257_c3_sigma_half', (2, 257, 4, 3, 3, 0.5)),
    ('n5_p255_c8_sigma3', (5, 255, 8, 9, 8, 3.0)),
    ('n5_p1_c3', (5, 1, 4, 5, 3, 1.0)),
    ('n2_striding', (2, 1024 * 256 + 77, 1, 2, 1, 1.0)),
    ('identical', (2, 257, 4, 3, 3, 1.0)),
]


@pytest.mark.parametrize('case', [m[1] for m in MMD], ids=[m[0] for m in MMD])
def test_mmd_value_and_gradient(case, request):
    dev, lib, _ = _dev()
    n, npos, c_a, c_b, cu, sigma = case
    rng = np.random.default_rng(14)
    a = (rng.standard_normal((n, npos, c_a)) * 0.7).astype(np.float32)
    b = (rng.standard_normal((n, npos, c_b)) * 0.7).astype(np.float32)
    if 'identical' in request.node.name:
        b[..., :cu] = a[..., :cu]
    weight = 0.75
    d0 = _d0((n, npos, c_a), weight / (n * n * npos))
    ad, bd, dd, out = _up(a), _up(b), _up(d0), _up(np.full(4, 7.0))
    _ok(lib.s3_loss_mmd(dev.ctx, _p(ad), c_a, _p(bd), c_b, n, npos, cu, sigma, weight, _p(out), _p(dd)), 'mmd')
    val, grad = R.mmd(a, b, cu, sigma, weight)
    nblk = min(-(-npos // 256), 8 * _cu(), 1024)
    per_thread = -(-npos // (nblk * 256))
    chain = 3 * n * n * per_thread + 6 + 4 + -(-nblk // 256) + 256
    vb, gb = R.mmd_bounds(a, b, cu, sigma, weight, d0, chain)
    got_v, got = _np(out)[0], _np(dd)
    rv = abs(got_v - val) / vb
    rg = (np.abs(got - (d0 + grad))[..., :cu] / gb[..., :cu]).max()
    print(f'RATIO mmd {case}: value {rv:.4f}, gradient {rg:.4f}')
    assert rv <= 1 and rg <= 1
    np.testing.assert_array_equal(got[..., cu:], d0[..., cu:])
    # no gradient asked for: the same value
    _ok(lib.s3_loss_mmd(dev.ctx, _p(ad), c_a, _p(bd), c_b, n, npos, cu, sigma, weight, _p(out), None), 'mmd')
    assert _np(out)[0] == got_v


def test_mmd_refuses_nine_features():
    dev, lib, _ = _dev()
    buf = dev.empty((64,))
    assert lib.s3_loss_mmd(dev.ctx, _p(buf), 9, _p(buf), 9, 1, 1, 9, 1.0, 1.0, _p(buf), None) == EINVAL


# ================================================================ sliced Wasserstein
def _sw(a, b, cu, n_proj, seed, weight):
    """-> value, d_a after the call, its pre-fill, bound of the value, bound
    per element, reference gradient, the device's directions"""
    dev, lib, _ = _dev()
    n, npos, c_a = a.shape
    dirs = dev.empty((n_proj, npos))
    _ok(lib.s3_sw_directions(dev.ctx, seed, n_proj, npos, _p(dirs)), 'sw_directions')
    dirs = _np(dirs)
    vb, gb, ref = R.sw_bounds(a, b, dirs, cu, weight, np.zeros(a.shape))
    d0 = _d0(a.shape, np.sqrt((ref[..., :cu] ** 2).mean()))
    gb = gb + R.HIGHER * R.EPS * np.abs(d0)                # the add into d_a rounds relative to |d0| + |gradient|
    ad, bd, dd, out = _up(a), _up(b), _up(d0), _up(np.full(4, 7.0))
    _ok(lib.s3_loss_sliced_wasserstein(dev.ctx, _p(ad), c_a, _p(bd), b.shape[2], n, npos, cu, n_proj, seed, weight,
                                       _p(out), _p(dd)), 'sliced_wasserstein')
    return _np(out)[0], _np(dd), d0, vb, gb, ref, dirs


@pytest.mark.parametrize('case', R.SW_ZERO_TRUTH, ids=lambda c: f'{c[0]}x{c[1]}x{c[2] * c[3]}')
def test_sliced_wasserstein_zero_truth(case):
    """b = 0: every partner is 0 and d_a no longer depends on the ranks — a
    linear map through projection, range reduction, the scatter through the
    sorted indices, the 512-projection chunks and the back-projection.  The
    largest bound stays below a quarter of what one dropped projection moves
    (RMS / sqrt(n_proj)); a case that cannot say so is an error."""
    n_proj, npos, n, cu, nnz = case
    c_a = cu + 1
    a = R.sw_zero_truth_field(npos, n, nnz, c_a)
    b = np.zeros((n, npos, cu))
    weight = 0.75
    got_v, got, d0, vb, gb, ref, dirs = _sw(a, b, cu, n_proj, 1234 + n_proj, weight)
    rms = np.sqrt((ref[..., :cu] ** 2).mean())
    sharp = gb[..., :cu].max() / rms
    print(f'sw {case}: largest bound / RMS = {sharp:.5f}, limit {1 / (4 * np.sqrt(n_proj)):.5f}')
    assert sharp < 1 / (4 * np.sqrt(n_proj)), 'the bound would hide a dropped projection'
    val, _ = R.sliced_wasserstein(a, b, dirs, cu, weight)
    rv = abs(got_v - val) / vb
    rg = (np.abs(got - (d0 + ref))[..., :cu] / gb[..., :cu]).max()
    print(f'RATIO sw zero truth {case}: value {rv:.4f}, gradient {rg:.4f}')
    assert rv <= 1 and rg <= 1
    np.testing.assert_array_equal(got[..., cu:], d0[..., cu:])


SW_GENERAL_SEED = 7       # of the seeds 1 .. 12 tried on an MI355X the one with the widest gaps (17.8 and 12.3)


def test_sliced_wasserstein_general_truth():
    """(n_proj, n_pos, n c_used) = (17, 61, 33): three column passes, one exo
    channel; value and every element of d_a.  The ranks of the fp32
    projections are the reference's only if no two adjacent sorted projections
    are closer than their error bounds: asserted for the device's directions."""
    n_proj, npos, n, cu, c_a = 17, 61, 11, 3, 4
    rng = np.random.default_rng(15)
    a = rng.standard_normal((n, npos, c_a)).astype(np.float32)
    b = (rng.standard_normal((n, npos, c_a)) * 1.3 + 0.2).astype(np.float32)
    weight = 0.75
    got_v, got, d0, vb, gb, ref, dirs = _sw(a, b, cu, n_proj, SW_GENERAL_SEED, weight)
    gap = min(R.sw_min_gap_ratio(a, dirs, cu), R.sw_min_gap_ratio(b, dirs, cu))
    print(f'sw general truth: smallest gap / error bounds = {gap:.3f}')
    assert gap > 1, 'two projections too close to rank in fp32: pick another seed'
    val, grad = R.sliced_wasserstein(a, b, dirs, cu, weight)
    np.testing.assert_allclose(ref, grad, rtol=1e-9, atol=1e-14)
    rv = abs(got_v - val) / vb
    rg = (np.abs(got - (d0 + grad))[..., :cu] / gb[..., :cu]).max()
    print(f'RATIO sw general truth: value {rv:.4f}, gradient {rg:.4f}')
    assert rv <= 1 and rg <= 1
    np.testing.assert_array_equal(got[..., cu:], d0[..., cu:])
