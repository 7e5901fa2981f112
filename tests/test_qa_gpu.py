"""GPU tests (``-m gpu``) of ``sup3r_amd.qa``: the kernels of
``csrc/kernels_qa.hip`` against ``tests/qa_ref.py``, bit for bit unless said.

NaN: "bit for bit" compares the bits of every value that is not NaN and the
places of the NaNs; a NaN's sign and payload are not compared.

Summary words: the device folds fp64 partial sums in a fixed tree, numpy adds
float64 pairwise; both are many orders below a float32 ulp, so after one
rounding to float32 they are at most one ulp apart.

``norm`` of the distributions: numpy squares in float32 (2^-24 relative each)
and adds pairwise in float32 (log2(n) 2^-24); the device's fp64 sum is exact
at that scale, so the two means differ by at most (log2(n) + 2) 2^-24
relative, the roots by half of it, plus one rounding."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

from tests import qa_ref as R

pytestmark = pytest.mark.gpu

EINVAL = -1
PAD = 64
SENTINEL = 0x7FC5A5A5                        # a NaN: poisoned guards
CFG = os.path.join(os.path.dirname(os.path.dirname(__file__)), 'sup3r_amd',
                   'configs')


def backend():
    from sup3r_amd import qa
    return qa.QaDeviceBackend()


def guarded(shape):
    """an fp32 device tensor of ``shape`` inside a NaN-poisoned buffer"""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.int32,
                     device='cuda')
    return buf.view(torch.float32)[PAD:PAD + n].view(*shape), buf


def guards_intact(buf, n):
    b = buf.cpu().numpy()
    return bool((b[:PAD] == SENTINEL).all() and (b[PAD + n:] == SENTINEL).all())


def raw_recoarsen(hr, layout, dims, c, channels, methods, s, te, true=None,
                  syn=None, err=None, summary=None):
    from sup3r_amd import _lib
    dev = backend().dev
    F = len(methods)
    ints = C.c_int32 * max(F, 1)

    def ptrs(ts):
        if ts is None:
            return None
        return (C.c_void_p * F)(*[None if t is None else t.data_ptr()
                                  for t in ts])
    rc = _lib.lib().s3_qa_recoarsen(
        dev.ctx, C.c_void_p(hr.data_ptr()), layout, *dims, c,
        ints(*channels) if channels is not None else None, ints(*methods), F,
        s, te, ptrs(true), ptrs(syn), ptrs(err),
        None if summary is None else C.c_void_p(summary.data_ptr()))
    dev.sync()
    return rc


def field(rng, shape, mean=280.0):
    return (rng.standard_normal(shape) * 30 + mean).astype(np.float32)


def plant(rng, x):
    """NaN and +-inf in a few places"""
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=min(flat.size, 1 + flat.size // 97),
                     replace=False)
    for n, i in enumerate(idx):
        flat[i] = (np.nan, np.inf, -np.inf)[n % 3]
    return x


def ulps32(a, b):
    a, b = np.float32(a), np.float32(b)
    if a == b:
        return 0
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def check_summary(words, err):
    want = R.summary(err)
    assert words[0] == want[0] and words[4] == want[4], (words, want)
    for k in (1, 2, 3):
        assert ulps32(words[k], want[k]) <= 1, (k, words[k], want[k])


# ------------------------------------------------------------- re-coarsening
GRIDS = [(1, 1, 1), (3, 5, 2), (8, 8, 8), (2, 63, 5), (2, 64, 5), (2, 65, 5)]


@pytest.mark.parametrize('s', [1, 2, 3, 5])
@pytest.mark.parametrize('te', [1, 4, 24])
def test_recoarsen_both_layouts_every_method(s, te):
    """one feature: time-first and the C = 1 cube, every method and grid,
    NaN and +-inf planted, syn / err / summary against qa_ref, two runs"""
    be = backend()
    rng = np.random.default_rng(10 * s + te)
    for grid in GRIDS:
        S1, S2, T = grid
        hr = plant(rng, field(rng, (S1 * s, S2 * s, T * te)))
        true = field(rng, grid)
        tf = np.ascontiguousarray(hr.transpose(2, 0, 1))
        for method in R.METHODS:
            want = R.fixed_order(hr, s, te, method)
            with np.errstate(invalid='ignore'):
                want_err = want - true
            runs = []
            for data, layout in ((tf, 'tfirst'), (hr[..., None], 'cube'),
                                 (tf, 'tfirst')):
                (syn, err, words), = be.recoarsen(data, layout, [0], [method],
                                                  s, te, true=[true])
                syn, err = syn.cpu().numpy(), err.cpu().numpy()
                assert R.same_bits(syn, want), (grid, method, layout)
                assert R.same_bits(err, want_err), (grid, method, layout)
                check_summary(words, want_err)
                runs.append((layout, syn, err, words))
            # two runs of the time-first kernel: equal bits, NaN included
            a, b = runs[0], runs[2]
            assert a[1].tobytes() == b[1].tobytes()
            assert a[2].tobytes() == b[2].tobytes()
            assert a[3].tobytes() == b[3].tobytes()


@pytest.mark.parametrize('F', [1, 3, 16])
def test_recoarsen_cube_channel_map_guards_and_null_outputs(F):
    """a 16-channel cube, a permuted channel map, a method per feature, two
    step chunks per pixel (t_enhance 24 x 16 channels x 11 steps > 4096
    floats); NaN-poisoned guards around every output; NULL outputs"""
    import torch
    rng = np.random.default_rng(F)
    s, te, grid, c = 2, 24, (2, 3, 11), 16
    cube = plant(rng, field(rng, (grid[0] * s, grid[1] * s, grid[2] * te, c)))
    chans = [int(v) for v in rng.permutation(c)[:F]]
    methods = [R.METHODS[(i + F) % 5] for i in range(F)]
    from sup3r_amd import _lib
    codes = [_lib.TC_METHODS[m] for m in methods]
    trues = [field(rng, grid) for _ in range(F)]
    cube_d = backend().asarray(cube)
    true_d = [backend().asarray(t) for t in trues]
    n = int(np.prod(grid))
    syn, err = [guarded(grid) for _ in range(F)], [guarded(grid)
                                                   for _ in range(F)]
    words, wbuf = guarded((F, 10))            # F x 5 doubles
    dims = cube.shape[:3]
    rc = raw_recoarsen(cube_d, 0, dims, c, chans, codes, s, te, true_d,
                       [t for t, _ in syn], [t for t, _ in err], words)
    assert rc == 0
    got_words = words.cpu().numpy().view(np.float64).reshape(F, 5)
    for f in range(F):
        want = R.fixed_order(cube[..., chans[f]], s, te, methods[f])
        with np.errstate(invalid='ignore'):
            want_err = want - trues[f]
        assert R.same_bits(syn[f][0].cpu().numpy(), want), (f, methods[f])
        assert R.same_bits(err[f][0].cpu().numpy(), want_err)
        check_summary(got_words[f], want_err)
        assert guards_intact(syn[f][1], n) and guards_intact(err[f][1], n)
    assert guards_intact(wbuf, F * 10)
    # a second run gives the same bits
    words2 = torch.zeros((F, 5), dtype=torch.float64, device='cuda')
    assert raw_recoarsen(cube_d, 0, dims, c, chans, codes, s, te, true_d,
                         None, None, words2) == 0
    assert words2.cpu().numpy().tobytes() == got_words.tobytes()
    # NULL outputs: synthetic alone (no true field), error alone
    only, obuf = guarded(grid)
    assert raw_recoarsen(cube_d, 0, dims, c, chans[:1], codes[:1], s, te,
                         None, [only], None, None) == 0
    assert R.same_bits(only.cpu().numpy(),
                       R.fixed_order(cube[..., chans[0]], s, te, methods[0]))
    assert guards_intact(obuf, n)
    only, obuf = guarded(grid)
    assert raw_recoarsen(cube_d, 0, dims, c, chans[:1], codes[:1], s, te,
                         true_d[:1], None, [only], None) == 0
    with np.errstate(invalid='ignore'):
        assert R.same_bits(only.cpu().numpy(), R.fixed_order(
            cube[..., chans[0]], s, te, methods[0]) - trues[0])
    assert guards_intact(obuf, n)


def test_recoarsen_time_first_tiles():
    """several column tiles and step chunks, neither a multiple of the LDS
    tile: 130 low-res columns in tiles of 64 / s = 21, 37 steps in chunks of
    128 / t_enhance = 32; then s = 7, which has no unrolled instantiation"""
    be = backend()
    rng = np.random.default_rng(77)
    s, te, grid = 3, 4, (2, 130, 37)
    hr = field(rng, (grid[0] * s, grid[1] * s, grid[2] * te))
    true = field(rng, grid)
    tf = np.ascontiguousarray(hr.transpose(2, 0, 1))
    for method in ('average', 'max'):
        (syn, err, words), = be.recoarsen(tf, 'tfirst', [0], [method], s, te,
                                          true=[true])
        want = R.fixed_order(hr, s, te, method)
        assert R.same_bits(syn.cpu().numpy(), want)
        assert R.same_bits(err.cpu().numpy(), want - true)
        check_summary(words, want - true)
    s, te, grid = 7, 3, (2, 11, 5)
    hr = field(rng, (grid[0] * s, grid[1] * s, grid[2] * te))
    true = field(rng, grid)
    for data, layout in ((np.ascontiguousarray(hr.transpose(2, 0, 1)),
                          'tfirst'), (hr[..., None], 'cube')):
        (syn, err, words), = be.recoarsen(data, layout, [0], ['total'], s, te,
                                          true=[true])
        assert R.same_bits(syn.cpu().numpy(), R.fixed_order(hr, s, te, 'total'))


def test_recoarsen_einval():
    x = backend().asarray(np.zeros((6, 6, 8, 2), np.float32))
    out, _ = guarded((2, 2, 2))
    ok = dict(hr=x, layout=0, dims=(6, 6, 8), c=2, channels=[0], methods=[0],
              s=3, te=4, syn=[out])
    assert raw_recoarsen(**ok) == 0
    assert raw_recoarsen(**{**ok, 's': 4}) == EINVAL          # H1, H2
    assert raw_recoarsen(**{**ok, 'dims': (6, 8, 6), 's': 3}) == EINVAL
    assert raw_recoarsen(**{**ok, 'te': 3}) == EINVAL         # HT
    assert raw_recoarsen(**{**ok, 'methods': [5]}) == EINVAL
    assert raw_recoarsen(**{**ok, 'channels': [2]}) == EINVAL
    assert raw_recoarsen(**{**ok, 'layout': 2}) == EINVAL
    many = dict(ok, channels=[0] * 17, methods=[0] * 17, syn=[out] * 17)
    assert raw_recoarsen(**many) == EINVAL                    # 17 features
    with pytest.raises(KeyError, match='Did not recognize temporal_coarsening'):
        backend().recoarsen(x, 'cube', [0], ['median'], 3, 4)


# -------------------------------------------------------------------- select
def _select_cases(rng, n):
    return {
        'normal': rng.standard_normal(n).astype(np.float32),
        'equal': np.full(n, -1.5, np.float32),
        'lowest bit': (np.float32(1) + rng.integers(0, 2, n).astype(np.float32)
                       * np.float32(2.0 ** -23)).astype(np.float32),
        'zeros': np.array([0.0, -0.0] * n, np.float32)[:n],
        'denormal': rng.integers(0, 50, n).astype(np.uint32).view(np.float32),
    }


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 255, 256, 257, 2 ** 20 + 3])
def test_select_is_np_percentile(n):
    from sup3r_amd import qa
    be = backend()
    rng = np.random.default_rng(n)
    for name, x in _select_cases(rng, n).items():
        v = be.asarray(x)
        xf = qa._Xform('direct', x.shape)
        for q in (0, 50, 99.9, 100):
            got, want = be.percentile(v, xf, q), np.percentile(np.abs(x), q)
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), \
                (name, q, got, want)


# ----------------------------------------------------------------- histogram
def _raw_counts(x, bins, rng_, diff_max=None):
    from sup3r_amd import _lib, qa
    be = backend()
    v = be.asarray(x)
    xf = qa._Xform('direct', x.shape)
    base = _lib.QA_HIST_KEEP_ALL if diff_max is None else 0
    st, counts, edges = be._counts(v, xf, base, np.float32(diff_max or 0),
                                   bins, rng_)
    return st, counts, edges


@pytest.mark.parametrize('bins', [1, 40, 4096])
@pytest.mark.parametrize('rng_', [None, (-1.0, 1.5), (0, 2)])
def test_histogram_counts_are_np_histogram(bins, rng_):
    rng = np.random.default_rng(bins)
    x = rng.standard_normal(70001).astype(np.float32)
    edges = np.histogram(x, bins=bins, range=rng_)[1].astype(np.float32)
    planted = np.concatenate([edges, np.nextafter(edges, np.float32(-9)),
                              np.nextafter(edges, np.float32(9))])
    if rng_ is None:       # keep the data's min and max (and so the edges)
        planted = planted[(planted >= x.min()) & (planted <= x.max())]
    x = np.concatenate([x, planted])
    st, counts, e = _raw_counts(x, bins, rng_)
    want, e2 = np.histogram(x, bins=bins, range=rng_)
    assert e.dtype == e2.dtype and np.array_equal(e, e2)
    assert np.array_equal(counts, want)
    assert st[0] == x.size and st[2] == x.min() and st[3] == x.max()
    assert ulps32(st[1], (x.astype(np.float64) ** 2).sum()) <= 1


def test_histogram_min_is_max_nothing_kept_and_nan():
    from sup3r_amd import qa
    one = np.full(300, 3.25, np.float32)
    _, counts, e = _raw_counts(one, 40, None)
    want, e2 = np.histogram(one, bins=40)
    assert np.array_equal(counts, want) and np.array_equal(e, e2)
    x = np.random.default_rng(0).standard_normal(1000).astype(np.float32) + 5
    st, counts, e = _raw_counts(x, 40, None, diff_max=1e-3)    # nothing kept
    want, e2 = np.histogram(x[:0], bins=40)
    assert st[0] == 0 and np.array_equal(counts, want) and np.array_equal(e, e2)
    x[[3, 500, 999]] = np.nan
    for fn in (qa.direct_dist, qa.gradient_dist, qa.time_derivative_dist):
        for kw in ({}, {'diff_max': 2.0}):
            with pytest.raises(ValueError, match=r'\d+ NaN values'):
                fn(x.reshape(10, 10, 10), **kw)
    with pytest.raises(ValueError, match='^3 NaN values'):
        qa.direct_dist(x.reshape(10, 10, 10))
    with pytest.raises(NotImplementedError):
        qa.continuous_dist(backend().asarray(x))


@pytest.mark.parametrize('name', ['direct_dist', 'gradient_dist',
                                  'time_derivative_dist'])
@pytest.mark.parametrize('period', [None, 360])
def test_dist_functions(name, period):
    from sup3r_amd import qa
    rng = np.random.default_rng(len(name))
    var = (rng.random((9, 11, 13)) * 360).astype(np.float32)
    flat = (rng.random((10, 10)) * 5).astype(np.float32)
    cases = [(var, dict(scale=3, period=period)),
             (var, dict(bins=12, range=(-50.0, 70.0), period=period,
                        interpolate=True, percentile=90)),
             (var, dict(diff_max=40.0, scale=3, period=period)),
             (flat, dict(period=period))]
    for x, kw in cases:
        if name == 'time_derivative_dist' and x is var:
            kw = dict(kw, t_steps=2)
        for data in (x, backend().asarray(x)):
            centers, counts, norm = getattr(qa, name)(data, **kw)
            c2, n2, norm2 = getattr(R, name)(x, **kw)
            assert centers.dtype == c2.dtype and np.array_equal(centers, c2)
            assert counts.dtype == n2.dtype and np.array_equal(counts, n2)
            n = max(2, R.transformed(name.split('_')[0], x, **{
                k: v for k, v in kw.items()
                if k in ('scale', 'period', 't_steps')}).size)
            tol = (np.log2(n) + 2) * 2.0 ** -24 / 2 + 2.0 ** -23
            assert isinstance(norm, np.float32)
            assert abs(float(norm) - float(norm2)) <= tol * float(norm2)


# ------------------------------------------------------------------- spectra
def _rel_err(E, E64):
    return float(np.abs(np.asarray(E, np.float64) - E64).max() / E64.max())


@pytest.mark.parametrize('shape', [(10, 10), (7, 12, 9), (9, 31)])
def test_spectra_within_four_times_numpy_float32(shape, capsys):
    """device L-inf error relative to max E, against the float64 reference;
    numpy's own float32 fftn route measured at the same inputs; the direct
    DFT's longer sums are allowed 4x the latter"""
    from sup3r_amd import qa
    rng = np.random.default_rng(sum(shape))
    u32 = (rng.standard_normal(shape) * 3 + 1).astype(np.float32)
    v32 = (rng.standard_normal(shape) * 2 - 1).astype(np.float32)
    u64, v64 = u32.astype(np.float64), v32.astype(np.float64)
    jobs = [('frequency_spectrum', (u32,), (u64,), {}),
            ('tke_frequency_spectrum', (u32, v32), (u64, v64),
             {'f_range': [0.0, 2.0]})]
    if len(shape) == 2:
        jobs += [('wavenumber_spectrum', (u32,), (u64,), {}),
                 ('wavenumber_spectrum', (u32,), (u64,), {'axis': 1}),
                 ('tke_wavenumber_spectrum', (u32, v32), (u64, v64),
                  {'x_range': [0.1, 3.0], 'axis': 1})]
    for name, a32, a64, kw in jobs:
        x64, E64 = getattr(R, name)(*a64, **kw)
        x32, E32 = getattr(R, name)(*a32, **kw)
        x, E = getattr(qa, name)(*a32, **kw)
        assert np.array_equal(x, x64) and E.shape == E64.shape
        dev, ref = _rel_err(E, E64), _rel_err(E32, E64)
        with capsys.disabled():
            print(f'\n  {name}{shape}{kw}: device {dev:.3e}, numpy float32 '
                  f'{ref:.3e}')
        assert dev <= 4 * ref, (name, shape, dev, ref)


def test_spectrum_axis_limit():
    from sup3r_amd import qa
    x = np.zeros((2, 700), np.float32)
    with pytest.raises(ValueError, match='longest axis'):
        qa.frequency_spectrum(x)


# ---------------------------------------------------------------- end to end
def test_forward_pass_then_qa(tmp_path):
    """a toy Sup3rGan through ForwardPass with NpzOutputHandler on an
    (8, 8, 8) domain at 3x / 4x, Sup3rQa on the result: the device's errors
    are the NumpyBackend's of the same objects, bit for bit"""
    from sup3r_amd import ForwardPass, Sup3rGan, Sup3rQa, derive
    from sup3r_amd import qa as Q
    from sup3r_amd.forward_pass import register_model
    from sup3r_amd.strategy import ArrayStrategy
    feats = ['u_10m', 'v_10m']
    Sup3rGan.seed(5)
    model = Sup3rGan(os.path.join(CFG, 'gen_3x_4x_2f.json'),
                     os.path.join(CFG, 'test_disc_st_same.json'),
                     means={f: np.float32(0.1) for f in feats},
                     stdevs={f: np.float32(1.5) for f in feats})
    model.set_model_params(lr_features=feats, hr_out_features=feats,
                           s_enhance=3, t_enhance=4)
    model.init_weights((1, 8, 8, 8, 2), (1, 24, 24, 32, 2))
    rng = np.random.default_rng(8)
    domain = rng.standard_normal((8, 8, 8, 2)).astype(np.float32)
    register_model('Sup3rGan', {'model_dir': 'qa-test'}, model)
    pat = os.path.join(str(tmp_path), 'out_{file_id}.npz')
    st = ArrayStrategy(domain, {'model_dir': 'qa-test'}, (8, 8, 8),
                       spatial_pad=1, temporal_pad=1, out_pattern=pat,
                       max_nodes=1, model=model)
    assert ForwardPass.run(st, 0) == 1
    out_fp, = st.out_files

    def source():
        lat = np.linspace(40, 39, 8)[:, None] * np.ones((1, 8))
        lon = np.ones((8, 1)) * np.linspace(-105, -104, 8)[None]
        return derive.DeriveData(
            {f: domain[..., i] for i, f in enumerate(feats)},
            np.stack([lat, lon], -1),
            pd.date_range('2020-01-01', periods=8, freq='h'))
    results = {}
    for name, be in (('device', Q.QaDeviceBackend()),
                     ('numpy', Q.QaNumpyBackend())):
        qa_fp = os.path.join(str(tmp_path), f'qa_{name}.npz')
        with Sup3rQa(source(), out_fp, 3, 4, ['average', 'subsample'],
                     qa_fp=qa_fp, backend=be) as qa:
            assert qa.features == feats
            errors = qa.run()
            results[name] = ({k: np.asarray(be.to_numpy(v))
                              for k, v in errors.items()}, qa.error_stats,
                             dict(np.load(qa_fp)))
    dev, ref = results['device'], results['numpy']
    with np.load(out_fp) as z:
        cube = z['data']
    for i, f in enumerate(feats):
        assert dev[0][f].shape == (8, 8, 8)
        assert R.same_bits(dev[0][f], ref[0][f])
        want = R.fixed_order(cube[..., i], 3, 4, ('average', 'subsample')[i])
        assert R.same_bits(dev[0][f], want - domain[..., i])
        assert dev[1][f]['count'] == ref[1][f]['count'] == 512
        assert dev[1][f]['max_abs'] == ref[1][f]['max_abs']
        for k in ('bias', 'mae', 'rmse'):
            assert ulps32(dev[1][f][k], ref[1][f][k]) <= 1
    assert sorted(dev[2]) == sorted(ref[2])
    for k in dev[2]:
        assert np.array_equal(dev[2][k], ref[2][k]), k
