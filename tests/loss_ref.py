"""float64 restatement of the structured content-loss entry points
(sup3r_amd/csrc/kernels_loss.hip, kernels_loss_sw.hip, kernels_time_window.hip,
``s3_coarsen`` of kernels_transform.hip) — TEST INFRASTRUCTURE ONLY.

One function per C ABI call, with the device's argument shapes: x is
(n, s1, s2, t, c) (t = 1 for 4-D batches) and only the first ``c_used``
channels take part.  The adjoints are written independently of the kernels'
stencil code:

* linear maps (derivatives, mean, coarsening, time windows, DFT): a dense
  matrix per axis made by applying the forward to unit vectors, transposed; or
  the transpose of explicit index arithmetic (``np.repeat`` for a block mean);
* non-linear maps (material derivative, extremes, MMD, specmap, sliced
  Wasserstein): torch float64 autograd on the CPU.  ``amin`` / ``amax`` share a
  tie's gradient equally, as tf.reduce_min / reduce_max do.

Pinned on the CPU by tests/test_loss_ref_cpu.py (against oracle/losses.py, by
``<F x, y> = <x, F^T y>`` and against autograd).  The ``*_bound`` functions are
the per-element error bounds of the fp32 kernels, computed in float64 from the
reference's own sums of absolute terms; profiles/losses/NOTES.md derives them.
"""
import numpy as np

DERIV_S, DERIV_T, MATERIAL, MEAN_S, EXT_S, EXT_T, COARSEN = range(7)
TC_SUBSAMPLE, TC_AVERAGE = 0, 1
EPS = 2.0 ** -24            # half an fp32 ulp, relative: one rounding
HIGHER = 1 + 2.0 ** -10     # room for the products of two such errors


def _t():
    import torch
    return torch


# ------------------------------------------------------------ linear pieces
def derivative_rows(x):
    """np.gradient's first-order scheme along axis 0: one-sided at both ends,
    central inside (sup3r/utilities/loss_metrics.py:12-59)"""
    L = x.shape[0]
    out = np.empty_like(x)
    out[0] = x[1] - x[0]
    out[L - 1] = x[L - 1] - x[L - 2]
    for i in range(1, L - 1):
        out[i] = (x[i + 1] - x[i - 1]) / 2
    return out


def derivative_matrix(L):
    """dense (L, L) matrix of ``derivative_rows``: the forward applied to the
    unit vectors"""
    return derivative_rows(np.eye(L, dtype=np.float64))


def apply_axis(m, x, axis):
    """y = m applied along ``axis`` of x"""
    return np.moveaxis(np.tensordot(m, x, axes=(1, axis)), 0, axis)


def coarsen(x, s, te, method):
    """s3_coarsen as LowResLoss uses it: s x s block mean, then the mean
    (TC_AVERAGE) or the first step (TC_SUBSAMPLE) of every te steps; te <= 1:
    spatial only.  (n, s1, s2, t, c) -> (n, s1/s, s2/s, t/te, c)"""
    x = np.asarray(x, np.float64)
    n, s1, s2, t, c = x.shape
    y = x.reshape(n, s1 // s, s, s2 // s, s, t, c).mean(axis=(2, 4))
    if te > 1:
        y = y.reshape(n, s1 // s, s2 // s, t // te, te, c)
        y = y.mean(axis=4) if method == TC_AVERAGE else y[:, :, :, :, 0]
    return y


def coarsen_adjoint(g, s, te, method):
    """transpose of ``coarsen``: (n, o1, o2, ot, c) -> (n, o1 s, o2 s, ot te, c)"""
    g = np.asarray(g, np.float64)
    d = np.repeat(np.repeat(g, s, axis=1), s, axis=2) / (s * s)
    if te > 1:
        if method == TC_AVERAGE:
            d = np.repeat(d, te, axis=3) / te
        else:
            n, a, b, ot, c = d.shape
            full = np.zeros((n, a, b, ot, te, c))
            full[:, :, :, :, 0] = d
            d = full.reshape(n, a, b, ot * te, c)
    return d


# ------------------------------------------------------------ s3_lossmap_*
def _material_torch(xt, hub):
    torch = _t()
    n, s1, s2, t, _ = xt.shape
    d1 = torch.from_numpy(derivative_matrix(s1))
    d2 = torch.from_numpy(derivative_matrix(s2))
    dt = torch.from_numpy(derivative_matrix(t))
    u, v = xt[..., 0:2 * hub:2], xt[..., 1:2 * hub:2]
    return (torch.einsum('ab,nijbk->nijak', dt, u) +
            u * torch.einsum('ab,nbjtk->najtk', d1, u) +
            v * torch.einsum('ab,nibtk->niatk', d2, u))


def _extremes_torch(xt, spatial):
    dims = (1, 2) if spatial else (3,)
    return _t().stack([xt.amin(dim=dims), xt.amax(dim=dims)])


def lossmap_fwd(kind, x, c_used):
    """F(x): the shapes of include/sup3r_hip.h; the extremes as (2, ...)"""
    x = np.asarray(x, np.float64)
    xu = x[..., :c_used]
    n, s1, s2, t, _ = x.shape
    if kind == DERIV_S:
        return (apply_axis(derivative_matrix(s1), xu, 1) +
                apply_axis(derivative_matrix(s2), xu, 2))
    if kind == DERIV_T:
        return apply_axis(derivative_matrix(t), xu, 3)
    if kind == MATERIAL:
        return _material_torch(_t().from_numpy(np.ascontiguousarray(xu)), c_used // 2).numpy()
    if kind == MEAN_S:
        return xu.mean(axis=(1, 2))
    if kind == EXT_S:
        return np.stack([xu.min(axis=(1, 2)), xu.max(axis=(1, 2))])
    if kind == EXT_T:
        return np.stack([xu.min(axis=3), xu.max(axis=3)])
    raise KeyError(kind)


def lossmap_adjoint(kind, x, g_out, c_used, p=(0, 0, 0)):
    """F'(x)^T g_out as an (n, s1, s2, t, c) array that is zero in the channels
    >= c_used: what s3_lossmap_bwd ADDS to d_x.  g_out has the shape of
    ``lossmap_fwd`` (COARSEN: (n, s1/s, s2/s, t/te, c), all c channels)"""
    torch = _t()
    x = np.asarray(x, np.float64)
    g = np.asarray(g_out, np.float64)
    n, s1, s2, t, c = x.shape
    out = np.zeros_like(x)
    if kind == DERIV_S:
        out[..., :c_used] = (apply_axis(derivative_matrix(s1).T, g, 1) +
                             apply_axis(derivative_matrix(s2).T, g, 2))
    elif kind == DERIV_T:
        out[..., :c_used] = apply_axis(derivative_matrix(t).T, g, 3)
    elif kind == MEAN_S:
        out[..., :c_used] = g[:, None, None] / (s1 * s2)
    elif kind == COARSEN:
        out[..., :c_used] = coarsen_adjoint(g, *p)[..., :c_used]
    elif kind in (MATERIAL, EXT_S, EXT_T):
        xt = torch.from_numpy(np.ascontiguousarray(x[..., :c_used])).requires_grad_(True)
        y = (_material_torch(xt, c_used // 2) if kind == MATERIAL
             else _extremes_torch(xt, kind == EXT_S))
        (y * torch.from_numpy(np.ascontiguousarray(g))).sum().backward()
        out[..., :c_used] = xt.grad.numpy()
    else:
        raise KeyError(kind)
    return out


def extremes_counts(x, c_used, spatial):
    """(2, ...) number of elements tied at the min | max"""
    xu = np.asarray(x, np.float64)[..., :c_used]
    ax = (1, 2) if spatial else (3,)
    return np.stack([(xu == xu.min(axis=ax, keepdims=True)).sum(axis=ax),
                     (xu == xu.max(axis=ax, keepdims=True)).sum(axis=ax)])


# ------------------------------------------------------------ time windows
def time_window(full, t0, ln):
    return np.asarray(full, np.float64)[:, t0:t0 + ln, :].copy()


def time_window_adjoint(window, t, t0, ln, scale):
    w = np.asarray(window, np.float64)
    out = np.zeros((w.shape[0], t, w.shape[2]))
    out[:, t0:t0 + ln, :] = scale * w
    return out


def time_mean(full, t0, ln):
    return np.asarray(full, np.float64)[:, t0:t0 + ln, :].mean(axis=1)


def time_mean_adjoint(mean, t, t0, ln, scale):
    m = np.asarray(mean, np.float64)
    out = np.zeros((m.shape[0], t, m.shape[1]))
    out[:, t0:t0 + ln, :] = (scale / ln) * m[:, None, :]
    return out


# ------------------------------------------------------------ s3_dft_axis
def twiddles(L, sign):
    """W[k, j] = exp(sign 2 pi i (j k mod L) / L), the index reduced in
    integers so that the float64 argument stays below 2 pi"""
    jk = np.outer(np.arange(L), np.arange(L)) % L
    ang = 2.0 * np.pi * jk / L
    return np.cos(ang) + (1j if sign > 0 else -1j) * np.sin(ang)


def dft_axis(re, im, outer, L, inner, sign):
    """unnormalised DFT along the middle axis of an (outer, L, inner) view;
    sign < 0 forward.  Returns a complex (outer, L, inner) array"""
    z = np.asarray(re, np.float64).reshape(outer, L, inner).astype(np.complex128)
    if im is not None:
        z = z + 1j * np.asarray(im, np.float64).reshape(outer, L, inner)
    return np.einsum('kj,oji->oki', twiddles(L, sign), z)


def dft_bound(re, im, outer, L, inner):
    """(outer, 1, inner): (L + 8) 2^-23 sum_j |x_j| of the column, for both
    parts of every output of that column"""
    z = np.asarray(re, np.float64).reshape(outer, L, inner).astype(np.complex128)
    if im is not None:
        z = z + 1j * np.asarray(im, np.float64).reshape(outer, L, inner)
    return (L + 8) * 2.0 ** -23 * np.abs(z).sum(axis=1, keepdims=True)


# ------------------------------------------------------------ s3_specmap
def spec_weights(s1, s2, t, mode3d):
    """w = k1^2 k2^2 (kt^2), exact integers in float64, (1, s1, s2, t, 1)"""
    w = (np.arange(s1, dtype=np.float64) ** 2)[:, None, None] * \
        (np.arange(s2, dtype=np.float64) ** 2)[None, :, None] * \
        ((np.arange(t, dtype=np.float64) ** 2) if mode3d else np.ones(t))[None, None, :]
    return w[None, :, :, :, None]


def specmap_fwd(re, im, mode3d):
    re, im = np.asarray(re, np.float64), np.asarray(im, np.float64)
    _, s1, s2, t, _ = re.shape
    return np.log1p(spec_weights(s1, s2, t, mode3d) * np.hypot(re, im))


def specmap_bwd(re, im, g_y, mode3d):
    """(G_re, G_im) = d sum(g_y y) / d (re, im) by autograd; 0 where |X| = 0,
    as tf.abs' gradient is"""
    torch = _t()
    _, s1, s2, t, _ = np.shape(re)
    w = torch.from_numpy(np.broadcast_to(spec_weights(s1, s2, t, mode3d), np.shape(re)).copy())
    r = torch.from_numpy(np.asarray(re, np.float64).copy()).requires_grad_(True)
    i = torch.from_numpy(np.asarray(im, np.float64).copy()).requires_grad_(True)
    z = torch.complex(r, i)
    y = torch.log1p(w * z.abs())
    (y * torch.from_numpy(np.asarray(g_y, np.float64).copy())).sum().backward()
    return r.grad.numpy(), i.grad.numpy()


def _spec_w_roundings(mode3d):
    # (float)i1 * i1 * i2 * i2 (* (it * it)): every product may round once
    return 5 if mode3d else 3


def specmap_fwd_bound(re, im, mode3d):
    """y = log1pf(z), z = w |X|: z carries the roundings of w, two of |X|
    (re^2 + im^2: each product and the sum, halved by the root, and the root)
    and the product's, d y = d z / (1 + z); log1pf itself within 1 ulp"""
    y = specmap_fwd(re, im, mode3d)
    z = np.expm1(y)
    nz = _spec_w_roundings(mode3d) + 3
    return HIGHER * (nz * EPS * z / (1 + z) + 2 * EPS * np.abs(y))


def specmap_bwd_bound(ref, mode3d):
    """f = g w / ((1 + w |X|) |X|), G = f X: relative roundings — numerator
    w's + 1; 1 + z: z's (w's + 3) + 1; times |X|: 2 + 1; the division; the
    last product: 2 w's + 10"""
    return HIGHER * (2 * _spec_w_roundings(mode3d) + 10) * EPS * np.abs(ref)


# ------------------------------------------------------------ s3_loss_mmd
def _mmd_kernels(a, b, sigma):
    """kaa, kab, kbb[i, j, p] over the used channels"""
    def k(x, y):
        d = ((x[:, None] - y[None]) ** 2).sum(axis=-1)
        return np.exp(-0.5 * d / sigma ** 2), 0.5 * d / sigma ** 2
    return k(a, a), k(a, b), k(b, b)


def mmd(a, b, c_used, sigma, weight):
    """value and weight * d value / d a ((n, n_pos, c_a), zero in the channels
    >= c_used) by autograd; a, b = (n, n_pos, c_*)"""
    torch = _t()
    a = np.asarray(a, np.float64)
    at = torch.from_numpy(np.ascontiguousarray(a[..., :c_used])).requires_grad_(True)
    bt = torch.from_numpy(np.ascontiguousarray(np.asarray(b, np.float64)[..., :c_used]))

    def k(x, y):
        return torch.exp(-0.5 * ((x[:, None] - y[None]) ** 2).sum(dim=-1) / sigma ** 2)
    val = k(at, at).mean() + k(bt, bt).mean() - 2 * k(at, bt).mean()
    val.backward()
    d = np.zeros_like(a)
    d[..., :c_used] = weight * at.grad.numpy()
    return float(val.detach()), d


def mmd_terms(a, b, c_used, sigma, weight):
    """the kernel's sum written out in float64: T1, T2[i, j, p, c] with
    d_a[i, p, c] = sum_j (T1 + T2), and the relative error of every gaussian"""
    a = np.asarray(a, np.float64)[..., :c_used]
    b = np.asarray(b, np.float64)[..., :c_used]
    n, npos, _ = a.shape
    (kaa, xaa), (kab, xab), (kbb, xbb) = _mmd_kernels(a, b, sigma)
    gs = weight / (n * n * npos) / sigma ** 2
    t1 = -2 * gs * kaa[..., None] * (a[:, None] - a[None])
    t2 = 2 * gs * kab[..., None] * (a[:, None] - b[None])
    # argument: (cu + 2) roundings of the squared distance, 2 of 1 / sigma^2,
    # the product; __expf(x) within (2 + |x|) 2^-23 relative
    def ek(x):
        return x * (c_used + 5) * EPS + (2 + x) * 2 * EPS
    return (kaa, kab, kbb), (t1, t2), (ek(xaa), ek(xab), ek(xbb))


def mmd_bounds(a, b, c_used, sigma, weight, d0, chain):
    """(bound of the value, bound of every d_a element).  ``chain``: the
    longest chain of fp32 additions a term of the value goes through"""
    a = np.asarray(a, np.float64)
    n, npos, _ = a.shape
    (kaa, kab, kbb), (t1, t2), (eaa, eab, ebb) = mmd_terms(a, b, c_used, sigma, weight)
    norm = 1.0 / (n * n * npos)
    s_abs = norm * (kaa + kbb + 2 * kab).sum()
    vb = norm * (kaa * eaa + kbb * ebb + 2 * kab * eab).sum() + (chain + 4) * EPS * s_abs
    # per term: the gaussian, the difference, 1 / sigma^2 (2), two products;
    # the adds over j and of T1 + T2 (n + 1); norm (3), weight, the product
    # with gscale; the add into d_a
    at1, at2 = np.abs(t1), np.abs(t2)
    ref = (t1 + t2).sum(axis=1)
    gb = (at1 * (eaa[..., None] + 5 * EPS) + at2 * (eab[..., None] + 5 * EPS)).sum(axis=1) + \
        (n + 6) * EPS * (at1 + at2).sum(axis=1)
    out = np.zeros_like(a)
    out[..., :c_used] = gb
    d0 = np.asarray(d0, np.float64)
    full = np.zeros_like(a)
    full[..., :c_used] = ref
    return HIGHER * vb, HIGHER * (out + EPS * (np.abs(d0) + np.abs(full)))


# ------------------------------------------------------------ sliced Wasserstein
def sliced_wasserstein(a, b, dirs, c_used, weight):
    """value and weight * d value / d a for the raw direction matrix ``dirs``
    (n_proj, n_pos); a, b = (n, n_pos, c_*).  torch.sort's gradient sends each
    sorted difference back to the projection it came from"""
    torch = _t()
    a = np.asarray(a, np.float64)
    at = torch.from_numpy(np.ascontiguousarray(a[..., :c_used])).requires_grad_(True)
    bt = torch.from_numpy(np.ascontiguousarray(np.asarray(b, np.float64)[..., :c_used]))
    pr = torch.from_numpy(np.asarray(dirs, np.float64).copy())
    pr = pr / torch.sqrt((pr ** 2).sum(dim=-1, keepdim=True))
    pa = torch.sort(torch.einsum('pl,nlc->npc', pr, at), dim=1).values
    pb = torch.sort(torch.einsum('pl,nlc->npc', pr, bt), dim=1).values
    val = ((pa - pb) ** 2).mean()
    val.backward()
    d = np.zeros_like(a)
    d[..., :c_used] = weight * at.grad.numpy()
    return float(val.detach()), d


def _sw_projections(x, dirs, c_used):
    """raw r[p, col], sum of |terms| R[p, col], non-zero terms per column;
    col = observation * c_used + channel"""
    x = np.asarray(x, np.float64)[..., :c_used]
    n, npos, _ = x.shape
    cols = np.moveaxis(x, 1, 0).reshape(npos, n * c_used)
    d = np.asarray(dirs, np.float64)
    return d @ cols, np.abs(d) @ np.abs(cols), (cols != 0).sum(axis=0)


def sw_bounds(a, b, dirs, c_used, weight, d0):
    """(bound of the value, bound of every d_a element (n, n_pos, c_a)):
    nnz + 8 roundings on a projection, n_pos / 2 + 10 on the squared norm (and
    on each factor 1 / |dir| made from it), n_proj + 8 on the back-projection,
    one on the add into d_a"""
    a = np.asarray(a, np.float64)
    n, npos, c_a = a.shape
    d = np.asarray(dirs, np.float64)
    P = d.shape[0]
    nv = n * c_used
    s = (d ** 2).sum(axis=1)[:, None]
    inv = 1 / np.sqrt(s)
    ra, Ra, nza = _sw_projections(a, d, c_used)
    rb, Rb, nzb = _sw_projections(b, d, c_used)
    en = (npos / 2 + 10) * EPS
    ea = inv * ((nza + 8) * EPS * Ra + np.abs(ra) * en)      # of a normalised projection
    eb = inv * ((nzb + 8) * EPS * Rb + np.abs(rb) * en)
    va, vb = ra * inv, rb * inv
    oa, ob = np.argsort(va, axis=0), np.argsort(vb, axis=0)
    rank = np.empty_like(oa)
    np.put_along_axis(rank, oa, np.arange(P)[:, None].repeat(nv, 1), axis=0)
    partner = np.take_along_axis(ob, rank, axis=0)           # b projection that a's p meets
    diff = va - np.take_along_axis(vb, partner, axis=0)
    ediff = ea + np.take_along_axis(eb, partner, axis=0)
    scale = weight * 2.0 / (nv * P)
    g = scale * diff * inv
    eg = scale * inv * ediff + np.abs(g) * en
    grad = np.abs(d).T @ eg + (P + 8) * EPS * (np.abs(d).T @ np.abs(g))   # (n_pos, nv)
    ref = d.T @ g
    out = np.zeros_like(a)
    out[..., :c_used] = np.moveaxis(grad.reshape(npos, n, c_used), 0, 1)
    full = np.zeros_like(a)
    full[..., :c_used] = np.moveaxis(ref.reshape(npos, n, c_used), 0, 1)
    value = (diff ** 2).sum() / (nv * P)
    # value: 2 |d| e(d) per term; chain of adds: P / 256 per lane, 8 tree
    # levels, the columns, three more for the norm
    vbnd = (2 * np.abs(diff) * ediff).sum() / (nv * P) + (P / 256 + nv + 12) * EPS * value
    return HIGHER * vbnd, HIGHER * (out + EPS * (np.abs(np.asarray(d0, np.float64)) + np.abs(full))), full


def sw_min_gap_ratio(x, dirs, c_used):
    """smallest, over the columns, of (gap between adjacent sorted normalised
    projections) / (sum of the two neighbours' projection error bounds,
    (n_pos + 4) 2^-24 sum |terms| each) — must exceed 1 for the ranks of the
    fp32 projections to be those of the reference"""
    d = np.asarray(dirs, np.float64)
    npos = d.shape[1]
    inv = 1 / np.sqrt((d ** 2).sum(axis=1))[:, None]
    r, R, _ = _sw_projections(x, d, c_used)
    v, e = r * inv, (npos + 4) * EPS * R * inv
    o = np.argsort(v, axis=0)
    vs, es = np.take_along_axis(v, o, axis=0), np.take_along_axis(e, o, axis=0)
    if vs.shape[0] < 2:
        return np.inf
    return float(((vs[1:] - vs[:-1]) / (es[1:] + es[:-1])).min())


# the zero-truth sliced-Wasserstein cases: n_proj, n_pos, n, c_used, positions
# of a that are not zero (None: all)
SW_ZERO_TRUTH = [(1, 7, 1, 1, None), (513, 462, 5, 5, None), (1024, 378, 17, 1, None),
                 (4096, 61, 2, 2, None), (33, 32768 + 300, 1, 3, 64), (33, 65536 + 300, 17, 1, 64)]


def sw_zero_truth_field(n_pos, n, nnz, c_a, seed=70):
    """the field of a zero-truth case: k / 4 values, in the long cases at 64
    positions only, the first and the last among them"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-32, 33, size=(n, n_pos, c_a)).astype(np.float64) / 4
    if nnz is not None:
        keep = np.zeros(n_pos, bool)
        keep[[0, n_pos - 1]] = True
        keep[rng.choice(np.arange(1, n_pos - 1), nnz - 2, replace=False)] = True
        a[:, ~keep, :] = 0
    return a
