"""Float64 numpy restatement of the training step's support passes (TEST
INFRASTRUCTURE): the adjoints of pad / crop / temporal repeat / depth-to-space /
concat, the activation adjoint with the device's convention, channel sums, a
tap-loop convolution with its two adjoints, the content losses and the
relativistic BCE.

Written from the definitions of the operations (index maps + ``np.add.at``),
not from ``oracle/``: ``tests/test_support_ref_cpu.py`` pins the two
restatements against each other before either judges a kernel.  Tensors are
channels-last 5-D ``(N, s1, s2, t, C)`` like the device's; a 4-D keras tensor is
the ``t == 1`` case (``to5`` / ``from5``).
"""
import numpy as np

F64 = np.float64


def to5(x):
    x = np.asarray(x, F64)
    return x[:, :, :, None, :] if x.ndim == 4 else x


def from5(x, nd):
    return x[:, :, :, 0, :] if nd == 2 else x


# ------------------------------------------------------------------ pad
def pad_index(n, lo, hi, mode):
    """source index of every cell of the padded axis; -1 = a zero cell.
    'reflect' mirrors about the edge samples without repeating them (period
    2 (n - 1)), 'constant' pads zeros."""
    j = np.arange(-lo, n + hi)
    if mode == 'constant':
        return np.where((j >= 0) & (j < n), j, -1)
    assert mode == 'reflect'
    if lo == 0 and hi == 0:
        return j
    assert n >= 2 and lo <= n - 1 and hi <= n - 1, (n, lo, hi)
    p = 2 * (n - 1)
    j = np.mod(j, p)
    return np.where(j >= n, p - j, j)


def pad_fwd(x, lo, hi, mode):
    for d in range(3):
        idx = pad_index(x.shape[1 + d], lo[d], hi[d], mode)
        y = np.take(x, np.maximum(idx, 0), axis=1 + d)
        sh = [1] * 5
        sh[1 + d] = len(idx)
        x = y * (idx >= 0).reshape(sh)
    return x


def pad_adj(dy, in_shape, lo, hi, mode):
    """adjoint of ``pad_fwd``: scatter-add through the same index map"""
    for d in range(3):
        n = in_shape[1 + d]
        idx = pad_index(n, lo[d], hi[d], mode)
        assert dy.shape[1 + d] == len(idx)
        src = np.moveaxis(dy, 1 + d, 0)
        out = np.zeros((n,) + src.shape[1:], F64)
        keep = idx >= 0
        np.add.at(out, idx[keep], src[keep])
        dy = np.moveaxis(out, 0, 1 + d)
    return dy


# ----------------------------------------------------------------- crop
def crop_fwd(x, lo, hi):
    s = x.shape
    return x[:, lo[0]:s[1] - hi[0], lo[1]:s[2] - hi[1], lo[2]:s[3] - hi[2], :]


def crop_adj(dy, in_shape, lo, hi):
    dx = np.zeros(in_shape, F64)
    s = in_shape
    dx[:, lo[0]:s[1] - hi[0], lo[1]:s[2] - hi[1], lo[2]:s[3] - hi[2], :] = dy
    return dx


# ------------------------------------------------- temporal nearest repeat
def repeat_t_fwd(x, m):
    return np.take(x, np.arange(x.shape[3] * m) // m, axis=3)


def repeat_t_adj(dy, m):
    t = dy.shape[3] // m
    out = np.zeros((t,) + dy.shape[:3] + dy.shape[4:], F64)
    np.add.at(out, np.arange(t * m) // m, np.moveaxis(dy, 3, 0))
    return np.moveaxis(out, 0, 3)


# ------------------------------------------------- depth-to-space (DCR)
def d2s_fwd(x, b):
    """out[n, h b + i, w b + j, t, c] = in[n, h, w, t, (i b + j) C' + c]"""
    n, h, w, t, c = x.shape
    co = c // (b * b)
    y = np.zeros((n, h * b, w * b, t, co), F64)
    for i in range(b):
        for j in range(b):
            y[:, i::b, j::b] = x[..., (i * b + j) * co:(i * b + j + 1) * co]
    return y


def d2s_adj(dy, b):
    n, hb, wb, t, co = dy.shape
    dx = np.zeros((n, hb // b, wb // b, t, co * b * b), F64)
    for i in range(b):
        for j in range(b):
            dx[..., (i * b + j) * co:(i * b + j + 1) * co] = dy[:, i::b, j::b]
    return dx


# --------------------------------------------------------------- concat
def concat_fwd(x, e):
    return np.concatenate([x, e], axis=-1)


def concat_adj(dy, nx):
    return dy[..., :nx], dy[..., nx:]


# ----------------------------------------------------------- activation
def act_fwd(x, slope):
    """slope 0 = ReLU, 1 = identity, else LeakyReLU"""
    return np.where(x > 0, x, slope * x)


def act_adj(y, dy, slope):
    """the device's convention: decided from the OUTPUT, ``y > 0 ? 1 : slope``
    (a zero or negative-zero output takes the slope)"""
    return dy * np.where(np.asarray(y) > 0, 1.0, slope)


def channel_sums(a):
    return np.asarray(a, F64).reshape(-1, a.shape[-1]).sum(axis=0)


# ----------------------------------------------------------------- conv
def _strides3(strides, nd=3):
    """an int (for each of the conv's nd axes) or one stride per axis; the t
    axis of a 2-D conv has stride 1"""
    if isinstance(strides, (int, np.integer)):
        strides = (int(strides),) * nd
    st = tuple(int(v) for v in strides)
    return st + (1,) * (3 - len(st))


def _taps(xp_shape, k, o, st):
    """(tap, the slices of the padded input its o outputs read) of a strided
    'valid' correlation: output i of an axis reads cell i * stride + tap"""
    for a in range(k[0]):
        for b in range(k[1]):
            for c in range(k[2]):
                yield (a, b, c), (slice(None),) + tuple(
                    slice(q, q + (o[d] - 1) * st[d] + 1, st[d]) for d, q in enumerate((a, b, c)))


def conv_out(n, k, s=1):
    """outputs of a 'valid' correlation with stride s over n (padded) cells"""
    return (n - k) // s + 1


def conv_fwd(xp, w, bias=None, strides=1):
    """'valid' correlation over an already padded input, stride 1 or
    ``strides`` (an int or per axis).  w: (k0, k1, k2, C_in, C_out)"""
    k, st = w.shape[:3], _strides3(strides)
    o = [conv_out(xp.shape[1 + d], k[d], st[d]) for d in range(3)]
    y = np.zeros((xp.shape[0], o[0], o[1], o[2], w.shape[4]), F64)
    for tap, sl in _taps(xp.shape, k, o, st):
        y += xp[sl] @ w[tap]
    return y if bias is None else y + bias


def conv_adj_x(dy, w, xp_shape, strides=1):
    k, st = w.shape[:3], _strides3(strides)
    o = dy.shape[1:4]
    dxp = np.zeros(xp_shape, F64)
    for tap, sl in _taps(xp_shape, k, o, st):
        dxp[sl] += dy @ w[tap].T
    return dxp


def conv_adj_w(xp, dy, k, strides=1):
    st = _strides3(strides)
    o = dy.shape[1:4]
    dw = np.zeros(tuple(k) + (xp.shape[4], dy.shape[4]), F64)
    d2 = dy.reshape(-1, dy.shape[4])
    for tap, sl in _taps(xp.shape, k, o, st):
        dw[tap] = xp[sl].reshape(-1, xp.shape[4]).T @ d2
    return dw


def same_pad(n, k, s=1):
    """TF 'same': ceil(n / s) outputs; total pad = max((ceil(n / s) - 1) s + k
    - n, 0), the smaller half in front"""
    total = max((-(-n // s) - 1) * s + k - n, 0)
    return total // 2, total - total // 2


# ------------------------------------------------- a chain of these ops
def _pairs(v, nd):
    if isinstance(v, (int, np.integer)):
        v = [(int(v), int(v))] * nd
    out = [(int(p), int(p)) if isinstance(p, (int, np.integer))
           else (int(p[0]), int(p[1])) for p in v]
    return out + [(0, 0)] * (3 - len(out))


class RefNet:
    """Eager float64 forward / reverse-mode backward of a ``hidden_layers``
    list restricted to the classes the support-pass tests use: FlexiblePadding,
    Conv2D / Conv3D ('valid' / 'same', any stride), LeakyReLU, ReLU, SkipConnection, Cropping2D /
    3D, SpatialExpansion, SpatioTemporalExpansion (nearest), Sup3rConcat.
    Weights are keras-layout arrays in keras order (kernel, bias per conv)."""

    def __init__(self, spec, nd):
        self.nd = nd
        self.spec = [dict(s) for s in spec]
        self.weights = None

    def conv_specs(self):
        return [s for s in self.spec if s['class'] in ('Conv2D', 'Conv3D')]

    def set_weights(self, arrays):
        self.weights = [np.asarray(a, F64) for a in arrays]

    def _kernel5(self, w):
        return w[:, :, None] if self.nd == 2 else w

    def forward(self, x, exo=None):
        x = to5(x)
        tape, skips, wi = [], {}, 0
        for s in self.spec:
            cls = s['class']
            if cls == 'FlexiblePadding':
                p = _pairs(s['paddings'][1:-1], self.nd)
                lo, hi = [q[0] for q in p], [q[1] for q in p]
                mode = s.get('mode', 'REFLECT').lower()
                tape.append(('pad', x.shape, lo, hi, mode))
                x = pad_fwd(x, lo, hi, mode)
            elif cls in ('Conv2D', 'Conv3D'):
                w = self._kernel5(self.weights[wi])
                wi += 1
                b = None
                if s.get('use_bias', True):
                    b = self.weights[wi]
                    wi += 1
                lo = hi = [0, 0, 0]
                st = _strides3(s.get('strides', 1), self.nd)
                if s.get('padding', 'valid') == 'same':
                    sp = [same_pad(x.shape[1 + d], w.shape[d], st[d]) for d in range(3)]
                    lo, hi = [q[0] for q in sp], [q[1] for q in sp]
                xp = pad_fwd(x, lo, hi, 'constant')
                # (a strided conv may leave the last cells of xp unread: they
                # take no part in either adjoint)
                tape.append(('conv', x.shape, lo, hi, xp, w, b is not None, st))
                x = conv_fwd(xp, w, b, st)
            elif cls in ('LeakyReLU', 'ReLU'):
                slope = float(s.get('alpha', 0.3)) if cls == 'LeakyReLU' else 0.0
                x = act_fwd(x, slope)
                tape.append(('act', x, slope))
            elif cls == 'SkipConnection':
                if s['name'] in skips:
                    x = x + skips.pop(s['name'])
                    tape.append(('skip_end', s['name']))
                else:
                    skips[s['name']] = x
                    tape.append(('skip_start', s['name']))
            elif cls in ('Cropping2D', 'Cropping3D'):
                p = _pairs(s.get('cropping', 0), self.nd)
                lo, hi = [q[0] for q in p], [q[1] for q in p]
                tape.append(('crop', x.shape, lo, hi))
                x = crop_fwd(x, lo, hi)
            elif cls in ('SpatialExpansion', 'SpatioTemporalExpansion'):
                m, b = int(s.get('temporal_mult', 1)), int(s.get('spatial_mult', 1))
                assert s.get('temporal_method', 'nearest') == 'nearest'
                if m > 1:
                    tape.append(('repeat', m))
                    x = repeat_t_fwd(x, m)
                if b > 1:
                    tape.append(('d2s', b))
                    x = d2s_fwd(x, b)
            elif cls == 'Sup3rConcat':
                tape.append(('concat', x.shape[-1]))
                x = concat_fwd(x, to5(exo[s['name']]))
            else:
                raise KeyError(cls)
        self._tape = tape
        return from5(x, self.nd)

    def backward(self, dy):
        """-> dx; ``self.grads`` in keras order, ``self.dpre`` = dL/d(conv
        output) per conv in layer order"""
        dy = to5(dy)
        grads, dpre, pend = [], [], {}
        for rec in reversed(self._tape):
            kind = rec[0]
            if kind == 'pad':
                dy = pad_adj(dy, rec[1], rec[2], rec[3], rec[4])
            elif kind == 'conv':
                _, in_shape, lo, hi, xp, w, has_b, st = rec
                g = [conv_adj_w(xp, dy, w.shape[:3], st)]
                if self.nd == 2:
                    g[0] = g[0][:, :, 0]
                if has_b:
                    g.append(channel_sums(dy))
                grads = g + grads
                dpre.insert(0, dy)
                dy = pad_adj(conv_adj_x(dy, w, xp.shape, st), in_shape, lo, hi,
                             'constant')
            elif kind == 'act':
                dy = act_adj(rec[1], dy, rec[2])
            elif kind == 'skip_end':
                pend[rec[1]] = dy
            elif kind == 'skip_start':
                if rec[1] in pend:        # (a start without an end joins nothing)
                    dy = dy + pend.pop(rec[1])
            elif kind == 'crop':
                dy = crop_adj(dy, rec[1], rec[2], rec[3])
            elif kind == 'repeat':
                dy = repeat_t_adj(dy, rec[1])
            elif kind == 'd2s':
                dy = d2s_adj(dy, rec[1])
            elif kind == 'concat':
                dy, self.d_exo = concat_adj(dy, rec[1])
        self.grads, self.dpre = grads, dpre
        return from5(dy, self.nd)


# --------------------------------------------------------------- losses
def content_loss(kind, a, b, c_used=None, mask=None, weight=1.0):
    """mean over the first ``c_used`` channels of |d|, d^2 or 1 - exp(-d^2)
    with d = (a - b) * mask; -> (weight-free value, weight * d value / d a with
    a's channel count, zero in the unused channels)"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    c = a.shape[-1] if c_used is None else c_used
    mk = 1.0 if mask is None else np.asarray(mask, F64)[..., :c]
    d = (a[..., :c] - b[..., :c]) * mk
    n = d.size
    if kind == 'mae':
        val, g = np.abs(d).sum() / n, np.sign(d)
    elif kind == 'mse':
        val, g = (d * d).sum() / n, 2.0 * d
    elif kind == 'exp':
        e = np.exp(-d * d)
        val, g = (1.0 - e).sum() / n, 2.0 * d * e
    else:
        raise KeyError(kind)
    grad = np.zeros(a.shape, F64)
    grad[..., :c] = g * mk * (weight / n)
    return val, grad


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def rel_bce(dt, dg):
    """mean of the sigmoid cross entropy of [dt - mean(dg); dg - mean(dt)]
    against the labels [1; 0] -> (loss, d loss / d dt, d loss / d dg)"""
    dt, dg = np.asarray(dt, F64).ravel(), np.asarray(dg, F64).ravel()
    n = dt.size
    xt, xf = dt - dg.mean(), dg - dt.mean()
    loss = (_softplus(-xt).sum() + _softplus(xf).sum()) / (2 * n)
    gt = (_sigmoid(xt) - 1.0) / (2 * n)       # d loss / d xt
    gf = _sigmoid(xf) / (2 * n)               # d loss / d xf
    return loss, gt - gf.sum() / n, gf - gt.sum() / n
