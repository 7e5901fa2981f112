"""``tests/support_ref.py`` pinned on the CPU: every restated operation against
the oracle's own layer (``oracle/layers.py``, written from reshape / slicing,
where support_ref uses index maps) and by the dot-product identity
``<A x, y> == <x, A^T y>`` on random float64 data — the two restatements check
each other before either judges a kernel (tests/test_train_support_gpu.py)."""
import numpy as np
import pytest

from oracle import gan as G
from oracle import layers as OL
from oracle.network import Network as OracleNet
from tests import support_ref as R

RTOL = 1e-12


def _close(a, b):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=RTOL * max(1.0, float(np.abs(b).max())))


def _dot_identity(fwd, adj, x_shape, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(x_shape)
    ax = fwd(x)
    y = rng.standard_normal(ax.shape)
    aty = adj(y)
    assert aty.shape == x.shape
    lhs, rhs = float((ax * y).sum()), float((x * aty).sum())
    assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs)), (lhs, rhs)


PADS = [
    # (shape, lo, hi): widths 1, 2, 3, the asymmetric pad / crop pairs of
    # tests/test_ref_surface.py::PAD_CROP, extents down to lo + 1
    ((2, 5, 6, 4, 3), [1, 1, 1], [1, 1, 1]),
    ((1, 5, 6, 4, 2), [2, 2, 2], [2, 2, 2]),
    ((2, 6, 5, 4, 1), [3, 3, 3], [3, 3, 3]),
    ((2, 6, 5, 3, 3), [3, 3, 2], [2, 2, 1]),
    ((1, 4, 3, 2, 4), [3, 2, 1], [3, 2, 1]),       # every extent = lo + 1
    ((1, 4, 4, 3, 2), [3, 0, 2], [0, 3, 1]),
    ((3, 7, 5, 1, 2), [2, 1, 0], [1, 2, 0]),       # the 2-D case
]


@pytest.mark.parametrize('mode', ['reflect', 'constant'])
@pytest.mark.parametrize('shape,lo,hi', PADS)
def test_pad_and_its_adjoint(shape, lo, hi, mode):
    rng = np.random.default_rng(1)
    x = rng.standard_normal(shape)
    pads = [(0, 0)] + list(zip(lo, hi)) + [(0, 0)]
    np.testing.assert_array_equal(R.pad_fwd(x, lo, hi, mode), np.pad(x, pads, mode=mode))
    layer = OL.FlexiblePadding(pads, mode=mode.upper())
    yp = layer.forward(x)
    dy = rng.standard_normal(yp.shape)
    _close(R.pad_adj(dy, shape, lo, hi, mode), layer.backward(dy))
    _dot_identity(lambda v: R.pad_fwd(v, lo, hi, mode), lambda v: R.pad_adj(v, shape, lo, hi, mode), shape)


def test_reflect_index_map_repeats_no_edge_sample():
    np.testing.assert_array_equal(R.pad_index(4, 3, 2, 'reflect'), [3, 2, 1, 0, 1, 2, 3, 2, 1])
    np.testing.assert_array_equal(R.pad_index(3, 1, 2, 'constant'), [-1, 0, 1, 2, -1, -1])
    with pytest.raises(AssertionError):
        R.pad_index(3, 3, 0, 'reflect')     # wider than n - 1: not a legal reflect


@pytest.mark.parametrize('shape,lo,hi', [((2, 6, 5, 4, 3), [1, 1, 1], [1, 1, 1]),
                                         ((1, 7, 6, 5, 2), [2, 1, 2], [2, 2, 1]),
                                         ((2, 5, 5, 1, 4), [2, 0, 0], [1, 3, 0])])
def test_crop_and_its_adjoint(shape, lo, hi):
    rng = np.random.default_rng(2)
    x = rng.standard_normal(shape)
    layer = OL.Cropping(list(zip(lo, hi)), 3)
    y = layer.forward(x)
    np.testing.assert_array_equal(R.crop_fwd(x, lo, hi), y)
    dy = rng.standard_normal(y.shape)
    np.testing.assert_array_equal(R.crop_adj(dy, shape, lo, hi), layer.backward(dy))
    _dot_identity(lambda v: R.crop_fwd(v, lo, hi), lambda v: R.crop_adj(v, shape, lo, hi), shape)


@pytest.mark.parametrize('m,b,shape', [(3, 1, (2, 3, 4, 5, 2)), (1, 2, (2, 3, 4, 2, 8)),
                                       (2, 3, (1, 2, 3, 3, 18)), (1, 5, (1, 2, 2, 1, 50))])
def test_repeat_and_depth_to_space_and_their_adjoints(m, b, shape):
    rng = np.random.default_rng(3)
    x = rng.standard_normal(shape)
    layer = OL.SpatioTemporalExpansion(spatial_mult=b, temporal_mult=m)
    y = layer.forward(x)

    def fwd(v):
        v = R.repeat_t_fwd(v, m) if m > 1 else v
        return R.d2s_fwd(v, b) if b > 1 else v

    def adj(v):
        v = R.d2s_adj(v, b) if b > 1 else v
        return R.repeat_t_adj(v, m) if m > 1 else v
    np.testing.assert_array_equal(fwd(x), y)
    dy = rng.standard_normal(y.shape)
    _close(adj(dy), layer.backward(dy))
    _dot_identity(fwd, adj, shape)
    if m == 1:      # the 4-D layer is the t == 1 case
        l2 = OL.SpatialExpansion(spatial_mult=b)
        y2 = l2.forward(x[:, :, :, 0, :])
        np.testing.assert_array_equal(R.d2s_fwd(x[:, :, :, :1, :], b)[:, :, :, 0, :], y2)


def test_concat_and_its_adjoint():
    rng = np.random.default_rng(4)
    x, e = rng.standard_normal((2, 3, 4, 2, 5)), rng.standard_normal((2, 3, 4, 2, 1))
    layer = OL.Sup3rConcat('topo')
    y = layer.forward(x, e)
    np.testing.assert_array_equal(R.concat_fwd(x, e), y)
    dy = rng.standard_normal(y.shape)
    dx, de = R.concat_adj(dy, 5)
    np.testing.assert_array_equal(dx, layer.backward(dy))
    assert abs((y * dy).sum() - (x * dx).sum() - (e * de).sum()) < 1e-11


@pytest.mark.parametrize('slope', [0.0, 0.25, 1.0])
def test_activation_adjoint_follows_the_output_sign(slope):
    rng = np.random.default_rng(5)
    x = rng.integers(-3, 4, size=(2, 3, 4, 2, 5)).astype(np.float64)     # zeros included
    y = R.act_fwd(x, slope)
    dy = rng.standard_normal(x.shape)
    layer = OL.LeakyReLU(alpha=slope)
    np.testing.assert_array_equal(layer.forward(x), y)
    # the oracle decides from the pre-activation, the device (and support_ref)
    # from the output: the same wherever the slope is positive; for ReLU
    # (y == 0 for every x <= 0) both give 0
    np.testing.assert_array_equal(R.act_adj(y, dy, slope), layer.backward(dy))
    np.testing.assert_array_equal(R.act_adj(np.array([0.0, -0.0, 1.0, -1.0]), np.ones(4), slope),
                                  [slope, slope, 1.0, slope])
    np.testing.assert_array_equal(R.channel_sums(dy), dy.sum(axis=(0, 1, 2, 3)))


@pytest.mark.parametrize('nd,k,pad', [(3, 3, 'valid'), (3, 1, 'valid'), (2, 3, 'same'), (3, (3, 1, 2), 'same')])
def test_conv_and_its_two_adjoints(nd, k, pad):
    rng = np.random.default_rng(6)
    shape = (2, 5, 6, 3) if nd == 2 else (2, 5, 6, 4, 3)
    x = rng.standard_normal(shape)
    layer = OL.ConvND(nd, 4, k, padding=pad)
    y = layer.forward(x)
    layer.kernel = rng.standard_normal(layer.kernel.shape)
    layer.bias = rng.standard_normal(layer.bias.shape)
    y = layer.forward(x)
    net = R.RefNet([{'class': f'Conv{nd}D', 'filters': 4, 'kernel_size': k, 'padding': pad}], nd)
    net.set_weights([layer.kernel, layer.bias])
    _close(net.forward(x), y)
    dy = rng.standard_normal(y.shape)
    dx_o = layer.backward(dy)
    dx = net.backward(dy)
    _close(dx, dx_o)
    for a, b in zip(net.grads, layer.grads):
        _close(a, b)
    w5 = net._kernel5(net.weights[0])
    xp = R.to5(x) if pad == 'valid' else None
    if xp is not None:
        _dot_identity(lambda v: R.conv_fwd(v, w5), lambda v: R.conv_adj_x(v, w5, xp.shape), xp.shape)
        # linear in w too: <conv(x, w), dy> == <w, conv_adj_w(x, dy)>
        lhs = float((R.conv_fwd(xp, w5) * R.to5(dy)).sum())
        rhs = float((w5 * R.conv_adj_w(xp, R.to5(dy), w5.shape[:3])).sum())
        assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


def test_same_padding_of_a_strided_conv_puts_the_smaller_half_in_front():
    assert R.same_pad(8, 3, 2) == (0, 1)        # even extent: nothing in front, one zero cell past the end
    assert R.same_pad(7, 3, 2) == (1, 1)        # odd extent: one cell either side
    assert R.same_pad(7, 3, 1) == (1, 1) and R.same_pad(7, 1, 2) == (0, 0)
    assert R.same_pad(6, 2, 3) == (0, 0) and R.same_pad(5, 4, 3) == (1, 1) and R.same_pad(4, 4, 3) == (1, 2)
    assert [R.conv_out(n, 3, 2) for n in (3, 4, 5, 6)] == [1, 1, 2, 2]


STRIDED = [
    # nd, spatial extents, strides, padding: k = 3, s = 2 on odd and even
    # extents, both paddings, 2-D and 3-D; one stride per axis
    (3, (7, 8, 9), 2, 'valid'), (3, (8, 7, 6), 2, 'valid'),
    (3, (7, 9, 5), 2, 'same'), (3, (8, 6, 10), 2, 'same'), (3, (7, 8, 5), 2, 'same'),
    (2, (7, 8), 2, 'valid'), (2, (9, 6), 2, 'same'), (2, (8, 7), 2, 'same'),
    (3, (7, 8, 9), (2, 1, 2), 'same'), (3, (9, 8, 7), (1, 2, 3), 'valid'),
]


@pytest.mark.parametrize('nd,sp,strides,pad', STRIDED)
def test_strided_conv_and_its_two_adjoints(nd, sp, strides, pad):
    rng = np.random.default_rng(12)
    shape = (2,) + sp + (3,)
    x = rng.standard_normal(shape)
    layer = OL.ConvND(nd, 4, 3, strides=strides, padding=pad)
    layer.forward(x)
    layer.kernel = rng.standard_normal(layer.kernel.shape)
    layer.bias = rng.standard_normal(layer.bias.shape)
    y = layer.forward(x)
    net = R.RefNet([{'class': f'Conv{nd}D', 'filters': 4, 'kernel_size': 3, 'strides': strides, 'padding': pad}], nd)
    net.set_weights([layer.kernel, layer.bias])
    y_net = net.forward(x)
    assert y_net.shape == y.shape
    _close(y_net, y)
    dy = rng.standard_normal(y.shape)
    dx_o = layer.backward(dy)
    _close(net.backward(dy), dx_o)
    for a, b in zip(net.grads, layer.grads):
        _close(a, b)
    # the tape records the GPU tests read: the padded input and dL / d(conv output)
    rec = [r for r in net._tape if r[0] == 'conv'][0]
    st = R._strides3(strides, nd)
    lo, hi = rec[2], rec[3]
    assert rec[4].shape[1:4] == tuple(n + a + b for n, a, b in zip(R.to5(x).shape[1:4], lo, hi))
    np.testing.assert_array_equal(net.dpre[0], R.to5(dy))
    # ... and the three operations on their own, by the dot-product identities
    w5, xp = net._kernel5(net.weights[0]), rec[4]
    _dot_identity(lambda v: R.conv_fwd(v, w5, strides=st), lambda v: R.conv_adj_x(v, w5, xp.shape, st), xp.shape)
    lhs = float((R.conv_fwd(xp, w5, strides=st) * R.to5(dy)).sum())
    rhs = float((w5 * R.conv_adj_w(xp, R.to5(dy), w5.shape[:3], st)).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


NETS = [
    # a residual block with reflect convs, a skip tensor with two consumers, a
    # depth-to-space conv, pad / crop
    (3, (2, 5, 6, 4, 2), [
        {'class': 'FlexiblePadding', 'paddings': [[0, 0], [1, 1], [1, 1], [1, 1], [0, 0]], 'mode': 'REFLECT'},
        {'class': 'Conv3D', 'filters': 8, 'kernel_size': 3}, {'class': 'LeakyReLU', 'alpha': 0.25},
        {'class': 'SkipConnection', 'name': 'a'},
        {'class': 'FlexiblePadding', 'paddings': [[0, 0], [1, 1], [1, 1], [1, 1], [0, 0]], 'mode': 'REFLECT'},
        {'class': 'Conv3D', 'filters': 8, 'kernel_size': 3}, {'class': 'ReLU'},
        {'class': 'FlexiblePadding', 'paddings': [[0, 0], [1, 1], [1, 1], [1, 1], [0, 0]], 'mode': 'REFLECT'},
        {'class': 'Conv3D', 'filters': 8, 'kernel_size': 3},
        {'class': 'SkipConnection', 'name': 'a'},
        {'class': 'SpatioTemporalExpansion', 'temporal_mult': 2, 'temporal_method': 'nearest'},
        {'class': 'Conv3D', 'filters': 8, 'kernel_size': 1},
        {'class': 'SpatioTemporalExpansion', 'spatial_mult': 2}, {'class': 'LeakyReLU', 'alpha': 0.25},
        {'class': 'FlexiblePadding', 'paddings': [[0, 0], [3, 3], [3, 3], [2, 2], [0, 0]], 'mode': 'REFLECT'},
        {'class': 'Cropping3D', 'cropping': [[2, 2], [2, 2], [1, 1]]},
        {'class': 'Conv3D', 'filters': 3, 'kernel_size': 3, 'padding': 'same', 'use_bias': False}]),
    (2, (3, 7, 5, 3), [
        {'class': 'Conv2D', 'filters': 16, 'kernel_size': 3, 'padding': 'same'},
        {'class': 'SpatialExpansion', 'spatial_mult': 2}, {'class': 'ReLU'},
        {'class': 'SkipConnection', 'name': 's'},
        {'class': 'Conv2D', 'filters': 4, 'kernel_size': 1},
        {'class': 'SkipConnection', 'name': 's'},
        {'class': 'Cropping2D', 'cropping': [[1, 0], [2, 1]]},
        {'class': 'FlexiblePadding', 'paddings': [[0, 0], [2, 1], [0, 2], [0, 0]], 'mode': 'CONSTANT'},
        {'class': 'Conv2D', 'filters': 2, 'kernel_size': 1}]),
    # the discriminator's front: valid / stride-2 / 'same' stride-2 convs chained
    # (last, so that the ids of the cases above stay what they were)
    (3, (2, 13, 12, 15, 2), [
        {'class': 'Conv3D', 'filters': 8, 'kernel_size': 3, 'strides': 1, 'padding': 'valid'},
        {'class': 'LeakyReLU', 'alpha': 0.25},
        {'class': 'Conv3D', 'filters': 8, 'kernel_size': 3, 'strides': 2, 'padding': 'valid'},
        {'class': 'ReLU'},
        {'class': 'Conv3D', 'filters': 6, 'kernel_size': 3, 'strides': 2, 'padding': 'same'},
        {'class': 'LeakyReLU', 'alpha': 0.5},
        {'class': 'Conv3D', 'filters': 4, 'kernel_size': 3, 'strides': 1, 'padding': 'same', 'use_bias': False}]),
]


@pytest.mark.parametrize('nd,shape,spec', NETS)
def test_chain_matches_the_oracle_network(nd, shape, spec):
    rng = np.random.default_rng(7)
    x = rng.standard_normal(shape)
    ref = OracleNet(spec)
    ref.init_weights(x, seed=3, bias_scale=0.2)
    ref.cast(np.float64)
    y_ref = ref.forward(x)
    net = R.RefNet(spec, nd)
    net.set_weights(ref.weights)
    y = net.forward(x)
    _close(y, y_ref)
    dy = rng.standard_normal(y_ref.shape)
    _close(net.backward(dy), ref.backward(dy))
    assert len(net.grads) == len(ref.grads)
    for a, b in zip(net.grads, ref.grads):
        _close(a, b)


def test_concat_in_a_chain():
    spec = [{'class': 'Conv2D', 'filters': 3, 'kernel_size': 1},
            {'class': 'Sup3rConcat', 'name': 'topo'},
            {'class': 'Conv2D', 'filters': 2, 'kernel_size': 3, 'padding': 'same'}]
    rng = np.random.default_rng(8)
    x, e = rng.standard_normal((2, 4, 5, 2)), rng.standard_normal((2, 4, 5, 1))
    ref = OracleNet(spec)
    ref.init_weights(x, exo={'topo': e}, seed=3, bias_scale=0.2)
    ref.cast(np.float64)
    net = R.RefNet(spec, 2)
    net.set_weights(ref.weights)
    y_ref = ref.forward(x, {'topo': e})
    _close(net.forward(x, {'topo': e}), y_ref)
    dy = rng.standard_normal(y_ref.shape)
    _close(net.backward(dy), ref.backward(dy))
    for a, b in zip(net.grads, ref.grads):
        _close(a, b)


@pytest.mark.parametrize('kind,fn', [('mae', G.mae), ('mse', G.mse)])
def test_content_loss_against_the_oracle(kind, fn):
    rng = np.random.default_rng(9)
    a, b = rng.standard_normal((3, 4, 5, 2)), rng.standard_normal((3, 4, 5, 3))
    val, grad = R.content_loss(kind, a, b, c_used=2, weight=0.5)
    ref_l, ref_g, _ = fn(a, b[..., :2])
    assert abs(val - ref_l) < 1e-14
    _close(grad, 0.5 * ref_g)


@pytest.mark.parametrize('kind', ['mae', 'mse', 'exp'])
def test_content_loss_gradient_is_the_derivative(kind):
    """channel subset + mask: central differences of the value (the mask
    multiplies d, so it enters the gradient once more)"""
    rng = np.random.default_rng(10)
    a, b = rng.standard_normal((2, 3, 4, 5)), rng.standard_normal((2, 3, 4, 3))
    mask = rng.integers(0, 3, size=(2, 3, 4, 4)).astype(np.float64) / 2
    val, grad = R.content_loss(kind, a, b, c_used=3, mask=mask, weight=2.0)
    assert np.all(grad[..., 3:] == 0)
    v = rng.standard_normal(a.shape)
    h = 1e-6
    up = R.content_loss(kind, a + h * v, b, c_used=3, mask=mask)[0]
    dn = R.content_loss(kind, a - h * v, b, c_used=3, mask=mask)[0]
    assert abs(2.0 * (up - dn) / (2 * h) - (grad * v).sum()) < 1e-7


@pytest.mark.parametrize('n', [1, 15, 257])
def test_rel_bce_against_the_oracle_and_its_derivative(n):
    rng = np.random.default_rng(11)
    dt, dg = rng.standard_normal((n, 1)) * 3, rng.standard_normal((n, 1)) * 3
    loss, gt, gg = R.rel_bce(dt, dg)
    rl, rt, rg = G.rel_bce(dt, dg)
    assert abs(loss - rl) < 1e-14
    _close(gt, rt[:, 0])
    _close(gg, rg[:, 0])
    v, u, h = rng.standard_normal(n), rng.standard_normal(n), 1e-6
    up = R.rel_bce(dt[:, 0] + h * v, dg[:, 0] + h * u)[0]
    dn = R.rel_bce(dt[:, 0] - h * v, dg[:, 0] - h * u)[0]
    assert abs((up - dn) / (2 * h) - (gt * v).sum() - (gg * u).sum()) < 1e-8
