#!/usr/bin/env python
"""Bit-level fingerprint of the backward pass: for a fixed list of cases (every
shape is one the test suite or bench.py already runs) forward + backward from
fixed seeds, and per case the kernel selection of every conv plus the sha256
of y, dx and every gradient tensor.  No kernel uses atomics and every
reduction has a fixed order, so two builds of the library that launch the same
kernels with the same arguments write byte-identical files:

  SUP3R_AMD_LIB=<other build> python tools/backward_digest.py --out a.json
  python tools/backward_digest.py --out b.json && cmp a.json b.json

Also prints which weight / data gradient kernels the cases reach."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORCE = {'HALO32_MIN_TILES': 1, 'FEWCH_HALO_MIN_TILES': 1, 'DGRAD_S2_MIN_TILES': 1,
         'PERSIST_DGRAD_MIN_TILES': 1, 'HALO_S2_MIN_TILES': 1}
ALONE = ('NO_MASK_FUSE', 'NO_BIAS_FUSE', 'NO_FOLD16', 'NO_PLAIN_FOLD16', 'NO_DPRE16', 'NO_DPRE16_ONLY_MASK')
# every Wgrad / Dgrad of csrc/plan_internal.h; s3_plan_op_info merges some of them:
# told apart below by the precision (x3), the op's padding (chunked) and the
# fewpos_mfma / forward-kernel fields (approximate for fewpos and gen)
WGRADS = ('direct', 'fewpos_mfma', 'fewpos', 'tail', 'c2', 'bf16_trunk', 'f32_trunk', 'bf16_gen', 'bf16_2d', 'f32_gen')
DGRADS = ('direct', 'mfma_frame', 'mfma_valid', 'gen', 'fewch_frame', 'chunked_frame', 'chunked_valid', 'c2', 'c2_x3',
          's2', 's2_x3', 'gconv', 'fewpos_mfma', 'fewpos')


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def selection(ph, precision):
    from sup3r_amd import spec as S
    out = []
    for i, op in enumerate(ph.plan.ops):
        if op['kind'] != S.OP_CONV:
            continue
        d = ph.op_info(i)
        w, g = d['wgrad'], d['dgrad']
        if 'fewpos' in (w, g) and d['fewpos_mfma']:
            w, g = (x + '_mfma' if x == 'fewpos' else x for x in (w, g))
        if g in ('c2', 's2') and precision == 'bf16x3':
            g += '_x3'
        if g == 'mfma_chunked':
            g = 'chunked_frame' if any(op['lo']) else 'chunked_valid'
        if g == 'mfma_frame' and d['fwd'] in ('mfma_gen', 'conv2d_ws', 'conv2d_head'):
            g = 'gen'
        out.append([i, d['fwd'], w, g])
    return out


def fwd_bwd(spec, shape, precision, seed, exo_name=None, options=None, need_dx=True):
    from sup3r_amd.engine import Network
    rng = np.random.default_rng(seed)
    net = Network(spec, precision=precision)
    net.build(shape, seed=seed)
    net.set_weights([w if w.ndim > 1 else (0.1 * rng.standard_normal(w.shape)).astype(np.float32)
                     for w in (np.array(w) for w in net.weights)])
    ph = net.plan(shape, training=True, options=options)
    dev = net.dev
    exo = {}
    if exo_name:
        sh = ph.plan.tensors[ph.plan.inputs[exo_name]]
        sh = tuple(sh) if ph.plan.out_rank == 5 else (sh[0], sh[1], sh[2], sh[4])
        exo = {exo_name: dev.to_device(rng.standard_normal(sh).astype(np.float32))}
    y = ph.forward(dev.to_device(rng.standard_normal(shape).astype(np.float32)), exo)
    dy = dev.to_device(rng.standard_normal(tuple(y.shape)).astype(np.float32))
    dx = ph.backward(dy, need_dx=need_dx)
    res = {'sel': selection(ph, precision), 'y': sha(y.cpu().numpy()),
           'dx': sha(dx.cpu().numpy()) if need_dx else None, 'grads': [sha(g) for g in net.grads]}
    ph.backward(dy, need_dx=need_dx, accumulate_wgrad=True)   # a second shard adds into dW / db
    res['grads_acc'] = [sha(g) for g in net.grads]
    net.clear_plans()
    return res


def train(config, batch, steps=2):
    import types
    import torch
    import bench
    from sup3r_amd import Sup3rCondMom, Sup3rGan
    from sup3r_amd.engine import Device
    Sup3rGan.seed(7)
    dev, rng = Device.get(), np.random.default_rng(3)
    if config == 'c5base':
        model, lr_s, hr_s = Sup3rCondMom(os.path.join(bench.CFGDIR, 'gen_3x_4x_2f.json'), precision='bf16'), \
            (4, 4, 4, 2), (12, 12, 16, 2)
    else:
        model, lr_s, hr_s = bench.train_models(config)[:3]
    model.init_weights((batch,) + lr_s, (batch,) + hr_s)
    losses = []
    for _ in range(steps):
        lr = dev.to_device(rng.standard_normal((batch,) + lr_s).astype(np.float32))
        hr = dev.to_device(rng.standard_normal((batch,) + hr_s).astype(np.float32))
        if config == 'c5base':
            b = types.SimpleNamespace(low_res=lr, output=hr, mask=dev.to_device(np.ones((batch,) + hr_s, np.float32)))
            losses.append(float(model._train_step(b).resolve()['loss_gen']))
        else:
            b = types.SimpleNamespace(low_res=lr, high_res=hr)
            d = model._train_batch(b, True, False, False, True, False, False, 1e-3)
            losses.append([float(d['loss_gen']), float(d['loss_disc'])])
    torch.cuda.synchronize()
    nets = [model.generator] + ([model.discriminator] if getattr(model, '_disc', None) is not None else [])
    res = {'losses': losses, 'weights': [sha(np.array(w)) for n in nets for w in n.weights],
           'sel': [s for n in nets for ph in n._plans.values() if ph.training for s in selection(ph, 'bf16')]}
    del model
    torch.cuda.empty_cache()
    return res


def fuzz_nets():
    from sup3r_amd.configs.author_configs import pcc
    from tools.fuzz_paths import conv

    def block(name):
        return [{'class': 'SkipConnection', 'name': name}] + pcc(3, 64) + pcc(3, 64, act=False) + \
            [{'class': 'SkipConnection', 'name': name}]
    return [   # (name, spec, a shape some test runs this network class at)
        ('disc_stack', conv(32) + conv(32, 2) + conv(64) + [{'class': 'Flatten'}, {'class': 'Dense', 'units': 1}],
         (2, 27, 33, 77, 2)),
        ('gen_tail', pcc(3, 64) + pcc(3, 64) + pcc(3, 200, act=False) +
         [{'class': 'SpatioTemporalExpansion', 'spatial_mult': 5}, {'alpha': 0.2, 'class': 'LeakyReLU'}] +
         pcc(3, 2, act=False), (4, 8, 8, 32, 4)),
        ('trunk', pcc(3, 64) + block('b') + block('c') + pcc(3, 2, act=False), (2, 9, 10, 37, 4)),
        ('disc_prod', conv(32) + conv(32, 2) + conv(64) + conv(64, 2) + conv(128) + conv(128, 2) +
         [{'class': 'Flatten'}, {'class': 'Dense', 'units': 16}, {'alpha': 0.2, 'class': 'LeakyReLU'},
          {'class': 'Dense', 'units': 1}], (2, 64, 64, 112, 2))]


def cases():
    from tests.test_parity_r04 import _fewpos_specs
    from tests.test_ref_surface import CASES, load_surface
    for rel in sorted(CASES):
        shape, exo = CASES[rel]
        for prec in ('f32', 'bf16', 'bf16x3'):
            for dx in (True, False):
                yield f'surface/{rel}/{prec}/dx{int(dx)}', lambda s=load_surface(rel), sh=shape, p=prec, e=exo, dx=dx: \
                    fwd_bwd(s, sh, p, 41, exo_name=e, need_dx=dx)
    # (the few-time-step trunk at a batch that fills the persistent data gradient)
    yield 'surface/solar_1x_8x_1f/b8', lambda: fwd_bwd(
        load_surface('sup3rcc/gen_solar_1x_8x_1f.json'), (8, 54, 54, 3, 3), 'bf16', 2, need_dx=False)
    for name, spec, shape in _fewpos_specs():
        for prec in ('f32', 'bf16'):
            for nofuse in (0, 1):
                for side in (0, 1):
                    opt = dict({'NO_FEWPOS_BWD_FUSE': 1} if nofuse else {}, **({'WGRAD_SIDE_STREAM': 1} if side else {}))
                    yield f'fewpos/{name}/{prec}/nofuse{nofuse}/side{side}', \
                        lambda s=spec, sh=shape, p=prec, o=opt: fwd_bwd(s, sh, p, 11, options=o)
    for name, spec, shape in fuzz_nets():
        for extra in (None,) + ALONE:
            opt = dict(FORCE, **({extra: 1} if extra else {}))
            yield f'paths/{name}/{extra or "forced"}', lambda s=spec, sh=shape, o=opt: fwd_bwd(s, sh, 'bf16', 5, options=o)
        yield f'paths/{name}/forced_x3', lambda s=spec, sh=shape: fwd_bwd(s, sh, 'bf16x3', 5, options=FORCE)
    for config, batch in (('c2', 8), ('c1', 15), ('c4', 4), ('c4toy', 4), ('c5base', 4)):
        yield f'train/{config}/b{batch}', lambda c=config, b=batch: train(c, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--only', default='', help='run the cases whose name starts with this')
    a = ap.parse_args()
    out, wg, dg = {}, set(), set()
    for name, run in cases():
        if not name.startswith(a.only):
            continue
        out[name] = run()
        for _, _, w, g in out[name].get('sel', []):
            wg.add(w)
            dg.add(g)
        print(name, 'done', flush=True)
        with open(a.out, 'w') as f:          # (kept up to date: a partial file says where a run stopped)
            json.dump(out, f, indent=0, sort_keys=True)
    print('wgrad reached:', sorted(wg), '| not reached:', sorted(set(WGRADS) - wg))
    print('dgrad reached:', sorted(dg), '| not reached:', sorted(set(DGRADS) - dg))
    print('sha256 of', a.out, hashlib.sha256(open(a.out, 'rb').read()).hexdigest())


if __name__ == '__main__':
    main()
