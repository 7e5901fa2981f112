#!/usr/bin/env python
"""Launch shapes of two builds of the library, compared per kernel name.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/launch_trace.py run
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python bench.py --mode train ...   (any fixed command)
    python tools/launch_trace.py table OUT_A OUT_B [...] > table.md

``run`` is the fixed workload: forward + backward of the 2-D and 3-D test
configs in f32, bf16 and bf16x3, then one call of each support entry point
that sizes its grid through launch_shape.h (loss map, branch join, time pad,
st_interp, coarsen, time window / mean, nn fill, night mask, conditional-moment
target, sample gather).  SUP3R_AMD_LIB selects the build.  ``table`` reads the
kernel traces of several runs: per kernel name the call count and the multiset
of (grid, workgroup, LDS) must be the same in all of them; exit status 1 where
they are not (the runtime's own copy and fill kernels and torch's, which
fill the inputs, are listed but not required to agree)."""
import collections
import csv
import ctypes as C
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETS = [   # (config, input shape) as tests/test_hip_parity.py runs them
    ('test_gen_s_2x_2f.json', (3, 7, 6, 2)),
    ('test_disc_s_same.json', (2, 20, 20, 2)),
    ('test_gen_st_2x_4x_2f.json', (2, 5, 6, 4, 3)),
    ('test_gen_st_64ch.json', (1, 6, 5, 12, 3)),
    ('test_disc_st_same.json', (2, 12, 12, 16, 2)),
]


def nets():
    import numpy as np
    from sup3r_amd.engine import Network
    for cfg, shape in NETS:
        with open(os.path.join(ROOT, 'sup3r_amd', 'configs', cfg)) as f:
            spec = json.load(f)
        for prec in ('f32', 'bf16', 'bf16x3'):
            rng = np.random.default_rng(5)
            net = Network(spec, precision=prec)
            net.build(shape, seed=5)
            ph = net.plan(shape, training=True)
            y = ph.forward(net.dev.to_device(rng.standard_normal(shape).astype(np.float32)))
            ph.backward(net.dev.to_device(rng.standard_normal(tuple(y.shape)).astype(np.float32)))
            net.clear_plans()
            print(cfg, prec, 'done', flush=True)


def support():
    import numpy as np
    import torch
    from sup3r_amd import _lib
    from sup3r_amd.engine import Device
    from sup3r_amd.linear import _axes_table
    dev, L = Device.get(), _lib.lib()
    td = dev.torch_device

    def p(t):
        return C.c_void_p(t.data_ptr())

    def ints(v):
        return (C.c_int32 * len(v))(*v)

    def ok(rc, what):
        _lib.check(rc, dev.ctx, what)
        print(what, 'done', flush=True)

    n, s1, s2, t, c = 2, 12, 10, 8, 3
    x = torch.randn(n, s1, s2, t, c, device=td)
    out = torch.zeros(1 << 20, device=td)
    work = torch.zeros(1 << 20, device=td)
    ok(L.s3_lossmap_fwd(dev.ctx, 1, p(x), n, s1, s2, t, c, c, 0, 0, 0, p(out), p(work)), 's3_lossmap_fwd')
    # branch join: two sources of 3 / 2 channels -> 4, over (t, h, w)
    ya, yb = torch.randn(t, 40, 37, 3, device=td), torch.randn(t, 40, 37, 2, device=td)
    ok(L.s3_branch_join(dev.ctx, p(ya), 3, ints([0, 2]), 2, None, None, p(yb), 2, ints([1, 0]), 2, None, None,
                        t, 40, 37, None, None, p(out)), 's3_branch_join')
    ok(L.s3_time_pad_reflect(dev.ctx, p(x), n * s1 * s2, t, c, 3, None, None, p(out)), 's3_time_pad_reflect')
    axes = _axes_table(dev, s1, s2, t, 2, 3, False)
    big = torch.zeros(x.numel() * 12, device=td)
    ok(L.s3_st_interp(dev.ctx, p(x), n, s1, s2, t, c, 2, 3, p(axes), p(big)), 's3_st_interp')
    ok(L.s3_coarsen(dev.ctx, p(x), n, s1, s2, t, c, 2, 2, 1, p(out)), 's3_coarsen')
    ok(L.s3_time_window(dev.ctx, p(x), n * s1 * s2, t, c, 2, 4, p(out), 0, 1.0), 's3_time_window')
    ok(L.s3_time_mean(dev.ctx, p(x), n * s1 * s2, t, c, 2, 4, p(out), 0, 1.0), 's3_time_mean')
    holes = x.clone()
    holes[:, ::3, ::2, :, 1] = float('nan')
    count = torch.zeros(4, dtype=torch.int32, device=td)
    key = torch.zeros(2 * n * s1 * s2 * t + 16, dtype=torch.int64, device=td)
    ok(L.s3_nn_fill(dev.ctx, p(holes), n, s1, s2, t, c, 1, p(key), p(count)), 's3_nn_fill')
    cube = torch.randn(30, 28, 72, 3, device=td)
    origins = ints([0, 0, 0, 5, 7, 24, 18, 16, 48])
    status = torch.zeros(4, dtype=torch.int32, device=td)
    ok(L.s3_cc_night_mask(dev.ctx, p(cube), 30, 28, 72, 3, origins, 3, 12, 12, 2, p(status)), 's3_cc_night_mask')
    ok(L.s3_sample_gather(dev.ctx, p(cube), 30, 28, 72, 3, origins, 3, 12, 12, 24, ints([2, 0]), 2, p(big)),
       's3_sample_gather')
    lr = torch.randn(n, s1 // 2, s2 // 2, t // 2, 2, device=td)
    mask = torch.zeros_like(x)
    ok(L.s3_condmom_target(dev.ctx, p(x), p(lr), None, n, s1, s2, t, c, 2, 0, ints([0, 1, 1]), 2, 2,
                           _lib.CM_SUBFILTER, 1, 1, t - 1, p(out), p(mask)), 's3_condmom_target')
    torch.cuda.synchronize()


def shapes(out_dir):
    """{kernel name: Counter of (grid, workgroup, LDS)} of one traced run"""
    files = glob.glob(os.path.join(out_dir, '**', '*kernel_trace.csv'), recursive=True)
    assert files, f'no kernel trace under {out_dir}'
    res = collections.defaultdict(collections.Counter)
    for path in files:
        for r in csv.DictReader(open(path)):
            grid = tuple(int(r[k]) for k in ('Grid_Size_X', 'Grid_Size_Y', 'Grid_Size_Z'))
            wg = tuple(int(r[k]) for k in ('Workgroup_Size_X', 'Workgroup_Size_Y', 'Workgroup_Size_Z'))
            res[r['Kernel_Name']][(grid, wg, int(r['LDS_Block_Size']))] += 1
    return res


def ours(name):
    return not ('at::' in name or name.startswith('__amd_rocclr'))


def table(dirs):
    runs = [shapes(d) for d in dirs]
    names = sorted(set().union(*runs))
    bad = 0
    print('| kernel | calls | distinct (grid, workgroup, LDS) | same in all runs |')
    print('|---|---|---|---|')
    for name in names:
        same = all(r.get(name) == runs[0].get(name) for r in runs[1:])
        required = ours(name)
        if not same and required:
            bad += 1
        calls = ' / '.join(str(sum(r.get(name, {}).values())) for r in runs)
        kinds = ' / '.join(str(len(r.get(name, {}))) for r in runs)
        short = name.replace('(anonymous namespace)::', '').split('(')[0].replace('void ', '')[:90]
        print(f'| `{short}` | {calls} | {kinds} | {"yes" if same else ("NO" if required else "no (runtime)")} |')
    runs_named = ', '.join(os.path.basename(os.path.normpath(d)) for d in dirs)
    print(f'\n{len(names)} kernel names over {len(dirs)} runs ({runs_named}), {bad} differences')
    return 1 if bad else 0


if __name__ == '__main__':
    if sys.argv[1:2] == ['run']:
        nets()
        support()
    elif sys.argv[1:2] == ['table'] and len(sys.argv) > 3:
        sys.exit(table(sys.argv[2:]))
    else:
        sys.exit(__doc__)
