"""The host arithmetic of launch shapes (sup3r_amd/csrc/launch_shape.h) against
the formulas restated here: tests/launch_shape_main.cpp is compiled alone with
a plain C++ compiler (the header has no HIP in it) and prints each function's
result; no GPU, no hipcc."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')


def ceil_div(a, b):
    return -(-a // b)


def grid_for(n, num_cu, per_cu):
    """ceil(n / 256) workgroups, at most per_cu per CU, at least 1"""
    return max(1, min(ceil_div(n, 256), num_cu * per_cu))


def persistent(slots, items, min1):
    """slots workgroups raised to 1, then at most one per item (0 for no
    items); min1: the two bounds the other way round (1 for no items)"""
    return max(1, min(slots, items)) if min1 else min(max(slots, 1), items)


@pytest.fixture(scope='module')
def printed(tmp_path_factory):
    if CXX is None:
        pytest.skip('no C++ compiler')
    exe = str(tmp_path_factory.mktemp('launch_shape') / 'launch_shape_main')
    subprocess.run([CXX, '-std=c++17', '-I', os.path.join(ROOT, 'sup3r_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'launch_shape_main.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        what, *vals = line.split()
        rows.setdefault(what, []).append([int(v) for v in vals])
    return rows


def test_block(printed):
    assert printed['block'] == [[256]]


def test_grid_for(printed):
    seen = set()
    for n, num_cu, per_cu, got in printed['grid_for']:
        assert got == grid_for(n, num_cu, per_cu), (n, num_cu, per_cu)
        seen.add((n, num_cu, per_cu))
    want = set()
    for num_cu in (256, 1):
        for per_cu in (8, 16):
            cap = num_cu * per_cu
            for n in (0, 1, 255, 256, 257, cap * 256 - 1, cap * 256, cap * 256 + 1, 2 ** 40):
                want.add((n, num_cu, per_cu))
    assert seen == want
    # per_cu defaults to 8
    assert printed['grid_for_default'] == [[256 * 8, 8]]


def test_persistent_grid(printed):
    seen = set()
    for min1, slots, items, got in printed['persistent']:
        assert got == persistent(slots, items, min1), (min1, slots, items)
        seen.add((min1, slots, items))
    assert seen == {(m, s, i) for m in (0, 1) for s in (0, 1, 256) for i in (0, 1, 255, 256, 257)}
    # what tells the two orders apart
    assert persistent(256, 0, 0) == 0 and persistent(256, 0, 1) == 1


def test_tile_counts(printed):
    seen = set()
    for N, o0, o1, o2, T, t0, t1, t2, total in printed['tiles']:
        want = [ceil_div(o, T) for o in (o0, o1, o2)]
        assert [t0, t1, t2] == want and total == N * want[0] * want[1] * want[2], (N, o0, o1, o2, T)
        seen.add((N, o0, o1, o2, T))
    assert seen == {(N, a, b, c, T) for T in (2, 4, 16) for N in (1, 3)
                    for a in (1, T - 1, T, T + 1) for b in (1, T - 1, T, T + 1) for c in (1, T - 1, T, T + 1)}
    # two tiled axes: the third counts one tile
    for N, o0, o1, T, t0, t1, t2, total in printed['tiles2d']:
        want = [ceil_div(o0, T), ceil_div(o1, T), 1]
        assert [t0, t1, t2] == want and total == N * want[0] * want[1], (N, o0, o1, T)
    assert len(printed['tiles2d']) == 3 * 2 * 4 * 4
