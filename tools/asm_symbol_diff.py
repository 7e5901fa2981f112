"""Per-kernel text diff of device assembly, for moves of kernels between files.

    hipcc <the Makefile's flags> --cuda-device-only -S a.hip -o a.s      (per file, old and new tree)
    python tools/asm_symbol_diff.py --old old/*.s --new new/*.s

Every ``.amdhsa_kernel`` of either side is compared by mangled name: the
instruction stream (label to the descriptor) and the ``.amdhsa_*`` descriptor
block.  Function-local label numbers (``BB<n>_`` in labels and comments, ``.Lfunc_end<n>``) depend on
a function's position in its file and are normalised, and so are the runs of blanks that align comments.  Exit status 1 on any
difference in the set of names or in a body."""
import argparse
import difflib
import re
import sys

_LABEL = re.compile(r'(BB|\.Lfunc_begin|\.Lfunc_end|\.Ltmp)\d+')


def kernels(paths):
    """{mangled name: (instruction lines, descriptor lines)} over the files"""
    out = {}
    for path in paths:
        lines = [' '.join(_LABEL.sub(r'\1', ln).split()) for ln in open(path)]
        names = [ln.split()[1] for ln in lines if ln.startswith('.amdhsa_kernel ')]
        for name in names:
            assert name not in out, f'{name} is defined twice'
            a = next(i for i, ln in enumerate(lines) if ln.startswith(name + ':'))
            b = next(i for i in range(a, len(lines)) if lines[i] == '.amdhsa_kernel ' + name)
            c = next(i for i in range(b, len(lines)) if lines[i] == '.end_amdhsa_kernel')
            assert not any(ln.startswith('.type') for ln in lines[a:b]), f'{name}: ran into the next function'
            out[name] = (lines[a:b], lines[b:c + 1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--old', nargs='+', required=True)
    ap.add_argument('--new', nargs='+', required=True)
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    bad = 0
    for name in sorted(set(old) ^ set(new)):
        print('only in', 'old:' if name in old else 'new:', name)
        bad += 1
    for name in sorted(set(old) & set(new)):
        for what, a, b in zip(('code', 'descriptor'), old[name], new[name]):
            if a != b:
                bad += 1
                print(f'{name}: {what} differs')
                sys.stdout.write('\n'.join(list(difflib.unified_diff(a, b, 'old', 'new', lineterm=''))[:40]) + '\n')
    print(f'{len(old)} kernels old, {len(new)} new, {bad} differences')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
