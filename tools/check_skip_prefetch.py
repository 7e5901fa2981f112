"""Static check of the skip-row prefetch of conv3_mfma_persist_kernel<..., SKP = true>
(kernels_conv_mfma_persist.hip).

The consumer waves of that variant request the eight 16-B residual rows of a lane from
`asm volatile` statements behind the barrier of tap 25 and wait for them with ONE
explicit `s_waitcnt vmcnt(0)` behind the barrier of tap 26.  The compiler's waitcnt pass sees
neither, so between a load and that wait nothing may read or write its destination
registers: a register-allocator copy, a spill or an early use there would move a value
that has not arrived.  With the machinery of tools/check_inflight.py (control-flow graph
of the compiler's assembly, forward data flow to a fixed point) this checks, for every
hand-issued load of a basic block that also issues MFMAs (the producer waves' loads,
ordered by counted waits, sit in blocks without one):

  - from the load to the next inline-asm `s_waitcnt vmcnt(0)` on every path no
    instruction mentions v[a:b];
  - no path reaches the end of the kernel with such a load in flight;
  - there are exactly eight of them, in flight across the s_barrier of tap 26;
  - the kernel uses no scratch.

Usage: python tools/check_skip_prefetch.py [asm file]  (default: compiles the kernel file)
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import check_inflight as ci  # noqa: E402

SRC = os.path.join(HERE, '..', 'sup3r_amd', 'csrc', 'kernels_conv_mfma_persist.hip')
# template arguments <4, false, 0, false, false, 8, true>
MANGLED = r'^_ZN.*conv3_mfma_persist_kernelILi4ELb0ELi0ELb0ELb0ELi8ELb1EE.*:\s'


def compile_asm(tmpdir):
    out = os.path.join(tmpdir, 'persist.s')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    run = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                          os.path.abspath(SRC), '-o', out], cwd=os.path.dirname(os.path.abspath(SRC)),
                         capture_output=True, text=True)
    if run.returncode != 0:
        sys.exit('hipcc failed (%d):\n%s' % (run.returncode, run.stderr[-4000:]))
    return out


def is_load(code, in_asm):
    return in_asm and code.startswith('global_load_dwordx4')


def is_wait0(code, in_asm):
    return in_asm and code.startswith('s_waitcnt') and 'vmcnt(0)' in code


def transfer(b, live_in, tracked, problems):
    """walk one block; live: register -> (line of the load in flight, barriers passed since)"""
    live = dict(live_in)
    for ln, code, in_asm in b['ins']:
        if 'scratch_' in code and problems is not None:
            problems.append('scratch access at line %d: %s' % (ln, code))
        if is_load(code, in_asm) and ln in tracked:
            dst = ci.regs_of(code.split()[1].rstrip(','))
            if problems is not None:
                for r in (ci.mentioned(code) - dst) & set(live):
                    problems.append('line %d reads v%d (in flight since line %d): %s' % (ln, r, live[r][0], code))
            for r in dst:
                live[r] = (ln, 0)
        elif is_wait0(code, in_asm):
            if problems is not None and live:
                tracked_done = {v[0]: v[1] for v in live.values()}
                for l0, nb in tracked_done.items():
                    if nb < 1:
                        problems.append('load of line %d is waited for after %d s_barriers (line %d)' % (l0, nb, ln))
            live = {}
        elif live:
            if code.startswith('s_barrier'):
                live = {r: (v[0], v[1] + 1) for r, v in live.items()}
            if problems is not None:
                for r in ci.mentioned(code) & set(live):
                    problems.append('line %d touches v%d (in flight since line %d): %s' % (ln, r, live[r][0], code))
                if code.split()[0] == 's_endpgm':
                    problems.append('line %d: kernel ends with loads in flight' % ln)
    return live


def check(path):
    lines = open(path).read().split('\n')
    problems, n_loads, n_kern = [], 0, 0
    i = 0
    while i < len(lines):
        if re.match(MANGLED, lines[i] + ' '):
            n_kern += 1
            j = i + 1
            body = []
            while j < len(lines) and not lines[j].startswith('.Lfunc_end'):
                body.append((j + 1, lines[j]))
                j += 1
            blocks = ci.parse_blocks(body)
            tracked = set()
            for b in blocks:
                if any(c.startswith('v_mfma') for _, c, _ in b['ins']):
                    tracked |= {ln for ln, c, a in b['ins'] if is_load(c, a)}
            n_loads += len(tracked)
            # forward data flow to a fixed point (union over predecessors; of two
            # records of one register the one with fewer barriers passed is kept)
            live_in = [None] * len(blocks)
            live_in[0] = {}
            work = [0]
            while work:
                k = work.pop()
                out = transfer(blocks[k], live_in[k], tracked, None)
                for sidx in blocks[k]['succ']:
                    old = live_in[sidx]
                    new = dict(old or {})
                    for r, v in out.items():
                        if r not in new or v[1] < new[r][1]:
                            new[r] = v
                    if old is None or new != old:
                        live_in[sidx] = new
                        work.append(sidx)
            for k, b in enumerate(blocks):
                if live_in[k] is not None:
                    transfer(b, live_in[k], tracked, problems)
            i = j
        i += 1
    return n_kern, n_loads, problems


if __name__ == '__main__':
    with tempfile.TemporaryDirectory() as tmp:
        nk, nl, pr = check(sys.argv[1] if len(sys.argv) > 1 else compile_asm(tmp))
    print('%d kernels, %d skip-row loads, %d problems' % (nk, nl, len(pr)))
    for p in pr[:40]:
        print('  ' + p)
    sys.exit(1 if pr or nk != 1 or nl != 8 else 0)
