"""Issue-slot count of one kernel instance from its gfx950 assembly, split at its LM loop.

    hipcc <the build's flags> --cuda-device-only -S acinoset_amd/csrc/sba.hip -o sba.s
    python tools/isa_loop_slots.py sba.s [kernel-name substring]

The default kernel is the headline instance k_sba_lm<16, 1, false, true, 3> (the row instance for
5 or 6 slots; before round 11 the headline ran k_sba_lm<8, 1, false, true>). One wave alone on a
SIMD issues one instruction per ~4 cycles whatever its kind, so the count of instructions is
the figure of merit; they are classified by mnemonic only:

    f64     mnemonic contains _f64 (arithmetic, compares, conversions, rcp / rsq seeds)
    dpp     mnemonic ends in _dpp
    vector  every other v_*
    scalar  s_* (branches, exec-mask bookkeeping, waits, s_nop)
    memory  global_ / flat_ / buffer_ / scratch_ / ds_

The loop is the run of basic blocks the compiler's own comments mark 'Loop Header' / 'in
Loop'; 'pre-loop' is everything from the kernel's entry to the first of them (the early-exit
store blocks the compiler places there included), 'post-loop' the rest.
"""
import re
import sys
from collections import Counter

CLASSES = ('f64', 'dpp', 'vector', 'scalar', 'memory', 'other')
DEFAULT = '_Z8k_sba_lmILi16ELi1ELb0ELb1ELi3ELi0EE'


def classify(mn):
    if mn.endswith('_dpp'):
        return 'dpp'
    if mn.startswith('v_'):
        return 'f64' if '_f64' in mn else 'vector'
    if mn.startswith('s_'):
        return 'scalar'
    if mn.startswith(('global_', 'flat_', 'buffer_', 'scratch_', 'ds_')):
        return 'memory'
    return 'other'


def kernel_lines(lines, name):
    start = None
    for i, l in enumerate(lines):
        if start is None:
            if re.match(r'^[A-Za-z_]\w*:', l) and name in l.split(':')[0]:
                start = i + 1
        elif l.lstrip().startswith('.Lfunc_end'):
            return lines[start:i]
    if start is None:
        sys.exit(f'no kernel whose symbol contains {name!r}')
    return lines[start:]


def count(body):
    """-> {'pre-loop' | 'loop' | 'post-loop': Counter of classes}, Counter of loop mnemonics"""
    parts = {k: Counter() for k in ('pre-loop', 'loop', 'post-loop')}
    loop_mn = Counter()
    where = 'pre-loop'
    for l in body:
        s = l.strip()
        if not s or s.startswith((';', '.')) and not s.startswith('.LBB'):
            continue
        if s.startswith('.LBB'):
            in_loop = 'Loop Header' in s or 'in Loop' in s
            if in_loop:
                where = 'loop'
            elif where == 'loop':
                where = 'post-loop'
            continue
        mn = s.split()[0]
        if not re.match(r'^[a-z]', mn):
            continue
        parts[where][classify(mn)] += 1
        if where == 'loop':
            loop_mn[mn] += 1
    return parts, loop_mn


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    name = sys.argv[2] if len(sys.argv) > 2 else DEFAULT
    with open(sys.argv[1]) as f:
        body = kernel_lines(f.read().splitlines(), name)
    parts, loop_mn = count(body)
    print(f'{"part":10s} {"slots":>6s} ' + ' '.join(f'{c:>7s}' for c in CLASSES))
    for k, c in parts.items():
        print(f'{k:10s} {sum(c.values()):6d} ' + ' '.join(f'{c[x]:7d}' for x in CLASSES))
    sel = {m: n for m, n in loop_mn.items() if classify(m) in ('vector', 'scalar', 'dpp')}
    print('loop, non-f64:', ', '.join(f'{m} {n}' for m, n in sorted(sel.items(), key=lambda t: -t[1])))


if __name__ == '__main__':
    main()
