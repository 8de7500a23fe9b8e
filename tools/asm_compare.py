"""Kernel-by-kernel text comparison of two device assembly listings of the same source file
(hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S), comments, debug lines and
the function index inside block labels aside:
  python tools/asm_compare.py LABEL A.s B.s [LABEL A.s B.s ...]
prints one table per triple and exits 1 if a kernel differs or the kernel counts differ."""
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: [instruction lines]} of every kernel (.amdhsa_kernel symbol) in the listing"""
    names = set()
    lines = open(path).read().split('\n')
    for ln in lines:
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln)
        if m:
            names.add(m.group(1))
    out, cur = {}, None
    for ln in lines:
        m = re.match(r'^(\S+):', ln)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        s = ln.split(';')[0].rstrip()
        if re.match(r'\s*\.Lfunc_end', s):
            cur = None
            continue
        if not s.strip() or re.match(r'\s*\.(loc|file|cfi_|Ltmp)', s) or re.match(r'^\.Ltmp\d+:', s):
            continue
        # a block label .LBB<f>_<n> carries f, the function's position in the listing, which moves
        # when the host code names the instances in another order; n stays
        cur.append(re.sub(r'\.LBB\d+_', '.LBB_', s))
    return out


def demangle(names):
    try:
        r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, (x.split('(')[0] for x in r.stdout.split('\n'))))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def compare(label, a, b):
    ka, kb = kernels(a), kernels(b)
    nice = demangle(sorted(set(ka) | set(kb)))
    print(f'{label}: {len(ka)} kernels in the parent, {len(kb)} here')
    ok = len(ka) == len(kb)
    for n in sorted(set(ka) | set(kb), key=lambda n: nice[n]):
        if n not in ka or n not in kb:
            verdict = 'only in the parent' if n in ka else 'only here'
        else:
            verdict = 'identical' if ka[n] == kb[n] else 'DIFFERENT'
        ok &= verdict == 'identical'
        print(f'  {nice[n]:<72s}{len(kb.get(n, ka.get(n))):>7d} lines  {verdict}')
    return ok


if __name__ == '__main__':
    args = sys.argv[1:]
    good = True
    for i in range(0, len(args), 3):
        good &= compare(*args[i:i + 3])
    sys.exit(0 if good else 1)
