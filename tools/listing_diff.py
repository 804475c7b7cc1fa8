"""Per-kernel diff of two `hipcc -S --offload-device-only` listings (e.g. of the parent commit and of a change): kernels are matched
by demangled name with an empty template argument pack dropped, local labels are renumbered per function, comments are dropped and
the kernel's own symbol is written <sym> inside its body, so that what is reported is a difference in the code.  A changed
symbol is listed beside the verdict.
python tools/listing_diff.py old.s new.s [--show]"""
import difflib, re, subprocess, sys


def funcs(path):
    txt = open(path).read()
    ms = list(re.finditer(r'^(_Z[^:\s]+):[^\n]*\n', txt, re.M))
    names = subprocess.run(['c++filt'] + [m.group(1) for m in ms], capture_output=True, text=True).stdout.split('\n')
    out = {}
    for m, d in zip(ms, names):
        sym = m.group(1)
        body = txt[m.end():txt.find('.Lfunc_end', m.end())]
        lines = [l for l in body.split('\n') if l.strip() and not l.strip().startswith((';', '.loc'))]
        lines = [re.sub(r'\.L(BB|tmp|func_end|_)(\d+)_', r'.L\1F_', re.sub(r'\s*;.*$', '', l)).replace(sym, '<sym>') for l in lines]
        out[d.replace('<>', '').replace('void ', '', 1)] = (sym, lines)
    return out


a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
show = '--show' in sys.argv
for n in sorted(set(a) | set(b)):
    if n not in a:
        print('NEW ', n[:110], len(b[n][1]), 'lines')
        continue
    if n not in b:
        print('GONE', n[:110])
        continue
    tag = 'SAME' if a[n][1] == b[n][1] else 'DIFF'
    print(tag, n[:110], len(a[n][1]), 'lines', '' if a[n][0] == b[n][0] else f'(symbol {a[n][0]} -> {b[n][0]})')
    if tag == 'DIFF' and show:
        for l in difflib.unified_diff(a[n][1], b[n][1], lineterm='', n=1):
            print('   ', l)
