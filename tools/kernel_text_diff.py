#!/usr/bin/env python3
"""Compare the kernels of two device assembly files symbol by symbol.

    python tools/kernel_text_diff.py OLD.s NEW.s [--gone NAME ...]

Both files come from the same unit compiled with the Makefile's FLAGS plus
`--cuda-device-only -S`.  For every `.amdhsa_kernel` symbol the text from its
label to its `.Lfunc_end` label (its `.amdhsa_kernel ... .end_amdhsa_kernel`
block lies in between) is compared as text.  The only thing set aside is the
function's ordinal in the file, which the compiler writes into its local
labels (`.LBB<n>_<k>`, `.Lfunc_end<n>`, `BB<n>_<k>` in its loop comments),
and with it the blanks that pad a label's comment to its column: a kernel
that merely moved in the source keeps its text.  Prints the symbol
counts and every name that is only on one side or differs; exit status 0 when
every NEW symbol is in OLD with the same text and every OLD symbol is in NEW
or named by --gone.
"""
import argparse
import re
import sys


def kernels(path):
    lines = open(path).read().split('\n')
    names = [m.group(1) for ln in lines for m in [re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln)] if m]
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r'(\S+):', ln)
        if m and m.group(1) in names and m.group(1) not in start:
            start[m.group(1)] = i
    out = {}
    for name in names:
        i = start[name]
        j = i
        while not re.match(r'\.Lfunc_end(\d+):', lines[j]):
            j += 1
        n = re.match(r'\.Lfunc_end(\d+):', lines[j]).group(1)
        # (the compiler writes the kernel's descriptor block before its end label)
        text = '\n'.join(lines[i:j + 1])
        assert '.amdhsa_kernel ' + name in text and '.end_amdhsa_kernel' in text, name
        text = re.sub(r'(\.L[A-Za-z_]+|\bBB)' + n + r'(?![0-9])', r'\1#', text)
        # (a label's comment is padded to a column, so the ordinal's digit
        # count -- 99 against 100 -- shows in the blanks before its `;`)
        out[name] = re.sub(r'[ \t]+;', ' ;', text)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--gone', nargs='*', default=[],
                    help='OLD symbols that NEW may lack (unreachable instantiations)')
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    added = sorted(set(new) - set(old))
    missing = sorted(set(old) - set(new) - set(a.gone))
    differ = sorted(k for k in new if k in old and new[k] != old[k])
    print('kernels: old %d, new %d, in both %d' % (len(old), len(new), len(set(old) & set(new))))
    print('identical text: %d' % (len(set(old) & set(new)) - len(differ)))
    for title, ks in (('only in new', added), ('only in old, not listed as gone', missing),
                      ('text differs', differ)):
        print('%s: %d' % (title, len(ks)))
        for k in ks:
            print('  ' + k)
    ok = not (added or missing or differ)
    print('verdict: %s' % ('device code unchanged' if ok else 'DIFFERENT'))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
