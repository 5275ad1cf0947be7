#!/usr/bin/env python3
"""Developer helper: gfx950 assembly listings of every csrc object, and their comparison with another tree's (a refactor must not change them).
usage: tools/isa_listing.py OUTDIR [--csrc DIR] [object ...]     write OUTDIR/<object>.s, each compiled with that object's own Makefile flags
       tools/isa_listing.py OUTDIR --against DIR    compare with listings written earlier from the parent tree (no compilation)
Lines holding __hip_cuid_ (a hash of the source text) are dropped.  Where two listings differ the kernels are compared one by one, local labels
without their function number; a kernel whose body is the same under a new name (a dropped template parameter) is reported as renamed."""
import os, re, shlex, subprocess, sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neural-navier-stokes_amd', 'csrc')

def compile_cmd(csrc, stem):
    """The hipcc command the Makefile uses for <stem>.o, without its -c/-o/source words: the flags live in one place."""
    out = subprocess.run(['make', '-n', '-B', '-C', csrc, stem + '.o'], capture_output=True, text=True, check=True).stdout
    words = shlex.split(next(l for l in out.splitlines() if 'hipcc' in l))
    return [w for i, w in enumerate(words) if w != '-c' and w != '-o' and words[i - 1] != '-o' and not w.startswith(stem + '.')]

def objects(csrc):
    objs = re.search(r'^OBJS\s*=\s*(.*)$', open(os.path.join(csrc, 'Makefile')).read(), re.M).group(1).split()
    return [o[:-2] for o in objs if os.path.exists(os.path.join(csrc, o[:-2] + '.hip'))]

def kernels(text):
    """{name: body + descriptor} of every kernel in a listing."""
    out = {}
    for name in re.findall(r'^\s*\.amdhsa_kernel (\S+)', text, re.M):
        body = re.search(r'^%s:.*?^\s*\.end_amdhsa_kernel' % re.escape(name), text, re.M | re.S).group(0)
        out[name] = re.sub(r'[ \t]+', ' ', re.sub(r'(BB|Lfunc_end|Lfunc_begin)\d+', r'\1', body))      # (comment columns move with the number's width)
    return out

def compare(stem, mine, theirs):
    a, b = kernels(theirs), kernels(mine)
    if mine == theirs:
        return '%-22s %3d kernels  identical' % (stem, len(b))
    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    renamed = [(g, n) for n in new for g in gone if a[g].replace(g, n) == b[n]]
    gone = [g for g in gone if g not in [r[0] for r in renamed]]
    new = [n for n in new if n not in [r[1] for r in renamed]]
    changed = [k for k in a if k in b and a[k] != b[k]]
    lines = ['%-22s %3d kernels (parent %d)  %s' % (stem, len(b), len(a), 'DIFFERENT' if changed or new else 'every kept kernel identical')]
    lines += ['    changed  ' + k for k in changed] + ['    added    ' + k for k in new] + ['    removed  ' + k for k in gone]
    return '\n'.join(lines + ['    renamed  %s -> %s' % r for r in renamed])

def main():
    args = sys.argv[1:]
    opt = {k: args[args.index(k) + 1] for k in ('--csrc', '--against') if k in args}
    outdir, csrc = args[0], opt.get('--csrc', CSRC)
    os.makedirs(outdir, exist_ok=True)
    strip = lambda p: ''.join(l for l in open(p) if '__hip_cuid_' not in l)
    only = [a for a in args[1:] if not a.startswith('--') and a not in opt.values()]        # optional: object names, to redo a few
    for stem in only or objects(csrc):
        path = os.path.join(outdir, stem + '.s')
        if '--against' in opt:
            print(compare(stem, strip(path), strip(os.path.join(opt['--against'], stem + '.s'))), flush=True)
        else:
            subprocess.run(compile_cmd(csrc, stem) + ['--cuda-device-only', '-S', stem + '.hip', '-o', os.path.abspath(path)], cwd=csrc, check=True)

if __name__ == '__main__':
    main()
