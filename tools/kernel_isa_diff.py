#!/usr/bin/env python3
"""What a change of the sources did to the kernels the compiler emits: the gfx950 assembly of two trees, kernel by kernel
(cross-compiles without a GPU).

    python tools/kernel_isa_diff.py OLD_TREE NEW_TREE nearfield_simple.hip [file.hip ...]

Every named file that a tree has under metalens_amd/csrc is compiled device-only to assembly with the flags of
tools/kernel_resources.py.  Kernels are paired by demangled name across ALL the files given (kernels move between files).
Per kernel, differences only:
  * nothing if the instruction streams are identical - comments stripped, the function number of block labels normalised;
  * else the compiler's resource figures of both sides (a `!` in front of one that changed) and every mnemonic whose
    count differs, with both counts;
  * kernels only one tree has.
The last line counts the kernels compared.  Exit status 1 if a resource figure changed or a kernel is unpaired.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-I../../include', '-I.']
FIGURES = [('VGPR', '.vgpr_count'), ('AGPR', '.agpr_count'), ('SGPR', '.sgpr_count'), ('spill V', '.vgpr_spill_count'),
           ('spill S', '.sgpr_spill_count'), ('scratch', '.private_segment_fixed_size'), ('LDS', '.group_segment_fixed_size'),
           ('occ', 'occupancy')]


def assembly(tree, src, tmp):
    csrc = os.path.join(tree, 'metalens_amd', 'csrc')
    if not os.path.exists(os.path.join(csrc, src)):
        return None
    out = os.path.join(tmp, '%x_%s.s' % (abs(hash(tree)), src))
    flags = FLAGS + (['-mllvm', '-amdgpu-kernarg-preload-count=1'] if 'nearfield_simple' in src else [])
    run = subprocess.run(['/opt/rocm/bin/hipcc'] + flags + ['-S', '--cuda-device-only', '-Wno-unused-command-line-argument',
                                                            '-o', out, src], cwd=csrc, capture_output=True, text=True)
    if run.returncode:
        sys.exit('%s/%s does not compile:\n%s' % (tree, src, run.stderr))
    return open(out).read()


def kernels(text):
    """{mangled name: (instruction stream, figures)} of one assembly listing."""
    figures = {}
    note = re.split(r'\n(?=\S)', text.split('amdhsa.kernels:')[1])[0]   # the kernel list of the metadata note
    for block in note.split('\n  - ')[1:]:
        f = dict(re.findall(r'^\s*(\.\w+):\s+(\S+)$', block, re.M))
        figures[f['.name']] = f
    found, name, stream = {}, None, None
    for line in text.splitlines():
        label = re.match(r'(\w+):', line)
        if label and label.group(1) in figures:
            name, stream = label.group(1), []
        elif name and stream is not None:
            if line.startswith('.Lfunc_end'):
                found[name] = (stream, figures[name])
                stream = None   # (the compiler's summary of the kernel follows)
                continue
            line = re.sub(r'\.LBB\d+_', '.LBB_', line.split(';')[0]).strip()
            if line:
                stream.append(line)
        elif name and line.startswith('; Occupancy:'):
            figures[name]['occupancy'] = line.split()[-1]
            name = None
    return found


def mnemonics(stream):
    return collections.Counter(l.split()[0] for l in stream if not l.endswith(':') and not l.startswith('.'))


def main():
    old_tree, new_tree, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    sides = [{}, {}]
    with tempfile.TemporaryDirectory() as tmp:
        for side, tree in zip(sides, (old_tree, new_tree)):
            for src in files:
                text = assembly(tree, src, tmp)
                if text is not None:
                    side.update(kernels(text))
    names = sorted(set(sides[0]) | set(sides[1]))
    demangled = subprocess.run(['c++filt'] + names, capture_output=True, text=True).stdout.splitlines() if names else []
    bad = same = 0
    for name, pretty in zip(names, demangled):
        pretty = re.sub(r'\(.*', '', pretty).replace('void ml::', '')
        if name not in sides[0] or name not in sides[1]:
            print('%-52s only in %s' % (pretty, old_tree if name in sides[0] else new_tree))
            bad += 1
            continue
        (s0, f0), (s1, f1) = sides[0][name], sides[1][name]
        if s0 == s1:
            same += 1
            continue
        changed = [k for _, k in FIGURES if f0.get(k) != f1.get(k)]
        bad += bool(changed)
        print('%s: %d -> %d instructions' % (pretty, sum(mnemonics(s0).values()), sum(mnemonics(s1).values())))
        for side, f in (('old', f0), ('new', f1)):
            print('    %s  %s' % (side, '  '.join('%s%s %s' % ('!' if k in changed else '', label, f.get(k)) for label, k in FIGURES)))
        m0, m1 = mnemonics(s0), mnemonics(s1)
        diff = ['%s %d -> %d' % (k, m0[k], m1[k]) for k in sorted(set(m0) | set(m1)) if m0[k] != m1[k]]
        print('    ' + ('; '.join(diff) if diff else 'the same count of every mnemonic (order or registers differ)'))
    print('%d kernels compared: %d identical, %d differ' % (len(names), same, len(names) - same))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
