#!/usr/bin/env python3
"""Mutation check of the sweep-program compilers: does the CPU suite notice a compiler that decides wrongly?

    python tools/mutate_compilers.py SCRATCH_DIR [mutation ...]

Copies the working tree to SCRATCH_DIR/<mutation> (object files included, so only the mutated file is compiled again), applies
one textual mutation to csrc/mlbp_compile.cpp, rebuilds libmlbp.so there and runs the CPU suite of the copy (-m "not gpu").
Prints, per mutation, the failing tests (and modules that no longer import) of tests/test_image_semantics_cpu.py, of the word-for-word fixture test
(tests/test_program_images.py) and of every other module.  Needs no GPU; never touches the tree it was started from.
"""
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = os.path.join('macaronicusermodeling_amd', 'csrc', 'mlbp_compile.cpp')

# name -> (what it breaks, text to find (exactly once; or a list of such texts), replacement(s))
MUTATIONS = {
    'dead_live': ("drop_dead_variable_updates treats a live update as dead: the liveness of a plain pairwise update's source is lost",
                  'if (is_plain_pair(kd)) { live[w[3]] = 0; live[w[2]] = 1; continue; }',
                  'if (is_plain_pair(kd)) { live[w[3]] = 0; continue; }'),
    'store_vf_final': ('the UOP_STORE_VF decision inverted for the final-value case: a message nobody reads or writes later is not stored',
                       ['    bool needed = true;\n    for (int j = i + 1; j < n_uops; ++j) {', '      if (reads) break;'],
                       ['    bool needed = false;\n    for (int j = i + 1; j < n_uops; ++j) {', '      if (reads) { needed = true; break; }']),
    'carry_last_link': ('the last link of a carry chain hands its product on instead of storing it',
                        '(first ? 0 : UOP_CARRY_IN) | (done < n ? UOP_CARRY_OUT : 0);',
                        '(first ? 0 : UOP_CARRY_IN) | ((done < n || !first) ? UOP_CARRY_OUT : 0);'),
    'cprod_loses_source': ('a constant product of two or more hoisted messages loses its last one',
                           '    out.cpw.push_back((int)l.size());\n    for (int v : l) out.cpw.push_back(v);',
                           '    if (l.size() > 1) l.pop_back();\n    out.cpw.push_back((int)l.size());\n    for (int v : l) out.cpw.push_back(v);'),
    'prune_changed': ('drop_unchanged_updates names a pairwise update by its table alone: an update whose source changed is dropped',
                      '        key.push_back(a);\n        key.push_back(val[b]);',
                      '        key.push_back(a);'),
}


def run(name, scratch):
    what, find, repl = MUTATIONS[name]
    dst = os.path.join(scratch, name)
    if os.path.exists(dst):
        shutil.rmtree(dst)
    shutil.copytree(ROOT, dst, symlinks=True, ignore=shutil.ignore_patterns('.git', '__pycache__', '.pytest_cache'))
    path = os.path.join(dst, TARGET)
    text = open(path).read()
    for a, b in zip(*(([x] if isinstance(x, str) else x) for x in (find, repl))):
        assert text.count(a) == 1, '%s: the text to mutate occurs %d times' % (name, text.count(a))
        text = text.replace(a, b)
    open(path, 'w').write(text)
    subprocess.check_call([sys.executable, '-m', 'macaronicusermodeling_amd.build'], cwd=dst, stdout=subprocess.DEVNULL)
    p = subprocess.run([sys.executable, '-m', 'pytest', 'tests', '-m', 'not gpu', '-q', '-p', 'no:cacheprovider', '-rfE'], cwd=dst,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    failed = sorted(set(re.findall(r'^(?:FAILED|ERROR) (\S+)', p.stdout, re.M)))
    groups = {'new': [], 'fixture': [], 'other': []}
    for t in failed:
        mod = t.split('::')[0]
        groups['new' if mod.endswith('test_image_semantics_cpu.py') else 'fixture' if mod.endswith('test_program_images.py') else 'other'].append(t)
    print('%s: %s' % (name, what))
    for k in ('new', 'fixture', 'other'):
        print('  %-8s %s' % (k, ', '.join(t.split('::', 1)[1] if k != 'other' else t for t in groups[k]) or '-'))
    sys.stdout.flush()
    return bool(groups['new'])


def main():
    scratch = os.path.abspath(sys.argv[1])
    assert not scratch.startswith(ROOT + os.sep) and scratch != ROOT, 'the scratch directory lies outside the tree'
    names = sys.argv[2:] or list(MUTATIONS)
    caught = [run(n, scratch) for n in names]
    sys.exit(0 if all(caught) else 1)


if __name__ == '__main__':
    main()
