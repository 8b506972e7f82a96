#!/usr/bin/env python3
"""Per-kernel comparison of the device code of two source trees: is a kernel of this tree the code it was in the parent commit?

    python tools/isa_diff.py --parent-tree DIR [--files wilson.hip meta.hip ...] [--jobs 6] [--dump DIR] [--out profiles/resident_plan_isa.json]
                             [--rename PATTERN REPLACEMENT ...]

Every file is compiled to device assembly in both trees with exactly the flags the Makefile gives it (the command `make -n FILE.o`
prints, -c swapped for --cuda-device-only -S), every kernel is cut from its label to its .Lfunc_end, comments and directives are
dropped and basic-block labels renumbered in order of appearance, and the two texts are compared.  Per kernel the document says
whether they are equal and gives, for both trees, the instruction count and VGPRs, SGPRs, scratch and LDS bytes of the metadata.
An equal kernel has the parent's behaviour and speed by construction.  Needs hipcc, no GPU.  Exit status 1 if a kernel differs,
appeared or went away.

--rename PATTERN REPLACEMENT (a regular expression and its substitution, repeatable): a parent symbol's new name, for a kernel template
that gained a parameter -- the mangled names of all its instances change though their code need not.  The substitution is applied to
the parent's kernel symbols and to the same names where the parent's instructions mention them; the instances are then compared
pairwise under their new names, and a row says which parent symbol it was compared with."""
import argparse
import concurrent.futures
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ['wilson.hip', 'meta.hip', 'local.hip', 'topo.hip', 'loops.hip', 'flow_small.hip']
META = dict(vgpr='.vgpr_count', sgpr='.sgpr_count', scratch_bytes='.private_segment_fixed_size', lds_bytes='.group_segment_fixed_size')


def assembly(tree, src, outdir):
    """device assembly of tree/fthmc_amd/csrc/src by the Makefile's own command -> the listing's text"""
    csrc = os.path.join(tree, 'fthmc_amd', 'csrc')
    obj = src[:-len('.hip')] + '.o'
    plan = subprocess.run(['make', '-n', '-B', obj], cwd=csrc, check=True, capture_output=True, text=True).stdout
    cmd = next(shlex.split(l) for l in plan.splitlines() if ' -c ' + src in l)
    out = os.path.join(outdir, src + '.s')
    i = cmd.index('-c')
    cmd[i:i + 1] = ['--cuda-device-only', '-S']
    cmd[cmd.index('-o') + 1] = out
    subprocess.run(cmd, cwd=csrc, check=True)
    with open(out) as f:
        return f.read()


def kernels(text):
    """{kernel symbol: (normalised instruction lines, metadata)} of one listing"""
    meta = {}
    note = re.search(r'^amdhsa\.kernels:\n((?: .*\n)*)', text, re.M)
    note = '\n' + note.group(1) if note else ''
    for entry in re.split(r'\n  - ', note)[1:]:               # the entries of the metadata note; their own keys sit at four columns
        keys = dict(re.findall(r'^(?:    )?(\.\w+): +(\S+) *$', entry, re.M))
        meta[keys['.name']] = {k: int(keys[v]) for k, v in META.items()}
    lines, out, body, cur = text.splitlines(), {}, None, None
    for l in lines:
        t = l.split(';')[0].strip()
        m = re.match(r'^(_Z\w+):$', t)
        if m and m.group(1) in meta:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if t.startswith('.Lfunc_end'):
            out[cur] = (renumber(body), meta[cur])
            cur = None
        elif t and (not t.startswith('.') or re.match(r'^\.LBB\w+:$', t)):
            body.append(' '.join(t.split()))
    return out


def renumber(body):
    """basic-block labels by order of appearance (function numbers and block numbers shift with every function added before)"""
    ids = {}
    for l in body:
        for lab in re.findall(r'\.LBB\d+_\d+', l):
            ids.setdefault(lab, f'.L{len(ids)}')
    return [re.sub(r'\.LBB\d+_\d+', lambda m: ids[m.group(0)], l) for l in body]


def side(body, meta):
    return dict(instructions=sum(not l.endswith(':') for l in body), **meta)


def renamed(kp, renames):
    """the parent's kernels under their new names -> ({new name: (body, meta)}, {new name: parent symbol} of those that changed)"""
    def new_name(sym):
        for pat, repl in renames:
            sym = re.sub(pat, repl, sym)
        return sym
    names = {k: new_name(k) for k in kp}
    was = {n: k for k, n in names.items() if n != k}
    sym = re.compile(r'_Z\w+')
    return {names[k]: ([sym.sub(lambda m: new_name(m.group(0)), l) for l in body], meta) for k, (body, meta) in kp.items()}, was


def compare(src, parent, new, dump=None, renames=()):
    with tempfile.TemporaryDirectory() as dp, tempfile.TemporaryDirectory() as dn:
        kp, kn = kernels(assembly(parent, src, dp)), kernels(assembly(new, src, dn))
    kp, was = renamed(kp, renames)
    rows = {}
    for k in sorted(set(kp) | set(kn)):
        if k in kp and k in kn:
            rows[k] = dict(equal=kp[k][0] == kn[k][0], parent=side(*kp[k]), new=side(*kn[k]))
            if k in was:
                rows[k]['parent_symbol'] = was[k]
            if dump and not rows[k]['equal']:                # the two normalised texts, for diff
                os.makedirs(dump, exist_ok=True)
                for tag, body in (('parent', kp[k][0]), ('new', kn[k][0])):
                    with open(os.path.join(dump, f'{k}.{tag}.s'), 'w') as f:
                        f.write('\n'.join(body) + '\n')
        else:
            rows[k] = dict(equal=False, parent=side(*kp[k]) if k in kp else None, new=side(*kn[k]) if k in kn else None)
    return rows


def demangled(names):
    if not names:
        return {}
    try:
        out = subprocess.run(['c++filt'] + names, check=True, capture_output=True, text=True).stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        out = names
    return dict(zip(names, out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--parent-tree', required=True, help='a checkout or copy of the parent commit')
    ap.add_argument('--files', nargs='+', default=FILES)
    ap.add_argument('--jobs', type=int, default=6)
    ap.add_argument('--out', default=None)
    ap.add_argument('--dump', default=None, help='a directory for the normalised texts of the kernels that differ')
    ap.add_argument('--rename', nargs=2, action='append', default=[], metavar=('PATTERN', 'REPLACEMENT'),
                    help='a parent symbol -> its new name (re.sub), for a kernel template that gained a parameter; repeatable')
    ap.add_argument('--new-only', nargs='*', default=[], metavar='REGEX',
                    help='demangled names of kernels this tree adds on purpose: listed, not counted as a difference')
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_tree)
    with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        res = dict(zip(args.files, pool.map(lambda f: compare(f, parent, ROOT, args.dump, args.rename), args.files)))
    doc = dict(tool='tools/isa_diff.py', files={}, renames=[list(r) for r in args.rename], added=[])
    bad = []
    for f, rows in res.items():
        names = demangled(list(rows))
        doc['files'][f] = dict(kernels=len(rows), equal=sum(r['equal'] for r in rows.values()),
                               rows={names[k]: dict(symbol=k, **r) for k, r in rows.items()})
        for k, r in rows.items():
            if r['parent'] is None and any(re.search(p, names[k]) for p in args.new_only):
                doc['added'].append(f'{f}: {names[k]}')
            elif not r['equal']:
                bad.append(f'{f}: {names[k]}')
    doc['all_equal'] = not bad
    doc['not_equal'] = bad
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    for f, d in doc['files'].items():
        print(f"{f}: {d['equal']} of {d['kernels']} kernels equal")
    for b in bad:
        print('NOT EQUAL', b)
    return 0 if not bad else 1


if __name__ == '__main__':
    sys.exit(main())
