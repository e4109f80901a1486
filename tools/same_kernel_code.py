"""Per-kernel form of tests/wave_emu/same_device_code.py: is the gfx950 code of every kernel that a source held at a git
revision the same in the working tree, when the file has GAINED kernels (so that the whole-file comparison must differ)?

    python tools/same_kernel_code.py [--rev HEAD] samattn.hip samdec.hip
    python tools/same_kernel_code.py --moved mask_polygons.hip:mp_count_kernel=run_pieces.hip:run_pieces_count_kernel

A kernel is the same when its instructions AND the register / scratch / LDS fields of its kernel descriptor are; for every
kernel that differs both are printed for both sides.  A kernel of the revision that the tree no longer has is listed as gone
(and does not fail the comparison: say where it went with --moved).  --moved OLDFILE:OLDNAME=NEWFILE:NEWNAME compares one
kernel of a file at the revision with a kernel of another name in another file of the tree: its own symbol, which a moved or
renamed kernel cannot keep, is written as <self> on both sides.  Splits both assemblies into functions (label ... .Lfunc_end) and compares the instruction lines of every function of the
revision with the function of the same symbol in the working tree.  Labels of basic blocks and function-end markers are
numbered per file, so they are renumbered per function in order of first appearance before comparing."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'wave_emu'))
from same_device_code import device_asm, headers_at  # noqa: E402


def functions(lines):
    """{symbol: [instruction lines]} of the .text functions of a device assembly"""
    out, name, body = {}, None, []
    for ln in lines:
        m = re.match(r'^(_Z\w+|[A-Za-z_]\w*):$', ln)
        if m and not ln.startswith('.L') and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r'^\.Lfunc_end\d+:$', ln):
                ids = {}
                norm = []
                for b in body:
                    norm.append(re.sub(r'\.L(BB|tmp|func_end)?\d+(_\d+)?', lambda k: ids.setdefault(k.group(0), f'.L{len(ids)}'), b))
                out[name] = norm
                name = None
            elif not ln.lstrip().startswith(('.p2align', '.section', '.type', '.globl', '.weak', '.protected', '.hidden')):
                body.append(ln)
    return out


RES = ('next_free_vgpr', 'next_free_sgpr', 'private_segment_fixed_size', 'group_segment_fixed_size')


def resources(lines):
    """{symbol: the RES fields of its .amdhsa_kernel descriptor}"""
    out, name = {}, None
    for ln in lines:
        w = ln.split()
        if w[0] == '.amdhsa_kernel':
            name = w[1]
            out[name] = {}
        elif name and w[0].startswith('.amdhsa_') and w[0][8:] in RES:
            out[name][w[0][8:]] = w[1]
    return out


def symbol_of(fn, kernel):
    """the one symbol of the assembly whose name holds the source name of a kernel"""
    hits = [k for k in fn if k == kernel or f'{len(kernel)}{kernel}' in k]          # extern "C", or the mangled <length><name>
    if len(hits) != 1:
        raise SystemExit(f'{kernel}: {len(hits)} symbols match: {hits}')
    return hits[0]


def row(fn, res, k):
    if k not in fn:
        return 'absent'
    n = sum(1 for b in fn[k] if not b.endswith(':') and not b.lstrip().startswith('.'))
    return f'{n} instructions, ' + ', '.join(f'{r} {res[k].get(r)}' for r in RES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rev', default='HEAD')
    ap.add_argument('--moved', action='append', default=[], metavar='OLDFILE:OLDNAME=NEWFILE:NEWNAME')
    ap.add_argument('sources', nargs='*')
    a = ap.parse_args()
    moved = [tuple(side.split(':') for side in m.split('=')) for m in a.moved]
    rc = 0
    with tempfile.TemporaryDirectory() as tmp:
        csrc = os.path.join(tmp, 'rsprompter_amd', 'csrc')
        os.makedirs(csrc)
        os.makedirs(os.path.join(tmp, 'include'))
        for rel in headers_at(a.rev):
            open(os.path.join(tmp, rel), 'wb').write(subprocess.check_output(['git', '-C', ROOT, 'show', f'{a.rev}:{rel}']))
        def old_side(name):
            rel = 'rsprompter_amd/csrc/' + name
            open(os.path.join(tmp, rel), 'wb').write(subprocess.check_output(['git', '-C', ROOT, 'show', f'{a.rev}:{rel}']))
            asm = device_asm(os.path.join(tmp, rel), os.path.join(tmp, name + '.old.s'))
            return functions(asm), resources(asm)

        def new_side(name):
            asm = device_asm(os.path.join(ROOT, 'rsprompter_amd/csrc/' + name), os.path.join(tmp, name + '.new.s'))
            return functions(asm), resources(asm)

        for name in a.sources:
            (old, old_res), (new, new_res) = old_side(name), new_side(name)
            gone = [k for k in old if k not in new]
            bad = [k for k in old if k in new and (old[k] != new[k] or old_res[k] != new_res[k])]
            added = [k for k in new if k not in old]
            print(f'{name}: {len(old)} kernels at {a.rev}; of the {len(old) - len(gone)} that the working tree has, '
                  f'{len(old) - len(gone) - len(bad)} identical (instructions, VGPR / SGPR / scratch / LDS), {len(bad)} different; '
                  f'{len(gone)} gone, {len(added)} new')
            for k in bad:
                print('  DIFFERENT:', k)
                print(f'    {a.rev}: {row(old, old_res, k)}')
                print(f'    tree: {row(new, new_res, k)}')
            for k in gone:
                print('  gone:', k)
                print(f'    {a.rev}: {row(old, old_res, k)}')
            for k in added:
                print('  new:', k)
                print(f'    tree: {row(new, new_res, k)}')
            rc |= 1 if bad or not old else 0
        for (old_file, old_name), (new_file, new_name) in moved:
            (old, old_res), (new, new_res) = old_side(old_file), new_side(new_file)
            ko, kn = symbol_of(old, old_name), symbol_of(new, new_name)
            same = [b.replace(ko, '<self>') for b in old[ko]] == [b.replace(kn, '<self>') for b in new[kn]] and old_res[ko] == new_res[kn]
            print(f'{old_file} {old_name} at {a.rev} -> {new_file} {new_name} in the working tree: '
                  f'{"identical (instructions, VGPR / SGPR / scratch / LDS)" if same else "DIFFERENT"}')
            print(f'    {a.rev}: {row(old, old_res, ko)}')
            print(f'    tree: {row(new, new_res, kn)}')
            rc |= 0 if same else 1
    return rc


if __name__ == '__main__':
    sys.exit(main())
