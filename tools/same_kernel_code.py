"""Per-kernel form of tests/wave_emu/same_device_code.py: is the gfx950 code of every kernel that a source held at a git
revision the same in the working tree, when the file has GAINED kernels (so that the whole-file comparison must differ)?

    python tools/same_kernel_code.py [--rev HEAD] samattn.hip samdec.hip

For every kernel that differs it prints the instruction count and the register / scratch / LDS fields of the kernel descriptor
on both sides.  Splits both assemblies into functions (label ... .Lfunc_end) and compares the instruction lines of every function of the
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


def row(fn, res, k):
    if k not in fn:
        return 'absent'
    n = sum(1 for b in fn[k] if not b.endswith(':') and not b.lstrip().startswith('.'))
    return f'{n} instructions, ' + ', '.join(f'{r} {res[k].get(r)}' for r in RES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rev', default='HEAD')
    ap.add_argument('sources', nargs='+')
    a = ap.parse_args()
    rc = 0
    with tempfile.TemporaryDirectory() as tmp:
        csrc = os.path.join(tmp, 'rsprompter_amd', 'csrc')
        os.makedirs(csrc)
        os.makedirs(os.path.join(tmp, 'include'))
        for rel in headers_at(a.rev):
            open(os.path.join(tmp, rel), 'wb').write(subprocess.check_output(['git', '-C', ROOT, 'show', f'{a.rev}:{rel}']))
        for name in a.sources:
            rel = 'rsprompter_amd/csrc/' + name
            open(os.path.join(tmp, rel), 'wb').write(subprocess.check_output(['git', '-C', ROOT, 'show', f'{a.rev}:{rel}']))
            old_asm = device_asm(os.path.join(tmp, rel), os.path.join(tmp, name + '.old.s'))
            new_asm = device_asm(os.path.join(ROOT, rel), os.path.join(tmp, name + '.new.s'))
            old, new = functions(old_asm), functions(new_asm)
            old_res, new_res = resources(old_asm), resources(new_asm)
            bad = [k for k in old if old[k] != new.get(k)]
            added = [k for k in new if k not in old]
            print(f'{name}: {len(old)} kernels at {a.rev}, {len(old) - len(bad)} instruction-identical in the working tree, '
                  f'{len(bad)} different or missing, {len(added)} new')
            for k in bad:
                print('  DIFFERENT:', k)
                print(f'    {a.rev}: {row(old, old_res, k)}')
                print(f'    tree: {row(new, new_res, k)}')
            for k in added:
                print('  new:', k)
                print(f'    tree: {row(new, new_res, k)}')
            rc |= 1 if bad or not old else 0
    return rc


if __name__ == '__main__':
    sys.exit(main())
