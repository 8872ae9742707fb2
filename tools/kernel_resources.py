"""Per-kernel resources of two builds side by side, from device assembly.

    hipcc <the file's Makefile flags> --cuda-device-only -S x.hip -o A/x.s      (once per tree)
    python tools/kernel_resources.py A B [--only REGEX] [--changed]

For every kernel of every .s file present in both directories: VGPRs, SGPRs, scratch bytes, LDS bytes, occupancy (the compiler's
kernel-info comments) and the instruction count, as `A -> B` where they differ, and whether the instruction streams are identical
once comments, label numbers and symbol names are removed: `yes`, `regs` (identical only once register numbers are removed too:
the same instructions in the same order on other registers) or `no`.  Reads text; runs nothing on a GPU.
"""
import argparse
import os
import re
import shutil
import subprocess

INFO = {'vgpr': r'; NumVgprs: (\d+)', 'agpr': r'; NumAgprs: (\d+)', 'sgpr': r'; TotalNumSgprs: (\d+)', 'scratch': r'; ScratchSize: (\d+)',
        'lds': r'; LDSByteSize: (\d+)', 'occ': r'; Occupancy: (\d+)'}


def kernels(path):
    """{mangled name: (info dict, [normalised instruction, ...])} of one assembly file."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r'^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:.*?^; Kernel info:\n(.*?)^\t\.', text, re.S | re.M):
        name, body, info = m.groups()
        if '.amdhsa_kernel ' + name not in text:
            continue
        ins = []
        for line in body.split('\n'):
            line = line.split(';')[0].strip()
            if not line or line.startswith('.') or line.endswith(':'):
                continue
            ins.append(re.sub(r'\b_Z\w+', 'SYM', re.sub(r'\.LBB\d+_\d+', 'L', line)))
        out[name] = ({k: int(re.search(p, info).group(1)) for k, p in INFO.items()}, ins)
    return out


def demangle(names):
    tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    if not tool or not names:
        return {n: n for n in names}
    res = subprocess.run([tool], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    short = lambda s: re.sub(r'\(anonymous namespace\)::', '', re.sub(r'^void ', '', s.split('(')[0] if '<' not in s else s[:s.rindex('>(') + 1]))
    return {n: short(r).replace('__hip_bfloat16', 'bf16').replace('unsigned short', 'bf16') for n, r in zip(names, res)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('a')
    ap.add_argument('b')
    ap.add_argument('--only', default='', help='regex on the demangled kernel name')
    ap.add_argument('--changed', action='store_true', help='only kernels whose instruction stream differs')
    args = ap.parse_args()
    cell = lambda x, y: str(x) if x == y else f'{x} -> {y}'
    print('| file | kernel | VGPR | AGPR | SGPR | scratch | LDS | occupancy | instructions | same stream |')
    print('|---|---|---|---|---|---|---|---|---|---|')
    n_same = n_all = 0
    noreg = lambda ins: [re.sub(r'\b[vsa](\d+|\[\d+:\d+\])', 'r', i) for i in ins]
    for f in sorted(set(os.listdir(args.a)) & set(os.listdir(args.b))):
        if not f.endswith('.s'):
            continue
        ka, kb = kernels(os.path.join(args.a, f)), kernels(os.path.join(args.b, f))
        names = demangle(sorted(set(ka) | set(kb)))
        for n in sorted(names, key=names.get):
            if not re.search(args.only, names[n]):
                continue
            if n not in ka or n not in kb:
                print(f'| {f} | `{names[n]}` | only in {"A" if n in ka else "B"} |||||||||')
                continue
            (ia, sa), (ib, sb) = ka[n], kb[n]
            n_all += 1
            n_same += sa == sb
            if args.changed and sa == sb:
                continue
            print(f'| {f} | `{names[n]}` | ' + ' | '.join(cell(ia[k], ib[k]) for k in INFO) + f' | {cell(len(sa), len(sb))} | {"yes" if sa == sb else ("regs" if noreg(sa) == noreg(sb) else "no")} |')
    print(f'\n{n_same} of {n_all} kernels have an identical instruction stream.')


if __name__ == '__main__':
    main()
