#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 machine code of two builds of babelbrain_amd/csrc (refactor check).

    make -C <tree>/babelbrain_amd/csrc -O -j16 EXTRA=-Rpass-analysis=kernel-resource-usage > <tree>.log 2>&1     (both trees; -O keeps the
                                                            remarks of one compiler together: without it parallel compilers tear each other's lines)
    scripts/isa_identity.py <parent tree>/babelbrain_amd/csrc <parent>.log <branch tree>/babelbrain_amd/csrc <branch>.log [new=old ...] [kernel:new=old ...]

new=old (optional, e.g. bfd_outputs=bfd_api, bfd_bhte_kernels=bfd_bhte): kernels and resource records of object `new` of the second build are looked up under object `old`
of the first (code that moved from one source file to another). An `old` that the Makefile no longer names (a source file that was split up) is read from the
first build all the same.
kernel:new=old (optional): in the kernel names of the second build the text `new` is replaced by `old` before the lookup (a kernel that lost a template
parameter: kernel:12stress_fluidILb=12stress_fluidILb1ELb). Without it such a kernel is listed once under each "only in".

The fat binary section of every object is unbundled (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler --unbundle),
disassembled (llvm-objdump -d) and cut at the kernel symbols; the instruction text of a kernel (addresses and encodings dropped) and its resource remarks (registers, spills, scratch, occupancy, LDS) must be equal on both sides.
The literal of the s_add_u32 behind an s_getpc_b64 is left out of the comparison: it is the distance from the instruction to a constant of the object, which changes with
the kernels that lie between them and not with the kernel's code.
The s_nop filling behind a kernel's last instruction is left out as well: its length depends on the symbol that follows in the object.
Exit status 0 = nothing differs and no kernel exists only in the second build."""
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/lib/llvm/bin')

def sources():
    """the objects of the library: the SRC := line of csrc/Makefile, so that a new source file is compared from the day it is built"""
    makefile = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'babelbrain_amd', 'csrc', 'Makefile')
    line = next(l for l in open(makefile) if re.match(r'^SRC\s*:=', l))
    return [s[:-len('.hip')] for s in line.split(':=', 1)[1].split()]


SRC = sources()


def kernels(obj, tmp):
    fb, co = os.path.join(tmp, 'x.fb'), os.path.join(tmp, 'x.co')
    if subprocess.call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fb, obj, os.devnull], stderr=subprocess.DEVNULL) != 0:
        return {}       # an object without device code
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950',
                           '--input=' + fb, '--output=' + co])
    text = subprocess.check_output([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', co], text=True)
    out, cur = {}, None
    for line in text.split('\n'):
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and line.strip() != '...':      # '...': objdump's mark for the zero padding behind a kernel
            ins = re.sub(r'\s*//.*$', '', line).strip()
            if cur and cur[-1].startswith('s_getpc_b64'):      # the low word of a pc-relative address: where the object's data lies from here, not code
                ins = re.sub(r'^(s_add_u32 \S+ \S+) 0x[0-9a-f]+$', r'\1 <pc-relative>', ins)
            cur.append(ins)
    for ins in out.values():      # the s_nop filling between a kernel's end and the next aligned symbol: it changes with the kernel that follows
        while ins and ins[-1] == 's_nop 0':
            ins.pop()
    return out


def owner(f):
    """the source a remark belongs to: an include file of kernels counts for the source it is named after (bfd_bhte_monitors.inc -> bfd_bhte.hip; its kernels are
    compiled into bfd_bhte_kernels.o, so compare that object with bfd_bhte_kernels=bfd_bhte, which puts both under one name)"""
    f = os.path.basename(f)
    if f.endswith('.inc'):
        f = max((s for s in SRC if f.startswith(s)), key=len) + '.hip'
    return f


def resources(log):
    """remarks of a (possibly parallel) build: per source file in order, Function Name opens a record"""
    res, cur = {}, {}
    for line in open(log, errors='replace'):
        m = re.match(r'^(\S+?\.(?:hip|inc)):\d+:\d+: remark: (.*?) \[-Rpass-analysis=kernel-resource-usage\]', line)
        if not m:
            continue
        f, body = m.group(1), m.group(2).strip()
        if body.startswith('Function Name:'):
            cur[f] = res.setdefault((owner(f), body.split(':', 1)[1].strip()), [])
        elif f in cur:
            cur[f].append(body)
    return res


def main():
    dirA, logA, dirB, logB = sys.argv[1:5]
    moved = dict(a.split('=') for a in sys.argv[5:] if not a.startswith('kernel:'))
    renamed = [a[len('kernel:'):].split('=') for a in sys.argv[5:] if a.startswith('kernel:')]

    def old_name(name):
        for new, old in renamed:
            name = name.replace(new, old)
        return name
    SRC.extend(sorted(set(moved.values()) - set(SRC)))
    with tempfile.TemporaryDirectory() as tmp:
        A, B = {}, {}
        for s in SRC:
            for d, K in ((dirA, A), (dirB, B)):
                for name, ins in kernels(os.path.join(d, s + '.o'), tmp).items():
                    key = (moved.get(s, s), old_name(name)) if K is B else (s, name)
                    assert key not in K, 'kernel in two objects of one build (a copy): %s %s' % key
                    K[key] = ins
    RA = resources(logA)
    RB = {(moved.get(f[:-4], f[:-4]) + '.hip', old_name(name)): v for (f, name), v in resources(logB).items()}
    onlyA, onlyB = sorted(set(A) - set(B)), sorted(set(B) - set(A))
    print('code symbols: first build %d, second build %d, in both %d' % (len(A), len(B), len(set(A) & set(B))))
    print('instructions compared: %d' % sum(len(A[k]) for k in set(A) & set(B)))
    print('only in the first build (%d):' % len(onlyA))
    for k in onlyA:
        print('    %s  %s' % k)
    print('only in the second build (%d):' % len(onlyB))
    for k in onlyB:
        print('    %s  %s' % k)
    diff = [k for k in sorted(set(A) & set(B)) if A[k] != B[k]]
    print('kernels whose instruction stream differs: %d' % len(diff))
    for k in diff:
        n = next((i for i, (x, y) in enumerate(zip(A[k], B[k])) if x != y), min(len(A[k]), len(B[k])))
        print('    %s  %s: %d / %d instructions, first difference at %d' % (k[0], k[1], len(A[k]), len(B[k]), n))
    ra = {k: v for k, v in RA.items() if k in RB}
    rdiff = [k for k in sorted(ra) if RA[k] != RB[k]]
    print('resource records: first build %d, second build %d; differing among the common %d: %d' % (len(RA), len(RB), len(ra), len(rdiff)))
    for k in rdiff:
        print('    %s %s\n      first:  %s\n      second: %s' % (k[0], k[1], '; '.join(RA[k]), '; '.join(RB[k])))
    hist = collections.Counter(s for s, _ in A)
    print('symbols per object (first build): ' + ', '.join('%s %d' % (s, hist[s]) for s in SRC))
    return 1 if (diff or rdiff or onlyB) else 0


if __name__ == '__main__':
    sys.exit(main())
