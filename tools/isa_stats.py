"""Static figures of one kernel of csrc/woltka_hip.hip, from its gfx950
assembly: registers, LDS, scratch, barriers, and per stretch between
consecutive barriers (as the ISA lays them out) the vector, lane-move, scalar
and LDS instructions and the branches.  No GPU is needed.

  python tools/isa_stats.py [kernel ...] [--root DIR] [--asm FILE] [--total]

`kernel`: a substring of the kernel's symbol (default: dtok_fused_kernel and
dtok_fused_measure_kernel, where the tree has them).  `--root`: another
checkout of this repository (a parent, say) to compile instead of this one.
`--asm`: assembly that exists already (nothing is compiled).  The device code
is compiled with the flags of `__graft_entry__.build_native` plus `-S
--cuda-device-only` into a temporary directory that is removed afterwards.

Lines are classified by their prefix alone: `v_` (of those `v_readlane` /
`v_writelane` apart, as lane moves), `s_` (`s_barrier` ends a stretch), `ds_`;
a branch is an `s_` line whose operand is a label of the function."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
KEYS = ('valu', 'lane', 'salu', 'lds', 'branch')


def compile_asm(root, out):
    src = os.path.join(root, 'woltka_amd', 'csrc', 'woltka_hip.hip')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC',
           '-pthread', '-Wall', '-Wno-unused-function',
           '-DWK_BUILD_ID="isa_stats"', '-S', '--cuda-device-only',
           '-o', out, src]
    subprocess.check_call(cmd, cwd=os.path.dirname(out))


def kernels(asm):
    """symbol -> (body lines, trailer comment lines) of every kernel."""
    found = {}
    lines = asm.split('\n')
    entry = {m.group(1) for ln in lines
             for m in [re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln)] if m}
    i = 0
    while i < len(lines):
        m = re.match(r'(\S+):', lines[i])
        if m and m.group(1) in entry and m.group(1) not in found:
            j = i + 1
            while j < len(lines) and not lines[j].startswith('.Lfunc_end'):
                j += 1
            k = j
            while k < len(lines) and '.amdhsa_kernel' not in lines[k] \
                    and not re.match(r'\s*\.text', lines[k]):
                k += 1
            found[m.group(1)] = (lines[i + 1:j], lines[j:k])
            i = j
        i += 1
    return found


def resources(body, trailer):
    want = {'NumVgprs': 'VGPRs', 'TotalNumSgprs': 'SGPRs (with VCC etc.)',
            'LDSByteSize': 'LDS bytes', 'ScratchSize': 'scratch bytes',
            'Occupancy': 'occupancy'}
    res = {}
    for ln in trailer:
        m = re.match(r';\s*(\w+):\s*(\d+)', ln.strip())
        if m and m.group(1) in want:
            res.setdefault(want[m.group(1)], int(m.group(2)))
    for ln in body:
        m = re.match(r'\s*\.amdhsa_next_free_sgpr\s+(\d+)', ln)
        if m:
            res['next_free_sgpr'] = int(m.group(1))
    return res


def segments(body):
    segs = [dict.fromkeys(KEYS, 0)]
    for ln in body:
        op = ln.strip()
        if not op or op[0] in ';.' or op.endswith(':'):
            continue
        op = op.split(';')[0].split()
        name, args = op[0], ' '.join(op[1:])
        cur = segs[-1]
        if name.startswith('s_barrier'):
            segs.append(dict.fromkeys(KEYS, 0))
        elif name.startswith(('v_readlane', 'v_writelane')):
            cur['lane'] += 1
        elif name.startswith('v_'):
            cur['valu'] += 1
        elif name.startswith('ds_'):
            cur['lds'] += 1
        elif name.startswith('s_'):
            if re.search(r'\.LBB\d+_\d+', args):
                cur['branch'] += 1
            else:
                cur['salu'] += 1
    return segs


def report(sym, body, trailer, total_only):
    res = resources(body, trailer)
    segs = segments(body)
    reads = sum(1 for ln in body if ln.strip().startswith('v_readlane'))
    writes = sum(1 for ln in body if ln.strip().startswith('v_writelane'))
    print(f'== {sym}')
    print('   ' + ', '.join(f'{k} {v}' for k, v in res.items()))
    print(f'   barriers {len(segs) - 1}; lane moves {writes} + {reads} = '
          f'{writes + reads} (v_writelane + v_readlane)')
    head = f'   {"stretch":>8}' + ''.join(f'{k:>8}' for k in KEYS)
    print(head)
    if not total_only:
        for i, s in enumerate(segs):
            print(f'   {i:>8}' + ''.join(f'{s[k]:>8}' for k in KEYS))
    print(f'   {"all":>8}' + ''.join(f'{sum(s[k] for s in segs):>8}' for k in KEYS))
    print('   (v_ without lane moves; s_ without barriers and branches)')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('kernel', nargs='*')
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--asm')
    ap.add_argument('--total', action='store_true',
                    help='the whole kernel only, no stretches')
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as f:
            asm = f.read()
    else:
        with tempfile.TemporaryDirectory(prefix='isa_stats_') as tmp:
            out = os.path.join(tmp, 'woltka_hip.s')
            compile_asm(os.path.abspath(a.root), out)
            with open(out) as f:
                asm = f.read()
    ks = kernels(asm)
    names = a.kernel or ['dtok_fused_kernel', 'dtok_fused_measure_kernel']
    hit = 0
    for want in names:
        for sym, (body, trailer) in ks.items():
            if want in sym:
                report(sym, body, trailer, a.total)
                hit += 1
    if not hit:
        sys.exit(f'no kernel matches {names}; the file has {len(ks)}')


if __name__ == '__main__':
    main()
