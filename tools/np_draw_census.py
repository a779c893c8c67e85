#!/usr/bin/env python3
"""Static ISA census of k_np_draw_compact (the int16 draw pass of the numpy streams), priced in SIMD cycles: the byte-parked
instantiation <EmitI16B8> the bench runs, or with --emit EmitI16 the int16-parked one.

Compiles vkit_amd/csrc/nprand.hip for gfx950 with the Makefile's flags, splits the kernel into basic blocks and prices every VALU
instruction with the issue rates measured by tools/ubench (cycles per wavefront instruction per SIMD: profiles/r2_instruction_rates.md,
overridden by profiles/np_instruction_rates.md where both have a form).  LDS and SALU instructions are counted, not priced: they issue
to other units.  The phase-1 loop (the depth-2 loop with the most v_mad_u64_u32; one ds_read_b128 per round) and the compaction block (the
most v_readlane) are summed per round, so are the blocks that widen parked bytes on the way to the slot (v_pk_ashrrev_i16); the event-push blocks of phase 1 (the ones holding ds_write_b128) run in the ~62 % of rounds
that have a draw that is not a fast accept and are listed apart.
Usage: tools/np_draw_census.py [--emit EmitI16B8|EmitI16] [--src nprand.hip] [-D NAME=VALUE ...] [--asm out.s] > profiles/np_draw_census.md"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden', '-Wno-unused-function',
         '-S', '--cuda-device-only']
KERNEL_OF = {'EmitI16': '_ZN12_GLOBAL__N_117k_np_draw_compactINS_7EmitI16EEE', 'EmitI16B8': '_ZN12_GLOBAL__N_117k_np_draw_compactINS_9EmitI16B8EEE'}
KERNEL = KERNEL_OF['EmitI16B8']
RATE_FILES = ['profiles/r2_instruction_rates.md', 'profiles/np_instruction_rates.md']
# forms whose ubench row measures something else than the form the kernel uses
ALIAS = {
    'v_cndmask_b32': 'v_cndmask_b32_e64_sgpr',       # the e32 row is a chain through vcc; the kernel's selects are independent
    'v_cmp_ge_u64': 'v_cmp_ge_u64_e64_sgpr',
    'v_cmp_gt_u32': 'v_cmp_lt_u32',
    'v_cmp_lt_u32_e64': 'v_cmp_lt_u32_e64_sgpr',
    'v_alignbit_b32': 'v_alignbit_b32_9',
    'v_lshrrev_b64': 'v_lshrrev_b64_vshift',
    'v_lshlrev_b64': 'v_lshlrev_b64_vshift',
}
DEFAULT_RATE = 4.5


def load_rates():
    rates = {}
    for rel in RATE_FILES:
        path = os.path.join(ROOT, rel)
        if not os.path.exists(path):
            continue
        for line in open(path):
            m = re.match(r'\|\s*([a-z0-9_]+)\s*\|\s*[\d.]+\s*\|\s*([\d.]+)\s*\|', line)
            if m:
                rates[m.group(1)] = float(m.group(2))
    return rates


def base_op(op):
    return re.sub(r'_(e32|e64|sdwa|dpp)$', '', op)


def price(op, rates, text=''):
    """(cycles, priced?) of one VALU instruction (`text`: the whole instruction, for the forms whose rate depends on its operands)."""
    b = base_op(op)
    keys = (ALIAS.get(b), b, op)
    if b == 'v_bitop3_b32' and re.search(r'[ ,]s(\d+|\[)', text):   # an SGPR operand: the VOP3 rate
        keys = ('v_bitop3_b32_sgpr',) + keys
    for key in keys:
        if key and key in rates:
            return rates[key], True
    return DEFAULT_RATE, False


def compile_asm(src, defines):
    fd, out = tempfile.mkstemp(suffix='.s')
    os.close(fd)
    cmd = ['/opt/rocm/bin/hipcc', *FLAGS, *[f'-D{d}' for d in defines], '-I', os.path.join(ROOT, 'vkit_amd', 'csrc'), '-o', out, src]
    subprocess.run(cmd, check=True, capture_output=True)
    text = open(out).read()
    os.unlink(out)
    return text


def kernel_blocks(asm):
    lines = asm.split('\n')
    start = next(i for i, l in enumerate(lines) if l.startswith(KERNEL) and l.rstrip().endswith(':') is False and ':' in l
                 and not l.startswith('\t'))
    blocks, cur = [], None
    for l in lines[start:]:
        if l.startswith('.Lfunc_end'):
            break
        m = re.match(r'^(\.LBB\w+|_Z\w+):\s*(;.*)?$', l)
        if m:
            note = m.group(2) or ''
            hdr = re.search(r'Header=(BB\w+) Depth=(\d)', note)
            own = re.search(r'Loop Header: Depth=(\d)', note)
            nested = re.search(r'Parent Loop (BB\w+) Depth=(\d)', note)   # the header of a loop inside another
            name = m.group(1)
            if own:
                loop, depth = name[len('.L'):], int(own.group(1))
            elif nested and not hdr:
                loop, depth = name[len('.L'):], int(nested.group(2)) + 1
            elif hdr:
                loop, depth = hdr.group(1), int(hdr.group(2))
            else:
                loop, depth = None, 0
            cur = {'name': name, 'loop': loop, 'depth': depth, 'ops': []}
            blocks.append(cur)
            continue
        s = l.strip()
        if cur is None or not s or s.startswith(('.', ';')):
            continue
        op = s.split()[0]
        cur['ops'].append(op)
        cur.setdefault('text', []).append(s)
        if op.startswith(('s_cbranch', 's_branch')):     # a branch ends the basic block; what falls through is the next one
            cur = {'name': f"{cur['name'].split('+')[0]}+{len(blocks)}", 'loop': cur['loop'], 'depth': cur['depth'], 'ops': []}
            blocks.append(cur)
    return blocks


def is_push(block):
    """A piece of the event push: the slot (v_mbcnt) or the queue writes (ds_write_b128), run only in rounds with slow lanes."""
    return any(op.startswith('v_mbcnt') or op == 'ds_write_b128' for op in block['ops'])


def summarize(block, rates):
    c = collections.Counter()
    unpriced = set()
    for op, text in zip(block['ops'], block.get('text', [])):
        if op.startswith('v_'):
            cyc, ok = price(op, rates, text)
            c['valu'] += 1
            c['cycles'] += cyc
            if not ok:
                unpriced.add(op)
        elif op.startswith('ds_'):
            c['lds'] += 1
        elif op.startswith('s_'):
            c['salu'] += 1
        elif op.startswith(('global_', 'buffer_', 'flat_')):
            c['vmem'] += 1
    return c, unpriced


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--emit', default='EmitI16B8', choices=sorted(KERNEL_OF))
    ap.add_argument('--src', default=os.path.join(ROOT, 'vkit_amd', 'csrc', 'nprand.hip'))
    ap.add_argument('-D', dest='defines', action='append', default=[])
    ap.add_argument('--asm', help='also write the assembly here')
    ap.add_argument('--min-ops', type=int, default=8, help='list blocks with at least this many instructions')
    args = ap.parse_args()
    global KERNEL
    KERNEL = KERNEL_OF[args.emit]
    rates = load_rates()
    asm = compile_asm(args.src, args.defines)
    if args.asm:
        open(args.asm, 'w').write(asm)
    blocks = kernel_blocks(asm)
    rows = [(b, *summarize(b, rates)) for b in blocks]
    mads = collections.Counter()
    for b in blocks:
        if b['depth'] == 2:
            mads[b['loop']] += b['ops'].count('v_mad_u64_u32')
    p1 = mads.most_common(1)[0][0] if mads else None
    comp = max(blocks, key=lambda b: b['ops'].count('v_readlane_b32'))
    all_unpriced = set()
    print(f'# k_np_draw_compact<{args.emit}>: VALU cycles per basic block ({os.path.relpath(args.src, ROOT)}'
          f'{", " + " ".join("-D" + d for d in args.defines) if args.defines else ""})\n')
    print('Cycles = sum over the block\'s VALU instructions of the issue cycles per wavefront instruction per SIMD (tools/ubench; '
          f'forms without a row: {DEFAULT_RATE}).  LDS / SALU / VMEM: instruction counts.\n')
    print('| block | loop | VALU | VALU cycles | LDS | SALU | VMEM |')
    print('|---|---|---|---|---|---|---|')
    for b, c, un in rows:
        all_unpriced |= un
        if len(b['ops']) < args.min_ops:
            continue
        tag = ''
        if p1 and b['loop'] == p1:
            tag = ' (phase 1' + (', event push)' if is_push(b) else ')')
        if b is comp:
            tag = ' (compaction)'
        print(f"| {b['name']}{tag} | {b['loop'] or ''} d{b['depth']} | {c['valu']} | {c['cycles']:.1f} | {c['lds']} | {c['salu']} | {c['vmem']} |")
    if p1:
        body = [r for r in rows if r[0]['loop'] == p1 and not is_push(r[0])]
        push = [r for r in rows if r[0]['loop'] == p1 and is_push(r[0])]
        bv, bc = sum(r[1]['valu'] for r in body), sum(r[1]['cycles'] for r in body)
        pv, pc = sum(r[1]['valu'] for r in push), sum(r[1]['cycles'] for r in push)
        lds = sum(r[1]['lds'] for r in body)
        k1 = sum(r[0]['ops'].count('ds_read_b128') for r in body) or 2     # rounds per trip of the loop: one table look-up each
        print('\n| per round | VALU | VALU cycles | LDS |')
        print('|---|---|---|---|')
        print(f'| phase 1, every round (loop of {k1} rounds / {k1}) | {bv / k1:.1f} | {bc / k1:.1f} | {lds / k1:.1f} |')
        print(f'| phase 1, event push (when taken; x ~0.62 per round) | {pv / k1:.1f} | {pc / k1:.1f} | {sum(r[1]["lds"] for r in push) / k1:.1f} |')
        cc, _ = summarize(comp, rates)
        k = comp['ops'].count('v_readlane_b32') // 2
        if k:
            print(f'| compaction ({comp["name"]}, {k} rounds) | {cc["valu"] / k:.1f} | {cc["cycles"] / k:.1f} | {cc["lds"] / k:.1f} |')
        # the slot write of the byte-parked pass: per 16-byte group a perm and a packed shift per dword, kTile / 512 groups per lane
        widen = [r for r in rows if 'v_pk_ashrrev_i16' in r[0]['ops']]
        wv, wc = sum(r[1]['valu'] for r in widen), sum(r[1]['cycles'] for r in widen)
        if widen and k:
            print(f'| slot write with widening ({len(widen)} blocks, {k} rounds) | {wv / k:.1f} | {wc / k:.1f} | {sum(r[1]["lds"] for r in widen) / k:.1f} |')
        kk = k or 1
        print(f'| **sum (event push at 0.62)** | **{(bv + 0.62 * pv) / k1 + (cc["valu"] + wv) / kk:.1f}** | '
              f'**{(bc + 0.62 * pc) / k1 + (cc["cycles"] + wc) / kk:.1f}** | |')
    if all_unpriced:
        print(f'\nForms without a measured rate (priced at {DEFAULT_RATE}): ' + ', '.join(sorted(all_unpriced)))


if __name__ == '__main__':
    sys.exit(main())
