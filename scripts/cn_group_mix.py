#!/usr/bin/env python3
"""Static instruction stream of the check pass in the BP loops of a kernel, per group of four positions and by class:
    scripts/cn_group_mix.py <file.s> <mangled kernel name prefix> <KG> [min LDS instructions]
Sibling of scripts/loop_mix.py (same attribution of basic blocks to their innermost loop, from the compiler's asm comments).  In every
loop whose body holds a v_min_f64 with an |x| operand (the clip of the check pass, csrc/swd_osdw_kernel.h, bp_run) the text of the loop
is cut in two at the first v_bcnt_u32_b32 (the parity count that follows the last read group) and at the first s_barrier:
    read phase          loop header .. first v_bcnt_u32_b32   the KG groups of four message reads with the two-minimum update
    merge + write phase .. first s_barrier                    quad merge, argslot re-read, the KG groups of four message stores
Both are printed as totals and divided by KG.  Classes:
    algorithm   ds_read / ds_write of messages, v_min / v_max / v_cmp on f64, v_cndmask, v_addc_co (sign shift), v_bcnt, v_and_or / v_or /
                v_lshl (sign of a stored message), v_mul_f64
    lane reads  v_readlane / v_writelane (SGPR spills kept in VGPR lanes)
    s_nop       wait states
    copies      v_mov_b32, unpack of the packed offsets (v_and 0xffff, v_lshrrev 16), v_add_u32 x, 0, y
    guards      s_cmp*, s_cbranch*, s_branch, s_cselect, s_and / s_andn2 / s_or / s_mov of 64-bit masks
    constants   s_mov_b32 of a literal, v_mov_b64
    other       whatever is left (s_waitcnt among it)"""
import re, sys, collections
src, name, KG = sys.argv[1], sys.argv[2], int(sys.argv[3])
min_ds = int(sys.argv[4]) if len(sys.argv) > 4 else 40
text = open(src).read().split('\n')
start = next(i for i, l in enumerate(text) if l.startswith(name) and ':' in l)
end = next(i for i in range(start, len(text)) if 's_endpgm' in text[i])
loops = collections.OrderedDict()
cur_loop, cur_blk = None, None
for i in range(start + 1, end):
    l = text[i]
    m = re.match(r'^(\.LBB\d+_\d+):(.*)', l)
    if m:
        cur_blk, cur_loop, rest = m.group(1)[2:], None, m.group(2)
        if 'Loop Header' in rest: cur_loop = (cur_blk, int(re.search(r'Depth=(\d+)', rest).group(1)))
        mm = re.search(r'in Loop: Header=(BB\d+_\d+) Depth=(\d+)', rest)
        if mm: cur_loop = (mm.group(1), int(mm.group(2)))
        continue
    s = l.strip()
    if s.startswith(';'):
        if cur_loop is None:
            if 'Loop Header' in s and 'Depth=' in s: cur_loop = (cur_blk, int(re.search(r'Depth=(\d+)', s).group(1)))
            mm = re.search(r'in Loop: Header=(BB\d+_\d+) Depth=(\d+)', s)
            if mm: cur_loop = (mm.group(1), int(mm.group(2)))
        continue
    if not s or s.startswith('.') or cur_loop is None: continue
    loops.setdefault(cur_loop, []).append(s)

CLASSES = ('algorithm', 'lane reads', 's_nop', 'copies', 'guards', 'constants', 'other')


def klass(s):
    op = s.split()[0]
    args = s[len(op):]
    if op.startswith('v_readlane') or op.startswith('v_writelane'): return 'lane reads'
    if op == 's_nop': return 's_nop'
    if op.startswith('ds_read_b64') or op.startswith('ds_write_b64') or op.startswith('ds_read2_b64') or op.startswith('ds_write2_b64'): return 'algorithm'
    if re.match(r'v_(min|max|cmp_\w+|mul)_f64', op) or op.startswith('v_cndmask') or op.startswith('v_addc_co') or op.startswith('v_bcnt'): return 'algorithm'
    if op.startswith('v_and_or_b32') or op.startswith('v_or_b32') or op.startswith('v_lshl_or') or op.startswith('v_xor_b32'): return 'algorithm'
    if op.startswith('v_mov_b64'): return 'constants'
    if op.startswith('s_mov_b32') and re.search(r',\s*0x[0-9a-f]+\s*$', args): return 'constants'
    if op.startswith('v_mov_b32'): return 'copies'
    if op.startswith('v_and_b32') and '0xffff' in args: return 'copies'
    if op.startswith('v_lshrrev_b32') and re.search(r',\s*16,', args): return 'copies'
    if op.startswith('v_add_u32') and re.search(r',\s*0,', args): return 'copies'
    if op.startswith('s_cmp') or op.startswith('s_cbranch') or op == 's_branch' or op.startswith('s_cselect'): return 'guards'
    if re.match(r's_(and|andn2|or|mov|and_saveexec|or_saveexec)_b64', op): return 'guards'
    return 'other'


for (h, depth), ins in loops.items():
    if sum(1 for s in ins if s.startswith('ds_')) < min_ds: continue
    if not any(re.match(r'v_min_f64 [^,]+, \|', s) for s in ins): continue
    cut1 = next((i for i, s in enumerate(ins) if s.startswith('v_bcnt_u32_b32')), None)
    cut2 = next((i for i, s in enumerate(ins) if s.startswith('s_barrier')), None)
    if cut1 is None or cut2 is None or cut2 < cut1: continue
    print(f"loop {h} depth {depth}: {len(ins)} instructions, {sum(1 for s in ins if s.startswith('v_readlane') or s.startswith('v_writelane'))} lane reads / writes and {sum(1 for s in ins if s.startswith('s_nop'))} s_nop in the whole body")
    for label, part in (('read phase', ins[:cut1]), ('merge + write phase', ins[cut1:cut2])):
        c = collections.Counter(klass(s) for s in part)
        print(f"  {label:20s} {len(part):5d} = {len(part) / KG:5.1f} per group | " + '  '.join(f"{k} {c[k]} ({c[k] / KG:.1f})" for k in CLASSES))
