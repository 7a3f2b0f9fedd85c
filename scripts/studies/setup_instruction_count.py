#!/usr/bin/env python3
"""setup_instruction_count.py <kr_trace_kernels.hip.s> [kernel substring ...]

Static size of what a wave of a per-ray trace kernel runs OUTSIDE its loops, in the device assembly `make -C ntrace_amd/csrc resources`
writes: the wave set-up (launch scalars, the ray, the FAST and octant votes, the reciprocals), the dispatch to a loop instance and the
result store.  Counted per basic block by the compiler's own loop annotations, so the figure does not depend on where the blocks were laid
out (a count "from the entry to the prologue's first s_load_dwordx16" in layout order does: one more loop instance moves it by a hundred).
Printed beside it, both in layout order: the instructions from the entry to the first loop header, and from the entry to the first
s_load_dwordx16 behind the ray's own loads (the prologue's first record).  Default kernels: the AO launch trace_bvh_perray<1, false, true, true> and trace_bvh_perray_mini.
No GPU needed."""
import re
import sys


def main():
    path = sys.argv[1]
    wants = sys.argv[2:] or ["trace_bvh_perrayILi1ELb0ELb1ELb1EE", "trace_bvh_perray_miniE"]
    text = open(path).read().split("\n")
    is_inst = lambda l: l.startswith("\t") and not l.strip().startswith((";", ".")) and l.strip() != ""
    block_start = re.compile(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)")
    for want in wants:
        start = next(i for i, l in enumerate(text) if re.match(r"^_ZN3ntr\w+:", l) and want in l)
        end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
        outside, head, in_loop, before_first_loop = [], [], False, True
        to_record, ray_loaded = [], False   # layout order from the entry to the first s_load_dwordx16 behind the ray's own loads
        for l in text[start + 1:end]:
            if is_inst(l):
                if l.strip().startswith("global_load_dwordx4"):
                    ray_loaded = True
                if ray_loaded and l.strip().startswith("s_load_dwordx16"):
                    break
                to_record.append(l.strip())
        for l in text[start + 1:end]:
            if block_start.match(l):
                in_loop = "Loop" in l
                if in_loop:
                    before_first_loop = False
                continue
            if not is_inst(l):
                continue
            if not in_loop:
                outside.append(l.strip())
                if before_first_loop:
                    head.append(l.strip())
        def line(body):
            cnt = lambda p: sum(1 for s in body if re.match(p, s))
            return "%d (valu %d: v_cmp %d v_cndmask %d v_mov %d; salu %d: saveexec %d; smem %d branch %d waitcnt %d)" % (
                len(body), cnt(r"v_"), cnt(r"v_cmp"), cnt(r"v_cndmask"), cnt(r"v_mov"), cnt(r"s_(?!cbranch|branch|waitcnt|nop|load|endpgm)"),
                cnt(r"s_\w+_saveexec"), cnt(r"s_load"), cnt(r"s_c?branch"), cnt(r"s_waitcnt"))
        print("%s\n  outside the loops    %s\n  entry to first loop  %s\n  entry to the prologue's first s_load_dwordx16  %s" % (want, line(outside), line(head), line(to_record)))


if __name__ == "__main__":
    main()
