#!/usr/bin/env python3
"""loop_instruction_count.py <kr_trace_kernels.hip.s> [kernel substring] [loop index]

Static size of the general unified-step loops of one trace kernel in the device assembly `make -C ntrace_amd/csrc resources` writes
(default kernel: trace_bvh_perray<1, false, true, true>, the AO launch).  For every depth-1 inner loop of the kernel -- the first is the
while-while loop of the prologue-less path, then the GENERIC instance and the FAST / octant instances of traverse_unified -- it prints
the instructions in the loop's extent and the count without the blocks (label to label) that hold the descriptor fallback, the scratch
levels of the stack or the overflow report: one iteration in which the inner and the triangle path both run.  No GPU needed."""
import re
import sys


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "trace_bvh_perrayILi1ELb0ELb1ELb1EE"
    only = int(sys.argv[3]) if len(sys.argv) > 3 else None
    text = open(path).read().split("\n")
    start = next(i for i, l in enumerate(text) if re.match(r"^_ZN3ntr\w+:", l) and want in l)
    end = next(i for i in range(start, len(text)) if "s_endpgm" in text[i])
    lines = text[start:end + 1]
    is_inst = lambda l: l.startswith("\t") and not l.strip().startswith((";", ".")) and l.strip() != ""
    label = re.compile(r"\.LBB\d+_\d+:")
    heads = [(i, label.match(l).group(0)[1:-1]) for i, l in enumerate(lines) if "This Inner Loop Header: Depth=1" in l]
    for n, (hi, name) in enumerate(heads):
        if only is not None and n != only:
            continue
        tag = "Header=" + name[1:] + " "
        idx = [i for i, l in enumerate(lines) if tag in l] + [hi]
        lo, j = min(idx), max(idx) + 1
        while j < len(lines) and not label.match(lines[j]):
            j += 1
        blocks, cur = [], []
        for l in lines[lo:j]:
            if label.match(l) or l.startswith("; %bb."):
                if cur:
                    blocks.append(cur)
                cur = []
            cur.append(l)
        blocks.append(cur)
        body = [l for b in blocks for l in b if is_inst(l)]
        cold = sum(sum(is_inst(l) for l in b) for b in blocks if re.search(r"buffer_load|scratch_|global_atomic|v_mbcnt", "\n".join(b)))
        cnt = lambda p: sum(1 for l in body if re.match(p, l.strip()))
        print("loop %d (%s): extent %d, without fallback / scratch / overflow blocks %d; valu %d (v_mov %d) salu %d branch %d waitcnt %d lds %d" % (
            n, name, len(body), len(body) - cold, cnt(r"v_"), cnt(r"v_mov"), cnt(r"s_(?!cbranch|branch|waitcnt|nop)"), cnt(r"s_c?branch"), cnt(r"s_waitcnt"), cnt(r"ds_")))


if __name__ == "__main__":
    main()
