#!/bin/bash
# kernel_isa_diff.sh <other-tree> [file.hip ...]: is every kernel's gfx950 code in this tree the same as in <other-tree> (a checkout of
# the commit a refactor started from: `git worktree add <dir> <commit>`, outside the repository)?  Compiles the translation units
# (default: trace_kernels.hip) in both trees with the Makefile's own flags (target `resources`; no GPU needed) and compares, per kernel,
# the text from its label to its .Lfunc_end and its .amdhsa_kernel block.  What is not code is normalised away: comments, the numbers of
# the basic-block labels (.LBB<n>_<m>) and of the inline-asm labels (.Lcs_*<n>) -- renumbered by first appearance inside the kernel, so
# a branch that moved to another block still shows -- and the __hip_cuid_* symbol.  Exit status 1 when any kernel differs.
OTHER=$(cd "${1:?usage: kernel_isa_diff.sh <other-tree> [file.hip ...]}" && pwd) || exit 2
shift
HERE=$(cd "$(dirname "$0")/.." && pwd)
FILES=${@:-trace_kernels.hip}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
mkdir "$TMP/other" "$TMP/here"
make -s -C "$OTHER/ntrace_amd/csrc" resources RES_DIR="$TMP/other" RES_FILES="$FILES" || exit 2
make -s -C "$HERE/ntrace_amd/csrc" resources RES_DIR="$TMP/here" RES_FILES="$FILES" || exit 2

# kernel_text <file.s> <begin regex> <end regex>: the lines from the first to the second, normalised
kernel_text() {
  awk -v beg="$2" -v end="$3" '
    $0 ~ beg { on = 1 }
    on {
      line = $0
      sub(/[ \t]*;.*$/, "", line); sub(/[ \t]*\/\/.*$/, "", line)
      gsub(/__hip_cuid_[0-9a-f]+/, "__hip_cuid", line)
      out = ""
      while (match(line, /\.LBB[0-9]+_[0-9]+|\.Lcs_[a-z]+[0-9]+|\.Lfunc_end[0-9]+/)) {
        lab = substr(line, RSTART, RLENGTH)
        if (!(lab in id)) id[lab] = ++n
        out = out substr(line, 1, RSTART - 1) ".L" id[lab]; line = substr(line, RSTART + RLENGTH)
      }
      line = out line
      if (line !~ /^[ \t]*$/) print line
    }
    on && $0 ~ end { exit }' "$1"
}

RC=0
for F in $FILES; do
  echo "== $F"
  A="$TMP/other/kr_$F.s"; B="$TMP/here/kr_$F.s"
  for K in $( (sed -n 's/^[ \t]*\.amdhsa_kernel \([^ \t]*\).*/\1/p' "$A" "$B") | sort -u); do
    for T in other here; do
      { kernel_text "$TMP/$T/kr_$F.s" "^$K:" "^\\.Lfunc_end[0-9]+:"
        kernel_text "$TMP/$T/kr_$F.s" "^[ \t]*\\.amdhsa_kernel $K\$" "^[ \t]*\\.end_amdhsa_kernel"; } > "$TMP/$T.txt"
    done
    N=$(diff "$TMP/other.txt" "$TMP/here.txt" | grep -c '^[<>]')
    NAME=$(echo "$K" | c++filt | sed 's/(ntr::TraceParams)//;s/ntr:://')
    if [ "$N" -eq 0 ] && [ -s "$TMP/here.txt" ]; then printf "%-62s identical\n" "$NAME"
    else printf "%-62s differs (%d lines)\n" "$NAME" "$N"; RC=1; fi
  done
done
exit $RC
