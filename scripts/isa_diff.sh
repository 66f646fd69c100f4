#!/bin/bash
# Do two trees emit the same device code?  scripts/isa_diff.sh <csrc A> <csrc B> compares the build/isa/*.s files that `make isa` wrote
# in the two csrc directories, without the lines that name the __hip_cuid_<hex> symbol (a hash of the source text).  One line per
# file: `same`, the number of differing lines, or `missing`; exit status 1 on any difference or missing file.
if [ $# -ne 2 ]; then echo "usage: $0 <csrc A> <csrc B>" >&2; exit 2; fi
A=$1/build/isa B=$2/build/isa
names=$( (cd "$A" 2>/dev/null && ls *.s; cd "$B" 2>/dev/null && ls *.s) 2>/dev/null | sort -u)
if [ -z "$names" ]; then echo "no build/isa/*.s in $1 or $2: run make isa in both" >&2; exit 1; fi
rc=0
for f in $names; do
  if [ ! -f "$A/$f" ] || [ ! -f "$B/$f" ]; then echo "$f: missing"; rc=1; continue; fi
  n=$(diff <(grep -v __hip_cuid_ "$A/$f") <(grep -v __hip_cuid_ "$B/$f") | grep -c '^[<>]')
  if [ "$n" -eq 0 ]; then echo "$f: same"; else echo "$f: $n lines differ"; rc=1; fi
done
exit $rc
