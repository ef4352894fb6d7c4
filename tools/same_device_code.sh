#!/bin/bash
# tools/same_device_code.sh OTHER_TREE: proves that a source cleanup left the kernels alone (CPU only).
# Compiles the device side of every .hip in the Makefile's SRCS, with each tree's own Makefile flags plus
# --cuda-device-only -c, in this tree and in OTHER_TREE (e.g. a `git worktree` of the parent commit), prints
# both SHA-256 values per translation unit with IDENTICAL or DIFFERENT, and exits non-zero if any differ.
# (-cuid=NAME: hipcc otherwise names a symbol after a hash of the source path and the command line, which differ between two trees)
set -euo pipefail
[ $# -eq 1 ] || { echo "usage: $0 OTHER_TREE" >&2; exit 2; }
sub=generative_recommenders_amd/csrc
this=$(cd "$(dirname "$0")/.." && pwd)
other=$(cd "$1" && pwd)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
var() { make -s --no-print-directory -C "$1/$sub" --eval 'print-%: ; @echo $($*)' "print-$2"; }
srcs=$(var "$this" SRCS)
compile() {  # compile TREE OUTDIR: one device code object per translation unit, 16 at a time
  mkdir -p "$2"
  (cd "$1/$sub" && printf '%s\n' $srcs | xargs -P 16 -I{} \
     sh -c "$(var "$1" HIPCC) $(var "$1" CXXFLAGS) --cuda-device-only -cuid=\$1 -c \$1 -o $2/\$1.co 2>$2/\$1.log || { cat $2/\$1.log >&2; exit 255; }" _ {})
}
compile "$this" "$tmp/this"
compile "$other" "$tmp/other"
rc=0
for s in $srcs; do
  a=$(sha256sum < "$tmp/this/$s.co" | cut -d' ' -f1)
  b=$(sha256sum < "$tmp/other/$s.co" | cut -d' ' -f1)
  if [ "$a" = "$b" ]; then verdict=IDENTICAL; else verdict=DIFFERENT; rc=1; fi
  printf '%-20s %s %s %s\n' "$s" "$a" "$b" "$verdict"
done
exit $rc
