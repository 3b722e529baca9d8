#!/bin/bash
# same_codeobj.sh <csrc A> <csrc B> [-D...]: is the device code of hk_kernels.hip the same in two trees?  Compiles both csrc
# directories to gfx950 assembly, each with the CXXFLAGS of its own Makefile (side by side, ~5 minutes), drops the lines that hold the
# per-compile __hip_cuid_ symbol, and prints `identical` or the names of the functions whose bodies differ (exit status 1).
set -eu
A=$(cd "$1" && pwd) B=$(cd "$2" && pwd); shift 2
out=$(mktemp -d); trap 'rm -rf "$out"' EXIT
for t in A B; do
    (cd "${!t}" && /opt/rocm/bin/hipcc --offload-arch=gfx950 $(sed -n 's/^CXXFLAGS := //p' Makefile) "$@" \
        --cuda-device-only -S hk_kernels.hip -o "$out/$t.full" 2> "$out/$t.log" && grep -v __hip_cuid_ "$out/$t.full" > "$out/$t.s") &
done
wait
for t in A B; do [ -s "$out/$t.s" ] || { echo "compile of ${!t} failed:" >&2; cat "$out/$t.log" >&2; exit 2; }; done
cmp -s "$out/A.s" "$out/B.s" && { echo identical; exit 0; }
# the lines of A that the diff touches, each under the last function label (`name:`) above it
diff "$out/A.s" "$out/B.s" | sed -n 's/^\([0-9]*\).*/\1/p' > "$out/lines" || true
awk 'NR == FNR { want[$1]; next } /^[A-Za-z_][^ ]*:/ { fn = substr($1, 1, length($1) - 1) } (FNR in want) { print fn }' "$out/lines" "$out/A.s" | uniq | c++filt | cut -c1-200
exit 1
