#!/bin/bash
# Which kernels does a change leave byte-for-byte alone?  Needs no GPU.
#   scripts/kernel_code_identity.sh <tree A> <tree B>  > profiles/rNN_kernel_code_identity.txt
# For every mopo_amd/csrc/*.hip of each tree: compile the gfx950 device code alone (with the extra flags that
# tree's Makefile gives the unit), disassemble it, split the listing at the "<symbol>:" headers, drop the "//"
# address comments and hash each function's instruction text.  Prints "sha256  demangled name" per function,
# the two sorted lists' diff, and a count; exit status 1 if the lists differ.  It compares text and nothing else.
set -euo pipefail
export LC_ALL=C
[ $# -eq 2 ] || { echo "usage: $0 <tree A> <tree B>" >&2; exit 2; }
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OBJDUMP=${OBJDUMP:-/opt/rocm/lib/llvm/bin/llvm-objdump}
JOBS=${JOBS:-16}
W=$(mktemp -d)
trap 'rm -rf "$W"' EXIT

# unit_flags <csrc dir> <unit.hip>: what the Makefile adds to CXXFLAGS for that unit's object
unit_flags() {
  sed -n 's/^\(\$(BUILD)\/[^:]*\):[[:space:]]*CXXFLAGS[[:space:]]*+=[[:space:]]*\(.*\)$/\1|\2/p' "$1/Makefile" |
    while IFS='|' read -r targets flags; do
      case " $targets " in *"/${2%.hip}.o "*) printf '%s ' "$flags";; esac
    done
}

# hashes <tree> <out>: sorted "sha256  name" of every function in the tree's device code
hashes() {
  local src="$1/mopo_amd/csrc" out="$2" d="$W/$(basename "$2").d" f
  mkdir -p "$d"
  for f in "$src"/*.hip; do
    f=$(basename "$f")
    echo "cd '$src' && $HIPCC -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only --no-gpu-bundle-output $(unit_flags "$src" "$f") -c '$f' -o '$d/$f.o' && $OBJDUMP -d --no-show-raw-insn --no-leading-addr '$d/$f.o' > '$d/$f.dis'"
  done | xargs -P "$JOBS" -d '\n' -n 1 bash -c
  cat "$d"/*.dis | python3 -c '
import hashlib, re, sys
name, body, rows = None, [], []
def flush():
    if name is not None:
        rows.append((hashlib.sha256("\n".join(body).encode()).hexdigest(), name))
for line in sys.stdin:
    line = line.split("//")[0].rstrip()
    m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
    if m:
        flush()
        name, body = m.group(1), []
    elif "file format" in line or line.startswith("Disassembly of section"):   # the listing of the next unit begins
        flush()
        name = None
    elif name is not None and line.strip() and line.strip() != "...":   # "...": zero fill up to the next symbol
        body.append(line.strip())
flush()
for h, n in rows:
    print(h + "  " + n)
' | c++filt | sort -k2 > "$out"
}

hashes "$1" "$W/a.txt"
hashes "$2" "$W/b.txt"
echo "# A: $(wc -l < "$W/a.txt") functions, B: $(wc -l < "$W/b.txt") functions"
echo "# ---- A: sha256 of the instruction text, demangled name"
cat "$W/a.txt"
echo "# ---- diff A B (empty: every function's code is identical)"
if diff "$W/a.txt" "$W/b.txt" > "$W/diff.txt"; then
  echo "# identical: $(wc -l < "$W/a.txt") of $(wc -l < "$W/a.txt") functions"
else
  cat "$W/diff.txt"
  echo "# DIFFERENT: $(grep -c '^<' "$W/diff.txt") of A's and $(grep -c '^>' "$W/diff.txt") of B's lines above have no equal in the other list"
  exit 1
fi
