#!/bin/bash
# Hashes of the device code in a build of libbgs_hip.so: for every gfx950 code object of the library (one per translation unit),
# sha256 of .text, of .rodata and of the kernel metadata (.note).  Equal lines for two builds mean equal device code; a host-only
# change must leave them equal.
#   tools/device_code_hash.sh [tracking_amd/lib/libbgs_hip.so]
set -euo pipefail
lib=$(readlink -f "${1:-$(dirname "$0")/../tracking_amd/lib/libbgs_hip.so}")
llvm=${ROCM_PATH:-/opt/rocm}/llvm/bin
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
cd "$tmp"
"$llvm/llvm-objcopy" -O binary --only-section=.hip_fatbin "$lib" fat.bin
# the section holds one bundle per translation unit, each starting with the bundler's magic string
python3 - <<'EOF'
data = open("fat.bin", "rb").read()
magic = b"__CLANG_OFFLOAD_BUNDLE__"
starts, pos = [], data.find(magic)
while pos >= 0:
    starts.append(pos)
    pos = data.find(magic, pos + 1)
for k, s in enumerate(starts):
    open("bundle%d" % k, "wb").write(data[s:starts[k + 1] if k + 1 < len(starts) else len(data)])
EOF
for b in bundle*; do
  target=$("$llvm/clang-offload-bundler" --list --type=o --input="$b" | grep gfx950)
  "$llvm/clang-offload-bundler" --unbundle --type=o --input="$b" --targets="$target" --output="$b.co"
  for sec in .text .rodata .note; do
    "$llvm/llvm-objcopy" -O binary --only-section=$sec "$b.co" "$b$sec"
    echo "$b $sec $(stat -c %s "$b$sec") bytes sha256 $(sha256sum "$b$sec" | cut -d' ' -f1)"
  done
done
