#!/usr/bin/env bash
# TEST INFRASTRUCTURE: build the reference's OWN DLv3 quantizer (dlquant/quantizer.c, quantizer.h) into
# oracle/_ref/libdlquant_ref.so, the ground truth that pins oracle/palette.c and palette.hip.
#
# The two files are copied at build time from the reference tree into oracle/_ref/ (git-ignored) with three
# mechanical changes and nothing else -- no arithmetic is touched:
#   1. quantizer.h's `ulong` / `slong` become 32-bit (unsigned int / signed int): the reference DLL is built by
#      MSVC (dlquant_dll.vcxproj), where long is 32 bits, so CUBE3's sums and counts wrap modulo 2^32;
#   2. the MSVC-only `__declspec(dllexport)` and `__stdcall` are removed;
#   3. the stray prototype `static ulong calc_err(...)` is deleted (it conflicts with the float definition).
# The three progress_* callbacks it calls and the flat entry point ref_dl3quant are ours (ref_dlquant_wrap.c).
# Strict float: no contraction, no fast-math (x86-64: SSE single precision).  Nothing of the reference is copied
# into the repository, and no reference build system is run.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
SRC="${TILER_REFERENCE:-/root/reference}/dlquant"
OUT="$HERE/_ref"
if [ ! -f "$SRC/quantizer.c" ] || [ ! -f "$SRC/quantizer.h" ]; then
  echo "build_ref_dlquant: $SRC/quantizer.c not present: skipping reference DLv3 build" >&2
  exit 0
fi
mkdir -p "$OUT/dlquant"

sed -E \
  -e 's/^(#define[[:space:]]+slong[[:space:]]+)signed long[[:space:]]*$/\1signed int/' \
  -e 's/^(#define[[:space:]]+ulong[[:space:]]+)unsigned long[[:space:]]*$/\1unsigned int/' \
  -e 's/__declspec\(dllexport\)[[:space:]]*//g; s/__stdcall[[:space:]]*//g' \
  "$SRC/quantizer.h" > "$OUT/dlquant/quantizer.h"
sed -E -e '/^static[[:space:]]+ulong[[:space:]]+calc_err\(/d' "$SRC/quantizer.c" > "$OUT/dlquant/quantizer.c"

# every change took: a silent no-op (a reference that words these lines differently) must not pass for a pin
fail() { echo "build_ref_dlquant: $1" >&2; exit 1; }
grep -q '^#define[[:space:]]*ulong[[:space:]]*unsigned int$' "$OUT/dlquant/quantizer.h" || fail "ulong not made 32-bit"
grep -q '^#define[[:space:]]*slong[[:space:]]*signed int$' "$OUT/dlquant/quantizer.h" || fail "slong not made 32-bit"
if grep -q -e '__declspec' -e '__stdcall' "$OUT/dlquant/quantizer.h"; then fail "MSVC keywords left"; fi
[ "$(($(wc -l < "$SRC/quantizer.c") - $(wc -l < "$OUT/dlquant/quantizer.c")))" -eq 1 ] ||
  fail "expected exactly one calc_err prototype line to delete"

FLAGS="-O2 -fPIC -std=gnu11 -ffp-contract=off -fno-fast-math"
# -w: the reference's own warnings (the progress_* calls have no declaration) are not ours to fix
gcc $FLAGS -w -Wno-error=implicit-function-declaration -c -o "$OUT/dlquant/quantizer.o" "$OUT/dlquant/quantizer.c"
gcc $FLAGS -Wall -shared -o "$OUT/libdlquant_ref.so" "$HERE/ref_dlquant_wrap.c" "$OUT/dlquant/quantizer.o" -lm
echo "built $OUT/libdlquant_ref.so"
