#!/usr/bin/env bash
# oracle/build_ref.sh -- TEST INFRASTRUCTURE ONLY.
#
# Builds the reference's own scalar path tracer (unmodified, compiled where it lies under
# /root/reference) and, at the end of this script, its v4 renderer's lines 1-1556 into oracle/_ref/
# so it can (a) generate the golden fixtures in tests/golden and (b) serve as the "reference" CPU baseline in bench.py.  Nothing from the reference is
# copied into the repository: the one generated header (a selection of mathlib.h's own scalar
# lines, see below) lives in a temporary directory that is deleted on exit, and only the
# compiled binary/.so land in oracle/_ref/ (git-ignored).
#
# Why a generated header: the reference's full mathlib.h only compiles under MSVC (it overloads
# operators on __m256 and calls SVML).  demofox_path_tracing_scalar.cpp only needs mathlib.h's
# scalar f32xN subset, so we extract exactly those line ranges and add
# `using std::{sqrt,abs,cos,sin,tan};`: MSVC's <cmath> declares the float overloads of these in
# the global namespace, so the reference's unqualified calls on f32 (scalar.cpp:46-48,122,126,
# 169,173,338) are sqrtf/fabsf/cosf/sinf/tanf under MSVC.  libstdc++'s <cmath> only has the double
# versions globally: without the using-declarations GCC binds abs(float) to abs(int) (5 pixels
# differ) and cos/sin/tan to double precision (a different rounding of x, y and
# the camera distance).  The float overloads here resolve to glibc's sinf/cosf/tanf.
# `-I-` stops GCC from searching the reference directory first for "mathlib.h".
#
# Flags: -O2 -ffp-contract=off  (MSVC /fp:precise does not contract a*b+c).
set -euo pipefail
REF=${REF:-/root/reference/CPUPerformanceRayTracer}
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/_ref"
if [ ! -f "$REF/demofox_path_tracing_scalar.cpp" ]; then
    echo "build_ref.sh: reference not present at $REF -- skipping (prebuilt files are used)" >&2
    exit 0
fi
mkdir -p "$OUT"
GEN="$(mktemp -d "${TMPDIR:-/tmp}/ptref.XXXXXX")"
trap 'rm -rf "$GEN"' EXIT
M="$REF/mathlib.h"
{
    echo '#pragma once'
    echo '#include "utils.h"'
    echo '#include <cmath>'
    echo 'using std::sqrt; using std::abs; using std::cos; using std::sin; using std::tan;'
    awk 'NR>=12&&NR<=72' "$M"              # f32x2/3/4 structs + add/sub/mul/div/dot/fmadd
    awk 'NR==415||NR==436||NR==437' "$M"   # (comment) + sroot/rsroot(f32)
    awk 'NR>=582&&NR<=619' "$M"            # scalar operator+ - * /
    awk 'NR>=723&&NR<=726' "$M"            # len(f32xN)
    awk 'NR>=729&&NR<=731' "$M"            # (comments)
    awk 'NR>=749&&NR<=751' "$M"            # normalize(f32xN)
    awk 'NR==763||NR==768' "$M"            # lerp, cross(f32x3)
} > "$GEN/mathlib.h"
CXX=${CXX:-g++}
FLAGS="-std=c++17 -O2 -ffp-contract=off -fPIC -w"
INC="-I$GEN -I- -I$GEN -I$REF"
$CXX $FLAGS $INC -c "$REF/demofox_path_tracing_scalar.cpp" -o "$GEN/scalar.o" 2>/dev/null
$CXX $FLAGS -c "$HERE/ref_driver.cpp" -o "$GEN/drv.o"
$CXX $FLAGS -DREF_DRIVER_MAIN -c "$HERE/ref_driver.cpp" -o "$GEN/drv_main.o"
$CXX -shared -o "$OUT/libref_scalar.so" "$GEN/scalar.o" "$GEN/drv.o" -lm
$CXX -o "$OUT/ref_scalar" "$GEN/scalar.o" "$GEN/drv_main.o" -lm

# --- c_numBounces = 8 (BASELINE configs[1]-[4]) ----------------------------------------------------
# The reference's own line 19 reads `const int c_numBounces = 4; //8`: the value it annotates as the
# alternative.  A temporary copy of the file (in $GEN, deleted on exit, never in the repository) with
# ONLY that constant changed is compiled exactly like the unmodified file.  The script checks that
# the copy differs from the original in that one line and records both sha256s and the diff in
# oracle/_ref/b8_patch.json (make_golden.py copies it into tests/golden/manifest.json).
SRC="$REF/demofox_path_tracing_scalar.cpp"
B8="$GEN/b8"
mkdir -p "$B8"
cp "$REF/demofox_path_tracing_scalar.h" "$B8/"
sed '19s/^const int c_numBounces = 4; \/\/8\r\{0,1\}$/const int c_numBounces = 8; \/\/8/' "$SRC" > "$B8/demofox_path_tracing_scalar.cpp"
NDIFF=$(diff "$SRC" "$B8/demofox_path_tracing_scalar.cpp" | grep -c '^[<>]' || true)
if [ "$NDIFF" != "2" ]; then
    echo "build_ref.sh: c_numBounces patch did not change exactly line 19 ($NDIFF diff lines)" >&2
    exit 1
fi
DIFF_TXT=$(diff "$SRC" "$B8/demofox_path_tracing_scalar.cpp" | tr -d '\r' || true)
python3 - "$SRC" "$B8/demofox_path_tracing_scalar.cpp" "$DIFF_TXT" > "$OUT/b8_patch.json" <<'PY'
import hashlib, json, sys
orig, patched, diff = sys.argv[1], sys.argv[2], sys.argv[3]
h = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()
print(json.dumps({"file": "demofox_path_tracing_scalar.cpp", "line": 19,
                  "sha256_original": h(orig), "sha256_patched": h(patched), "diff": diff}, indent=1))
PY
$CXX $FLAGS -I"$GEN" -I- -I"$B8" -I"$GEN" -I"$REF" -c "$B8/demofox_path_tracing_scalar.cpp" -o "$GEN/scalar_b8.o" 2>/dev/null
$CXX -o "$OUT/ref_scalar_b8" "$GEN/scalar_b8.o" "$GEN/drv_main.o" -lm

# --- config 4's miss term: EquirectangularTextureSample's per-lane body --------------------------
# texture.cpp:101-139 is an m256x3 (MSVC __m256) function whose per-lane body, :111-135, is plain
# scalar f32 code on f32x2/f32x3 (+ TexelFetch, :6-14, and struct texture, texture.h:6-12).  Those
# line ranges are extracted into a temporary file and compiled, with the same mathlib.h subset as
# above plus `using std::atan2; using std::asin;` (MSVC's float overloads, as for sqrt/cos above),
# inside ref_env.cpp's per-direction wrapper.  No arithmetic is added.
T="$REF/texture.cpp"
{
    echo '#include "mathlib.h"'
    echo 'using std::atan2; using std::asin;'
    awk 'NR>=6&&NR<=12' "$REF/texture.h"     # struct texture
    awk 'NR>=6&&NR<=14' "$T"                 # TexelFetch
} > "$GEN/ref_texture_fetch.inc"
awk 'NR>=111&&NR<=135' "$T" > "$GEN/ref_env_lane_body.inc"
$CXX $FLAGS -I"$GEN" -I"$HERE" -I"$REF" "$HERE/ref_env.cpp" -o "$OUT/ref_env" -lm
# LoadTexture's decoder (config 4): the reference's vendored stb_image.h, compiled where it lies
$CXX -std=c++17 -O2 -w -I"$REF" "$HERE/ref_hdr.cpp" -o "$OUT/ref_hdr" -lm
# WriteImage's encoder (output stage): the reference's vendored stb_image_write.h, where it lies
$CXX -std=c++17 -O2 -w -I"$REF" "$HERE/ref_bmp.cpp" -o "$OUT/ref_bmp" -lm
echo "build_ref.sh: built $OUT/libref_scalar.so, $OUT/ref_scalar, $OUT/ref_scalar_b8, $OUT/ref_env, $OUT/ref_hdr and $OUT/ref_bmp"

# --- the v4 renderer (demofox_path_tracing_optimization_v4.cpp) ------------------------------------
# The reference's own v4 lines 1-1556 (everything above the Win32 thread pool), compiled where
# mathlib.h, mathutils.h and texture.cpp lie, inside oracle/ref_v4.cpp's driver and behind
# oracle/ref_v4_shim.h (every substitution is listed in that header).  The extracted lines, the two
# Win32 stub headers (our text) and the flag-variant copies of global_preprocessor_flags.h live in
# $GEN only.  `-I-` keeps "global_preprocessor_flags.h" from being found next to the including file,
# so a variant's copy is the one every header sees.
# global_preprocessor_flags.h defines its switches unconditionally, so each variant is a temporary
# copy with ONLY the named lines' values changed; the script checks that exactly those lines differ
# and records the diff and both sha256s in oracle/_ref/v4_flags.json (tests/golden/make_golden_v4.py
# copies it into tests/golden/manifest.json).
V4="$REF/demofox_path_tracing_optimization_v4.cpp"
FLAGS_H="$REF/global_preprocessor_flags.h"
if [ ! -f "$V4" ] || [ ! -f "$FLAGS_H" ]; then
    echo "build_ref.sh: the reference's v4 file is not present -- skipping ref_v4 (committed fixtures are used)" >&2
    exit 0
fi
if ! grep -qw avx2 /proc/cpuinfo 2>/dev/null || ! grep -qw fma /proc/cpuinfo 2>/dev/null; then
    echo "build_ref.sh: this CPU lacks AVX2/FMA -- skipping ref_v4 (committed fixtures are used)" >&2
    exit 0
fi
V4GEN="$GEN/v4"
mkdir -p "$V4GEN/stubs"
awk 'NR<=1556' "$V4" > "$V4GEN/ref_v4_body.inc"
: > "$V4GEN/stubs/intrin.h"
printf '%s\n' '#pragma once' 'typedef void* HANDLE;' 'typedef unsigned long DWORD;' 'typedef void* LPVOID;' \
    '#define WINAPI' > "$V4GEN/stubs/windows.h"
V4FLAGS="-std=c++17 -O2 -mavx2 -mfma -ffp-contract=off -fno-operator-names -w"
# variant name, then line:MACRO:new-value for every changed line (global_preprocessor_flags.h :56-66)
V4_VARIANTS=(
    "shipped"
    "cubemap 57:USE_ENV_CUBEMAP:1"
    "bilinear 66:USE_RANDOM_JITTER_TEXTURE_SAMPLING:0"
    "angle 65:USE_UNIT_VECTOR_REJECTION_SAMPLING:0"
    "noenv 56:USE_ENV_MAP:0"
    "exactexp 64:USE_FAST_APPROXIMATE_EXP:0"
    "exactout 63:USE_FAST_APPROXIMATE_ACES_TONEMAP:0 62:USE_FAST_APPROXIMATE_GAMMA:0"
    "noaccum 60:ACCUMULATE_FRAMES:0"
)
V4_JSON_ARGS=()
V4_BUILT=""
for spec in "${V4_VARIANTS[@]}"; do
    set -- $spec
    name=$1; shift
    D="$V4GEN/$name"
    mkdir -p "$D"
    cp "$FLAGS_H" "$D/global_preprocessor_flags.h"
    nedits=0
    for e in "$@"; do
        IFS=: read -r ln macro val <<< "$e"
        sed -i "${ln}s/^#define ${macro} [01]\(\r\{0,1\}\)\$/#define ${macro} ${val}\1/" "$D/global_preprocessor_flags.h"
        nedits=$((nedits + 1))
    done
    NDIFF=$(diff "$FLAGS_H" "$D/global_preprocessor_flags.h" | grep -c '^[<>]' || true)
    if [ "$NDIFF" != "$((2 * nedits))" ]; then
        echo "build_ref.sh: v4 variant $name did not change exactly its $nedits flag line(s) ($NDIFF diff lines)" >&2
        exit 1
    fi
    diff "$FLAGS_H" "$D/global_preprocessor_flags.h" | tr -d '\r' > "$D/flags.diff" || true
    $CXX $V4FLAGS -D'__declspec(x)=__attribute__((x))' -D'align(n)=aligned(n)' \
        -DREF_V4_BODY="\"$V4GEN/ref_v4_body.inc\"" \
        -I"$D" -I"$V4GEN/stubs" -I"$HERE" -I- -I"$D" -I"$V4GEN/stubs" -I"$HERE" -I"$REF" \
        "$HERE/ref_v4.cpp" -o "$OUT/ref_v4_$name" -lm 2> "$D/cc.log" || { cat "$D/cc.log" >&2; exit 1; }
    V4_JSON_ARGS+=("$name" "$D/global_preprocessor_flags.h" "$D/flags.diff" "$*")
    V4_BUILT="$V4_BUILT ref_v4_$name"
done
python3 - "$V4" "$FLAGS_H" "${V4_JSON_ARGS[@]}" > "$OUT/v4_flags.json" <<'PY'
import hashlib, json, sys
h = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()
v4, flags, rest = sys.argv[1], sys.argv[2], sys.argv[3:]
out = {"file": "global_preprocessor_flags.h", "sha256_original": h(flags),
       "v4_file": "demofox_path_tracing_optimization_v4.cpp", "v4_lines": "1-1556", "v4_sha256": h(v4), "variants": {}}
for name, patched, diff, edits in zip(rest[0::4], rest[1::4], rest[2::4], rest[3::4]):
    out["variants"][name] = {
        "lines": {e.split(":")[0]: "#define %s %s" % tuple(e.split(":")[1:]) for e in edits.split()},
        "sha256_patched": h(patched), "diff": open(diff).read()}
print(json.dumps(out, indent=1))
PY
echo "build_ref.sh: built$V4_BUILT in $OUT"
