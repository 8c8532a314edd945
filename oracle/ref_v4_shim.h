/* oracle/ref_v4_shim.h -- TEST INFRASTRUCTURE ONLY (our code, no reference text).
 *
 * Lets GCC compile the reference's v4 renderer (demofox_path_tracing_optimization_v4.cpp :1-1556,
 * with mathlib.h, mathutils.h and texture.cpp where they lie) for oracle/ref_v4.cpp.  It must be
 * included before any reference header.  Everything it does, completely:
 *
 * 1. Types.  mathlib.h overloads operators on __m256 / __m256i, which GCC rejects for its built-in
 *    vector types.  After <immintrin.h>, `__m256` / `__m256i` are #defined to two wrapper structs
 *    with implicit conversions to and from the native types, so the reference's overloads bind to
 *    class types and every intrinsic still receives the native vector.  Like MSVC's unions the
 *    wrappers expose the lanes as m256_f32[8] / m256i_i32[8] (texture.cpp :107-134), and a
 *    converting constructor from int reproduces MSVC's aggregate initialisation `{ 0 }` of a
 *    vector member (lane 0 = the value, the other lanes zero; v4 :1415, :1429, :1446, :1460).
 *
 * 2. Instructions without a portable bit pattern (as in oracle/pt_oracle_v4.c):
 *      _mm256_rcp_ps(x)   -> 1.f / x          (correctly rounded division)
 *      _mm256_rsqrt_ps(x) -> 1.f / sqrtf(x)   (correctly rounded sqrt, then division)
 *
 * 3. SVML (MSVC only) -> lane by lane over glibc's float functions, the ones the oracle uses:
 *      _mm256_sin_ps sinf      _mm256_cos_ps cosf      _mm256_tan_ps tanf
 *      _mm256_asin_ps asinf    _mm256_acos_ps acosf    _mm256_atan_ps atanf
 *      _mm256_atan2_ps atan2f  _mm256_exp_ps expf      _mm256_log_ps logf
 *      _mm256_pow_ps powf      _mm256_sincos_ps sinf (returned) + cosf (stored)
 *      _mm256_div_epi32        C's truncating i32 division per lane
 *
 * 4. <cmath>: MSVC declares the float overloads of the math functions in the global namespace, so
 *    the reference's unqualified calls on f32 (tan at v4 :1500, atan2 / asin in texture.cpp) are the
 *    float functions; libstdc++ has only the double ones there.  `using std::...` restores that
 *    (the same step oracle/build_ref.sh documents for the scalar file).
 *
 * 5. Win32: the compiler flags -D'__declspec(x)=__attribute__((x))' -D'align(n)=aligned(n)' (for
 *    CACHE_ALIGN) and -fno-operator-names (mathlib.h :798-820 names functions `xor`, `or`, `and`),
 *    plus the stub headers intrin.h (empty) and windows.h (HANDLE, DWORD, LPVOID, WINAPI) that
 *    oracle/build_ref.sh writes into its temporary directory.
 *
 * No other arithmetic is added or changed.
 */
#pragma once
#include <immintrin.h>
#include <cmath>
#include <cstdint>

using std::sqrt; using std::abs; using std::cos; using std::sin; using std::tan;
using std::atan2; using std::asin; using std::acos; using std::atan; using std::exp; using std::log;
using std::pow; using std::floor; using std::ceil;

typedef __m256 ref_native_m256;
typedef __m256i ref_native_m256i;

struct ref_m256 {
    union {
        ref_native_m256 v;
        float m256_f32[8];
    };
    ref_m256() = default;
    ref_m256(ref_native_m256 x) : v(x) {}
    ref_m256(int x) : v(_mm256_set_ps(0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, (float)x)) {}
    operator ref_native_m256() const { return v; }
};

struct ref_m256i {
    union {
        ref_native_m256i v;
        int32_t m256i_i32[8];
    };
    ref_m256i() = default;
    ref_m256i(ref_native_m256i x) : v(x) {}
    ref_m256i(int x) : v(_mm256_set_epi32(0, 0, 0, 0, 0, 0, 0, x)) {}
    operator ref_native_m256i() const { return v; }
};

#define __m256 ref_m256
#define __m256i ref_m256i

/* ---- 2. rcp / rsqrt -------------------------------------------------------------------------- */
static inline __m256 ref_rcp_ps(__m256 x) { return _mm256_div_ps(_mm256_set1_ps(1.f), x); }
static inline __m256 ref_rsqrt_ps(__m256 x) { return _mm256_div_ps(_mm256_set1_ps(1.f), _mm256_sqrt_ps(x)); }
#define _mm256_rcp_ps ref_rcp_ps
#define _mm256_rsqrt_ps ref_rsqrt_ps

/* ---- 3. SVML ---------------------------------------------------------------------------------- */
#define REF_LANES1(NAME, FN)                                              \
    static inline __m256 NAME(__m256 a)                                   \
    {                                                                     \
        __m256 r;                                                         \
        for (int i = 0; i < 8; ++i) r.m256_f32[i] = FN(a.m256_f32[i]);    \
        return r;                                                         \
    }
#define REF_LANES2(NAME, FN)                                                              \
    static inline __m256 NAME(__m256 a, __m256 b)                                         \
    {                                                                                     \
        __m256 r;                                                                         \
        for (int i = 0; i < 8; ++i) r.m256_f32[i] = FN(a.m256_f32[i], b.m256_f32[i]);     \
        return r;                                                                         \
    }
REF_LANES1(_mm256_sin_ps, sinf)
REF_LANES1(_mm256_cos_ps, cosf)
REF_LANES1(_mm256_tan_ps, tanf)
REF_LANES1(_mm256_asin_ps, asinf)
REF_LANES1(_mm256_acos_ps, acosf)
REF_LANES1(_mm256_atan_ps, atanf)
REF_LANES1(_mm256_exp_ps, expf)
REF_LANES1(_mm256_log_ps, logf)
REF_LANES2(_mm256_atan2_ps, atan2f)
REF_LANES2(_mm256_pow_ps, powf)
static inline __m256 _mm256_sincos_ps(__m256* p_cos, __m256 a)
{
    __m256 s;
    for (int i = 0; i < 8; ++i) {
        s.m256_f32[i] = sinf(a.m256_f32[i]);
        p_cos->m256_f32[i] = cosf(a.m256_f32[i]);
    }
    return s;
}
static inline __m256i _mm256_div_epi32(__m256i a, __m256i b)
{
    __m256i r;
    for (int i = 0; i < 8; ++i) r.m256i_i32[i] = a.m256i_i32[i] / b.m256i_i32[i];
    return r;
}
