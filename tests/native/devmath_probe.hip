// tests/native/devmath_probe.hip -- the DEVICE builds of the exact-math headers, run on the GPU and
// compared bit for bit with their HOST builds (and, for division / reciprocal / square root, with x86
// hardware '/' and sqrtf).  The host builds are what the CPU tests prove equal to glibc 2.35
// (test_sincosf / test_libmf / test_invtrig / test_envcert); this probe carries that proof over to the
// code the kernels really run: the __HIP_DEVICE_COMPILE__ branch of sincosf_glibc, the constexpr tables
// of pt_libmf.h indexed at run time, pt_invtrig.h / pt_envcert.h with the kernels' macro substitutions,
// and the guarded forms of pt_exactmath.h on and around every guard bound.
//
//   devmath_probe SECTION [host]     SECTION: sincos exp pow invtrig guarded envcert (or all)
//
// Each set prints "name checked=<n> mismatches=<m>" and up to four "in / in2 / got / want" examples;
// exit status 1 on any mismatch.  "host" as a second argument runs the host side alone (no GPU is
// touched, nothing is compared): it times the reference and lets the generators be inspected.
//
// How results move: one set is a functor f(i) -> (counted, out, aux) that both passes of this file
// compile -- the device pass with the product's substitutions, the host pass with the headers'
// defaults.  The GPU reduces every 4096 consecutive items to one 64-bit checksum and a count, the host
// (at most 16 threads) computes the same checksums, and a block whose checksum differs is computed
// again on the GPU with every output written out, so the offending input is named.  At most kMaxDrill
// blocks are drilled into; further differing blocks count one mismatch each (a lower bound, noted
// beside the line).  The envcert sets are small and always move every output.  NaN matches any NaN.
//
// The reference side uses only exactly specified operations: x86 '/' and sqrt instructions, and
// fma / fmaf / floorf, which are correctly rounded / exact in any libm.  It never calls a libm
// function whose result depends on the libm's version; where an input generator does (cosf, log2),
// it runs once on the host and both sides read the generated floats.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 + the product's parity flags
// (cpuperformanceraytracer_amd/build.py PARITY_FLAGS).  Not part of libpt_mi355.so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <atomic>
#include <chrono>
#include <functional>
#include <thread>
#include <vector>

#include "../../cpuperformanceraytracer_amd/csrc/pt_exactmath.h"
#include "../../cpuperformanceraytracer_amd/csrc/pt_sincosf.h"
#include "../../cpuperformanceraytracer_amd/csrc/pt_libmf.h"
#if defined(__HIP_DEVICE_COMPILE__)
// The device pass: pt_v4.hip's substitutions (its lines 25-35; pt_kernel.hip's are the same).  These
// lines MUST stay equal to the product's -- they are what this probe exists to check.
// atan2f/asinf with the guarded fast '/' and sqrt (bit-identical to IEEE, pt_exactmath.h)
#define PT_IT_HD __device__ __forceinline__
#define PT_IT_DIV(a, b) pt::div_guarded((a), (b))
#define PT_IT_SQRT(x) pt::sqrt_guarded(x)
#include "../../cpuperformanceraytracer_amd/csrc/pt_invtrig.h"
// certified texel cells (the exact atan2f/asinf above only where a cell is not certified)
#define PT_EC_HD __device__ __forceinline__
#define PT_EC_RCP(x) pt::rcp_rn(x)                       // q in (1, 2^40)
#define PT_EC_DIV(a, b) pt::div_rn((a), (b), pt::rcp_rn(b))   // |x|, |y| in [2^-20, 2^20)
#define PT_EC_SQRT(x) pt::sqrt_rn(x)                     // t >= 2^-21 where the value is used
#include "../../cpuperformanceraytracer_amd/csrc/pt_envcert.h"
#else
// The host pass: the headers' defaults ('/', __builtin_sqrtf), as the CPU tests compile them.
#include "../../cpuperformanceraytracer_amd/csrc/pt_invtrig.h"
#include "../../cpuperformanceraytracer_amd/csrc/pt_envcert.h"
#endif

#define HD __host__ __device__ __forceinline__

namespace {

constexpr uint32_t kBlk = 4096;       // items per checksum
constexpr uint32_t kThreads = 256;    // GPU threads per checksum block
constexpr uint32_t kMaxDrill = 1024;  // differing blocks recomputed item by item (also the batch size)
bool g_host_only = false;

struct Sum {
    unsigned long long h, n;
};
struct Out {
    unsigned long long out;
    unsigned int aux, ok;
};
struct P2 {
    float a, b;
};
struct Dir {
    float x, y, z, r1, r2;
};

HD uint32_t fb(float f) { return __builtin_bit_cast(uint32_t, f); }
HD float bf(uint32_t u) { return __builtin_bit_cast(float, u); }
HD uint32_t canon(float f)   // NaN matches any NaN
{
    const uint32_t u = fb(f);
    return (u & 0x7fffffffu) > 0x7f800000u ? 0x7fc00000u : u;
}
HD uint64_t item_hash(uint64_t i, uint64_t out, uint32_t aux)   // a bijection of out for fixed (i, aux)
{
    uint64_t z = out + 0x9e3779b97f4a7c15ull * (i + 1) + ((uint64_t)aux << 17);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    return z ^ (z >> 27);
}
HD uint32_t mix(uint64_t z)   // exactmath_probe.hip's
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)(z ^ (z >> 31));
}

// ---- the operations under test: the device form on the device, x86 hardware on the host ----
HD float dv_div(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return pt::div_guarded(a, b);
#else
    return a / b;
#endif
}
HD float dv_sqrt(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return pt::sqrt_guarded(x);
#else
    return __builtin_sqrtf(x);
#endif
}
HD float dv_sqrt_finite(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return pt::sqrt_finite_guarded(x);
#else
    return __builtin_sqrtf(x);
#endif
}
HD float dv_rcp(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return pt::rcp_guarded(x);
#else
    return 1.0f / x;
#endif
}
HD float dv_rcp_nonneg(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return pt::rcp_nonneg_guarded(x);
#else
    return 1.0f / x;
#endif
}

// a list both sides read: uploaded once, d on the device, h on the host
template <class T> struct List {
    const T* d;
    const T* h;
    HD const T& operator[](uint64_t i) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        return d[i];
#else
        return h[i];
#endif
    }
};

// ---- GPU side ----
template <class F> __global__ __launch_bounds__(kThreads) void k_sum(F f, uint64_t n, Sum* sums)
{
    __shared__ unsigned long long sh[2];
    if (threadIdx.x == 0) sh[0] = sh[1] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kBlk;
    unsigned long long h = 0, c = 0;
    for (uint32_t k = threadIdx.x; k < kBlk; k += kThreads) {
        const uint64_t i = base + k;
        if (i >= n) break;
        uint64_t out = 0;
        uint32_t aux = 0;
        if (f(i, out, aux)) {
            h += item_hash(i, out, aux);
            ++c;
        }
    }
    atomicAdd(&sh[0], h);
    atomicAdd(&sh[1], c);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = Sum{sh[0], sh[1]};   // one entry per block of the grid
}

template <class F> __global__ __launch_bounds__(kThreads) void k_dump(F f, uint64_t n, const uint32_t* blks, Out* o)
{
    const uint64_t base = (uint64_t)blks[blockIdx.x] * kBlk;   // blks has gridDim.x entries
    for (uint32_t k = threadIdx.x; k < kBlk; k += kThreads) {
        const uint64_t i = base + k;
        Out r{0, 0, 0};
        if (i < n) {
            uint64_t out = 0;
            uint32_t aux = 0;
            r.ok = f(i, out, aux) ? 1u : 0u;
            r.out = out;
            r.aux = aux;
        }
        o[(uint64_t)blockIdx.x * kBlk + k] = r;   // o has gridDim.x * kBlk entries
    }
}

#define CK(x)                                                                            \
    do {                                                                                 \
        const hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                          \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(2);                                                                     \
        }                                                                                \
    } while (0)

unsigned host_threads()
{
    unsigned nt = std::thread::hardware_concurrency();
    if (nt == 0) nt = 8;
    return nt > 16 ? 16 : nt;
}

// fn(first, last) over [0, n) in pieces handed to at most 16 threads
void parallel_for(uint64_t n, uint64_t piece, const std::function<void(uint64_t, uint64_t)>& fn)
{
    std::atomic<uint64_t> next{0};
    std::vector<std::thread> th;
    const unsigned nt = host_threads();
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&] {
            for (;;) {
                const uint64_t a = next.fetch_add(piece);
                if (a >= n) return;
                fn(a, a + piece < n ? a + piece : n);
            }
        });
    for (auto& x : th) x.join();
}

template <class T> List<T> upload(const std::vector<T>& v)
{
    List<T> l{nullptr, v.data()};
    if (!g_host_only && !v.empty()) {
        T* d;
        CK(hipMalloc(&d, v.size() * sizeof(T)));
        CK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        l.d = d;
    }
    return l;
}
template <class T> void release(List<T>& l)
{
    if (l.d) CK(hipFree(const_cast<T*>(l.d)));
    l.d = nullptr;
}

struct Examples {
    unsigned n = 0;
    uint32_t in[4], in2[4];
    unsigned long long got[4], want[4];
    unsigned gaux[4], waux[4];
    char note[4][96];
};
// a set whose input is more than two words (envcert: a direction and two random numbers) spells it out
template <class F> auto note_of(const F& f, uint64_t i, char* b, size_t n, int) -> decltype(f.note(i, b, n), void()) { f.note(i, b, n); }
template <class F> void note_of(const F&, uint64_t, char* b, size_t, long) { b[0] = 0; }

// extra(i, device_out) -> false = a violation of a host-only property (envcert: certified == exact)
using Extra = std::function<bool(uint64_t, const Out&)>;

template <class F> int run(const char* name, const F& f, uint64_t n, const Extra* extra = nullptr)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t nblk = (uint32_t)((n + kBlk - 1) / kBlk);
    const bool full = extra != nullptr;
    Sum* d_sums = nullptr;
    if (!g_host_only && !full) {
        CK(hipMalloc(&d_sums, (size_t)nblk * sizeof(Sum)));
        hipLaunchKernelGGL(k_sum<F>, dim3(nblk), dim3(kThreads), 0, 0, f, n, d_sums);
        CK(hipGetLastError());
    }
    // the host's checksums, while the GPU computes its own
    std::vector<Sum> want(nblk);
    if (!full || g_host_only)
        parallel_for(nblk, 16, [&](uint64_t b0, uint64_t b1) {
            for (uint64_t b = b0; b < b1; ++b) {
                unsigned long long h = 0, c = 0;
                const uint64_t last = (b + 1) * kBlk < n ? (b + 1) * kBlk : n;
                for (uint64_t i = b * kBlk; i < last; ++i) {
                    uint64_t out = 0;
                    uint32_t aux = 0;
                    if (f(i, out, aux)) {
                        h += item_hash(i, out, aux);
                        ++c;
                    }
                }
                want[b] = Sum{h, c};
            }
        });
    unsigned long long checked = 0;
    for (const Sum& s : want) checked += s.n;
    if (g_host_only) {
        printf("%s checked=%llu host_only seconds=%.2f\n", name, checked,
               std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        return 0;
    }
    std::vector<uint32_t> bad;
    if (full) {
        for (uint32_t b = 0; b < nblk; ++b) bad.push_back(b);
    } else {
        std::vector<Sum> got(nblk);
        CK(hipMemcpy(got.data(), d_sums, (size_t)nblk * sizeof(Sum), hipMemcpyDeviceToHost));
        CK(hipFree(d_sums));
        for (uint32_t b = 0; b < nblk; ++b)
            if (got[b].h != want[b].h || got[b].n != want[b].n) bad.push_back(b);
    }
    // every output of the differing blocks (of all blocks when an extra property is checked)
    std::atomic<unsigned long long> mism{0}, viol{0}, nchk{0};
    Examples ex;
    std::atomic<unsigned> nex{0};
    const size_t ndrill = full ? bad.size() : (bad.size() < kMaxDrill ? bad.size() : kMaxDrill);
    if (ndrill) {
        uint32_t* d_blks;
        Out* d_out;
        const size_t batch = ndrill < kMaxDrill ? ndrill : kMaxDrill;
        CK(hipMalloc(&d_blks, batch * sizeof(uint32_t)));
        CK(hipMalloc(&d_out, batch * kBlk * sizeof(Out)));
        std::vector<Out> outs(batch * kBlk);
        for (size_t o = 0; o < ndrill; o += batch) {
            const size_t nb = ndrill - o < batch ? ndrill - o : batch;
            CK(hipMemcpy(d_blks, bad.data() + o, nb * sizeof(uint32_t), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_dump<F>, dim3((uint32_t)nb), dim3(kThreads), 0, 0, f, n, d_blks, d_out);
            CK(hipGetLastError());
            CK(hipMemcpy(outs.data(), d_out, nb * kBlk * sizeof(Out), hipMemcpyDeviceToHost));
            parallel_for(nb, 4, [&](uint64_t j0, uint64_t j1) {
                unsigned long long m = 0, v = 0, c = 0;
                for (uint64_t j = j0; j < j1; ++j)
                    for (uint32_t k = 0; k < kBlk; ++k) {
                        const uint64_t i = (uint64_t)bad[o + j] * kBlk + k;
                        if (i >= n) break;
                        const Out& g = outs[j * kBlk + k];
                        uint64_t out = 0;
                        uint32_t aux = 0;
                        const bool ok = f(i, out, aux);
                        c += ok;
                        const bool differ = (ok ? 1u : 0u) != g.ok || (ok && (out != g.out || aux != g.aux));
                        const bool broke = !differ && ok && extra && !(*extra)(i, g);
                        if (differ || broke) {
                            differ ? ++m : ++v;
                            const unsigned e = nex.fetch_add(1);
                            if (e < 4) {
                                f.describe(i, ex.in[e], ex.in2[e]);
                                note_of(f, i, ex.note[e], sizeof(ex.note[e]), 0);
                                ex.got[e] = g.out, ex.gaux[e] = g.aux;
                                ex.want[e] = out, ex.waux[e] = aux;
                            }
                        }
                    }
                mism += m, viol += v, nchk += c;
            });
        }
        CK(hipFree(d_blks));
        CK(hipFree(d_out));
    }
    if (full) checked = nchk.load();
    const unsigned long long undrilled = bad.size() - ndrill;
    const unsigned long long total = mism.load() + viol.load() + undrilled;
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%s checked=%llu mismatches=%llu\n", name, checked, total);
    ex.n = nex.load() < 4 ? nex.load() : 4;
    for (unsigned e = 0; e < ex.n; ++e)
        printf("  in=%08x in2=%08x got=%016llx/%x want=%016llx/%x%s\n", ex.in[e], ex.in2[e], ex.got[e], ex.gaux[e], ex.want[e],
               ex.waux[e], ex.note[e]);
    if (viol.load()) printf("  %llu of them: the device agrees with the host but not with the exact pipeline\n", viol.load());
    if (undrilled)
        printf("  %zu blocks of %u items differ, %zu examined item by item; the other %llu count one mismatch each\n", bad.size(),
               kBlk, ndrill, undrilled);
    printf("  seconds=%.2f\n", secs);
    fflush(stdout);
    return total != 0;
}

// =============================== 1. sincos ===============================
struct FSincos {
    uint32_t u0;
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        float s, c;
        pt::sincosf_glibc(bf(u0 + (uint32_t)i), &s, &c);
        out = (uint64_t)canon(s) << 32 | canon(c);   // sin high, cos low
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = u0 + (uint32_t)i, in2 = 0; }
};

int section_sincos()
{
    int bad = 0;
    const uint32_t hi = fb(6.2831855f * 1.0001f);   // check_sincosf.cpp's default range [0, 2 pi 1.0001]
    bad |= run("sincos.0_2pi", FSincos{0u}, (uint64_t)hi + 1);
    const uint32_t n0 = fb(-1e-45f), n1 = fb(-6.2832f);   // its second range; -0 excluded (pt_sincosf.h)
    bad |= run("sincos.negative", FSincos{n0}, (uint64_t)(n1 - n0) + 1);
    return bad;
}

// =============================== 2. exp ===============================
struct FExp {
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        out = canon(pt::lm::expf_glibc(bf((uint32_t)i)));
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = (uint32_t)i, in2 = 0; }
};

int section_exp() { return run("exp.all", FExp{}, 1ull << 32); }

// =============================== 3. pow ===============================
struct FPowGamma {
    uint32_t lo;
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        out = canon(pt::lm::powf_glibc_main(bf(lo + (uint32_t)i), 1.0f / 2.4f));   // v4 :184
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = lo + (uint32_t)i, in2 = fb(1.0f / 2.4f); }
};
struct FPowPairs {
    List<P2> p;
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        out = canon(pt::lm::powf_glibc_main(p[i].a, p[i].b));
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = fb(p.h[i].a), in2 = fb(p.h[i].b); }
};

int section_pow()
{
    int bad = 0;
    const uint32_t lo = 0x3b000000u /* 2^-9 */, hi = 0x3f800000u /* 1 */;
    bad |= run("pow.gamma", FPowGamma{lo}, (uint64_t)(hi - lo) + 1);
    // check_libmf.cpp pow_random: its generator, its operand filter, and |y log2 x| < 126 (pt_libmf.h's
    // stated domain).  The filter runs here, once; both sides read the pairs it accepted.
    const uint64_t cand = 1ull << 25;
    std::vector<P2> acc(cand);
    std::vector<uint8_t> keep(cand);
    parallel_for(cand, 1 << 16, [&](uint64_t a, uint64_t b) {
        for (uint64_t i = a; i < b; ++i) {
            uint64_t s = i * 0x9E3779B97F4A7C15ull + 12345;
            s ^= s >> 29; s *= 0xBF58476D1CE4E5B9ull; s ^= s >> 32;
            const uint32_t ux = 0x00800000u + (uint32_t)(s % (0x7f800000u - 0x00800000u));   // positive normal
            const uint32_t uy = (uint32_t)(s >> 32);
            const float x = bf(ux), y = bf(uy);
            acc[i] = P2{x, y};
            keep[i] = (fabsf(y) < 1e30f) && y != 0.0f && (fabs((double)y * log2((double)x)) < 126.0);
        }
    });
    std::vector<P2> pairs;
    for (uint64_t i = 0; i < cand; ++i)
        if (keep[i]) pairs.push_back(acc[i]);
    std::vector<P2>().swap(acc);
    FPowPairs f{upload(pairs)};
    bad |= run("pow.random", f, pairs.size());
    release(f.p);
    return bad;
}

// =============================== 4. invtrig ===============================
struct FAsin {   // every f32 with |x| <= 1; then 2^20 patterns above 1 and everything from 2^127 up (NaN results)
    static constexpr uint64_t kIn = 2ull * 0x3f800001ull, kAbove = 1ull << 21, kTop = 1ull << 25;
    HD static uint32_t arg(uint64_t i)
    {
        uint32_t u;
        if (i < kIn) u = (uint32_t)(i >> 1);
        else if (i < kIn + kAbove) u = 0x3f800001u + (uint32_t)((i - kIn) >> 1);
        else u = 0x7f000000u + (uint32_t)((i - kIn - kAbove) >> 1);
        return u | ((uint32_t)(i & 1) << 31);
    }
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        out = canon(pt::asinf_glibc(bf(arg(i))));
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = arg(i), in2 = 0; }
};
struct FAtan {   // every non-negative f32, inf and NaN included
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        out = canon(pt::atanf_glibc(bf((uint32_t)i)));
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = (uint32_t)i, in2 = 0; }
};
struct FAtan2 {   // p[i] = (y, x)
    List<P2> p;
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        out = canon(pt::atan2f_glibc(p[i].a, p[i].b));
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = fb(p.h[i].a), in2 = fb(p.h[i].b); }
};

// the special operands of the atan2f and div_guarded cross products
std::vector<float> special_operands()
{
    const float pos[] = {0.0f, bf(1u), bf(0x007fffffu), 0x1p-126f, 0x1.8p-126f, 0x1p-125f, 0x1p-100f, 1.0f, bf(0x3f7fffffu),
                         bf(0x3f800001u), 0x1p60f, 0x1p124f, 0x1p125f, 0x1p126f, bf(0x7f7fffffu), bf(0x7f800000u)};
    std::vector<float> v;
    for (float p : pos) v.push_back(p), v.push_back(-p);
    v.push_back(bf(0x7fc00000u));
    return v;
}
std::vector<P2> special_pairs()
{
    const std::vector<float> v = special_operands();
    std::vector<P2> p;
    for (float a : v)
        for (float b : v) p.push_back(P2{a, b});
    return p;
}
uint64_t xorshift(uint64_t& s)
{
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    return s;
}
// a float of biased exponent e (1..254), the mantissa and sign from r
float with_exp(int e, uint64_t r) { return bf((uint32_t)(r & 0x807fffffu) | ((uint32_t)e << 23)); }

// (a, b) with exponent(a) - exponent(b) = d, every usable exponent of b, mantissas random or all-0 / all-1
void exp_diff_pairs(std::vector<P2>& out, const int* ds, int nd, uint64_t count, uint64_t seed)
{
    uint64_t s = seed;
    for (uint64_t i = 0; i < count; ++i) {
        const int d = ds[i % (uint64_t)nd];
        const int lo = d > 0 ? 1 : 1 - d, hi = d > 0 ? 254 - d : 254;   // eb in [lo, hi] keeps ea in [1, 254]
        const int eb = lo + (int)(xorshift(s) % (uint64_t)(hi - lo + 1));
        uint64_t ra = xorshift(s), rb = xorshift(s);
        const uint64_t edge = xorshift(s);
        if ((edge & 7) == 0) ra &= ~0x7fffffull;
        if ((edge & 7) == 1) ra |= 0x7fffffull;
        if ((edge & 56) == 0) rb &= ~0x7fffffull;
        if ((edge & 56) == 8) rb |= 0x7fffffull;
        out.push_back(P2{with_exp(eb + d, ra), with_exp(eb, rb)});
    }
}

int section_invtrig()
{
    int bad = 0;
    bad |= run("invtrig.asin", FAsin{}, FAsin::kIn + FAsin::kAbove + FAsin::kTop);
    bad |= run("invtrig.atan", FAtan{}, 1ull << 31);
    {   // check_invtrig.cpp's pairs: 16 xorshift streams, odd draws unit-vector components, even draws raw bits
        const uint64_t per = (1ull << 25) / 16;
        std::vector<P2> pairs(per * 16);
        parallel_for(16, 1, [&](uint64_t t, uint64_t) {
            uint64_t s = 0x9E3779B97F4A7C15ull * (t + 1);
            for (uint64_t i = 0; i < per; ++i) {
                s ^= s << 13; s ^= s >> 7; s ^= s << 17;
                float x, y;
                if (i & 1) {
                    const float a = (float)((s & 0xffffffffu) * (6.283185307179586 / 4294967296.0));
                    const float zz = ((float)((s >> 32) & 0xffffff) / 16777216.0f) * 2.0f - 1.0f;
                    const float rr = sqrtf(1.0f - zz * zz);
                    x = rr * cosf(a);
                    y = rr * sinf(a);
                } else {
                    x = bf((uint32_t)s);
                    y = bf((uint32_t)(s >> 32));
                }
                pairs[t * per + i] = P2{y, x};
            }
        });
        FAtan2 f{upload(pairs)};
        bad |= run("invtrig.atan2.random", f, pairs.size());
        release(f.p);
    }
    {
        const std::vector<P2> pairs = special_pairs();
        FAtan2 f{upload(pairs)};
        bad |= run("invtrig.atan2.special", f, pairs.size());
        release(f.p);
    }
    {   // the k = exponent(y) - exponent(x) switch of e_atan2f.c at +-60
        const int ds[] = {59, 60, 61, 62, -59, -60, -61, -62};
        std::vector<P2> pairs;
        exp_diff_pairs(pairs, ds, 8, 1ull << 20, 0x1234567ull);
        FAtan2 f{upload(pairs)};
        bad |= run("invtrig.atan2.expdiff", f, pairs.size());
        release(f.p);
    }
    {   // quotients in [2^-127, 2^-124] and [2^125, 2^127]: the ends of div_guarded's acceptance window
        const int ds[] = {-128, -127, -126, -125, -124, 124, 125, 126, 127};
        std::vector<P2> pairs;
        exp_diff_pairs(pairs, ds, 9, 1ull << 20, 0x7654321ull);
        FAtan2 f{upload(pairs)};
        bad |= run("invtrig.atan2.window", f, pairs.size());
        release(f.p);
    }
    return bad;
}

// =============================== 5. guarded ===============================
struct FSqrt {   // every non-negative pattern (NaN included), then -0 and 2^16 negative patterns over the whole range
    static constexpr uint64_t kPos = 1ull << 31, kNeg = 1ull << 16;
    HD static uint32_t arg(uint64_t i) { return i < kPos ? (uint32_t)i : 0x80000000u + (uint32_t)(i - kPos) * 0x7fffu; }
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        out = canon(dv_sqrt(bf(arg(i))));
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = arg(i), in2 = 0; }
};
struct FSqrtFinite {   // sqrt_finite_guarded's contract: every finite x >= 0, FSqrt's negative patterns less -inf, three NaNs
    static constexpr uint64_t kPos = 0x7f800000ull, kNeg = FSqrt::kNeg;
    HD static uint32_t arg(uint64_t i)
    {
        if (i < kPos) return (uint32_t)i;
        if (i < kPos + kNeg) {
            const uint32_t u = FSqrt::arg(FSqrt::kPos + (i - kPos));
            return u == 0xff800000u ? 0xff7fffffu : u;
        }
        return i == kPos + kNeg ? 0x7fc00000u : (i == kPos + kNeg + 1 ? 0x7f800001u : 0xffffffffu);
    }
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        out = canon(dv_sqrt_finite(bf(arg(i))));
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = arg(i), in2 = 0; }
};
struct FDivOne {   // pt_tonemap.h's rcp: div_guarded(1, x)
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        out = canon(dv_div(1.0f, bf((uint32_t)i)));
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = fb(1.0f), in2 = (uint32_t)i; }
};
struct FRcp {
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        out = canon(dv_rcp(bf((uint32_t)i)));
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = (uint32_t)i, in2 = 0; }
};
struct FRcpNonneg {   // every x in [0, 2^125] (the function's contract), then three NaNs
    static constexpr uint64_t kIn = 0x7e000000ull + 1;
    HD static uint32_t arg(uint64_t i)
    {
        return i < kIn ? (uint32_t)i : (i == kIn ? 0x7fc00000u : (i == kIn + 1 ? 0x7f800001u : 0x7fffffffu));
    }
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        out = canon(dv_rcp_nonneg(bf(arg(i))));
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = arg(i), in2 = 0; }
};
// exactmath_probe.hip k_div's three operand classes, every quotient kept (normal or not)
struct FDivClass {
    int cls;
    HD static float rnd(uint32_t h, uint32_t h2, int e0, int e1)
    {
        const uint32_t e = (uint32_t)(e0 + (int)(h2 % (uint32_t)(e1 - e0 + 1)));
        return bf((h & 0x807fffffu) | (e << 23));
    }
    HD void operands(uint64_t i, float& a, float& b) const
    {
        const uint32_t h0 = mix(i * 4 + 0), h1 = mix(i * 4 + 1), h2 = mix(i * 4 + 2), h3 = mix(i * 4 + 3);
        if (cls == 0) {          // path-tracer shape: |b| in [2^-4, 1], |a| in [2^-20, 2^7]
            b = rnd(h0, h1, 127 - 4, 127);
            a = rnd(h2, h3, 127 - 20, 127 + 7);
        } else if (cls == 1) {   // wide: exponents over +-60
            b = rnd(h0, h1, 127 - 60, 127 + 60);
            a = rnd(h2, h3, 127 - 60, 127 + 60);
        } else {                 // mantissa edge cases: all-ones / all-zeros significands
            b = bf((h0 & 0x80000000u) | ((uint32_t)(127 - 3 + (h1 % 7)) << 23) | ((h1 & 8) ? 0x7fffffu : (h0 & 0xffu)));
            a = rnd(h2, h3, 127 - 30, 127 + 30);
        }
    }
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        float a, b;
        operands(i, a, b);
        out = canon(dv_div(a, b));
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const
    {
        float a, b;
        operands(i, a, b);
        in = fb(a), in2 = fb(b);
    }
};
struct FDivPairs {   // p[i] = (a, b)
    List<P2> p;
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t&) const
    {
        out = canon(dv_div(p[i].a, p[i].b));
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = fb(p.h[i].a), in2 = fb(p.h[i].b); }
};

// the boundary class: operands within 2 ulp of the guard bounds, quotients straddling the window's ends
std::vector<P2> div_boundary_pairs()
{
    std::vector<float> bs, as, any;
    for (int sg = 0; sg < 2; ++sg)
        for (int k = -2; k <= 2; ++k) {
            bs.push_back(bf((fb(0x1p-125f) + (uint32_t)k) | ((uint32_t)sg << 31)));
            bs.push_back(bf((fb(0x1p125f) + (uint32_t)k) | ((uint32_t)sg << 31)));
            as.push_back(bf((fb(0x1p124f) + (uint32_t)k) | ((uint32_t)sg << 31)));
        }
    // |a| within 2 ulp of 2^-100, the lower guard on a (below it div_rn's remainders are no longer exact)
    for (int sg = 0; sg < 2; ++sg)
        for (int k = -2; k <= 2; ++k) as.push_back(bf((fb(0x1p-100f) + (uint32_t)k) | ((uint32_t)sg << 31)));
    uint64_t s = 0xB0B0B0B0ull;
    for (int i = 0; i < 4096; ++i) any.push_back(with_exp(1 + (int)(xorshift(s) % 254), xorshift(s)));
    for (float sp : special_operands()) any.push_back(sp);
    std::vector<P2> p;
    for (float b : bs) {
        for (float a : as) p.push_back(P2{a, b});
        for (float a : any) p.push_back(P2{a, b});
    }
    for (float a : as)
        for (float b : any) p.push_back(P2{a, b});
    // Operands the first run of this probe found one ulp off (div_guarded then accepted div_rn's
    // result for any |a| < 2^124: with |a| < 2^-102 and a normal quotient the remainders underflow),
    // and the class they belong to: a denormal or below 2^-96, b of any exponent up to 2^23.
    const uint32_t found[][2] = {{0x0000030au, 0x384208dau}, {0x00000029u, 0x361af183u}, {0x8009be59u, 0xbd1be57cu},
                                 {0x8000037du, 0xb85f2486u}, {0x8030d4e9u, 0x37ed5504u}, {0x00a32cbeu, 0x1fb68567u},
                                 {0x037fffffu, 0x419a01bau}, {0x80fe43b4u, 0x3f68d233u}};
    for (const auto& ab : found) p.push_back(P2{bf(ab[0]), bf(ab[1])});
    for (int i = 0; i < (1 << 17); ++i) {
        const uint64_t r = xorshift(s);
        const float a = bf((uint32_t)(r & 0x807fffffu) | ((uint32_t)((r >> 32) % 32) << 23));
        p.push_back(P2{a, with_exp(1 + (int)(xorshift(s) % 150), xorshift(s))});
    }
    // a ~ T b for T = 2^-125, 2^-126 (subnormal below), 2^126, 2^128 (overflow): a within 3 ulp of RN(T b),
    // for random b of every exponent that keeps a finite and non-zero
    const double targets[] = {0x1p-125, 0x1p-126, 0x1p126, 0x1p128};
    for (double T : targets)
        for (int i = 0; i < (1 << 16); ++i) {
            const float b = with_exp(1 + (int)(xorshift(s) % 254), xorshift(s));
            const float a0 = (float)(T * (double)b);   // a scaling by a power of two: exact unless out of range
            if (!(fabsf(a0) > 0.0f) || !(fabsf(a0) <= 3.4028235e38f)) continue;
            for (int k = -3; k <= 3; ++k) {
                const uint32_t u = (fb(a0) & 0x7fffffffu) + (uint32_t)k;
                if (u == 0 || u >= 0x7f800000u) continue;
                p.push_back(P2{bf(u | (fb(a0) & 0x80000000u)), b});
            }
        }
    return p;
}

int section_guarded()
{
    int bad = 0;
    bad |= run("guarded.sqrt", FSqrt{}, FSqrt::kPos + FSqrt::kNeg);
    bad |= run("guarded.sqrt_finite", FSqrtFinite{}, FSqrtFinite::kPos + FSqrtFinite::kNeg + 3);
    bad |= run("guarded.div_one_over_x", FDivOne{}, 1ull << 32);
    for (int cls = 0; cls < 3; ++cls) {
        char name[40];
        snprintf(name, sizeof(name), "guarded.div.class%d", cls);
        bad |= run(name, FDivClass{cls}, 1ull << 28);
    }
    {
        const std::vector<P2> pairs = div_boundary_pairs();
        FDivPairs f{upload(pairs)};
        bad |= run("guarded.div.boundary", f, pairs.size());
        release(f.p);
    }
    {
        const std::vector<P2> pairs = special_pairs();
        FDivPairs f{upload(pairs)};
        bad |= run("guarded.div.special", f, pairs.size());
        release(f.p);
    }
    bad |= run("guarded.rcp", FRcp{}, 1ull << 32);
    bad |= run("guarded.rcp_nonneg", FRcpNonneg{}, FRcpNonneg::kIn + 3);
    return bad;
}

// =============================== 6. envcert ===============================
// aux = certified, out = row << 32 | col (f32 bits for the random sampler, int32 for the nearest one)
struct FCellRandom {
    List<Dir> d;
    float w, h;
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t& aux) const
    {
        const Dir& v = d[i];
        float row = 0.0f, col = 0.0f;
        aux = pt::ec_cell_random(v.z, v.x, v.y, w, h, v.r1, v.r2, row, col) ? 1u : 0u;
        out = (uint64_t)fb(row) << 32 | fb(col);
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = (uint32_t)i, in2 = fb(d.h[i].y); }   // item, d.y
    void note(uint64_t i, char* b, size_t n) const
    {
        const Dir& v = d.h[i];
        snprintf(b, n, " x=%08x y=%08x z=%08x r1=%08x r2=%08x", fb(v.x), fb(v.y), fb(v.z), fb(v.r1), fb(v.r2));
    }
};
struct FCellNearest {
    List<Dir> d;
    float wm1, hm1;
    HD bool operator()(uint64_t i, uint64_t& out, uint32_t& aux) const
    {
        const Dir& v = d[i];
        int32_t row = 0, col = 0;
        aux = pt::ec_cell_nearest(v.z, v.x, v.y, wm1, hm1, row, col) ? 1u : 0u;
        out = (uint64_t)(uint32_t)row << 32 | (uint32_t)col;
        return true;
    }
    void describe(uint64_t i, uint32_t& in, uint32_t& in2) const { in = (uint32_t)i, in2 = fb(d.h[i].y); }   // item, d.y
    void note(uint64_t i, char* b, size_t n) const
    {
        const Dir& v = d.h[i];
        snprintf(b, n, " x=%08x y=%08x z=%08x", fb(v.x), fb(v.y), fb(v.z));
    }
};

// check_envcert.cpp's exact pipelines (pt_v4.hip equirect/sample_random, pt_kernel.hip env_sample), on
// the host build of pt_invtrig.h; fmaf and floorf are exact operations in any libm.  Host functions:
// the device pass parses them and emits nothing.
float saturate(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
void exact_random(float y, float x, float s, float w, float h, float r1, float r2, float& row, float& col)
{
    const float at = pt::atan2f_glibc(y, x), as = pt::asinf_glibc(s);
    float u = fmaf(0.1591f, at, 0.5f), v = fmaf(0.3183f, as, 0.5f);
    u = saturate(u - floorf(u));
    v = saturate(v - floorf(v));
    row = floorf(fmaf(v, h, -v) + r1);
    col = floorf(fmaf(u, w, -u) + r2);
}
bool exact_nearest(float y, float x, float s, int W, int H, int32_t& row, int32_t& col)
{
    float u = pt::atan2f_glibc(y, x), v = pt::asinf_glibc(s);
    u = u * 0.1591f;
    v = v * 0.3183f;
    u = u + 0.5f;
    v = v + 0.5f;
    u -= (float)(int32_t)u;
    v -= (float)(int32_t)v;
    if (!(u >= 0.0f && u < 1.0f && v >= 0.0f && v < 1.0f)) return false;
    row = (int32_t)(v * (float)(H - 1));
    col = (int32_t)(u * (float)(W - 1));
    return true;
}

std::vector<Dir> envcert_directions()
{
    std::vector<Dir> v;
    // check_envcert.cpp item 4: 16 xorshift streams, the grazing scalings, normalised as the kernels do
    const uint64_t per = (1ull << 23) / 16;
    for (uint64_t t = 0; t < 16; ++t) {
        uint64_t st = 0x9E3779B97F4A7C15ull * (t + 1);
        for (uint64_t i = 0; i < per; ++i) {
            const uint64_t a = xorshift(st), b = xorshift(st), c = xorshift(st);
            float dx = (float)((int32_t)(a & 0xffffffffu)) * 0x1p-31f, dy = (float)((int32_t)(b & 0xffffffffu)) * 0x1p-31f,
                  dz = (float)((int32_t)(c & 0xffffffffu)) * 0x1p-31f;
            if (i % 7 == 0) dy *= 0x1p-12f;   // grazing directions
            if (i % 11 == 0) dx *= 0x1p-14f;
            const float dd = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
            if (!(dd > 1e-6f)) continue;
            const float g = 1.0f / __builtin_sqrtf(dd);
            dx *= g, dy *= g, dz *= g;
            const float r1 = (float)(int32_t)(xorshift(st) & 0x7fffffffu) * 0x1p-31f,
                        r2 = (float)(int32_t)(xorshift(st) & 0x7fffffffu) * 0x1p-31f;
            v.push_back(Dir{dx, dy, dz, r1, r2});
        }
    }
    // out of the domain on purpose, one component at a time, the other two ordinary: magnitude 2^-20 +- 2 ulp,
    // below 2^-20, zero, denormal, 2^20 +- 2 ulp, 1 - 2^-20 +- 2 ulp, exactly 1, above 1, NaN
    std::vector<float> odd;
    for (int k = -2; k <= 2; ++k) {
        odd.push_back(bf(fb(0x1p-20f) + (uint32_t)k));
        odd.push_back(bf(fb(0x1p20f) + (uint32_t)k));
        odd.push_back(bf(0x3f7ffff0u + (uint32_t)k));   // 1 - 2^-20
    }
    for (float f : {0x1p-21f, 0x1p-30f, 0x1p-100f, 0.0f, 0x1p-126f, 1.0f, 1.5f, 0x1p30f}) odd.push_back(f);
    odd.push_back(bf(1u)), odd.push_back(bf(0x007fffffu)), odd.push_back(bf(0x7fc00000u)), odd.push_back(bf(0x7f800000u));
    uint64_t st = 0xE7CE47ull;
    for (int slot = 0; slot < 3; ++slot)
        for (float o : odd)
            for (int sg = 0; sg < 2; ++sg)
                for (int rep = 0; rep < 64; ++rep) {
                    float c[3];
                    for (float& q : c) q = (float)((int32_t)(xorshift(st) & 0xffffffffu)) * 0x1p-31f;
                    c[slot] = sg ? -o : o;
                    const float r1 = (float)(int32_t)(xorshift(st) & 0x7fffffffu) * 0x1p-31f,
                                r2 = (float)(int32_t)(xorshift(st) & 0x7fffffffu) * 0x1p-31f;
                    v.push_back(Dir{c[0], c[1], c[2], r1, r2});
                }
    return v;
}

int section_envcert()
{
    int bad = 0;
    const std::vector<Dir> dirs = envcert_directions();
    List<Dir> l = upload(dirs);
    const int sizes[3][2] = {{2048, 1024}, {3, 5}, {1, 1}};
    for (const auto& wh : sizes) {
        const int W = wh[0], H = wh[1];
        char name[48];
        std::atomic<unsigned long long> fb_dev{0}, fb_host{0};
        {
            FCellRandom f{l, (float)W, (float)H};
            const Extra extra = [&](uint64_t i, const Out& g) {
                const Dir& d = dirs[i];
                uint64_t o;
                uint32_t a;
                f(i, o, a);
                fb_host += !a;
                fb_dev += !g.aux;
                if (!g.aux) return true;
                float er, ec;
                exact_random(d.z, d.x, d.y, (float)W, (float)H, d.r1, d.r2, er, ec);
                return g.out == ((uint64_t)fb(er) << 32 | fb(ec));
            };
            snprintf(name, sizeof(name), "envcert.random.%dx%d", W, H);
            bad |= run(name, f, dirs.size(), &extra);
            if (!g_host_only)
                printf("  fallback_rate device=%.4g host=%.4g\n", (double)fb_dev.load() / (double)dirs.size(),
                       (double)fb_host.load() / (double)dirs.size());
        }
        fb_dev = 0, fb_host = 0;
        {
            FCellNearest f{l, (float)(W - 1), (float)(H - 1)};
            const Extra extra = [&](uint64_t i, const Out& g) {
                const Dir& d = dirs[i];
                uint64_t o;
                uint32_t a;
                f(i, o, a);
                fb_host += !a;
                fb_dev += !g.aux;
                if (!g.aux) return true;
                int32_t xr = 0, xc = 0;
                if (!exact_nearest(d.z, d.x, d.y, W, H, xr, xc)) return false;
                return g.out == ((uint64_t)(uint32_t)xr << 32 | (uint32_t)xc);
            };
            snprintf(name, sizeof(name), "envcert.nearest.%dx%d", W, H);
            bad |= run(name, f, dirs.size(), &extra);
            if (!g_host_only)
                printf("  fallback_rate device=%.4g host=%.4g\n", (double)fb_dev.load() / (double)dirs.size(),
                       (double)fb_host.load() / (double)dirs.size());
        }
    }
    release(l);
    return bad;
}

}  // namespace

int main(int argc, char** argv)
{
    const char* what = argc > 1 ? argv[1] : "all";
    g_host_only = argc > 2 && !strcmp(argv[2], "host");
    const struct {
        const char* name;
        int (*fn)();
    } sections[] = {{"sincos", section_sincos}, {"exp", section_exp},         {"pow", section_pow},
                    {"invtrig", section_invtrig}, {"guarded", section_guarded}, {"envcert", section_envcert}};
    int bad = 0, ran = 0;
    for (const auto& s : sections)
        if (!strcmp(what, "all") || !strcmp(what, s.name)) {
            bad |= s.fn();
            ++ran;
        }
    if (!ran) {
        fprintf(stderr, "unknown section %s\n", what);
        return 2;
    }
    return bad ? 1 : 0;
}
