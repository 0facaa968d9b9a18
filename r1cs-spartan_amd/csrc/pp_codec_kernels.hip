// Bulk conversion between ark-serialize compressed points and the public parameter's device layout
// ("Compressed public parameters"): the kernels of spx_pp_load_compressed and
// spx_pp_serialize_compressed.
//
// Decompression is a throughput kernel: a 2^20 parameter has 2^21 - 2 points per curve and every one
// costs a fixed 381-bit exponentiation (two for G2). All points share the exponent, so the kernels walk
// a compile-time sliding-window schedule (multipliers a and a^3, both in registers): no table, no LDS.
// The arithmetic is the accumulation's radix-2^29 field (ff29.hpp) in its lockstep pairs, so every wave
// carries two independent multiply-add chains: a G1 lane decompresses two points, a G2 lane one point
// whose two Fq2 coefficients are the two chains. Acceptance is that of k_decompress / host::g1_decompress /
// host::g2_decompress. Integer-only and deterministic.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "ff29.hpp"
#include "kernels.hpp"

namespace spx {

#define CDCHK(x)                                                              \
    do {                                                                      \
        hipError_t e_ = (x);                                                  \
        if (e_ != hipSuccess) throw std::runtime_error(hipGetErrorString(e_)); \
    } while (0)

// ------------------------------------------------------------------ constants (R = 2^406, ff29.hpp)
// R^2 mod q: REDC(c R^2) = c R, canonical integer -> field element
__device__ __constant__ constexpr uint32_t kCdR2[14] = {0x15bef7ae, 0x1031cd0e, 0x02dd93e8, 0x09226323, 0x0e6e2cd2,
                                                       0x11684daa, 0x1170e5db, 0x088e25b1, 0x1b366399, 0x1c536f47,
                                                       0x0d1f9cbc, 0x0278b67f, 0x1ea66a2b, 0x0000000c};
// 4 R mod q: the curves' b = 4 and b = 4 (1 + u)
__device__ __constant__ constexpr uint32_t kCdFour[14] = {0x0ea898ba, 0x0e901a40, 0x124a23e8, 0x0d66f84f, 0x0aee547c,
                                                         0x03760629, 0x181b776e, 0x12a47aa6, 0x137ec460, 0x05c6f549,
                                                         0x0fdc4fe8, 0x1707174d, 0x0c3ccef5, 0x0000000c};

// Sliding-window schedule of a fixed exponent, 2-bit windows: walking the bits from kCdTop down, the
// accumulator is squared at every position and then multiplied by a^mul[i] (0: nothing, 1: a, 3: a^3).
// A window "11" at bits (i, i - 1) puts its 3 at i - 1. 143 or 144 products for 381 squarings.
static constexpr int kCdTop = 380;  // (q - 1) / 2 has 380 bits, the other two exponents 379
struct CdSched {
    uint8_t mul[kCdTop + 1];
};
// exponent (q >> shift) + add
static constexpr CdSched cd_sched(int shift, uint32_t add) {
    uint32_t e[12] = {};
    for (int i = 0; i < 12; ++i) e[i] = (kFqP[i] >> shift) | (i + 1 < 12 ? kFqP[i + 1] << (32 - shift) : 0u);
    for (int i = 0; i < 12 && add; ++i) {
        const uint32_t s = e[i] + add;
        add = s < e[i] ? 1u : 0u;
        e[i] = s;
    }
    CdSched s{};
    int i = kCdTop;
    while (i >= 0) {
        const bool b1 = (e[i >> 5] >> (i & 31)) & 1u;
        const bool b0 = i > 0 && ((e[(i - 1) >> 5] >> ((i - 1) & 31)) & 1u);
        if (!b1) {
            --i;
        } else if (b0) {
            s.mul[i - 1] = 3;
            i -= 2;
        } else {
            s.mul[i] = 1;
            --i;
        }
    }
    return s;
}
// [0] (q + 1) / 4: the Fq root. [1] (q - 3) / 4 and [2] (q - 1) / 2: Algorithm 9's two powers in Fq2.
__device__ __constant__ constexpr CdSched kCdSched[3] = {cd_sched(2, 1), cd_sched(2, 0), cd_sched(1, 0)};

// ------------------------------------------------------------------ pairs of field elements in lockstep
// The two chains of a lane: two G1 points' coordinates (PairG1), or the coefficients of one Fq2 (PairG2).
// Values are < 2p unless noted (ff29.hpp's bounds).
using Pair = F2_29;  // c0: chain 0, c1: chain 1

// r = (REDC(a.c0 k), REDC(a.c1 k)) for a constant k
DEV void pair_mulc(Pair& r, const Pair& a, const uint32_t (&k)[14]) {
    F29 c;
    f29_set(c, k);
    f29_mul_x2(r.c0, a.c0, c, r.c1, a.c1, c);
}
// r = (REDC(a.c0), REDC(a.c1)): out of the Montgomery domain, canonical
DEV void pair_from_mont(Pair& r, const Pair& a) {
    F29 one;
    f29_zero(one);
    one.v[0] = 1;
    f29_mul_x2(r.c0, a.c0, one, r.c1, a.c1, one);
    f29_canon(r.c0);
    f29_canon(r.c1);
}
// x >= p for limbs normalized
DEV bool f29_geq_p(const F29& x) {
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        const int32_t t = (int32_t)x.v[i] - (int32_t)Q29::P[i] + c;
        c = t >> 29;
    }
    return (int32_t)x.v[13] - (int32_t)Q29::P[13] + c >= 0;
}
// canonical y > q - y (ark-ff's order on Fq): 2 y >= q, q odd
DEV bool f29_canon_gt_neg(const F29& yc) {
    F29 t;
    f29_add(t, yc, yc);
    return f29_geq_p(t);
}
// canonical -y of canonical y
DEV void f29_neg_canon(F29& r, const F29& y) {
    F29 z;
    f29_zero(z);
    f29_sub<1>(r, z, y);  // q - y, q for y = 0
    f29_canon(r);
}

struct PairG1 {  // two Fq values
    static DEV void sqr(Pair& r, const Pair& a) { f29_sqr_x2(r.c0, a.c0, r.c1, a.c1); }
    static DEV void mul(Pair& r, const Pair& a, const Pair& b) { f29_mul_x2(r.c0, a.c0, b.c0, r.c1, a.c1, b.c1); }
    static DEV void one(Pair& r) {
        f29_one(r.c0);
        f29_one(r.c1);
    }
};
struct PairG2 {  // one Fq2 value, c0 + c1 u
    // (a0 + a1)(a0 - a1) + 2 a0 a1 u; operands < 4p
    static DEV void sqr(Pair& r, const Pair& a) {
        F29 s, d, t;
        f29_add(s, a.c0, a.c1);
        f29_sub<2>(d, a.c0, a.c1);
        f29_add(t, a.c0, a.c0);
        f29_mul_x2(r.c0, s, d, r.c1, t, a.c1);
    }
    // REDC(a0 b0 + a1 (2p - b1)) + REDC(a0 b1 + a1 b0) u
    static DEV void mul(Pair& r, const Pair& a, const Pair& b) {
        F29 nb1, z;
        f29_zero(z);
        f29_sub<2>(nb1, z, b.c1);
        f29_mul2_x2(r.c0, a.c0, b.c0, a.c1, nb1, r.c1, a.c0, b.c1, a.c1, b.c0);
    }
    static DEV void one(Pair& r) {
        f29_one(r.c0);
        f29_zero(r.c1);
    }
};

// r = a^e for schedule `which` of kCdSched: one squaring and one product site per instance (a
// uniform branch to two product sites compiled to 314 registers against 194 for the select)
template <class K>
DEV void pair_pow(Pair& r, const Pair& a, int which) {
    Pair a3, acc;
    K::sqr(acc, a);
    K::mul(a3, acc, a);
    K::one(acc);
#pragma unroll 1
    for (int i = kCdTop; i >= 0; --i) {
        K::sqr(acc, acc);
        const uint32_t d = kCdSched[which].mul[i];  // the same in every lane
        if (d) {
            Pair m;
#pragma unroll
            for (int k = 0; k < 14; ++k) {
                m.c0.v[k] = d == 3 ? a3.c0.v[k] : a.c0.v[k];
                m.c1.v[k] = d == 3 ? a3.c1.v[k] : a.c1.v[k];
            }
            K::mul(acc, acc, m);
        }
    }
    r = acc;
}

// x^3 + b of both chains (b = 4 in each: G1's b twice, or G2's 4 + 4 u)
template <class K>
DEV void pair_rhs(Pair& rhs, const Pair& x) {
    Pair t;
    K::sqr(t, x);
    K::mul(t, t, x);
    F29 four;
    f29_set(four, kCdFour);
    f29_add(rhs.c0, t.c0, four);  // < 3p
    f29_add(rhs.c1, t.c1, four);
    f29_reduce<4>(rhs.c0);
    f29_reduce<4>(rhs.c1);
}
// each chain: a == b mod p
DEV bool f29_eq_mod(const F29& a, const F29& b) {
    F29 d;
    f29_sub<2>(d, a, b);  // < 4p
    return f29_zero4(d);
}

// 48 bytes (LE) -> canonical 29-bit limbs with the flag bits masked off; `flags` bit 0: infinity, bit 1:
// positive y (host::fq_from_bytes). false: the masked value is >= q.
// Again: a second read of bytes the kernel has read before; volatile, so that the compiler reads them
// again and does not keep the first read's words in registers across the exponentiation.
template <bool Again = false>
DEV bool cd_load_canon(F29& c, const uint8_t* p, uint32_t& flags) {
    uint32_t w[12];
    if constexpr (Again) {
        const volatile uint32_t* s = reinterpret_cast<const volatile uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < 12; ++i) w[i] = s[i];
    } else {
        const uint4* s = reinterpret_cast<const uint4*>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint4 q = s[i];
            w[4 * i] = q.x, w[4 * i + 1] = q.y, w[4 * i + 2] = q.z, w[4 * i + 3] = q.w;
        }
    }
    flags = w[11] >> 30;
    w[11] &= 0x3fffffffu;
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const uint64_t t = (uint64_t)w[i] - kFqP[i] - br;
        br = (uint32_t)(t >> 63);
    }
    f29_unpack(c, w);
    return br != 0;
}
// field element (R = 2^406, < 2p) -> the device layout's Fq (R = 2^384, canonical, 12 words)
DEV void cd_store_pair(Fq& o0, Fq& o1, const Pair& a) {
    Pair t;
    pair_mulc(t, a, Q29::TO_R1);
    f29_canon(t.c0);
    f29_canon(t.c1);
    f29_pack(o0.v, t.c0);
    f29_pack(o1.v, t.c1);
}

// the error word: the minimum over all rejected points of (point number in the order G1 levels, G2
// levels) << 2 | reason, so the report names the lowest offender whatever order the blocks ran in
DEV void cd_report(unsigned long long* err, uint64_t point, uint32_t reason) {
    atomicMin(err, (unsigned long long)((point << 2) | reason));
}

static constexpr int kCdLanes = 128;  // threads per block
// two waves per SIMD (256 registers): the register allocator's target, which it meets without scratch
#define SPX_TWO_WAVES __attribute__((amdgpu_waves_per_eu(2)))

// ------------------------------------------------------------------ G1: two points per lane
// Lane t of the grid takes points 2t and 2t + 1. A point that is rejected, infinite or past the end still
// runs its chain beside its neighbour's (on whatever x the bytes gave); only the verdicts differ.
__global__ __launch_bounds__(kCdLanes) SPX_TWO_WAVES void k_decompress_bulk_g1(const uint8_t* __restrict__ in, uint64_t n,
                                                                 G1Aff* __restrict__ out, uint64_t point_base,
                                                                 unsigned long long* __restrict__ err,
                                                                 uint8_t* __restrict__ ok) {
    const uint64_t j0 = 2 * (blockIdx.x * (uint64_t)kCdLanes + threadIdx.x);
    if (j0 >= n) return;
    const bool two = j0 + 1 < n;
    Pair xc;
    uint32_t f0, f1 = 0;
    const bool canon0 = cd_load_canon(xc.c0, in + 48 * j0, f0);
    bool canon1 = true;
    if (two)
        canon1 = cd_load_canon(xc.c1, in + 48 * (j0 + 1), f1);
    else
        xc.c1 = xc.c0;
    Pair x, rhs, y, s;
    pair_mulc(x, xc, kCdR2);
    pair_rhs<PairG1>(rhs, x);
    pair_pow<PairG1>(y, rhs, 0);
    PairG1::sqr(s, y);
    const bool root0 = f29_eq_mod(s.c0, rhs.c0), root1 = f29_eq_mod(s.c1, rhs.c1);
    Pair yc;
    pair_from_mont(yc, y);
    G1Aff a0, a1;
    cd_store_pair(a0.x, a1.x, x);
    cd_store_pair(a0.y, a1.y, y);  // canonical
    {
        F29 t, ny;
        Fq nq;
        f29_unpack(t, a0.y.v);
        f29_neg_canon(ny, t);
        f29_pack(nq.v, ny);
        if (f29_canon_gt_neg(yc.c0) != ((f0 & 2u) != 0)) a0.y = nq;
        f29_unpack(t, a1.y.v);
        f29_neg_canon(ny, t);
        f29_pack(nq.v, ny);
        if (f29_canon_gt_neg(yc.c1) != ((f1 & 2u) != 0)) a1.y = nq;
    }
    const bool inf0 = canon0 && (f0 & 1u), inf1 = canon1 && (f1 & 1u);
    const bool good0 = canon0 && ((f0 & 1u) || root0), good1 = canon1 && ((f1 & 1u) || root1);
    if (!good0 || inf0) {
        fe_zero(a0.x);
        fe_zero(a0.y);
    }
    if (!good1 || inf1) {
        fe_zero(a1.x);
        fe_zero(a1.y);
    }
    store_vec(out + j0, a0);
    if (!good0) cd_report(err, point_base + j0, canon0 ? kCodecNoPoint : kCodecNotCanonical);
    if (ok) ok[j0] = good0 ? 1 : 0;
    if (two) {
        store_vec(out + j0 + 1, a1);
        if (!good1) cd_report(err, point_base + j0 + 1, canon1 ? kCodecNoPoint : kCodecNotCanonical);
        if (ok) ok[j0 + 1] = good1 ? 1 : 0;
    }
}

// ------------------------------------------------------------------ G2: one point per lane
// Algorithm 9 of "Square root computation over even extension fields" (q = 3 mod 4), as host::f2_sqrt:
// a1 = a^((q-3)/4), x0 = a1 a, alpha = a1 x0; the root is u x0 if alpha = -1, else (1 + alpha)^((q-1)/2) x0.
// Both powers run in every lane (alpha = -1 only for a in Fq, and then the second power is of 0).
__global__ __launch_bounds__(kCdLanes) SPX_TWO_WAVES void k_decompress_bulk_g2(const uint8_t* __restrict__ in, uint64_t n,
                                                                 G2Aff* __restrict__ out, uint64_t point_base,
                                                                 unsigned long long* __restrict__ err,
                                                                 uint8_t* __restrict__ ok) {
    const uint64_t j = blockIdx.x * (uint64_t)kCdLanes + threadIdx.x;
    if (j >= n) return;
    Pair xc;
    uint32_t fl, fignored;
    const bool canon0 = cd_load_canon(xc.c0, in + 96 * j, fignored);  // the first half's flag bits are ignored
    const bool canon1 = cd_load_canon(xc.c1, in + 96 * j + 48, fl);
    const bool canon = canon0 && canon1;
    Pair x, rhs, x0, y, base, pw;
    pair_mulc(x, xc, kCdR2);
    pair_rhs<PairG2>(base, x);
    bool is_m1 = false;
    // x0 waits out the second power in this point's own output slot (as x, 96 bytes): in registers it
    // would be the 28 that pass the two-wave budget
    Fq2* const stash = &out[j].x;
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {
        pair_pow<PairG2>(pw, base, phase + 1);
        if (phase == 0) {
            Pair alpha;
            PairG2::mul(x0, pw, base);  // base: x^3 + b
            PairG2::mul(alpha, pw, x0);
            Fq2 w;
            f29_pack(w.c0.v, x0.c0);  // < 2p: 12 words
            f29_pack(w.c1.v, x0.c1);
            store_vec(stash, w);
            F29 one;
            f29_one(one);
            f29_add(base.c0, alpha.c0, one);  // < 3p
            f29_reduce<4>(base.c0);
            base.c1 = alpha.c1;
            is_m1 = f29_zero2(base.c0) && f29_zero2(base.c1);
        }
    }
    {
        uint32_t w[24];
        const volatile uint32_t* sp = reinterpret_cast<const volatile uint32_t*>(stash);  // not forwarded from the store
#pragma unroll
        for (int i = 0; i < 24; ++i) w[i] = sp[i];
        f29_unpack(x0.c0, w);
        f29_unpack(x0.c1, w + 12);
    }
    PairG2::mul(y, pw, x0);
    if (is_m1) {  // u x0 = -x0.c1 + x0.c0 u
        F29 z;
        f29_zero(z);
        f29_sub<2>(y.c0, z, x0.c1);
        f29_canon(y.c0);  // 2p for x0.c1 = 0 would pass the bound of the products below
        y.c1 = x0.c0;
    }
    // x and x^3 + b once more from the bytes: kept across the two powers they would cost the registers
    // that the second wave of the SIMD needs
    cd_load_canon<true>(xc.c0, in + 96 * j, fignored);
    cd_load_canon<true>(xc.c1, in + 96 * j + 48, fignored);
    pair_mulc(x, xc, kCdR2);
    pair_rhs<PairG2>(rhs, x);
    Pair s;
    PairG2::sqr(s, y);
    const bool root = f29_eq_mod(s.c0, rhs.c0) && f29_eq_mod(s.c1, rhs.c1);
    Pair yc;
    pair_from_mont(yc, y);
    G2Aff a;
    cd_store_pair(a.x.c0, a.x.c1, x);
    cd_store_pair(a.y.c0, a.y.c1, y);
    // the sign: ark-ff orders Fq2 by c1 first, then c0
    const bool gt = f29_is_zero_raw(yc.c1) ? f29_canon_gt_neg(yc.c0) : f29_canon_gt_neg(yc.c1);
    if (gt != ((fl & 2u) != 0)) {
        F29 t, ny;
        f29_unpack(t, a.y.c0.v);
        f29_neg_canon(ny, t);
        f29_pack(a.y.c0.v, ny);
        f29_unpack(t, a.y.c1.v);
        f29_neg_canon(ny, t);
        f29_pack(a.y.c1.v, ny);
    }
    const bool inf = canon && (fl & 1u);
    const bool good = canon && ((fl & 1u) || root);
    if (!good || inf) {
        fe_zero(a.x.c0);
        fe_zero(a.x.c1);
        fe_zero(a.y.c0);
        fe_zero(a.y.c1);
    }
    store_vec(out + j, a);
    if (!good) cd_report(err, point_base + j, canon ? kCodecNoPoint : kCodecNotCanonical);
    if (ok) ok[j] = good ? 1 : 0;
}

void launch_decompress_bulk_g1(const uint8_t* in, uint64_t n, G1Aff* out, uint64_t point_base, unsigned long long* err,
                               uint8_t* ok, hipStream_t s) {
    if (!n) return;
    const uint64_t lanes = (n + 1) / 2;
    hipLaunchKernelGGL(k_decompress_bulk_g1, dim3((unsigned)((lanes + kCdLanes - 1) / kCdLanes)), dim3(kCdLanes), 0, s,
                       in, n, out, point_base, err, ok);
    CDCHK(hipGetLastError());
}
void launch_decompress_bulk_g2(const uint8_t* in, uint64_t n, G2Aff* out, uint64_t point_base, unsigned long long* err,
                               uint8_t* ok, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_decompress_bulk_g2, dim3((unsigned)((n + kCdLanes - 1) / kCdLanes)), dim3(kCdLanes), 0, s, in, n,
                       out, point_base, err, ok);
    CDCHK(hipGetLastError());
}

// ------------------------------------------------------------------ compression: one point per lane
// canonical x with the flags of host::g1_compress / g2_compress: positive y iff canonical y > -y (Fq2: c1
// first, then c0), the (0, 0) sentinel as x = 0 with the infinity flag. Two Montgomery reductions per
// coordinate: bound by the stores, not by the arithmetic.
DEV void cd_store48(uint8_t* p, const Fq& c) {
    uint4* d = reinterpret_cast<uint4*>(p);
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = make_uint4(c.v[4 * i], c.v[4 * i + 1], c.v[4 * i + 2], c.v[4 * i + 3]);
}
// canonical a > q - a, from the Montgomery form
DEV bool cd_gt_neg(const Fq& a) {
    Fq c;
    fe_from_mont(c, a);
    uint32_t t[12];
    unsigned cy = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = __builtin_addc(c.v[i], c.v[i], cy, &cy);  // 2 a < 2^382: no carry out
    unsigned br = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) (void)__builtin_subc(t[i], kFqP[i], br, &br);
    return br == 0;  // 2 a >= q
}
static constexpr int kCdCompressLanes = 256;
__global__ __launch_bounds__(kCdCompressLanes) void k_compress_g1(const G1Aff* __restrict__ in, uint64_t n,
                                                                  uint8_t* __restrict__ out) {
    const uint64_t j = blockIdx.x * (uint64_t)kCdCompressLanes + threadIdx.x;
    if (j >= n) return;
    G1Aff a;
    load_vec(a, in + j);
    const bool inf = fe_is_zero(a.x) && fe_is_zero(a.y);
    Fq xc;
    fe_from_mont(xc, a.x);
    const uint32_t flags = inf ? 1u : cd_gt_neg(a.y) ? 2u : 0u;
    xc.v[11] |= flags << 30;
    cd_store48(out + 48 * j, xc);
}
__global__ __launch_bounds__(kCdCompressLanes) void k_compress_g2(const G2Aff* __restrict__ in, uint64_t n,
                                                                  uint8_t* __restrict__ out) {
    const uint64_t j = blockIdx.x * (uint64_t)kCdCompressLanes + threadIdx.x;
    if (j >= n) return;
    G2Aff a;
    load_vec(a, in + j);
    const bool inf = fe_is_zero(a.x.c0) && fe_is_zero(a.x.c1) && fe_is_zero(a.y.c0) && fe_is_zero(a.y.c1);
    Fq x0, x1;
    fe_from_mont(x0, a.x.c0);
    fe_from_mont(x1, a.x.c1);
    const bool gt = fe_is_zero(a.y.c1) ? cd_gt_neg(a.y.c0) : cd_gt_neg(a.y.c1);
    const uint32_t flags = inf ? 1u : gt ? 2u : 0u;
    x1.v[11] |= flags << 30;
    cd_store48(out + 96 * j, x0);
    cd_store48(out + 96 * j + 48, x1);
}
void launch_compress_g1(const G1Aff* in, uint64_t n, uint8_t* out, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_compress_g1, dim3((unsigned)((n + kCdCompressLanes - 1) / kCdCompressLanes)),
                       dim3(kCdCompressLanes), 0, s, in, n, out);
    CDCHK(hipGetLastError());
}
void launch_compress_g2(const G2Aff* in, uint64_t n, uint8_t* out, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_compress_g2, dim3((unsigned)((n + kCdCompressLanes - 1) / kCdCompressLanes)),
                       dim3(kCdCompressLanes), 0, s, in, n, out);
    CDCHK(hipGetLastError());
}

}  // namespace spx
