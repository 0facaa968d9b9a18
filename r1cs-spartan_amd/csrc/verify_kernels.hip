// Kernels of the batch verifier (spx_verify_many): decompression of the proofs' points
// and segmented linear combinations of them.
//
// Both are one point per lane. A batch has a few thousand points at most, so the launches are a few
// dozen waves wide and latency-bound: the layout favours few registers per lane and small code over
// occupancy. Point operations are calls (one instance per curve in this translation unit): a kernel
// body with its doublings and additions inline is several times the instruction cache.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "kernels.hpp"

namespace spx {

#define VCHK(x)                                                               \
    do {                                                                      \
        hipError_t e_ = (x);                                                  \
        if (e_ != hipSuccess) throw std::runtime_error(hipGetErrorString(e_)); \
    } while (0)

// ------------------------------------------------------------------ fixed exponents of the square roots
struct Exp12 {
    uint32_t v[12];
};
// (q >> shift) + add
static constexpr Exp12 q_shifted(int shift, uint32_t add) {
    Exp12 e{};
    for (int i = 0; i < 12; ++i) e.v[i] = (kFqP[i] >> shift) | (i + 1 < 12 ? kFqP[i + 1] << (32 - shift) : 0u);
    for (int i = 0; i < 12 && add; ++i) {
        const uint32_t s = e.v[i] + add;
        add = s < e.v[i] ? 1u : 0u;
        e.v[i] = s;
    }
    return e;
}
__device__ __constant__ constexpr Exp12 kExpQp1d4 = q_shifted(2, 1);  // (q + 1) / 4
__device__ __constant__ constexpr Exp12 kExpQm3d4 = q_shifted(2, 0);  // (q - 3) / 4
__device__ __constant__ constexpr Exp12 kExpQm1d2 = q_shifted(1, 0);  // (q - 1) / 2
// R^2 mod q: canonical -> Montgomery by one product
__device__ __constant__ constexpr uint32_t kVfQR2[12] = {0x1c341746u, 0xf4df1f34u, 0x09d104f1u, 0x0a76e6a6u,
                                                        0x4c95b6d5u, 0x8de5476cu, 0x939d83c0u, 0x67eb88a9u,
                                                        0xb519952du, 0x9a793e85u, 0x92cae3aau, 0x11988fe5u};

static constexpr int kLanes = 64;  // threads per block of the one-point-per-lane kernels

// a^e for a fixed 384-bit exponent, W-bit windows, the same digits in every lane. The table a^1 ..
// a^(2^W - 1) lives in LDS, word-interleaved over the lanes (word k of entry d of lane l at
// ((d - 1) words + k) 64 + l: conflict-free): 15 Fq per lane do not fit the register file beside the
// product's operands, and a table indexed by a run-time digit would go to scratch.
template <class F>
struct Words {
    static constexpr int n = (int)(sizeof(F) / 4);
};
template <class F>
DEV void lds_put(uint32_t* tab, int d, const F& a) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&a);
#pragma unroll
    for (int k = 0; k < Words<F>::n; ++k) tab[((d - 1) * Words<F>::n + k) * kLanes + threadIdx.x] = w[k];
}
template <class F>
DEV void lds_get(F& a, const uint32_t* tab, int d) {
    uint32_t* w = reinterpret_cast<uint32_t*>(&a);
#pragma unroll
    for (int k = 0; k < Words<F>::n; ++k) w[k] = tab[((d - 1) * Words<F>::n + k) * kLanes + threadIdx.x];
}
template <class F, int W>
DEV void pow_fixed(F& r, const F& a, const Exp12& e, uint32_t* tab) {
    using O = FieldOps<F>;
    static_assert(384 % W == 0, "window");
    F t = a;
    lds_put(tab, 1, t);
#pragma unroll 1
    for (int d = 2; d < (1 << W); ++d) {
        O::mul(t, t, a);
        lds_put(tab, d, t);
    }
    F acc;
    O::one(acc);
    bool started = false;
#pragma unroll 1
    for (int pos = 384 - W; pos >= 0; pos -= W) {
        if (started) {
#pragma unroll 1
            for (int k = 0; k < W; ++k) O::sqr(acc, acc);
        }
        const int lo = pos >> 5, sh = pos & 31;
        uint32_t d = e.v[lo] >> sh;
        if (sh + W > 32) d |= e.v[lo + 1] << (32 - sh);  // pos + W <= 384: lo + 1 <= 11 here
        d &= (1u << W) - 1u;
        if (d) {
            lds_get(t, tab, (int)d);
            if (started)
                O::mul(acc, acc, t);
            else
                acc = t;
            started = true;
        }
    }
    r = acc;
}

// ------------------------------------------------------------------ decompression
// 48 bytes (LE) -> Montgomery; the two flag bits come back in `flags` (bit 0: infinity, bit 1:
// positive y) and are masked off the value, as host::fq_from_bytes does. false: value >= q.
DEV bool fq_load_canon(Fq& m, const uint8_t* p, uint32_t& flags) {
    Fq c;
    const uint4* s = reinterpret_cast<const uint4*>(p);
    uint4* d = reinterpret_cast<uint4*>(&c);
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = s[i];
    flags = c.v[11] >> 30;
    c.v[11] &= 0x3fffffffu;
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const uint64_t t = (uint64_t)c.v[i] - kFqP[i] - br;
        br = (uint32_t)(t >> 63);
    }
    Fq r2;
#pragma unroll
    for (int i = 0; i < 12; ++i) r2.v[i] = kVfQR2[i];
    fe_mul(m, c, r2);
    return br != 0;
}
// canonical-integer a > b (ark-ff Ord)
DEV bool fq_canon_gt(const Fq& a, const Fq& b) {
    Fq x, y;
    fe_from_mont(x, a);
    fe_from_mont(y, b);
    bool gt = false, decided = false;
#pragma unroll
    for (int i = 11; i >= 0; --i) {
        if (!decided && x.v[i] != y.v[i]) {
            gt = x.v[i] > y.v[i];
            decided = true;
        }
    }
    return gt;
}
DEV bool canon_gt(const Fq& a, const Fq& b) { return fq_canon_gt(a, b); }
DEV bool canon_gt(const Fq2& a, const Fq2& b) {  // c1 first, then c0
    if (!fe_eq(a.c1, b.c1)) return fq_canon_gt(a.c1, b.c1);
    return fq_canon_gt(a.c0, b.c0);
}
DEV void curve_b(Fq& b) {
    fe_one(b);
    fe_add(b, b, b);
    fe_add(b, b, b);
}
DEV void curve_b(Fq2& b) {
    curve_b(b.c0);
    b.c1 = b.c0;
}
// q = 3 mod 4: a^((q + 1) / 4)
DEV bool sqrt_f(Fq& r, const Fq& a, uint32_t* tab) {
    pow_fixed<Fq, 4>(r, a, kExpQp1d4, tab);
    Fq s;
    fe_sqr(s, r);
    return fe_eq(s, a);
}
// Algorithm 9 of "Square root computation over even extension fields" (q = 3 mod 4); 3-bit windows:
// the 7-entry table of a 64-lane block is 42 KiB of LDS, the 15 entries of 4-bit windows would be 90
DEV bool sqrt_f(Fq2& r, const Fq2& a, uint32_t* tab) {
    Fq2 a1, alpha, x0, x, m1;
    pow_fixed<Fq2, 3>(a1, a, kExpQm3d4, tab);
    f2_mul(x0, a1, a);
    f2_mul(alpha, a1, x0);
    f2_one(m1);
    f2_neg(m1, m1);
    if (f2_eq(alpha, m1)) {
        fe_neg(x.c0, x0.c1);
        x.c1 = x0.c0;
    } else {
        Fq2 b, one;
        f2_one(one);
        f2_add(b, one, alpha);
        pow_fixed<Fq2, 3>(b, b, kExpQm1d2, tab);
        f2_mul(x, b, x0);
    }
    Fq2 s;
    f2_sqr(s, x);
    r = x;
    return f2_eq(s, a);
}
template <class F>
struct Dec;
template <>
struct Dec<Fq> {
    static constexpr int kBytes = 48, kTabWords = 15 * 12 * kLanes;
    static DEV bool load_x(Fq& x, const uint8_t* p, uint32_t& flags) { return fq_load_canon(x, p, flags); }
};
template <>
struct Dec<Fq2> {
    static constexpr int kBytes = 96, kTabWords = 7 * 24 * kLanes;
    static DEV bool load_x(Fq2& x, const uint8_t* p, uint32_t& flags) {
        uint32_t f0;
        const bool ok0 = fq_load_canon(x.c0, p, f0);  // the first half's flag bits are ignored
        const bool ok1 = fq_load_canon(x.c1, p + 48, flags);
        return ok0 && ok1;
    }
};

// host::g1_decompress / g2_decompress (pairing.hpp) per lane: canonical x, the infinity flag, y =
// sqrt(x^3 + b), rejection when the root does not square back, the sign by canon_gt(-y) against the
// positive-y flag. A rejected point and infinity both store the (0, 0) sentinel; ok tells them apart.
template <class F>
__global__ __launch_bounds__(kLanes) void k_decompress(const uint8_t* __restrict__ in, uint64_t n, Aff<F>* __restrict__ out,
                                                       uint8_t* __restrict__ ok) {
    using O = FieldOps<F>;
    __shared__ uint32_t tab[Dec<F>::kTabWords];
    const uint64_t j = blockIdx.x * (uint64_t)kLanes + threadIdx.x;
    if (j >= n) return;  // no barrier below: a lane's table slots are its own
    Aff<F> a;
    O::zero(a.x);
    O::zero(a.y);
    F x;
    uint32_t flags;
    bool good = Dec<F>::load_x(x, in + j * Dec<F>::kBytes, flags);
    if (good && !(flags & 1u)) {
        F rhs, b, y, ny;
        O::sqr(rhs, x);
        O::mul(rhs, rhs, x);
        curve_b(b);
        O::add(rhs, rhs, b);
        good = sqrt_f(y, rhs, tab);
        if (good) {
            O::neg(ny, y);
            if (canon_gt(y, ny) != ((flags & 2u) != 0)) y = ny;
            a.x = x;
            a.y = y;
        }
    }
    store_vec(out + j, a);
    ok[j] = good ? 1 : 0;
}

void launch_decompress_g1(const uint8_t* in, uint64_t n, G1Aff* out, uint8_t* ok, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_decompress<Fq>, dim3((unsigned)((n + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, in, n, out, ok);
    VCHK(hipGetLastError());
}
void launch_decompress_g2(const uint8_t* in, uint64_t n, G2Aff* out, uint8_t* ok, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_decompress<Fq2>, dim3((unsigned)((n + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, in, n, out, ok);
    VCHK(hipGetLastError());
}

// ------------------------------------------------------------------ segmented linear combination
template <class F>
static __device__ __noinline__ void pt_dbl(Xyzz<F>* p) {
    xyzz_dbl(*p, *p);
}
template <class F>
static __device__ __noinline__ void pt_add(Xyzz<F>* p, const Xyzz<F>* q) {
    xyzz_add(*p, *q);
}
template <class F>
static __device__ __noinline__ void pt_madd(Xyzz<F>* p, const Aff<F>* a) {
    xyzz_madd(*p, *a, false);
}
template <class F>
DEV bool aff_is_inf(const Aff<F>& a) {
    return FieldOps<F>::is_zero(a.x) && FieldOps<F>::is_zero(a.y);
}

// prod[j] = k_j P_j. Plain 4-bit windows from the scalar's top non-zero digit down, so a 128-bit
// coefficient costs half of a full scalar. The 15 multiples of P_j are XYZZ points in global scratch
// (tab[(d - 1) n + j]): beside the accumulator they do not fit the registers, and in LDS a block's G2
// tables would be 360 KiB.
template <class F>
__global__ __launch_bounds__(kLanes) void k_lincomb_mul(const Aff<F>* __restrict__ pts, const Fr* __restrict__ scalars,
                                                        uint64_t n, Xyzz<F>* __restrict__ tab, Xyzz<F>* __restrict__ prod) {
    const uint64_t j = blockIdx.x * (uint64_t)kLanes + threadIdx.x;
    if (j >= n) return;
    Xyzz<F> acc;
    xyzz_set_inf(acc);
    Aff<F> P;
    load_vec(P, pts + j);
    const uint32_t* sc = reinterpret_cast<const uint32_t*>(scalars + j);  // canonical, 8 words
    int top = -1;  // highest non-zero 4-bit digit
#pragma unroll 1
    for (int w = 63; w >= 0; --w)
        if ((sc[w >> 3] >> (4 * (w & 7))) & 15u) {
            top = w;
            break;
        }
    if (top >= 0 && !aff_is_inf(P)) {
        Xyzz<F> t;
        xyzz_set_inf(t);
#pragma unroll 1
        for (int d = 1; d < 16; ++d) {
            pt_madd(&t, &P);  // d = 2 takes madd's doubling branch
            store_vec(tab + (uint64_t)(d - 1) * n + j, t);
        }
#pragma unroll 1
        for (int w = top; w >= 0; --w) {
            if (w != top) {
#pragma unroll 1
                for (int k = 0; k < 4; ++k) pt_dbl(&acc);
            }
            const uint32_t d = (sc[w >> 3] >> (4 * (w & 7))) & 15u;
            if (d) {
                load_vec(t, tab + (uint64_t)(d - 1) * n + j);
                pt_add(&acc, &t);
            }
        }
    }
    store_vec(prod + j, acc);
}

template <class F>
DEV Xyzz<F> shfl_xor_pt(const Xyzz<F>& a, int mask) {
    Xyzz<F> r;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(&a);
    uint32_t* d = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(Xyzz<F>) / 4); ++i) d[i] = __shfl_xor(s[i], mask, 64);
    return r;
}

// out[s] = sum of prod over segment s, affine. One block per segment: every lane adds its strided
// share, a shfl_xor tree sums the wave (both lanes of a pair compute the same sum; xyzz_add takes the
// doubling and the cancelling cases), the waves meet in LDS, and thread 0 normalises.
static constexpr int kRedThreads = 256;
template <class F>
__global__ __launch_bounds__(kRedThreads) void k_lincomb_reduce(const Xyzz<F>* __restrict__ prod,
                                                               const uint64_t* __restrict__ seg_off,
                                                               Aff<F>* __restrict__ out) {
    using O = FieldOps<F>;
    __shared__ Xyzz<F> sh[kRedThreads / 64];
    const uint64_t b = seg_off[blockIdx.x], e = seg_off[blockIdx.x + 1];
    Xyzz<F> acc, q;
    xyzz_set_inf(acc);
#pragma unroll 1
    for (uint64_t i = b + threadIdx.x; i < e; i += kRedThreads) {
        load_vec(q, prod + i);
        pt_add(&acc, &q);
    }
#pragma unroll 1
    for (int m = 1; m < 64; m <<= 1) {
        q = shfl_xor_pt(acc, m);
        pt_add(&acc, &q);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll 1
    for (int w = 1; w < kRedThreads / 64; ++w) {
        q = sh[w];
        pt_add(&acc, &q);
    }
    Aff<F> a;
    O::zero(a.x);
    O::zero(a.y);
    if (!xyzz_is_inf(acc)) {
        F d, i, izz, izzz;
        O::mul(d, acc.zz, acc.zzz);
        O::inv(i, d);
        O::mul(izz, i, acc.zzz);
        O::mul(izzz, i, acc.zz);
        O::mul(a.x, acc.x, izz);
        O::mul(a.y, acc.y, izzz);
    }
    store_vec(out + blockIdx.x, a);
}

size_t lincomb_tmp_bytes(bool g2, uint64_t n) { return (size_t)16 * n * (g2 ? sizeof(G2Xyzz) : sizeof(G1Xyzz)); }

template <class F>
static void lincomb_t(const Aff<F>* pts, const Fr* scalars, uint64_t n, const uint64_t* seg_off, uint32_t nseg,
                      Aff<F>* out, void* tmp, hipStream_t s) {
    if (!nseg) return;
    Xyzz<F>* tab = (Xyzz<F>*)tmp;
    Xyzz<F>* prod = tab + 15 * n;
    if (n)
        hipLaunchKernelGGL(k_lincomb_mul<F>, dim3((unsigned)((n + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, pts, scalars,
                           n, tab, prod);
    hipLaunchKernelGGL(k_lincomb_reduce<F>, dim3(nseg), dim3(kRedThreads), 0, s, prod, seg_off, out);
    VCHK(hipGetLastError());
}
void launch_lincomb_g1(const G1Aff* pts, const Fr* scalars, uint64_t n, const uint64_t* seg_off, uint32_t nseg,
                       G1Aff* out, void* tmp, hipStream_t s) {
    lincomb_t<Fq>(pts, scalars, n, seg_off, nseg, out, tmp, s);
}
void launch_lincomb_g2(const G2Aff* pts, const Fr* scalars, uint64_t n, const uint64_t* seg_off, uint32_t nseg,
                       G2Aff* out, void* tmp, hipStream_t s) {
    lincomb_t<Fq2>(pts, scalars, n, seg_off, nseg, out, tmp, s);
}

}  // namespace spx
