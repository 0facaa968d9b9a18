// Subgroup membership of curve points ("Subgroup membership"): the fixed-scalar
// endomorphism tests, one point per lane.
//
//   G1: phi(x, y) = (beta x, y);                  P in G1  <=>  phi(P) = -[z^2] P
//   G2: psi(x, y) = (conj(x) c_x, conj(y) c_y);   P in G2  <=>  psi(P) = [z] P = -[|z|] P
//
// [|z|] P is 63 doublings and 5 additions, MSB first; |z| is the same in every lane, so the loop is
// uniform. G1 runs the chain twice (the second time over the first one's Jacobian result). The inputs
// are affine Montgomery points on the curve, (0, 0) = infinity (a member), where the batch verifier's
// decompression and the public parameters' raw levels already hold them.
//
// Code size and registers. verify_kernels.hip keeps its code small by calling the point operations
// through pointers, which puts the accumulator in scratch. Here the call is one level down: every Fq
// product is a call that takes and returns its operands in registers (24 + 12 VGPRs), and the point
// operations are inline around it, each once per loop. The accumulator is Jacobian (3 coordinates, and
// a doubling of 7 products where XYZZ takes 9), so the state is the affine input and one accumulator,
// 5 field elements, and stays in registers: no scratch (G1 226 VGPRs, G2 256 VGPRs + 113 AGPRs). The
// whole kernels are 28 KiB (G1) and 64 KiB (G2) of code beside the 4 KiB product, and the loop that runs
// 63 times in 68, the doubling, is a fraction of that: it fits the instruction cache.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>

#include "kernels.hpp"
#include "subgroup_consts.hpp"

namespace spx {

#define SGCHK(x)                                                              \
    do {                                                                      \
        hipError_t e_ = (x);                                                  \
        if (e_ != hipSuccess) throw std::runtime_error(hipGetErrorString(e_)); \
    } while (0)

// the generated 64-bit Montgomery limbs as the device's 32-bit limbs
struct SgWords {
    uint32_t v[12];
};
static constexpr SgWords sg_words(const uint64_t (&m)[6]) {
    SgWords w{};
    for (int i = 0; i < 6; ++i) {
        w.v[2 * i] = (uint32_t)m[i];
        w.v[2 * i + 1] = (uint32_t)(m[i] >> 32);
    }
    return w;
}
__device__ __constant__ constexpr SgWords kDevBeta = sg_words(host::kSgBeta);
__device__ __constant__ constexpr SgWords kDevPsiX0 = sg_words(host::kSgPsiX0);
__device__ __constant__ constexpr SgWords kDevPsiX1 = sg_words(host::kSgPsiX1);
__device__ __constant__ constexpr SgWords kDevPsiY0 = sg_words(host::kSgPsiY0);
__device__ __constant__ constexpr SgWords kDevPsiY1 = sg_words(host::kSgPsiY1);
static constexpr uint64_t kZAbs = host::kSgZAbs;

static constexpr int kSgLanes = (int)kSubgroupLanes;

// ------------------------------------------------------------------ fields whose products are calls
// The layouts of Fq and Fq2: a G1Aff / G2Aff array is read as Aff<FqC> / Aff<Fq2C>.
// (the operands as vectors: of two 48-byte structs the second would be passed in memory)
static __device__ __noinline__ Fq fq_mul_regs(uint4 a0, uint4 a1, uint4 a2, uint4 b0, uint4 b1, uint4 b2) {
    const Fq a = {{a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w}};
    const Fq b = {{b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w}};
    Fq r;
    fe_mul(r, a, b);
    return r;
}
DEV Fq fq_mul_call(const Fq& a, const Fq& b) {
    return fq_mul_regs(make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]), make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]),
                       make_uint4(a.v[8], a.v[9], a.v[10], a.v[11]), make_uint4(b.v[0], b.v[1], b.v[2], b.v[3]),
                       make_uint4(b.v[4], b.v[5], b.v[6], b.v[7]), make_uint4(b.v[8], b.v[9], b.v[10], b.v[11]));
}
struct FqC {
    Fq f;
};
struct Fq2C {
    Fq c0, c1;
};
static_assert(sizeof(Aff<FqC>) == sizeof(G1Aff) && sizeof(Aff<Fq2C>) == sizeof(G2Aff), "layout");
template <>
struct FieldOps<FqC> {
    static DEV void zero(FqC& r) { fe_zero(r.f); }
    static DEV void one(FqC& r) { fe_one(r.f); }
    static DEV bool is_zero(const FqC& a) { return fe_is_zero(a.f); }
    static DEV bool eq(const FqC& a, const FqC& b) { return fe_eq(a.f, b.f); }
    static DEV void add(FqC& r, const FqC& a, const FqC& b) { fe_add(r.f, a.f, b.f); }
    static DEV void sub(FqC& r, const FqC& a, const FqC& b) { fe_sub(r.f, a.f, b.f); }
    static DEV void neg(FqC& r, const FqC& a) { fe_neg(r.f, a.f); }
    static DEV void mul(FqC& r, const FqC& a, const FqC& b) { r.f = fq_mul_call(a.f, b.f); }
    static DEV void sqr(FqC& r, const FqC& a) { r.f = fq_mul_call(a.f, a.f); }
};
template <>
struct FieldOps<Fq2C> {
    static DEV void zero(Fq2C& r) {
        fe_zero(r.c0);
        fe_zero(r.c1);
    }
    static DEV void one(Fq2C& r) {
        fe_one(r.c0);
        fe_zero(r.c1);
    }
    static DEV bool is_zero(const Fq2C& a) { return fe_is_zero(a.c0) && fe_is_zero(a.c1); }
    static DEV bool eq(const Fq2C& a, const Fq2C& b) { return fe_eq(a.c0, b.c0) && fe_eq(a.c1, b.c1); }
    static DEV void add(Fq2C& r, const Fq2C& a, const Fq2C& b) {
        fe_add(r.c0, a.c0, b.c0);
        fe_add(r.c1, a.c1, b.c1);
    }
    static DEV void sub(Fq2C& r, const Fq2C& a, const Fq2C& b) {
        fe_sub(r.c0, a.c0, b.c0);
        fe_sub(r.c1, a.c1, b.c1);
    }
    static DEV void neg(Fq2C& r, const Fq2C& a) {
        fe_neg(r.c0, a.c0);
        fe_neg(r.c1, a.c1);
    }
    // the forms of f2_mul_inl / f2_sqr_inl (ff_dev.hpp)
    static DEV void mul(Fq2C& r, const Fq2C& a, const Fq2C& b) {
        Fq s0, s1;
        fe_add(s0, a.c0, a.c1);
        fe_add(s1, b.c0, b.c1);
        const Fq t0 = fq_mul_call(a.c0, b.c0), t1 = fq_mul_call(a.c1, b.c1);
        Fq m = fq_mul_call(s0, s1);
        fe_sub(r.c0, t0, t1);
        fe_sub(m, m, t0);
        fe_sub(r.c1, m, t1);
    }
    static DEV void sqr(Fq2C& r, const Fq2C& a) {
        Fq s, d;
        fe_add(s, a.c0, a.c1);
        fe_sub(d, a.c0, a.c1);
        const Fq p = fq_mul_call(a.c0, a.c1);
        r.c0 = fq_mul_call(s, d);
        fe_add(r.c1, p, p);
    }
};

DEV void sg_load(Fq& r, const SgWords& w) {
#pragma unroll
    for (int i = 0; i < 12; ++i) r.v[i] = w.v[i];
}

// ------------------------------------------------------------------ Jacobian points (a = 0), Z = 0: infinity
template <class F>
struct Jac {
    F x, y, z;
};
// dbl-2009-l. Infinity stays infinity and a point with y = 0 becomes it: Z3 = 2 Y Z.
template <class F>
DEV void jac_dbl(Jac<F>& p) {
    using O = FieldOps<F>;
    F A, B, C, D, E, t;
    O::sqr(A, p.x);
    O::sqr(B, p.y);
    O::sqr(C, B);
    O::add(t, p.x, B);
    O::sqr(D, t);
    O::sub(D, D, A);
    O::sub(D, D, C);
    O::add(D, D, D);
    O::add(E, A, A);
    O::add(E, E, A);
    O::mul(t, p.y, p.z);
    O::add(p.z, t, t);
    O::sqr(t, E);
    O::sub(t, t, D);
    O::sub(p.x, t, D);
    O::sub(t, D, p.x);
    O::mul(t, E, t);
    O::add(C, C, C);
    O::add(C, C, C);
    O::add(C, C, C);
    O::sub(p.y, t, C);
}
// the tail shared by the two additions: H = U2 - U1 != 0, r = S2 - S1, (U1, S1) = p scaled to the
// common denominator; zh = Z1 (Z2) H
template <class F>
DEV void jac_add_tail(Jac<F>& p, const F& U1, const F& S1, const F& H, const F& r, const F& zh) {
    using O = FieldOps<F>;
    F HH, HHH, V, t;
    O::sqr(HH, H);
    O::mul(HHH, H, HH);
    O::mul(V, U1, HH);
    O::sqr(t, r);
    O::sub(t, t, HHH);
    O::sub(t, t, V);
    O::sub(p.x, t, V);
    O::sub(t, V, p.x);
    O::mul(t, r, t);
    O::mul(HHH, S1, HHH);
    O::sub(p.y, t, HHH);
    p.z = zh;
}
// p += a (a affine, finite)
template <class F>
DEV void jac_madd(Jac<F>& p, const Aff<F>& a) {
    using O = FieldOps<F>;
    if (O::is_zero(p.z)) {
        p.x = a.x;
        p.y = a.y;
        O::one(p.z);
        return;
    }
    F zz, U2, S2, H, r;
    O::sqr(zz, p.z);
    O::mul(U2, a.x, zz);
    O::mul(S2, a.y, p.z);
    O::mul(S2, S2, zz);
    O::sub(H, U2, p.x);
    O::sub(r, S2, p.y);
    if (O::is_zero(H)) {
        if (O::is_zero(r))
            jac_dbl(p);
        else
            O::zero(p.z);
        return;
    }
    O::mul(zz, p.z, H);
    const F U1 = p.x, S1 = p.y;
    jac_add_tail(p, U1, S1, H, r, zz);
}
// p += q
template <class F>
DEV void jac_add(Jac<F>& p, const Jac<F>& q) {
    using O = FieldOps<F>;
    if (O::is_zero(q.z)) return;
    if (O::is_zero(p.z)) {
        p = q;
        return;
    }
    F z1z1, z2z2, U1, U2, S1, S2, H, r;
    O::sqr(z1z1, p.z);
    O::sqr(z2z2, q.z);
    O::mul(U1, p.x, z2z2);
    O::mul(U2, q.x, z1z1);
    O::mul(S1, p.y, q.z);
    O::mul(S1, S1, z2z2);
    O::mul(S2, q.y, p.z);
    O::mul(S2, S2, z1z1);
    O::sub(H, U2, U1);
    O::sub(r, S2, S1);
    if (O::is_zero(H)) {
        if (O::is_zero(r))
            jac_dbl(p);
        else
            O::zero(p.z);
        return;
    }
    O::mul(z1z1, p.z, q.z);
    O::mul(z1z1, z1z1, H);
    jac_add_tail(p, U1, S1, H, r, z1z1);
}

// the endomorphism's image of the (finite) input, and how often the [|z|] chain runs
template <class F>
struct Sg;
template <>
struct Sg<FqC> {
    static constexpr int kChains = 2;
    static DEV void endo(Aff<FqC>& e, const Aff<FqC>& p) {
        Fq beta;
        sg_load(beta, kDevBeta);
        e.x.f = fq_mul_call(p.x.f, beta);
        e.y = p.y;
    }
};
template <>
struct Sg<Fq2C> {
    static constexpr int kChains = 1;
    static DEV void endo(Aff<Fq2C>& e, const Aff<Fq2C>& p) {
        Fq2C c, t;
        t.c0 = p.x.c0;
        fe_neg(t.c1, p.x.c1);
        sg_load(c.c0, kDevPsiX0);
        sg_load(c.c1, kDevPsiX1);
        FieldOps<Fq2C>::mul(e.x, t, c);
        t.c0 = p.y.c0;
        fe_neg(t.c1, p.y.c1);
        sg_load(c.c0, kDevPsiY0);
        sg_load(c.c1, kDevPsiY1);
        FieldOps<Fq2C>::mul(e.y, t, c);
    }
};

// ok[j] = 1: pts[j] is infinity or lies in the prime-order subgroup. The additions take the doubling
// and the cancelling cases (a point of small order meets them), so every input ends with a definite
// answer; an accumulator at infinity for a finite input is a non-member.
template <class F>
__global__ __launch_bounds__(kSgLanes) void k_in_subgroup(const Aff<F>* __restrict__ pts, uint64_t n,
                                                          uint8_t* __restrict__ ok) {
    using O = FieldOps<F>;
#pragma unroll 1
    for (uint64_t j = blockIdx.x * (uint64_t)kSgLanes + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kSgLanes) {
        Aff<F> P;
        load_vec(P, pts + j);
        bool good = true;
        if (!(O::is_zero(P.x) && O::is_zero(P.y))) {
            Jac<F> acc;
            acc.x = P.x;
            acc.y = P.y;
            O::one(acc.z);
#pragma unroll 1
            for (int b = 62; b >= 0; --b) {
                jac_dbl(acc);
                if ((kZAbs >> b) & 1) jac_madd(acc, P);
            }
            if constexpr (Sg<F>::kChains == 2) {
                const Jac<F> base = acc;
#pragma unroll 1
                for (int b = 62; b >= 0; --b) {
                    jac_dbl(acc);
                    if ((kZAbs >> b) & 1) jac_add(acc, base);
                }
            }
            // endo(P) == -acc without an inversion: ex Z^2 = X and ey Z^3 = -Y
            good = !O::is_zero(acc.z);
            if (good) {
                Aff<F> e;
                Sg<F>::endo(e, P);
                F zz, t;
                O::sqr(zz, acc.z);
                O::mul(t, e.x, zz);
                good = O::eq(t, acc.x);
                O::mul(zz, zz, acc.z);
                O::mul(t, e.y, zz);
                O::neg(zz, acc.y);
                good = good && O::eq(t, zz);
            }
        }
        ok[j] = good ? 1 : 0;
    }
}

static unsigned sg_grid(uint64_t n) {
    return (unsigned)std::min<uint64_t>((n + kSgLanes - 1) / kSgLanes, kSubgroupMaxBlocks);
}
void launch_in_subgroup_g1(const G1Aff* pts, uint64_t n, uint8_t* ok, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_in_subgroup<FqC>, dim3(sg_grid(n)), dim3(kSgLanes), 0, s,
                       reinterpret_cast<const Aff<FqC>*>(pts), n, ok);
    SGCHK(hipGetLastError());
}
void launch_in_subgroup_g2(const G2Aff* pts, uint64_t n, uint8_t* ok, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_in_subgroup<Fq2C>, dim3(sg_grid(n)), dim3(kSgLanes), 0, s,
                       reinterpret_cast<const Aff<Fq2C>*>(pts), n, ok);
    SGCHK(hipGetLastError());
}

// out[0] += the zeros among ok[0 .. n), out[1] = min(out[1], index of the first one): a count and a
// minimum, so the result does not depend on the order the blocks run in
__global__ __launch_bounds__(256) void k_ok_scan(const uint8_t* __restrict__ ok, uint64_t n, unsigned long long* out) {
    unsigned long long cnt = 0, first = ~0ull;
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
        if (!ok[j]) {
            ++cnt;
            if (j < first) first = j;
        }
    if (cnt) {
        atomicAdd(out, cnt);
        atomicMin(out + 1, first);
    }
}
void launch_ok_scan(const uint8_t* ok, uint64_t n, uint64_t* out2, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_ok_scan, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 2048)), dim3(256), 0, s, ok, n,
                       reinterpret_cast<unsigned long long*>(out2));
    SGCHK(hipGetLastError());
}

}  // namespace spx
