// Test-only device library: one thin __global__ wrapper per field / curve device function of
// ff_dev.hpp, ff29.hpp, fq2pair.hpp, curve29.hpp, curve_dev.hpp and the split additions of msm_impl.hpp, so that
// tests/test_gpu_field_ops.py can feed each of them chosen operands (tests/field_cases.py) and read
// the raw result. Nothing here is part of libspartan_hip.so and nothing depends on it.
//
// Every op is "per lane": lane l reads NI words at in + l * NI and writes NO words at out + l * NO.
// How the lanes of a pair / quad share one Fq2 element or one split addition is decided by the
// caller's layout of `in`; the launch is always whole 64-lane waves and no wrapper returns early,
// so both lanes of every pair (all four of every quad) are active together as the DPP exchanges
// of fq2pair.hpp and Split<> require.
#include "msm_impl.hpp"

namespace {
using namespace spx;

template <class F>
struct Io;
template <>
struct Io<F29> {
    static constexpr int W = 14;
    static DEV void ld(F29& r, const uint32_t* in) {
#pragma unroll
        for (int i = 0; i < 14; ++i) r.v[i] = in[i];
    }
    static DEV void st(uint32_t* out, const F29& r) {
#pragma unroll
        for (int i = 0; i < 14; ++i) out[i] = r.v[i];
    }
};
template <>
struct Io<FP29> {
    static constexpr int W = 14;
    static DEV void ld(FP29& r, const uint32_t* in) { Io<F29>::ld(r.v, in); }
    static DEV void st(uint32_t* out, const FP29& r) { Io<F29>::st(out, r.v); }
};
template <>
struct Io<FP29A> {
    static constexpr int W = 14;
    static DEV void ld(FP29A& r, const uint32_t* in) { Io<F29>::ld(r.v, in); }
    static DEV void st(uint32_t* out, const FP29A& r) { Io<F29>::st(out, r.v); }
};
template <>
struct Io<F2_29> {
    static constexpr int W = 28;
    static DEV void ld(F2_29& r, const uint32_t* in) {
        Io<F29>::ld(r.c0, in);
        Io<F29>::ld(r.c1, in + 14);
    }
    static DEV void st(uint32_t* out, const F2_29& r) {
        Io<F29>::st(out, r.c0);
        Io<F29>::st(out + 14, r.c1);
    }
};
template <class C>
struct Io<Fe<C>> {
    static constexpr int W = C::N;
    static DEV void ld(Fe<C>& r, const uint32_t* in) {
#pragma unroll
        for (int i = 0; i < C::N; ++i) r.v[i] = in[i];
    }
    static DEV void st(uint32_t* out, const Fe<C>& r) {
#pragma unroll
        for (int i = 0; i < C::N; ++i) out[i] = r.v[i];
    }
};
template <>
struct Io<Fq2> {
    static constexpr int W = 24;
    static DEV void ld(Fq2& r, const uint32_t* in) {
        Io<Fq>::ld(r.c0, in);
        Io<Fq>::ld(r.c1, in + 12);
    }
    static DEV void st(uint32_t* out, const Fq2& r) {
        Io<Fq>::st(out, r.c0);
        Io<Fq>::st(out + 12, r.c1);
    }
};
template <class F>
DEV void ldx(X29<F>& p, const uint32_t* in) {
    constexpr int W = Io<F>::W;
    Io<F>::ld(p.x, in);
    Io<F>::ld(p.y, in + W);
    Io<F>::ld(p.zz, in + 2 * W);
    Io<F>::ld(p.zzz, in + 3 * W);
}
template <class F>
DEV void stx(uint32_t* out, const X29<F>& p) {
    constexpr int W = Io<F>::W;
    Io<F>::st(out, p.x);
    Io<F>::st(out + W, p.y);
    Io<F>::st(out + 2 * W, p.zz);
    Io<F>::st(out + 3 * W, p.zzz);
}

// ---------------------------------------------------------------- 32-bit limb layer
template <class C>
struct OpMul {  // a, b -> asm product, CIOS product
    static constexpr int N = C::N, NI = 2 * N, NO = 2 * N;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Fe<C> a, b, r, s;
        Io<Fe<C>>::ld(a, in);
        Io<Fe<C>>::ld(b, in + N);
        if constexpr (N == 8)
            fr_mul_asm(r, a, b);
        else
            fq_mul_asm(r, a, b);
        fe_mul_cios(s, a, b);
        Io<Fe<C>>::st(out, r);
        Io<Fe<C>>::st(out + N, s);
    }
};
struct OpFrMulX2 {  // a0, b0, a1, b1 -> r0, r1
    static constexpr int NI = 32, NO = 16;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Fr a0, b0, a1, b1, r0, r1;
        Io<Fr>::ld(a0, in);
        Io<Fr>::ld(b0, in + 8);
        Io<Fr>::ld(a1, in + 16);
        Io<Fr>::ld(b1, in + 24);
        fr_mul_x2_asm(r0, a0, b0, r1, a1, b1);
        Io<Fr>::st(out, r0);
        Io<Fr>::st(out + 8, r1);
    }
};
template <class C>
struct OpLin {  // a, b -> a + b, a - b, -a, 2a
    static constexpr int N = C::N, NI = 2 * N, NO = 4 * N;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Fe<C> a, b, r;
        Io<Fe<C>>::ld(a, in);
        Io<Fe<C>>::ld(b, in + N);
        fe_add(r, a, b);
        Io<Fe<C>>::st(out, r);
        fe_sub(r, a, b);
        Io<Fe<C>>::st(out + N, r);
        fe_neg(r, a);
        Io<Fe<C>>::st(out + 2 * N, r);
        fe_dbl(r, a);
        Io<Fe<C>>::st(out + 3 * N, r);
    }
};
struct OpFrMont {  // a -> to_mont(a), from_mont(a), from_mont(to_mont(a))
    static constexpr int NI = 8, NO = 24;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Fr a, m, f, b;
        Io<Fr>::ld(a, in);
        fr_to_mont(m, a);
        fe_from_mont(f, a);
        fe_from_mont(b, m);
        Io<Fr>::st(out, m);
        Io<Fr>::st(out + 8, f);
        Io<Fr>::st(out + 16, b);
    }
};
struct OpFqMont {  // a -> from_mont(a)
    static constexpr int NI = 12, NO = 12;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Fq a, f;
        Io<Fq>::ld(a, in);
        fe_from_mont(f, a);
        Io<Fq>::st(out, f);
    }
};
struct OpFrCanon {  // a (any 256-bit value) -> a < r
    static constexpr int NI = 8, NO = 1;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Fr a;
        Io<Fr>::ld(a, in);
        out[0] = fr_is_canonical(a) ? 1u : 0u;
    }
};
template <class C>
struct OpInv {
    static constexpr int N = C::N, NI = N, NO = N;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Fe<C> a, r;
        Io<Fe<C>>::ld(a, in);
        fe_inv(r, a);
        Io<Fe<C>>::st(out, r);
    }
};
struct OpF2 {  // a, b -> a b, a^2
    static constexpr int NI = 48, NO = 48;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Fq2 a, b, r;
        Io<Fq2>::ld(a, in);
        Io<Fq2>::ld(b, in + 24);
        f2_mul(r, a, b);
        Io<Fq2>::st(out, r);
        f2_sqr(r, a);
        Io<Fq2>::st(out + 24, r);
    }
};
struct OpF2Inv {
    static constexpr int NI = 24, NO = 24;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Fq2 a, r;
        Io<Fq2>::ld(a, in);
        f2_inv(r, a);
        Io<Fq2>::st(out, r);
    }
};

// ---------------------------------------------------------------- radix-2^29 field ops
struct OpF29Mul {
    static constexpr int NI = 28, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 a, b, r;
        Io<F29>::ld(a, in);
        Io<F29>::ld(b, in + 14);
        f29_mul(r, a, b);
        Io<F29>::st(out, r);
    }
};
struct OpF29Mul2 {
    static constexpr int NI = 56, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 a, b, c, d, r;
        Io<F29>::ld(a, in);
        Io<F29>::ld(b, in + 14);
        Io<F29>::ld(c, in + 28);
        Io<F29>::ld(d, in + 42);
        f29_mul2(r, a, b, c, d);
        Io<F29>::st(out, r);
    }
};
struct OpF29Redc4 {  // a0, b0, a1, b1, a2, b2, a3, b3 in the order of f29_redc_sum4's parameters
    static constexpr int NI = 112, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 x[8], r;
#pragma unroll
        for (int i = 0; i < 8; ++i) Io<F29>::ld(x[i], in + 14 * i);
        f29_redc_sum4(r, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
        Io<F29>::st(out, r);
    }
};
struct OpF29Add {
    static constexpr int NI = 28, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 a, b, r;
        Io<F29>::ld(a, in);
        Io<F29>::ld(b, in + 14);
        f29_add(r, a, b);
        Io<F29>::st(out, r);
    }
};
template <int K>
struct OpF29Sub {
    static constexpr int NI = 28, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 a, b, r;
        Io<F29>::ld(a, in);
        Io<F29>::ld(b, in + 14);
        f29_sub<K>(r, a, b);
        Io<F29>::st(out, r);
    }
};
template <int K>
struct OpF29Csub {
    static constexpr int NI = 14, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 x;
        Io<F29>::ld(x, in);
        f29_csub<K>(x);
        Io<F29>::st(out, x);
    }
};
template <int K>
struct OpF29Reduce {
    static constexpr int NI = 14, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 x;
        Io<F29>::ld(x, in);
        f29_reduce<K>(x);
        Io<F29>::st(out, x);
    }
};
struct OpF29Canon {
    static constexpr int NI = 14, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 x;
        Io<F29>::ld(x, in);
        f29_canon(x);
        Io<F29>::st(out, x);
    }
};
// the predicates of Ops29<F>: zero2, zero4, zero_lt<4>, zero_lt<8>, zero_lt<16>, is_zero_raw
template <class F>
DEV void preds(uint32_t* out, const F& x) {
    using O = Ops29<F>;
    out[0] = O::zero2(x) ? 1u : 0u;
    out[1] = O::zero4(x) ? 1u : 0u;
    out[2] = O::template zero_lt<4>(x) ? 1u : 0u;
    out[3] = O::template zero_lt<8>(x) ? 1u : 0u;
    out[4] = O::template zero_lt<16>(x) ? 1u : 0u;
    out[5] = O::is_zero_raw(x) ? 1u : 0u;
}
struct OpF29Pred {
    static constexpr int NI = 14, NO = 6;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 x;
        Io<F29>::ld(x, in);
        preds<F29>(out, x);
    }
};
struct OpF29Pack {  // x -> pack(x) (12 words), unpack(pack(x))
    static constexpr int NI = 14, NO = 26;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 x, y;
        uint32_t w[12];
        Io<F29>::ld(x, in);
        f29_pack(w, x);
        f29_unpack(y, w);
#pragma unroll
        for (int i = 0; i < 12; ++i) out[i] = w[i];
        Io<F29>::st(out + 12, y);
    }
};
struct OpF29Unpack {  // 12 words -> limbs
    static constexpr int NI = 12, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        uint32_t w[12];
        F29 y;
#pragma unroll
        for (int i = 0; i < 12; ++i) w[i] = in[i];
        f29_unpack(y, w);
        Io<F29>::st(out, y);
    }
};

// ---------------------------------------------------------------- the Fq2 forms (F2_29, FP29, FP29A)
template <class F>
struct OpQMul {
    static constexpr int W = Io<F>::W, NI = 2 * W, NO = W;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F a, b, r;
        Io<F>::ld(a, in);
        Io<F>::ld(b, in + W);
        Ops29<F>::mul(r, a, b);
        Io<F>::st(out, r);
    }
};
template <class F>
struct OpQMulSum {
    static constexpr int W = Io<F>::W, NI = 4 * W, NO = W;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F a, b, c, d, r;
        Io<F>::ld(a, in);
        Io<F>::ld(b, in + W);
        Io<F>::ld(c, in + 2 * W);
        Io<F>::ld(d, in + 3 * W);
        Ops29<F>::mul_sum(r, a, b, c, d);
        Io<F>::st(out, r);
    }
};
template <class F, int KB>
struct OpQSqr {
    static constexpr int W = Io<F>::W, NI = W, NO = W;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F a, r;
        Io<F>::ld(a, in);
        Ops29<F>::template sqr_b<KB>(r, a);
        Io<F>::st(out, r);
    }
};
template <class F>
struct OpQPred {  // x -> one, the six predicates on x
    static constexpr int W = Io<F>::W, NI = W, NO = W + 6;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F x, o;
        Io<F>::ld(x, in);
        Ops29<F>::one(o);
        Io<F>::st(out, o);
        preds<F>(out + W, x);
    }
};

// ---------------------------------------------------------------- curve formulas
template <class F>
struct OpMadd {  // acc (X, Y, ZZ, ZZZ), ax, ay, neg -> acc
    static constexpr int W = Io<F>::W, NI = 6 * W + 1, NO = 4 * W;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        X29<F> p;
        F ax, ay;
        ldx(p, in);
        Io<F>::ld(ax, in + 4 * W);
        Io<F>::ld(ay, in + 5 * W);
        x29_madd(p, ax, ay, in[6 * W] != 0);
        stx(out, p);
    }
};
template <class F>
struct OpAffDbl {
    static constexpr int W = Io<F>::W, NI = 2 * W, NO = 4 * W;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        X29<F> p;
        F ax, ay;
        Io<F>::ld(ax, in);
        Io<F>::ld(ay, in + W);
        x29_from_aff_dbl(p, ax, ay);
        stx(out, p);
    }
};
template <class F, bool kSplit>
struct OpAdd {
    static constexpr int W = Io<F>::W, NI = 8 * W, NO = 4 * W;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        X29<F> p, q;
        ldx(p, in);
        ldx(q, in + 4 * W);
        if constexpr (kSplit)
            x29_add_split(p, q);
        else
            x29_add(p, q);
        stx(out, p);
    }
};
template <class F, bool kSplit>
struct OpDbl {
    static constexpr int W = Io<F>::W, NI = 4 * W, NO = 4 * W;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        X29<F> p;
        ldx(p, in);
        if constexpr (kSplit)
            x29_dbl_split(p);
        else
            x29_dbl(p);
        stx(out, p);
    }
};

// ---------------------------------------------------------------- 32-bit-limb XYZZ layer (curve_dev.hpp)
// one whole point per lane (F = Fq: 12 words per coordinate, Fq2: 24), Montgomery R = 2^384, canonical
template <class F>
DEV void ldz(Xyzz<F>& p, const uint32_t* in) {
    constexpr int W = Io<F>::W;
    Io<F>::ld(p.x, in);
    Io<F>::ld(p.y, in + W);
    Io<F>::ld(p.zz, in + 2 * W);
    Io<F>::ld(p.zzz, in + 3 * W);
}
template <class F>
DEV void stz(uint32_t* out, const Xyzz<F>& p) {
    constexpr int W = Io<F>::W;
    Io<F>::st(out, p.x);
    Io<F>::st(out + W, p.y);
    Io<F>::st(out + 2 * W, p.zz);
    Io<F>::st(out + 3 * W, p.zzz);
}
template <class F>
struct OpZMadd {  // acc (X, Y, ZZ, ZZZ), ax, ay, neg -> acc
    static constexpr int W = Io<F>::W, NI = 6 * W + 1, NO = 4 * W;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Xyzz<F> p;
        Aff<F> a;
        ldz(p, in);
        Io<F>::ld(a.x, in + 4 * W);
        Io<F>::ld(a.y, in + 5 * W);
        xyzz_madd(p, a, in[6 * W] != 0);
        stz(out, p);
    }
};
template <class F>
struct OpZAdd {  // p, q -> p + q
    static constexpr int W = Io<F>::W, NI = 8 * W, NO = 4 * W;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Xyzz<F> p, q;
        ldz(p, in);
        ldz(q, in + 4 * W);
        xyzz_add(p, q);
        stz(out, p);
    }
};
template <class F>
struct OpZDbl {  // p -> 2p into another point, 2p in place (as every caller in the library uses it)
    static constexpr int W = Io<F>::W, NI = 4 * W, NO = 8 * W;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Xyzz<F> p, r;
        ldz(p, in);
        xyzz_dbl(r, p);
        stz(out, r);
        xyzz_dbl(p, p);
        stz(out + 4 * W, p);
    }
};
template <class F>
struct OpZAffDbl {  // ax, ay -> 2a
    static constexpr int W = Io<F>::W, NI = 2 * W, NO = 4 * W;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Xyzz<F> r;
        Aff<F> a;
        Io<F>::ld(a.x, in);
        Io<F>::ld(a.y, in + W);
        xyzz_from_aff_dbl(r, a);
        stz(out, r);
    }
};
template <class F>
struct OpZMulSmall {  // p, k -> k p
    static constexpr int W = Io<F>::W, NI = 4 * W + 1, NO = 4 * W;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Xyzz<F> p, r;
        ldz(p, in);
        xyzz_mul_small(r, p, in[4 * W]);
        stz(out, r);
    }
};
template <class F>
struct OpZFromAff {  // ax, ay (the (0, 0) sentinel: infinity) -> point, xyzz_is_inf(point)
    static constexpr int W = Io<F>::W, NI = 2 * W, NO = 4 * W + 1;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        Xyzz<F> r;
        Aff<F> a;
        Io<F>::ld(a.x, in);
        Io<F>::ld(a.y, in + W);
        xyzz_from_aff(r, a);
        stz(out, r);
        out[4 * W] = xyzz_is_inf(r) ? 1u : 0u;
    }
};

template <class Op>
__global__ __launch_bounds__(64) void k_op(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const size_t lane = blockIdx.x * (size_t)64 + threadIdx.x;
    Op::run(in + lane * Op::NI, out + lane * Op::NO);
}

template <class Op>
int run_op(const uint32_t* in, uint32_t* out, uint64_t lanes, int* ni, int* no) {
    *ni = Op::NI;
    *no = Op::NO;
    if (!in) return 0;  // shape query
    if (lanes == 0 || lanes % 64 != 0 || lanes > (1ull << 20)) return -1;
    const size_t bi = lanes * Op::NI * sizeof(uint32_t), bo = lanes * Op::NO * sizeof(uint32_t);
    uint32_t *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&din, bi);
    if (e == hipSuccess) e = hipMalloc(&dout, bo);
    if (e == hipSuccess) e = hipMemcpy(din, in, bi, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0xA5, bo);
    if (e == hipSuccess) {
        k_op<Op><<<dim3((unsigned)(lanes / 64)), dim3(64)>>>(din, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return (int)e;
}

template <class F>
int run_q(int sub, const uint32_t* in, uint32_t* out, uint64_t lanes, int* ni, int* no) {
    switch (sub) {
        case 0: return run_op<OpQMul<F>>(in, out, lanes, ni, no);
        case 1: return run_op<OpQMulSum<F>>(in, out, lanes, ni, no);
        case 2: return run_op<OpQSqr<F, 8>>(in, out, lanes, ni, no);
        case 3: return run_op<OpQSqr<F, 16>>(in, out, lanes, ni, no);
        case 4: return run_op<OpQPred<F>>(in, out, lanes, ni, no);
    }
    return -2;
}
template <class F>
int run_c(int sub, const uint32_t* in, uint32_t* out, uint64_t lanes, int* ni, int* no) {
    switch (sub) {
        case 0: return run_op<OpMadd<F>>(in, out, lanes, ni, no);
        case 1: return run_op<OpAffDbl<F>>(in, out, lanes, ni, no);
        case 2: return run_op<OpAdd<F, false>>(in, out, lanes, ni, no);
        case 3: return run_op<OpDbl<F, false>>(in, out, lanes, ni, no);
    }
    return -2;
}
template <class F>
int run_z(int sub, const uint32_t* in, uint32_t* out, uint64_t lanes, int* ni, int* no) {
    switch (sub) {
        case 0: return run_op<OpZMadd<F>>(in, out, lanes, ni, no);
        case 1: return run_op<OpZAdd<F>>(in, out, lanes, ni, no);
        case 2: return run_op<OpZDbl<F>>(in, out, lanes, ni, no);
        case 3: return run_op<OpZAffDbl<F>>(in, out, lanes, ni, no);
        case 4: return run_op<OpZMulSmall<F>>(in, out, lanes, ni, no);
        case 5: return run_op<OpZFromAff<F>>(in, out, lanes, ni, no);
    }
    return -2;
}
}  // namespace

// Runs op `op` on `lanes` lanes (a multiple of 64): copies in, launches whole waves, copies out.
// Returns the HIP error code (0 = success), -1 for a bad lane count, -2 for an unknown op. With
// in == nullptr only the per-lane word counts are written to *ni / *no. The op ids are those of
// tests/field_cases.py (OPS).
extern "C" int spx_field_op(int op, const uint32_t* in, uint32_t* out, uint64_t lanes, int* ni, int* no) {
    switch (op) {
        case 0: return run_op<OpMul<FrCfg>>(in, out, lanes, ni, no);
        case 1: return run_op<OpMul<FqCfg>>(in, out, lanes, ni, no);
        case 2: return run_op<OpFrMulX2>(in, out, lanes, ni, no);
        case 3: return run_op<OpLin<FrCfg>>(in, out, lanes, ni, no);
        case 4: return run_op<OpLin<FqCfg>>(in, out, lanes, ni, no);
        case 5: return run_op<OpFrMont>(in, out, lanes, ni, no);
        case 6: return run_op<OpFrCanon>(in, out, lanes, ni, no);
        case 7: return run_op<OpFqMont>(in, out, lanes, ni, no);
        case 8: return run_op<OpInv<FrCfg>>(in, out, lanes, ni, no);
        case 9: return run_op<OpInv<FqCfg>>(in, out, lanes, ni, no);
        case 10: return run_op<OpF2>(in, out, lanes, ni, no);
        case 11: return run_op<OpF2Inv>(in, out, lanes, ni, no);
        case 20: return run_op<OpF29Mul>(in, out, lanes, ni, no);
        case 21: return run_op<OpF29Mul2>(in, out, lanes, ni, no);
        case 22: return run_op<OpF29Redc4>(in, out, lanes, ni, no);
        case 23: return run_op<OpF29Add>(in, out, lanes, ni, no);
        case 24: return run_op<OpF29Sub<2>>(in, out, lanes, ni, no);
        case 25: return run_op<OpF29Sub<4>>(in, out, lanes, ni, no);
        case 26: return run_op<OpF29Sub<8>>(in, out, lanes, ni, no);
        case 27: return run_op<OpF29Sub<16>>(in, out, lanes, ni, no);
        case 28: return run_op<OpF29Csub<1>>(in, out, lanes, ni, no);
        case 29: return run_op<OpF29Csub<2>>(in, out, lanes, ni, no);
        case 30: return run_op<OpF29Csub<4>>(in, out, lanes, ni, no);
        case 31: return run_op<OpF29Csub<8>>(in, out, lanes, ni, no);
        case 32: return run_op<OpF29Canon>(in, out, lanes, ni, no);
        case 33: return run_op<OpF29Reduce<4>>(in, out, lanes, ni, no);
        case 34: return run_op<OpF29Reduce<8>>(in, out, lanes, ni, no);
        case 35: return run_op<OpF29Reduce<16>>(in, out, lanes, ni, no);
        case 36: return run_op<OpF29Pred>(in, out, lanes, ni, no);
        case 37: return run_op<OpF29Pack>(in, out, lanes, ni, no);
        case 38: return run_op<OpF29Unpack>(in, out, lanes, ni, no);
        case 40: case 41: case 42: case 43: case 44: return run_q<F2_29>(op - 40, in, out, lanes, ni, no);
        case 50: case 51: case 52: case 53: case 54: return run_q<FP29>(op - 50, in, out, lanes, ni, no);
        case 60: case 61: case 62: case 63: case 64: return run_q<FP29A>(op - 60, in, out, lanes, ni, no);
        case 80: case 81: case 82: case 83: return run_c<F29>(op - 80, in, out, lanes, ni, no);
        case 90: case 91: case 92: case 93: return run_c<FP29A>(op - 90, in, out, lanes, ni, no);
        case 100: return run_op<OpAdd<F29, true>>(in, out, lanes, ni, no);
        case 101: return run_op<OpDbl<F29, true>>(in, out, lanes, ni, no);
        case 102: return run_op<OpAdd<FP29, true>>(in, out, lanes, ni, no);
        case 103: return run_op<OpDbl<FP29, true>>(in, out, lanes, ni, no);
        case 110: case 111: case 112: case 113: case 114: case 115: return run_z<Fq>(op - 110, in, out, lanes, ni, no);
        case 120: case 121: case 122: case 123: case 124: case 125: return run_z<Fq2>(op - 120, in, out, lanes, ni, no);
    }
    return -2;
}
