// Test-only device library for the field functions on the bucket accumulation's mixed-addition path
// (ff29.hpp, fq2pair.hpp): the Montgomery scan joined (f29_mul, f29_mul2, f29_redc_sum4) and seeded
// in lockstep pairs (f29_mul_x2, f29_mul2_x2, the symmetric squares f29_sqr_x2), and the lane-pair
// products of PairOps<FP29A>, single and paired, with their prepared operands. tests/test_gpu_accum_ops.py feeds each the operands of
// tests/accum_cases.py and compares the raw words with that module's integer models, word for word.
// Nothing here is part of libspartan_hip.so and nothing depends on it.
//
// As tests/native/field_ops.hip: lane l reads NI words at in + l * NI and writes NO words at
// out + l * NO; launches are whole 64-lane waves and no wrapper returns early, so both lanes of
// every pair are active together as the DPP exchanges of fq2pair.hpp require.
#include "msm_impl.hpp"

namespace {
using namespace spx;

DEV void ld(F29& r, const uint32_t* in) {
#pragma unroll
    for (int i = 0; i < 14; ++i) r.v[i] = in[i];
}
DEV void st(uint32_t* out, const F29& r) {
#pragma unroll
    for (int i = 0; i < 14; ++i) out[i] = r.v[i];
}

struct OpSqrX2 {  // a0, a1 -> f29_sqr_x2, then f29_mul(a0, a0), f29_mul(a1, a1)
    static constexpr int NI = 28, NO = 56;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 a0, a1, r0, r1, s0, s1;
        ld(a0, in);
        ld(a1, in + 14);
        f29_sqr_x2(r0, a0, r1, a1);
        f29_mul(s0, a0, a0);
        f29_mul(s1, a1, a1);
        st(out, r0);
        st(out + 14, r1);
        st(out + 28, s0);
        st(out + 42, s1);
    }
};
struct OpMulX2 {  // a0, b0, a1, b1 -> r0, r1
    static constexpr int NI = 56, NO = 28;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 x[4], r0, r1;
#pragma unroll
        for (int i = 0; i < 4; ++i) ld(x[i], in + 14 * i);
        f29_mul_x2(r0, x[0], x[1], r1, x[2], x[3]);
        st(out, r0);
        st(out + 14, r1);
    }
};
struct OpMul2X2 {  // a0, b0, c0, d0, a1, b1, c1, d1 -> r0, r1
    static constexpr int NI = 112, NO = 28;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 x[8], r0, r1;
#pragma unroll
        for (int i = 0; i < 8; ++i) ld(x[i], in + 14 * i);
        f29_mul2_x2(r0, x[0], x[1], x[2], x[3], r1, x[4], x[5], x[6], x[7]);
        st(out, r0);
        st(out + 14, r1);
    }
};
struct OpPairMulX2 {  // this lane's coefficient of a0, b0, a1, b1 -> r0, r1
    static constexpr int NI = 56, NO = 28;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        FP29A x[4], r0, r1;
#pragma unroll
        for (int i = 0; i < 4; ++i) ld(x[i].v, in + 14 * i);
        Ops29<FP29A>::mul_x2(r0, x[0], x[1], r1, x[2], x[3]);
        st(out, r0.v);
        st(out + 14, r1.v);
    }
};
struct OpPairSqrX2 {  // a0 (c1 < 16p), a1 (c1 < 8p) -> a0^2, a1^2 as x29_madd pairs them
    static constexpr int NI = 28, NO = 28;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        FP29A a0, a1, r0, r1;
        ld(a0.v, in);
        ld(a1.v, in + 14);
        Ops29<FP29A>::template sqr_x2<16, 8>(r0, a0, r1, a1);
        st(out, r0.v);
        st(out + 14, r1.v);
    }
};
struct OpMul {
    static constexpr int NI = 28, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 a, b, r;
        ld(a, in);
        ld(b, in + 14);
        f29_mul(r, a, b);
        st(out, r);
    }
};
struct OpMul2 {
    static constexpr int NI = 56, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 x[4], r;
#pragma unroll
        for (int i = 0; i < 4; ++i) ld(x[i], in + 14 * i);
        f29_mul2(r, x[0], x[1], x[2], x[3]);
        st(out, r);
    }
};
struct OpRedc4 {  // in the order of f29_redc_sum4's parameters
    static constexpr int NI = 112, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 x[8], r;
#pragma unroll
        for (int i = 0; i < 8; ++i) ld(x[i], in + 14 * i);
        f29_redc_sum4(r, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
        st(out, r);
    }
};
struct OpPairMul {  // this lane's coefficient of a, of b
    static constexpr int NI = 28, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        FP29A a, b, r;
        ld(a.v, in);
        ld(b.v, in + 14);
        Ops29<FP29A>::mul(r, a, b);
        st(out, r.v);
    }
};
struct OpPairMulSum {
    static constexpr int NI = 56, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        FP29A x[4], r;
#pragma unroll
        for (int i = 0; i < 4; ++i) ld(x[i].v, in + 14 * i);
        Ops29<FP29A>::mul_sum(r, x[0], x[1], x[2], x[3]);
        st(out, r.v);
    }
};
template <int KB>
struct OpPairSqr {
    static constexpr int NI = 14, NO = 14;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        FP29A a, r;
        ld(a.v, in);
        Ops29<FP29A>::template sqr_b<KB>(r, a);
        st(out, r.v);
    }
};
struct OpPrep {  // b -> y1, y2 of PairOps<FP29A, true>::prep
    static constexpr int NI = 14, NO = 28;
    static DEV void run(const uint32_t* in, uint32_t* out) {
        F29 b, y1, y2;
        ld(b, in);
        Ops29<FP29A>::prep(y1, y2, b, pair_odd());
        st(out, y1);
        st(out + 14, y2);
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
}  // namespace

// Runs op `op` on `lanes` lanes (a multiple of 64). Returns the HIP error code (0 = success), -1 for
// a bad lane count, -2 for an unknown op; with in == nullptr only *ni / *no are written. The op ids
// are those of tests/accum_cases.py (OPS).
extern "C" int spx_accum_op(int op, const uint32_t* in, uint32_t* out, uint64_t lanes, int* ni, int* no) {
    switch (op) {
        case 0: return run_op<OpSqrX2>(in, out, lanes, ni, no);
        case 1: return run_op<OpMul>(in, out, lanes, ni, no);
        case 2: return run_op<OpMul2>(in, out, lanes, ni, no);
        case 3: return run_op<OpRedc4>(in, out, lanes, ni, no);
        case 4: return run_op<OpPairMul>(in, out, lanes, ni, no);
        case 5: return run_op<OpPairMulSum>(in, out, lanes, ni, no);
        case 6: return run_op<OpPairSqr<8>>(in, out, lanes, ni, no);
        case 7: return run_op<OpPairSqr<16>>(in, out, lanes, ni, no);
        case 8: return run_op<OpPrep>(in, out, lanes, ni, no);
        case 9: return run_op<OpMulX2>(in, out, lanes, ni, no);
        case 10: return run_op<OpMul2X2>(in, out, lanes, ni, no);
        case 11: return run_op<OpPairMulX2>(in, out, lanes, ni, no);
        case 12: return run_op<OpPairSqrX2>(in, out, lanes, ni, no);
    }
    return -2;
}
