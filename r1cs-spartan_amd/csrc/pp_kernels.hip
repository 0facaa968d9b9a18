// Kernels of the public-parameter structure check and of the derived verifier parameter (DESIGN §6b,
// "Public-parameter structure and views").
//
// Both read every raw point of a parameter once and do a curve addition per pair of points: they are
// bound by the 32-bit-limb field products, not by HBM. Point operations are calls, as in
// verify_kernels.hip: inlined, a kernel body is several times the instruction cache. Integer-only and
// deterministic: a group element does not depend on the order its summands are added in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>

#include "kernels.hpp"

namespace spx {

#define PPCHK(x)                                                              \
    do {                                                                      \
        hipError_t e_ = (x);                                                  \
        if (e_ != hipSuccess) throw std::runtime_error(hipGetErrorString(e_)); \
    } while (0)

template <class F>
static __device__ __noinline__ void pp_madd(Xyzz<F>* p, const Aff<F>* a) {
    xyzz_madd(*p, *a, false);
}
template <class F>
static __device__ __noinline__ void pp_add(Xyzz<F>* p, const Xyzz<F>* q) {
    xyzz_add(*p, *q);
}
template <class F>
DEV bool pp_aff_inf(const Aff<F>& a) {
    return FieldOps<F>::is_zero(a.x) && FieldOps<F>::is_zero(a.y);
}

// ------------------------------------------------------------------ fold relation
// The levels of an nv-variable parameter are contiguous: level i holds 2^(nv - i) points from point
// offset 2^(nv+1) - 2^(nv-i+1). Pair j of the flat array is points 2j, 2j + 1; with r = 2^(nv+1) - 2j
// (the points from the pair to the end, plus 2) its level has 2^m points for 2^m < r <= 2^(m+1).
// ok[j] = 1 if the pair's sum equals point b of the next level, the last level's against `last` (g / h).
// The sum stays in XYZZ and is compared against the affine target T without an inversion:
// X == T.x ZZ and Y == T.y ZZZ; an infinite sum needs the (0, 0) sentinel as its target and the reverse.
template <class F>
__global__ __launch_bounds__(kPPFoldLanes) void k_fold_check(const Aff<F>* __restrict__ pts, int nv, Aff<F> last,
                                                            uint8_t* __restrict__ ok) {
    using O = FieldOps<F>;
    const uint64_t pairs = (1ull << nv) - 1;
    const uint64_t j = blockIdx.x * (uint64_t)kPPFoldLanes + threadIdx.x;
    if (j >= pairs) return;
    const uint64_t r = (2ull << nv) - 2 * j;
    const int m = 63 - __clzll((long long)(r - 1));  // the level has 2^m points: level nv - m
    const uint64_t lvl_off = (2ull << nv) - (2ull << m);
    const uint64_t b = j - lvl_off / 2;
    Aff<F> p0, p1, T;
    load_vec(p0, pts + 2 * j);
    load_vec(p1, pts + 2 * j + 1);
    if (m > 1)
        load_vec(T, pts + lvl_off + (1ull << m) + b);
    else
        T = last;
    Xyzz<F> S;
    if (pp_aff_inf(p0)) {
        xyzz_set_inf(S);
    } else {
        S.x = p0.x;
        S.y = p0.y;
        O::one(S.zz);
        O::one(S.zzz);
    }
    if (!pp_aff_inf(p1)) pp_madd(&S, &p1);  // equal points take madd's doubling branch
    bool good;
    if (xyzz_is_inf(S)) {
        good = pp_aff_inf(T);
    } else if (pp_aff_inf(T)) {
        good = false;
    } else {
        F t;
        O::mul(t, T.x, S.zz);
        good = O::eq(t, S.x);
        O::mul(t, T.y, S.zzz);
        good = good && O::eq(t, S.y);
    }
    ok[j] = good ? 1 : 0;
}

template <class F>
static void fold_check_t(const Aff<F>* pts, int nv, const Aff<F>& last, uint8_t* ok, hipStream_t s) {
    const uint64_t pairs = (1ull << nv) - 1;
    hipLaunchKernelGGL(k_fold_check<F>, dim3((unsigned)((pairs + kPPFoldLanes - 1) / kPPFoldLanes)), dim3(kPPFoldLanes),
                       0, s, pts, nv, last, ok);
    PPCHK(hipGetLastError());
}
void launch_fold_check_g1(const G1Aff* pts, int nv, const G1Aff& g, uint8_t* ok, hipStream_t s) {
    fold_check_t<Fq>(pts, nv, g, ok, s);
}
void launch_fold_check_g2(const G2Aff* pts, int nv, const G2Aff& h, uint8_t* ok, hipStream_t s) {
    fold_check_t<Fq2>(pts, nv, h, ok, s);
}

// ------------------------------------------------------------------ odd-index sums (G1)
template <class F>
DEV Xyzz<F> pp_shfl_xor(const Xyzz<F>& a, int mask) {
    Xyzz<F> r;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(&a);
    uint32_t* d = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(Xyzz<F>) / 4); ++i) d[i] = __shfl_xor(s[i], mask, 64);
    return r;
}
// the block's sum of the lanes' accumulators, in thread 0: a shfl_xor tree per wave (every lane of a
// wave ends with the same sum; xyzz_add takes the doubling and the cancelling cases), the waves through LDS
template <class F>
DEV void pp_block_sum(Xyzz<F>& acc, Xyzz<F>* sh) {
    Xyzz<F> q;
#pragma unroll 1
    for (int m = 1; m < 64; m <<= 1) {
        q = pp_shfl_xor(acc, m);
        pp_add(&acc, &q);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll 1
    for (int w = 1; w < (int)kPPSumThreads / 64; ++w) {
        q = sh[w];
        pp_add(&acc, &q);
    }
}
// part[i * gridDim.x + blockIdx.x] = this block's share of sum_b pts_i[2b + 1], level i = blockIdx.y.
// Each lane adds its strided share of the level's 2^(nv - i - 1) odd points into an XYZZ accumulator;
// equal points (t_{i+1} = 1/2 makes [4b+1] = [4b+3]) take madd's doubling branch.
__global__ __launch_bounds__(kPPSumThreads) void k_odd_sum(const G1Aff* __restrict__ pts, int nv,
                                                          G1Xyzz* __restrict__ part) {
    __shared__ G1Xyzz sh[kPPSumThreads / 64];
    const int i = blockIdx.y;
    const uint64_t lvl_off = (2ull << nv) - (2ull << (nv - i));
    const uint64_t odd = 1ull << (nv - i - 1);
    G1Xyzz acc;
    xyzz_set_inf(acc);
    G1Aff a;
#pragma unroll 1
    for (uint64_t b = blockIdx.x * (uint64_t)kPPSumThreads + threadIdx.x; b < odd;
         b += (uint64_t)gridDim.x * kPPSumThreads) {
        load_vec(a, pts + lvl_off + 2 * b + 1);
        if (!pp_aff_inf(a)) pp_madd(&acc, &a);
    }
    pp_block_sum(acc, sh);
    if (threadIdx.x == 0) store_vec(part + (uint64_t)i * gridDim.x + blockIdx.x, acc);
}
// out[i] = sum of level i's nblk block partials (XYZZ; the host normalises the nv results)
__global__ __launch_bounds__(kPPSumThreads) void k_odd_sum_final(const G1Xyzz* __restrict__ part, uint32_t nblk,
                                                                G1Xyzz* __restrict__ out) {
    __shared__ G1Xyzz sh[kPPSumThreads / 64];
    G1Xyzz acc, q;
    xyzz_set_inf(acc);
#pragma unroll 1
    for (uint32_t k = threadIdx.x; k < nblk; k += kPPSumThreads) {
        load_vec(q, part + (uint64_t)blockIdx.x * nblk + k);
        pp_add(&acc, &q);
    }
    pp_block_sum(acc, sh);
    if (threadIdx.x == 0) store_vec(out + blockIdx.x, acc);
}

uint32_t odd_sum_blocks(int nv) {
    const uint64_t odd = 1ull << (nv - 1);  // the largest level's odd points
    return (uint32_t)std::min<uint64_t>((odd + kPPSumThreads - 1) / kPPSumThreads, kPPSumMaxBlocks);
}
void launch_odd_sum_g1(const G1Aff* pts, int nv, G1Xyzz* part, G1Xyzz* out, hipStream_t s) {
    const uint32_t nblk = odd_sum_blocks(nv);
    hipLaunchKernelGGL(k_odd_sum, dim3(nblk, (unsigned)nv), dim3(kPPSumThreads), 0, s, pts, nv, part);
    hipLaunchKernelGGL(k_odd_sum_final, dim3((unsigned)nv), dim3(kPPSumThreads), 0, s, part, nblk, out);
    PPCHK(hipGetLastError());
}

}  // namespace spx
