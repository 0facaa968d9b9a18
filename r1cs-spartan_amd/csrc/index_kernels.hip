// Index build on the GPU ("Index build on the GPU"): the device layouts of an index made
// from the uploaded host CSR by kernels instead of by the host builder (prover.cpp: upload_sparse,
// upload_sliced, build_csc, upload_cols). Every array equals the host builder's byte for byte, so
// nothing here may depend on launch order, block scheduling or the order in which atomics land:
//   * both sorts are stable LSD radix sorts whose every pass is a per-thread count of a contiguous run,
//     one exclusive scan and a per-thread sequential scatter (no atomics, no cross-lane traffic);
//   * the only atomic is a counter of long columns (a sum, the same in any order).
// All entry indices are 32-bit: the host side refuses matrices of 2^31 entries or more.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace spx {

static constexpr int kIdxThreads = 256;
static constexpr uint64_t kScanTile = 1024;  // 256 threads x 4 words
static constexpr int kRadixBits = 4;
static constexpr int kRadixBins = 1 << kRadixBits;
static constexpr uint64_t kRadixRun = 32;  // consecutive entries counted and scattered by one thread

static unsigned idx_grid(uint64_t n) { return (unsigned)((n + kIdxThreads - 1) / kIdxThreads); }

struct alignas(16) Val32 {  // one Fr moved as two 16-byte accesses (value arrays are 32-byte aligned)
    uint4 a, b;
};

// ---------------------------------------------------------------- exclusive scan (32-bit, in place)
__global__ __launch_bounds__(kIdxThreads) void k_idx_scan_tile(uint32_t* __restrict__ d, uint64_t n,
                                                               uint32_t* __restrict__ sums) {
    __shared__ uint32_t sh[kIdxThreads];
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + 4ull * tid;
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = base + k < n ? d[base + k] : 0u;
    const uint32_t t = v[0] + v[1] + v[2] + v[3];
    sh[tid] = t;
    __syncthreads();
    for (uint32_t off = 1; off < kIdxThreads; off <<= 1) {
        const uint32_t x = tid >= off ? sh[tid - off] : 0u;
        __syncthreads();
        sh[tid] += x;
        __syncthreads();
    }
    uint32_t run = sh[tid] - t;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < n) d[base + k] = run;
        run += v[k];
    }
    if (tid == kIdxThreads - 1) sums[blockIdx.x] = sh[tid];
}
__global__ __launch_bounds__(kIdxThreads) void k_idx_scan_add(uint32_t* __restrict__ d, uint64_t n,
                                                              const uint32_t* __restrict__ sums) {
    const uint64_t i = (uint64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (i < n) d[i] += sums[i / kScanTile];
}
uint64_t index_scan_scratch(uint64_t n) {
    uint64_t tot = 0;
    while (n) {
        n = (n + kScanTile - 1) / kScanTile;
        tot += n;
        if (n == 1) break;
    }
    return tot + 1;
}
void launch_index_scan(uint32_t* d, uint64_t n, uint32_t* sums, hipStream_t s) {
    if (!n) return;
    const uint64_t nb = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(k_idx_scan_tile, dim3((unsigned)nb), dim3(kIdxThreads), 0, s, d, n, sums);
    if (nb == 1) return;
    launch_index_scan(sums, nb, sums + nb, s);
    hipLaunchKernelGGL(k_idx_scan_add, dim3(idx_grid(n)), dim3(kIdxThreads), 0, s, d, n, sums);
}

// ---------------------------------------------------------------- stable LSD radix sort of (key, payload)
// thread t owns entries [t kRadixRun, (t + 1) kRadixRun); hist[b T + t] = its count of digit b, which the
// scan turns into the first output slot of (digit b, thread t): digits ascending, threads ascending,
// and inside a thread the run's own order. Each thread's counters are its own LDS column.
__global__ __launch_bounds__(kIdxThreads) void k_idx_radix_hist(const uint32_t* __restrict__ key, uint64_t E, int shift,
                                                                uint32_t* __restrict__ hist, uint64_t T) {
    __shared__ uint32_t c[kRadixBins][kIdxThreads];
    const uint32_t tid = threadIdx.x;
    const uint64_t t = (uint64_t)blockIdx.x * kIdxThreads + tid;
    if (t >= T) return;
#pragma unroll
    for (int b = 0; b < kRadixBins; ++b) c[b][tid] = 0;
    const uint64_t i0 = t * kRadixRun, i1 = i0 + kRadixRun < E ? i0 + kRadixRun : E;
    for (uint64_t i = i0; i < i1; ++i) ++c[(key[i] >> shift) & (kRadixBins - 1)][tid];
#pragma unroll
    for (int b = 0; b < kRadixBins; ++b) hist[(uint64_t)b * T + t] = c[b][tid];
}
__global__ __launch_bounds__(kIdxThreads) void k_idx_radix_scatter(const uint32_t* __restrict__ key,
                                                                   const uint32_t* __restrict__ pay,
                                                                   uint32_t* __restrict__ key_out,
                                                                   uint32_t* __restrict__ pay_out, uint64_t E, int shift,
                                                                   const uint32_t* __restrict__ hist, uint64_t T) {
    __shared__ uint32_t c[kRadixBins][kIdxThreads];
    const uint32_t tid = threadIdx.x;
    const uint64_t t = (uint64_t)blockIdx.x * kIdxThreads + tid;
    if (t >= T) return;
#pragma unroll
    for (int b = 0; b < kRadixBins; ++b) c[b][tid] = hist[(uint64_t)b * T + t];
    const uint64_t i0 = t * kRadixRun, i1 = i0 + kRadixRun < E ? i0 + kRadixRun : E;
    for (uint64_t i = i0; i < i1; ++i) {
        const uint32_t k = key[i];
        const uint32_t p = c[(k >> shift) & (kRadixBins - 1)][tid]++;  // < E: the scan of counts that sum to E
        key_out[p] = k;
        pay_out[p] = pay[i];
    }
}
uint64_t index_sort_hist_words(uint64_t E) { return kRadixBins * ((E + kRadixRun - 1) / kRadixRun); }
int launch_index_sort(uint32_t* key, uint32_t* pay, uint32_t* key2, uint32_t* pay2, uint64_t E, int bits, uint32_t* hist,
                      uint32_t* sums, hipStream_t s) {
    if (!E) return 0;
    const uint64_t T = (E + kRadixRun - 1) / kRadixRun;
    int side = 0;
    for (int shift = 0; shift < bits; shift += kRadixBits, side ^= 1) {
        uint32_t *ki = side ? key2 : key, *pi = side ? pay2 : pay, *ko = side ? key : key2, *po = side ? pay : pay2;
        hipLaunchKernelGGL(k_idx_radix_hist, dim3(idx_grid(T)), dim3(kIdxThreads), 0, s, ki, E, shift, hist, T);
        launch_index_scan(hist, kRadixBins * T, sums, s);
        hipLaunchKernelGGL(k_idx_radix_scatter, dim3(idx_grid(T)), dim3(kIdxThreads), 0, s, ki, pi, ko, po, E, shift, hist, T);
    }
    return side;
}

// ---------------------------------------------------------------- rows
__global__ __launch_bounds__(kIdxThreads) void k_idx_iota(uint32_t* __restrict__ d, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (i < n) d[i] = (uint32_t)i;
}
// ptr[x] = rp[lo + x] - rp[lo], x in [0, nl]
__global__ __launch_bounds__(kIdxThreads) void k_idx_rebase(const uint64_t* __restrict__ rp, uint64_t lo, uint64_t nl,
                                                            uint64_t* __restrict__ ptr) {
    const uint64_t x = (uint64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (x <= nl) ptr[x] = rp[lo + x] - rp[lo];
}
// sliced list, before the sort: entry i = m nl + (x - lo) of the (matrix, row) sequence; its key is the
// column of the row's only entry, or the row itself for an empty (row, matrix)
__global__ __launch_bounds__(kIdxThreads) void k_idx_sliced_keys(IndexSrc src, uint64_t lo, uint64_t nl,
                                                                 uint32_t* __restrict__ key, uint32_t* __restrict__ pay) {
    const uint64_t i = (uint64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (i >= 3 * nl) return;
    const uint32_t m = (uint32_t)(i / nl);
    const uint64_t x = lo + i % nl, k = src.rp[m][x];
    key[i] = src.rp[m][x + 1] > k ? src.col[src.base[m] + k] : (uint32_t)x;
    pay[i] = (uint32_t)i;
}
__global__ __launch_bounds__(kIdxThreads) void k_idx_sliced_fill(IndexSrc src, uint64_t lo, uint64_t nl,
                                                                 const uint32_t* __restrict__ key,
                                                                 const uint32_t* __restrict__ pay, Fr* __restrict__ val,
                                                                 uint32_t* __restrict__ col, uint32_t* __restrict__ dst) {
    const uint64_t e = (uint64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (e >= 3 * nl) return;
    const uint64_t i = pay[e];
    const uint32_t m = (uint32_t)(i / nl);
    const uint64_t xl = i % nl, k = src.rp[m][lo + xl];
    col[e] = key[e];
    dst[e] = (uint32_t)xl | (m << 30);
    Val32 v;
    v.a = v.b = make_uint4(0, 0, 0, 0);
    if (src.rp[m][lo + xl + 1] > k) v = reinterpret_cast<const Val32*>(src.val)[src.base[m] + k];
    reinterpret_cast<Val32*>(val)[e] = v;
}

// ---------------------------------------------------------------- CSC (intermediate)
// rowm[i] = row | matrix << 30 of the concatenated entry pay[i]: the last x with rp[x] <= k
__global__ __launch_bounds__(kIdxThreads) void k_idx_csc_rowm(IndexSrc src, const uint32_t* __restrict__ pay, uint64_t E,
                                                              uint32_t* __restrict__ rowm) {
    const uint64_t i = (uint64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (i >= E) return;
    const uint64_t g = pay[i];
    const uint32_t m = g >= src.base[2] ? 2u : g >= src.base[1] ? 1u : 0u;
    const uint64_t k = g - src.base[m];
    const uint64_t* __restrict__ rp = src.rp[m];
    uint64_t a = 0, b = src.n;  // rp[a] <= k < rp[b]
    while (b - a > 1) {
        const uint64_t mid = (a + b) >> 1;
        if (rp[mid] <= k)
            a = mid;
        else
            b = mid;
    }
    rowm[i] = (uint32_t)a | (m << 30);
}
// last entry wins: sorted entry i is superseded when the next one has its column, matrix and row (the
// sort keeps a row's entries of one column in their order in the row). live[E] = 0 closes the scan.
__global__ __launch_bounds__(kIdxThreads) void k_idx_csc_live(const uint32_t* __restrict__ key,
                                                              const uint32_t* __restrict__ rowm, uint64_t E,
                                                              uint32_t* __restrict__ live) {
    const uint64_t i = (uint64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (i > E) return;
    uint32_t v = 0;
    if (i < E) v = !(i + 1 < E && key[i + 1] == key[i] && rowm[i + 1] == rowm[i]);
    live[i] = v;
}
// pos = the exclusive scan of live ([E + 1]; pos[E] = live entries)
__global__ __launch_bounds__(kIdxThreads) void k_idx_csc_compact(const uint32_t* __restrict__ pos,
                                                                 const uint32_t* __restrict__ key,
                                                                 const uint32_t* __restrict__ rowm,
                                                                 const uint32_t* __restrict__ pay, uint64_t E,
                                                                 uint32_t* __restrict__ ckey, uint32_t* __restrict__ crowm,
                                                                 uint32_t* __restrict__ cpay) {
    const uint64_t i = (uint64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (i >= E) return;
    const uint32_t p = pos[i];
    if (pos[i + 1] == p) return;
    ckey[p] = key[i];
    crowm[p] = rowm[i];
    cpay[p] = pay[i];
}
// cpl[j], j in [0, 3 nl]: the first live entry of (column lo + j / 3, matrix j % 3) in the compacted list
// (cpl[3 nl]: of column lo + nl), so local column y holds entries [cpl[3 y], cpl[3 y + 3])
__global__ __launch_bounds__(kIdxThreads) void k_idx_col_ptr(const uint32_t* __restrict__ ckey,
                                                             const uint32_t* __restrict__ crowm,
                                                             const uint32_t* __restrict__ nlive_p, uint64_t lo,
                                                             uint64_t nl, uint32_t* __restrict__ cpl) {
    const uint64_t j = (uint64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (j > 3 * nl) return;
    const uint64_t want = 4 * (lo + j / 3) + j % 3;
    uint64_t a = 0, b = *nlive_p;  // first i in [0, nlive] with key(i) >= want
    while (a < b) {
        const uint64_t mid = (a + b) >> 1;
        if (4ull * ckey[mid] + (crowm[mid] >> 30) < want)
            a = mid + 1;
        else
            b = mid;
    }
    cpl[j] = (uint32_t)a;
}

// ---------------------------------------------------------------- column stream
// One block per window of 64 kColWindow columns: a column's rank is the number of columns of the window
// that are longer, plus the equally long ones before it (the host builder's stable sort, longest first).
// lanes is preset to kColNone. The column of rank 64 s is its slice's longest.
__global__ __launch_bounds__(kIdxThreads) void k_idx_col_window(const uint32_t* __restrict__ cpl, uint64_t nl,
                                                                uint32_t* __restrict__ lanes,
                                                                uint32_t* __restrict__ slice_len,
                                                                uint32_t* __restrict__ nlong) {
    constexpr uint32_t kWin = 64 * kColWindow;
    __shared__ uint32_t len[kWin];
    const uint64_t w0 = (uint64_t)blockIdx.x * kWin;
    const uint32_t wn = (uint32_t)(nl - w0 < kWin ? nl - w0 : kWin);
    for (uint32_t i = threadIdx.x; i < wn; i += kIdxThreads) {
        uint32_t L = cpl[3 * (w0 + i) + 3] - cpl[3 * (w0 + i)];
        if (L > kLongCol) {
            atomicAdd(nlong, 1u);
            L = 0;
        }
        len[i] = L;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < wn; i += kIdxThreads) {
        const uint32_t my = len[i];
        uint32_t r = 0;
        for (uint32_t j = 0; j < wn; ++j) {
            const uint32_t o = len[j];
            r += (o > my) | ((o == my) & (j < i));
        }
        lanes[w0 + r] = (uint32_t)(w0 + i) | (my << 26);  // r < wn: a permutation of the window
        if ((r & 63) == 0) slice_len[(w0 + r) >> 6] = my;
    }
}
// one thread per lane slot: entry j of lane l of slice si at off + 64 j + l (rowm and val preset to 0)
__global__ __launch_bounds__(kIdxThreads) void k_idx_stream_fill(const ColSlice* __restrict__ slices,
                                                                 const uint32_t* __restrict__ lanes, uint64_t nslots,
                                                                 const uint32_t* __restrict__ cpl,
                                                                 const uint32_t* __restrict__ crowm,
                                                                 const uint32_t* __restrict__ cpay,
                                                                 const Fr* __restrict__ src_val,
                                                                 uint32_t* __restrict__ rowm, Fr* __restrict__ val) {
    const uint64_t t = (uint64_t)blockIdx.x * kIdxThreads + threadIdx.x;
    if (t >= nslots) return;
    const uint32_t info = lanes[t];
    if (info == kColNone) return;
    const uint32_t y = info & 0x3FFFFFFu, n = info >> 26;
    const uint64_t off = slices[t >> 6].off + (t & 63);
    const uint32_t b = cpl[3 * (uint64_t)y];  // n = cpl[3 y + 3] - b entries (0 for a long column)
    for (uint32_t j = 0; j < n; ++j) {
        const uint64_t e = off + 64ull * j;  // j < n <= the slice's len: inside its 64 len slots
        rowm[e] = crowm[b + j];
        reinterpret_cast<Val32*>(val)[e] = reinterpret_cast<const Val32*>(src_val)[cpay[b + j]];
    }
}
// long columns: one block per LongRow record (matrix m, local column x): its entries to the per-matrix
// arrays at the record's first chunk's begin
__global__ __launch_bounds__(kIdxThreads) void k_idx_long_fill(const LongRow* __restrict__ lrows,
                                                               const LongChunk* __restrict__ chunks,
                                                               const uint32_t* __restrict__ cpl,
                                                               const uint32_t* __restrict__ crowm,
                                                               const uint32_t* __restrict__ cpay,
                                                               const Fr* __restrict__ src_val, IndexLongOut out) {
    const LongRow lr = lrows[blockIdx.x];
    const uint64_t begin = chunks[lr.chunk_begin].begin, cnt = chunks[lr.chunk_end - 1].end - begin;
    const uint32_t b = cpl[3 * lr.x + lr.m];  // cnt = cpl[3 x + m + 1] - b
    uint32_t* __restrict__ idx = out.idx[lr.m];
    Val32* __restrict__ val = reinterpret_cast<Val32*>(out.val[lr.m]);
    for (uint64_t k = threadIdx.x; k < cnt; k += kIdxThreads) {
        idx[begin + k] = crowm[b + k] & 0x3FFFFFFFu;
        val[begin + k] = reinterpret_cast<const Val32*>(src_val)[cpay[b + k]];
    }
}

// ---------------------------------------------------------------- launchers
void launch_index_rebase(const uint64_t* rp, uint64_t lo, uint64_t nl, uint64_t* ptr, hipStream_t s) {
    hipLaunchKernelGGL(k_idx_rebase, dim3(idx_grid(nl + 1)), dim3(kIdxThreads), 0, s, rp, lo, nl, ptr);
}
void launch_index_sliced_keys(const IndexSrc& src, uint64_t lo, uint64_t nl, uint32_t* key, uint32_t* pay, hipStream_t s) {
    hipLaunchKernelGGL(k_idx_sliced_keys, dim3(idx_grid(3 * nl)), dim3(kIdxThreads), 0, s, src, lo, nl, key, pay);
}
void launch_index_sliced_fill(const IndexSrc& src, uint64_t lo, uint64_t nl, const uint32_t* key, const uint32_t* pay,
                              Fr* val, uint32_t* col, uint32_t* dst, hipStream_t s) {
    hipLaunchKernelGGL(k_idx_sliced_fill, dim3(idx_grid(3 * nl)), dim3(kIdxThreads), 0, s, src, lo, nl, key, pay, val, col,
                       dst);
}
void launch_index_iota(uint32_t* d, uint64_t n, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_idx_iota, dim3(idx_grid(n)), dim3(kIdxThreads), 0, s, d, n);
}
void launch_index_csc(const IndexSrc& src, const uint32_t* key, const uint32_t* pay, uint64_t E, uint32_t* rowm,
                      uint32_t* pos, uint32_t* sums, uint32_t* ckey, uint32_t* crowm, uint32_t* cpay, hipStream_t s) {
    if (E) hipLaunchKernelGGL(k_idx_csc_rowm, dim3(idx_grid(E)), dim3(kIdxThreads), 0, s, src, pay, E, rowm);
    hipLaunchKernelGGL(k_idx_csc_live, dim3(idx_grid(E + 1)), dim3(kIdxThreads), 0, s, key, rowm, E, pos);
    launch_index_scan(pos, E + 1, sums, s);
    if (E) hipLaunchKernelGGL(k_idx_csc_compact, dim3(idx_grid(E)), dim3(kIdxThreads), 0, s, pos, key, rowm, pay, E, ckey, crowm, cpay);
}
void launch_index_col_ptr(const uint32_t* ckey, const uint32_t* crowm, const uint32_t* nlive, uint64_t lo, uint64_t nl,
                          uint32_t* cpl, hipStream_t s) {
    hipLaunchKernelGGL(k_idx_col_ptr, dim3(idx_grid(3 * nl + 1)), dim3(kIdxThreads), 0, s, ckey, crowm, nlive, lo, nl, cpl);
}
void launch_index_col_window(const uint32_t* cpl, uint64_t nl, uint32_t* lanes, uint32_t* slice_len, uint32_t* nlong,
                             hipStream_t s) {
    const uint64_t win = 64ull * kColWindow;
    hipLaunchKernelGGL(k_idx_col_window, dim3((unsigned)((nl + win - 1) / win)), dim3(kIdxThreads), 0, s, cpl, nl, lanes,
                       slice_len, nlong);
}
void launch_index_stream_fill(const ColSlice* slices, const uint32_t* lanes, uint64_t nslices, const uint32_t* cpl,
                              const uint32_t* crowm, const uint32_t* cpay, const Fr* src_val, uint32_t* rowm, Fr* val,
                              hipStream_t s) {
    if (!nslices) return;
    hipLaunchKernelGGL(k_idx_stream_fill, dim3(idx_grid(64 * nslices)), dim3(kIdxThreads), 0, s, slices, lanes,
                       64 * nslices, cpl, crowm, cpay, src_val, rowm, val);
}
void launch_index_long_fill(const LongRow* lrows, int nlrows, const LongChunk* chunks, const uint32_t* cpl,
                            const uint32_t* crowm, const uint32_t* cpay, const Fr* src_val, const IndexLongOut& out,
                            hipStream_t s) {
    if (!nlrows) return;
    hipLaunchKernelGGL(k_idx_long_fill, dim3((unsigned)nlrows), dim3(kIdxThreads), 0, s, lrows, chunks, cpl, crowm, cpay,
                       src_val, out);
}

}  // namespace spx
