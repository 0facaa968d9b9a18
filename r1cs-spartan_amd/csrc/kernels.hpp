// Kernel-launch interface shared by the device translation units and the host prover.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "curve_dev.hpp"

namespace spx {

// rows longer than this go to the chunked long-row path (nnz skew, e.g. the dense row of
// the reference's TestSynthesizer at density 0, constraints.rs:77-88)
static constexpr uint64_t kLongRow = 64;
static constexpr uint64_t kChunk = 4096;

struct SparseView3 {            // three CSR (or CSC) matrices, local index space
    const uint64_t* ptr[3];     // [count + 1]
    const uint32_t* idx[3];     // column (CSR) / row (CSC) indices, global
    const Fr* val[3];           // Montgomery values
};
struct LongChunk {
    uint32_t m;
    uint32_t pad;
    uint64_t begin, end;
};
struct LongRow {
    uint32_t m;
    uint32_t chunk_begin, chunk_end;
    uint32_t pad;
    uint64_t x;  // local output index
};
// eval_on_x column stream (k_col_stream): the A, B, C entries of each column concatenated, columns
// sorted by length inside windows of 64 x kColWindow columns and dealt to the 64 lanes of a slice (SELL-64),
// so the lanes of a wave run columns of (nearly) equal length. Columns with more than kLongCol
// entries go to the chunked long path (a lane's length is a 6-bit field).
static constexpr uint32_t kLongCol = 62;
static constexpr uint32_t kColNone = 0xFFFFFFFFu;  // lane slot without a column
static constexpr uint32_t kColWindow = 16;         // slices per sorting window (1024 columns)
struct ColSlice {
    uint64_t off;  // first entry slot of the slice: entry j of lane l at off + 64 j + l
    uint32_t len;  // the slice's longest column (steps)
    uint32_t pad;
};
struct ColStreamView {
    const ColSlice* slices;  // [nslices]
    const uint32_t* lanes;   // [64 nslices]: local column | entries << 26, or kColNone
    const uint32_t* rowm;    // entry slots: row | matrix << 30
    const Fr* val;           // entry slots: Montgomery values
    uint32_t nslices;
};
// sum_over_y for matrices whose every row has at most one entry (the R1CS multiplication-gate form;
// the benchmark generators): the entries of the rank's rows of A, B and C, with an explicit zero entry
// for an empty (row, matrix), sorted by column. Workgroups of XCD d take the d-th eighth of the list
// (k_spmv_sliced), so each XCD gathers a contiguous eighth of z through its own L2, nearly in order,
// instead of every XCD fetching whole 128-byte lines of z for 32-byte reads (k_sparse3<0>: 2.0x its
// algorithmic bytes).
struct SpmvSlicedView {
    const Fr* val;        // [entries] Montgomery values
    const uint32_t* col;  // [entries] global column, ascending
    const uint32_t* dst;  // [entries] local row | matrix << 30
};
// per-block partial sums of one sumcheck round (3 Fr per block, up to 8192 blocks)
static constexpr uint64_t kRoundPartials = 3 * 8192;

struct Tables3 {
    Fr* t[3];
};

// Lockstep groups (spx_ctx_set_group): one launch runs the same sumcheck round of up to kGroupMax
// proofs of one index, proof j's blocks at blockIdx.y = j, each with its own tables, challenge,
// partials, ticket and result (the per-proof launches' arguments, passed by value)
static constexpr int kGroupMax = 16;
// the last rounds of each sumcheck a lockstep group runs on the host (prove_group): <= 5 (the tables
// then fit each proof's 8 KiB pinned region)
static constexpr int kGroupHostTail = 5;
struct Sc1Job {
    Tables3 in, out;
    const Fr* Ein;
    Fr* Eout;
    Fr r;
    Fr* partial;  // kRoundPartials Fr of this proof
    uint32_t* ticket;
    Fr* result3;
};
struct Sc2Job {
    const Fr* Min;
    const Fr* Zin;
    Fr* Mout;
    Fr* Zout;
    Fr r;
    Fr* partial;
    uint32_t* ticket;
    Fr* result3;
};
struct Sc1Group {
    Sc1Job j[kGroupMax];
};
struct Sc2Group {
    Sc2Job j[kGroupMax];
};
// the other steps' jobs: one per proof, as the sumcheck rounds'
struct SpmvJob {
    const Fr* z;
    Fr* o[3];  // Az, Bz, Cz
};
struct EqTableJob {
    const Fr* r;   // nvar device Fr
    Fr* out;       // count Fr
    Fr *lo, *hi;   // scratch tables, 2^13 Fr each
};
struct ColStreamJob {
    const Fr* r_x;    // L device Fr
    const Fr* scale;  // 3 device Fr
    Fr* out;
    Fr* eq_scratch;  // kEqScratch Fr
    Fr* partial;     // the long columns' chunk sums (one Fr per chunk; unused without long columns)
};
struct OpenEvalJob {
    const Fr* z;        // 2^L Fr
    Fr *bufA, *bufB;    // 2^L / 2 and 2^L / 4 Fr: step s of the chain writes buffer s & 1
    const Fr* points;   // L host Fr
    Fr* last;           // receives z(points); null: the value stays where the chain leaves it (open_eval_result)
};
struct CopyJob {  // up to 3 runs of `per` Fr -> dst, back to back
    const Fr* src[3];
    Fr* dst;
};

// ---- live kernel statistics (HIP events around selected launches; off unless enabled)
struct KProf {
    bool on = false;
    struct Rec {
        int id;
        hipEvent_t a, b;
        double bytes, ops;
    };
    std::vector<Rec> open;  // recorded, not yet harvested
    std::vector<hipEvent_t> pool;
    uint64_t launches[16] = {0};
    double ms[16] = {0}, bytes[16] = {0}, ops[16] = {0};
    // the launches moving the most algorithmic bytes per id (e.g. round 1 of a sumcheck: the
    // HBM-streaming case; later rounds are small and cache-resident)
    uint64_t big_launches[16] = {0};
    double big_ms[16] = {0}, big_bytes[16] = {0};
    int cur_id = -1;
    hipEvent_t cur_a = nullptr;
    hipEvent_t get() {
        if (pool.empty()) {
            hipEvent_t e;
            (void)hipEventCreate(&e);
            return e;
        }
        hipEvent_t e = pool.back();
        pool.pop_back();
        return e;
    }
    void begin(int id, hipStream_t s) {
        if (!on) return;
        cur_id = id;
        cur_a = get();
        (void)hipEventRecord(cur_a, s);
    }
    void end(double algo_bytes, hipStream_t s, double n_ops) {
        if (!on || cur_id < 0) return;
        hipEvent_t b = get();
        (void)hipEventRecord(b, s);
        open.push_back({cur_id, cur_a, b, algo_bytes, n_ops});
        cur_id = -1;
    }
    void harvest() {  // call after a stream sync
        for (auto& r : open) {
            float t = 0;
            if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
                launches[r.id] += 1;
                ms[r.id] += t;
                bytes[r.id] += r.bytes;
                ops[r.id] += r.ops;
                const double top = big_launches[r.id] ? big_bytes[r.id] / big_launches[r.id] : 0.0;
                if (r.bytes > top * 1.0001) {
                    big_launches[r.id] = 0, big_ms[r.id] = 0, big_bytes[r.id] = 0;
                }
                if (r.bytes >= top * 0.9999) {
                    big_launches[r.id] += 1;
                    big_ms[r.id] += t;
                    big_bytes[r.id] += r.bytes;
                }
            }
            pool.push_back(r.a);
            pool.push_back(r.b);
        }
        open.clear();
    }
    void reset() {
        for (int i = 0; i < 16; ++i)
            launches[i] = 0, ms[i] = 0, bytes[i] = 0, ops[i] = 0, big_launches[i] = 0, big_ms[i] = 0, big_bytes[i] = 0;
    }
};
extern thread_local KProf* g_kprof;  // set by the host for the calling thread
inline void kp_begin(int id, hipStream_t s) {
    if (g_kprof) g_kprof->begin(id, s);
}
// bytes: algorithmic bytes of the launch; ops: its unit operations (curve additions for the MSM
// levels, table entries elsewhere; 0 where no op count is defined)
inline void kp_end(double bytes, hipStream_t s, double ops = 0) {
    if (g_kprof) g_kprof->end(bytes, s, ops);
}
enum { KP_SC1 = 0, KP_SC2, KP_SPMV, KP_MTV, KP_OPEN, KP_EQ, KP_SORT, KP_ACC_G1, KP_ACC_G2, KP_ACCX_G1, KP_ACCX_G2,
       KP_RED_G1, KP_RED_G2 };

// ---- index_kernels.hip: the index's device layouts built from the uploaded host CSR (index_build_gpu)
struct IndexSrc {           // A, B, C as uploaded: entries concatenated in that order
    const uint64_t* rp[3];  // [n + 1] row pointers of each matrix
    uint64_t base[4];       // first concatenated entry of matrix m; base[3] = all entries (< 2^31)
    const uint32_t* col;    // [base[3]]
    const Fr* val;          // [base[3]] Montgomery
    uint64_t n;
};
struct IndexLongOut {  // DevColStream::longc's per-matrix entry arrays
    uint32_t* idx[3];
    Fr* val[3];
};
// exclusive scan of n 32-bit words in place; sums: index_scan_scratch(n) words
uint64_t index_scan_scratch(uint64_t n);
void launch_index_scan(uint32_t* d, uint64_t n, uint32_t* sums, hipStream_t s);
// stable sort of E (key, payload) pairs by the low `bits` bits of the key, ping-pong between the two
// buffer pairs; returns the pair that holds the result (0: key / pay, 1: key2 / pay2). hist:
// index_sort_hist_words(E) words, sums: index_scan_scratch(that)
uint64_t index_sort_hist_words(uint64_t E);
int launch_index_sort(uint32_t* key, uint32_t* pay, uint32_t* key2, uint32_t* pay2, uint64_t E, int bits, uint32_t* hist,
                      uint32_t* sums, hipStream_t s);
void launch_index_iota(uint32_t* d, uint64_t n, hipStream_t s);
void launch_index_rebase(const uint64_t* rp, uint64_t lo, uint64_t nl, uint64_t* ptr, hipStream_t s);
// the sliced list of rows [lo, lo + nl): 3 nl (column, m nl + row - lo) pairs to sort by column, then the list
void launch_index_sliced_keys(const IndexSrc& src, uint64_t lo, uint64_t nl, uint32_t* key, uint32_t* pay, hipStream_t s);
void launch_index_sliced_fill(const IndexSrc& src, uint64_t lo, uint64_t nl, const uint32_t* key, const uint32_t* pay,
                              Fr* val, uint32_t* col, uint32_t* dst, hipStream_t s);
// CSC of the three matrices from the column-sorted (column, concatenated entry) pairs: row | m << 30 of
// every entry, last-entry-wins, compaction (ckey, crowm, cpay: the live entries; pos[E] = their number;
// pos: E + 1 words, sums: index_scan_scratch(E + 1))
void launch_index_csc(const IndexSrc& src, const uint32_t* key, const uint32_t* pay, uint64_t E, uint32_t* rowm,
                      uint32_t* pos, uint32_t* sums, uint32_t* ckey, uint32_t* crowm, uint32_t* cpay, hipStream_t s);
// cpl[3 y + m], y in [0, nl): first live entry of (column lo + y, matrix m); cpl[3 nl] closes the last
void launch_index_col_ptr(const uint32_t* ckey, const uint32_t* crowm, const uint32_t* nlive, uint64_t lo, uint64_t nl,
                          uint32_t* cpl, hipStream_t s);
// lanes ([64 nslices], preset to kColNone) and every slice's length; *nlong += columns longer than kLongCol
void launch_index_col_window(const uint32_t* cpl, uint64_t nl, uint32_t* lanes, uint32_t* slice_len, uint32_t* nlong,
                             hipStream_t s);
void launch_index_stream_fill(const ColSlice* slices, const uint32_t* lanes, uint64_t nslices, const uint32_t* cpl,
                              const uint32_t* crowm, const uint32_t* cpay, const Fr* src_val, uint32_t* rowm, Fr* val,
                              hipStream_t s);
void launch_index_long_fill(const LongRow* lrows, int nlrows, const LongChunk* chunks, const uint32_t* cpl,
                            const uint32_t* crowm, const uint32_t* cpay, const Fr* src_val, const IndexLongOut& out,
                            hipStream_t s);

// ---- mle_kernels.hip
void launch_to_mont(Fr* d, size_t n, int* err, hipStream_t s);
void launch_from_mont(Fr* out, const Fr* in, size_t n, hipStream_t s);
void launch_sparse3(int mode, const SparseView3& mv, const Fr* vec, Fr* o0, Fr* o1, Fr* o2, const Fr* scale,
                    uint64_t count, const LongChunk* chunks, int nchunks, const LongRow* lrows, int nlrows,
                    Fr* partial, hipStream_t s);
// eq(r_x, .) over L variables as the product of nf tables over consecutive bit fields of x (variable
// 0 = LSB): t[f] has 2^k[f] entries, the last one three copies scaled by r_A, r_B, r_C (m 2^k + x).
// eq_factors_for: nf = 2 (k[0] = ceil(L / 2) <= 13)
struct EqFactors {
    const Fr* t[3];
    int k[3];
    int nf;
};
// the split used for L variables, tables carved from `scratch` (kEqScratch Fr)
static constexpr uint64_t kEqScratch = 4 * 8192;
EqFactors eq_factors_for(int L, Fr* scratch);
// Every launcher below takes the jobs of k proofs (1 <= k <= kGroupMax), as launch_r1cs_check. k == 1
// is the per-proof launch (prove()); k > 1 is ONE launch for a lockstep group, proof j's blocks at
// blockIdx.y = j, running the per-proof kernels' bodies, so each proof's outputs are bit-identical
// to its own launch's. Shapes without a group kernel launch per proof inside the launcher.
//
// SpMV over the column-sorted entry list into jobs[j].o = (Az, Bz, Cz) (k > 1: the entries are
// streamed once for the group)
void launch_spmv_sliced(int k, const SpmvJob* jobs, const SpmvSlicedView& v, uint64_t entries, hipStream_t s);
// out[i] = eq(r, base + i), i < count, over nvar (<= 26) variables
void launch_eq_table(int k, const EqTableJob* jobs, int nvar, uint64_t base, uint64_t count, hipStream_t s);
// out[y] = sum_m scale[m] sum_x eq(r_x, x) M[x][y] over the column stream, then the long columns' chunks
// (over `lv`'s per-matrix entry arrays) added in; an index with long columns launches per proof
void launch_col_stream(int k, const ColStreamJob* jobs, const ColStreamView& cv, int L, const SparseView3& lv,
                       const LongChunk* chunks, int nchunks, const LongRow* lrows, int nlrows, hipStream_t s);
int sc_grid(uint64_t half);
// A round: fold with the previous challenge r (by value; unused in round 1), evaluate the round
// polynomial at 0, 1, 2 (at 1 only if need1: otherwise result3[1] = 0 and the caller derives it from
// the previous claim), and reduce over the blocks into result3 (3 Fr; device or host-mapped pinned
// memory) - in the last block for small grids, by a second one-block launch otherwise.
// partial: kRoundPartials Fr of scratch (3 per block; the quad / lane-pair and wave forms launch more
// blocks than sc_grid(half)); ticket: a device counter that is 0 (left 0). fold and need1 apply to
// every proof. Small rounds that need G(1) / P(1), and a round 1 below 2^14 pairs, have no group kernel.
void launch_sc1_round(int k, const Sc1Job* jobs, bool fold, bool need1, uint64_t half, hipStream_t s);
void launch_sc2_round(int k, const Sc2Job* jobs, bool fold, bool need1, uint64_t half, hipStream_t s);
// what a round launches: the kernel form, its grid per proof, whether the last block reduces (else a
// second launch does), and whether the k proofs are launched one by one. The one place that decides.
enum { kRoundLane = 0, kRoundSplit = 1, kRoundWave = 2 };  // split: a quad (sumcheck 1) / lane pair (2) per pair
struct RoundPlan {
    int form, grid;
    bool fused, per_proof;
};
RoundPlan sc_round_plan(int which, int k, bool fold, bool need1, uint64_t half);
// z(points) of an L-variable table by the opening's fold chain without quotients (the stubbed opening):
// the steps, each writing the buffer its index selects (bufA, bufB, bufA, ...). copy: the chain ends on a
// fold, whose one-entry output is then copied to `last` (where the job names one).
enum { kOpenTail = 0, kOpenFold = 1, kOpenLevel = 2 };
struct OpenStep {
    int kind, first, levels;  // levels [first, first + levels) of the chain
    uint64_t size;            // tail, level: pairs going in; fold: entries coming out
    bool wave;                // fold: the wave-transposed kernel
};
struct OpenEvalPlan {
    std::vector<OpenStep> steps;
    bool copy;
};
OpenEvalPlan open_eval_plan(int L);
void launch_open_eval(int k, const OpenEvalJob* jobs, int L, hipStream_t s);
// where launch_open_eval leaves the job's value: `last`, or the chain's last output if the job names none
const Fr* open_eval_result(const OpenEvalJob& job, int L);
// per proof j: nruns (<= 3) runs of `per` Fr (nruns x per <= 4096) from src[i] to dst back to back, one launch
void launch_copy_runs(int k, const CopyJob* jobs, int nruns, int per, hipStream_t s);
void launch_open_level(const Fr* rin, Fr* rout, Fr* q, const Fr& point, uint64_t half, hipStream_t s);
// Witness check (k_r1cs_check): over the rank-local tables Az, Bz, Cz (nl rows each, row0 =
// the global index of local row 0) the rows with Az[i] Bz[i] != Cz[i] are counted and the lowest one is
// found. One job per proof (blockIdx.y; k <= kGroupMax), one launch, no other launch or copy:
//   partial: 2 x uint64 per block of the launch (at most kR1csMaxBlocks blocks);
//   ticket:  a device counter that is 0 (left 0), as the sumcheck rounds';
//   record:  kR1csRecordWords uint64 (device or host-mapped pinned memory, 16-byte aligned): the count,
//            the global first row (UINT64_MAX if none), then Az, Bz, Cz of that row (Montgomery; zero if
//            none). A count and a minimum: independent of the order the blocks ran in.
static constexpr int kR1csMaxBlocks = 2048;
static constexpr int kR1csRecordWords = 14;
static constexpr size_t kR1csRecordStride = 128;  // bytes between the records of a group
struct R1csCheckJob {
    const Fr *az, *bz, *cz;
    uint64_t* partial;
    uint32_t* ticket;
    uint64_t* record;
};
void launch_r1cs_check(int k, const R1csCheckJob* jobs, uint64_t nl, uint64_t row0, hipStream_t s);
// the last levels of an opening in one launch: how many of the `remaining` levels starting at a level
// of `half` pairs it takes (0: none), and the launch (points[j] folds level j; q receives the levels'
// quotients contiguously; `last` the final value)
int open_tail_levels(uint64_t half, int remaining);
// nf (2 or 3) consecutive levels in one launch: nout = the last level's table size; level j's
// quotients go to q + qoffs[j] (~0: not written), points[j] folds level j
void launch_open_fold(const Fr* rin, Fr* rout, Fr* q, int nf, const Fr* points, const uint64_t* qoffs, uint64_t nout,
                      hipStream_t s);
void launch_open_tail(const Fr* rin, Fr* q, uint64_t half, int nlev, const Fr* points, Fr* last, hipStream_t s);

// ---- msm.hip
// One MSM inside a batch. Bases are the PRECOMPUTED window copies of a base set:
// pts[pts_off + w * stride + j] = 2^(c w) * B_j (affine), so every window shares one bucket set.
struct MsmInst {
    uint64_t pts_off;     // first precomputed point of this base set
    uint64_t scalar_off;  // first scalar (Montgomery Fr) in the batch scalar array
    uint32_t size;        // number of (base, scalar) pairs
    uint32_t c, W;        // window bits, windows
    uint32_t stride;      // points per window copy of the base set (>= size)
    // filled in by the MSM driver:
    uint32_t bucket_off;  // first local bucket of this instance
    uint32_t ref_off;     // first (bucket, reference) slot of this instance (dense key layout)
    uint32_t lb;          // log2 of the buckets this rank weights: c - 1 (whole) or c - 1 - lg (split)
    uint32_t lg;          // split: this rank weights buckets u = sel + 2^lg k (u = |digit| - 1); whole: 0
    uint32_t sel;
    uint32_t out;         // output slot (index in the caller's instance list)
};

// Bucket partition of a batch over the ranks of a proof-sharded prove: every rank
// reads ALL scalars of an instance and keeps the digits whose bucket is one of its own, so the
// accumulation, the partial levels and the bucket weighting all divide by the world size. Buckets
// are dealt round-robin (rank r: u = r, r + G, r + 2G, ...): the digits of the top windows, which
// crowd the low buckets (scalars < r < 2^255), spread evenly over the ranks. Rank r's result for an
// instance is sum_{its u} (u + 1) S_u; the ranks' results sum to the MSM. Instances too small to
// split (fewer than 4 buckets per rank) go whole to rank (index mod world).
struct MsmShard {
    int rank = 0, world = 1;
    bool dense = false;  // world > 1: one key slot per (scalar, window), as at world 1 (never overflows)
};
static constexpr uint32_t kMsmOverflow = 1;  // status bit: compacted keys exceeded their capacity
// the other three status words: hot buckets listed / reduced, and the largest number of partials the
// weighting leaf added for one bucket where that exceeds 1 (0: no bucket had more than one)
enum { kMsmStHot = 1, kMsmStReduced = 2, kMsmStLeafMax = 3 };

// buckets one batch may hold: the sort's 2048 bins of <= 2^8 buckets (msm_common.hip); prover.hpp ties
// kMaxLogN to it
static constexpr uint64_t kMsmMaxBuckets = 2048ull << 8;
// The wide window plan: c = 17 takes 15 windows (17 x 15 = 255 bits of an Fr scalar), which holds
// only because the digit pass replaces a scalar above (r - 1) / 2 by its negative and flips the sign
// of its references (msm_common.hip, Digits::fold_half). Every other c takes ceil(256 / c) windows.
static constexpr uint32_t kMsmWideBits = 17, kMsmWideWindows = 15;
static constexpr uint32_t msm_windows(uint32_t c) { return c == kMsmWideBits ? kMsmWideWindows : (256 + c - 1) / c; }
struct MsmWorkspace;  // opaque, owned by the host side (msm.hip)
MsmWorkspace* msm_ws_create();
void msm_ws_destroy(MsmWorkspace* ws);
// the pinned staging of the small per-batch tables: call only after a sync covering the workspace's stream
void msm_ws_staging_reset(MsmWorkspace* ws);
// a batch of this workspace reported kMsmOverflow: raise its compacted-key capacity for later batches
void msm_ws_note_overflow(MsmWorkspace* ws);
// hot-bucket reduction of this workspace's batches: on (the default), or off (listed and counted, then
// left to the weighting leaf: A/B); msm_hot_default: SPX_MSM_HOT=0 -> off, else on
void msm_ws_set_hot(MsmWorkspace* ws, bool on);
bool msm_hot_default();

// bytes of a batch's output buffer: one XYZZ point per instance (G1: 4 x 48 B, G2: 4 x 96 B,
// Montgomery limbs; infinity = all zero), then a 16-byte status word (kMsmOverflow, kMsmSt*)
inline size_t msm_out_bytes(bool g2, int ninst) { return (size_t)ninst * (g2 ? 4 * 96 : 4 * 48) + 16; }
// Enqueues a batch of MSMs on `s` without any host synchronisation. With world > 1 and !dense the
// keys are compacted into a capacity planned from the expected bucket occupancy; if the status word
// reads kMsmOverflow afterwards, the outputs are invalid and the batch must be rerun with dense = true.
void msm_run_g1(MsmWorkspace* ws, const MsmInst* insts_host, int ninst, const G1Slot* pts, const Fr* scalars,
                void* out_dev, hipStream_t s, const MsmShard& sh = MsmShard());
void msm_run_g2(MsmWorkspace* ws, const MsmInst* insts_host, int ninst, const G2Aff* pts, const Fr* scalars,
                void* out_dev, hipStream_t s, const MsmShard& sh = MsmShard());

// PP preprocessing: for each base B_j (raw affine, level array), write the W window copies
// 2^(c w) B_j (affine) to dst[w * count + j]. pair_sum: B_j := raw[2j] + raw[2j+1].
void precompute_windows_g1(const G1Aff* raw, uint64_t count, bool pair_sum, int c, int W, G1Aff* dst, void* tmp,
                           hipStream_t s);
void precompute_windows_g2(const G2Aff* raw, uint64_t count, bool pair_sum, int c, int W, G2Aff* dst, void* tmp,
                           hipStream_t s);
// raw ark-serialize uncompressed points (canonical, flags) -> device affine Montgomery, in place.
// Infinity (flag bit 6) becomes the (0,0) sentinel. err |= 1 on malformed input.
void launch_points_from_bytes_g1(G1Aff* pts, uint64_t n, int* err, hipStream_t s);
void launch_points_from_bytes_g2(G2Aff* pts, uint64_t n, int* err, hipStream_t s);
void launch_points_to_canon_g1(G1Aff* pts, uint64_t n, hipStream_t s);
void launch_points_to_canon_g2(G2Aff* pts, uint64_t n, hipStream_t s);
// keygen: out[i] = scalar_i * base, with table[w * 256 + d] = d * 2^(8 w) * base (affine, 32 windows)
void fixed_base_g1(const G1Aff* table, const Fr* scalars, uint64_t n, G1Aff* out, void* tmp, hipStream_t s);
void fixed_base_g2(const G2Aff* table, const Fr* scalars, uint64_t n, G2Aff* out, void* tmp, hipStream_t s);

// ---- verify_kernels.hip (the batch verifier)
// n ark-serialize compressed points (48 / 96 bytes each, `in` 16-byte aligned) -> affine Montgomery with
// the semantics of host::g1_decompress / g2_decompress (pairing.hpp). ok[j] = 1: accepted (infinity is
// the (0, 0) sentinel); ok[j] = 0: non-canonical x or x^3 + b not a square (the sentinel is stored).
void launch_decompress_g1(const uint8_t* in, uint64_t n, G1Aff* out, uint8_t* ok, hipStream_t s);
void launch_decompress_g2(const uint8_t* in, uint64_t n, G2Aff* out, uint8_t* ok, hipStream_t s);
// out[s] = sum_{seg_off[s] <= i < seg_off[s + 1]} k_i P_i (affine, (0, 0) = infinity) for n affine points
// and n canonical scalars (plain integers below 2^256; the cost follows each scalar's bit length);
// seg_off: nseg + 1 ascending device offsets ending at n. Sentinel points and zero scalars contribute
// nothing. tmp: lincomb_tmp_bytes() of device scratch.
size_t lincomb_tmp_bytes(bool g2, uint64_t n);
void launch_lincomb_g1(const G1Aff* pts, const Fr* scalars, uint64_t n, const uint64_t* seg_off, uint32_t nseg,
                       G1Aff* out, void* tmp, hipStream_t s);
void launch_lincomb_g2(const G2Aff* pts, const Fr* scalars, uint64_t n, const uint64_t* seg_off, uint32_t nseg,
                       G2Aff* out, void* tmp, hipStream_t s);

// ---- subgroup_kernels.hip ("Subgroup membership")
// ok[j] = 1 if pts[j] (affine Montgomery, on the curve, (0, 0) = infinity) is infinity or lies in the
// prime-order subgroup, else 0. One point per lane; at most kSubgroupMaxBlocks blocks of kSubgroupLanes
// lanes, which stride over the rest.
static constexpr uint32_t kSubgroupLanes = 64, kSubgroupMaxBlocks = 4096;
void launch_in_subgroup_g1(const G1Aff* pts, uint64_t n, uint8_t* ok, hipStream_t s);
void launch_in_subgroup_g2(const G2Aff* pts, uint64_t n, uint8_t* ok, hipStream_t s);
// out2[0] += the number of zeros in ok[0 .. n), out2[1] = min(out2[1], the first zero's index)
void launch_ok_scan(const uint8_t* ok, uint64_t n, uint64_t* out2, hipStream_t s);

// ---- pp_kernels.hip ("Public-parameter structure and views")
// pts: the 2^(nv+1) - 2 raw points of an nv-variable parameter, levels contiguous (level i: 2^(nv-i) points,
// affine Montgomery, (0, 0) = infinity). ok[j] = 1 if pair j of the flat array (points 2j, 2j + 1; 2^nv - 1
// pairs) sums to its target: pair b of level i against point b of level i + 1, the last level's only pair
// against `last` (g / h). One pair per lane, blocks of kPPFoldLanes.
static constexpr uint32_t kPPFoldLanes = 64;
void launch_fold_check_g1(const G1Aff* pts, int nv, const G1Aff& last, uint8_t* ok, hipStream_t s);
void launch_fold_check_g2(const G2Aff* pts, int nv, const G2Aff& last, uint8_t* ok, hipStream_t s);
// out[i] = sum_b pts_i[2b + 1] for every level i of the same array, as XYZZ (ZZ = 0: infinity): per level
// odd_sum_blocks(nv) blocks of kPPSumThreads write partials to part (nv * odd_sum_blocks(nv) XYZZ), and a
// second pass of one block per level sums them.
static constexpr uint32_t kPPSumThreads = 256, kPPSumMaxBlocks = 256;
uint32_t odd_sum_blocks(int nv);
void launch_odd_sum_g1(const G1Aff* pts, int nv, G1Xyzz* part, G1Xyzz* out, hipStream_t s);

// ---- pp_codec_kernels.hip ("Compressed public parameters")
// n ark-serialize compressed points (`in` 16-byte aligned) -> out[0 .. n), affine Montgomery, (0, 0) for
// infinity and for a rejected point, with the acceptance of launch_decompress_g1 / _g2. Every rejected
// point j lowers *err (initialised to kCodecNoError) to ((point_base + j) << 2) | reason by one atomic
// minimum: afterwards it names the lowest rejected point. ok: one byte per point as launch_decompress_*,
// or null (the loader wants only the report).
static constexpr unsigned long long kCodecNoError = ~0ull;
static constexpr uint32_t kCodecNotCanonical = 1, kCodecNoPoint = 2;  // reasons
void launch_decompress_bulk_g1(const uint8_t* in, uint64_t n, G1Aff* out, uint64_t point_base, unsigned long long* err,
                               uint8_t* ok, hipStream_t s);
void launch_decompress_bulk_g2(const uint8_t* in, uint64_t n, G2Aff* out, uint64_t point_base, unsigned long long* err,
                               uint8_t* ok, hipStream_t s);
// n affine Montgomery points -> 48 / 96 compressed bytes each (`out` 16-byte aligned), the bytes of
// host::g1_compress / g2_compress
void launch_compress_g1(const G1Aff* in, uint64_t n, uint8_t* out, hipStream_t s);
void launch_compress_g2(const G2Aff* in, uint64_t n, uint8_t* out, hipStream_t s);

}  // namespace spx
