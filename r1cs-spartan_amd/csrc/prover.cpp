// MI355X prover orchestration: the reference's `MLArgumentForR1CS::prove`
// (/root/reference/src/lib.rs:58-146) with the AHP rounds of src/ahp/prover.rs:109-281 run as
// HIP kernels (mle_kernels.hip, msm.hip) and the Fiat-Shamir transcript on the host.
//
// Sharding: G = 2^g ranks own contiguous blocks of the hypercube (top g bits of x
// or y) for the SpMV, eval_on_x and both sumchecks. Variables bind LSB first, so every rank folds
// locally for the first L - g rounds; each round exchanges 3 Fr per rank, and the last g rounds run
// on the gathered G-entry tables. The MSMs (commitment, openings) split every instance by bucket
// range instead (MsmShard, kernels.hpp): z is replicated, every rank folds the opening tables in
// full (HBM-streaming) and weights 1/G of the buckets; each MSM exchanges one XYZZ point per rank.
// Every rank replays the same transcript, so no challenge broadcast.
#include "prover.hpp"
#include "sumcheck_host.hpp"
#include "pairing.hpp"

#include <type_traits>

#include <algorithm>
#include <sys/prctl.h>

#include <chrono>
#include <thread>
#include <cstdlib>
#include <cstring>

namespace spx {

using host::Affine;
using HFr = host::Fr;
using HFq = host::Fq;
using HFq2 = host::Fq2;

// ====================================================================== context
Ctx::Ctx(int dev) : device(dev) {
    // SPX_BLOCKING_SYNC=1: host waits sleep instead of spinning (frees cores for the transcript
    // hashing pool when many proofs are in flight); must precede the device's first use
    static const bool blocking = [] {
        const char* e = getenv("SPX_BLOCKING_SYNC");
        return e && e[0] == '1';
    }();
    if (blocking) (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
    SPX_HIP(hipSetDevice(dev));
    SPX_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    SPX_HIP(hipHostMalloc((void**)&pin, kPinBytes));
    SPX_HIP(hipHostGetDevicePointer((void**)&pin_dev_base, pin, 0));
    SPX_HIP(hipMalloc((void**)&ticket, 64));
    SPX_HIP(hipMemset(ticket, 0, 64));
    msm = msm_ws_create();
    comm.reset(new LocalComm());
}
// SPX_SYNC_POLL_US (see Ctx::wait_stream): 0 = hipStreamSynchronize
static int sync_poll_us() {
    static const int v = [] {
        const char* e = getenv("SPX_SYNC_POLL_US");
        return e ? std::max(0, atoi(e)) : 0;
    }();
    return v;
}
void Ctx::wait_stream(hipStream_t s) {
    const int pu = poll_us.load(std::memory_order_relaxed);
    const int us = pu >= 0 ? pu : sync_poll_us();
    if (us <= 0) {
        SPX_HIP(hipStreamSynchronize(s));
        return;
    }
    // one event per (thread, device): waits on this context from different threads (a prove worker,
    // an uploader) never record or query the same event
    struct TlEvents {
        std::vector<hipEvent_t> ev;
        ~TlEvents() {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
    };
    thread_local TlEvents tl;
    if ((int)tl.ev.size() <= device) tl.ev.resize(device + 1, nullptr);
    hipEvent_t& ev = tl.ev[device];
    if (!ev) SPX_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    SPX_HIP(hipEventRecord(ev, s));
    // sleeps of tens of microseconds, not the default 50 us timer slack on top: the calling thread's
    // slack is lowered for the poll loop and restored after it
    const int old_slack = prctl(PR_GET_TIMERSLACK, 0, 0, 0, 0);
    (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);
    struct Restore {
        int v;
        ~Restore() {
            if (v > 0) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)v, 0, 0, 0);
        }
    } restore{old_slack};
    for (int i = 0;; ++i) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return;
        if (e != hipErrorNotReady) SPX_HIP(e);
        if (i < 4)
            std::this_thread::yield();
        else
            std::this_thread::sleep_for(std::chrono::microseconds(us));
    }
}
void Ctx::ensure_side() {
    if (side) return;
    SPX_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    SPX_HIP(hipEventCreateWithFlags(&side_ev, hipEventDisableTiming));
    msm_side = msm_ws_create();
    set_msm_hot(hot_mode);
}
void Ctx::set_msm_hot(int mode) {
    hot_mode = mode;
    const bool on = mode < 0 ? msm_hot_default() : mode == 1;
    msm_ws_set_hot(msm, on);
    msm_ws_set_hot(msm_side, on);
}
// SPX_SUBGROUP_CHECK=1: contexts check proof points for subgroup membership unless told otherwise
static bool subgroup_check_default() {
    static const bool v = [] {
        const char* e = getenv("SPX_SUBGROUP_CHECK");
        return e && e[0] == '1' && e[1] == 0;
    }();
    return v;
}
bool Ctx::subgroup_check() const { return subgroup_mode < 0 ? subgroup_check_default() : subgroup_mode == 1; }
// SPX_WITNESS_CHECK=1: contexts check every witness they prove unless told otherwise
static bool witness_check_default() {
    static const bool v = [] {
        const char* e = getenv("SPX_WITNESS_CHECK");
        return e && e[0] == '1' && e[1] == 0;
    }();
    return v;
}
bool Ctx::witness_check() const { return witness_check_mode < 0 ? witness_check_default() : witness_check_mode == 1; }
Ctx::~Ctx() {
    (void)hipSetDevice(device);
    if (msm_side) msm_ws_destroy(msm_side);
    if (side_ev) (void)hipEventDestroy(side_ev);
    if (side) (void)hipStreamDestroy(side);
    msm_ws_destroy(msm);
    scratch.release();
    if (ticket) (void)hipFree(ticket);
    if (pin) (void)hipHostFree(pin);
    if (stream) (void)hipStreamDestroy(stream);
}
uint8_t* Ctx::pin_at(size_t off, size_t bytes, size_t region) {
    if (bytes > region || off + region > kPinBytes) throw SpxError(kDevice, "pinned staging region too small");
    return pin + off;
}


// ====================================================================== public parameters
// Pippenger window bits: 16 for >= 2^14 points (c = 18..20 for >= 2^18 and narrower ones for
// 2^14-2^17 measured slower or equal: profiles/r02_ab6_window_bits.jsonl, r02_ab7_window_mid.jsonl).
// From 2^wide_min_log points on: 17 bits, which take 15 windows where 16 bits take 16 (a sixteenth
// fewer mixed additions for twice the buckets; kernels.hpp, kMsmWideBits). wide_min_log 0: never.
// Thresholds 2^16 .. 2^19 and off against the 16-bit build at 2^20, alternating on one box: 2^18 is
// the best, +2.3% (profiles/r07/r07b_ab_wide_thresholds.jsonl).
int window_bits_for(uint64_t size, int wide_min_log) {
    const int k = size ? ilog2(size) : 0;
    if (wide_min_log > 0 && k >= wide_min_log) return (int)kMsmWideBits;
    return k >= 14 ? 16 : std::max(3, k - 2);
}
int windows_for(int c) { return (int)msm_windows((uint32_t)c); }
// SPX_MSM_WIDE_MIN_LOG: log2 of the smallest MSM that takes the wide plan (0: none; otherwise at
// least 8). Read when a public parameter is preprocessed and at the stand-alone MSM entry.
int msm_wide_min_log() {
    const char* e = getenv("SPX_MSM_WIDE_MIN_LOG");
    if (!e || !*e) return kMsmWideMinLogDefault;
    const int v = atoi(e);
    return v <= 0 ? 0 : std::max(v, 8);
}
// Window bits of the G2 levels of an nv-variable public parameter (level i: 2^(nv - i - 1) points).
// All levels of an opening may run as one batch (level 0 included in the level-0 batch mode), and a
// batch holds at most kMsmMaxBuckets buckets: the wide plan goes to the largest levels first and the
// remaining candidates keep 16 bits once another 2^16 buckets would pass the limit.
std::vector<int> g2_window_plan(int nv, int wide_min_log) {
    std::vector<int> c(nv);
    uint64_t buckets = 0;
    for (int i = 0; i < nv; ++i) {
        c[i] = window_bits_for(1ull << (nv - i - 1), 0);
        buckets += 1ull << (c[i] - 1);
    }
    for (int i = 0; i < nv; ++i) {
        const int cw = window_bits_for(1ull << (nv - i - 1), wide_min_log);
        if (cw == c[i]) break;  // smaller levels are below the threshold too
        const uint64_t with = buckets - (1ull << (c[i] - 1)) + (1ull << (cw - 1));
        if (with > kMsmMaxBuckets) break;
        c[i] = cw;
        buckets = with;
    }
    return c;
}

// dst: G2Aff rows, or G1Slot rows (128-byte slots) for G1
template <class A, class D>
static void precompute_level(Ctx& C, const A* raw, uint64_t count, bool pair, int c, int W, D* dst) {
    // chunked to bound the XYZZ temporary: tmp XYZZ [W][chunk] -> affine [W][chunk] -> dst rows (pitch count)
    const uint64_t chunk = std::min<uint64_t>(count, 1ull << 18);
    const size_t xyzz_sz = 2 * sizeof(A);
    DevMem tmp(xyzz_sz * chunk * W), aff(sizeof(A) * chunk * W);
    for (uint64_t j0 = 0; j0 < count; j0 += chunk) {
        const uint64_t cn = std::min(chunk, count - j0);
        const A* src = raw + (pair ? 2 * j0 : j0);
        if constexpr (sizeof(A) == sizeof(G1Aff))
            precompute_windows_g1((const G1Aff*)src, cn, pair, c, W, aff.as<G1Aff>(), tmp.p, C.stream);
        else
            precompute_windows_g2((const G2Aff*)src, cn, pair, c, W, aff.as<G2Aff>(), tmp.p, C.stream);
        if constexpr (sizeof(D) == sizeof(A)) {
            SPX_HIP(hipMemcpy2DAsync(dst + j0, sizeof(A) * count, aff.p, sizeof(A) * cn, sizeof(A) * cn, W,
                                     hipMemcpyDeviceToDevice, C.stream));
        } else {  // one point per slot: a 2-D copy per window, rows = points (pitch 96 -> 128 bytes)
            for (int w = 0; w < W; ++w)
                SPX_HIP(hipMemcpy2DAsync(dst + (uint64_t)w * count + j0, sizeof(D), aff.as<A>() + (uint64_t)w * cn,
                                         sizeof(A), sizeof(A), cn, hipMemcpyDeviceToDevice, C.stream));
        }
    }
    C.sync();
}

void pp_preprocess(Ctx& C, PP& P) {
    const int nv = P.nv;
    const uint64_t n = 1ull << nv;
    const int wide = msm_wide_min_log();
    P.g1_c = window_bits_for(n, wide);
    P.g1_W = windows_for(P.g1_c);
    P.g1_pre = std::make_shared<DevMem>(sizeof(G1Slot) * n * P.g1_W);
    precompute_level(C, P.g1_level(0), n, false, P.g1_c, P.g1_W, P.g1_pre->as<G1Slot>());
    P.g2_off.assign(nv + 1, 0);
    P.g2_c = g2_window_plan(nv, wide);
    P.g2_W.assign(nv, 0);
    uint64_t tot = 0;
    for (int i = 0; i < nv; ++i) {
        uint64_t cnt = 1ull << (nv - i - 1);
        P.g2_W[i] = windows_for(P.g2_c[i]);
        P.g2_off[i] = tot;
        tot += cnt * P.g2_W[i];
    }
    P.g2_off[nv] = tot;
    P.store->g2_pre.alloc(sizeof(G2Aff) * std::max<uint64_t>(tot, 1));
    for (int i = 0; i < nv; ++i) {
        uint64_t cnt = 1ull << (nv - i - 1);
        precompute_level(C, P.g2_level(i), cnt, true, P.g2_c[i], P.g2_W[i], P.store->g2_pre.as<G2Aff>() + P.g2_off[i]);
    }
}

static void pp_alloc_raw(PP& P, int nv, int device) {
    P.nv = nv;
    P.lvl_off.assign(nv + 1, 0);
    uint64_t tot = 0;
    for (int i = 0; i < nv; ++i) {
        P.lvl_off[i] = tot;
        tot += 1ull << (nv - i);
    }
    P.lvl_off[nv] = tot;
    P.store = std::make_shared<PPStore>();
    P.store->device = device;
    P.store->g1_raw_mem.alloc(sizeof(G1Aff) * std::max<uint64_t>(tot, 1));
    P.store->g2_raw_mem.alloc(sizeof(G2Aff) * std::max<uint64_t>(tot, 1));
}

std::unique_ptr<PP> pp_load(Ctx& C, const uint8_t* b, size_t len) {
    auto P = std::make_unique<PP>();
    size_t pos = 0;
    auto need = [&](size_t k) {
        if (pos + k > len) throw SpxError(kSerialization, "truncated public parameter bytes");
    };
    auto u64 = [&]() {
        need(8);
        uint64_t v;
        memcpy(&v, b + pos, 8);
        pos += 8;
        return v;
    };
    uint64_t nv = u64();
    if (nv < 1 || nv > (uint64_t)kMaxLogN) throw SpxError(kSerialization, "bad public parameter nv (1..26 supported)");
    if (u64() != nv) throw SpxError(kSerialization, "powers_of_g length != nv");
    pp_alloc_raw(*P, (int)nv, C.device);
    std::vector<size_t> g1_pos(nv), g2_pos(nv);
    for (uint64_t i = 0; i < nv; ++i) {
        if (u64() != (1ull << (nv - i))) throw SpxError(kSerialization, "powers_of_g level size");
        need(96ull << (nv - i));
        g1_pos[i] = pos;
        pos += 96ull << (nv - i);
    }
    if (u64() != nv) throw SpxError(kSerialization, "powers_of_h length != nv");
    for (uint64_t i = 0; i < nv; ++i) {
        if (u64() != (1ull << (nv - i))) throw SpxError(kSerialization, "powers_of_h level size");
        need(192ull << (nv - i));
        g2_pos[i] = pos;
        pos += 192ull << (nv - i);
    }
    need(96 + 192);
    if (!host::g1_from_uncompressed(P->g, b + pos) || !host::g2_from_uncompressed(P->h, b + pos + 96))
        throw SpxError(kSerialization, "bad g / h");
    for (uint64_t i = 0; i < nv; ++i) {
        SPX_HIP(hipMemcpyAsync(P->g1_level((int)i), b + g1_pos[i], 96ull << (nv - i), hipMemcpyHostToDevice, C.stream));
        SPX_HIP(hipMemcpyAsync(P->g2_level((int)i), b + g2_pos[i], 192ull << (nv - i), hipMemcpyHostToDevice, C.stream));
    }
    DevMem err(sizeof(int));
    SPX_HIP(hipMemsetAsync(err.p, 0, sizeof(int), C.stream));
    launch_points_from_bytes_g1(P->g1_raw(), P->lvl_off[nv], err.as<int>(), C.stream);
    launch_points_from_bytes_g2(P->g2_raw(), P->lvl_off[nv], err.as<int>(), C.stream);
    int herr = 0;
    SPX_HIP(hipMemcpyAsync(&herr, err.p, sizeof(int), hipMemcpyDeviceToHost, C.stream));
    C.sync();
    if (herr & 1) throw SpxError(kSerialization, "non-canonical coordinate in public parameters");
    if (herr & 2) throw SpxError(kSerialization, "public parameter point not on the curve");
    pp_preprocess(C, *P);
    return P;
}

// SplitMix64 (the synthetic-input / keygen PRNG shared with oracle/c/oracle.c)
struct SplitMix64 {
    uint64_t s;
    uint64_t next() {
        s += 0x9E3779B97F4A7C15ULL;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    }
    HFr fr() {
        for (;;) {
            uint64_t c[4] = {next(), next(), next(), next() & 0x7FFFFFFFFFFFFFFFULL};
            if (!HFr::geq_p(c)) return HFr::from_canon(c);
        }
    }
};

template <class F>
static std::vector<Affine<F>> fixed_base_table(const Affine<F>& base) {
    std::vector<host::Jac<F>> jac(32 * 256);
    host::Jac<F> outer = host::jac_from(base);
    for (int w = 0; w < 32; ++w) {
        host::Jac<F> acc = host::jac_inf<F>();
        jac[w * 256] = acc;
        for (int d = 1; d < 256; ++d) {
            acc = host::jac_add(acc, outer);
            jac[w * 256 + d] = acc;
        }
        for (int k = 0; k < 8; ++k) outer = host::jac_dbl(outer);
    }
    std::vector<F> zs(jac.size());
    for (size_t i = 0; i < jac.size(); ++i) zs[i] = jac[i].z;
    host::batch_inverse(zs);
    std::vector<Affine<F>> out(jac.size());
    for (size_t i = 0; i < jac.size(); ++i) {
        if (jac[i].z.is_zero()) {
            out[i] = {F::zero(), F::zero(), true};  // device sentinel (0,0)
            continue;
        }
        F zi2 = zs[i] * zs[i];
        out[i] = {jac[i].x * zi2, jac[i].y * zi2 * zs[i], false};
    }
    return out;
}
template <class F, class A>
static void upload_affine(const std::vector<Affine<F>>& v, A* dst, hipStream_t s) {
    static_assert(sizeof(A) == 2 * sizeof(F), "layout");
    std::vector<A> tmp(v.size());
    for (size_t i = 0; i < v.size(); ++i) {
        memcpy((uint8_t*)&tmp[i], &v[i].x, sizeof(F));
        memcpy((uint8_t*)&tmp[i] + sizeof(F), &v[i].y, sizeof(F));
    }
    SPX_HIP(hipMemcpyAsync(dst, tmp.data(), sizeof(A) * v.size(), hipMemcpyHostToDevice, s));
    SPX_HIP(hipStreamSynchronize(s));
}

std::unique_ptr<PP> pp_generate(Ctx& C, int nv, uint64_t seed) {
    if (nv < 1 || nv > kMaxLogN) invalid("keygen: nv out of range (1..26 supported)");
    auto P = std::make_unique<PP>();
    SplitMix64 rng{seed};
    HFr gs = rng.fr(), hs = rng.fr();
    P->t.resize(nv);
    for (int i = 0; i < nv; ++i) P->t[i] = rng.fr();
    P->has_t = true;
    uint64_t c[4];
    gs.to_canon(c);
    P->g = host::jac_to_affine(host::jac_mul(host::jac_from(host::g1_generator()), c));
    hs.to_canon(c);
    P->h = host::jac_to_affine(host::jac_mul(host::jac_from(host::g2_generator()), c));
    pp_alloc_raw(*P, nv, C.device);
    const uint64_t tot = P->lvl_off[nv];
    // eq(t[i..], x) scalars for every level (setup.rs:37-60), Montgomery
    DevMem tdev(32 * nv), scal(32 * tot), lo(32 << 14), hi(32 << 14);
    SPX_HIP(hipMemcpyAsync(tdev.p, P->t.data(), 32 * nv, hipMemcpyHostToDevice, C.stream));
    for (int i = 0; i < nv; ++i) {
        const EqTableJob job{tdev.as<Fr>() + i, scal.as<Fr>() + P->lvl_off[i], lo.as<Fr>(), hi.as<Fr>()};
        launch_eq_table(1, &job, nv - i, 0, 1ull << (nv - i), C.stream);
    }
    {
        auto tg = fixed_base_table(P->g);
        DevMem tab(sizeof(G1Aff) * tg.size()), tmp(2 * sizeof(G1Aff) * tot);
        upload_affine(tg, tab.as<G1Aff>(), C.stream);
        fixed_base_g1(tab.as<G1Aff>(), scal.as<Fr>(), tot, P->g1_raw(), tmp.p, C.stream);
        C.sync();
    }
    {
        auto th = fixed_base_table(P->h);
        DevMem tab(sizeof(G2Aff) * th.size()), tmp(2 * sizeof(G2Aff) * tot);
        upload_affine(th, tab.as<G2Aff>(), C.stream);
        fixed_base_g2(tab.as<G2Aff>(), scal.as<Fr>(), tot, P->g2_raw(), tmp.p, C.stream);
        C.sync();
    }
    pp_preprocess(C, *P);
    return P;
}

std::vector<uint8_t> pp_serialize(Ctx& C, const PP& P) {
    const int nv = P.nv;
    const uint64_t tot = P.lvl_off[nv];
    size_t need = 8 + 8 + 8 + 96 + 192;
    for (int i = 0; i < nv; ++i) need += 16 + (96 + 192) * (1ull << (nv - i));
    std::vector<uint8_t> out(need);
    DevMem t1(sizeof(G1Aff) * tot), t2(sizeof(G2Aff) * tot);
    SPX_HIP(hipMemcpyAsync(t1.p, P.g1_raw(), sizeof(G1Aff) * tot, hipMemcpyDeviceToDevice, C.stream));
    SPX_HIP(hipMemcpyAsync(t2.p, P.g2_raw(), sizeof(G2Aff) * tot, hipMemcpyDeviceToDevice, C.stream));
    launch_points_to_canon_g1(t1.as<G1Aff>(), tot, C.stream);
    launch_points_to_canon_g2(t2.as<G2Aff>(), tot, C.stream);
    std::vector<uint8_t> h1(sizeof(G1Aff) * tot), h2(sizeof(G2Aff) * tot);
    SPX_HIP(hipMemcpyAsync(h1.data(), t1.p, h1.size(), hipMemcpyDeviceToHost, C.stream));
    SPX_HIP(hipMemcpyAsync(h2.data(), t2.p, h2.size(), hipMemcpyDeviceToHost, C.stream));
    C.sync();
    auto fix_inf = [](uint8_t* p, size_t bytes) {  // (0,0) sentinel -> ark-serialize infinity (x=0, y=1, flag)
        for (size_t k = 0; k < bytes; ++k)
            if (p[k]) return;
        HFq zero = HFq::zero(), one = HFq::one();
        if (bytes == 96) {
            host::fq_to_bytes(p, zero);
            host::fq_to_bytes(p + 48, one, host::kFlagInf);
        } else {
            host::fq_to_bytes(p, zero);
            host::fq_to_bytes(p + 48, zero);
            host::fq_to_bytes(p + 96, one);
            host::fq_to_bytes(p + 144, zero, host::kFlagInf);
        }
    };
    uint8_t* p = out.data();
    uint64_t u = (uint64_t)nv;
    memcpy(p, &u, 8), p += 8;
    memcpy(p, &u, 8), p += 8;
    for (int i = 0; i < nv; ++i) {
        uint64_t k = 1ull << (nv - i);
        memcpy(p, &k, 8), p += 8;
        memcpy(p, h1.data() + 96 * P.lvl_off[i], 96 * k);
        for (uint64_t j = 0; j < k; ++j) fix_inf(p + 96 * j, 96);
        p += 96 * k;
    }
    memcpy(p, &u, 8), p += 8;
    for (int i = 0; i < nv; ++i) {
        uint64_t k = 1ull << (nv - i);
        memcpy(p, &k, 8), p += 8;
        memcpy(p, h2.data() + 192 * P.lvl_off[i], 192 * k);
        for (uint64_t j = 0; j < k; ++j) fix_inf(p + 192 * j, 192);
        p += 192 * k;
    }
    host::g1_to_uncompressed(p, P.g), p += 96;
    host::g2_to_uncompressed(p, P.h), p += 192;
    return out;
}

// ---- the compressed wire form ("Compressed public parameters"): what ark-serialize's
// serialize() / deserialize() write and read. The framing is the uncompressed form's with 48 / 96-byte
// points; the bulk conversion runs on the GPU (pp_codec_kernels.hip) and only compressed bytes cross PCIe.
size_t pp_serialized_size(int nv, bool compressed) {
    if (nv < 1 || nv > kMaxLogN) invalid("nv out of range (1..26 supported)");
    const size_t g1 = compressed ? 48 : 96, pts = (2ull << nv) - 2;
    return 24 + 16 * (size_t)nv + 3 * g1 * pts + 3 * g1;
}
// SPX_PP_STAGE_LOG: log2 of the points per staging chunk of the compressed loader and serializer (default
// 20: a staging buffer of at most 96 MiB, whatever the parameter's size). Read at each call.
static constexpr int kPPStageLogDefault = 20;
static uint64_t pp_stage_points() {
    const char* e = getenv("SPX_PP_STAGE_LOG");
    long v = kPPStageLogDefault;
    if (e && *e) {
        char* end = nullptr;
        const long t = strtol(e, &end, 10);
        if (end != e && *end == 0) v = std::min(std::max(t, 0l), 27l);  // anything but a number: the default
    }
    return 1ull << v;
}
// The 2 tot points of a parameter in the order G1 levels, G2 levels, cut into chunks of at most `chunk`
// points; a chunk is at most one run of G1 points followed by one run of G2 points. fn(first G1 point,
// G1 points, first G2 point, G2 points).
template <class Fn>
static void pp_for_chunks(uint64_t tot, uint64_t chunk, const Fn& fn) {
    for (uint64_t c0 = 0; c0 < 2 * tot; c0 += chunk) {
        const uint64_t c1 = std::min(c0 + chunk, 2 * tot);
        const uint64_t a0 = std::min(c0, tot), a1 = std::min(c1, tot);
        const uint64_t b0 = std::max(c0, tot) - tot, b1 = std::max(c1, tot) - tot;
        fn(a0, a1 - a0, b0, b1 - b0);
    }
}
// Points [p0, p0 + cnt) of one curve, level by level: fn(level, first point within the level, points,
// points of the run before this piece)
template <class Fn>
static void pp_for_level_pieces(const std::vector<uint64_t>& lvl_off, int nv, uint64_t p0, uint64_t cnt, const Fn& fn) {
    uint64_t done = 0;
    for (int i = 0; i < nv && done < cnt; ++i) {
        const uint64_t lo = std::max(p0 + done, lvl_off[i]), hi = std::min(p0 + cnt, lvl_off[i + 1]);
        if (lo >= hi) continue;
        fn(i, lo - lvl_off[i], hi - lo, done);
        done += hi - lo;
    }
}
// 0: host::g1_decompress / g2_decompress accepts the bytes; else the kernels' reason (kernels.hpp)
static uint32_t point_reject_reason(const uint8_t* p, bool g2) {
    host::Fq t;
    if (!host::fq_from_bytes(t, p, nullptr) || (g2 && !host::fq_from_bytes(t, p + 48, nullptr))) return kCodecNotCanonical;
    if (g2) {
        host::Affine<host::Fq2> a;
        return host::g2_decompress(a, p) ? 0 : kCodecNoPoint;
    }
    host::Affine<host::Fq> a;
    return host::g1_decompress(a, p) ? 0 : kCodecNoPoint;
}
static const char* codec_reason(uint32_t r) {
    return r == kCodecNotCanonical ? "x is not canonical" : "no point on the curve with this x";
}

std::unique_ptr<PP> pp_load_compressed(Ctx& C, const uint8_t* b, size_t len) {
    auto P = std::make_unique<PP>();
    size_t pos = 0;
    auto need = [&](size_t k) {
        if (pos + k > len) throw SpxError(kSerialization, "truncated public parameter bytes");
    };
    auto u64 = [&]() {
        need(8);
        uint64_t v;
        memcpy(&v, b + pos, 8);
        pos += 8;
        return v;
    };
    uint64_t nv = u64();
    if (nv < 1 || nv > (uint64_t)kMaxLogN) throw SpxError(kSerialization, "bad public parameter nv (1..26 supported)");
    if (u64() != nv) throw SpxError(kSerialization, "powers_of_g length != nv");
    std::vector<size_t> g1_pos(nv), g2_pos(nv);
    for (uint64_t i = 0; i < nv; ++i) {
        if (u64() != (1ull << (nv - i))) throw SpxError(kSerialization, "powers_of_g level size");
        need(48ull << (nv - i));
        g1_pos[i] = pos;
        pos += 48ull << (nv - i);
    }
    if (u64() != nv) throw SpxError(kSerialization, "powers_of_h length != nv");
    for (uint64_t i = 0; i < nv; ++i) {
        if (u64() != (1ull << (nv - i))) throw SpxError(kSerialization, "powers_of_h level size");
        need(96ull << (nv - i));
        g2_pos[i] = pos;
        pos += 96ull << (nv - i);
    }
    need(48 + 96);
    pp_alloc_raw(*P, (int)nv, C.device);
    const uint64_t tot = P->lvl_off[nv], chunk = pp_stage_points();
    DevMem stage(96 * std::min(chunk, 2 * tot)), err(sizeof(unsigned long long));
    const unsigned long long none = kCodecNoError;
    unsigned long long herr = none;
    SPX_HIP(hipMemcpyAsync(err.p, &none, sizeof(none), hipMemcpyHostToDevice, C.stream));
    uint8_t* const st = stage.as<uint8_t>();
    pp_for_chunks(tot, chunk, [&](uint64_t a0, uint64_t na, uint64_t b0, uint64_t nb) {
        pp_for_level_pieces(P->lvl_off, (int)nv, a0, na, [&](int i, uint64_t first, uint64_t cnt, uint64_t before) {
            SPX_HIP(hipMemcpyAsync(st + 48 * before, b + g1_pos[i] + 48 * first, 48 * cnt, hipMemcpyHostToDevice, C.stream));
        });
        pp_for_level_pieces(P->lvl_off, (int)nv, b0, nb, [&](int i, uint64_t first, uint64_t cnt, uint64_t before) {
            SPX_HIP(hipMemcpyAsync(st + 48 * na + 96 * before, b + g2_pos[i] + 96 * first, 96 * cnt, hipMemcpyHostToDevice,
                                   C.stream));
        });
        launch_decompress_bulk_g1(st, na, P->g1_raw() + a0, a0, err.as<unsigned long long>(), nullptr, C.stream);
        launch_decompress_bulk_g2(st + 48 * na, nb, P->g2_raw() + b0, tot + b0, err.as<unsigned long long>(), nullptr,
                                  C.stream);
    });
    SPX_HIP(hipMemcpyAsync(&herr, err.p, sizeof(herr), hipMemcpyDeviceToHost, C.stream));
    C.sync();
    // the lowest offender in the order G1 levels, G2 levels, g, h
    if (herr != none) {
        const uint64_t pt = herr >> 2;
        const bool g2 = pt >= tot;
        const uint64_t idx = g2 ? pt - tot : pt;
        int lvl = 0;
        while (idx >= P->lvl_off[lvl + 1]) ++lvl;
        throw SpxError(kSerialization, std::string(g2 ? "powers_of_h" : "powers_of_g") + " level " + std::to_string(lvl) +
                                           " point " + std::to_string(idx - P->lvl_off[lvl]) + ": " +
                                           codec_reason((uint32_t)(herr & 3)));
    }
    if (const uint32_t r = point_reject_reason(b + pos, false)) throw SpxError(kSerialization, std::string("g: ") + codec_reason(r));
    if (const uint32_t r = point_reject_reason(b + pos + 48, true)) throw SpxError(kSerialization, std::string("h: ") + codec_reason(r));
    host::g1_decompress(P->g, b + pos);
    host::g2_decompress(P->h, b + pos + 48);
    pp_preprocess(C, *P);
    return P;
}

std::vector<uint8_t> pp_serialize_compressed(Ctx& C, const PP& P) {
    const int nv = P.nv;
    const uint64_t tot = P.lvl_off[nv], chunk = pp_stage_points();
    std::vector<uint8_t> out(pp_serialized_size(nv, true));
    // the framing first: where each level's points go
    std::vector<size_t> g1_pos(nv), g2_pos(nv);
    uint8_t* p = out.data();
    const uint64_t u = (uint64_t)nv;
    memcpy(p, &u, 8), p += 8;
    for (int c = 0; c < 2; ++c) {
        memcpy(p, &u, 8), p += 8;
        for (int i = 0; i < nv; ++i) {
            const uint64_t k = 1ull << (nv - i);
            memcpy(p, &k, 8), p += 8;
            (c ? g2_pos : g1_pos)[i] = (size_t)(p - out.data());
            p += (c ? 96 : 48) * k;
        }
    }
    host::g1_compress(p, P.g), p += 48;
    host::g2_compress(p, P.h), p += 96;
    DevMem stage(96 * std::min(chunk, 2 * tot));
    uint8_t* const st = stage.as<uint8_t>();
    pp_for_chunks(tot, chunk, [&](uint64_t a0, uint64_t na, uint64_t b0, uint64_t nb) {
        launch_compress_g1(P.g1_raw() + a0, na, st, C.stream);
        launch_compress_g2(P.g2_raw() + b0, nb, st + 48 * na, C.stream);
        pp_for_level_pieces(P.lvl_off, nv, a0, na, [&](int i, uint64_t first, uint64_t cnt, uint64_t before) {
            SPX_HIP(hipMemcpyAsync(out.data() + g1_pos[i] + 48 * first, st + 48 * before, 48 * cnt, hipMemcpyDeviceToHost,
                                   C.stream));
        });
        pp_for_level_pieces(P.lvl_off, nv, b0, nb, [&](int i, uint64_t first, uint64_t cnt, uint64_t before) {
            SPX_HIP(hipMemcpyAsync(out.data() + g2_pos[i] + 96 * first, st + 48 * na + 96 * before, 96 * cnt,
                                   hipMemcpyDeviceToHost, C.stream));
        });
    });
    C.sync();
    return out;
}

// ====================================================================== index
static void check_csr(const HostCsr& m, uint64_t n) {
    if (m.n != n) invalid("matrix size is inconsistent with number of constraints");
    if (m.rp.size() != n + 1 || m.rp[0] != 0) invalid("malformed row_ptr");
    for (uint64_t x = 0; x < n; ++x)
        if (m.rp[x + 1] < m.rp[x]) invalid("malformed row_ptr");
    const uint64_t nnz = m.rp[n];
    if (m.col.size() < nnz || m.val.size() < 32 * nnz) invalid("malformed CSR arrays");
    for (uint64_t k = 0; k < nnz; ++k)
        if (m.col[k] >= n) invalid("sparse index out of bound");
}

// upload a rank-local block [lo, lo + cnt) of `ptr`-indexed segments, with long-row chunking
static void upload_sparse(Ctx& C, DevSparse& D, const std::vector<uint64_t>* ptrs, const std::vector<uint32_t>* idxs,
                          const std::vector<uint8_t>* vals, uint64_t lo, uint64_t cnt, int* err_dev) {
    std::vector<LongChunk> chunks;
    std::vector<LongRow> lrows;
    for (int m = 0; m < 3; ++m) {
        const uint64_t base = ptrs[m][lo], end = ptrs[m][lo + cnt], nnz = end - base;
        std::vector<uint64_t> p(cnt + 1);
        for (uint64_t x = 0; x <= cnt; ++x) p[x] = ptrs[m][lo + x] - base;
        D.ptr[m].alloc(8 * (cnt + 1));
        D.idx[m].alloc(4 * std::max<uint64_t>(nnz, 1));
        D.val[m].alloc(32 * std::max<uint64_t>(nnz, 1));
        SPX_HIP(hipMemcpyAsync(D.ptr[m].p, p.data(), 8 * (cnt + 1), hipMemcpyHostToDevice, C.stream));
        if (nnz) {
            SPX_HIP(hipMemcpyAsync(D.idx[m].p, idxs[m].data() + base, 4 * nnz, hipMemcpyHostToDevice, C.stream));
            SPX_HIP(hipMemcpyAsync(D.val[m].p, vals[m].data() + 32 * base, 32 * nnz, hipMemcpyHostToDevice, C.stream));
            launch_to_mont(D.val[m].as<Fr>(), nnz, err_dev, C.stream);
        }
        for (uint64_t x = 0; x < cnt; ++x) {
            if (p[x + 1] - p[x] <= kLongRow) continue;
            LongRow lr{};
            lr.m = (uint32_t)m;
            lr.x = x;
            lr.chunk_begin = (uint32_t)chunks.size();
            for (uint64_t k = p[x]; k < p[x + 1]; k += kChunk) {
                LongChunk ch{};
                ch.m = (uint32_t)m;
                ch.begin = k;
                ch.end = std::min(k + kChunk, p[x + 1]);
                chunks.push_back(ch);
            }
            lr.chunk_end = (uint32_t)chunks.size();
            lrows.push_back(lr);
        }
        C.sync();  // host vectors go out of scope
    }
    D.nchunks = (int)chunks.size();
    D.nlrows = (int)lrows.size();
    if (D.nchunks) {
        D.chunks.alloc(sizeof(LongChunk) * chunks.size());
        D.lrows.alloc(sizeof(LongRow) * lrows.size());
        SPX_HIP(hipMemcpyAsync(D.chunks.p, chunks.data(), sizeof(LongChunk) * chunks.size(), hipMemcpyHostToDevice, C.stream));
        SPX_HIP(hipMemcpyAsync(D.lrows.p, lrows.data(), sizeof(LongRow) * lrows.size(), hipMemcpyHostToDevice, C.stream));
        C.sync();
    }
}

// Rows [lo, lo + cnt) of A, B, C as the column-sorted entry list (kernels.hpp: SpmvSlicedView) when
// every one of them has at most one entry: the entries by column, within a column in (matrix, row)
// order; an empty (row, matrix) is a zero entry whose column is the row (a product of 0 without a
// branch). Returns false, uploading nothing, otherwise (the CSR path then serves the SpMV).
static bool upload_sliced(Ctx& C, DevSliced& S, const HostCsr* mats, uint64_t n, uint64_t lo, uint64_t cnt,
                          int* err_dev) {
    if (n < (1ull << 12)) return false;
    for (int m = 0; m < 3; ++m)
        for (uint64_t x = lo; x < lo + cnt; ++x)
            if (mats[m].rp[x + 1] - mats[m].rp[x] > 1) return false;
    auto col_of = [&](int m, uint64_t x) -> uint32_t {
        const uint64_t k = mats[m].rp[x];
        return mats[m].rp[x + 1] > k ? mats[m].col[k] : (uint32_t)x;
    };
    std::vector<uint64_t> start(n + 1, 0);  // counting sort by column
    for (int m = 0; m < 3; ++m)
        for (uint64_t x = lo; x < lo + cnt; ++x) ++start[col_of(m, x) + 1];
    for (uint64_t c = 0; c < n; ++c) start[c + 1] += start[c];
    const uint64_t E = start[n];
    std::vector<uint32_t> col(E), dst(E);
    std::vector<uint8_t> val(32 * E, 0);
    for (int m = 0; m < 3; ++m)
        for (uint64_t x = lo; x < lo + cnt; ++x) {
            const uint32_t c = col_of(m, x);
            const uint64_t e = start[c]++;
            col[e] = c;
            dst[e] = (uint32_t)(x - lo) | ((uint32_t)m << 30);
            const uint64_t k = mats[m].rp[x];
            if (mats[m].rp[x + 1] > k) memcpy(val.data() + 32 * e, mats[m].val.data() + 32 * k, 32);
        }
    S.val.alloc(32 * E);
    S.col.alloc(4 * E);
    S.dst.alloc(4 * E);
    SPX_HIP(hipMemcpyAsync(S.val.p, val.data(), 32 * E, hipMemcpyHostToDevice, C.stream));
    SPX_HIP(hipMemcpyAsync(S.col.p, col.data(), 4 * E, hipMemcpyHostToDevice, C.stream));
    SPX_HIP(hipMemcpyAsync(S.dst.p, dst.data(), 4 * E, hipMemcpyHostToDevice, C.stream));
    launch_to_mont(S.val.as<Fr>(), E, err_dev, C.stream);
    C.sync();  // host vectors go out of scope
    S.entries = E;
    S.on = true;
    return true;
}

// CSC copy of M for eval_on_x (rows ascending within a column). The reference inserts every
// (xy_combine(x, y), value) pair into a SparseMLExtensionMap (r1cs_reader.rs:98-108), so when a
// row repeats a column only the LAST entry of that row survives; sum_over_y (r1cs_reader.rs:75-85)
// keeps adding every entry, so only this copy drops the superseded ones.
static void build_csc(const HostCsr& M, uint64_t n, std::vector<uint64_t>& cp, std::vector<uint32_t>& rows,
                      std::vector<uint8_t>& vals) {
    const uint64_t nnz = M.rp[n];
    std::vector<uint8_t> dead(nnz, 0);
    std::vector<uint64_t> last_row(n, ~0ull), last_k(n, 0);
    uint64_t live = 0;
    for (uint64_t x = 0; x < n; ++x)
        for (uint64_t k = M.rp[x]; k < M.rp[x + 1]; ++k) {
            const uint32_t y = M.col[k];
            if (last_row[y] == x)
                dead[last_k[y]] = 1;
            else
                ++live;
            last_row[y] = x;
            last_k[y] = k;
        }
    cp.assign(n + 1, 0);
    for (uint64_t k = 0; k < nnz; ++k)
        if (!dead[k]) cp[M.col[k] + 1]++;
    for (uint64_t y = 0; y < n; ++y) cp[y + 1] += cp[y];
    std::vector<uint64_t> cur(cp.begin(), cp.end() - 1);
    rows.assign(live, 0);
    vals.assign(32 * live, 0);
    for (uint64_t x = 0; x < n; ++x)
        for (uint64_t k = M.rp[x]; k < M.rp[x + 1]; ++k) {
            if (dead[k]) continue;
            const uint64_t pos = cur[M.col[k]]++;
            rows[pos] = (uint32_t)x;
            memcpy(&vals[32 * pos], &M.val[32 * k], 32);
        }
}

// The column stream of the rank-local columns [lo, lo + cnt) of (up to) three CSC matrices for
// k_col_stream (kernels.hpp: ColStreamView). A column's entries are A's, then B's, then C's (rows
// ascending); columns are sorted by entry count, longest first, inside windows of 64 kColWindow columns and
// dealt to the lanes of 64-column slices, so a wave's lanes run columns of nearly equal length (the
// per-column loop left lanes of Poisson-length columns idle for most of a wave's steps). Columns with
// more than kLongCol entries take the chunked long path instead.
static void upload_cols(Ctx& C, DevColStream& D, const std::vector<uint64_t>* cps, const std::vector<uint32_t>* rws,
                        const std::vector<uint8_t>* vals, uint64_t lo, uint64_t cnt, int* err_dev) {
    std::vector<uint32_t> len(cnt);
    std::vector<uint64_t> long_cols;
    uint64_t live = 0;
    for (uint64_t y = 0; y < cnt; ++y) {
        uint64_t L = 0;
        for (int m = 0; m < 3; ++m) L += cps[m][lo + y + 1] - cps[m][lo + y];
        live += L;
        len[y] = L > kLongCol ? 0u : (uint32_t)L;
        if (L > kLongCol) long_cols.push_back(y);
    }
    D.entries = live;
    const uint64_t win = 64ull * kColWindow, nslices = (cnt + 63) / 64;
    D.nslices = (uint32_t)nslices;
    std::vector<ColSlice> sl(nslices);
    std::vector<uint32_t> lanes(64 * nslices, kColNone);
    std::vector<uint64_t> order;
    uint64_t tot = 0;
    for (uint64_t w0 = 0; w0 < cnt; w0 += win) {
        const uint64_t wn = std::min(win, cnt - w0);
        order.resize(wn);
        for (uint64_t i = 0; i < wn; ++i) order[i] = w0 + i;
        std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return len[a] > len[b]; });
        for (uint64_t s0 = 0; s0 < wn; s0 += 64) {
            const uint64_t si = (w0 + s0) / 64;
            uint32_t mx = 0;
            for (uint64_t l = 0; l < 64 && s0 + l < wn; ++l) {
                const uint64_t y = order[s0 + l];
                lanes[64 * si + l] = (uint32_t)y | (len[y] << 26);
                mx = std::max(mx, len[y]);
            }
            sl[si].off = tot;
            sl[si].len = mx;
            tot += 64ull * mx;
        }
    }
    std::vector<uint32_t> rowm(std::max<uint64_t>(tot, 1), 0);
    std::vector<uint8_t> val(32 * std::max<uint64_t>(tot, 1), 0);
    for (uint64_t si = 0; si < nslices; ++si)
        for (uint64_t l = 0; l < 64; ++l) {
            const uint32_t info = lanes[64 * si + l];
            if (info == kColNone) continue;
            const uint64_t y = info & 0x3FFFFFFu;
            if (!len[y]) continue;
            uint64_t j = 0;
            for (uint32_t m = 0; m < 3; ++m)
                for (uint64_t k = cps[m][lo + y]; k < cps[m][lo + y + 1]; ++k, ++j) {
                    const uint64_t e = sl[si].off + 64 * j + l;
                    rowm[e] = rws[m][k] | (m << 30);
                    memcpy(&val[32 * e], &vals[m][32 * k], 32);
                }
        }
    D.slices.alloc(sizeof(ColSlice) * std::max<uint64_t>(nslices, 1));
    D.lanes.alloc(4 * std::max<uint64_t>(lanes.size(), 1));
    D.rowm.alloc(4 * rowm.size());
    D.val.alloc(val.size());
    if (nslices) {
        SPX_HIP(hipMemcpyAsync(D.slices.p, sl.data(), sizeof(ColSlice) * nslices, hipMemcpyHostToDevice, C.stream));
        SPX_HIP(hipMemcpyAsync(D.lanes.p, lanes.data(), 4 * lanes.size(), hipMemcpyHostToDevice, C.stream));
    }
    SPX_HIP(hipMemcpyAsync(D.rowm.p, rowm.data(), 4 * rowm.size(), hipMemcpyHostToDevice, C.stream));
    SPX_HIP(hipMemcpyAsync(D.val.p, val.data(), val.size(), hipMemcpyHostToDevice, C.stream));
    launch_to_mont(D.val.as<Fr>(), val.size() / 32, err_dev, C.stream);
    C.sync();  // host vectors go out of scope
    // long columns: per-matrix entry arrays holding only their entries, chunked (k_sparse_chunks)
    std::vector<uint32_t> li[3];
    std::vector<uint8_t> lvv[3];
    std::vector<LongChunk> chunks;
    std::vector<LongRow> lrows;
    for (uint32_t m = 0; m < 3; ++m)
        for (uint64_t y : long_cols) {
            const uint64_t b = cps[m][lo + y], e = cps[m][lo + y + 1];
            if (b == e) continue;
            LongRow lr{};
            lr.m = m;
            lr.x = y;
            lr.chunk_begin = (uint32_t)chunks.size();
            const uint64_t base = li[m].size();
            for (uint64_t k = 0; k < e - b; k += kChunk) {
                LongChunk ch{};
                ch.m = m;
                ch.begin = base + k;
                ch.end = base + std::min<uint64_t>(k + kChunk, e - b);
                chunks.push_back(ch);
            }
            lr.chunk_end = (uint32_t)chunks.size();
            lrows.push_back(lr);
            li[m].insert(li[m].end(), rws[m].begin() + b, rws[m].begin() + e);
            lvv[m].insert(lvv[m].end(), vals[m].begin() + 32 * b, vals[m].begin() + 32 * e);
        }
    DevSparse& L = D.longc;
    for (int m = 0; m < 3; ++m) {
        L.ptr[m].alloc(8);
        L.idx[m].alloc(4 * std::max<size_t>(li[m].size(), 1));
        L.val[m].alloc(std::max<size_t>(lvv[m].size(), 32));
        if (!li[m].empty()) {
            SPX_HIP(hipMemcpyAsync(L.idx[m].p, li[m].data(), 4 * li[m].size(), hipMemcpyHostToDevice, C.stream));
            SPX_HIP(hipMemcpyAsync(L.val[m].p, lvv[m].data(), lvv[m].size(), hipMemcpyHostToDevice, C.stream));
            launch_to_mont(L.val[m].as<Fr>(), li[m].size(), err_dev, C.stream);
        }
    }
    L.nchunks = (int)chunks.size();
    L.nlrows = (int)lrows.size();
    if (L.nchunks) {
        L.chunks.alloc(sizeof(LongChunk) * chunks.size());
        L.lrows.alloc(sizeof(LongRow) * lrows.size());
        SPX_HIP(hipMemcpyAsync(L.chunks.p, chunks.data(), sizeof(LongChunk) * chunks.size(), hipMemcpyHostToDevice, C.stream));
        SPX_HIP(hipMemcpyAsync(L.lrows.p, lrows.data(), sizeof(LongRow) * lrows.size(), hipMemcpyHostToDevice, C.stream));
    }
    C.sync();
}

// sink: update(data, len) of one state or of a group of states absorbing the same bytes
template <class Sink>
static void feed_matrix(Sink&& h, const HostCsr& m) {
    // CanonicalSerialize of MatrixExtension { constraint: Vec<Vec<(F, usize)>>, num_constraints: usize },
    // streamed through a 64 KiB staging block (u64 lengths, then (32-byte Fr, u64 column) per entry)
    constexpr size_t kBlk = 1 << 16;
    alignas(64) uint8_t buf[kBlk];
    size_t len = 0;
    auto put64 = [&](uint64_t v) {
        if (len + 8 > kBlk) h.update(buf, len), len = 0;
        memcpy(buf + len, &v, 8);
        len += 8;
    };
    put64(m.n);
    const uint8_t* val = m.val.data();
    const uint32_t* col = m.col.data();
    for (uint64_t x = 0; x < m.n; ++x) {
        put64(m.rp[x + 1] - m.rp[x]);
        for (uint64_t k = m.rp[x]; k < m.rp[x + 1]; ++k) {
            if (len + 40 > kBlk) h.update(buf, len), len = 0;
            memcpy(buf + len, val + 32 * k, 32);
            const uint64_t c = col[k];
            memcpy(buf + len + 32, &c, 8);
            len += 40;
        }
    }
    put64(m.n);
    h.update(buf, len);
}

Blake2s absorb_matrices(const Index& I) {
    Blake2s h;
    for (int m = 0; m < 3; ++m) feed_matrix(h, I.m[m]);
    return h;
}

void absorb_matrices_lanes(const Index& I, Blake2s* out, int k) {
    for (int l = 0; l < k; ++l) out[l].reset();
    struct Lanes {
        Blake2s* st;
        int k;
        void update(const void* d, size_t n) { blake2s_update_lanes(st, k, d, n); }
    } sink{out, k};
    for (int m = 0; m < 3; ++m) feed_matrix(sink, I.m[m]);
}

bool index_gpu_default() {  // SPX_INDEX_BUILD=gpu: contexts build their indices on the GPU unless told otherwise
    const char* e = getenv("SPX_INDEX_BUILD");
    return e && !strcmp(e, "gpu");
}
bool Ctx::index_gpu() const { return index_mode < 0 ? index_gpu_default() : index_mode == 1; }

namespace {
struct EventPair {  // device time of a stretch of the stream
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() {
        SPX_HIP(hipEventCreate(&a));
        SPX_HIP(hipEventCreate(&b));
    }
    ~EventPair() {
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
    }
    double ms() const {
        float t = 0;
        SPX_HIP(hipEventElapsedTime(&t, a, b));
        return t;
    }
};
double us_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

// The GPU builder ("Index build on the GPU"): the arrays upload_sliced / upload_sparse,
// build_csc and upload_cols make, byte for byte, from one upload of each matrix (row_ptr, col, val; the
// values converted to Montgomery form once) and the kernels of index_kernels.hip. The calling thread
// absorbs A while the sorts run, waits for the slice lengths (the stream's size), queues the fills and
// absorbs B and C beside them. Every host source of a copy (the caller's matrices, the tables below)
// lives until the last sync; the scratch is freed on return.
static void index_build_gpu(Ctx& C, Index& I, const HostCsr* mats, uint64_t n, uint64_t lo, uint64_t nl, int* err_dev) {
    hipStream_t s = C.stream;
    uint64_t base[4] = {0, 0, 0, 0};
    for (int m = 0; m < 3; ++m) base[m + 1] = base[m] + mats[m].rp[n];
    const uint64_t E = base[3];
    if (E >= (1ull << 31)) invalid("the GPU index builder takes fewer than 2^31 matrix entries in all");
    // ---- the one upload
    DevMem rp[3], col(4 * std::max<uint64_t>(E, 1)), val(32 * std::max<uint64_t>(E, 1));
    for (int m = 0; m < 3; ++m) {
        rp[m].alloc(8 * (n + 1));
        SPX_HIP(hipMemcpyAsync(rp[m].p, mats[m].rp.data(), 8 * (n + 1), hipMemcpyHostToDevice, s));
        const uint64_t nnz = base[m + 1] - base[m];
        if (!nnz) continue;
        SPX_HIP(hipMemcpyAsync(col.as<uint32_t>() + base[m], mats[m].col.data(), 4 * nnz, hipMemcpyHostToDevice, s));
        SPX_HIP(hipMemcpyAsync(val.as<uint8_t>() + 32 * base[m], mats[m].val.data(), 32 * nnz, hipMemcpyHostToDevice, s));
    }
    EventPair ev1, ev2;
    SPX_HIP(hipEventRecord(ev1.a, s));
    launch_to_mont(val.as<Fr>(), E, err_dev, s);
    IndexSrc src{};
    for (int m = 0; m < 3; ++m) src.rp[m] = rp[m].as<uint64_t>();
    for (int m = 0; m < 4; ++m) src.base[m] = base[m];
    src.col = col.as<uint32_t>();
    src.val = val.as<Fr>();
    src.n = n;
    bool sliced = n >= (1ull << 12);
    for (int m = 0; m < 3 && sliced; ++m)
        for (uint64_t x = lo; x < lo + nl; ++x)
            if (mats[m].rp[x + 1] - mats[m].rp[x] > 1) {
                sliced = false;
                break;
            }
    // ---- scratch of both sorts and of the CSC
    const uint64_t Es = std::max<uint64_t>(std::max<uint64_t>(E, sliced ? 3 * nl : 0), 1);
    const uint64_t hw = std::max<uint64_t>(index_sort_hist_words(Es), 1);
    DevMem k1(4 * Es), p1(4 * Es), k2(4 * Es), p2(4 * Es), hist(4 * hw);
    DevMem sums(4 * index_scan_scratch(std::max(hw, E + 1)));
    std::vector<LongChunk> chunks;  // rows' long tables (CSR path)
    std::vector<LongRow> lrows;
    if (sliced) {
        DevSliced& S = I.rows_sliced;
        const uint64_t Er = 3 * nl;
        launch_index_sliced_keys(src, lo, nl, k1.as<uint32_t>(), p1.as<uint32_t>(), s);
        const int side = launch_index_sort(k1.as<uint32_t>(), p1.as<uint32_t>(), k2.as<uint32_t>(), p2.as<uint32_t>(), Er,
                                           I.log_n, hist.as<uint32_t>(), sums.as<uint32_t>(), s);
        S.val.alloc(32 * Er);
        S.col.alloc(4 * Er);
        S.dst.alloc(4 * Er);
        launch_index_sliced_fill(src, lo, nl, (side ? k2 : k1).as<uint32_t>(), (side ? p2 : p1).as<uint32_t>(),
                                 S.val.as<Fr>(), S.col.as<uint32_t>(), S.dst.as<uint32_t>(), s);
        S.entries = Er;
        S.on = true;
    } else {
        DevSparse& D = I.rows;
        for (int m = 0; m < 3; ++m) {
            const std::vector<uint64_t>& r = mats[m].rp;
            const uint64_t b0 = r[lo], nnz = r[lo + nl] - b0;
            D.ptr[m].alloc(8 * (nl + 1));
            D.idx[m].alloc(4 * std::max<uint64_t>(nnz, 1));
            D.val[m].alloc(32 * std::max<uint64_t>(nnz, 1));
            launch_index_rebase(src.rp[m], lo, nl, D.ptr[m].as<uint64_t>(), s);
            if (nnz) {
                SPX_HIP(hipMemcpyAsync(D.idx[m].p, src.col + base[m] + b0, 4 * nnz, hipMemcpyDeviceToDevice, s));
                SPX_HIP(hipMemcpyAsync(D.val[m].p, src.val + base[m] + b0, 32 * nnz, hipMemcpyDeviceToDevice, s));
            }
            for (uint64_t x = 0; x < nl; ++x) {
                const uint64_t b = r[lo + x] - b0, e = r[lo + x + 1] - b0;
                if (e - b <= kLongRow) continue;
                LongRow lr{};
                lr.m = (uint32_t)m;
                lr.x = x;
                lr.chunk_begin = (uint32_t)chunks.size();
                for (uint64_t k = b; k < e; k += kChunk) {
                    LongChunk ch{};
                    ch.m = (uint32_t)m;
                    ch.begin = k;
                    ch.end = std::min(k + kChunk, e);
                    chunks.push_back(ch);
                }
                lr.chunk_end = (uint32_t)chunks.size();
                lrows.push_back(lr);
            }
        }
        D.nchunks = (int)chunks.size();
        D.nlrows = (int)lrows.size();
        if (D.nchunks) {
            D.chunks.alloc(sizeof(LongChunk) * chunks.size());
            D.lrows.alloc(sizeof(LongRow) * lrows.size());
            SPX_HIP(hipMemcpyAsync(D.chunks.p, chunks.data(), sizeof(LongChunk) * chunks.size(), hipMemcpyHostToDevice, s));
            SPX_HIP(hipMemcpyAsync(D.lrows.p, lrows.data(), sizeof(LongRow) * lrows.size(), hipMemcpyHostToDevice, s));
        }
    }
    // ---- CSC of the whole matrices: entries sorted by column (stable: A, B, C, rows ascending, a row's
    // entries in their order), the superseded ones dropped, then the local columns' pointers
    if (E) SPX_HIP(hipMemcpyAsync(k1.p, col.p, 4 * E, hipMemcpyDeviceToDevice, s));
    launch_index_iota(p1.as<uint32_t>(), E, s);
    const int side = launch_index_sort(k1.as<uint32_t>(), p1.as<uint32_t>(), k2.as<uint32_t>(), p2.as<uint32_t>(), E,
                                       I.log_n, hist.as<uint32_t>(), sums.as<uint32_t>(), s);
    const uint32_t *skey = (side ? k2 : k1).as<uint32_t>(), *spay = (side ? p2 : p1).as<uint32_t>();
    uint32_t *ckey = (side ? k1 : k2).as<uint32_t>(), *cpay = (side ? p1 : p2).as<uint32_t>();
    DevMem rowm(4 * std::max<uint64_t>(E, 1)), crowm(4 * std::max<uint64_t>(E, 1)), pos(4 * (E + 1)), cpl(4 * (3 * nl + 1));
    launch_index_csc(src, skey, spay, E, rowm.as<uint32_t>(), pos.as<uint32_t>(), sums.as<uint32_t>(), ckey,
                     crowm.as<uint32_t>(), cpay, s);
    launch_index_col_ptr(ckey, crowm.as<uint32_t>(), pos.as<uint32_t>() + E, lo, nl, cpl.as<uint32_t>(), s);
    // ---- column stream: the windows' lane words and slice lengths, then (sizes known) the entry slots
    DevColStream& D = I.cols;
    const uint64_t nslices = (nl + 63) / 64;
    D.nslices = (uint32_t)nslices;
    D.slices.alloc(sizeof(ColSlice) * nslices);
    D.lanes.alloc(4 * 64 * nslices);
    DevMem slen(4 * nslices), nlong_dev(4);
    SPX_HIP(hipMemsetAsync(D.lanes.p, 0xFF, 4 * 64 * nslices, s));
    SPX_HIP(hipMemsetAsync(nlong_dev.p, 0, 4, s));
    launch_index_col_window(cpl.as<uint32_t>(), nl, D.lanes.as<uint32_t>(), slen.as<uint32_t>(), nlong_dev.as<uint32_t>(), s);
    SPX_HIP(hipEventRecord(ev1.b, s));
    std::vector<uint32_t> h_slen(nslices), h_cpl;
    uint32_t h_nlong = 0, h_cp[2] = {0, 0};
    SPX_HIP(hipMemcpyAsync(h_slen.data(), slen.p, 4 * nslices, hipMemcpyDeviceToHost, s));
    SPX_HIP(hipMemcpyAsync(&h_nlong, nlong_dev.p, 4, hipMemcpyDeviceToHost, s));
    SPX_HIP(hipMemcpyAsync(&h_cp[0], cpl.p, 4, hipMemcpyDeviceToHost, s));
    SPX_HIP(hipMemcpyAsync(&h_cp[1], cpl.as<uint32_t>() + 3 * nl, 4, hipMemcpyDeviceToHost, s));
    auto t0 = std::chrono::steady_clock::now();
    feed_matrix(I.cache, mats[0]);
    I.absorb_us += us_since(t0);
    C.sync();
    if (h_nlong) {  // long columns are rare: only then do the local column pointers come back
        h_cpl.resize(3 * nl + 1);
        SPX_HIP(hipMemcpyAsync(h_cpl.data(), cpl.p, 4 * (3 * nl + 1), hipMemcpyDeviceToHost, s));
        C.sync();
    }
    D.entries = h_cp[1] - h_cp[0];
    I.long_cols = h_nlong;
    std::vector<ColSlice> sl(nslices);
    uint64_t tot = 0;
    for (uint64_t si = 0; si < nslices; ++si) {
        sl[si].off = tot;
        sl[si].len = h_slen[si];
        sl[si].pad = 0;
        tot += 64ull * h_slen[si];
    }
    D.rowm.alloc(4 * std::max<uint64_t>(tot, 1));
    D.val.alloc(32 * std::max<uint64_t>(tot, 1));
    SPX_HIP(hipEventRecord(ev2.a, s));
    SPX_HIP(hipMemcpyAsync(D.slices.p, sl.data(), sizeof(ColSlice) * nslices, hipMemcpyHostToDevice, s));
    SPX_HIP(hipMemsetAsync(D.rowm.p, 0, D.rowm.bytes, s));
    SPX_HIP(hipMemsetAsync(D.val.p, 0, D.val.bytes, s));
    launch_index_stream_fill(D.slices.as<ColSlice>(), D.lanes.as<uint32_t>(), nslices, cpl.as<uint32_t>(),
                             crowm.as<uint32_t>(), cpay, src.val, D.rowm.as<uint32_t>(), D.val.as<Fr>(), s);
    // long columns: per-matrix entry arrays holding only their entries, chunked (as upload_cols)
    std::vector<LongChunk> lchunks;
    std::vector<LongRow> llrows;
    uint64_t lcount[3] = {0, 0, 0};
    if (h_nlong)
        for (uint32_t m = 0; m < 3; ++m)
            for (uint64_t y = 0; y < nl; ++y) {
                if (h_cpl[3 * y + 3] - h_cpl[3 * y] <= kLongCol) continue;
                const uint64_t cnt = h_cpl[3 * y + m + 1] - h_cpl[3 * y + m];
                if (!cnt) continue;
                LongRow lr{};
                lr.m = m;
                lr.x = y;
                lr.chunk_begin = (uint32_t)lchunks.size();
                for (uint64_t k = 0; k < cnt; k += kChunk) {
                    LongChunk ch{};
                    ch.m = m;
                    ch.begin = lcount[m] + k;
                    ch.end = lcount[m] + std::min<uint64_t>(k + kChunk, cnt);
                    lchunks.push_back(ch);
                }
                lr.chunk_end = (uint32_t)lchunks.size();
                llrows.push_back(lr);
                lcount[m] += cnt;
            }
    DevSparse& L = D.longc;
    IndexLongOut lout{};
    for (int m = 0; m < 3; ++m) {
        L.ptr[m].alloc(8);
        L.idx[m].alloc(4 * std::max<uint64_t>(lcount[m], 1));
        L.val[m].alloc(32 * std::max<uint64_t>(lcount[m], 1));
        lout.idx[m] = L.idx[m].as<uint32_t>();
        lout.val[m] = L.val[m].as<Fr>();
    }
    L.nchunks = (int)lchunks.size();
    L.nlrows = (int)llrows.size();
    if (L.nchunks) {
        L.chunks.alloc(sizeof(LongChunk) * lchunks.size());
        L.lrows.alloc(sizeof(LongRow) * llrows.size());
        SPX_HIP(hipMemcpyAsync(L.chunks.p, lchunks.data(), sizeof(LongChunk) * lchunks.size(), hipMemcpyHostToDevice, s));
        SPX_HIP(hipMemcpyAsync(L.lrows.p, llrows.data(), sizeof(LongRow) * llrows.size(), hipMemcpyHostToDevice, s));
        launch_index_long_fill(L.lrows.as<LongRow>(), L.nlrows, L.chunks.as<LongChunk>(), cpl.as<uint32_t>(),
                               crowm.as<uint32_t>(), cpay, src.val, lout, s);
    }
    SPX_HIP(hipEventRecord(ev2.b, s));
    t0 = std::chrono::steady_clock::now();
    feed_matrix(I.cache, mats[1]);
    feed_matrix(I.cache, mats[2]);
    I.absorb_us += us_since(t0);
    C.sync();
    I.build_kernel_us = 1000.0 * (ev1.ms() + ev2.ms());
}

std::unique_ptr<Index> index_build(Ctx& C, const HostCsr* mats) {
    auto I = std::make_unique<Index>();
    const uint64_t n = mats[0].n;
    if (!is_pow2(n)) invalid("Matrix width should be a power of 2.");  // indexer.rs:49-51
    if (n < 2) invalid("at least 2 constraints are required");
    if (n > (1ull << kMaxLogN)) invalid("more than 2^26 constraints are not supported");
    for (int m = 0; m < 3; ++m) check_csr(mats[m], n);
    I->n = n;
    I->log_n = ilog2(n);
    for (int m = 0; m < 3; ++m) I->m[m] = mats[m];
    const int G = C.comm->size(), rank = C.comm->rank();
    if (!is_pow2((uint64_t)G) || (uint64_t)G > n / 2) invalid("world size must be a power of two <= n / 2");
    I->G = G;
    I->rank = rank;
    const uint64_t nl = n / G, lo = (uint64_t)rank * nl;
    DevMem err(sizeof(int));
    SPX_HIP(hipMemsetAsync(err.p, 0, sizeof(int), C.stream));
    const bool gpu = C.index_gpu();
    I->builder = gpu ? 1 : 0;
    if (gpu) {
        index_build_gpu(C, *I, mats, n, lo, nl, err.as<int>());
    } else {
        // rows (CSR) for sum_over_y
        std::vector<uint64_t> rps[3];
        std::vector<uint32_t> cols[3];
        std::vector<uint8_t> vals[3];
        for (int m = 0; m < 3; ++m) rps[m] = mats[m].rp;
        if (!upload_sliced(C, I->rows_sliced, mats, n, lo, nl, err.as<int>())) {
            const std::vector<uint32_t>* ci[3] = {&mats[0].col, &mats[1].col, &mats[2].col};
            const std::vector<uint8_t>* vi[3] = {&mats[0].val, &mats[1].val, &mats[2].val};
            std::vector<uint32_t> c3[3];
            std::vector<uint8_t> v3[3];
            for (int m = 0; m < 3; ++m) c3[m] = *ci[m], v3[m] = *vi[m];
            upload_sparse(C, I->rows, rps, c3, v3, lo, nl, err.as<int>());
        }
        // columns (CSC, last entry of a repeated (x, y) kept) for eval_on_x
        for (int m = 0; m < 3; ++m) build_csc(mats[m], n, rps[m], cols[m], vals[m]);
        upload_cols(C, I->cols, rps, cols, vals, lo, nl, err.as<int>());
        for (uint64_t y = 0; y < nl; ++y) {  // spx_index_stats: columns on the long path
            uint64_t L = 0;
            for (int m = 0; m < 3; ++m) L += rps[m][lo + y + 1] - rps[m][lo + y];
            I->long_cols += L > kLongCol;
        }
    }
    {
        double e_rows = 0;
        for (int m = 0; m < 3; ++m) e_rows += (double)(mats[m].rp[lo + nl] - mats[m].rp[lo]);
        I->row_entries = I->rows_sliced.on ? I->rows_sliced.entries : (uint64_t)e_rows;
        if (I->rows_sliced.on) {
            // column-sorted list: 40 B per entry (value, column, row | matrix), z read once (each XCD
            // its contiguous eighth), one 32 B output per local row and matrix
            I->rows_index_bytes = 40.0 * (double)I->rows_sliced.entries;
            I->rows_bytes = I->rows_index_bytes + 32.0 * n + 3.0 * 32.0 * nl;
        } else {  // CSR: value + column + a 32 B gather of z per entry, row pointers, 3 outputs
            I->rows_index_bytes = 36.0 * e_rows + 3.0 * 8.0 * nl;
            I->rows_bytes = 68.0 * e_rows + 3.0 * 8.0 * nl + 3.0 * 32.0 * nl;
        }
        // column stream: 32 B value + 4 B row|matrix per entry (eq(r_x) is gathered from its two
        // cache-resident factor tables, not from HBM); 4 B lane word and one 32 B output per column
        I->cols_bytes = 36.0 * (double)I->cols.entries + 4.0 * nl + 32.0 * nl;
    }
    int herr = 0;
    SPX_HIP(hipMemcpyAsync(&herr, err.p, sizeof(int), hipMemcpyDeviceToHost, C.stream));
    C.sync();
    if (herr) throw SpxError(kSerialization, "non-canonical field element in matrix");
    // witness-independent transcript prefix (lib.rs:61-64), absorbed once (the GPU builder did, beside its kernels)
    if (!gpu) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int m = 0; m < 3; ++m) feed_matrix(I->cache, mats[m]);
        I->absorb_us = us_since(t0);
    } else {
        C.timings.clear();
        C.timings.emplace_back("index_gpu_kernels", I->build_kernel_us);
    }
    I->has_cache = true;
    return I;
}

std::vector<uint8_t> index_export(const Index& I, int part) {
    enum { kPtr = 0, kIdx = 3, kVal = 6, kChunks = 9, kLrows, kSVal, kSCol, kSDst, kSlices, kLanes, kRowm, kCVal,
           kLIdx = 18, kLVal = 21, kLChunks = 24, kLLrows, kCount };
    if (part < 0 || part >= kCount) invalid("no such index part");
    const uint64_t nl = I.n / I.G, lo = (uint64_t)I.rank * nl;
    auto fetch = [](const DevMem& d, uint64_t bytes) {
        std::vector<uint8_t> out(bytes);
        if (bytes) SPX_HIP(hipMemcpy(out.data(), d.p, bytes, hipMemcpyDeviceToHost));
        return out;
    };
    auto chunks_of = [&](const DevSparse& D) {
        std::vector<LongChunk> ch(D.nchunks);
        if (D.nchunks) SPX_HIP(hipMemcpy(ch.data(), D.chunks.p, sizeof(LongChunk) * ch.size(), hipMemcpyDeviceToHost));
        return ch;
    };
    const bool csr = I.rows.ptr[0].p != nullptr;
    if (part < kChunks) {
        const int m = part % 3;
        const uint64_t nnz = I.m[m].rp[lo + nl] - I.m[m].rp[lo];
        if (!csr) return {};
        if (part < kIdx) return fetch(I.rows.ptr[m], 8 * (nl + 1));
        return part < kVal ? fetch(I.rows.idx[m], 4 * nnz) : fetch(I.rows.val[m], 32 * nnz);
    }
    switch (part) {
        case kChunks: return fetch(I.rows.chunks, sizeof(LongChunk) * (uint64_t)I.rows.nchunks);
        case kLrows: return fetch(I.rows.lrows, sizeof(LongRow) * (uint64_t)I.rows.nlrows);
        case kSVal: return fetch(I.rows_sliced.val, I.rows_sliced.on ? 32 * I.rows_sliced.entries : 0);
        case kSCol: return fetch(I.rows_sliced.col, I.rows_sliced.on ? 4 * I.rows_sliced.entries : 0);
        case kSDst: return fetch(I.rows_sliced.dst, I.rows_sliced.on ? 4 * I.rows_sliced.entries : 0);
        case kSlices: return fetch(I.cols.slices, sizeof(ColSlice) * (uint64_t)I.cols.nslices);
        case kLanes: return fetch(I.cols.lanes, 4 * 64 * (uint64_t)I.cols.nslices);
        case kRowm:
        case kCVal: {  // entry slots: up to the end of the last slice
            uint64_t tot = 0;
            if (I.cols.nslices) {
                ColSlice last{};
                SPX_HIP(hipMemcpy(&last, I.cols.slices.as<ColSlice>() + (I.cols.nslices - 1), sizeof last, hipMemcpyDeviceToHost));
                tot = last.off + 64ull * last.len;
            }
            return part == kRowm ? fetch(I.cols.rowm, 4 * tot) : fetch(I.cols.val, 32 * tot);
        }
        case kLChunks: return fetch(I.cols.longc.chunks, sizeof(LongChunk) * (uint64_t)I.cols.longc.nchunks);
        case kLLrows: return fetch(I.cols.longc.lrows, sizeof(LongRow) * (uint64_t)I.cols.longc.nlrows);
        default: break;
    }
    const uint32_t m = (uint32_t)(part - kLIdx) % 3;  // a matrix's long-column entries end with its last chunk
    uint64_t cnt = 0;
    for (const LongChunk& ch : chunks_of(I.cols.longc))
        if (ch.m == m) cnt = std::max(cnt, ch.end);
    return part < kLVal ? fetch(I.cols.longc.idx[m], 4 * cnt) : fetch(I.cols.longc.val[m], 32 * cnt);
}

std::unique_ptr<Witness> witness_upload(Ctx& C, const uint8_t* v, size_t nv, const uint8_t* w, size_t nw) {
    if (!is_pow2(nv)) invalid("public input should be power of two");  // prover.rs:114-116
    auto W = std::make_unique<Witness>();
    W->n = nv + nw;
    W->v.assign(v, v + 32 * nv);
    W->z.alloc(32 * std::max<uint64_t>(W->n, 1));
    SPX_HIP(hipMemcpyAsync(W->z.p, v, 32 * nv, hipMemcpyHostToDevice, C.stream));
    if (nw) SPX_HIP(hipMemcpyAsync(W->z.as<uint8_t>() + 32 * nv, w, 32 * nw, hipMemcpyHostToDevice, C.stream));
    DevMem err(sizeof(int));
    SPX_HIP(hipMemsetAsync(err.p, 0, sizeof(int), C.stream));
    launch_to_mont(W->z.as<Fr>(), W->n, err.as<int>(), C.stream);
    int herr = 0;
    SPX_HIP(hipMemcpyAsync(&herr, err.p, sizeof(int), hipMemcpyDeviceToHost, C.stream));
    C.sync();
    if (herr) throw SpxError(kSerialization, "non-canonical field element in witness");
    return W;
}

// ====================================================================== prove helpers
// (Ser, ld_hfr, eq1, quad_at and both sumchecks' host halves: sumcheck_host.hpp)
static Fr dev_fr(const HFr& x) {  // host Fr -> device Fr (same Montgomery bytes), e.g. a kernel argument
    Fr r;
    memcpy(&r, x.v, 32);
    return r;
}

size_t proof_size(int L) {
    const size_t open = 32 + 96 + 8 + 96 * (size_t)L;
    return 56 + open + 16 + 8 + (size_t)L * (8 + 32 * (size_t)(L + 3)) + 96 + 16 + 8 + (size_t)L * (8 + 96) + open;
}

struct Timer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double us() const {
        return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
};

// Host CPU of the proving threads by phase, process-wide (spx_host_phase_stats): the calling thread's
// CPU time (CLOCK_THREAD_CPUTIME_ID) between prove()'s phase marks, with the wall time and the count.
// A rank of a G-rank proof replays the whole transcript and host arithmetic of every proof while its
// device work is 1/G, so this host work is what does not divide when proofs are sharded.
static uint64_t thread_cpu_ns() {
    timespec ts;
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}
static const char* const kPhaseNames[kHostPhases] = {"transcript_matrices", "commit", "open_rv", "sumcheck1",
                                                     "eval_on_x", "sumcheck2", "open_ry"};
static std::atomic<uint64_t> g_phase_cpu[kHostPhases], g_phase_wall[kHostPhases], g_phase_cnt[kHostPhases];
void host_phase_stats(uint64_t* out) {  // [phase][cpu ns, wall ns, count]
    for (int i = 0; i < kHostPhases; ++i) {
        out[3 * i] = g_phase_cpu[i].load();
        out[3 * i + 1] = g_phase_wall[i].load();
        out[3 * i + 2] = g_phase_cnt[i].load();
    }
}

// device MSM output (XYZZ, R = 2^384 Montgomery limbs) -> host Jacobian without an inversion:
// Z = ZZ ZZZ, X = x Z^2 = X ZZ ZZZ^2, Y = y Z^3 = Y ZZ^3 ZZZ^2 (ZZ = 0: infinity)
template <class F>
static host::Jac<F> xyzz_bytes_to_jac(const uint8_t* p) {
    F X, Y, ZZ, ZZZ;
    memcpy(&X, p, sizeof(F));
    memcpy(&Y, p + sizeof(F), sizeof(F));
    memcpy(&ZZ, p + 2 * sizeof(F), sizeof(F));
    memcpy(&ZZZ, p + 3 * sizeof(F), sizeof(F));
    if (ZZ.is_zero()) return host::jac_inf<F>();
    const F z3s = ZZZ * ZZZ;
    return {X * ZZ * z3s, Y * (ZZ * ZZ * ZZ) * z3s, ZZ * ZZZ};
}
template <class F>
static std::vector<Affine<F>> jac_to_affine_batch(const std::vector<host::Jac<F>>& v) {
    std::vector<F> zi(v.size());
    for (size_t k = 0; k < v.size(); ++k) zi[k] = v[k].z;
    host::batch_inverse(zi);
    std::vector<Affine<F>> out(v.size());
    for (size_t k = 0; k < v.size(); ++k) {
        if (v[k].z.is_zero()) {
            out[k] = {F::zero(), F::one(), true};
            continue;
        }
        const F z2 = zi[k] * zi[k];
        out[k] = {v[k].x * z2, v[k].y * z2 * zi[k], false};
    }
    return out;
}

// Outputs of an MSM batch (`cnt` instances, this rank's bucket ranges) -> the affine MSM results:
// every rank's partial of every instance, gathered over the communicator and summed.
template <class F>
static std::vector<Affine<F>> msm_results(Comm& comm, const uint8_t* xyzz, int cnt) {
    const size_t psz = 4 * sizeof(F);
    const int G = comm.size();
    std::vector<uint8_t> all;
    const uint8_t* src = xyzz;
    if (G > 1) {
        all.resize(psz * cnt * G);
        comm.allgather(xyzz, all.data(), psz * cnt);
        src = all.data();
    }
    std::vector<host::Jac<F>> sum(cnt, host::jac_inf<F>());
    for (int r = 0; r < G; ++r)
        for (int k = 0; k < cnt; ++k) sum[k] = host::jac_add(sum[k], xyzz_bytes_to_jac<F>(src + psz * ((size_t)r * cnt + k)));
    return jac_to_affine_batch(sum);
}

static uint32_t msm_status(const uint8_t* h, bool g2, int cnt) {
    uint32_t st;
    memcpy(&st, h + msm_out_bytes(g2, cnt) - 16, 4);
    return st;
}

// the skew words of a finished batch (not one that is about to rerun dense) into the context's totals
static void msm_skew_fold(Ctx& C, const uint8_t* h, bool g2, int cnt) {
    uint32_t st[4];
    memcpy(st, h + msm_out_bytes(g2, cnt) - 16, 16);
    ++C.skew_batches;
    if (st[kMsmStHot]) ++C.skew_hot_batches;
    C.skew_reduced += st[kMsmStReduced];
    const uint64_t leaf = st[kMsmStLeafMax] ? st[kMsmStLeafMax] : 1;  // the word is written only past 1
    uint64_t cur = C.skew_leaf_max.load();
    while (cur < leaf && !C.skew_leaf_max.compare_exchange_weak(cur, leaf)) {
    }
}

static MsmShard shard_of(const Comm& comm) {
    MsmShard sh;
    sh.rank = comm.rank();
    sh.world = comm.size();
    return sh;
}

static std::vector<HFr> allgather_fr(Comm& comm, const std::vector<HFr>& mine) {
    const int G = comm.size();
    std::vector<HFr> all(mine.size() * G);
    comm.allgather(mine.data(), all.data(), sizeof(HFr) * mine.size());
    return all;
}

// ---------------------------------------------------------------- commit (commit.rs:17-29)
// Split in two so the MSM runs while the host absorbs the matrices into the transcript: launch
// enqueues the MSM and the copy of its XYZZ result into pinned memory; finish waits and decodes.
// Proof-sharded (world > 1): every rank holds all of z and weights its range of the buckets.
static void commit_launch(Ctx& C, PP& P, const Fr* z, uint64_t n, const MsmShard& sh) {
    MsmInst inst{};
    inst.pts_off = 0;
    inst.stride = (uint32_t)n;
    inst.scalar_off = 0;
    inst.size = (uint32_t)n;
    inst.c = (uint32_t)P.g1_c;
    inst.W = (uint32_t)P.g1_W;
    const size_t ob = msm_out_bytes(false, 1);
    void* out = C.buf(Ctx::kSlotCommit, ob);
    msm_run_g1(C.msm, &inst, 1, P.g1_tab(), z, out, C.stream, sh);
    SPX_HIP(hipMemcpyAsync(C.pin_at(Ctx::kPinCommit, ob, 2 << 10), out, ob, hipMemcpyDeviceToHost, C.stream));
}
static Affine<HFq> commit_finish(Ctx& C, PP& P, const Fr* z, uint64_t n, Comm& comm) {
    C.sync();
    const uint8_t* h = C.pin_at(Ctx::kPinCommit, msm_out_bytes(false, 1), 2 << 10);
    if (msm_status(h, false, 1) & kMsmOverflow) {  // compacted keys overflowed: once more with a slot per digit
        msm_ws_note_overflow(C.msm);
        ++C.msm_reruns;
        MsmShard sh = shard_of(comm);
        sh.dense = true;
        commit_launch(C, P, z, n, sh);
        C.sync();
    }
    msm_skew_fold(C, h, false, 1);
    return msm_results<HFq>(comm, h, 1)[0];
}

// ---------------------------------------------------------------- level 0 of both openings
// open.rs:37-49 at i = 0 reads only the table itself: q_L[b] = z[2b+1] - z[2b] does not depend on
// the opening point, so pi_0 = MSM(powers_of_h[0], q_L) is the same group element in the opening at
// (r_v, 0..0) (prover.rs:152) and in the one at r_y (prover.rs:275). It is computed once per proof,
// launched right behind the commitment (before any challenge exists, overlapping the host's
// absorption of the matrices) and handed to both open_z calls: a quarter of the proof's G2 work.
// on_side: on the context's second stream (ordered after the main stream's work so far), without
// kernel statistics (they time the main stream only)
static void lvl0_launch(Ctx& C, PP& P, const Fr* z, int L, const MsmShard& sh, bool on_side = false) {
    const uint64_t half = (1ull << L) / 2;
    hipStream_t st = C.stream;
    MsmWorkspace* ws = C.msm;
    struct KpRestore {
        KProf* kp = g_kprof;
        ~KpRestore() { g_kprof = kp; }
    } restore;
    if (on_side) {  // C.side_ev: recorded on the main stream once z is in place (prove)
        SPX_HIP(hipStreamWaitEvent(C.side, C.side_ev, 0));
        st = C.side;
        ws = C.msm_side;
        g_kprof = nullptr;
    }
    Fr* q = C.buf<Fr>(Ctx::kSlotLvl0Q, 32 * half);
    launch_open_level(z, nullptr, q, Fr{}, half, st);
    MsmInst I{};
    I.pts_off = P.g2_off[0];
    I.stride = (uint32_t)half;
    I.scalar_off = 0;
    I.size = (uint32_t)half;
    I.c = (uint32_t)P.g2_c[0];
    I.W = (uint32_t)P.g2_W[0];
    const size_t ob = msm_out_bytes(true, 1);
    void* out = C.buf(Ctx::kSlotLvl0Out, ob);
    msm_run_g2(ws, &I, 1, P.g2_pre(), q, out, st, sh);
    SPX_HIP(hipMemcpyAsync(C.pin_at(Ctx::kPinLvl0, ob, 4 << 10), out, ob, hipMemcpyDeviceToHost, st));
}
static Affine<HFq2> lvl0_finish(Ctx& C, PP& P, const Fr* z, int L, Comm& comm, bool on_side = false) {
    if (on_side)
        C.side_sync();
    else
        C.sync();
    const uint8_t* h = C.pin_at(Ctx::kPinLvl0, msm_out_bytes(true, 1), 4 << 10);
    if (msm_status(h, true, 1) & kMsmOverflow) {
        msm_ws_note_overflow(on_side ? C.msm_side : C.msm);
        ++C.msm_reruns;
        MsmShard sh = shard_of(comm);
        sh.dense = true;
        lvl0_launch(C, P, z, L, sh, on_side);
        if (on_side)
            C.side_sync();
        else
            C.sync();
    }
    msm_skew_fold(C, h, true, 1);
    return msm_results<HFq2>(comm, h, 1)[0];
}

// ---------------------------------------------------------------- open (open.rs:19-58)
struct OpenOut {
    HFr eval;
    std::vector<Affine<HFq2>> proofs;
};
// Every level's quotient and fold run here on the whole table (also on proof-sharded ranks, which
// all hold z: the folds are HBM-streaming and cheap, and the bucket-range MSM needs every scalar);
// all MSMs of the opening are one batch. proof0: the shared level-0 proof (lvl0_launch /
// lvl0_finish), or null to compute every level here.
static OpenOut open_z(Ctx& C, PP& P, const Fr* z, int L, const std::vector<HFr>& point, Comm& comm,
                      const Affine<HFq2>* proof0 = nullptr) {
    const uint64_t n = 1ull << L;
    const int first = proof0 ? 1 : 0;  // first level whose MSM runs here
    OpenOut res;
    res.proofs.resize(L);
    if (proof0) res.proofs[0] = *proof0;
    Fr* q = C.buf<Fr>(Ctx::kSlotOpenQ, 32 * n);
    Fr* bufs[2] = {C.buf<Fr>(Ctx::kSlotOpenA, 32 * std::max<uint64_t>(n / 2, 1)),
                   C.buf<Fr>(Ctx::kSlotOpenB, 32 * std::max<uint64_t>(n / 4, 1))};
    std::vector<MsmInst> insts(L - first);
    const Fr* rin = z;
    uint64_t qoff = 0;
    // folds: groups of up to 3 levels per launch while the tables are large, then the last levels
    // (<= 512 pairs) in one single-block launch; the fold-only level 0 (proof0 given) writes no quotient
    std::vector<uint64_t> lvl_qoff(L, ~0ull);  // level i's quotients: q + lvl_qoff[i] (~0: not kept)
    {
        uint64_t o = 0;
        for (int i = first; i < L; ++i) lvl_qoff[i] = o, o += n >> (i + 1);
    }
    int pp = 0;  // ping-pong: the next output buffer
    for (int i = 0; i < L;) {
        const uint64_t half = n >> (i + 1);
        if (i >= first && open_tail_levels(half, L - i) == L - i) {
            std::vector<Fr> pts(L - i);
            for (int j = i; j < L; ++j) pts[j - i] = dev_fr(point[j]);
            Fr* last = bufs[pp];
            launch_open_tail(rin, q + lvl_qoff[i], half, L - i, pts.data(), last, C.stream);
            rin = last;
            break;
        }
        int nf = 1;  // levels in this launch: stop before the tail's start
        while (nf < 3 && i + nf < L && open_tail_levels(n >> (i + nf + 1), L - i - nf) != L - i - nf) ++nf;
        Fr* rout = bufs[pp];
        pp ^= 1;
        if (nf >= 2) {
            Fr pts[3];
            uint64_t qo[3];
            for (int j = 0; j < nf; ++j) pts[j] = dev_fr(point[i + j]), qo[j] = lvl_qoff[i + j];
            launch_open_fold(rin, rout, q, nf, pts, qo, n >> (i + nf), C.stream);
        } else {
            launch_open_level(rin, rout, lvl_qoff[i] != ~0ull ? q + lvl_qoff[i] : q, dev_fr(point[i]), half, C.stream);
        }
        rin = rout;
        i += nf;
    }
    for (int i = 0; i < L; ++i) {
        const uint64_t half = n >> (i + 1);
        if (i < first) continue;  // the level's proof is proof0
        MsmInst& I = insts[i - first];
        I.pts_off = P.g2_off[i];
        I.stride = (uint32_t)half;
        I.scalar_off = qoff;
        I.size = (uint32_t)half;
        I.c = (uint32_t)P.g2_c[i];
        I.W = (uint32_t)P.g2_W[i];
        qoff += half;
    }
    const int nm = L - first;  // MSMs of this batch
    const size_t ob = msm_out_bytes(true, nm);
    void* out = C.buf(Ctx::kSlotOpenOut, ob);
    uint8_t* h = C.pin_at(Ctx::kPinOpen, ob + 32, 56 << 10);
    for (int attempt = 0;; ++attempt) {
        MsmShard sh = shard_of(comm);
        sh.dense = attempt > 0;
        if (nm) {
            msm_run_g2(C.msm, insts.data(), nm, P.g2_pre(), q, out, C.stream, sh);
            SPX_HIP(hipMemcpyAsync(h, out, ob, hipMemcpyDeviceToHost, C.stream));
        }
        if (!attempt) SPX_HIP(hipMemcpyAsync(h + ob, rin, 32, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        if (!nm || !(msm_status(h, true, nm) & kMsmOverflow)) break;
        msm_ws_note_overflow(C.msm);  // compacted keys overflowed: once more with a slot per digit
        ++C.msm_reruns;
    }
    if (nm) msm_skew_fold(C, h, true, nm);
    res.eval = ld_hfr(h + ob);
    std::vector<Affine<HFq2>> part = msm_results<HFq2>(comm, h, nm);
    for (int k = 0; k < nm; ++k) res.proofs[first + k] = part[k];
    return res;
}

// BASELINE config C2 (commitment stubbed): the opening under the all-identity public parameter.
// The evaluation z(point) is computed exactly as open_z computes it (the same folds, no quotients,
// no MSM); h and every level's proof are the identity.
static OpenOut open_stub(Ctx& C, const Fr* z_local, int L, const std::vector<HFr>& point, int G) {
    const int g = ilog2((uint64_t)G);
    const uint64_t nl = (1ull << L) / G;
    const int nloc = L - g;
    OpenOut res;
    res.proofs.assign(L, Affine<HFq2>{HFq2::zero(), HFq2::zero(), true});
    Fr* bufs[2] = {C.buf<Fr>(Ctx::kSlotOpenA, 32 * std::max<uint64_t>(nl / 2, 1)),
                   C.buf<Fr>(Ctx::kSlotOpenB, 32 * std::max<uint64_t>(nl / 4, 1))};
    uint8_t* h = C.pin_at(Ctx::kPinOpen, 32 * (L + 1), 56 << 10);
    // z(point) only (no quotients): three levels per launch while the table is large, then the tail
    // in one launch (level by level this was ~L launches per opening: C2's proofs are launch-bound).
    // The value stays where the chain's last step writes it (no `last`) and is copied from there.
    std::vector<Fr> pts(std::max(nloc, 1));
    for (int j = 0; j < nloc; ++j) pts[j] = dev_fr(point[j]);
    const OpenEvalJob job{z_local, bufs[0], bufs[1], pts.data(), nullptr};
    launch_open_eval(1, &job, nloc, C.stream);
    SPX_HIP(hipMemcpyAsync(h + 32 * L, open_eval_result(job, nloc), 32, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    HFr rlast = ld_hfr(h + 32 * L);
    if (G == 1) {
        res.eval = rlast;
        return res;
    }
    std::vector<HFr> rg = allgather_fr(*C.comm, {rlast});
    for (int i = nloc; i < L; ++i) {
        std::vector<HFr> nr(rg.size() / 2);
        for (size_t b = 0; b < nr.size(); ++b) nr[b] = rg[2 * b] + point[i] * (rg[2 * b + 1] - rg[2 * b]);
        rg.swap(nr);
    }
    res.eval = rg[0];
    return res;
}
static Affine<HFq2> h_of(const PP* P) { return P ? P->h : Affine<HFq2>{HFq2::zero(), HFq2::zero(), true}; }

static void ser_open(Ser& s, const HFr& eval, const Affine<HFq2>& h, const std::vector<Affine<HFq2>>& proofs) {
    s.fr(eval);
    uint8_t b[96];
    host::g2_compress(b, h);
    s.raw(b, 96);
    s.u64(proofs.size());
    for (auto& p : proofs) {
        host::g2_compress(b, p);
        s.raw(b, 96);
    }
}
// the public input v (lib.rs:65): absorbed as a Vec<Fr>, not a prover message
static void absorb_public(Transcript& T, const std::vector<uint8_t>& v) {
    Ser s;
    s.u64(v.size() / 32);
    s.raw(v.data(), v.size());
    T.absorb(s.b.data(), s.b.size());
}
// the prover messages outside the sumchecks: the commitment (round 1), an opening (round 2)
static void emit_commitment(ProofStream& io, int L, const Affine<HFq>& com) {
    io.emit([&](Ser& s) {
        s.u64((uint64_t)L);
        uint8_t b[48];
        host::g1_compress(b, com);
        s.raw(b, 48);
    });
}
static void emit_open(ProofStream& io, const HFr& eval, const Affine<HFq2>& h, const std::vector<Affine<HFq2>>& proofs) {
    io.emit([&](Ser& s) { ser_open(s, eval, h, proofs); });
}

// ====================================================================== prove
// A prove that throws may leave work queued that still reads W.z and writes the context's slots: drain
// it while unwinding, so the caller may free the witness and the next proof on this context starts from
// idle streams. all: the second stream too, and the MSM staging of both (prove(); the stubbed group and
// the witness check queue on the main stream only and run no MSM).
struct UnwindDrain {
    Ctx& C;
    bool all;
    int pending = std::uncaught_exceptions();
    ~UnwindDrain() {
        if (std::uncaught_exceptions() <= pending) return;
        (void)hipStreamSynchronize(C.stream);
        if (!all) return;
        if (C.side) (void)hipStreamSynchronize(C.side);
        msm_ws_staging_reset(C.msm);
        if (C.msm_side) msm_ws_staging_reset(C.msm_side);
    }
};

// the index's SpMV Az, Bz, Cz of this rank's nl rows: the column-sorted entry list, or CSR rows
static void launch_rows_spmv(Index& I, const Fr* z, Fr* Az, Fr* Bz, Fr* Cz, Fr* partial, uint64_t nl, hipStream_t s) {
    const SpmvJob job{z, {Az, Bz, Cz}};
    if (I.rows_sliced.on)
        launch_spmv_sliced(1, &job, I.rows_sliced.view(), I.rows_sliced.entries, s);
    else
        launch_sparse3(0, I.rows.view(), z, Az, Bz, Cz, nullptr, nl, I.rows.chunks.as<LongChunk>(), I.rows.nchunks,
                       I.rows.lrows.as<LongRow>(), I.rows.nlrows, partial, s);
}

// A proof's device buffers, carved from the context's scratch (Fr units): one layout for prove() (this
// rank's nl rows of one proof, with its challenges chdev behind) and for each proof of a lockstep group
// (with the two buffers of its opening's fold chain behind; the group's challenges are one block).
struct ProofScratch {
    Fr *Az, *Bz, *Cz, *F1[3], *F2[3];  // SpMV outputs, their fold ping-pong
    Fr *E1, *Ea, *Eb;                  // eq tables
    Fr *M0, *M1, *M2, *Z1, *Z2;        // M_rx and z folds
    Fr *partial, *eqlo, *eqhi, *eqf;   // partials, eq scratch
    Fr* chdev = nullptr;               // tau, r_x, (r_a, r_b, r_c), ...
    Fr *oA = nullptr, *oB = nullptr;
    // carves from `base` (null: sizes only) and returns the Fr taken
    uint64_t carve(Fr* base, const Index& I, uint64_t nl, int L, bool group) {
        const uint64_t n2 = std::max<uint64_t>(nl / 2, 1), n4 = std::max<uint64_t>(nl / 4, 1);
        uint64_t off = 0;
        auto take = [&](uint64_t k) {
            Fr* p = base ? base + off : nullptr;
            off += k;
            return p;
        };
        Az = take(nl), Bz = take(nl), Cz = take(nl);
        for (int m = 0; m < 3; ++m) F1[m] = take(n2);
        for (int m = 0; m < 3; ++m) F2[m] = take(n4);
        E1 = take(n2), Ea = take(n4), Eb = take(std::max<uint64_t>(nl / 8, 1));
        M0 = take(nl), M1 = take(n2), M2 = take(n4);
        Z1 = take(n2), Z2 = take(n4);
        partial = take(std::max<uint64_t>(kRoundPartials, std::max(I.rows.nchunks, I.cols.longc.nchunks)));
        eqlo = take(8192), eqhi = take(8192), eqf = take(kEqScratch);
        if (group)
            oA = take(n2), oB = take(n4);
        else
            chdev = take(8 * L);
        take(64);  // slack
        return off;
    }

    // The sumchecks' device rounds. Round i (1-based) reads the running tables; from round 2 on it first
    // binds the previous challenge into the ping-pong buffers of its parity, which become the running
    // tables (done_round). The rounds' sums land in res_dev (host-mapped pinned memory).
    Tables3 cur{};
    const Fr *Ecur = nullptr, *Mc = nullptr, *Zc = nullptr;
    uint32_t* ticket = nullptr;
    Fr* res_dev = nullptr;
    void begin1() { cur = Tables3{{Az, Bz, Cz}}, Ecur = E1; }
    void begin2(const Fr* z_local) { Mc = M0, Zc = z_local; }
    // (nvars local variables: the last round's fold writes no E, nothing reads it)
    Sc1Job sc1_job(int i, int nvars, const std::vector<HFr>& r) const {
        Sc1Job j{cur, Tables3{{nullptr, nullptr, nullptr}}, Ecur, nullptr, Fr{}, partial, ticket, res_dev};
        if (i >= 2) {
            Fr* const* fb = (i % 2 == 0) ? F1 : F2;
            j.out = Tables3{{fb[0], fb[1], fb[2]}};
            if (i < nvars) j.Eout = (i & 1) ? Eb : Ea;
            j.r = dev_fr(r[i - 2]);
        }
        return j;
    }
    Sc2Job sc2_job(int i, const std::vector<HFr>& r) const {
        Sc2Job j{Mc, Zc, nullptr, nullptr, Fr{}, partial, ticket, res_dev};
        if (i >= 2) {
            j.Mout = (i & 1) ? M2 : M1;
            j.Zout = (i & 1) ? Z2 : Z1;
            j.r = dev_fr(r[i - 2]);
        }
        return j;
    }
    void done_round(const Sc1Job& j) {
        if (j.out.t[0]) cur = j.out;
        if (j.Eout) Ecur = j.Eout;
    }
    void done_round(const Sc2Job& j) {
        if (j.Mout) Mc = j.Mout, Zc = j.Zout;
    }
};
// a round's G(1) / P(1) is computed on the device if the host cannot derive it from the claim, or checks it
template <class Sumcheck>
static bool round_need1(const Sumcheck& sc, bool check) {
    return check || !sc.derivable();
}

// round 3's eq table of a 1-variable proof is the constant 1
static void upload_one(Fr* E1, uint8_t* pin, hipStream_t s) {
    const HFr one = HFr::one();
    memcpy(pin, &one, 32);
    SPX_HIP(hipMemcpyAsync(E1, pin, 32, hipMemcpyHostToDevice, s));
}
// a rank's three sums of a round -> the sums over all ranks
static void sum_ranks(Comm& comm, HFr s[3]) {
    if (comm.size() == 1) return;
    const std::vector<HFr> all = allgather_fr(comm, {s[0], s[1], s[2]});
    s[0] = s[1] = s[2] = HFr::zero();
    for (size_t r = 0; r < all.size() / 3; ++r)
        for (int k = 0; k < 3; ++k) s[k] += all[3 * r + k];
}

// ---------------------------------------------------------------- witness check
// The kernel writes each proof's record straight into the context's pinned carve-out (as the sumcheck
// rounds write their sums): it is read after the next wait that covers the launch, no copy is queued.
static_assert(kGroupMax * kR1csRecordStride <= (2 << 10) && 8 * kR1csRecordWords <= kR1csRecordStride,
              "the group's records fit their pinned region");
static uint8_t* witness_record(Ctx& C, int j) {
    return C.pin_at(Ctx::kPinWitness, kGroupMax * kR1csRecordStride, 2 << 10) + kR1csRecordStride * j;
}
// proof j's job: its tables, 2 x kR1csMaxBlocks words of `partial`, the context's ticket j and record j
static R1csCheckJob witness_job(Ctx& C, int j, const Fr* Az, const Fr* Bz, const Fr* Cz, Fr* partial) {
    static_assert(16 * (uint64_t)kR1csMaxBlocks <= 32 * kRoundPartials, "the check's partials fit a proof's round partials");
    return R1csCheckJob{Az, Bz, Cz, reinterpret_cast<uint64_t*>(partial), C.ticket + j,
                        C.pin_dev<uint64_t>(witness_record(C, j))};
}
static void witness_check_launch(Ctx& C, const R1csCheckJob* jobs, int k, uint64_t nl, uint64_t row0) {
    launch_r1cs_check(k, jobs, nl, row0, C.stream);
    C.wcstat[2] += 1;
    C.wcstat[3] += (uint64_t)k * nl;
}
std::string WitnessReport::message() const {
    return "constraint " + std::to_string(first_row) + " is not satisfied: (Az)(Bz) != Cz (" + std::to_string(bad) +
           " of " + std::to_string(rows) + " constraints fail)";
}
// Proof j's verdict, after a wait that covers its check. Sharded: one exchange of the ranks' records
// (112 B each); every rank then holds the sum of the counts, the lowest first row and that row's values.
static WitnessReport witness_verdict(Ctx& C, int j, Comm& comm, uint64_t n) {
    constexpr size_t kRec = 8 * kR1csRecordWords;
    const int G = comm.size();
    std::vector<uint8_t> all(kRec * G);
    if (G > 1)
        comm.allgather(witness_record(C, j), all.data(), kRec);
    else
        memcpy(all.data(), witness_record(C, j), kRec);
    WitnessReport rep;
    rep.rows = n;
    const uint8_t* at = nullptr;
    for (int r = 0; r < G; ++r) {
        uint64_t w[2];
        memcpy(w, all.data() + kRec * r, 16);
        rep.bad += w[0];
        if (w[1] < rep.first_row) rep.first_row = w[1], at = all.data() + kRec * r + 16;
    }
    if (at)
        for (int m = 0; m < 3; ++m) {
            uint64_t c[4];
            ld_hfr(at + 32 * m).to_canon(c);
            memcpy(rep.abc + 32 * m, c, 32);
        }
    ++C.wcstat[0];
    if (rep.bad) ++C.wcstat[1];
    return rep;
}

std::vector<uint8_t> prove(Ctx& C, Index& I, Witness& W, PP* P, const ProveOpts& o) {
    CtxClaim claim;
    if (!o.claimed) claim.take(C);  // before anything is queued: a refused prove touches nothing
    UnwindDrain drain{C, true};
    Timer tall;
    C.timings.clear();
    int phase = 0;
    uint64_t cpu0 = thread_cpu_ns();
    auto mark = [&](const char* name, Timer& t) {
        const double us = t.us();
        C.timings.emplace_back(name, us);
        t = Timer();
        const uint64_t c1 = thread_cpu_ns();
        if (phase < kHostPhases) {
            g_phase_cpu[phase] += c1 - cpu0;
            g_phase_wall[phase] += (uint64_t)(us * 1e3);
            g_phase_cnt[phase] += 1;
        }
        ++phase;
        cpu0 = c1;
    };
    Timer tp;
    const int L = I.log_n;
    const uint64_t n = I.n;
    Comm& comm = *C.comm;
    const int G = comm.size(), rank = comm.rank();
    if (G != I.G || rank != I.rank) invalid("index was built for a different communicator");
    const int g = ilog2((uint64_t)G);
    const uint64_t nl = n / G, lo = (uint64_t)rank * nl;
    const uint64_t nvv = W.v.size() / 32;
    if (!is_pow2(nvv)) invalid("public input should be power of two");
    if (W.n != n) invalid("|v| + |w| != number of variables");  // prover.rs:117-119
    if (!o.stub && !P) invalid("null public parameter");
    C.side_sync();  // a proof that threw may have left its level-0 MSM running on the second stream
    if (P && P->nv != L) invalid("public parameter nv != log_n");
    const int log_v = ilog2(nvv);
    const Fr* z = W.z.as<Fr>();
    const Fr* zl = z + lo;
    ProofScratch S;
    C.scratch.ensure(32 * S.carve(nullptr, I, nl, L, false));
    S.carve(C.scratch.as<Fr>(), I, nl, L, false);
    Fr* const partial = S.partial;
    uint8_t* hp = C.pin_at(Ctx::kPinHp, 1 << 16, 64 << 10);

    // ---- SpMV Az, Bz, Cz (challenge-independent: queued first, overlaps the commit's host work)
    kp_begin(KP_SPMV, C.stream);
    launch_rows_spmv(I, z, S.Az, S.Bz, S.Cz, partial, nl, C.stream);
    kp_end(I.rows_bytes, C.stream);
    // ---- witness check (off by default): one launch behind the SpMV; its record is read at the proof's
    // first host wait (witness_checked below), so it adds no wait
    const bool wcheck = C.witness_check();
    if (wcheck) {
        const R1csCheckJob job = witness_job(C, 0, S.Az, S.Bz, S.Cz, partial);
        witness_check_launch(C, &job, 1, nl, lo);
    }
    auto witness_checked = [&] {
        const WitnessReport rep = witness_verdict(C, 0, comm, n);
        if (!rep.bad) return;
        C.sync();  // what the proof has queued so far, both streams: the next prove starts clean
        C.side_sync();
        throw SpxError(kWrongWitness, rep.message());
    };
    // The shared level-0 opening proof is launched right behind the commitment, before any challenge,
    // when the host has the matrix absorption to do meanwhile. With the index-cached transcript there
    // is nothing to hide it behind: a sharded proof then runs it on the context's second stream, beside
    // the commitment and the first opening (reused by the second opening); an unsharded one puts it in
    // the first opening's batch (below). (Both forms give every rank the same
    // batches, so the exchanges of a proof-sharded prove line up.)
    // SPX_LVL0=batch (A/B; must be the same on every rank of a proof-sharded prove): level 0 inside the
    // first opening's MSM batch instead, one MSM pipeline (sort, weighting tree) less per proof
    static const bool lvl0_batch_env = [] {
        const char* e = getenv("SPX_LVL0");
        return e && std::string(e) == "batch";
    }();
    // Unsharded index-cached proofs default to the batch form: with no absorption to hide level 0
    // behind, one MSM pipeline less measured +2% index-cached at N = 1 (profiles/r06/r06zq_ab_lvl0_n1.jsonl)
    const bool lvl0_batch =
        C.lvl0_mode >= 0 ? C.lvl0_mode == 1 : (lvl0_batch_env || (G == 1 && o.cached && I.has_cache && !o.coins));
    const bool check = check_derived();
    if (G > 1 && !C.knobs_agreed) {
        // the level-0 mode decides the order and sizes of a proof's exchanges: every rank of the
        // communicator must read the same SPX_LVL0 (one exchange on a context's first sharded proof)
        // (and so does the witness check, which adds one: bit 1)
        const uint32_t mine = (lvl0_batch ? 1u : 0u) | (wcheck ? 2u : 0u);
        std::vector<uint32_t> all(G);
        comm.allgather(&mine, all.data(), sizeof mine);
        for (int r = 0; r < G; ++r) {
            if ((all[r] ^ mine) & 1u) invalid("SPX_LVL0 / level-0 mode differs between the ranks of this communicator");
            if (all[r] != mine) invalid("SPX_WITNESS_CHECK / witness check mode differs between the ranks of this communicator");
        }
        C.knobs_agreed = true;
    }
    const bool share0 = !o.stub;
    const bool early0 = share0 && !lvl0_batch && !(o.cached && I.has_cache);
    const bool side0 = share0 && !lvl0_batch && !early0;
    const MsmShard sh = shard_of(comm);
    if (side0) {  // z is in place: the second stream may start
        C.ensure_side();
        SPX_HIP(hipEventRecord(C.side_ev, C.stream));
    }
    // ---- round 1: commitment (prover.rs:123-141); the MSM runs while the host absorbs A, B, C
    if (!o.stub) commit_launch(C, *P, z, n, sh);
    if (early0) lvl0_launch(C, *P, z, L, sh);
    if (side0) lvl0_launch(C, *P, z, L, sh, true);
    ProofStream io{Transcript(o.mode == 1, o.seed, o.coins), {}};
    Transcript& T = io.T;
    const uint64_t ctr = C.prove_seq++;
    const uint64_t seq = o.seq >= 0 ? (uint64_t)o.seq : ctr;
    const Blake2s* absorbed = o.await_absorbed ? o.await_absorbed() : o.absorbed;
    if (o.coins) {
        // interactive: the caller is the verifier; nothing is absorbed
    } else if (o.cached && I.has_cache)
        T.set_state(I.cache);
    else if (G == 1) {
        T.set_state(absorbed ? *absorbed : absorb_matrices(I));
    } else {
        // the (sequential, ~150 MB at 2^20) absorption of A, B, C is done once per proof, by one rank
        // in turn; the others take its Blake2s state from the allgather (bit-identical transcript)
        static_assert(std::is_trivially_copyable<Blake2s>::value, "Blake2s state is shipped as bytes");
        const int owner = (int)(seq % (uint64_t)G);
        Blake2s h;
        if (rank == owner) h = absorbed ? *absorbed : absorb_matrices(I);
        std::vector<uint8_t> all(sizeof(Blake2s) * G);
        comm.allgather(&h, all.data(), sizeof(Blake2s));
        memcpy(&h, all.data() + sizeof(Blake2s) * owner, sizeof(Blake2s));
        T.set_state(h);
    }
    absorb_public(T, W.v);
    mark("transcript_matrices", tp);
    Affine<HFq> com = o.stub ? Affine<HFq>{HFq::zero(), HFq::zero(), true} : commit_finish(C, *P, z, n, comm);
    // the commitment's wait covered the check: before any challenge is drawn or message emitted (a
    // stubbed proof has no wait here: its verdict follows its first opening's wait, below)
    if (wcheck && !o.stub) witness_checked();
    Affine<HFq2> proof0{};
    if (early0) proof0 = lvl0_finish(C, *P, z, L, comm);
    emit_commitment(io, L, com);
    mark("commit", tp);
    // ---- round 2: open at (r_v, 0...0) (prover.rs:143-160)
    std::vector<HFr> pt1(L, HFr::zero());
    for (int i = 0; i < log_v; ++i) pt1[i] = T.rand_fr();
    {
        OpenOut op = o.stub ? open_stub(C, zl, L, pt1, G)
                            : open_z(C, *P, z, L, pt1, comm, (early0 || side0) ? &proof0 : nullptr);
        if (wcheck && o.stub) witness_checked();  // the stubbed proof's first wait (r_v is derived, nothing emitted)
        if (side0) op.proofs[0] = proof0 = lvl0_finish(C, *P, z, L, comm, true);
        if (share0 && !early0 && !side0) proof0 = op.proofs[0];
        emit_open(io, op.eval, h_of(P), op.proofs);
    }
    mark("open_rv", tp);
    // ---- round 3: tau, eq, sumcheck #1 setup (prover.rs:163-196)
    std::vector<HFr> tau(L);
    for (int i = 0; i < L; ++i) tau[i] = T.rand_fr();
    memcpy(hp, tau.data(), 32 * L);
    SPX_HIP(hipMemcpyAsync(S.chdev, hp, 32 * L, hipMemcpyHostToDevice, C.stream));
    // E_1[b] = eq(tau_1..tau_{L-1}, b) on this rank's block of b
    if (L >= 2) {
        const EqTableJob job{S.chdev + 1, S.E1, S.eqlo, S.eqhi};
        launch_eq_table(1, &job, L - 1, (uint64_t)rank * (nl / 2), nl / 2, C.stream);
    } else {
        upload_one(S.E1, hp + 4096, C.stream);
    }
    // ---- sumcheck #1 (lib.rs:86-103)
    io.sumcheck_header(L + 2, L);
    Sumcheck1 s1(io, std::move(tau));
    S.ticket = C.ticket;
    S.res_dev = C.pin_dev<Fr>(hp);  // the rounds' sums land in pinned host memory (hp)
    S.begin1();
    // The last ht1 rounds of each sumcheck run on the host, as in prove_group: each rank binds its local
    // tables (<= 64 entries) and, sharded, the ranks' tables are gathered in rank order (the g high
    // variables) before the last g + ht1 rounds. Unsharded: one proof at a time 22.5 vs 22.6 ms
    // index-cached, throughput equal (profiles/r05/r05zt_ab_hosttail1.jsonl); a rank of an 8-rank proof
    // +2.3% (r05zu_ab_shardtail_G8.jsonl: 10 fewer launches and exchanges per proof). Fixed, so every
    // rank of a communicator agrees.
    const int ht1 = std::max(0, std::min(kGroupHostTail, L - g - 1));
    const uint32_t tn = 2u << ht1;  // entries per table after the device rounds
    for (int i = 1; i <= L - g - ht1; ++i) {
        const Sc1Job job = S.sc1_job(i, L - g, s1.r);
        launch_sc1_round(1, &job, i >= 2, round_need1(s1, check), nl >> i, C.stream);
        C.sync();
        HFr gs[3] = {ld_hfr(hp), ld_hfr(hp + 32), ld_hfr(hp + 64)};
        sum_ranks(comm, gs);
        s1.device_round(gs, check);
        S.done_round(job);
    }
    // local tables now hold tn entries each (2 when sharded; folded up to r_{L-g-ht1-1}): r_{L-g-ht1} is
    // bound on the host, the ranks' tables are gathered, and the last g + ht1 rounds run there
    for (int m = 0; m < 3; ++m)
        SPX_HIP(hipMemcpyAsync(hp + 32 * tn * m, S.cur.t[m], 32 * tn, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    std::vector<HFr> mine = s1.bind(hp, tn);
    const std::vector<HFr> vabc = s1.tail(rank_order(G == 1 ? std::move(mine) : allgather_fr(comm, mine), 3, G));
    mark("sumcheck1", tp);
    // ---- round 4 (prover.rs:210-228)
    io.emit([&](Ser& s) {
        for (int m = 0; m < 3; ++m) s.fr(vabc[m]);
    });
    HFr rabc[3] = {T.rand_fr(), T.rand_fr(), T.rand_fr()};
    // ---- round 5: M_rx = sum_m r_m M(r_x, .) on this rank's columns (prover.rs:230-255)
    Fr* rxdev = S.chdev + 2 * L;  // r_x (L) then r_abc (3)
    memcpy(hp, s1.r.data(), 32 * L);
    memcpy(hp + 32 * L, rabc, 96);
    SPX_HIP(hipMemcpyAsync(rxdev, hp, 32 * (L + 3), hipMemcpyHostToDevice, C.stream));
    {
        kp_begin(KP_MTV, C.stream);
        const ColStreamJob job{rxdev, rxdev + L, S.M0, S.eqf, partial};
        I.cols.launch(1, &job, L, C.stream);
        kp_end(I.cols_bytes, C.stream);
    }
    io.sumcheck_header(2, L);
    mark("eval_on_x", tp);
    // ---- sumcheck #2 (lib.rs:114-131)
    Sumcheck2 s2(io, L);
    S.begin2(zl);
    for (int i = 1; i <= L - g - ht1; ++i) {
        const Sc2Job job = S.sc2_job(i, s2.r);
        launch_sc2_round(1, &job, i >= 2, round_need1(s2, check), nl >> i, C.stream);
        C.sync();
        HFr ps[3] = {ld_hfr(hp), ld_hfr(hp + 32), ld_hfr(hp + 64)};
        sum_ranks(comm, ps);
        s2.device_round(ps, check);
        S.done_round(job);
    }
    if (g + ht1 > 0) {
        SPX_HIP(hipMemcpyAsync(hp, S.Mc, 32 * tn, hipMemcpyDeviceToHost, C.stream));
        SPX_HIP(hipMemcpyAsync(hp + 32 * tn, S.Zc, 32 * tn, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        mine = s2.bind(hp, tn);
        s2.tail(rank_order(G == 1 ? std::move(mine) : allgather_fr(comm, mine), 2, G));
    }
    mark("sumcheck2", tp);
    // ---- round 6: open at r_y (prover.rs:268-281)
    {
        OpenOut op = o.stub ? open_stub(C, zl, L, s2.r, G) : open_z(C, *P, z, L, s2.r, comm, share0 ? &proof0 : nullptr);
        ser_open(io.proof, op.eval, h_of(P), op.proofs);
    }
    mark("open_ry", tp);
    C.timings.emplace_back("total", tall.us());
    return std::move(io.proof.b);
}

// ====================================================================== lockstep groups
// prove() for k stubbed-commitment proofs of one index on one rank (BASELINE C2), interleaved step by
// step. A C2 proof is ~55 small launches and ~40 host waits: with 32 proofs in flight on the context
// streams' 4 hardware queues the GPU ran ~1 kernel at a time and was idle 65% of the time (trace
// profiles/r05/r05zg_c2_busy.txt), each proof waiting its turn in a queue. Here the k proofs' sumcheck
// rounds are one launch each (launch_sc1_round with k jobs: blockIdx.y = proof) with one wait, and the other
// steps queue the k proofs' launches back to back before one wait. Every value is computed by the same
// kernels as prove() and by the same host code (sumcheck_host.hpp), so each proof's bytes are its own
// prove()'s.
std::vector<std::vector<uint8_t>> prove_group(Ctx& C, Index& I, Witness* const* Ws, int k, const ProveOpts* os,
                                              std::vector<std::string>* rejected) {
    static_assert(kGroupMax <= 16, "one sumcheck ticket per proof of a group: Ctx::ticket holds 16 counters");
    if (k < 1 || k > kGroupMax) invalid("lockstep group size must be 1.." + std::to_string(kGroupMax));
    CtxClaim claim;
    claim.take(C);
    UnwindDrain drain{C, false};
    // a group records no per-phase marks (its phases interleave k proofs): spx_last_timings reports
    // its total alone, and the host-phase counters (spx_host_phase_stats) count prove() calls only
    C.timings.clear();
    Timer tgroup;
    Comm& comm = *C.comm;
    if (comm.size() != 1 || I.G != 1) invalid("lockstep groups need an unsharded context and index");
    const int L = I.log_n;
    const uint64_t n = I.n, nl = n;
    for (int j = 0; j < k; ++j) {
        if (!Ws[j]) invalid("null witness");
        if (!os[j].stub || os[j].coins || os[j].claimed) invalid("lockstep groups prove stubbed-commitment proofs only");
        if (!is_pow2(Ws[j]->v.size() / 32)) invalid("public input should be power of two");
        if (Ws[j]->n != n) invalid("|v| + |w| != number of variables");  // prover.rs:117-119
    }
    const bool check = check_derived();
    // per-proof scratch, prove()'s layout at G = 1 (plus the opening folds' two buffers per proof: the
    // group's fold chains run side by side)
    const uint64_t need = ProofScratch().carve(nullptr, I, nl, L, true);
    // the group's challenges: proof j's tau, r_x, r_abc at chg + 8 L j (one host-to-device copy each time)
    C.scratch.ensure(32 * (need + 8 * (uint64_t)L) * (uint64_t)k);
    Fr* chg = C.scratch.as<Fr>() + need * k;
    static_assert(kGroupMax * 8192 <= (128 << 10), "per-proof pinned regions");
    if (32 * (L + 3) > 4096 || 32 * 8 * L * kGroupMax > (128 << 10)) invalid("log_n too large for a lockstep group");
    uint8_t* hp0 = C.pin_at(Ctx::kPinHp, kGroupMax * 8192, 128 << 10);
    uint8_t* ho0 = C.pin_at(Ctx::kPinOpen, kGroupMax * 2048, 56 << 10);
    uint8_t* stage = C.pin_at(Ctx::kPinStage, (size_t)32 * 8 * L * k, 128 << 10);
    struct P : ProofScratch {
        uint8_t *hp, *ho;
        const Fr* z;
        int log_v;
        ProofStream io;
        Sumcheck1 s1;
        Sumcheck2 s2;
    };
    std::vector<P> ps(k);  // (sized once: s1 and s2 point at their proof's io)
    for (int j = 0; j < k; ++j) {
        P& p = ps[j];
        p.carve(C.scratch.as<Fr>() + need * j, I, nl, L, true);
        p.chdev = chg + (uint64_t)8 * L * j;
        p.hp = hp0 + 8192 * j;
        p.ho = ho0 + 2048 * j;
        p.ticket = C.ticket + j;
        p.res_dev = C.pin_dev<Fr>(p.hp);
        p.z = Ws[j]->z.as<Fr>();
        p.log_v = ilog2(Ws[j]->v.size() / 32);
        p.io.T = Transcript(os[j].mode == 1, os[j].seed, nullptr);
    }
    // ---- SpMV Az, Bz, Cz of every proof (challenge-independent)
    if (I.rows_sliced.on) {
        kp_begin(KP_SPMV, C.stream);
        std::vector<SpmvJob> jobs;
        for (auto& p : ps) jobs.push_back(SpmvJob{p.z, {p.Az, p.Bz, p.Cz}});
        launch_spmv_sliced(k, jobs.data(), I.rows_sliced.view(), I.rows_sliced.entries, C.stream);
        // one index stream for the group (k_spmv_sliced_group), z and the outputs per proof
        kp_end(I.rows_index_bytes + (I.rows_bytes - I.rows_index_bytes) * k, C.stream);
    } else {
        for (auto& p : ps) launch_rows_spmv(I, p.z, p.Az, p.Bz, p.Cz, p.partial, nl, C.stream);
    }
    // ---- witness check (off by default): the k proofs' checks in one launch (blockIdx.y = proof); the
    // records are read behind the group's first wait (round 2's)
    const bool wcheck = C.witness_check();
    std::vector<std::string> why(k);
    if (wcheck) {
        std::vector<R1csCheckJob> jobs;
        for (int j = 0; j < k; ++j) jobs.push_back(witness_job(C, j, ps[j].Az, ps[j].Bz, ps[j].Cz, ps[j].partial));
        witness_check_launch(C, jobs.data(), k, nl, 0);
    }
    // ---- transcripts: A, B, C (cached or absorbed), v; round 1 with the stubbed commitment
    for (int j = 0; j < k; ++j) {
        P& p = ps[j];
        const ProveOpts& o = os[j];
        C.prove_seq++;
        if (o.cached && I.has_cache)
            p.io.T.set_state(I.cache);
        else {
            const Blake2s* absorbed = o.await_absorbed ? o.await_absorbed() : o.absorbed;
            p.io.T.set_state(absorbed ? *absorbed : absorb_matrices(I));
        }
        absorb_public(p.io.T, Ws[j]->v);
        emit_commitment(p.io, L, Affine<HFq>{HFq::zero(), HFq::zero(), true});
    }
    // stubbed openings: every proof's z(point) by open_stub's fold chain, one launch per step for the
    // group, the values written straight into pinned memory; one wait
    auto open_all = [&](const std::vector<std::vector<HFr>>& pts) {
        std::vector<Fr> flat((size_t)k * L);
        for (int j = 0; j < k; ++j)
            for (int i = 0; i < L; ++i) flat[(size_t)j * L + i] = dev_fr(pts[j][i]);
        std::vector<OpenEvalJob> jobs;
        for (int j = 0; j < k; ++j)
            jobs.push_back(OpenEvalJob{ps[j].z, ps[j].oA, ps[j].oB, flat.data() + (size_t)j * L, C.pin_dev<Fr>(ps[j].ho)});
        launch_open_eval(k, jobs.data(), L, C.stream);
        C.sync();
        const std::vector<Affine<HFq2>> none(L, Affine<HFq2>{HFq2::zero(), HFq2::zero(), true});
        for (auto& p : ps) emit_open(p.io, ld_hfr(p.ho), h_of(nullptr), none);
    };
    {  // round 2: open at (r_v, 0...0)
        std::vector<std::vector<HFr>> pts(k);
        for (int j = 0; j < k; ++j) {
            pts[j].assign(L, HFr::zero());
            for (int i = 0; i < ps[j].log_v; ++i) pts[j][i] = ps[j].io.T.rand_fr();
        }
        open_all(pts);
    }
    if (wcheck)  // a rejected proof keeps its slot (the group runs on in lockstep); its bytes are dropped at the end
        for (int j = 0; j < k; ++j) {
            const WitnessReport rep = witness_verdict(C, j, comm, n);
            if (!rep.bad) continue;
            why[j] = rep.message();
            if (!rejected) throw SpxError(kWrongWitness, why[j]);  // (the stream is idle: open_all waited)
        }
    // ---- round 3: tau (one copy for the group), eq tables (one launch pair); sumcheck 1 setup
    for (int j = 0; j < k; ++j) {
        P& p = ps[j];
        std::vector<HFr> tau(L);
        for (int i = 0; i < L; ++i) tau[i] = p.io.T.rand_fr();
        memcpy(stage + (size_t)32 * 8 * L * j, tau.data(), 32 * L);
        p.s1 = Sumcheck1(p.io, std::move(tau));
    }
    SPX_HIP(hipMemcpyAsync(chg, stage, (size_t)32 * 8 * L * k, hipMemcpyHostToDevice, C.stream));
    if (L >= 2) {
        std::vector<EqTableJob> jobs;
        for (auto& p : ps) jobs.push_back(EqTableJob{p.chdev + 1, p.E1, p.eqlo, p.eqhi});
        launch_eq_table(k, jobs.data(), L - 1, 0, nl / 2, C.stream);
    }
    for (auto& p : ps) {
        if (L < 2) upload_one(p.E1, p.hp + 4096, C.stream);
        p.io.sumcheck_header(L + 2, L);
        p.begin1();
    }
    // The last ht rounds of each sumcheck run on the host (the tables are then <= 2^(ht+1) entries: a few
    // microseconds of host arithmetic per round, against a ~30 us launch that holds one of the 4 hardware
    // queues), with prove()'s formulas for the gathered tables of a sharded proof: the same field values.
    // (2,216 - 2,221 M index-cached against 2,138 - 2,155 M with every round on the device, 3 or 4 rounds
    // between: profiles/r05/r05zs_hosttail.jsonl)
    static_assert(kGroupHostTail >= 0 && kGroupHostTail <= 5, "3 x 2^(ht+1) Fr fit each proof's 8 KiB pinned region");
    const int ht = std::min(kGroupHostTail, L - 1);
    // ---- sumcheck 1: one launch and one wait per round for the group
    std::vector<Sc1Job> j1(k);
    for (int i = 1; i <= L - ht; ++i) {
        bool need1 = false;  // one flag for the launch: G(1) for all if any proof needs it
        for (int j = 0; j < k; ++j) {
            j1[j] = ps[j].sc1_job(i, L, ps[j].s1.r);
            need1 = need1 || round_need1(ps[j].s1, check);
        }
        launch_sc1_round(k, j1.data(), i >= 2, need1, nl >> i, C.stream);
        C.sync();
        for (int j = 0; j < k; ++j) {
            P& p = ps[j];
            HFr gs[3] = {ld_hfr(p.hp), ld_hfr(p.hp + 32), ld_hfr(p.hp + 64)};
            p.s1.device_round(gs, check);
            p.done_round(j1[j]);
        }
    }
    // the tables hold tn = 2^(ht+1) entries each: bind r_{L-ht} on the host, then the host rounds
    const uint32_t tn = 2u << ht;
    {
        std::vector<CopyJob> jobs;
        for (auto& p : ps) jobs.push_back(CopyJob{{p.cur.t[0], p.cur.t[1], p.cur.t[2]}, C.pin_dev<Fr>(p.hp)});
        launch_copy_runs(k, jobs.data(), 3, (int)tn, C.stream);
    }
    C.sync();
    for (int j = 0; j < k; ++j) {
        P& p = ps[j];
        const std::vector<HFr> vabc = p.s1.tail(p.s1.bind(p.hp, tn));
        // ---- round 4
        p.io.emit([&](Ser& s) {
            for (int m = 0; m < 3; ++m) s.fr(vabc[m]);
        });
        HFr rabc[3] = {p.io.T.rand_fr(), p.io.T.rand_fr(), p.io.T.rand_fr()};
        // ---- round 5's challenges, staged for one copy (the waits above cover the stage's earlier copy)
        uint8_t* st = stage + (size_t)32 * (8 * L * j + 2 * L);
        memcpy(st, p.s1.r.data(), 32 * L);
        memcpy(st + 32 * L, rabc, 96);
        p.io.sumcheck_header(2, L);
        p.s2 = Sumcheck2(p.io, L);
        p.begin2(p.z);
    }
    // ---- round 5: M_rx = sum_m r_m M(r_x, .) of every proof
    SPX_HIP(hipMemcpyAsync(chg, stage, (size_t)32 * 8 * L * k, hipMemcpyHostToDevice, C.stream));
    kp_begin(KP_MTV, C.stream);
    {
        std::vector<ColStreamJob> jobs;
        for (auto& p : ps) jobs.push_back(ColStreamJob{p.chdev + 2 * L, p.chdev + 3 * L, p.M0, p.eqf, p.partial});
        I.cols.launch(k, jobs.data(), L, C.stream);
    }
    kp_end(I.cols_bytes * k, C.stream);
    // ---- sumcheck 2
    std::vector<Sc2Job> j2(k);
    for (int i = 1; i <= L - ht; ++i) {
        for (int j = 0; j < k; ++j) j2[j] = ps[j].sc2_job(i, ps[j].s2.r);
        launch_sc2_round(k, j2.data(), i >= 2, round_need1(ps[0].s2, check), nl >> i, C.stream);  // (the same for every proof)
        C.sync();
        for (int j = 0; j < k; ++j) {
            P& p = ps[j];
            HFr q[3] = {ld_hfr(p.hp), ld_hfr(p.hp + 32), ld_hfr(p.hp + 64)};
            p.s2.device_round(q, check);
            p.done_round(j2[j]);
        }
    }
    if (ht > 0) {  // M and Z hold tn entries each: bind r_{L-ht}, then the host rounds
        {
            std::vector<CopyJob> jobs;
            for (auto& p : ps) jobs.push_back(CopyJob{{p.Mc, p.Zc, nullptr}, C.pin_dev<Fr>(p.hp)});
            launch_copy_runs(k, jobs.data(), 2, (int)tn, C.stream);
        }
        C.sync();
        for (auto& p : ps) p.s2.tail(p.s2.bind(p.hp, tn));
    }
    // ---- round 6: open at r_y
    {
        std::vector<std::vector<HFr>> pts(k);
        for (int j = 0; j < k; ++j) pts[j] = ps[j].s2.r;
        open_all(pts);
    }
    std::vector<std::vector<uint8_t>> out(k);
    for (int j = 0; j < k; ++j)
        if (why[j].empty()) out[j] = std::move(ps[j].io.proof.b);
    if (rejected) *rejected = std::move(why);
    C.timings.emplace_back("total_group", tgroup.us());
    return out;
}

// ====================================================================== stand-alone witness check
// prove()'s first launch (the index's SpMV, sliced or CSR) into scratch, the check kernel, one wait.
WitnessReport check_witness(Ctx& C, Index& I, Witness& W) {
    CtxClaim claim(C);
    UnwindDrain drain{C, false};  // a failed exchange leaves nothing running that reads W.z
    Comm& comm = *C.comm;
    const int G = comm.size(), rank = comm.rank();
    if (G != I.G || rank != I.rank) invalid("index was built for a different communicator");
    if (W.n != I.n) invalid("|v| + |w| != number of variables");
    C.side_sync();
    const uint64_t nl = I.n / G, lo = (uint64_t)rank * nl;
    const uint64_t npart = std::max<uint64_t>(kRoundPartials, I.rows.nchunks);
    C.scratch.ensure(32 * (3 * nl + npart));
    Fr *Az = C.scratch.as<Fr>(), *Bz = Az + nl, *Cz = Bz + nl, *partial = Cz + nl;
    launch_rows_spmv(I, W.z.as<Fr>(), Az, Bz, Cz, partial, nl, C.stream);
    const R1csCheckJob job = witness_job(C, 0, Az, Bz, Cz, partial);
    witness_check_launch(C, &job, 1, nl, lo);
    C.sync();
    return witness_verdict(C, 0, comm, I.n);
}

// ====================================================================== kernel-level entry points
// ====================================================================== verifier
// lib.rs:147-212 with verifier.rs:143-512. The transcript is replayed on the host; the O(nnz) matrix
// evaluation (A, B, C)(r_x, r_y) runs on the GPU with the prover's kernels (eq table, CSC gather into
// sum_M r_M M(r_x, .), then L fold levels at r_y); the two mKZG checks (verify.rs:12-45) use the
// host pairing of pairing.hpp.
VP vp_load(const uint8_t* b, size_t len) {
    VP V;
    size_t pos = 0;
    auto take = [&](size_t k) {
        if (pos + k > len) throw SpxError(kSerialization, "truncated verifier parameter");
        const uint8_t* p = b + pos;
        pos += k;
        return p;
    };
    uint64_t nv, cnt;
    memcpy(&nv, take(8), 8);
    if (nv > (uint64_t)kMaxLogN) throw SpxError(kSerialization, "bad verifier parameter nv (<= 26 supported)");
    V.nv = (int)nv;
    if (!host::g1_from_uncompressed(V.g, take(96)) || !host::g2_from_uncompressed(V.h, take(192)))
        throw SpxError(kSerialization, "bad verifier parameter point");
    memcpy(&cnt, take(8), 8);
    if (cnt != nv) throw SpxError(kSerialization, "g_mask_random length != nv");
    V.g_mask.resize(cnt);
    for (auto& g : V.g_mask)
        if (!host::g1_from_uncompressed(g, take(96))) throw SpxError(kSerialization, "bad g_mask_random point");
    if (pos != len) throw SpxError(kSerialization, "trailing bytes in verifier parameter");
    return V;
}
std::vector<uint8_t> vp_serialize(const VP& V) {
    Ser s;
    s.u64((uint64_t)V.nv);
    uint8_t b[192];
    host::g1_to_uncompressed(b, V.g);
    s.raw(b, 96);
    host::g2_to_uncompressed(b, V.h);
    s.raw(b, 192);
    s.u64(V.g_mask.size());
    for (auto& g : V.g_mask) {
        host::g1_to_uncompressed(b, g);
        s.raw(b, 96);
    }
    return s.b;
}
VP vp_from_pp(const PP& P) {
    if (!P.has_t) invalid("verifier parameter needs a keygen-generated PP (trapdoor unknown)");
    VP V;
    V.nv = P.nv;
    V.g = P.g;
    V.h = P.h;
    for (int i = 0; i < P.nv; ++i) {  // setup.rs:91-101: g_mask_random[i] = g^{t_i}
        uint64_t k[4];
        P.t[i].to_canon(k);
        V.g_mask.push_back(host::jac_to_affine(host::jac_mul(host::jac_from(P.g), k)));
    }
    return V;
}

namespace {
struct ProofReader {
    const uint8_t* b;
    size_t len, pos = 0;
    // lazy: points stay bytes (spx_verify_many decompresses a whole batch's points on the GPU); the
    // callers keep each point's offset
    bool lazy = false;
    // strict: the context whose subgroup check is on ("Subgroup membership"). Every point is
    // tested right after it decompresses, as arkworks' checked deserialization does; `field` names the
    // point being read for the error
    Ctx* strict = nullptr;
    std::string field;
    template <class A, class Fn>
    void member(const A& a, Fn&& in_subgroup) {
        if (!strict || lazy) return;
        strict->sgstat[1] += 1;
        if (in_subgroup(a)) return;
        strict->sgstat[2] += 1;
        throw SpxError(kSerialization, field + " is not in the prime-order subgroup");
    }
    const uint8_t* take(size_t k) {
        if (pos + k > len) throw SpxError(kSerialization, "truncated proof");
        const uint8_t* p = b + pos;
        pos += k;
        return p;
    }
    uint64_t u64() {
        uint64_t v;
        memcpy(&v, take(8), 8);
        return v;
    }
    HFr fr() {
        HFr r;
        if (!host::fr_from_bytes(r, take(32))) throw SpxError(kSerialization, "non-canonical field element");
        return r;
    }
    host::Affine<HFq> g1() {
        host::Affine<HFq> a{HFq::zero(), HFq::zero(), false};
        const uint8_t* p = take(48);
        if (!lazy && !host::g1_decompress(a, p)) throw SpxError(kSerialization, "invalid G1 point");
        member(a, host::g1_in_subgroup);
        return a;
    }
    host::Affine<HFq2> g2() {
        host::Affine<HFq2> a{HFq2::zero(), HFq2::zero(), false};
        const uint8_t* p = take(96);
        if (!lazy && !host::g2_decompress(a, p)) throw SpxError(kSerialization, "invalid G2 point");
        member(a, host::g2_in_subgroup);
        return a;
    }
};
struct OpenProof {
    HFr eval;
    host::Affine<HFq2> h;
    std::vector<host::Affine<HFq2>> proofs;
    size_t h_at = 0;             // byte offsets of the compressed points in the proof
    std::vector<size_t> at;
};
OpenProof read_open(ProofReader& R, const char* name) {
    OpenProof o;
    o.eval = R.fr();
    o.h_at = R.pos;
    if (R.strict) R.field = std::string(name) + " h";
    o.h = R.g2();
    const uint64_t k = R.u64();
    if (k > 64) throw SpxError(kSerialization, "bad opening proof length");
    for (uint64_t i = 0; i < k; ++i) {
        o.at.push_back(R.pos);
        if (R.strict) R.field = std::string(name) + " proof point " + std::to_string(i);
        o.proofs.push_back(R.g2());
    }
    return o;
}
std::vector<std::vector<HFr>> read_msgs(ProofReader& R, std::vector<std::pair<size_t, size_t>>& spans) {
    const uint64_t rounds = R.u64();
    if (rounds > 64) throw SpxError(kSerialization, "bad sumcheck round count");
    std::vector<std::vector<HFr>> m(rounds);
    for (auto& e : m) {
        const size_t start = R.pos;
        const uint64_t k = R.u64();
        if (k > 1024) throw SpxError(kSerialization, "bad sumcheck message length");
        for (uint64_t i = 0; i < k; ++i) e.push_back(R.fr());
        spans.emplace_back(start, R.pos - start);
    }
    return m;
}
// linear-sumcheck interpolate_uni_poly: value at x of the polynomial through (i, ev[i]).
// dinv[i] = 1 / prod_{j != i} (i - j): the same for every round of a sumcheck, so one batch inversion
// serves them all (an inversion per term was most of the verifier's host arithmetic)
std::vector<HFr> interpolation_weights(size_t n) {
    std::vector<HFr> den(n, HFr::one());
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j)
            if (j != i) den[i] = den[i] * (HFr::from_u64(i) - HFr::from_u64(j));
    host::batch_inverse(den);
    return den;
}
HFr interpolate(const std::vector<HFr>& ev, const HFr& x, const std::vector<HFr>& dinv) {
    const size_t n = ev.size();
    HFr total = HFr::zero();
    for (size_t i = 0; i < n; ++i) {
        HFr num = HFr::one();
        for (size_t j = 0; j < n; ++j) {
            if (j == i) continue;
            num = num * (x - HFr::from_u64(j));
        }
        total = total + ev[i] * num * dinv[i];
    }
    return total;
}
// linear-sumcheck check_and_generate_subclaim; its errors surface as Error::SumCheckError
HFr check_subclaim(const std::vector<std::vector<HFr>>& msgs, const std::vector<HFr>& rnd, HFr expected, int nv,
                   uint64_t max_mult) {
    if ((int)msgs.size() != nv) throw SpxError(kSumcheck, "insufficient rounds");
    std::vector<HFr> dinv;
    for (size_t i = 0; i < msgs.size(); ++i) {
        if (msgs[i].size() != max_mult + 1) throw SpxError(kSumcheck, "wrong number of evaluations");
        if (!(msgs[i][0] + msgs[i][1] == expected))
            throw SpxError(kSumcheck, "Prover message is not consistent with the claim.");
        if (dinv.empty()) dinv = interpolation_weights(msgs[i].size());
        expected = interpolate(msgs[i], rnd[i], dinv);
    }
    return expected;
}
// MLPolyCommit::verify (verify.rs:12-45), vp.h on the left as in the reference
bool mkzg_check(const VP& V, const host::Affine<HFq>& com, const std::vector<HFr>& point, const HFr& value,
                const OpenProof& op) {
    if ((int)op.proofs.size() < V.nv || (int)point.size() < V.nv) return false;
    using host::jac_add;
    using host::jac_from;
    using host::jac_mul;
    using host::jac_to_affine;
    auto neg = [](host::Affine<HFq> a) {
        a.y = -a.y;
        return a;
    };
    uint64_t k[4];
    value.to_canon(k);
    std::vector<std::pair<host::Affine<HFq>, host::Affine<HFq2>>> pairs;
    pairs.push_back({jac_to_affine(jac_add(jac_from(com), jac_from(neg(jac_to_affine(jac_mul(jac_from(V.g), k)))))),
                     V.h});
    for (int i = 0; i < V.nv; ++i) {
        point[i].to_canon(k);
        host::Affine<HFq> li = jac_to_affine(
            jac_add(jac_from(V.g_mask[i]), jac_from(neg(jac_to_affine(jac_mul(jac_from(V.g), k))))));
        if (!li.inf) li = neg(li);
        pairs.push_back({li, op.proofs[i]});
    }
    return host::pairing_product_is_one(pairs);
}
HFr mle_eval_host(std::vector<HFr> t, const std::vector<HFr>& point) {
    for (const HFr& r : point) {
        std::vector<HFr> nt(t.size() / 2);
        for (size_t b = 0; b < nt.size(); ++b) nt[b] = t[2 * b] + r * (t[2 * b + 1] - t[2 * b]);
        t.swap(nt);
    }
    return t[0];
}
}  // namespace

// sum_M r_M M(r_x, r_y) on the GPU: eq(r_x) table, CSC gather (the prover's eval_on_x pass), L folds
static HFr eval_matrices_at(Ctx& C, Index& I, const std::vector<HFr>& r_x, const HFr rabc[3],
                            const std::vector<HFr>& r_y) {
    const int L = I.log_n;
    const uint64_t n = I.n;
    const uint64_t parts = std::max<uint64_t>(3 * 2048, (uint64_t)I.cols.longc.nchunks);
    C.scratch.ensure(32 * (n + n + n / 2 + 2 + parts + kEqScratch + 4 * L + 8));
    Fr* base = C.scratch.as<Fr>();
    Fr *EQ = base, *M0 = EQ + n, *Mb = M0 + n, *partial = Mb + n / 2 + 2, *eqf = partial + parts;
    Fr* ch = eqf + kEqScratch;  // r_x (L), r_abc (3), r_y (L)
    std::vector<HFr> hch(r_x);
    hch.insert(hch.end(), rabc, rabc + 3);
    hch.insert(hch.end(), r_y.begin(), r_y.end());
    uint8_t* hs = C.pin_at(Ctx::kPinStage, 32 * hch.size(), 64 << 10);
    memcpy(hs, hch.data(), 32 * hch.size());
    SPX_HIP(hipMemcpyAsync(ch, hs, 32 * hch.size(), hipMemcpyHostToDevice, C.stream));
    const ColStreamJob cjob{ch, ch + L, M0, eqf, partial};
    I.cols.launch(1, &cjob, L, C.stream);
    // fold at r_y (variable 0 = LSB): M0 -> EQ (as q scratch) / Mb ping-pong
    const Fr* rin = M0;
    Fr* bufs[2] = {Mb, M0};
    for (int i = 0; i < L; ++i) {
        const uint64_t half = n >> (i + 1);
        Fr* rout = bufs[i & 1];
        launch_open_level(rin, rout, EQ, dev_fr(r_y[i]), half, C.stream);
        rin = rout;
    }
    uint8_t* hp = C.pin_at(Ctx::kPinOpen, 32, 56 << 10);
    SPX_HIP(hipMemcpyAsync(hp, rin, 32, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    return ld_hfr(hp);
}

// ---- the pieces of the verifier, shared by verify() and verify_many()
namespace {
// verifier_init (verifier.rs:143-146)
std::vector<HFr> parse_public(const uint8_t* v, size_t nv, uint64_t n) {
    if (!is_pow2(nv) || nv > n)
        invalid("public input should be power of two and has size smaller than number of constraints");
    std::vector<HFr> vv(nv);
    for (size_t i = 0; i < nv; ++i)
        if (!host::fr_from_bytes(vv[i], v + 32 * i)) invalid("public input is not a canonical field element");
    return vv;
}
// a proof's fields (proof.rs:10-20 field order) with each message's byte span for the transcript
struct ParsedProof {
    size_t pm1_at, pm1_len, pm2_at, pm2_len, pm3_at, pm4_at, pm5_at, pm6_at, pm6_len, com_at;
    uint64_t mm1, nv1, mm2, nv2;
    host::Affine<HFq> com;
    OpenProof op1, op2;
    std::vector<std::vector<HFr>> sc1, sc2;
    std::vector<std::pair<size_t, size_t>> sp1, sp2;
    HFr va, vb, vc;
};
// strict: the context when its subgroup check is on, else null (ProofReader::strict)
ParsedProof parse_proof(const uint8_t* proof, size_t len, bool lazy, Ctx* strict = nullptr) {
    ParsedProof P;
    ProofReader R{proof, len};
    R.lazy = lazy;
    R.strict = strict;
    R.field = "commitment";
    P.pm1_at = R.pos;
    (void)R.u64();  // the commitment's nv
    P.com_at = R.pos;
    P.com = R.g1();
    P.pm1_len = R.pos - P.pm1_at, P.pm2_at = R.pos;
    P.op1 = read_open(R, "opening 1");
    P.pm2_len = R.pos - P.pm2_at, P.pm3_at = R.pos;
    P.mm1 = R.u64(), P.nv1 = R.u64();
    P.sc1 = read_msgs(R, P.sp1);
    P.pm4_at = R.pos;
    P.va = R.fr(), P.vb = R.fr(), P.vc = R.fr();
    P.pm5_at = R.pos;
    P.mm2 = R.u64(), P.nv2 = R.u64();
    P.sc2 = read_msgs(R, P.sp2);
    P.pm6_at = R.pos;
    P.op2 = read_open(R, "opening 2");
    P.pm6_len = R.pos - P.pm6_at;
    if (R.pos != len) throw SpxError(kSerialization, "trailing bytes in proof");
    return P;
}
// the transcript state after A, B, C: the index cache, or a fresh absorption
Blake2s matrices_state(const Index& I, const ProveOpts& o) {
    if (o.cached && I.has_cache) return I.cache;
    Blake2s h;
    for (int m = 0; m < 3; ++m) feed_matrix(h, I.m[m]);
    return h;
}
struct Challenges {
    std::vector<HFr> r_v, tau, rand1, rand2;
    HFr r_a, r_b, r_c;
};
// transcript replay (lib.rs:152-212 feed order) from the state after the matrices
Challenges replay_transcript(const ParsedProof& P, const uint8_t* proof, const uint8_t* v, size_t nv, int L,
                             const Blake2s& mats, const ProveOpts& o) {
    Challenges c;
    Transcript T(o.mode == 1, o.seed);
    T.set_state(mats);
    {
        Ser s;
        s.u64(nv);
        s.raw(v, 32 * nv);
        T.feed(s.b.data(), s.b.size());
    }
    T.feed(proof + P.pm1_at, P.pm1_len);
    c.r_v.resize(ilog2(nv));
    for (auto& r : c.r_v) r = T.rand_fr();
    T.feed(proof + P.pm2_at, P.pm2_len);
    c.tau.resize(L);
    for (auto& t : c.tau) t = T.rand_fr();
    if (P.nv1 != (uint64_t)L) invalid("invalid sumcheck proposal");
    T.feed(proof + P.pm3_at, 16);
    if ((int)P.sc1.size() != L || (int)P.sc2.size() != L) invalid("malformed sumcheck message");
    for (auto& sp : P.sp1) {
        T.feed(proof + sp.first, sp.second);
        c.rand1.push_back(T.rand_fr());
    }
    T.feed(proof + P.pm4_at, 96);
    c.r_a = T.rand_fr(), c.r_b = T.rand_fr(), c.r_c = T.rand_fr();
    if (P.nv2 != (uint64_t)L) invalid("invalid sumcheck proposal");
    T.feed(proof + P.pm5_at, 16);
    for (auto& sp : P.sp2) {
        T.feed(proof + sp.first, sp.second);
        c.rand2.push_back(T.rand_fr());
    }
    T.feed(proof + P.pm6_at, P.pm6_len);
    return c;
}
// the first opening's point: r_v padded with zeros to L variables
std::vector<HFr> padded_r_v(const Challenges& c, int L) {
    std::vector<HFr> r(L, HFr::zero());
    for (size_t i = 0; i < c.r_v.size(); ++i) r[i] = c.r_v[i];
    return r;
}
// verify_sixth_round (verifier.rs:443-512) without its pairing checks and matrix evaluation: the
// public-input MLE, both sumcheck subclaims and the eq(tau, r_x) product. Returns the second
// sumcheck's subclaim, which (A, B, C)(r_x, r_y) z(r_y) must equal.
HFr algebraic_checks(const ParsedProof& P, const Challenges& c, const std::vector<HFr>& vv, int L) {
    if (!(mle_eval_host(vv, c.r_v) == P.op1.eval)) invalid("public witness is inconsistent with proof");
    const HFr expected1 = check_subclaim(P.sc1, c.rand1, HFr::zero(), L, P.mm1);
    HFr eq_rx = HFr::one();
    for (int i = 0; i < L; ++i) eq_rx = eq_rx * eq1(c.tau[i], c.rand1[i]);
    if (!((P.va * P.vb - P.vc) * eq_rx == expected1))
        throw SpxError(kWrongWitness, "first sumcheck has wrong subclaim");
    const HFr claimed2 = c.r_a * P.va + c.r_b * P.vb + c.r_c * P.vc;
    return check_subclaim(P.sc2, c.rand2, claimed2, L, P.mm2);
}
}  // namespace

void verify(Ctx& C, Index& I, const uint8_t* v, size_t nv, const uint8_t* proof, size_t len, const VP& V,
            const ProveOpts& o) {
    if (I.G != 1) invalid("verify needs an index built on a single-rank context");
    const int L = I.log_n;
    const std::vector<HFr> vv = parse_public(v, nv, I.n);
    const ParsedProof P = parse_proof(proof, len, false, C.subgroup_check() ? &C : nullptr);
    const Challenges c = replay_transcript(P, proof, v, nv, L, matrices_state(I, o), o);
    // verify_sixth_round (verifier.rs:443-512)
    if (V.nv != L) invalid("verifier parameter nv != log_n");
    if (!mkzg_check(V, P.com, padded_r_v(c, L), P.op1.eval, P.op1)) invalid("public witness failed in commitment check");
    const HFr expected2 = algebraic_checks(P, c, vv, L);
    const HFr rabc[3] = {c.r_a, c.r_b, c.r_c};
    const HFr actual = eval_matrices_at(C, I, c.rand1, rabc, c.rand2) * P.op2.eval;
    if (!(expected2 == actual)) throw SpxError(kWrongWitness, "Cannot verify matrix A, B, C");
    if (!mkzg_check(V, P.com, c.rand2, P.op2.eval, P.op2)) throw SpxError(kWrongWitness, "Cannot verify z_ry");
}

// ====================================================================== batch verifier
// spx_verify_many: the mKZG checks of every proof of a batch, all under one verifier
// parameter, folded into one product of L + 2 pairings by a random linear combination.
std::vector<uint8_t> verify_many_coeffs(const uint8_t* const* v, const size_t* nv, const uint8_t* const* proofs,
                                        const size_t* lens, int k, const uint8_t* vp, size_t vp_len,
                                        const uint8_t* entropy32) {
    static const char tag[] = "spx-verify-many-v1";
    static const uint8_t zeros[32] = {0};
    Blake2s h;
    h.update(tag, sizeof tag - 1);
    h.update(vp, vp_len);
    h.update(entropy32 ? entropy32 : zeros, 32);
    for (int j = 0; j < k; ++j) {
        const uint64_t a = nv[j], b = lens[j];
        h.update(&a, 8);
        h.update(v[j], 32 * nv[j]);
        h.update(&b, 8);
        h.update(proofs[j], lens[j]);
    }
    uint8_t seed[32];
    h.peek(seed);
    std::vector<uint8_t> out((size_t)64 * k, 0);
    for (uint64_t i = 0; i < (uint64_t)2 * k; ++i) {
        Blake2s g;
        g.update(seed, 32);
        g.update(&i, 8);
        uint8_t d[32];
        g.peek(d);
        uint8_t* r = out.data() + 32 * i;
        memcpy(r, d, 16);  // the low 128 bits
        bool zero = true;
        for (int t = 0; t < 16; ++t) zero &= r[t] == 0;
        if (zero) r[0] = 1;
    }
    return out;
}

namespace {
// one bump allocation over a device buffer and its pinned host mirror
struct Mirror {
    uint8_t *d, *h;
    size_t pos = 0;
    size_t take(size_t bytes) {
        const size_t at = pos;
        pos += (bytes + 255) & ~(size_t)255;
        return at;
    }
};
template <class F>
host::Affine<F> aff_from_dev(const uint8_t* p) {  // device affine Montgomery ((0, 0) = infinity) -> host
    host::Affine<F> a;
    memcpy(&a.x, p, sizeof(F));
    memcpy(&a.y, p + sizeof(F), sizeof(F));
    a.inf = a.x.is_zero() && a.y.is_zero();
    return a;
}
void fr_canon_to(uint8_t* out, const HFr& x) {
    uint64_t c[4];
    x.to_canon(c);
    memcpy(out, c, 32);
}
}  // namespace

void PinBuf::ensure(size_t b) {
    if (b <= bytes) return;
    if (p) (void)hipHostFree(p);
    p = nullptr, bytes = 0;
    SPX_HIP(hipHostMalloc(&p, b, hipHostMallocDefault));
    bytes = b;
}
PinBuf::~PinBuf() {
    if (p) (void)hipHostFree(p);
}

void verify_many(Ctx& C, Index& I, const uint8_t* const* v, const size_t* nv, const uint8_t* const* proofs,
                 const size_t* lens, int k, const VP& V, const uint8_t* vp, size_t vp_len, const ProveOpts& o,
                 const uint8_t* entropy32, std::vector<int>& status, std::vector<std::string>& msgs) {
    if (I.G != 1) invalid("verify needs an index built on a single-rank context");
    const int L = I.log_n;
    const bool strict = C.subgroup_check();  // the single-proof path reads the same setting
    status.assign(k, kOk);
    msgs.assign(k, std::string());
    struct Item {
        bool live = true;
        std::vector<HFr> vv;
        ParsedProof P;
        Challenges c;
        HFr expected2;
        HFr rho[2];
    };
    std::vector<Item> it(k);
    // host wall time of the phases, for spx_last_timings: parse and replay, points queued and algebraic
    // checks, the wait for the decompression, matrix evaluations, combinations, pairing, single-proof path
    C.timings.clear();
    Timer tph;
    auto mark = [&](const char* name) {
        C.timings.emplace_back(name, tph.us());
        tph = Timer();
    };
    // (a) parse and replay; the matrices' transcript state once per call
    {
        Blake2s mats;
        bool have = false;
        for (int j = 0; j < k; ++j) {
            Item& t = it[j];
            try {
                t.vv = parse_public(v[j], nv[j], I.n);
                t.P = parse_proof(proofs[j], lens[j], true);
                if (!have && o.mode != 1) mats = matrices_state(I, o);
                have = true;
                t.c = replay_transcript(t.P, proofs[j], v[j], nv[j], L, mats, o);
                // the batch's shape: L quotient points per opening under a verifier parameter of L variables
                if (V.nv != L || (int)t.P.op1.at.size() != L || (int)t.P.op2.at.size() != L) t.live = false;
            } catch (const SpxError&) {
                t.live = false;
            }
        }
    }
    mark("vm_parse_replay");
    std::vector<int> batch;  // the proofs whose points go to the GPU
    for (int j = 0; j < k; ++j)
        if (it[j].live) batch.push_back(j);
    const size_t nb = batch.size(), m = 2 * nb, n1 = nb, nq = (size_t)L * m, n2 = nq + m;
    if (nb) {
        // (d) first half: all points of the batch to the GPU, one launch per curve. G2 order: level i of
        // opening o at i m + o (the A_i are segments, B is the whole run), then the openings' h points.
        Mirror M{nullptr, nullptr};
        // strict: a second run of n1 + n2 flags behind the decompression's, the membership kernels'
        const size_t nok = strict ? 2 * (n1 + n2) : n1 + n2;
        const size_t cin1 = M.take(48 * n1), cin2 = M.take(96 * n2), okb = M.take(nok);
        const size_t sc1 = M.take(32 * (n1 + 1)), scA = M.take(32 * nq), scB = M.take(32 * nq);
        const size_t seg = M.take(8 * (L + 1 + 4)), gpt = M.take(96);
        const size_t outs = M.take(192 * (L + 1) + 96);
        const size_t mirrored = M.pos;
        const size_t pts1 = M.take(96 * (n1 + 1)), pts2 = M.take(192 * n2);
        const size_t tmp = M.take(std::max(lincomb_tmp_bytes(true, nq), lincomb_tmp_bytes(false, n1 + 1)));
        C.vdev.ensure(M.pos);
        C.vpin.ensure(mirrored);
        M.d = C.vdev.as<uint8_t>();
        M.h = static_cast<uint8_t*>(C.vpin.p);
        for (size_t b = 0; b < nb; ++b) {
            const int j = batch[b];
            const ParsedProof& P = it[j].P;
            memcpy(M.h + cin1 + 48 * b, proofs[j] + P.com_at, 48);
            for (int op = 0; op < 2; ++op) {
                const OpenProof& O = op ? P.op2 : P.op1;
                const size_t oi = 2 * b + op;
                for (int i = 0; i < L; ++i) memcpy(M.h + cin2 + 96 * ((size_t)i * m + oi), proofs[j] + O.at[i], 96);
                memcpy(M.h + cin2 + 96 * (nq + oi), proofs[j] + O.h_at, 96);
            }
        }
        SPX_HIP(hipMemcpyAsync(M.d + cin1, M.h + cin1, cin2 + 96 * n2 - cin1, hipMemcpyHostToDevice, C.stream));
        launch_decompress_g1(M.d + cin1, n1, reinterpret_cast<G1Aff*>(M.d + pts1), M.d + okb, C.stream);
        launch_decompress_g2(M.d + cin2, n2, reinterpret_cast<G2Aff*>(M.d + pts2), M.d + okb + n1, C.stream);
        if (strict) {  // on the points where they lie, behind their decompression on the same stream
            launch_in_subgroup_g1(reinterpret_cast<const G1Aff*>(M.d + pts1), n1, M.d + okb + n1 + n2, C.stream);
            launch_in_subgroup_g2(reinterpret_cast<const G2Aff*>(M.d + pts2), n2, M.d + okb + n1 + n2 + n1, C.stream);
            C.sgstat[0] += n1 + n2;
        }
        SPX_HIP(hipMemcpyAsync(M.h + okb, M.d + okb, nok, hipMemcpyDeviceToHost, C.stream));
        C.vstat[3] += n1 + n2;
        // (b) the algebraic checks, on the host while the points decompress
        for (int j : batch) {
            try {
                it[j].expected2 = algebraic_checks(it[j].P, it[j].c, it[j].vv, L);
            } catch (const SpxError&) {
                it[j].live = false;
            }
        }
        mark("vm_algebra");
        C.sync();
        for (size_t b = 0; b < nb; ++b) {
            bool ok = M.h[okb + b] != 0;
            for (int op = 0; op < 2; ++op) {
                const size_t oi = 2 * b + op;
                for (int i = 0; i <= L; ++i) ok &= M.h[okb + n1 + (size_t)i * m + oi] != 0;
            }
            // a point outside the subgroup leaves the batch as one that failed decompression does (the
            // flags of the membership kernels have the decompression's layout)
            if (strict) {
                const size_t q = n1 + n2;
                ok &= M.h[okb + q + b] != 0;
                for (int op = 0; op < 2; ++op)
                    for (int i = 0; i <= L; ++i) ok &= M.h[okb + q + n1 + (size_t)i * m + 2 * b + op] != 0;
            }
            if (!ok) it[batch[b]].live = false;
        }
        mark("vm_points_wait");
        // (c) the matrix evaluations
        for (int j : batch) {
            if (!it[j].live) continue;
            const Challenges& c = it[j].c;
            const HFr rabc[3] = {c.r_a, c.r_b, c.r_c};
            const HFr actual = eval_matrices_at(C, I, c.rand1, rabc, c.rand2) * it[j].P.op2.eval;
            if (!(it[j].expected2 == actual)) it[j].live = false;
        }
        mark("vm_matrix_eval");
        // (d) second half: the combinations. A proof that left the batch keeps its slots with zero scalars.
        const std::vector<uint8_t> rho = verify_many_coeffs(v, nv, proofs, lens, k, vp, vp_len, entropy32);
        size_t nlive = 0;
        HFr vsum = HFr::zero();
        memset(M.h + sc1, 0, scB + 32 * nq - sc1);
        for (size_t b = 0; b < nb; ++b) {
            Item& t = it[batch[b]];
            if (!t.live) continue;
            ++nlive;
            for (int op = 0; op < 2; ++op) {
                uint64_t c4[4] = {0, 0, 0, 0};
                memcpy(c4, rho.data() + 32 * (2 * (size_t)batch[b] + op), 16);
                t.rho[op] = HFr::from_canon(c4);
                const OpenProof& O = op ? t.P.op2 : t.P.op1;
                vsum = vsum + t.rho[op] * O.eval;
                const std::vector<HFr> z = op ? t.c.rand2 : padded_r_v(t.c, L);
                const size_t oi = 2 * b + op;
                for (int i = 0; i < L; ++i) {
                    memcpy(M.h + scA + 32 * ((size_t)i * m + oi), c4, 32);
                    fr_canon_to(M.h + scB + 32 * ((size_t)i * m + oi), t.rho[op] * z[i]);
                }
            }
            fr_canon_to(M.h + sc1 + 32 * b, t.rho[0] + t.rho[1]);
        }
        if (nlive) {
            fr_canon_to(M.h + sc1 + 32 * n1, HFr::zero() - vsum);
            uint64_t* so = reinterpret_cast<uint64_t*>(M.h + seg);
            for (int i = 0; i <= L; ++i) so[i] = (uint64_t)i * m;  // the A_i
            so[L + 1] = 0, so[L + 2] = nq;                         // B
            so[L + 3] = 0, so[L + 4] = n1 + 1;                     // C
            memset(M.h + gpt, 0, 96);
            if (!V.g.inf) {
                memcpy(M.h + gpt, &V.g.x, 48);
                memcpy(M.h + gpt + 48, &V.g.y, 48);
            }
            SPX_HIP(hipMemcpyAsync(M.d + sc1, M.h + sc1, gpt + 96 - sc1, hipMemcpyHostToDevice, C.stream));
            SPX_HIP(hipMemcpyAsync(M.d + pts1 + 96 * n1, M.d + gpt, 96, hipMemcpyDeviceToDevice, C.stream));
            const uint64_t* dso = reinterpret_cast<const uint64_t*>(M.d + seg);
            G2Aff* outA = reinterpret_cast<G2Aff*>(M.d + outs);
            G1Aff* outC = reinterpret_cast<G1Aff*>(M.d + outs + 192 * (L + 1));
            launch_lincomb_g2(reinterpret_cast<const G2Aff*>(M.d + pts2), reinterpret_cast<const Fr*>(M.d + scA), nq, dso,
                              (uint32_t)L, outA, M.d + tmp, C.stream);
            launch_lincomb_g2(reinterpret_cast<const G2Aff*>(M.d + pts2), reinterpret_cast<const Fr*>(M.d + scB), nq,
                              dso + L + 1, 1, outA + L, M.d + tmp, C.stream);
            launch_lincomb_g1(reinterpret_cast<const G1Aff*>(M.d + pts1), reinterpret_cast<const Fr*>(M.d + sc1), n1 + 1,
                              dso + L + 3, 1, outC, M.d + tmp, C.stream);
            SPX_HIP(hipMemcpyAsync(M.h + outs, M.d + outs, 192 * (L + 1) + 96, hipMemcpyDeviceToHost, C.stream));
            C.sync();
            mark("vm_combine");
            // e(C, h) e(g, B) prod_i e(-g_mask_i, A_i) == 1
            std::vector<std::pair<host::Affine<HFq>, host::Affine<HFq2>>> pairs;
            pairs.push_back({aff_from_dev<HFq>(M.h + outs + 192 * (L + 1)), V.h});
            pairs.push_back({V.g, aff_from_dev<HFq2>(M.h + outs + 192 * L)});
            for (int i = 0; i < L; ++i) {
                host::Affine<HFq> gm = V.g_mask[i];
                if (!gm.inf) gm.y = -gm.y;
                pairs.push_back({gm, aff_from_dev<HFq2>(M.h + outs + 192 * i)});
            }
            C.vstat[0] += 1;
            C.vstat[1] += pairs.size();
            bool one = false;
            try {
                one = host::pairing_product_is_one(pairs);
            } catch (const std::runtime_error&) {  // a degenerate Miller step: settle each proof alone
                one = false;
            }
            if (!one)
                for (int j : batch) it[j].live = false;
            mark("vm_pairing");
        }
    }
    // every proof that left the fast path takes the single-proof path, which names its error
    tph = Timer();
    for (int j = 0; j < k; ++j) {
        if (it[j].live) continue;
        C.vstat[2] += 1;
        try {
            verify(C, I, v[j], nv[j], proofs[j], lens[j], V, o);
        } catch (const SpxError& e) {
            status[j] = e.code;
            msgs[j] = e.what();
        } catch (const std::bad_alloc&) {
            throw;
        } catch (const std::exception& e) {
            status[j] = kDevice;
            msgs[j] = e.what();
        }
    }
    while (C.timings.size() < 6) C.timings.emplace_back("vm_not_run", 0.0);  // fixed positions
    mark("vm_single_path");
}

// ---- kernel-level entries of the batch verifier's kernels (parity tests)
void k_decompress(Ctx& C, bool g2, const uint8_t* in, size_t n, uint8_t* out, uint8_t* ok, bool bulk) {
    if (n == 0) invalid("no points");
    const size_t cs = g2 ? 96 : 48, ps = 2 * cs;
    DevMem din(cs * n), pts(ps * n), dok(n);
    EventPair ev;  // the decompression kernel alone, for spx_last_timings
    SPX_HIP(hipMemcpyAsync(din.p, in, cs * n, hipMemcpyHostToDevice, C.stream));
    DevMem err(sizeof(unsigned long long));  // the loader's report (bulk kernels); this entry answers per point
    SPX_HIP(hipMemsetAsync(err.p, 0xff, sizeof(unsigned long long), C.stream));
    SPX_HIP(hipEventRecord(ev.a, C.stream));
    if (bulk) {
        if (g2)
            launch_decompress_bulk_g2(din.as<uint8_t>(), n, pts.as<G2Aff>(), 0, err.as<unsigned long long>(),
                                      dok.as<uint8_t>(), C.stream);
        else
            launch_decompress_bulk_g1(din.as<uint8_t>(), n, pts.as<G1Aff>(), 0, err.as<unsigned long long>(),
                                      dok.as<uint8_t>(), C.stream);
    } else if (g2) {
        launch_decompress_g2(din.as<uint8_t>(), n, pts.as<G2Aff>(), dok.as<uint8_t>(), C.stream);
    } else {
        launch_decompress_g1(din.as<uint8_t>(), n, pts.as<G1Aff>(), dok.as<uint8_t>(), C.stream);
    }
    SPX_HIP(hipEventRecord(ev.b, C.stream));
    if (g2)
        launch_points_to_canon_g2(pts.as<G2Aff>(), n, C.stream);
    else
        launch_points_to_canon_g1(pts.as<G1Aff>(), n, C.stream);
    SPX_HIP(hipMemcpyAsync(out, pts.p, ps * n, hipMemcpyDeviceToHost, C.stream));
    SPX_HIP(hipMemcpyAsync(ok, dok.p, n, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    C.timings.clear();
    C.timings.emplace_back(bulk ? "decompress_bulk_kernel" : "decompress_kernel", 1000.0 * ev.ms());
    for (size_t j = 0; j < n; ++j) {  // infinity carries the ark flag; a rejected point stays all zero
        uint8_t* p = out + ps * j;
        bool zero = true;
        for (size_t t = 0; t < ps; ++t) zero &= p[t] == 0;
        if (zero && ok[j]) {
            p[cs] = 1;  // y = 1
            p[ps - 1] |= host::kFlagInf;
        }
    }
}
// n uncompressed ark points -> compressed bytes through the serializer's kernel
void k_compress(Ctx& C, bool g2, const uint8_t* in, size_t n, uint8_t* out) {
    if (n == 0) invalid("no points");
    const size_t cs = g2 ? 96 : 48, ps = 2 * cs;
    DevMem pts(ps * n), dout(cs * n), err(sizeof(int));
    EventPair ev;
    SPX_HIP(hipMemsetAsync(err.p, 0, sizeof(int), C.stream));
    SPX_HIP(hipMemcpyAsync(pts.p, in, ps * n, hipMemcpyHostToDevice, C.stream));
    if (g2)
        launch_points_from_bytes_g2(pts.as<G2Aff>(), n, err.as<int>(), C.stream);
    else
        launch_points_from_bytes_g1(pts.as<G1Aff>(), n, err.as<int>(), C.stream);
    SPX_HIP(hipEventRecord(ev.a, C.stream));
    if (g2)
        launch_compress_g2(pts.as<G2Aff>(), n, dout.as<uint8_t>(), C.stream);
    else
        launch_compress_g1(pts.as<G1Aff>(), n, dout.as<uint8_t>(), C.stream);
    SPX_HIP(hipEventRecord(ev.b, C.stream));
    int herr = 0;
    SPX_HIP(hipMemcpyAsync(&herr, err.p, sizeof(int), hipMemcpyDeviceToHost, C.stream));
    SPX_HIP(hipMemcpyAsync(out, dout.p, cs * n, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    if (herr & 1) throw SpxError(kSerialization, "non-canonical coordinate");
    if (herr & 2) throw SpxError(kSerialization, "point not on the curve");
    C.timings.clear();
    C.timings.emplace_back("compress_kernel", 1000.0 * ev.ms());
}
// A VerifierParameter between the two wire forms (nv, g, h, u64 count, g_mask_random), on the host
std::vector<uint8_t> vp_convert(const uint8_t* b, size_t len, bool to_compressed) {
    const size_t g1_in = to_compressed ? 96 : 48;
    size_t pos = 0;
    auto take = [&](size_t k) {
        if (k > len - pos) throw SpxError(kSerialization, "truncated verifier parameter");
        const uint8_t* p = b + pos;
        pos += k;
        return p;
    };
    Ser s;
    uint8_t buf[192];
    auto g1 = [&](const char* what) {
        const uint8_t* p = take(g1_in);
        host::Affine<host::Fq> a;
        if (to_compressed) {
            if (!host::g1_from_uncompressed(a, p)) throw SpxError(kSerialization, std::string("bad ") + what);
            host::g1_compress(buf, a);
        } else {
            if (const uint32_t r = point_reject_reason(p, false))
                throw SpxError(kSerialization, std::string(what) + ": " + codec_reason(r));
            host::g1_decompress(a, p);
            host::g1_to_uncompressed(buf, a);
        }
        s.raw(buf, to_compressed ? 48 : 96);
    };
    uint64_t nv, cnt;
    memcpy(&nv, take(8), 8);
    if (nv > (uint64_t)kMaxLogN) throw SpxError(kSerialization, "bad verifier parameter nv (<= 26 supported)");
    s.u64(nv);
    g1("g");
    {
        const uint8_t* p = take(2 * g1_in);
        host::Affine<host::Fq2> a;
        if (to_compressed) {
            if (!host::g2_from_uncompressed(a, p)) throw SpxError(kSerialization, "bad h");
            host::g2_compress(buf, a);
        } else {
            if (const uint32_t r = point_reject_reason(p, true)) throw SpxError(kSerialization, std::string("h: ") + codec_reason(r));
            host::g2_decompress(a, p);
            host::g2_to_uncompressed(buf, a);
        }
        s.raw(buf, to_compressed ? 96 : 192);
    }
    memcpy(&cnt, take(8), 8);
    if (cnt != nv) throw SpxError(kSerialization, "g_mask_random length != nv");
    s.u64(cnt);
    for (uint64_t i = 0; i < cnt; ++i) g1("g_mask_random point");
    if (pos != len) throw SpxError(kSerialization, "trailing bytes in verifier parameter");
    return s.b;
}
void k_lincomb(Ctx& C, bool g2, const uint8_t* bases, const uint8_t* scalars, size_t n, const uint64_t* seg_off,
               size_t nseg, uint8_t* out) {
    if (n == 0 || nseg == 0) invalid("empty linear combination");
    if (seg_off[0] != 0 || seg_off[nseg] != n) invalid("segment offsets must run from 0 to n");
    for (size_t s = 0; s < nseg; ++s)
        if (seg_off[s] > seg_off[s + 1]) invalid("segment offsets must ascend");
    for (size_t i = 0; i < n; ++i) {
        uint64_t c[4];
        memcpy(c, scalars + 32 * i, 32);
        if (HFr::geq_p(c)) throw SpxError(kSerialization, "non-canonical scalar");
    }
    const size_t ps = g2 ? 192 : 96;
    DevMem raw(ps * n), sc(32 * n), so(8 * (nseg + 1)), res(ps * nseg), tmp(lincomb_tmp_bytes(g2, n)), err(sizeof(int));
    SPX_HIP(hipMemsetAsync(err.p, 0, 4, C.stream));
    SPX_HIP(hipMemcpyAsync(raw.p, bases, ps * n, hipMemcpyHostToDevice, C.stream));
    SPX_HIP(hipMemcpyAsync(sc.p, scalars, 32 * n, hipMemcpyHostToDevice, C.stream));
    SPX_HIP(hipMemcpyAsync(so.p, seg_off, 8 * (nseg + 1), hipMemcpyHostToDevice, C.stream));
    if (g2) {
        launch_points_from_bytes_g2(raw.as<G2Aff>(), n, err.as<int>(), C.stream);
        launch_lincomb_g2(raw.as<G2Aff>(), sc.as<Fr>(), n, so.as<uint64_t>(), (uint32_t)nseg, res.as<G2Aff>(), tmp.p, C.stream);
        launch_points_to_canon_g2(res.as<G2Aff>(), nseg, C.stream);
    } else {
        launch_points_from_bytes_g1(raw.as<G1Aff>(), n, err.as<int>(), C.stream);
        launch_lincomb_g1(raw.as<G1Aff>(), sc.as<Fr>(), n, so.as<uint64_t>(), (uint32_t)nseg, res.as<G1Aff>(), tmp.p, C.stream);
        launch_points_to_canon_g1(res.as<G1Aff>(), nseg, C.stream);
    }
    int herr = 0;
    SPX_HIP(hipMemcpyAsync(out, res.p, ps * nseg, hipMemcpyDeviceToHost, C.stream));
    SPX_HIP(hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    if (herr & 1) throw SpxError(kSerialization, "non-canonical input");
    if (herr & 2) throw SpxError(kSerialization, "base point not on the curve");
    for (size_t s = 0; s < nseg; ++s) {
        uint8_t* p = out + ps * s;
        bool zero = true;
        for (size_t t = 0; t < ps; ++t) zero &= p[t] == 0;
        if (zero) {
            p[ps / 2] = 1;
            p[ps - 1] |= host::kFlagInf;
        }
    }
}

// ---- subgroup membership: the kernel-level entry and the public-parameter check
void k_in_subgroup(Ctx& C, bool g2, const uint8_t* pts, size_t n, uint8_t* ok) {
    if (n == 0) invalid("no points");
    // the encoding and the curve equation on the host, point by point (the kernel takes points on the
    // curve); a point that fails either goes up as the infinity sentinel and is reported 0
    const size_t ps = g2 ? 192 : 96;
    std::vector<uint8_t> mont(ps * n, 0), valid(n, 1);
    for (size_t j = 0; j < n; ++j) {
        uint8_t* d = mont.data() + ps * j;
        if (g2) {
            host::Affine<HFq2> a;
            valid[j] = host::g2_from_uncompressed(a, pts + ps * j) && host::on_curve(a);
            if (valid[j] && !a.inf) memcpy(d, &a.x, 96), memcpy(d + 96, &a.y, 96);
        } else {
            host::Affine<HFq> a;
            valid[j] = host::g1_from_uncompressed(a, pts + ps * j) && host::on_curve(a);
            if (valid[j] && !a.inf) memcpy(d, &a.x, 48), memcpy(d + 48, &a.y, 48);
        }
    }
    DevMem dp(ps * n), dok(n);
    SPX_HIP(hipMemcpyAsync(dp.p, mont.data(), ps * n, hipMemcpyHostToDevice, C.stream));
    if (g2)
        launch_in_subgroup_g2(dp.as<G2Aff>(), n, dok.as<uint8_t>(), C.stream);
    else
        launch_in_subgroup_g1(dp.as<G1Aff>(), n, dok.as<uint8_t>(), C.stream);
    SPX_HIP(hipMemcpyAsync(ok, dok.p, n, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    uint64_t rejected = 0;
    for (size_t j = 0; j < n; ++j) {
        ok[j] = ok[j] && valid[j] ? 1 : 0;
        rejected += !ok[j];
    }
    C.sgstat[0] += n;
    C.sgstat[2] += rejected;
}

PPSubgroupReport pp_check_subgroup(Ctx& C, const PP& P) {
    const int nv = P.nv;
    const uint64_t tot = P.lvl_off[nv];
    // every raw level of a curve in one launch (the levels are contiguous), then the count of the
    // rejected points and the lowest one's index
    DevMem ok(2 * tot), res(32);
    const uint64_t init[4] = {0, ~0ull, 0, ~0ull};
    uint64_t got[4];
    SPX_HIP(hipMemcpyAsync(res.p, init, 32, hipMemcpyHostToDevice, C.stream));
    launch_in_subgroup_g1(P.g1_raw(), tot, ok.as<uint8_t>(), C.stream);
    launch_in_subgroup_g2(P.g2_raw(), tot, ok.as<uint8_t>() + tot, C.stream);
    launch_ok_scan(ok.as<uint8_t>(), tot, res.as<uint64_t>(), C.stream);
    launch_ok_scan(ok.as<uint8_t>() + tot, tot, res.as<uint64_t>() + 2, C.stream);
    SPX_HIP(hipMemcpyAsync(got, res.p, 32, hipMemcpyDeviceToHost, C.stream));
    // g and h on the host meanwhile
    const bool g_ok = host::on_curve(P.g) && host::g1_in_subgroup(P.g);
    const bool h_ok = host::on_curve(P.h) && host::g2_in_subgroup(P.h);
    C.sync();
    PPSubgroupReport r;
    r.bad = got[0] + got[2] + !g_ok + !h_ok;
    C.sgstat[0] += 2 * tot;
    C.sgstat[1] += 2;
    C.sgstat[2] += r.bad;
    if (!r.bad) return r;
    // the lowest offender in the order G1 levels, G2 levels, g, h
    auto level_of = [&](uint64_t idx) {
        int i = 0;
        while (idx >= P.lvl_off[i + 1]) ++i;
        return i;
    };
    if (got[0] || got[2]) {
        const int c = got[0] ? 0 : 1;
        const uint64_t idx = got[2 * c + 1];
        const int lvl = level_of(idx);
        r.first[0] = (uint64_t)c + 1, r.first[1] = (uint64_t)lvl, r.first[2] = idx - P.lvl_off[lvl];
        r.message = std::string(c ? "powers_of_h" : "powers_of_g") + " level " + std::to_string(lvl) + " index " + std::to_string(r.first[2]);
    } else {
        r.first[0] = g_ok ? 2 : 1, r.first[1] = ~0ull, r.first[2] = 0;
        r.message = g_ok ? "h" : "g";
    }
    r.message = "public parameter point outside the prime-order subgroup: " + r.message + " (" +
                std::to_string(r.bad) + " such point" + (r.bad == 1 ? "" : "s") + ")";
    return r;
}

// ---- public-parameter structure, derived verifier parameter, views
VP pp_derive_vp(Ctx& C, const PP& P) {
    const int nv = P.nv;
    const uint32_t nblk = odd_sum_blocks(nv);
    DevMem part(sizeof(G1Xyzz) * nv * nblk), out(sizeof(G1Xyzz) * nv);
    launch_odd_sum_g1(P.g1_raw(), nv, part.as<G1Xyzz>(), out.as<G1Xyzz>(), C.stream);
    std::vector<uint8_t> h(out.bytes);
    SPX_HIP(hipMemcpyAsync(h.data(), out.p, out.bytes, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    VP V;
    V.nv = nv;
    V.g = P.g;
    V.h = P.h;
    for (int i = 0; i < nv; ++i)
        V.g_mask.push_back(host::jac_to_affine(xyzz_bytes_to_jac<HFq>(h.data() + sizeof(G1Xyzz) * i)));
    return V;
}

bool pc_verify(const VP& V, const uint8_t com56[56], const uint8_t* point, int nv, const uint8_t value[32],
               const uint8_t* proof, size_t proof_len) {
    if (nv != V.nv) invalid("point length != nv of the verifier parameter");
    if (proof_len != 96 + 8 + (size_t)96 * nv) invalid("opening proof length != 96 + 8 + 96 nv");
    uint64_t cnv;
    memcpy(&cnv, com56, 8);
    if (cnv != (uint64_t)nv) invalid("commitment nv != nv of the verifier parameter");
    host::Affine<HFq> com{HFq::zero(), HFq::zero(), false};
    if (!host::g1_decompress(com, com56 + 8)) throw SpxError(kSerialization, "invalid G1 point");
    std::vector<HFr> pt(nv);
    for (int i = 0; i < nv; ++i)
        if (!host::fr_from_bytes(pt[i], point + 32 * i)) throw SpxError(kSerialization, "non-canonical point");
    HFr val;
    if (!host::fr_from_bytes(val, value)) throw SpxError(kSerialization, "non-canonical field element");
    ProofReader R{proof, proof_len};
    OpenProof op;
    op.eval = val;
    op.h = R.g2();
    if (R.u64() != (uint64_t)nv) throw SpxError(kSerialization, "bad opening proof length");
    for (int i = 0; i < nv; ++i) op.proofs.push_back(R.g2());
    return mkzg_check(V, com, pt, val, op);
}

template <class A, class F>
static A dev_affine(const Affine<F>& a) {  // infinity: the (0, 0) sentinel
    static_assert(sizeof(A) == 2 * sizeof(F), "layout");
    A d;
    memset(&d, 0, sizeof(A));
    if (!a.inf) {
        memcpy((uint8_t*)&d, &a.x, sizeof(F));
        memcpy((uint8_t*)&d + sizeof(F), &a.y, sizeof(F));
    }
    return d;
}

PPStructureReport pp_check_structure(Ctx& C, PP& P, const uint8_t* entropy32) {
    const int nv = P.nv;
    const uint64_t pairs = P.lvl_off[nv] / 2;
    PPStructureReport r;
    Timer t1;
    {
        // every pair of every level of a curve in one launch (the levels are contiguous), then the count
        // of the failing pairs and the lowest one's flat index
        DevMem ok(2 * pairs), res(32);
        const uint64_t init[4] = {0, ~0ull, 0, ~0ull};
        uint64_t got[4];
        SPX_HIP(hipMemcpyAsync(res.p, init, 32, hipMemcpyHostToDevice, C.stream));
        hipEvent_t ev[2];  // device time of the two fold kernels (tools/pp_bench.py)
        SPX_HIP(hipEventCreate(&ev[0]));
        SPX_HIP(hipEventCreate(&ev[1]));
        SPX_HIP(hipEventRecord(ev[0], C.stream));
        launch_fold_check_g1(P.g1_raw(), nv, dev_affine<G1Aff>(P.g), ok.as<uint8_t>(), C.stream);
        launch_fold_check_g2(P.g2_raw(), nv, dev_affine<G2Aff>(P.h), ok.as<uint8_t>() + pairs, C.stream);
        SPX_HIP(hipEventRecord(ev[1], C.stream));
        launch_ok_scan(ok.as<uint8_t>(), pairs, res.as<uint64_t>(), C.stream);
        launch_ok_scan(ok.as<uint8_t>() + pairs, pairs, res.as<uint64_t>() + 2, C.stream);
        SPX_HIP(hipMemcpyAsync(got, res.p, 32, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        float kms = 0;
        (void)hipEventElapsedTime(&kms, ev[0], ev[1]);
        (void)hipEventDestroy(ev[0]);
        (void)hipEventDestroy(ev[1]);
        r.fold_kernel_ms = kms;
        r.bad = got[0] + got[2];
        if (r.bad) {
            const int c = got[0] ? 0 : 1;
            const uint64_t j = got[2 * c + 1];  // flat pair index: level i starts at pair lvl_off[i] / 2
            int lvl = 0;
            while (2 * j >= P.lvl_off[lvl + 1]) ++lvl;
            const uint64_t b = j - P.lvl_off[lvl] / 2;
            r.first[0] = (uint64_t)c + 1, r.first[1] = (uint64_t)lvl, r.first[2] = b;
            r.message = std::string(c ? "powers_of_h" : "powers_of_g") + " level " + std::to_string(lvl) + " pair " +
                        std::to_string(b) + ": points " + std::to_string(2 * b) + " + " + std::to_string(2 * b + 1) + " != " +
                        (lvl + 1 < nv ? "level " + std::to_string(lvl + 1) + " point " + std::to_string(b)
                                      : std::string(c ? "h" : "g")) +
                        " (" + std::to_string(r.bad) + " such pair" + (r.bad == 1 ? "" : "s") + ")";
        }
    }
    r.stage_ms[0] = t1.us() / 1000.0;
    if (r.bad) return r;
    // Stage 2: the opening identity for a pseudo-random table at a pseudo-random point, under the derived VP.
    // Four SplitMix64 streams, one per limb, each seeded with a word of the entropy.
    Timer t2;
    SplitMix64 rng[4];
    for (int k = 0; k < 4; ++k) {
        uint64_t w = 0x5350585f50505f32ULL * (k + 1);
        if (entropy32) memcpy(&w, entropy32 + 8 * k, 8), w ^= 0x9E3779B97F4A7C15ULL * (k + 1);
        rng[k].s = w;
    }
    auto next_fr = [&](uint8_t* out) {
        for (;;) {
            uint64_t c[4] = {rng[0].next(), rng[1].next(), rng[2].next(), rng[3].next() & 0x3FFFFFFFFFFFFFFFULL};
            if (!HFr::geq_p(c)) {
                memcpy(out, c, 32);
                return;
            }
        }
    };
    const uint64_t n = 1ull << nv;
    std::vector<uint8_t> table(32 * n), point(32 * nv);
    for (int i = 0; i < nv; ++i) next_fr(point.data() + 32 * i);
    for (uint64_t x = 0; x < n; ++x) next_fr(table.data() + 32 * x);
    const std::vector<uint8_t> com = k_commit(C, P, table.data(), nv);
    const std::vector<uint8_t> op = k_open(C, P, table.data(), nv, point.data());
    const VP V = pp_derive_vp(C, P);
    r.opening_ok = pc_verify(V, com.data(), point.data(), nv, op.data(), op.data() + 32, op.size() - 32) ? 1 : 0;
    if (!r.opening_ok) r.message = "opening self-test failed";
    r.stage_ms[1] = t2.us() / 1000.0;
    return r;
}

std::unique_ptr<PP> pp_view(Ctx& C, const PP& parent, int nv) {
    if (nv < 1 || nv > parent.nv) invalid("view: nv out of range (1 .. the parent's nv)");
    if (C.device != parent.store->device) invalid("view: the context is on another device than the public parameter");
    const int k = parent.nv - nv;
    auto V = std::make_unique<PP>();
    V->nv = nv;
    V->store = parent.store;
    V->raw_base = parent.raw_base + parent.lvl_off[k];
    V->lvl_off.resize(nv + 1);
    for (int i = 0; i <= nv; ++i) V->lvl_off[i] = parent.lvl_off[k + i] - parent.lvl_off[k];
    V->g = parent.g;
    V->h = parent.h;
    V->g2_off.assign(parent.g2_off.begin() + k, parent.g2_off.end());
    V->g2_c.assign(parent.g2_c.begin() + k, parent.g2_c.end());
    V->g2_W.assign(parent.g2_W.begin() + k, parent.g2_W.end());
    // the shared levels keep the root's window bits: a batch of them has no more buckets than the root's
    uint64_t buckets = 0;
    for (int i = 0; i < nv; ++i) buckets += 1ull << (V->g2_c[i] - 1);
    if (buckets > kMsmMaxBuckets) invalid("view: the shared levels' buckets exceed the MSM sort's bins");
    V->has_t = parent.has_t;
    if (parent.has_t) V->t.assign(parent.t.begin() + k, parent.t.end());
    V->borrowed = (sizeof(G1Aff) + sizeof(G2Aff)) * V->lvl_off[nv] + sizeof(G2Aff) * (V->g2_off[nv] - V->g2_off[0]);
    if (k == 0) {
        V->g1_pre = parent.g1_pre;
        V->g1_pre_own = false;
        V->g1_c = parent.g1_c, V->g1_W = parent.g1_W;
        V->borrowed += parent.g1_pre->bytes;
    } else {
        const uint64_t n = 1ull << nv;
        V->g1_c = window_bits_for(n, msm_wide_min_log());
        V->g1_W = windows_for(V->g1_c);
        V->g1_pre = std::make_shared<DevMem>(sizeof(G1Slot) * n * V->g1_W);
        precompute_level(C, V->g1_level(0), n, false, V->g1_c, V->g1_W, V->g1_pre->as<G1Slot>());
    }
    return V;
}

void pp_mem_info(const PP& P, uint64_t out[3]) {
    const PPStore& S = *P.store;
    const uint64_t g1 = P.g1_pre_own ? P.g1_pre->bytes : 0;
    out[0] = P.borrowed ? g1 : g1 + S.g1_raw_mem.bytes + S.g2_raw_mem.bytes + S.g2_pre.bytes;
    out[1] = P.borrowed;
    out[2] = (uint64_t)P.store.use_count();
}

static HostCsr single(const HostCsr& m) { return m; }

std::vector<uint8_t> k_sum_over_y(Ctx& C, const HostCsr& m, const uint8_t* z) {
    const uint64_t n = m.n;
    check_csr(m, n);
    HostCsr empty;
    empty.n = n;
    empty.rp.assign(n + 1, 0);
    HostCsr mats[3] = {single(m), empty, empty};
    DevSparse D;
    std::vector<uint64_t> rps[3] = {mats[0].rp, mats[1].rp, mats[2].rp};
    std::vector<uint32_t> cols[3] = {mats[0].col, mats[1].col, mats[2].col};
    std::vector<uint8_t> vals[3] = {mats[0].val, mats[1].val, mats[2].val};
    DevMem err(sizeof(int)), zd(32 * n), out(32 * n * 3), part(32 * 4096);
    SPX_HIP(hipMemsetAsync(err.p, 0, 4, C.stream));
    DevSliced S;  // the same two paths as prove(): sliced entries for single-entry rows, else CSR
    if (!upload_sliced(C, S, mats, n, 0, n, err.as<int>())) upload_sparse(C, D, rps, cols, vals, 0, n, err.as<int>());
    SPX_HIP(hipMemcpyAsync(zd.p, z, 32 * n, hipMemcpyHostToDevice, C.stream));
    launch_to_mont(zd.as<Fr>(), n, err.as<int>(), C.stream);
    Fr* o = out.as<Fr>();
    if (D.nchunks > (int)4096) part.alloc(32 * D.nchunks);
    const SpmvJob sjob{zd.as<Fr>(), {o, o + n, o + 2 * n}};
    if (S.on)
        launch_spmv_sliced(1, &sjob, S.view(), S.entries, C.stream);
    else
        launch_sparse3(0, D.view(), zd.as<Fr>(), o, o + n, o + 2 * n, nullptr, n, D.chunks.as<LongChunk>(), D.nchunks,
                       D.lrows.as<LongRow>(), D.nlrows, part.as<Fr>(), C.stream);
    launch_from_mont(o + n, o, n, C.stream);
    std::vector<uint8_t> res(32 * n);
    SPX_HIP(hipMemcpyAsync(res.data(), o + n, 32 * n, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    return res;
}

std::vector<uint8_t> k_eval_on_x(Ctx& C, const HostCsr& m, const uint8_t* r_x) {
    const uint64_t n = m.n;
    check_csr(m, n);
    if (!is_pow2(n)) invalid("2^(r_x) should have size: num_constraints");
    const int L = ilog2(n);
    // CSC of m (matrices B, C empty), scale (1, 0, 0)
    std::vector<uint64_t> cp;
    std::vector<uint32_t> rows;
    std::vector<uint8_t> vals;
    build_csc(m, n, cp, rows, vals);
    std::vector<uint64_t> rps[3] = {cp, std::vector<uint64_t>(n + 1, 0), std::vector<uint64_t>(n + 1, 0)};
    std::vector<uint32_t> cols[3] = {rows, {}, {}};
    std::vector<uint8_t> vv[3] = {vals, {}, {}};
    DevColStream D;
    DevMem err(sizeof(int)), rx(32 * L + 96), out(32 * n * 2), part(32 * std::max(4096, 1)), eqf(32 * kEqScratch);
    SPX_HIP(hipMemsetAsync(err.p, 0, 4, C.stream));
    upload_cols(C, D, rps, cols, vv, 0, n, err.as<int>());
    std::vector<uint8_t> hr(32 * L + 96, 0);
    memcpy(hr.data(), r_x, 32 * L);
    HFr one = HFr::one();
    uint64_t onec[4];
    one.to_canon(onec);
    memcpy(hr.data() + 32 * L, onec, 32);  // canonical 1, 0, 0
    SPX_HIP(hipMemcpyAsync(rx.p, hr.data(), hr.size(), hipMemcpyHostToDevice, C.stream));
    launch_to_mont(rx.as<Fr>(), L + 3, err.as<int>(), C.stream);
    if (D.longc.nchunks > 4096) part.alloc(32 * D.longc.nchunks);
    Fr* o = out.as<Fr>();
    const ColStreamJob cjob{rx.as<Fr>(), rx.as<Fr>() + L, o, eqf.as<Fr>(), part.as<Fr>()};
    D.launch(1, &cjob, L, C.stream);
    launch_from_mont(o + n, o, n, C.stream);
    std::vector<uint8_t> res(32 * n);
    SPX_HIP(hipMemcpyAsync(res.data(), o + n, 32 * n, hipMemcpyDeviceToHost, C.stream));
    int herr = 0;
    SPX_HIP(hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    if (herr) throw SpxError(kSerialization, "non-canonical field element");
    return res;
}

// One AHPForMLSumcheck::prove_round [upstream linear-sumcheck] of sum_b f(b) g(b) (the second sumcheck's
// product shape [r_M M(r_x, .), z], prover.rs:239-247) through the product's round kernels: with r_prev
// the tables are first bound at variable 0 (T'[b] = T[2b] + r (T[2b+1] - T[2b]), n/2 entries out), then
// P(t) = sum_b f'(b, t) g'(b, t) at t = 0, 1, 2. Canonical bytes in and out.
void k_sumcheck_round(Ctx& C, const uint8_t* f, const uint8_t* g, uint64_t n, const uint8_t* r_prev,
                      uint8_t* evals_out, uint8_t* f_out, uint8_t* g_out) {
    if (!is_pow2(n) || n < (r_prev ? 4u : 2u)) invalid("table size must be a power of two (>= 2, >= 4 with a challenge)");
    const bool fold = r_prev != nullptr;
    const uint64_t half = fold ? n / 4 : n / 2;
    DevMem err(sizeof(int)), tabs(32 * 2 * n), outs(32 * (fold ? n : 2)), res(32 * (3 + std::max<uint64_t>(n, 3))),
        part(32 * kRoundPartials);
    SPX_HIP(hipMemsetAsync(err.p, 0, 4, C.stream));
    Fr* F = tabs.as<Fr>();
    Fr* Gt = F + n;
    SPX_HIP(hipMemcpyAsync(F, f, 32 * n, hipMemcpyHostToDevice, C.stream));
    SPX_HIP(hipMemcpyAsync(Gt, g, 32 * n, hipMemcpyHostToDevice, C.stream));
    launch_to_mont(F, 2 * n, err.as<int>(), C.stream);
    Fr r{};
    if (fold) {
        uint64_t c[4];
        memcpy(c, r_prev, 32);
        if (HFr::geq_p(c)) throw SpxError(kSerialization, "non-canonical challenge");
        r = dev_fr(HFr::from_canon(c));
    }
    Fr* Fo = fold ? outs.as<Fr>() : nullptr;
    Fr* Go = fold ? Fo + n / 2 : nullptr;
    Fr* ev = res.as<Fr>();
    const Sc2Job rjob{F, Gt, Fo, Go, r, part.as<Fr>(), C.ticket, ev};
    launch_sc2_round(1, &rjob, fold, true, half, C.stream);
    Fr* canon = ev + 3;
    launch_from_mont(canon, ev, 3, C.stream);
    int herr = 0;
    SPX_HIP(hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, C.stream));
    SPX_HIP(hipMemcpyAsync(evals_out, canon, 96, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    if (herr) throw SpxError(kSerialization, "non-canonical field element");
    if (fold) {
        launch_from_mont(canon, Fo, n, C.stream);  // f' then g' (n / 2 each, contiguous)
        if (f_out) SPX_HIP(hipMemcpyAsync(f_out, canon, 16 * n, hipMemcpyDeviceToHost, C.stream));
        if (g_out) SPX_HIP(hipMemcpyAsync(g_out, canon + n / 2, 16 * n, hipMemcpyDeviceToHost, C.stream));
        C.sync();
    }
}

std::vector<uint8_t> k_msm(Ctx& C, bool g2, const uint8_t* bases, const uint8_t* scalars, size_t n) {
    if (n == 0) invalid("empty MSM");
    const size_t ps = g2 ? 192 : 96;
    DevMem raw(ps * n), sc(32 * n), err(sizeof(int));
    SPX_HIP(hipMemsetAsync(err.p, 0, 4, C.stream));
    SPX_HIP(hipMemcpyAsync(raw.p, bases, ps * n, hipMemcpyHostToDevice, C.stream));
    SPX_HIP(hipMemcpyAsync(sc.p, scalars, 32 * n, hipMemcpyHostToDevice, C.stream));
    launch_to_mont(sc.as<Fr>(), n, err.as<int>(), C.stream);
    if (g2)
        launch_points_from_bytes_g2(raw.as<G2Aff>(), n, err.as<int>(), C.stream);
    else
        launch_points_from_bytes_g1(raw.as<G1Aff>(), n, err.as<int>(), C.stream);
    MsmInst I{};
    I.c = (uint32_t)window_bits_for(n, msm_wide_min_log());
    I.W = (uint32_t)windows_for((int)I.c);
    I.size = (uint32_t)n;
    I.stride = (uint32_t)n;
    DevMem pre((g2 ? sizeof(G2Aff) : sizeof(G1Slot)) * n * I.W), out(msm_out_bytes(g2, 1));
    if (g2)
        precompute_level(C, raw.as<G2Aff>(), n, false, (int)I.c, (int)I.W, pre.as<G2Aff>());
    else
        precompute_level(C, raw.as<G1Aff>(), n, false, (int)I.c, (int)I.W, pre.as<G1Slot>());
    if (g2)
        msm_run_g2(C.msm, &I, 1, pre.as<G2Aff>(), sc.as<Fr>(), out.p, C.stream);
    else
        msm_run_g1(C.msm, &I, 1, pre.as<G1Slot>(), sc.as<Fr>(), out.p, C.stream);
    std::vector<uint8_t> h(out.bytes);
    int herr = 0;
    SPX_HIP(hipMemcpyAsync(h.data(), out.p, out.bytes, hipMemcpyDeviceToHost, C.stream));
    SPX_HIP(hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    if (herr & 1) throw SpxError(kSerialization, "non-canonical input");
    if (herr & 2) throw SpxError(kSerialization, "base point not on the curve");
    msm_skew_fold(C, h.data(), g2, 1);
    std::vector<uint8_t> res(ps);
    LocalComm local;
    if (g2)
        host::g2_to_uncompressed(res.data(), msm_results<HFq2>(local, h.data(), 1)[0]);
    else
        host::g1_to_uncompressed(res.data(), msm_results<HFq>(local, h.data(), 1)[0]);
    return res;
}

std::vector<uint8_t> k_commit(Ctx& C, PP& P, const uint8_t* table, int nv) {
    if (nv != P.nv) invalid("table size != 2^nv of the public parameters");
    auto W = witness_upload(C, table, 1, table + 32, (1ull << nv) - 1);
    LocalComm local;
    commit_launch(C, P, W->z.as<Fr>(), 1ull << nv, MsmShard());
    Affine<HFq> a = commit_finish(C, P, W->z.as<Fr>(), 1ull << nv, local);
    std::vector<uint8_t> out(56);
    uint64_t u = (uint64_t)nv;
    memcpy(out.data(), &u, 8);
    host::g1_compress(out.data() + 8, a);
    return out;
}

std::vector<uint8_t> k_open(Ctx& C, PP& P, const uint8_t* table, int nv, const uint8_t* point) {
    if (nv != P.nv) invalid("table size != 2^nv of the public parameters");
    auto W = witness_upload(C, table, 1, table + 32, (1ull << nv) - 1);
    std::vector<HFr> pt(nv);
    for (int i = 0; i < nv; ++i)
        if (!host::fr_from_bytes(pt[i], point + 32 * i)) throw SpxError(kSerialization, "non-canonical point");
    LocalComm local;
    OpenOut op = open_z(C, P, W->z.as<Fr>(), nv, pt, local);
    Ser s;
    ser_open(s, op.eval, P.h, op.proofs);
    return s.b;
}

}  // namespace spx
