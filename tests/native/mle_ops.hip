// Test-only library: the kernels and launchers of mle_kernels.hip behind C entry points, one per kernel
// family, so that tests/test_gpu_mle_ops.py can run each of them on chosen tables (tests/mle_cases.py)
// and compare every output word with a big-integer reference. Nothing here is part of
// libspartan_hip.so and nothing depends on it.
//
// The kernel file is #included, so the kernels, their static launch constants (kWaveMinHalf,
// kFuseMaxBlocks, kTailMax, ...) and the launchers are the ones the product compiles. That also
// re-defines spx::launch_* and spx::g_kprof, which libspartan_hip.so exports and which sit in the same
// pytest process. Linking choice: the library is compiled with -fvisibility=hidden and only the entry
// points below carry default visibility (MLE_API), so every spx:: symbol binds to this file's own copy
// and none is exported. The kernels' host-side handles get default visibility from the compiler
// whatever the flag says, so the link also takes tests/native/mle_ops.map, which makes everything
// but mle_* local.
//
// Two kinds of entry. mode 0 calls the product launcher with its production dispatch; the other modes
// launch one kernel template directly with the grid the test gives (>= 1) and the kernel's own block
// size, to reach stride loops and reduction paths the launchers only take at 2^17 - 2^24.
//
// Every entry copies its arguments in, launches on the null stream, synchronises, copies out and
// returns the first HIP error code (0: none; -1: a launcher refused its arguments). After an error
// nothing more is launched. Buffers marked in/out arrive filled with the caller's pattern and go back
// whole, so the caller sees every byte the kernel did or did not write; device buffers have exactly
// the documented size. Fr values are 8 x 32-bit words, Montgomery form unless said otherwise: the
// caller converts (the kernels under test never prepare or decode their own operands).
#include "mle_kernels.hip"

#include <type_traits>

#define MLE_API extern "C" __attribute__((visibility("default")))

namespace {
using namespace spx;

struct Sess {
    hipError_t e = hipSuccess;
    std::vector<void*> bufs;
    bool good() const { return e == hipSuccess; }
    bool ck(hipError_t x) {
        if (e == hipSuccess && x != hipSuccess) e = x;
        return e == hipSuccess;
    }
    // a device buffer of n items: a copy of host[0 .. n), or zeroed if host is null (null for n == 0)
    template <class T>
    T* up(const T* host, uint64_t n, bool zero_if_null = false) {
        if (!n || !good() || (!host && !zero_if_null)) return nullptr;
        void* p = nullptr;
        if (!ck(hipMalloc(&p, n * sizeof(T)))) return nullptr;
        bufs.push_back(p);
        if (host)
            ck(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
        else
            ck(hipMemset(p, 0, n * sizeof(T)));
        return (T*)p;
    }
    template <class T>
    T* scratch(uint64_t n) {
        return up<T>(nullptr, n, true);
    }
    template <class T>
    void down(T* host, const T* dev, uint64_t n) {
        if (host && dev && n && good()) ck(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost));
    }
    template <class T>
    void reup(T* dev, const T* host, uint64_t n) {
        if (host && dev && n && good()) ck(hipMemcpy(dev, host, n * sizeof(T), hipMemcpyHostToDevice));
    }
    bool sync() {
        if (!good()) return false;
        ck(hipGetLastError());
        return ck(hipDeviceSynchronize());
    }
    int done() {
        for (void* p : bufs) (void)hipFree(p);
        return (int)e;
    }
};

#define BV(x) SPX_BV(x)  // (with_bool is the launchers' own)

// the argument checks every entry shares: a launch is made only on a valid shape
bool bad_grid(int mode, int grid) { return mode != 0 && grid < 1; }

// one launch of a sumcheck round (which = 1: tables A, B, C and E; 2: tables M, Z)
void round_launch(int which, int mode, bool fold, bool need1, bool fused, int grid, const Tables3& in, const Tables3& out,
                  const Fr* Ein, Fr* Eout, const Fr& r, uint64_t half, Fr* partial, uint32_t* ticket, Fr* result3) {
    const hipStream_t s = nullptr;
    const int n1 = need1 ? 1 : 0;
    if (mode == 0) {
        const Sc1Job j1{in, out, Ein, Eout, r, partial, ticket, result3};
        const Sc2Job j2{in.t[0], in.t[1], out.t[0], out.t[1], r, partial, ticket, result3};
        if (which == 1)
            launch_sc1_round(1, &j1, fold, need1, half, s);
        else
            launch_sc2_round(1, &j2, fold, need1, half, s);
        return;
    }
    const dim3 g(grid), b(kThreads);
    if (mode == 1) {  // per-lane form
        with_bool(fold, [&](auto F) {
            with_bool(fused, [&](auto U) {
                if (which == 1)
                    hipLaunchKernelGGL((k_sc1_round<BV(F), BV(U)>), g, b, 0, s, in, out, Ein, Eout, r, half, partial, ticket,
                                       result3, n1);
                else
                    hipLaunchKernelGGL((k_sc2_round<BV(F), BV(U)>), g, b, 0, s, in.t[0], in.t[1], out.t[0], out.t[1], r,
                                       half, partial, ticket, result3, n1);
            });
        });
    } else if (mode == 2) {  // quad / lane-pair form (fold, no G(1))
        with_bool(fused, [&](auto U) {
            if (which == 1)
                hipLaunchKernelGGL((k_sc1_fold_quad<BV(U)>), g, b, 0, s, in, out, Ein, Eout, r, half, partial, ticket,
                                   result3);
            else
                hipLaunchKernelGGL((k_sc2_fold_pair<BV(U)>), g, b, 0, s, in.t[0], in.t[1], out.t[0], out.t[1], r, half,
                                   partial, ticket, result3);
        });
    } else {  // wave-transposed form
        with_bool(fold, [&](auto F) {
            with_bool(need1, [&](auto N) {
                with_bool(fused, [&](auto U) {
                    if (which == 1)
                        hipLaunchKernelGGL((k_sc1_wave<BV(F), BV(N), BV(U)>), g, b, 0, s, in, out, Ein, Eout, r, half,
                                           partial, ticket, result3);
                    else
                        hipLaunchKernelGGL((k_sc2_wave<BV(F), BV(N), BV(U)>), g, b, 0, s, in.t[0], in.t[1], out.t[0],
                                           out.t[1], r, half, partial, ticket, result3);
                });
            });
        });
    }
    if (!fused) hipLaunchKernelGGL(k_reduce_partials<3>, dim3(1), dim3(kThreads), 0, s, partial, grid, result3);
}

template <class F>
int guarded(Sess& S, F f) {
    try {
        f();
    } catch (const std::exception&) {
        S.done();
        return -1;
    }
    return S.done();
}
}  // namespace

// A sumcheck round, launched twice on the same ticket and partials.
//   which 1: tabs = A, B, C (3 x nin), E (nE);  which 2: tabs = M, Z (2 x nin), E unused
//   mode 0: launch_sc1_round / launch_sc2_round with one job;  1: k_sc?_round<fold, fused>;  2: k_sc1_fold_quad /
//   k_sc2_fold_pair<fused>;  3: k_sc?_wave<fold, need1, fused>. Direct unfused launches are followed by
//   k_reduce_partials<3> over `grid` blocks.
//   in/out: out (ntab x nout), Eout (nEout; null: no E output), partial (npartial), result6 (the pattern
//   in its first 3 Fr: launch i's result3 comes back at 3 i);  out: ticket2[i] = the ticket word after launch i
MLE_API int mle_round(int which, int mode, int fold, int need1, int fused, int grid, const Fr* tabs, uint64_t nin,
                      const Fr* E, uint64_t nE, const Fr* r, uint64_t half, Fr* out, uint64_t nout, Fr* Eout,
                      uint64_t nEout, Fr* partial, uint64_t npartial, uint32_t* ticket2, Fr* result6) {
    Sess S;
    const int ntab = which == 1 ? 3 : 2;
    if ((which != 1 && which != 2) || mode < 0 || mode > 3 || bad_grid(mode, grid) || half < 1 || !tabs || !r ||
        (mode == 2 && (!fold || need1)) || (mode != 0 && (uint64_t)grid * 3 > npartial))
        return -1;
    return guarded(S, [&] {
        Fr* dt = S.up(tabs, ntab * nin);
        Fr* dE = which == 1 ? S.up(E, nE) : nullptr;
        Fr* dout = S.up(out, ntab * nout);
        Fr* dEout = S.up(Eout, nEout);
        Fr* dpart = S.up(partial, npartial);
        uint32_t* dtick = S.scratch<uint32_t>(1);
        Fr* dres = S.up(result6, 3);
        Tables3 tin{}, tout{};
        for (int m = 0; m < ntab; ++m) tin.t[m] = dt + m * nin, tout.t[m] = dout ? dout + m * nout : nullptr;
        Fr pat[3];
        for (int k = 0; k < 3; ++k) pat[k] = result6[k];
        for (int rep = 0; rep < 2 && S.good(); ++rep) {
            S.reup(dres, pat, 3);
            if (!S.good()) break;
            round_launch(which, mode, fold, need1, fused, grid, tin, tout, dE, dEout, *r, half, dpart, dtick, dres);
            if (!S.sync()) break;
            S.down(result6 + 3 * rep, dres, 3);
            S.down(ticket2 + rep, dtick, 1);
        }
        S.down(out, dout, ntab * nout);
        S.down(Eout, dEout, nEout);
        S.down(partial, dpart, npartial);
    });
}

// The same round for the k jobs of a lockstep group through launch_sc1_round / launch_sc2_round,
// twice. Per job j: its tables at tabs + j ntab nin, E at E + j nE, challenge
// r[j], outputs at out + j ntab nout, Eout + j nEout, partials at partial + j npartial;
// result (2 x k x 3, the pattern in the first 3 Fr): launch i's result3 of job j at (i k + j) 3;
// ticket2: 2 x k words.
MLE_API int mle_round_group(int which, int k, int fold, int need1, const Fr* tabs, uint64_t nin, const Fr* E, uint64_t nE,
                            const Fr* r, uint64_t half, Fr* out, uint64_t nout, Fr* Eout, uint64_t nEout, Fr* partial,
                            uint64_t npartial, uint32_t* ticket2, Fr* result) {
    Sess S;
    const int ntab = which == 1 ? 3 : 2;
    if ((which != 1 && which != 2) || k < 1 || k > kGroupMax || half < 1 || !tabs || !r) return -1;
    return guarded(S, [&] {
        Fr* dt = S.up(tabs, (uint64_t)k * ntab * nin);
        Fr* dE = which == 1 ? S.up(E, (uint64_t)k * nE) : nullptr;
        Fr* dout = S.up(out, (uint64_t)k * ntab * nout);
        Fr* dEout = S.up(Eout, (uint64_t)k * nEout);
        Fr* dpart = S.up(partial, (uint64_t)k * npartial);
        uint32_t* dtick = S.scratch<uint32_t>(k);
        std::vector<Fr> pat((size_t)3 * k);
        for (int j = 0; j < 3 * k; ++j) pat[j] = result[j % 3];
        Fr* dres = S.up(pat.data(), 3 * k);
        std::vector<Sc1Job> j1(k);
        std::vector<Sc2Job> j2(k);
        for (int j = 0; j < k; ++j) {
            Fr* ti = dt + (uint64_t)j * ntab * nin;
            Fr* to = dout ? dout + (uint64_t)j * ntab * nout : nullptr;
            Fr* pj = dpart + (uint64_t)j * npartial;
            if (which == 1) {
                Sc1Job& J = j1[j];
                for (int m = 0; m < 3; ++m) J.in.t[m] = ti + m * nin, J.out.t[m] = to ? to + m * nout : nullptr;
                J.Ein = dE + (uint64_t)j * nE, J.Eout = dEout ? dEout + (uint64_t)j * nEout : nullptr;
                J.r = r[j], J.partial = pj, J.ticket = dtick + j, J.result3 = dres + 3 * j;
            } else {
                Sc2Job& J = j2[j];
                J.Min = ti, J.Zin = ti + nin, J.Mout = to, J.Zout = to ? to + nout : nullptr;
                J.r = r[j], J.partial = pj, J.ticket = dtick + j, J.result3 = dres + 3 * j;
            }
        }
        for (int rep = 0; rep < 2 && S.good(); ++rep) {
            S.reup(dres, pat.data(), 3 * k);
            if (!S.good()) break;
            if (which == 1)
                launch_sc1_round(k, j1.data(), fold, need1, half, nullptr);
            else
                launch_sc2_round(k, j2.data(), fold, need1, half, nullptr);
            if (!S.sync()) break;
            S.down(result + (uint64_t)3 * k * rep, dres, 3 * k);
            S.down(ticket2 + k * rep, dtick, k);
        }
        S.down(out, dout, (uint64_t)k * ntab * nout);
        S.down(Eout, dEout, (uint64_t)k * nEout);
        S.down(partial, dpart, (uint64_t)k * npartial);
    });
}

// k_reduce_partials<3> over nblk blocks' partials (3 nblk Fr) into out3 (in/out)
MLE_API int mle_reduce_partials(const Fr* partial, int nblk, Fr* out3) {
    Sess S;
    if (nblk < 1 || !partial) return -1;
    return guarded(S, [&] {
        Fr* dp = S.up(partial, (uint64_t)3 * nblk);
        Fr* dout = S.up(out3, 3);
        if (!S.good()) return;
        hipLaunchKernelGGL(k_reduce_partials<3>, dim3(1), dim3(kThreads), 0, nullptr, dp, nblk, dout);
        S.sync();
        S.down(out3, dout, 3);
    });
}

// eq tables. k == 0: launch_eq_table with one job; k >= 1: with the jobs of k proofs (r: k x nvar, out:
// k x count, in/out). The scratch tables hold 2^13 entries each, per proof.
MLE_API int mle_eq_table(int k, const Fr* r, int nvar, uint64_t base, uint64_t count, Fr* out) {
    Sess S;
    const int kk = k < 1 ? 1 : k;
    if (k < 0 || k > kGroupMax || nvar < 0 || nvar > 26 || count < 1 || base + count > (1ull << nvar) || !out) return -1;
    return guarded(S, [&] {
        Fr* dr = S.up(r, (uint64_t)kk * nvar);
        Fr* dout = S.up(out, (uint64_t)kk * count);
        Fr* dlo = S.scratch<Fr>((uint64_t)kk << 13);
        Fr* dhi = S.scratch<Fr>((uint64_t)kk << 13);
        if (!S.good()) return;
        std::vector<EqTableJob> jobs(kk);
        for (int j = 0; j < kk; ++j)
            jobs[j] = EqTableJob{dr + (uint64_t)j * nvar, dout + (uint64_t)j * count, dlo + ((uint64_t)j << 13),
                                 dhi + ((uint64_t)j << 13)};
        launch_eq_table(kk, jobs.data(), nvar, base, count, nullptr);
        S.sync();
        S.down(out, dout, (uint64_t)kk * count);
    });
}

// k_eq_factors on the split eq_factors_for(L) carves from `scratch` (kEqScratch Fr, in/out): lo at 0,
// the last table (three copies scale[m] hi[x] at m 2^k + x if scale, else one) behind it
MLE_API int mle_eq_factors(int L, const Fr* r, const Fr* scale, Fr* scratch) {
    Sess S;
    if (L < 1 || L > 26 || !r || !scratch) return -1;
    return guarded(S, [&] {
        Fr* dr = S.up(r, L);
        Fr* dsc = S.up(scale, 3);
        Fr* ds = S.up(scratch, kEqScratch);
        if (!S.good()) return;
        const EqFactors ef = eq_factors_for(L, ds);
        hipLaunchKernelGGL(k_eq_factors, dim3(ef.nf), dim3(kEqThreads), 0, nullptr, dr, ef, dsc);
        S.sync();
        S.down(scratch, ds, kEqScratch);
    });
}

// k_eq_expand with `grid` blocks: out[i] = lo[(i + base) & (2^klo - 1)] hi[(i + base) >> klo], i < count
MLE_API int mle_eq_expand(const Fr* lo, const Fr* hi, uint64_t nhi, int klo, uint64_t base, uint64_t count, int grid,
                          Fr* out) {
    Sess S;
    if (grid < 1 || klo < 0 || klo > 13 || count < 1 || !lo || !hi || !out || ((base + count - 1) >> klo) >= nhi) return -1;
    return guarded(S, [&] {
        Fr* dlo = S.up(lo, 1ull << klo);
        Fr* dhi = S.up(hi, nhi);
        Fr* dout = S.up(out, count);
        if (!S.good()) return;
        hipLaunchKernelGGL(k_eq_expand, dim3(grid), dim3(kThreads), 0, nullptr, dlo, dhi, klo, base, count, dout);
        S.sync();
        S.down(out, dout, count);
    });
}

// one opening level. mode 0: launch_open_level; 1: k_open_level with `grid` blocks. rin: 2 half;
// rout, q: half each, in/out, either may be null
MLE_API int mle_open_level(int mode, int grid, const Fr* rin, uint64_t half, Fr* rout, Fr* q, const Fr* p) {
    Sess S;
    if (mode < 0 || mode > 1 || bad_grid(mode, grid) || half < 1 || !rin || !p) return -1;
    return guarded(S, [&] {
        Fr* din = S.up(rin, 2 * half);
        Fr* dro = S.up(rout, half);
        Fr* dq = S.up(q, half);
        if (!S.good()) return;
        if (mode == 0)
            launch_open_level(din, dro, dq, *p, half, nullptr);
        else
            hipLaunchKernelGGL(k_open_level, dim3(grid), dim3(kThreads), 0, nullptr, din, dro, dq, *p, half);
        S.sync();
        S.down(rout, dro, half);
        S.down(q, dq, half);
    });
}

// nf (2 or 3) opening levels in one launch. mode 0: launch_open_fold; 1: k_open_fold<nf>; 2:
// k_open_fold_wave<nf> (nout a multiple of 64), with `grid` blocks. rin: nout 2^nf; rout: nout, in/out;
// q: nq, in/out (null if nq == 0: then every qoffs[j] must be ~0); level j's 2^(nf-1-j) nout quotients
// must fit behind qoffs[j]
MLE_API int mle_open_fold(int mode, int grid, int nf, const Fr* rin, uint64_t nout, Fr* rout, Fr* q, uint64_t nq,
                          const Fr* points, const uint64_t* qoffs) {
    Sess S;
    if (mode < 0 || mode > 2 || bad_grid(mode, grid) || (nf != 2 && nf != 3) || nout < 1 || !rin || !rout || !points ||
        !qoffs || (mode == 2 && nout % 64))
        return -1;
    for (int j = 0; j < nf; ++j)
        if (qoffs[j] != ~0ull && (!q || qoffs[j] + (nout << (nf - 1 - j)) > nq)) return -1;
    return guarded(S, [&] {
        Fr* din = S.up(rin, nout << nf);
        Fr* dro = S.up(rout, nout);
        Fr* dq = S.up(q, nq);
        if (!S.good()) return;
        if (mode == 0) {
            launch_open_fold(din, dro, dq, nf, points, qoffs, nout, nullptr);
        } else {
            auto run = [&](auto tag) {
                constexpr int NF = decltype(tag)::value;
                FoldArgs<NF> a;
                for (int j = 0; j < NF; ++j) a.p[j] = points[j], a.qoff[j] = qoffs[j];
                if (mode == 1)
                    hipLaunchKernelGGL(k_open_fold<NF>, dim3(grid), dim3(kThreads), 0, nullptr, din, dro, dq, a, nout);
                else
                    hipLaunchKernelGGL(k_open_fold_wave<NF>, dim3(grid), dim3(kThreads), 0, nullptr, din, dro, dq, a, nout);
            };
            if (nf == 3)
                run(std::integral_constant<int, 3>{});
            else
                run(std::integral_constant<int, 2>{});
        }
        S.sync();
        S.down(rout, dro, nout);
        S.down(q, dq, nq);
    });
}

// launch_open_tail: nlev levels from `half` pairs. rin: 2 half; q: half + half/2 + ... (nlev terms) = nq,
// in/out, or null; last: 1, in/out
MLE_API int mle_open_tail(const Fr* rin, uint64_t half, int nlev, const Fr* points, Fr* q, uint64_t nq, Fr* last) {
    Sess S;
    if (half < 1 || nlev < 1 || !rin || !points || !last) return -1;
    uint64_t need = 0;
    for (int j = 0; j < nlev; ++j) need += half >> j;
    if (q && nq != need) return -1;
    return guarded(S, [&] {
        Fr* din = S.up(rin, 2 * half);
        Fr* dq = S.up(q, nq);
        Fr* dl = S.up(last, 1);
        if (!S.good()) return;
        launch_open_tail(din, dq, half, nlev, points, dl, nullptr);
        S.sync();
        S.down(q, dq, nq);
        S.down(last, dl, 1);
    });
}

MLE_API int mle_open_tail_levels(uint64_t half, int remaining) { return open_tail_levels(half, remaining); }

// The launch plans, host arithmetic only (no launch). sc_round_plan: out4 = form (kRoundLane / kRoundSplit /
// kRoundWave), grid, fused, per-proof
MLE_API int mle_round_plan(int which, int k, int fold, int need1, uint64_t half, int* out4) {
    if ((which != 1 && which != 2) || k < 1 || k > kGroupMax || half < 1 || !out4) return -1;
    const RoundPlan p = sc_round_plan(which, k, fold, need1, half);
    out4[0] = p.form, out4[1] = p.grid, out4[2] = p.fused, out4[3] = p.per_proof;
    return 0;
}
// open_eval_plan(L): per step 5 words (kind kOpenTail / kOpenFold / kOpenLevel, first level, levels, size,
// wave) into steps (room for `cap` steps), *copy = the chain ends on a fold; returns the number of steps
MLE_API int mle_open_eval_plan(int L, uint64_t* steps, int cap, int* copy) {
    if (L < 1 || L > 26 || !steps || !copy) return -1;
    const OpenEvalPlan pl = open_eval_plan(L);
    if ((int)pl.steps.size() > cap) return -1;
    for (size_t i = 0; i < pl.steps.size(); ++i) {
        const OpenStep& st = pl.steps[i];
        uint64_t* w = steps + 5 * i;
        w[0] = st.kind, w[1] = st.first, w[2] = st.levels, w[3] = st.size, w[4] = st.wave;
    }
    *copy = pl.copy;
    return (int)pl.steps.size();
}

// launch_open_eval with k jobs: z (k x n, n = 2^L), points (k x L, host side as the launcher takes them),
// last (k, in/out); bufA / bufB are n/2 and n/4 Fr per proof
MLE_API int mle_open_eval_group(int k, const Fr* z, const Fr* points, int L, Fr* last) {
    Sess S;
    if (k < 1 || k > kGroupMax || L < 1 || L > 24 || !z || !points || !last) return -1;
    const uint64_t n = 1ull << L;
    return guarded(S, [&] {
        Fr* dz = S.up(z, (uint64_t)k * n);
        Fr* dA = S.scratch<Fr>((uint64_t)k * (n / 2));
        Fr* dB = S.scratch<Fr>((uint64_t)k * (n / 4));
        Fr* dl = S.up(last, k);
        if (!S.good()) return;
        std::vector<OpenEvalJob> jobs(k);
        for (int j = 0; j < k; ++j)
            jobs[j] = OpenEvalJob{dz + (uint64_t)j * n, dA + (uint64_t)j * (n / 2), dB ? dB + (uint64_t)j * (n / 4) : nullptr,
                                  points + (uint64_t)j * L, dl + j};
        launch_open_eval(k, jobs.data(), L, nullptr);
        S.sync();
        S.down(last, dl, k);
    });
}

// the sliced SpMV. mle_spmv: launch_spmv_sliced with one job (k == 0) or the jobs of k >= 1 proofs (a
// group of one is the per-proof kernel too). mle_spmv_group_direct: k_spmv_sliced_group itself for k >= 1
// proofs with `grid` blocks (a multiple of 8). val / col / dst: `entries` each (dst = row | matrix << 30,
// row < nrows, col < nz); z: k x nz; out: per proof Az, Bz, Cz (3 x nrows), in/out
static int spmv_entry(int k, const Fr* val, const uint32_t* col, const uint32_t* dst, uint64_t entries, const Fr* z,
                      uint64_t nz, Fr* out, uint64_t nrows, int grid) {
    Sess S;
    const int kk = k < 1 ? 1 : k;
    if (k < 0 || k > kGroupMax || entries < 1 || !val || !col || !dst || !z || !out) return -1;
    if (grid < 0 || grid % 8 || (grid && k < 1)) return -1;
    for (uint64_t e = 0; e < entries; ++e)
        if (col[e] >= nz || (dst[e] >> 30) > 2 || (dst[e] & 0x3FFFFFFFu) >= nrows) return -1;
    return guarded(S, [&] {
        SpmvSlicedView v{};
        v.val = S.up(val, entries), v.col = S.up(col, entries), v.dst = S.up(dst, entries);
        Fr* dz = S.up(z, (uint64_t)kk * nz);
        Fr* dout = S.up(out, (uint64_t)kk * 3 * nrows);
        if (!S.good()) return;
        GroupOf<SpmvJob> g{};
        for (int j = 0; j < kk; ++j) {
            g.j[j].z = dz + (uint64_t)j * nz;
            for (int m = 0; m < 3; ++m) g.j[j].o[m] = dout + ((uint64_t)j * 3 + m) * nrows;
        }
        if (grid == 0)
            launch_spmv_sliced(kk, g.j, v, entries, nullptr);
        else
            hipLaunchKernelGGL(k_spmv_sliced_group, dim3(grid), dim3(kThreads), 0, nullptr, v, g, k, entries);
        S.sync();
        S.down(out, dout, (uint64_t)kk * 3 * nrows);
    });
}
MLE_API int mle_spmv(int k, const Fr* val, const uint32_t* col, const uint32_t* dst, uint64_t entries, const Fr* z,
                     uint64_t nz, Fr* out, uint64_t nrows) {
    return spmv_entry(k, val, col, dst, entries, z, nz, out, nrows, 0);
}
MLE_API int mle_spmv_group_direct(int k, int grid, const Fr* val, const uint32_t* col, const uint32_t* dst,
                                  uint64_t entries, const Fr* z, uint64_t nz, Fr* out, uint64_t nrows) {
    return grid < 1 ? -1 : spmv_entry(k, val, col, dst, entries, z, nz, out, nrows, grid);
}

// conversions over n elements. mode 0: launch_to_mont in place (err: out, the kernel's flag word);
// 1: k_to_mont with `grid` blocks; 2: launch_from_mont (data: Montgomery in, canonical out)
MLE_API int mle_mont(int mode, int grid, Fr* data, uint64_t n, int* err) {
    Sess S;
    if (mode < 0 || mode > 2 || (mode == 1 && grid < 1) || n < 1 || !data || !err) return -1;
    return guarded(S, [&] {
        Fr* dd = S.up(data, n);
        int* derr = S.scratch<int>(1);
        Fr* dout = mode == 2 ? S.scratch<Fr>(n) : dd;
        if (!S.good()) return;
        if (mode == 0)
            launch_to_mont(dd, n, derr, nullptr);
        else if (mode == 1)
            hipLaunchKernelGGL(k_to_mont, dim3(grid), dim3(kThreads), 0, nullptr, dd, (size_t)n, derr);
        else
            launch_from_mont(dout, dd, n, nullptr);
        S.sync();
        S.down(data, dout, n);
        S.down(err, derr, 1);
    });
}

// launch_copy_runs: per proof j, nruns runs of `per` Fr (src: k x nruns x per) -> dst + j nruns per
// (dst: k x nruns x per, in/out)
MLE_API int mle_copy_runs(int k, const Fr* src, int nruns, int per, Fr* dst) {
    Sess S;
    if (k < 1 || k > kGroupMax || nruns < 1 || nruns > 3 || per < 1 || !src || !dst) return -1;
    return guarded(S, [&] {
        const uint64_t np = (uint64_t)nruns * per;
        Fr* ds = S.up(src, k * np);
        Fr* dd = S.up(dst, k * np);
        if (!S.good()) return;
        std::vector<CopyJob> jobs(k);
        for (int j = 0; j < k; ++j) {
            jobs[j] = CopyJob{{nullptr, nullptr, nullptr}, dd + j * np};
            for (int i = 0; i < nruns; ++i) jobs[j].src[i] = ds + j * np + (uint64_t)i * per;
        }
        launch_copy_runs(k, jobs.data(), nruns, per, nullptr);
        S.sync();
        S.down(dst, dd, k * np);
    });
}
