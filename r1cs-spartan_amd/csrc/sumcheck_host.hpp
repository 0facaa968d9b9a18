// Host half of the two sumchecks (prover.rs:199-207, lib.rs:86-131): everything the prover computes
// between a round kernel's three sums and the next launch -- the message, its bytes, the challenge, the
// running claim -- and the last rounds that run on the host altogether. prove() and prove_group() own
// the launches, waits and exchanges and call this for every field operation, so a proof's bytes cannot
// depend on which of them made it. Host-only (host_ff.hpp, transcript.hpp, the standard library):
// tests/native/sumcheck_host_check.cpp drives it without a GPU against the Python oracle.
#pragma once
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_ff.hpp"
#include "transcript.hpp"

namespace spx {

struct SpxError : std::runtime_error {
    int code;
    SpxError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
enum { kOk = 0, kInvalidArgument = 1, kSumcheck = 2, kWrongWitness = 3, kSerialization = 4, kDevice = 5 };

struct Ser {
    std::vector<uint8_t> b;
    void u64(uint64_t v) {
        uint8_t t[8];
        memcpy(t, &v, 8);
        b.insert(b.end(), t, t + 8);
    }
    void fr(const host::Fr& x) {
        uint8_t t[32];
        host::fr_to_bytes(t, x);
        b.insert(b.end(), t, t + 32);
    }
    void raw(const uint8_t* p, size_t k) { b.insert(b.end(), p, p + k); }
};

inline host::Fr ld_hfr(const uint8_t* p) {  // device Montgomery bytes -> host Fr
    host::Fr r;
    memcpy(r.v, p, 32);
    return r;
}
inline host::Fr eq1(const host::Fr& tau, const host::Fr& t) {  // eq(tau, t) = 1 - tau - t + 2 tau t  (eq.rs:14)
    host::Fr tt = tau * t;
    return host::Fr::one() - tau - t + tt + tt;
}
// the quadratic through (0, g0), (1, g1), (2, g2) at t
inline host::Fr quad_at(const host::Fr g[3], const host::Fr& t) {
    using F = host::Fr;
    static const F inv2 = F::from_u64(2).inv();
    const F one = F::one(), two = F::from_u64(2);
    return g[0] * ((t - one) * (t - two) * inv2) - g[1] * (t * (t - two)) + g[2] * (t * (t - one) * inv2);
}

// sumcheck #1 message from G(0), G(1), G(2): P(t) = C eq(tau_c, t) G(t), t = 0..L+2. G is quadratic
// and C eq(tau_c, t) = C (1 - tau) + t C (2 tau - 1) is linear in t, so both are stepped by finite
// differences and every point costs one product (exact field arithmetic: the same bytes as evaluating
// each point by Lagrange, sc1_message_lagrange).
inline std::vector<host::Fr> sc1_message(const host::Fr& Cc, const host::Fr& tau, const host::Fr g[3], int L) {
    using F = host::Fr;
    std::vector<F> P(L + 3);
    const F one = F::one();
    F Gt = g[0], d = g[1] - g[0];
    const F dd = g[2] - g[1] - d;  // second difference
    F Ce = Cc * (one - tau);
    const F Cs = Cc * (tau + tau - one);
    for (int t = 0; t <= L + 2; ++t) {
        P[t] = Ce * Gt;
        Gt = Gt + d;
        d = d + dd;
        Ce = Ce + Cs;
    }
    return P;
}

// the same message point by point: Lagrange through (0, g0), (1, g1), (2, g2), times
// C eq(tau, t) = C (1 - tau - t + 2 tau t) (eq.rs:14)
inline std::vector<host::Fr> sc1_message_lagrange(const host::Fr& Cc, const host::Fr& tau, const host::Fr g[3], int L) {
    using F = host::Fr;
    const F inv2 = F::from_u64(2).inv();
    std::vector<F> P(L + 3);
    const F one = F::one(), two = F::from_u64(2);
    for (int t = 0; t <= L + 2; ++t) {
        const F T = F::from_u64((uint64_t)t);
        const F l0 = (T - one) * (T - two) * inv2, l1 = T * (T - two), l2 = T * (T - one) * inv2;
        const F Gt = g[0] * l0 - g[1] * l1 + g[2] * l2;
        P[t] = Cc * (one - tau - T + (tau + tau) * T) * Gt;
    }
    return P;
}

// SPX_CHECK_DERIVED=1 (tests): from round 2 on, a sumcheck round's value at 1 is derived from the
// previous claim on the host (P(0) + P(1) = claim); with this set the device computes it too and the
// prove fails with SPX_SUMCHECK if they differ (the identity pinned round by round, every rank count).
// Read at every prove: a test sets it in a running process.
inline bool check_derived() {
    const char* e = getenv("SPX_CHECK_DERIVED");
    return e && e[0] == '1';
}

// A proof being written: its bytes and the transcript that absorbs each prover message.
struct ProofStream {
    Transcript T;
    Ser proof;
    // one prover message: what `write` appends to the proof is fed to the transcript
    template <class W>
    void emit(W&& write) {
        const size_t m0 = proof.b.size();
        write(proof);
        T.feed(proof.b.data() + m0, proof.b.size() - m0);
    }
    // a sumcheck round's message (a Vec<Fr>: length, elements)
    void emit_vec(const host::Fr* v, size_t n) {
        emit([&](Ser& s) {
            s.u64(n);
            for (size_t i = 0; i < n; ++i) s.fr(v[i]);
        });
    }
    // a sumcheck's IndexInfo message (max_multiplicands, num_variables: reconstructed field order),
    // then the count of its round messages (part of the proof, not of a message)
    void sumcheck_header(int max_multiplicands, int L) {
        emit([&](Ser& s) {
            s.u64((uint64_t)max_multiplicands);
            s.u64((uint64_t)L);
        });
        proof.u64((uint64_t)L);
    }
};

// ---------------------------------------------------------------- bind and tail
// After the device rounds a proof's `nt` tables hold tn entries each (`bytes`: table after table,
// Montgomery). The last device challenge r is bound here: this rank's half-tables, table after table.
inline std::vector<host::Fr> bind_tables(const uint8_t* bytes, int nt, uint32_t tn, const host::Fr& r) {
    const uint32_t hn = tn / 2;
    std::vector<host::Fr> mine((size_t)nt * hn);
    for (int m = 0; m < nt; ++m)
        for (uint32_t b = 0; b < hn; ++b) {
            const host::Fr a0 = ld_hfr(bytes + 32 * ((size_t)tn * m + 2 * b)), a1 = ld_hfr(bytes + 32 * ((size_t)tn * m + 2 * b + 1));
            mine[(size_t)m * hn + b] = a0 + r * (a1 - a0);
        }
    return mine;
}
// G ranks' half-tables as gathered (rank after rank, each bind_tables' layout) -> table after table,
// a table's entries in rank order (rank = the high variables). The identity at G = 1.
inline std::vector<host::Fr> rank_order(std::vector<host::Fr> all, int nt, int G) {
    if (G == 1) return all;
    const size_t hn = all.size() / ((size_t)nt * G);
    std::vector<host::Fr> t(all.size());
    for (int m = 0; m < nt; ++m)
        for (int r = 0; r < G; ++r)
            for (size_t b = 0; b < hn; ++b) t[((size_t)m * G + r) * hn + b] = all[((size_t)r * nt + m) * hn + b];
    return t;
}
// bind variable 0 of `nt` tables of 2 * half entries (table after table) at r, in place
inline void fold_tables(std::vector<host::Fr>& t, int nt, size_t half, const host::Fr& r) {
    for (int m = 0; m < nt; ++m)
        for (size_t b = 0; b < half; ++b) {
            const host::Fr a0 = t[2 * half * m + 2 * b], a1 = t[2 * half * m + 2 * b + 1];
            t[half * m + b] = a0 + r * (a1 - a0);  // written below everything still to be read
        }
    t.resize(nt * half);
}

// ---------------------------------------------------------------- sumcheck #1 (lib.rs:86-103)
// sum_x eq(tau, x) (Az(x) Bz(x) - Cz(x)): round i's polynomial is Cc eq(tau_i, t) G_i(t) with
// Cc = prod_{j < i} eq(tau_j, r_j) and G_i quadratic; the device (or tail()) supplies G_i(0), G_i(1), G_i(2).
struct Sumcheck1 {
    using F = host::Fr;
    ProofStream* io = nullptr;
    int L = 0;
    std::vector<F> tau, r;  // r: the challenges drawn so far (r_x in the end)
    F Cc = F::one(), claim = F::zero();

    Sumcheck1() = default;
    Sumcheck1(ProofStream& s, std::vector<F> tau_) : io(&s), L((int)tau_.size()), tau(std::move(tau_)) { r.reserve(L); }

    // Before the next round's launch: can its G(1) be derived? From round 2 on, P_i(0) + P_i(1) =
    // P_{i-1}(r_{i-1}) (the claim) is an identity of the folded tables, so G(1) follows from G(0):
    // Cc (1 - tau) G(0) + Cc tau G(1) = claim, unless Cc tau = 0. The kernel then skips it (2 of its 12
    // Fr products per pair). Exact field arithmetic: the same message bytes.
    bool derivable() const { return !r.empty() && !(Cc * tau[r.size()]).is_zero(); }

    // The next round from its three sums (over all ranks): message, challenge, claim. gs[1] is read only
    // if the round is not derivable or `check` is set (then compared with the derived value).
    void device_round(F gs[3], bool check) {
        const int i = (int)r.size() + 1;
        const F& t = tau[i - 1];
        if (derivable()) {
            const F ct = Cc * t;
            const F d1 = (claim - (Cc - ct) * gs[0]) * ct.inv();
            if (check && !(d1 == gs[1]))
                throw SpxError(kSumcheck, "sumcheck 1 round " + std::to_string(i) + ": derived G(1) differs from the device's");
            gs[1] = d1;
        }
        const F ch = message(t, gs);
        const F eqc = eq1(t, ch);
        claim = Cc * eqc * quad_at(gs, ch);  // P_i(r_i)
        Cc = Cc * eqc;
    }

    // this rank's half-tables from its copied-back Az, Bz, Cz (tn entries each), bound at the last challenge
    std::vector<F> bind(const uint8_t* bytes, uint32_t tn) const { return bind_tables(bytes, 3, tn, r.back()); }

    // The remaining rounds on the host, from the bound tables of all ranks (rank_order). Returns
    // (Az, Bz, Cz)(r_x), the fourth round's message.
    std::vector<F> tail(std::vector<F> t) {
        for (int i = (int)r.size() + 1; i <= L; ++i) {
            const size_t half = t.size() / 6;
            const int c = i - 1;
            F gs[3] = {F::zero(), F::zero(), F::zero()};
            for (size_t b = 0; b < half; ++b) {
                F e = F::one();  // eq(tau_{c+1..L-1}, b)
                for (int j = c + 1; j < L; ++j) e *= ((b >> (j - c - 1)) & 1) ? tau[j] : F::one() - tau[j];
                F x0[3], x1[3], y[3];
                for (int m = 0; m < 3; ++m) {
                    x0[m] = t[2 * half * m + 2 * b];
                    x1[m] = t[2 * half * m + 2 * b + 1];
                    y[m] = x1[m] + x1[m] - x0[m];
                }
                gs[0] += (x0[0] * x0[1] - x0[2]) * e;
                gs[1] += (x1[0] * x1[1] - x1[2]) * e;
                gs[2] += (y[0] * y[1] - y[2]) * e;
            }
            const F ch = message(tau[c], gs);
            Cc = Cc * eq1(tau[c], ch);
            fold_tables(t, 3, half, ch);
        }
        return t;
    }

   private:
    F message(const F& t, const F gs[3]) {
        const std::vector<F> msg = sc1_message(Cc, t, gs, L);
        io->emit_vec(msg.data(), msg.size());
        r.push_back(io->T.rand_fr());
        return r.back();
    }
};

// ---------------------------------------------------------------- sumcheck #2 (lib.rs:114-131)
// sum_y M_rx(y) z(y): a round's message is its three sums P(0), P(1), P(2) themselves.
struct Sumcheck2 {
    using F = host::Fr;
    ProofStream* io = nullptr;
    int L = 0;
    std::vector<F> r;  // the challenges drawn so far (r_y in the end)
    F claim = F::zero();

    Sumcheck2() = default;
    Sumcheck2(ProofStream& s, int L_) : io(&s), L(L_) { r.reserve(L); }

    // from round 2 on, P(1) = claim - P(0) (the folded tables' identity): the kernel skips it
    bool derivable() const { return !r.empty(); }

    void device_round(F ps[3], bool check) {
        if (derivable()) {
            const F d1 = claim - ps[0];
            if (check && !(d1 == ps[1]))
                throw SpxError(kSumcheck, "sumcheck 2 round " + std::to_string(r.size() + 1) + ": derived P(1) differs from the device's");
            ps[1] = d1;
        }
        claim = quad_at(ps, message(ps));  // P_i(r_i)
    }

    // this rank's half-tables from its copied-back M_rx and z (tn entries each)
    std::vector<F> bind(const uint8_t* bytes, uint32_t tn) const { return bind_tables(bytes, 2, tn, r.back()); }

    void tail(std::vector<F> t) {
        for (int i = (int)r.size() + 1; i <= L; ++i) {
            const size_t half = t.size() / 4;
            F ps[3] = {F::zero(), F::zero(), F::zero()};
            for (size_t b = 0; b < half; ++b) {
                const F m0 = t[2 * b], m1 = t[2 * b + 1], z0 = t[2 * half + 2 * b], z1 = t[2 * half + 2 * b + 1];
                ps[0] += m0 * z0;
                ps[1] += m1 * z1;
                ps[2] += (m1 + m1 - m0) * (z1 + z1 - z0);
            }
            fold_tables(t, 2, half, message(ps));
        }
    }

   private:
    F message(const F ps[3]) {
        io->emit_vec(ps, 3);
        r.push_back(io->T.rand_fr());
        return r.back();
    }
};

}  // namespace spx
