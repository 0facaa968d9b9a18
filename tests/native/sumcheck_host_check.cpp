// Host check of both sumchecks' host halves (r1cs-spartan_amd/csrc/sumcheck_host.hpp), driven as
// prove() drives them, with the device played by a few lines here: per emulated rank, the three sums of
// a round over its block of the current tables (sc_sums*), the fold, and the sum over the ranks.
//   sumcheck_host_check CASES
// CASES (written by tests/test_sumcheck_host.py): the case count, then per case `L seed corrupt`, tau
// (L), and the tables Az, Bz, Cz, M, z (2^L each), every Fr as 64 hex digits (canonical, little-endian).
// For every split of the rounds between device and host -- G in {1, 2, 4} ranks, host tail cap 0..5,
// the tail's length by prove()'s formula -- one line per run:
//   <case> <G> <ht> <check> <proof bytes, hex> <va vb vc, hex>      or      ... THROW <code> <message>
// corrupt = 1 / 2: the device's value at 1 of sumcheck 1 / 2's round 2 is off by one (G = 1, no tail).
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "sumcheck_host.hpp"

using F = spx::host::Fr;
using Tab = std::vector<F>;

static F from_hex(const std::string& h) {
    uint8_t b[32];
    for (int i = 0; i < 32; ++i) b[i] = (uint8_t)std::stoi(h.substr(2 * i, 2), nullptr, 16);
    F x;
    if (h.size() != 64 || !spx::host::fr_from_bytes(x, b)) throw std::runtime_error("bad field element: " + h);
    return x;
}
static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) s += d[p[i] >> 4], s += d[p[i] & 15];
    return s;
}

// ---- the device: a rank's block of a table, folded in place, and a round's sums over it
static void fold(Tab& t, const F& r) {
    for (size_t b = 0; b < t.size() / 2; ++b) t[b] = t[2 * b] + r * (t[2 * b + 1] - t[2 * b]);
    t.resize(t.size() / 2);
}
// sum over the block's pairs b of eq(tau_{c+1..}, B) (A B - C)(t, b) at t = 0, 1, 2; B: the pair's global index
static void sc_sums1(const Tab t[3], const std::vector<F>& tau, int c, size_t pair0, F out[3]) {
    const int L = (int)tau.size();
    for (size_t b = 0; b < t[0].size() / 2; ++b) {
        F e = F::one();
        for (int j = c + 1; j < L; ++j) e = e * ((((pair0 + b) >> (j - c - 1)) & 1) ? tau[j] : F::one() - tau[j]);
        F v[3][3];  // [table][t]
        for (int m = 0; m < 3; ++m) {
            v[m][0] = t[m][2 * b];
            v[m][1] = t[m][2 * b + 1];
            v[m][2] = v[m][1] + (v[m][1] - v[m][0]);
        }
        for (int k = 0; k < 3; ++k) out[k] = out[k] + e * (v[0][k] * v[1][k] - v[2][k]);
    }
}
static void sc_sums2(const Tab t[2], F out[3]) {
    for (size_t b = 0; b < t[0].size() / 2; ++b)
        for (int k = 0; k < 3; ++k) {
            const F kk = F::from_u64((uint64_t)k);
            out[k] = out[k] + (t[0][2 * b] + kk * (t[0][2 * b + 1] - t[0][2 * b])) * (t[1][2 * b] + kk * (t[1][2 * b + 1] - t[1][2 * b]));
        }
}
// a rank's tables as the device's Montgomery bytes, table after table
static std::vector<uint8_t> dev_bytes(const Tab* t, int nt) {
    std::vector<uint8_t> b;
    for (int m = 0; m < nt; ++m)
        for (const F& x : t[m]) b.insert(b.end(), (const uint8_t*)x.v, (const uint8_t*)x.v + 32);
    return b;
}

struct Case {
    int L, corrupt;
    uint64_t seed;
    std::vector<F> tau;
    Tab tab[5];  // Az, Bz, Cz, M, z
};

// one proof's two sumchecks with G ranks and the last `ht` local rounds on the host
static void run(const Case& c, int G, int ht, bool check, spx::ProofStream& io, std::vector<F>& vabc) {
    const int L = c.L, g = G == 1 ? 0 : (G == 2 ? 1 : 2), dev_rounds = L - g - ht;
    const size_t nl = ((size_t)1 << L) / G;
    const uint32_t tn = 2u << ht;
    const F garbage = F::from_u64(0xBAD);  // what a kernel that skips the value at 1 may leave there
    // ---- sumcheck 1
    std::vector<std::vector<Tab>> t1(G, std::vector<Tab>(3));
    for (int r = 0; r < G; ++r)
        for (int m = 0; m < 3; ++m) t1[r][m].assign(c.tab[m].begin() + r * nl, c.tab[m].begin() + (r + 1) * nl);
    io.sumcheck_header(L + 2, L);
    spx::Sumcheck1 s1(io, c.tau);
    for (int i = 1; i <= dev_rounds; ++i) {
        const bool need1 = !s1.derivable() || check;
        F gs[3] = {F::zero(), F::zero(), F::zero()};
        for (int r = 0; r < G; ++r) {
            if (i >= 2)
                for (int m = 0; m < 3; ++m) fold(t1[r][m], s1.r[i - 2]);
            sc_sums1(t1[r].data(), c.tau, i - 1, r * (nl >> i), gs);
        }
        if (!need1) gs[1] = garbage;
        if (c.corrupt == 1 && i == 2) gs[1] = gs[1] + F::one();
        s1.device_round(gs, check);
    }
    {
        std::vector<F> all;
        for (int r = 0; r < G; ++r) {
            const std::vector<F> mine = s1.bind(dev_bytes(t1[r].data(), 3).data(), tn);
            all.insert(all.end(), mine.begin(), mine.end());
        }
        vabc = s1.tail(spx::rank_order(all, 3, G));
    }
    io.emit([&](spx::Ser& s) {
        for (int m = 0; m < 3; ++m) s.fr(vabc[m]);
    });
    // ---- sumcheck 2
    std::vector<std::vector<Tab>> t2(G, std::vector<Tab>(2));
    for (int r = 0; r < G; ++r)
        for (int m = 0; m < 2; ++m) t2[r][m].assign(c.tab[3 + m].begin() + r * nl, c.tab[3 + m].begin() + (r + 1) * nl);
    io.sumcheck_header(2, L);
    spx::Sumcheck2 s2(io, L);
    for (int i = 1; i <= dev_rounds; ++i) {
        const bool need1 = !s2.derivable() || check;
        F ps[3] = {F::zero(), F::zero(), F::zero()};
        for (int r = 0; r < G; ++r) {
            if (i >= 2)
                for (int m = 0; m < 2; ++m) fold(t2[r][m], s2.r[i - 2]);
            sc_sums2(t2[r].data(), ps);
        }
        if (!need1) ps[1] = garbage;
        if (c.corrupt == 2 && i == 2) ps[1] = ps[1] + F::one();
        s2.device_round(ps, check);
    }
    if (g + ht > 0) {
        std::vector<F> all;
        for (int r = 0; r < G; ++r) {
            const std::vector<F> mine = s2.bind(dev_bytes(t2[r].data(), 2).data(), tn);
            all.insert(all.end(), mine.begin(), mine.end());
        }
        s2.tail(spx::rank_order(all, 2, G));
    }
    if ((int)s1.r.size() != L || (int)s2.r.size() != L) throw std::runtime_error("a sumcheck did not run L rounds");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int ncases = 0;
    in >> ncases;
    for (int ci = 0; ci < ncases; ++ci) {
        Case c;
        std::string h;
        in >> c.L >> c.seed >> c.corrupt;
        for (int i = 0; i < c.L; ++i) in >> h, c.tau.push_back(from_hex(h));
        for (auto& t : c.tab)
            for (size_t x = 0; x < (size_t)1 << c.L; ++x) in >> h, t.push_back(from_hex(h));
        if (!in) {
            fprintf(stderr, "truncated case file\n");
            return 2;
        }
        for (int g = 0; g <= 2 && c.L - g - 1 >= 0; ++g)
            for (int cap = 0; cap <= std::min(5, c.L - 1); ++cap)
                for (int check = 0; check <= 1; ++check) {
                    const int ht = std::max(0, std::min(cap, c.L - g - 1));  // prove()'s ht1 with kGroupHostTail = cap
                    if (c.corrupt && (g || ht)) continue;
                    spx::ProofStream io{spx::Transcript(true, c.seed), {}};
                    std::vector<F> vabc;
                    printf("%d %d %d %d ", ci, 1 << g, ht, check);
                    try {
                        run(c, 1 << g, ht, check != 0, io, vabc);
                        spx::Ser v;
                        for (const F& x : vabc) v.fr(x);
                        printf("%s %s\n", hex(io.proof.b.data(), io.proof.b.size()).c_str(), hex(v.b.data(), v.b.size()).c_str());
                    } catch (const spx::SpxError& e) {
                        printf("THROW %d %s\n", e.code, e.what());
                    }
                }
    }
    return 0;
}
