"""The host half of both sumchecks (r1cs-spartan_amd/csrc/sumcheck_host.hpp: what prove() and
prove_group() run between a round kernel's sums and the next launch, and the rounds they run on the host
altogether) against the Python oracle, without a GPU. tests/native/sumcheck_host_check.cpp drives the
header as prove() does, playing the device itself, for every split of the L rounds between device and
host: G = 1, 2, 4 ranks and a host tail of up to 5 rounds, each with SPX_CHECK_DERIVED's comparison off
and on. Every split must print the oracle's message bytes and its (Az, Bz, Cz)(r_x)."""
import os
import random
import shutil
import subprocess

import pytest

from bls12_381 import R, ser_fr, ser_u64
from spartan import MLSumcheckProver, eq_extension, mle_eval, prover_msg_bytes
from transcript import InjectedChallenges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MSG1 = "sumcheck 1 round 2: derived G(1) differs from the device's"
MSG2 = "sumcheck 2 round 2: derived P(1) differs from the device's"
K_SUMCHECK = 2  # SPX_SUMCHECK (include/spartan_hip.h)


def _cases():
    """(L, seed, corrupt, tau, [az, bz, cz, m, z])"""
    rng = random.Random(0x5C0DE)
    fr = lambda: rng.randrange(R)
    out = []
    for L in range(1, 8):  # random tables
        out.append((L, 100 + L, 0, [fr() for _ in range(L)], [[fr() for _ in range(1 << L)] for _ in range(5)]))
    for L in (1, 4, 7):  # all zeros
        out.append((L, 200 + L, 0, [fr() for _ in range(L)], [[0] * (1 << L) for _ in range(5)]))
    # tau = 0 at round 2 (Cc tau = 0: G(1) is not derivable, the device's value is the message's) and
    # tau = 1 at round 3 (the claim does not depend on G(0)); device rounds at the splits with few host
    # rounds, host rounds at the others; and the two the other way round, one round later
    for L, at0, at1 in ((5, 1, 2), (7, 1, 2), (7, 3, 2), (3, 1, 2)):
        tau = [fr() for _ in range(L)]
        tau[at0], tau[at1] = 0, 1
        out.append((L, 300 + L, 0, tau, [[fr() for _ in range(1 << L)] for _ in range(5)]))
    for corrupt in (1, 2):  # the device's value at 1 off by one in a derivable round
        out.append((4, 400, corrupt, [fr() for _ in range(4)], [[fr() for _ in range(16)] for _ in range(5)]))
    return out


def _oracle(L, seed, tau, tabs):
    """the bytes both sumchecks add to a proof (IndexInfo, round count, messages; round 4's message
    between them) and (va, vb, vc), with the rounds' challenges injected"""
    az, bz, cz, m, z = tabs
    fs = InjectedChallenges(seed)
    eq = eq_extension(tau)
    sc = MLSumcheckProver([[az, bz] + eq, [[(-x) % R for x in cz]] + eq], L)
    out = [sc.info_bytes(), ser_u64(L)]
    ch = None
    for _ in range(L):
        msg = sc.prove_round(ch)
        out.append(prover_msg_bytes(msg))
        ch = fs.rand_fr()
    r_x = sc.randomness + [ch]
    vabc = [mle_eval(t, r_x) for t in (az, bz, cz)]
    out += [ser_fr(x) for x in vabc]
    sc2 = MLSumcheckProver([[m, z]], L)
    out += [sc2.info_bytes(), ser_u64(L)]
    ch = None
    for _ in range(L):
        out.append(prover_msg_bytes(sc2.prove_round(ch)))
        ch = fs.rand_fr()
    return b"".join(out).hex(), b"".join(ser_fr(x) for x in vabc).hex()


def test_sumcheck_host_against_oracle(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "schost")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-w", "-I", os.path.join(ROOT, "r1cs-spartan_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "sumcheck_host_check.cpp"), "-o", exe])
    cases = _cases()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("%d\n" % len(cases))
        for L, seed, corrupt, tau, tabs in cases:
            f.write("%d %d %d\n" % (L, seed, corrupt))
            f.write(" ".join(ser_fr(x).hex() for x in tau) + "\n")
            for t in tabs:
                f.write(" ".join(ser_fr(x).hex() for x in t) + "\n")
    lines = subprocess.check_output([exe, path], timeout=120).decode().splitlines()
    want = [_oracle(L, seed, tau, tabs) for L, seed, _c, tau, tabs in cases]
    seen = [set() for _ in cases]
    for line in lines:
        ci, G, ht, check, rest = line.split(" ", 4)
        ci, G, ht, check = int(ci), int(G), int(ht), int(check)
        L, corrupt = cases[ci][0], cases[ci][2]
        seen[ci].add((G, ht, check))
        if corrupt and check:  # the comparison catches the corrupted value, with the product's message
            assert rest == "THROW %d %s" % (K_SUMCHECK, MSG1 if corrupt == 1 else MSG2), line[:200]
        else:  # (a corrupted value that is not compared is not used either: the same bytes)
            assert tuple(rest.split(" ")) == want[ci], (ci, L, G, ht, check)
    for ci, (L, _s, corrupt, _t, _tabs) in enumerate(cases):  # every split ran
        expect = {(1, 0, c) for c in (0, 1)} if corrupt else {
            (1 << g, max(0, min(cap, L - g - 1)), c)
            for g in range(3) if L - g - 1 >= 0 for cap in range(min(5, L - 1) + 1) for c in (0, 1)}
        assert seen[ci] == expect, (ci, L)
