"""The MSM bucket weighting's schedule (r1cs-spartan_amd/csrc/msm_impl.hpp: k_tree_chunk, k_tree_level,
k_tree_top; the hand-over level from msm_plan in msm_common.hip) restated over a toy additive group:
integers mod a 61-bit prime stand in for points, 0 for the point at infinity. The restatement keeps the
kernels' slot arithmetic (which slots a level reads and writes, the top kernel's local arrays, the
root's terms), so an index that is wrong there is wrong here, and checks that a level never reads a
slot it also writes.

  value = sum_u (u + 1) X_u = F0 + m sum_l 2^l U_l      (chunks of m = 2^lgm buckets)
  share = G value - (G - 1 - sel) S                       (a rank's part of a split instance)

Used by tests/test_weighting_cases.py (no GPU)."""
P61 = (1 << 61) - 1
K_TREE_CHUNK_LOG = 2  # kTreeChunkLog
K_TOP_NODES = 32      # kTopNodes
K_TOP_ELEMS = 192     # kTopElems


def chunk_log(lb):
    return min(lb - 1, K_TREE_CHUNK_LOG)


def direct(X):
    """sum_u (u + 1) X_u"""
    return sum((u + 1) * x for u, x in enumerate(X)) % P61


def parent_tree(X, lgm):
    """the (F, S, D) recurrence this schedule replaces: leaf (F, S, D = m S) per chunk, then
    parent = (F_l + D_r + F_r, S_l + S_r, 2 (D_l + D_r)); returns the root's (F, S)"""
    m = 1 << lgm
    nodes = []
    for k in range(len(X) >> lgm):
        c = X[k * m : (k + 1) * m]
        s = sum(c) % P61
        nodes.append((direct(c), s, (m * s) % P61))
    while len(nodes) > 1:
        nodes = [((l[0] + r[2] + r[0]) % P61, (l[1] + r[1]) % P61, (2 * (l[2] + r[2])) % P61)
                 for l, r in zip(nodes[0::2], nodes[1::2])]
    return nodes[0][0], nodes[0][1]


def leaf(X, lgm):
    """k_tree_chunk: per chunk the running sum from the top bucket down (run += X_j, F += run)"""
    m = 1 << lgm
    F, S = [], []
    for k in range(len(X) >> lgm):
        run = f = 0
        for j in range(m - 1, -1, -1):
            run = (run + X[k * m + j]) % P61
            f = (f + run) % P61
        F.append(f)
        S.append(run)
    return F, S


def top_from(maxc, levels, top_nodes=K_TOP_NODES, top_elems=K_TOP_ELEMS):
    """msm_plan: the first level k_tree_top runs (levels below it: one k_tree_level launch each)"""
    for lv in range(1, levels + 1):
        n = max(1, maxc >> (lv - 1))
        if n <= top_nodes and n + lv * max(1, n // 2) <= top_elems:
            return lv
    raise AssertionError("no level fits the top kernel")


def level(R, nout, cnt, F, S):
    """k_tree_level for one instance: (R + 1) sums per node of the level's nout = max(1, cnt >> R),
    in place; returns the additions done"""
    h = 1 << (R - 1)
    reads, writes, adds = set(), set(), 0
    for comp in range(R + 1):
        for k in range(nout):
            x = (k << R) + (0 if comp < 2 else 1 << (comp - 2))
            if x + h >= cnt:
                continue
            arr, tag = (F, "F") if comp == 0 else (S, "S")
            assert (tag, x) not in writes, "two sums write one slot"
            reads.add((tag, x + h))
            writes.add((tag, x))
            arr[x] = (arr[x] + arr[x + h]) % P61
            adds += 1
    assert not (reads & writes), "a level reads a slot it writes"
    return adds


def top(R0, lb, lg, sel, cnt, F, S, top_elems=K_TOP_ELEMS):
    """k_tree_top for one instance handed over after level R0: the remaining levels in the local
    arrays, the root's terms and their pairwise sum; returns (value or share, additions of its levels)"""
    lgm = chunk_log(lb)
    L = lb - lgm
    n = max(1, cnt >> R0)
    n2 = max(1, n >> 1)
    nu = min(R0, L)
    ns = 1 + nu
    assert n + ns * n2 <= top_elems, "the instance's sums pass the top kernel's buffer"
    buf = [None] * top_elems

    def plain_src(j, k):  # plain array j (0: F, 1 + l: U_l), node k of the hand-over level
        if j == 0:
            return F[k << R0]
        return S[(k << R0) + (1 << (j - 1))]

    for t in range(n):
        buf[t] = S[t << R0]
    if n == 1:
        for j in range(ns):
            buf[1 + j] = plain_src(j, 0)
    ops = 0
    r = 1
    while (1 << r) <= n:
        h, nout, per = 1 << (r - 1), n >> r, r + ns
        reads, writes = set(), set()
        for task in range(per * nout):
            comp, k = divmod(task, nout)
            if comp < r:
                dst = (k << r) + (0 if comp == 0 else 1 << (comp - 1))
                a, b = buf[dst], buf[dst + h]
                reads.add(dst + h)
            else:
                j = comp - r
                if r == 1:
                    dst = n + j * n2 + k
                    a, b = plain_src(j, 2 * k), plain_src(j, 2 * k + 1)
                else:
                    dst = n + j * n2 + (k << (r - 1))
                    a, b = buf[dst], buf[dst + (h >> 1)]
                    reads.add(dst + (h >> 1))
            assert dst not in writes
            writes.add(dst)
            buf[dst] = (a + b) % P61
            ops += 1
        assert not (reads & writes), "a level reads a slot it writes"
        r += 1
    ks = ((1 << lg) - 1 - sel) if lg else 0
    nterm = L + 1 + (1 if ks else 0)
    assert nterm <= 25
    terms = []
    for g in range(nterm):
        if g == L + 1:
            v = (-ks * buf[0]) % P61
        else:
            src, nd = n, lg
            if g:
                l = g - 1
                src = n + (1 + l) * n2 if l < nu else 1 << (l - R0)
                nd += lgm + l
            v = (buf[src] << nd) % P61
        terms.append(v)
    buf[:nterm] = terms
    s = 1
    while s < nterm:
        for g in range(nterm):
            x = 2 * s * g
            if x + s < nterm:
                buf[x] = (buf[x] + buf[x + s]) % P61
        s <<= 1
    return buf[0], ops


def run_batch(insts, top_nodes=K_TOP_NODES, top_elems=K_TOP_ELEMS):
    """a batch as msm_run_t runs it: insts = [(X, lg, sel)] with len(X) = 2^lb local buckets; every
    instance runs the levels the widest one needs. Returns ([value or share], additions below the root
    per instance)"""
    st = []
    for X, lg, sel in insts:
        lb = len(X).bit_length() - 1
        assert lb >= 1 and len(X) == 1 << lb
        lgm = chunk_log(lb)
        F, S = leaf(X, lgm)
        st.append([lb, lg, sel, len(F), F, S, 2 * len(X)])
    levels = max(s[0] - chunk_log(s[0]) for s in st)
    maxc = max(s[3] for s in st)
    tf = top_from(maxc, levels, top_nodes, top_elems)
    for lv in range(1, tf):
        for s in st:
            s[6] += level(lv, max(1, s[3] >> lv), s[3], s[4], s[5])
    out = []
    adds = []
    for lb, lg, sel, cnt, F, S, a in st:
        v, ta = top(tf - 1, lb, lg, sel, cnt, F, S, top_elems)
        out.append(v)
        adds.append(a + ta)
    return out, adds
