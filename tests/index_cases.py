"""The device layouts of an index, restated in plain Python from their description, and the
matrices that reach every branch of them. Shared by test_index_cases.py (pins this reference against
the oracle, no GPU) and test_gpu_index_build.py (the host and the GPU builder against it).

A matrix is a list of n rows, a row a list of (value, column) in the caller's order. reference() gives,
for rank `rank` of G, every part of spx_index_export by name: the index parts as bytes, the value parts
as lists of canonical integers."""
import random
import struct

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
LONG_ROW = 64  # rows longer than this take the chunked path
CHUNK = 4096
LONG_COL = 62  # columns longer than this leave the stream
WINDOW = 16  # slices of 64 columns per sorting window
COL_NONE = 0xFFFFFFFF
SLICED_MIN_N = 1 << 12

VALUE_PARTS = ("ROWS_VAL_A", "ROWS_VAL_B", "ROWS_VAL_C", "SLICED_VAL", "COLS_VAL", "LONGC_VAL_A", "LONGC_VAL_B", "LONGC_VAL_C")


def _u32(xs):
    return struct.pack("<%dI" % len(xs), *xs)


def _u64(xs):
    return struct.pack("<%dQ" % len(xs), *xs)


def _long_tables(segments):
    """segments: (m, x, first entry, entries) of the long rows / columns, in table order"""
    chunks, lrows = [], []
    for m, x, begin, cnt in segments:
        c0 = len(chunks)
        for k in range(0, cnt, CHUNK):
            chunks.append((m, begin + k, begin + min(k + CHUNK, cnt)))
        lrows.append((m, c0, len(chunks), x))
    return (b"".join(struct.pack("<IIQQ", m, 0, b, e) for m, b, e in chunks),
            b"".join(struct.pack("<IIIIQ", m, c0, c1, 0, x) for m, c0, c1, x in lrows))


def live_columns(mats, lo, nl):
    """cols[y][m] = [(row, value)] of local column y of matrix m, rows ascending; of the entries of a row
    that repeat a column only the last counts"""
    cols = [[[], [], []] for _ in range(nl)]
    for m in range(3):
        for x, row in enumerate(mats[m]):
            last = {}
            for v, c in row:
                last[c] = v
            for c in sorted(last):
                if lo <= c < lo + nl:
                    cols[c - lo][m].append((x, last[c]))
    return cols


def reference(mats, rank=0, G=1):
    n = len(mats[0])
    nl = n // G
    lo = rank * nl
    out = {}
    local = [mats[m][lo : lo + nl] for m in range(3)]
    sliced = n >= SLICED_MIN_N and all(len(r) <= 1 for m in range(3) for r in local[m])
    names = "ABC"
    if sliced:
        ents = []
        for m in range(3):
            for xl, row in enumerate(local[m]):
                v, c = row[0] if row else (0, lo + xl)
                ents.append((c, m, xl, v))
        ents.sort(key=lambda e: e[:3])
        out["SLICED_COL"] = _u32([e[0] for e in ents])
        out["SLICED_DST"] = _u32([e[2] | e[1] << 30 for e in ents])
        out["SLICED_VAL"] = [e[3] for e in ents]
        for m in range(3):
            out["ROWS_PTR_" + names[m]] = out["ROWS_IDX_" + names[m]] = b""
            out["ROWS_VAL_" + names[m]] = []
        out["ROWS_CHUNKS"] = out["ROWS_LROWS"] = b""
    else:
        out["SLICED_COL"] = out["SLICED_DST"] = b""
        out["SLICED_VAL"] = []
        segs = []
        for m in range(3):
            ptr = [0]
            for xl, row in enumerate(local[m]):
                if len(row) > LONG_ROW:
                    segs.append((m, xl, ptr[-1], len(row)))
                ptr.append(ptr[-1] + len(row))
            out["ROWS_PTR_" + names[m]] = _u64(ptr)
            out["ROWS_IDX_" + names[m]] = _u32([c for row in local[m] for _, c in row])
            out["ROWS_VAL_" + names[m]] = [v for row in local[m] for v, _ in row]
        out["ROWS_CHUNKS"], out["ROWS_LROWS"] = _long_tables(segs)
    # ---- column stream
    cols = live_columns(mats, lo, nl)
    full = [sum(len(c) for c in col) for col in cols]
    slen = [0 if L > LONG_COL else L for L in full]
    nslices = (nl + 63) // 64
    lanes = [COL_NONE] * (64 * nslices)
    slices = []
    tot = 0
    win = 64 * WINDOW
    for w0 in range(0, nl, win):
        order = sorted(range(w0, min(w0 + win, nl)), key=lambda y: -slen[y])  # stable: ties by column
        for s0 in range(0, len(order), 64):
            part = order[s0 : s0 + 64]
            for l, y in enumerate(part):
                lanes[w0 + s0 + l] = y | slen[y] << 26
            mx = max(slen[y] for y in part)
            slices.append((tot, mx))
            tot += 64 * mx
    rowm = [0] * tot
    val = [0] * tot
    for si in range(nslices):
        for l in range(64):
            info = lanes[64 * si + l]
            if info == COL_NONE or not info >> 26:
                continue
            y = info & 0x3FFFFFF
            j = 0
            for m in range(3):
                for x, v in cols[y][m]:
                    e = slices[si][0] + 64 * j + l
                    rowm[e] = x | m << 30
                    val[e] = v
                    j += 1
    out["COLS_SLICES"] = b"".join(struct.pack("<QII", off, mx, 0) for off, mx in slices)
    out["COLS_LANES"] = _u32(lanes)
    out["COLS_ROWM"] = _u32(rowm)
    out["COLS_VAL"] = val
    segs = []
    for m in range(3):
        idx, vals = [], []
        for y in range(nl):
            if full[y] > LONG_COL and cols[y][m]:
                segs.append((m, y, len(idx), len(cols[y][m])))
                idx += [x for x, _ in cols[y][m]]
                vals += [v for _, v in cols[y][m]]
        out["LONGC_IDX_" + names[m]] = _u32(idx)
        out["LONGC_VAL_" + names[m]] = vals
    out["LONGC_CHUNKS"], out["LONGC_LROWS"] = _long_tables(segs)
    out["_stats"] = {
        "sliced": int(sliced),
        "row_entries": 3 * nl if sliced else sum(len(r) for m in range(3) for r in local[m]),
        "col_entries": sum(full),
        "long_rows": len(out["ROWS_LROWS"]) // 24,
        "long_cols": sum(L > LONG_COL for L in full),
    }
    return out


# ---------------------------------------------------------------- the cases
def _rand_rows(rs, n, lo_cnt, hi_cnt):
    return [[(rs.randrange(R), rs.randrange(n)) for _ in range(rs.randint(lo_cnt, hi_cnt))] for _ in range(n)]


def _single(rs, n, col=None):
    return [[(rs.randrange(R), rs.randrange(n) if col is None else col(x))] for x in range(n)]


def _small(n):
    def make(oc):
        rs = random.Random(1000 + n)
        return [_rand_rows(rs, n, 0, 3) for _ in range(3)]

    return make


def _uniform(log_n, holes=False):
    def make(oc):
        inst = oc.Instance(0, log_n, 3, 5000 + log_n)
        mats = [M.to_rows() for M in inst.mats]
        if holes:
            for x in range(0, len(mats[1]), 5):
                mats[1][x] = []
        return mats

    return make


def _dups6(oc):
    """rows with columns repeated inside a row: pairs, a triple, a repeat as the row's last two entries, a
    repeat with other entries between"""
    n = 64
    rs = random.Random(66)
    mats = [_rand_rows(rs, n, 1, 4) for _ in range(3)]
    v = lambda: rs.randrange(R)  # noqa: E731
    mats[0][3] = [(v(), 9), (v(), 9), (v(), 9)]
    mats[0][4] = [(v(), 1), (v(), 17), (v(), 17)]
    mats[1][5] = [(v(), 20), (v(), 2), (v(), 40), (v(), 20)]
    mats[2][63] = [(v(), 63), (v(), 0), (v(), 63), (v(), 0), (v(), 63)]
    mats[2][0] = [(v(), 5), (v(), 5)]
    for m in range(3):
        for x in range(8, n, 3):
            row = mats[m][x]
            row.insert(rs.randrange(len(row) + 1), (v(), rs.choice(row)[1]))
    return mats


def _longrow7(oc):
    n = 128
    rs = random.Random(77)
    mats = [_rand_rows(rs, n, 0, 2) for _ in range(3)]
    mats[0][3] = [(rs.randrange(R), c) for c in rs.sample(range(n), 64)]  # exactly kLongRow: the short path
    mats[1][70] = [(rs.randrange(R), c) for c in rs.sample(range(n), 65)]  # one more: the long path
    mats[2][127] = [(rs.randrange(R), c) for c in rs.sample(range(n), 100)]
    return mats


def _ref13(oc):
    return [M.to_rows() for M in oc.Instance(1, 13, 3, 1313).mats]


def _longcol7(oc):
    """column 10 holds exactly 62 live entries (the last stream column), column 20 63 (the first long one);
    column 30 would hold 63 but for a repeat inside a row; columns 100.. stay empty"""
    n = 128
    rs = random.Random(707)
    v = lambda: rs.randrange(R)  # noqa: E731
    mats = [[[(v(), 40 + rs.randrange(50))] for _ in range(n)] for _ in range(3)]
    for x in range(31):
        mats[0][x].append((v(), 10))
        mats[1][x].insert(0, (v(), 10))
    for x in range(32):
        mats[0][x + 60].append((v(), 20))
    for x in range(31):
        mats[2][x + 50].append((v(), 20))
    for x in range(31):
        mats[0][x].append((v(), 30))
        mats[1][x + 90].append((v(), 30))
    mats[1][90].append((v(), 30))  # 63 entries in the rows, 62 live
    return mats


def _longcol13(oc):
    """single-entry rows (the sliced list) with a column of 5000 entries in A: two chunks of longc"""
    n = 1 << 13
    rs = random.Random(1307)
    a = _single(rs, n, lambda x: 7 if x < 5000 else 8 + rs.randrange(n - 8))
    return [a, _single(rs, n), _single(rs, n)]


def _windows(log_n):
    def make(oc):
        n = 1 << log_n
        rs = random.Random(40 + log_n)
        a = _single(rs, n, lambda x: x)  # every column once
        b = _single(rs, n, lambda x: x & ~3)  # every 4th column 4 more
        c = _single(rs, n, lambda x: (x * 5) % n | 1)  # the odd columns 2 more
        for x in range(0, n, 64):
            c[x].append((rs.randrange(R), (x + 600) % n))  # a few longer ones, also in the next window
        return [a, b, c]

    return make


CASES = {
    "n2": _small(2),
    "n4": _small(4),
    "n32": _small(32),
    "uniform6": _uniform(6),
    "uniform12": _uniform(12),
    "uniform12_holes": _uniform(12, True),
    "dups6": _dups6,
    "longrow7": _longrow7,
    "ref13": _ref13,
    "longcol7": _longcol7,
    "longcol13": _longcol13,
    "windows10": _windows(10),
    "windows11": _windows(11),
}
# the sharded forms of the GPU test (every case is sharded in the CPU test)
SHARDED = [(name, G) for G in (2, 4) for name in ("dups6", "uniform6", "longrow7", "uniform12", "uniform12_holes")]

_built = {}


def case(oc, name):
    """the case's matrices as rows and as oracle CsrMatrix objects (built once, not to be changed)"""
    if name not in _built:
        rows = CASES[name](oc)
        _built[name] = (rows, [oc.CsrMatrix.from_rows(r) for r in rows])
    return _built[name]


def worlds(n):
    return [G for G in (1, 2, 4) if G <= n // 2]
