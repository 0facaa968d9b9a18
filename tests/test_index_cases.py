"""Pins the Python restatement of the index layouts (index_cases.py) without a GPU: multiplied out, the
row layout gives the oracle's sum_over_y and the column stream plus its long-column arrays the oracle's
eval_on_x (which shows the last-entry-wins rule); every case reaches the branch it is named for; and the
library declares and exports the index-build interface."""
import os
import random
import re
import struct

import pytest

import index_cases as ic

R = ic.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["spx_ctx_set_index_build", "spx_index_export", "spx_index_stats"]


def _ints(b):
    return [int.from_bytes(b[i : i + 32], "little") for i in range(0, len(b), 32)]


def _u32s(b):
    return struct.unpack("<%dI" % (len(b) // 4), b)


def _rows_times_z(ref, z, nl):
    out = [[0] * nl for _ in range(3)]
    if ref["_stats"]["sliced"]:
        for c, d, v in zip(_u32s(ref["SLICED_COL"]), _u32s(ref["SLICED_DST"]), ref["SLICED_VAL"]):
            out[d >> 30][d & 0x3FFFFFFF] = (out[d >> 30][d & 0x3FFFFFFF] + v * z[c]) % R
        return out
    for m, nm in enumerate("ABC"):
        ptr = struct.unpack("<%dQ" % (nl + 1), ref["ROWS_PTR_" + nm])
        idx, val = _u32s(ref["ROWS_IDX_" + nm]), ref["ROWS_VAL_" + nm]
        for x in range(nl):
            out[m][x] = sum(val[k] * z[idx[k]] for k in range(ptr[x], ptr[x + 1])) % R
    return out


def _cols_times_eq(ref, eq, nl):
    out = [[0] * nl for _ in range(3)]
    lanes, rowm, val = _u32s(ref["COLS_LANES"]), _u32s(ref["COLS_ROWM"]), ref["COLS_VAL"]
    slices = [struct.unpack_from("<QII", ref["COLS_SLICES"], 16 * i) for i in range(len(ref["COLS_SLICES"]) // 16)]
    for t, info in enumerate(lanes):
        if info == ic.COL_NONE:
            continue
        y, cnt = info & 0x3FFFFFF, info >> 26
        assert cnt <= slices[t // 64][1]
        for j in range(cnt):
            e = slices[t // 64][0] + 64 * j + t % 64
            out[rowm[e] >> 30][y] = (out[rowm[e] >> 30][y] + val[e] * eq[rowm[e] & 0x3FFFFFFF]) % R
    chunks = [struct.unpack_from("<IIQQ", ref["LONGC_CHUNKS"], 24 * i) for i in range(len(ref["LONGC_CHUNKS"]) // 24)]
    for i in range(len(ref["LONGC_LROWS"]) // 24):
        m, c0, c1, _, y = struct.unpack_from("<IIIIQ", ref["LONGC_LROWS"], 24 * i)
        idx, vals = _u32s(ref["LONGC_IDX_" + "ABC"[m]]), ref["LONGC_VAL_" + "ABC"[m]]
        for cm, _, b, e in chunks[c0:c1]:
            assert cm == m and 0 < e - b <= ic.CHUNK
            out[m][y] = (out[m][y] + sum(vals[k] * eq[idx[k]] for k in range(b, e))) % R
    return out


@pytest.fixture(scope="module")
def pinned(oc):
    """per case: the oracle's sum_over_y and eval_on_x of A, B, C for one z and one r_x, and eq(r_x, .)"""
    memo = {}

    def get(name):
        if name not in memo:
            rows, mats = ic.case(oc, name)
            n = len(rows[0])
            rs = random.Random(len(name) + n)
            z = [rs.randrange(R) for _ in range(n)]
            zb = b"".join(v.to_bytes(32, "little") for v in z)
            r_x = b"".join(rs.randrange(R).to_bytes(32, "little") for _ in range(n.bit_length() - 1))
            eye = oc.CsrMatrix.from_rows([[(1, x)] for x in range(n)])
            memo[name] = (z, [_ints(oc.sum_over_y(M, zb)) for M in mats], _ints(oc.eval_on_x(eye, r_x)),
                          [_ints(oc.eval_on_x(M, r_x)) for M in mats])
        return memo[name]

    return get


@pytest.mark.parametrize("name", list(ic.CASES))
def test_reference_multiplies_out(oc, pinned, name):
    rows, _ = ic.case(oc, name)
    n = len(rows[0])
    z, az, eq, ev = pinned(name)
    for G in ic.worlds(n):
        nl = n // G
        for rank in range(G):
            ref = ic.reference(rows, rank, G)
            lo = rank * nl
            got = _rows_times_z(ref, z, nl)
            assert all(got[m] == az[m][lo : lo + nl] for m in range(3)), (name, G, rank, "rows")
            got = _cols_times_eq(ref, eq, nl)
            assert all(got[m] == ev[m][lo : lo + nl] for m in range(3)), (name, G, rank, "columns")
            # padding slots are zero, lane words of absent columns are kColNone
            assert len(ref["COLS_LANES"]) == 256 * ((nl + 63) // 64)


def _st(oc, name, rank=0, G=1):
    return ic.reference(ic.case(oc, name)[0], rank, G)


def test_cases_reach_their_branches(oc):
    chunks_of = lambda ref, key: [struct.unpack_from("<IIIIQ", ref[key], 24 * i)[1:3] for i in range(len(ref[key]) // 24)]  # noqa: E731
    for name in ("n2", "n4", "n32"):  # fewer than 64 columns: a partly filled slice
        assert ic.COL_NONE in _u32s(_st(oc, name)["COLS_LANES"])
    assert _st(oc, "uniform6")["_stats"]["sliced"] == 0  # n < 2^12
    for name in ("uniform12", "uniform12_holes", "longcol13"):
        assert _st(oc, name)["_stats"]["sliced"] == 1
    holes = _st(oc, "uniform12_holes")
    zero = [i for i, v in enumerate(holes["SLICED_VAL"]) if v == 0]
    assert len(zero) >= 819 and all(  # an emptied row of B: a zero whose column is the row
        _u32s(holes["SLICED_COL"])[i] == _u32s(holes["SLICED_DST"])[i] & 0x3FFFFFFF for i in zero[:50])
    d = _st(oc, "dups6")
    assert d["_stats"]["sliced"] == 0 and d["_stats"]["col_entries"] < d["_stats"]["row_entries"]
    lr = _st(oc, "longrow7")
    assert lr["_stats"]["long_rows"] == 2  # 65 and 100 entries; the row of exactly 64 stays short
    assert all(c1 - c0 == 1 for c0, c1 in chunks_of(lr, "ROWS_LROWS"))
    ref13 = _st(oc, "ref13")
    assert ref13["_stats"]["sliced"] == 0 and any(c1 - c0 == 2 for c0, c1 in chunks_of(ref13, "ROWS_LROWS"))
    lc = _st(oc, "longcol7")
    assert lc["_stats"]["long_cols"] == 1 and len(lc["LONGC_LROWS"]) == 2 * 24  # column 20: A and C
    lens = {w & 0x3FFFFFF: w >> 26 for w in _u32s(lc["COLS_LANES"])}
    assert lens[10] == 62 and lens[30] == 62 and lens[20] == 0 and lens[120] == 0
    l13 = _st(oc, "longcol13")
    assert l13["_stats"]["long_cols"] >= 1 and [c1 - c0 for c0, c1 in chunks_of(l13, "LONGC_LROWS")][0] == 2
    for name, nwin in (("windows10", 1), ("windows11", 2)):
        ref = _st(oc, name)
        words = _u32s(ref["COLS_LANES"])
        for w in range(nwin):
            part = words[1024 * w : 1024 * (w + 1)]
            assert sorted(x & 0x3FFFFFF for x in part) == list(range(1024 * w, 1024 * (w + 1)))
            keys = [(-(x >> 26), x & 0x3FFFFFF) for x in part]
            assert keys == sorted(keys) and len({k[0] for k in keys}) >= 3  # ties in column order
    # sharded: a dense row falls into one rank; 2^12 over 4 ranks is one window per rank
    assert [_st(oc, "longrow7", r, 2)["_stats"]["long_rows"] for r in range(2)] == [0, 2]
    assert [_st(oc, "longrow7", r, 4)["_stats"]["long_rows"] for r in range(4)] == [0, 0, 1, 1]
    assert len(_st(oc, "uniform12", 3, 4)["COLS_LANES"]) == 4 * 1024


def test_abi_declares_index_build(spx):
    header = open(os.path.join(ROOT, "include", "spartan_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in spx.EXPORTED
        assert hasattr(spx.lib(), name), name
    parts = re.findall(r"\bSPX_(IDX_[A-Z_]+)\b", header.split("spx_index_export")[0].split("enum {")[-1])
    assert parts[:-1] == spx.INDEX_PARTS and parts[-1] == "IDX_PART_COUNT"
    assert [getattr(spx, p) for p in spx.INDEX_PARTS] == list(range(spx.IDX_PART_COUNT))
    assert hasattr(spx.Context, "set_index_build") and hasattr(spx.IndexPK, "export") and hasattr(spx.IndexPK, "stats")
    L = spx.lib()
    assert L.spx_ctx_set_index_build(None, 1) != 0  # null context: a status, not a crash
    assert b"null context" in L.spx_last_error()
    assert L.spx_index_stats(None, None) != 0
