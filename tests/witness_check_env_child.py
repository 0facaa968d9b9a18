"""Child process of test_gpu_witness_check.py: a fresh process under SPX_WITNESS_CHECK, whose contexts take
the process default. Proves one violated witness (kind 0 at 2^6, 1 added to C's coefficient in row 5,
commitment stubbed) on a context per setting and prints one JSON line {default, off, on, default_again:
["ok" | "WrongWitness", witness_check_stats]}."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import ensure_oracle_lib, load_product  # noqa: E402

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def main():
    ensure_oracle_lib()
    import oracle_c as oc

    spx = load_product()
    inst = oc.Instance(0, 6, 3, 0x5EED0006, 0)
    rows = inst.mats[2].to_rows()
    coeff, col = rows[5][0]
    rows[5][0] = ((coeff + 1) % R, col)
    mats = [inst.mats[0], inst.mats[1], oc.CsrMatrix.from_rows(rows)]
    out = {}
    for name, mode in (("default", None), ("off", 0), ("on", 1), ("default_again", -1)):
        c = spx.Context(0)
        if mode is not None:
            c.set_witness_check(mode)
        pk = spx.MLArgumentForR1CS.index(c, *[spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in mats])
        try:
            spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, None, commitment_stub=True)
            verdict = "ok"
        except spx.WrongWitness:
            verdict = "WrongWitness"
        out[name] = [verdict, list(c.witness_check_stats())]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
