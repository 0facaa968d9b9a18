"""Child process of test_gpu_verify_strict.py: a fresh process under SPX_SUBGROUP_CHECK, whose contexts take
the process default. argv[1]: a JSON file {log_n, log_v, seed, v, vp, proof (hex)}; prints one JSON line
{default: verdict, off: verdict, on: verdict} with verdict = [exception class name or "ok", message]."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import ensure_oracle_lib, load_product  # noqa: E402


def main():
    job = json.load(open(sys.argv[1]))
    ensure_oracle_lib()
    import oracle_c as oc

    spx = load_product()
    ctx = spx.Context(0)
    inst = oc.Instance(0, job["log_n"], job["log_v"], job["seed"])
    pk = spx.MLArgumentForR1CS.index(ctx, *[spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in inst.mats])
    v, vp, proof = (bytes.fromhex(job[k]) for k in ("v", "vp", "proof"))

    def verdict():
        try:
            spx.MLArgumentForR1CS.verify(pk, v, proof, vp)
            return ["ok", ""]
        except spx.SpartanError as e:
            return [type(e).__name__, str(e)]

    out = {"default": verdict()}
    ctx.set_subgroup_check(0)
    out["off"] = verdict()
    ctx.set_subgroup_check(1)
    out["on"] = verdict()
    ctx.set_subgroup_check(-1)
    out["default_again"] = verdict()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
