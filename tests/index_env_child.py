"""Child process of test_gpu_index_build.py: a fresh process under SPX_INDEX_BUILD, whose contexts take the
process default. Prints one JSON line {default, host, default_again}: the builder (spx_index_stats[0]) of an
index built without any call, after set_index_build(0), and after set_index_build(-1)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_product  # noqa: E402


def main():
    spx = load_product()
    ctx = spx.Context(0)
    rows = [[[(3 + x + m, (x + m) % 4)] for x in range(4)] for m in range(3)]

    def builder():
        return spx.MLArgumentForR1CS.index(ctx, *[spx.Csr.from_rows(r) for r in rows]).stats()[0]

    out = {"default": builder()}
    ctx.set_index_build(0)
    out["host"] = builder()
    ctx.set_index_build(-1)
    out["default_again"] = builder()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
