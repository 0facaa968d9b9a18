"""A plain `bench.py --gpus 1 --steps N --warmup W` run: it times the N steps and prints the headline line
without the measurements that --full adds, and --dump-outputs writes the last timed step's proofs, which
must be the proofs the library gives for the same witnesses one at a time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_and_dump(spx, ctx, tmp_path):
    log_n, log_v, steps = 10, 5, 2
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--log-n", str(log_n), "--inflight", "4", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "R1CS constraints proved/sec at 2^%d" % log_n and d["unit"] == "constraints/s"
    assert d["higher_is_better"] is True and d["dtype"].startswith("bls12-381")
    assert d["steps"] == steps and d["full"] is False
    P = d["config"]["proofs_per_step"]
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(P * (1 << log_n) / (d["ms_per_step"] / 1e3), rel=1e-3)
    # nothing beside the headline was measured
    for k in ("value_single_proof", "value_index_cached_transcript", "roofline", "cpu_baseline", "cpu_baseline_all_cores"):
        assert d[k] is None, k
    assert "c2" not in d and "proof_sharded_rehearsal" not in d

    assert os.listdir(tmp_path / "out") == ["proofs.npy"]
    a = np.load(tmp_path / "out" / "proofs.npy")
    assert a.dtype == np.float32 and a.shape == (P, d["proof_bytes"])
    sys.path.insert(0, ROOT)
    import bench

    syn, mats, zs, nnz = bench.synth_instance(spx, 3, log_n, log_v, 0x5EED0000 + log_n, P, 0xB0B0)
    pk = spx.IndexPK(ctx, bench.index_from_c(spx, ctx, mats), log_n)
    pp = spx.MLProofForR1CS.setup(ctx, log_n, 0xC0FFEE)
    for i, z in enumerate(zs):
        w = spx.Witness(ctx, z[: 32 << log_v], z[32 << log_v:])
        assert spx.MLArgumentForR1CS.prove_witness(pk, w, pp, mode="fs", seed=7) == bytes(a[i].astype(np.uint8)), i
