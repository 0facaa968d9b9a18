"""bench.py --dump-outputs (host logic, no GPU): the last step's proofs as one float32 array, one byte
value per element, and a fixed seeded sample of the rows beyond the size limit."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _proofs(k, size):
    return [bytes((7 * i + j) & 0xFF for j in range(size)) for i in range(k)]


def test_dump_is_the_proof_bytes(bench, tmp_path):
    proofs = _proofs(5, 37)
    out = tmp_path / "dump" / "nested"  # created on demand
    bench.dump_outputs(str(out), proofs)
    assert os.listdir(out) == ["proofs.npy"]
    a = np.load(out / "proofs.npy")
    assert a.dtype == np.float32 and a.shape == (5, 37)
    assert [bytes(r.astype(np.uint8)) for r in a] == proofs


def test_dump_samples_rows_beyond_the_limit(bench, tmp_path, monkeypatch):
    proofs = _proofs(40, 16)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * 16 * 4)  # room for 10 rows
    bench.dump_outputs(str(tmp_path / "a"), proofs)
    bench.dump_outputs(str(tmp_path / "b"), proofs)
    a, b = np.load(tmp_path / "a" / "proofs.npy"), np.load(tmp_path / "b" / "proofs.npy")
    assert a.shape == (10, 16) and a.nbytes <= bench.DUMP_MAX_BYTES
    assert (a == b).all()  # the same rows every time
    rows = [proofs.index(bytes(r.astype(np.uint8))) for r in a]
    assert rows == sorted(set(rows))  # distinct proofs of the step, in their order


def test_dump_refuses_proofs_of_different_lengths(bench, tmp_path):
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path), [b"\x00" * 8, b"\x00" * 9])
