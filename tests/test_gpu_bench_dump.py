"""bench.py's plain run and --dump-outputs: the result line carries the headline figures and none of
the --full legs, and the arrays written are what the last timed step brought home -- every
document's summary, and the merged chunks and patch logs of the fixed document sample, equal to
the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = 4096    # one batch; more than the 2048 documents whose bytes are dumped, so they are sampled
SAMPLE = 2048


def test_plain_run_dumps_last_step(tmp_path):
    import oracle_ffi as O
    import workload
    from automerge_amd import patch as P

    cmd = [sys.executable, "bench.py", "--gpus", "1", "--docs", str(DOCS), "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["full"] is False and r["steps"] == 2 and r["warmup"] == 1 and r["errors"] == 0
    assert r["unit"] == "ops/s" and r["higher_is_better"] is True and r["dtype"] == "u8"
    assert r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(DOCS * 60 / (r["ms_per_step"] * 1e-3), rel=1e-9)
    for moved in ("cpu_baseline", "cpu_reference_node", "hbm_resident", "digest_pinned", "decode_GBps", "verified_docs"):
        assert moved not in r
    assert "GBps_alone" not in r["host_link"]

    assert sorted(os.listdir(tmp_path)) == ["documents.npy", "patches.npy", "summary.npy"]
    summary = np.load(tmp_path / "summary.npy")
    documents = np.load(tmp_path / "documents.npy")
    patches = np.load(tmp_path / "patches.npy")
    assert summary.dtype == np.float64 and summary.shape == (DOCS, 4)
    assert documents.dtype == np.float32 and patches.dtype == np.float32
    assert documents.shape[0] == SAMPLE and patches.shape[0] == SAMPLE
    assert summary.nbytes + documents.nbytes + patches.nbytes <= 64 << 20
    assert not summary[:, 0].any()  # every document merged in a timed step
    sample = _sample()
    assert documents.shape[1] == int(summary[sample, 1].max()) and patches.shape[1] == int(summary[sample, 2].max())

    arena, chunks, docs, _ = workload.c4(0, DOCS)
    canon = lambda x: json.dumps(x, sort_keys=True, default=lambda v: bytes(v).hex())
    for row in (0, 1, SAMPLE // 2, SAMPLE - 1):
        i = int(sample[row])
        base, changes = workload.doc_chunks(arena, chunks, docs, i)
        ref = O.Doc.load(base)
        want = ref.apply_patch(changes)
        saved = ref.save()
        n, m = int(summary[i, 1]), int(summary[i, 2])
        assert n == len(saved) and int(summary[i, 3]) == int.from_bytes(saved[4:8], "little")
        assert bytes(documents[row, :n].astype(np.uint8)) == saved
        assert (documents[row, n:] == -1).all() and (patches[row, m:] == -1).all()
        log = bytes(patches[row, :m].astype(np.uint8))
        pat = P.materialize(log, want["deps"], want["pendingChanges"], want["maxOp"])
        assert canon(pat) == canon(want)


def _sample():
    """The documents whose bytes bench.py dumps (dump_outputs: seed 0, sorted)."""
    return np.sort(np.random.default_rng(0).choice(DOCS, SAMPLE, replace=False))
