"""The edge-shaped histories of tests/codec_edges.py on the host only: the generator, the library's
encodeChange (am_change_enc.h, host code) and the CPU oracle checked against each other before a
GPU is involved. Every case must pass: a case the oracle rejects is a generator bug or a finding."""
import math
import struct
import zlib

import pytest

import codec_edges as E
import oracle_ffi as O
from docfmt import uleb

CASES = E.cases()


def _shown(v):
    """a written value as the patch's JSON shows it"""
    if isinstance(v, (bytes, bytearray)):
        return {"__bytes": bytes(v).hex()}
    if isinstance(v, float) and not math.isfinite(v):
        return None  # JSON has no Infinity: null, as JSON.stringify writes it
    return v


def _body(change):
    """the chunk body of a binary change, inflated if it is a compressed chunk"""
    ln, off = uleb(change, 9)
    body = change[off:off + ln]
    return zlib.decompress(body, -15) if change[8] == 2 else body


def _list_of(diff):
    out = []
    for e in diff["edits"]:
        if e["action"] == "insert":
            out.insert(e["index"], e["value"]["value"])
        elif e["action"] == "multi-insert":
            out[e["index"]:e["index"]] = e["values"]
        elif e["action"] == "update":
            out[e["index"]] = e["value"]["value"]
        else:
            assert e["action"] == "remove"
            del out[e["index"]:e["index"] + e["count"]]
    return out


def test_generator_covers_the_sizes():
    names = {c.name for c in CASES}
    for n in E.SIZES:
        for shape in ("append", "head", "alternate", "delete-desc", "zigzag"):
            assert "run/%s/%d" % (shape, n) in names
    assert 100 < len(CASES) < 400
    assert len(E.rejected_cases()) == 2
    for c in CASES:
        assert sum(E._nops(ch) for ch in c.changes) <= 800, c.name


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_encodes_and_applies(case):
    changes, hashes = E.encode_case(case)
    for js, b, h in zip(case.changes, changes, hashes):
        m = O.change_meta(b)
        assert (m["seq"], m["startOp"], m["numOps"], m["numDeps"]) == (js["seq"], js["startOp"], E._nops(js), len(js["deps"]))
    # floats keep every bit, the sign of -0.0 included (the patch's JSON cannot show it)
    bodies = b"".join(_body(b) for b in changes)
    for ch in case.changes:
        for op in ch["ops"]:
            if isinstance(op.get("value"), float) and op.get("datatype") == "float64":
                assert struct.pack("<d", op["value"]) in bodies, op
    d = O.Doc.init()
    d.apply(changes)
    assert d.pending() == 0
    props = d.patch()["diffs"].get("props", {})
    for k, v in case.root.items():
        assert k in props, k
        # the visible value of a key: the greatest opId's
        best = max(props[k], key=lambda i: (int(i.split("@")[0]), i.split("@")[1]))
        got = props[k][best]["value"]
        want = _shown(v)
        assert got == want and isinstance(got, bool) == isinstance(want, bool), (k, got, want)
    for k, vals in case.lists.items():
        (diff,) = props[k].values()
        assert _list_of(diff) == vals, k
    # the saved document loads again to the same bytes
    saved = d.save()
    assert O.Doc.load(saved).save() == saved
