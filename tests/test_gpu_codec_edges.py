"""The edge-shaped histories of tests/codec_edges.py through every decode and encode path of the
engine, byte for byte against the CPU oracle:

  fast   the default staging: k_doc_fast (Dec32 / enc32, am_doc_fast.h) where a document is eligible
  lane   AM_FAST=0, AM_DEC_LONG past every length: k_doc with the lane decoder (ColDec) and
         encode_column
  wave   AM_FAST=0, AM_DEC_LONG=1: k_doc with the wave decoder (decode_stream_wave)

as whole histories, as a reload (the first half saved by the oracle with its columns DEFLATEd, the
rest applied on top), with both kinds of patch, and back out of the saved document as the original
changes (k_history's REnc against the host encodeChange)."""
import math
import os

import pytest

import codec_edges as E
import oracle_ffi as O

pytestmark = pytest.mark.gpu

CASES = E.cases()
LANES_ONLY = 1 << 30
PATHS = {"fast": {}, "lane": {"AM_FAST": "0", "AM_DEC_LONG": str(LANES_ONLY)}, "wave": {"AM_FAST": "0", "AM_DEC_LONG": "1"}}
FIELDS = ("status", "err_change", "arg0", "arg1", "napplied", "nqueued", "nheads", "nops", "nchanges", "max_op", "out_len")

# Patches the engine may legitimately report as unsupported (AM_U_INC_VALUE): only float or other
# non-integer counter increments could be listed, and the cases hold none.
PATCH_UNSUPPORTED = {}

# The fast-envelope table: the cases k_doc_fast must merge itself; it must leave every other case
# to k_doc. Derived by reading fast_eligible, fast_layout and the Dec32 rules (am_doc_fast.h), as
# tests/codec_edges.py explains case by case, never by running.
MUST_TAKE = {
    "value/int/0", "value/int/1", "value/int/2", "value/int/3", "value/uint/0", "value/uint/1", "value/counter/0",
    "value/counter/1", "value/counter/2", "value/counter/3", "value/timestamp/0", "value/timestamp/1",
    "value/timestamp/2", "value/timestamp/3", "value/counter-sums", "value/counter-inc-null-false-true",
    "value/scalars", "value/strings-short", "opid/2p7", "opid/2p14", "opid/2p21", "opid/2p28", "opid/2p31-below",
    "time/neg", "time/neg-2p31", "time/2p53", "time/neg-2p53", "time/2p32", "run/append/1", "run/head/1",
    "run/alternate/1", "run/delete-desc/1", "run/zigzag/1", "run/append/2", "run/head/2", "run/alternate/2",
    "run/delete-desc/2", "run/zigzag/2", "run/append/3", "run/head/3", "run/alternate/3", "run/delete-desc/3",
    "run/zigzag/3", "run/append/63", "run/head/63", "run/blocks/1-1", "run/blocks/20-20", "run/blocks/30-2",
    "key/len/1", "key/len/63", "key/len/64", "key/len/65", "key/len/127", "key/len/128", "key/len/129",
    "key/len/255", "key/multibyte-below-ee", "key/common-prefix-64", "succ/1", "succ/2", "limit/rows/64",
    "limit/preds/64", "limit/changes/64", "limit/actors/64",
}

_ref = {}


def ref(case):
    """the oracle's results for a case, computed once: whole history, and the reload at the half"""
    if case.name not in _ref:
        changes, hashes = E.encode_case(case)
        d = O.Doc.init()
        diff = d.apply_patch(changes)
        # a single change: the base is the whole document and nothing is applied on top
        half = case.half if case.half is not None else max(1, len(changes) // 2)
        h = O.Doc.init()
        h.apply(changes[:half])
        base = h.save()  # the saved form: columns of 256 bytes or more are DEFLATEd
        h2 = O.Doc.load(base)
        rdiff = h2.apply_patch(changes[half:])
        assert h2.save() == d.save()
        _ref[case.name] = {"changes": changes, "hashes": hashes, "save": d.save(), "heads": d.heads(), "diff": diff,
                           "patch": d.patch(), "half": half, "base": base, "base_heads": h.heads(),
                           "rdiff": rdiff}
    return _ref[case.name]


def run(items, path, flags=0):
    from automerge_amd.batch import Batch
    old = {k: os.environ.get(k) for k in ("AM_FAST", "AM_DEC_LONG")}
    os.environ.update(PATHS[path])
    try:
        b = Batch()
        b.stage_docs(items, flags=flags)
        b.run()
        b.sync()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return b, b.results()


def _jsonable(x):
    if isinstance(x, (bytes, bytearray)):
        return {"__bytes": bytes(x).hex()}
    if isinstance(x, dict):
        return {k: _jsonable(v) for k, v in x.items()}
    if isinstance(x, list):
        return [_jsonable(v) for v in x]
    if isinstance(x, float) and not math.isfinite(x):
        return None  # the oracle's patch is JSON text, which writes Infinity as null (JSON.stringify)
    return x


def _report(bad):
    for x in bad:
        print("MISMATCH", x)
    assert not bad, (len(bad), bad[:12])


def _check_docs(b, r, want, what):
    """want: [(name, saved bytes, heads)] per document"""
    bad = []
    for i, (name, saved, heads) in enumerate(want):
        if int(r[i]["status"]) != 0:
            bad.append((what, name, "status", int(r[i]["status"])))
            continue
        if b.doc_save(i) != saved:
            bad.append((what, name, "doc_save"))
        if b.doc_heads(i, int(r[i]["nheads"])) != heads:
            bad.append((what, name, "heads"))
    return bad


def _agree(results, names):
    bad = []
    first = results["fast"]
    for p in ("lane", "wave"):
        for i, name in enumerate(names):
            for k in FIELDS:
                if first[i][k] != results[p][i][k]:
                    bad.append((p, name, k, int(first[i][k]), int(results[p][i][k])))
    return bad


def test_three_paths_match_oracle():
    items = [(None, ref(c)["changes"]) for c in CASES]
    want = [(c.name, ref(c)["save"], ref(c)["heads"]) for c in CASES]
    results, bad = {}, []
    for p in PATHS:
        b, r = run(items, p)
        results[p] = r
        flags = b.fast_flags()
        assert p == "fast" or not flags.any()
        bad += _check_docs(b, r, want, p)
    bad += _agree(results, [c.name for c in CASES])
    _report(bad)


def test_fast_envelope_table():
    """Which cases k_doc_fast must take; each boundary pair stands on both sides."""
    names = {c.name for c in CASES}
    assert MUST_TAKE <= names
    assert {c.name for c in CASES if c.fast} == MUST_TAKE  # the generator's derivations say the same
    for lo, hi in (("limit/rows/64", "limit/rows/65"), ("limit/preds/64", "limit/preds/65"),
                   ("limit/changes/64", "limit/changes/65"), ("limit/actors/64", "limit/actors/65"),
                   ("key/len/255", "key/len/256"), ("opid/2p31-below", "opid/2p31"), ("run/append/63", "run/append/64"),
                   ("key/multibyte-below-ee", "key/multibyte-from-ee"), ("value/strings-short", "value/strings-long"),
                   ("succ/2", "succ/63")):
        assert lo in MUST_TAKE and hi in names - MUST_TAKE, (lo, hi)
    b, r = run([(None, ref(c)["changes"]) for c in CASES], "fast")
    flags = b.fast_flags()
    wrong = [(c.name, "must" if c.name in MUST_TAKE else "must not", bool(flags[i])) for i, c in enumerate(CASES)
             if bool(flags[i]) != (c.name in MUST_TAKE)]
    _report(wrong)
    print("k_doc_fast took %d of %d cases" % (int(flags.sum()), len(CASES)))


def test_aliasing_references_are_rejected():
    """A pred / elemId counter of 2^32 + an existing op's counter: the oracle refuses the change, and
    so must every path, with the same status and the full counter in the error."""
    rej = E.rejected_cases()
    items = []
    for c, ctr in rej:
        changes, _ = E.encode_case(c)
        with pytest.raises(O.OracleError, match=str(ctr)):
            O.Doc.init().apply(changes)
        items.append((None, changes))
    results, bad = {}, []
    for p in PATHS:
        b, r = run(items, p)
        results[p] = r
        for i, (c, ctr) in enumerate(rej):
            if int(r[i]["status"]) == 0 or int(r[i]["arg0"]) != ctr:
                bad.append((p, c.name, int(r[i]["status"]), int(r[i]["arg0"])))
    bad += _agree(results, [c.name for c, _ in rej])
    _report(bad)


def test_reload_three_paths():
    """Every case: the oracle-saved base (DEFLATEd columns) plus the rest of the changes, the base
    re-saved with nothing applied, and the final document re-saved with nothing applied."""
    cs = CASES
    items = [(ref(c)["base"], ref(c)["changes"][ref(c)["half"]:]) for c in cs]
    want = [(c.name, ref(c)["save"], ref(c)["heads"]) for c in cs]
    same = [(ref(c)["base"], []) for c in cs]
    want_same = [(c.name, ref(c)["base"], ref(c)["base_heads"]) for c in cs]
    full = [(ref(c)["save"], []) for c in cs]
    results, bad, ran = {}, [], 0
    for p in PATHS:
        b, r = run(items, p)
        results[p] = r
        ran += len(r)
        bad += _check_docs(b, r, want, p)
        b, r = run(same, p)
        bad += _check_docs(b, r, want_same, p + "/resave-base")
        b, r = run(full, p)
        bad += _check_docs(b, r, want, p + "/resave-final")
    assert ran == 3 * len(CASES)
    bad += _agree(results, [c.name for c in cs])
    _report(bad)


def _patches(items, path, flags, wants, materialize):
    """[materialized patch | error text] per document; a document whose patch pools overflowed is
    run again with AM_DOC_PATCH_ROOM, as the per-document API does (am_doc_apply_changes)"""
    from automerge_amd import _native as N
    from automerge_amd import patch as P
    from automerge_amd.batch import PATCH_ROOM
    out = [None] * len(items)
    todo, flg = list(range(len(items))), flags
    for _ in range(2):
        b, r = run([items[i] for i in todo], path, flg)
        again = []
        for k, i in enumerate(todo):
            if int(r[k]["status"]) != 0:
                out[i] = "status %d" % int(r[k]["status"])
                continue
            blob = b.doc_patch(k)
            if int(P.header(blob)["status"]) == P.U_CAPACITY and flg == flags:
                again.append(i)
                continue
            try:
                out[i] = _jsonable(materialize(blob, wants[i]))
            except N.AutomergeError as e:
                out[i] = "error: %s" % e
        todo, flg = again, flags | PATCH_ROOM
        if not todo:
            break
    return out


@pytest.mark.parametrize("path", ["fast", "lane"])
def test_patches(path):
    from automerge_amd import patch as P
    from automerge_amd.batch import WANT_DIFF, WANT_PATCH
    assert not PATCH_UNSUPPORTED
    bad = []

    def diff(blob, want):
        return P.materialize(blob, want["deps"], want["pendingChanges"], want["maxOp"])

    def getpatch(blob, want):
        return P.materialize(blob, want["deps"], want["pendingChanges"])

    # the applyChanges patch of the whole history, of the second half over the reloaded base, and
    # the getPatch log of the merged document
    for what, cs, items, key, flags, mat in (
            ("diff", CASES, [(None, ref(c)["changes"]) for c in CASES], "diff", WANT_DIFF, diff),
            ("reload-diff", CASES, [(ref(c)["base"], ref(c)["changes"][ref(c)["half"]:]) for c in CASES], "rdiff", WANT_DIFF, diff),
            ("getPatch", CASES, [(None, ref(c)["changes"]) for c in CASES], "patch", WANT_PATCH, getpatch)):
        wants = [ref(c)[key] for c in cs]
        got = _patches(items, path, flags, wants, mat)
        for c, g, w in zip(cs, got, wants):
            if g != w:
                bad.append((what, c.name, g if isinstance(g, str) else _first_difference(g, w)))
    _report(bad)


def _first_difference(a, b, at=""):
    if type(a) is not type(b):
        return "%s: %r != %r" % (at, a, b)
    if isinstance(a, dict):
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                return "%s/%s: only on one side" % (at, k)
            d = _first_difference(a[k], b[k], at + "/" + str(k))
            if d:
                return d
        return None
    if isinstance(a, list):
        if len(a) != len(b):
            return "%s: %d != %d entries" % (at, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            d = _first_difference(x, y, "%s[%d]" % (at, i))
            if d:
                return d
        return None
    return None if a == b else "%s: %r != %r" % (at, a, b)


def test_history_returns_the_original_changes():
    from automerge_amd import _native as N
    docs = [ref(c)["save"] for c in CASES]
    got = N.document_changes_batch(docs)
    bad = []
    for c, g in zip(CASES, got):
        if isinstance(g, Exception):
            bad.append((c.name, str(g)))
        elif [x for x, _ in g] != ref(c)["changes"] or [h for _, h in g] != ref(c)["hashes"]:
            bad.append((c.name, "changes"))
    _report(bad)
