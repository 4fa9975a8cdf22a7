"""The lane column decoder (ColDec, am_dev_util.h) and the LEB128 readers on the device, called
directly (amx_coldec_selftest / amx_leb_selftest, am_kernels.hip) rather than through documents:

* every rle / delta / bool vector of tests/golden/codecs.json (recorded from the reference);
* its decode_errors vectors: values before the error, and the error's text in the engine's table;
* its leb_decode vectors for the readers the device has (53- and 64-bit; lane and line readers);
* seeded generated streams at LEB, run-length and string-length edges, encoded by the oracle's
  col_encode (tests/test_oracle.py pins it to the reference), so the expected values are the list
  that was encoded.
"""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu

DT = {"uint": 0, "int": 1, "utf8": 2, "delta": 3, "bool": 4}
AM_NULL64 = -(2 ** 63)
AM_NOSTR = 0xFFFFFFFF
MAX53 = 2 ** 53 - 1


def _lib():
    from automerge_amd import _native
    return _native.lib


def _pack(streams):
    offs = np.zeros(len(streams) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in streams], dtype=np.uint64)
    data = np.frombuffer(b"".join(streams) + b"\0", dtype=np.uint8).copy()
    return data, offs


def status_text(code):
    f = _lib().amx_status_message
    f.argtypes = [C.c_uint32, C.c_char_p, C.c_size_t]
    f.restype = C.c_size_t
    buf = C.create_string_buffer(256)
    f(code, buf, 256)
    return buf.value.decode()


def decode_streams(items, maxn):
    """items: [(type name, bytes)] -> [(status, values)]; strings come back as bytes (None = null)"""
    f = _lib().amx_coldec_selftest
    f.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
    f.restype = C.c_int
    n = len(items)
    data, offs = _pack([b for _, b in items])
    types = np.array([DT[t] for t, _ in items], dtype=np.uint8)
    status = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    count = np.zeros(n, dtype=np.uint32)
    vals = np.zeros((n, maxn), dtype=np.int64)
    lens = np.zeros((n, maxn), dtype=np.uint32)
    rc = f(data.ctypes.data, len(data) - 1, offs.ctypes.data, types.ctypes.data, n, maxn, status.ctypes.data,
           count.ctypes.data, vals.ctypes.data, lens.ctypes.data)
    assert rc == 0
    out = []
    for i, (t, b) in enumerate(items):
        k = int(count[i])
        assert k <= maxn
        v = vals[i, :k].tolist()
        if t == "bool":
            got = [bool(x) for x in v]
            assert all(x in (0, 1) for x in v)
        elif t == "utf8":
            ln = lens[i, :k].tolist()
            got = [None if l == AM_NOSTR else b[o:o + l] for o, l in zip(v, ln)]
            assert all(l == AM_NOSTR or o + l <= len(b) for o, l in zip(v, ln))
        else:
            got = [None if x == AM_NULL64 else x for x in v]
        out.append((int(status[i]), got))
    return out


def _expect(t, values):
    if t in ("uint", "int", "utf8", "delta") and all(x is None for x in values):
        return []  # an all-null column encodes to nothing (encoding.js:780)
    if t == "utf8":
        return [None if x is None else x.encode("utf-8", "surrogatepass") for x in values]
    return list(values)


def test_recorded_column_vectors(codecs):
    items, exp, ran = [], [], {}
    for kind in ("rle", "delta", "bool"):
        for v in codecs[kind]:
            t = v.get("type", kind)
            items.append((t, bytes.fromhex(v["bytes"])))
            exp.append(_expect(t, v["values"]))
        ran[kind] = len(codecs[kind])
    got = decode_streams(items, max(len(e) for e in exp) + 1)
    bad = [(i, items[i][0], items[i][1].hex(), g) for i, (g, e) in enumerate(zip(got, exp)) if g != (0, e)]
    assert not bad, bad[:5]
    assert ran == {k: len(codecs[k]) for k in ("rle", "delta", "bool")}
    print("recorded column vectors run:", ran)


def test_recorded_decode_errors(codecs):
    vs = codecs["decode_errors"]
    got = decode_streams([(v["type"], bytes.fromhex(v["bytes"])) for v in vs], 64)
    bad = []
    for v, (st, vals) in zip(vs, got):
        err = status_text(st) if st else None
        exp = v["values"]  # as decoded: no all-null rule here
        if v["type"] == "utf8":
            exp = [None if x is None else x.encode() for x in exp]
        if err != v["error"] or vals != exp:
            bad.append((v, st, err, vals))
    assert not bad, bad[:5]
    print("recorded decode_errors vectors run: %d" % len(vs))


# reference reader -> the device readers that restate it (fn codes of k_leb_selftest)
LEB_FNS = {"readUint53": (0, 6), "readInt53": (1, 7), "readUint64": (2, 4), "readInt64": (3, 5)}
LEB_NO_DEVICE_READER = ("readUint32", "readInt32")


def test_recorded_leb_vectors(codecs):
    f = _lib().amx_leb_selftest
    f.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
    f.restype = C.c_int
    cases, ran = [], {}
    for v in codecs["leb_decode"]:
        if v["fn"] in LEB_NO_DEVICE_READER:
            continue
        ran[v["fn"]] = ran.get(v["fn"], 0) + 1
        for fn in LEB_FNS[v["fn"]]:
            cases.append((fn, v))
    n = len(cases)
    data, offs = _pack([bytes.fromhex(v["bytes"]) for _, v in cases])
    fns = np.array([fn for fn, _ in cases], dtype=np.uint8)
    status, end, hi, lo = (np.full(n, 0xFFFFFFFF, dtype=np.uint32) for _ in range(4))
    assert f(data.ctypes.data, len(data) - 1, offs.ctypes.data, fns.ctypes.data, n, status.ctypes.data, end.ctypes.data,
             hi.ctypes.data, lo.ctypes.data) == 0
    bad = []
    for i, (fn, v) in enumerate(cases):
        st = int(status[i])
        err = status_text(st) if st else None
        h, l = int(hi[i]), int(lo[i])
        sh = h - 2 ** 32 if h >= 2 ** 31 else h
        if v["fn"].endswith("53"):
            val = sh * 2 ** 32 + l
        elif v["fn"] == "readInt64":
            val = [sh, l]
        else:
            val = [h, l]
        if err != v["error"] or int(end[i]) != v["offset"] or (err is None and val != v["value"]):
            bad.append((fn, v, err, int(end[i]), val))
    assert not bad, bad[:5]
    want = {}
    for v in codecs["leb_decode"]:
        want[v["fn"]] = want.get(v["fn"], 0) + 1
    for fn in LEB_FNS:
        assert ran[fn] == want[fn] > 0, fn
    assert sum(ran.values()) == len(codecs["leb_decode"]) - sum(want[f_] for f_ in LEB_NO_DEVICE_READER)
    print("recorded leb_decode vectors run:", ran, "no device reader:", {k: want[k] for k in LEB_NO_DEVICE_READER})


# ---- generated streams ----
RUNS = (2, 3, 63, 64, 65, 127, 128, 129)
NULL_RUNS = (1, 2, 63, 64, 65)
STR_LENS = (0, 1, 63, 64, 65, 127, 128, 300)
BOOL_RUNS = (1, 63, 64, 128, 2, 3, 65)
MAXV = 300


def _int_pool(signed):
    p = {0, 1, MAX53, MAX53 - 1}
    for k in range(1, 9):
        for d in (-1, 0, 1):
            b = 2 ** (7 * k - 1) + d  # the signed LEB128 length boundary
            u = 2 ** (7 * k) + d      # the unsigned one
            for x in (b, u) if not signed else (b, -b, u, -u):
                if abs(x) <= MAX53:
                    p.add(x)
    if signed:
        p |= {-1, -MAX53, -MAX53 + 1}
    return sorted(p)


def _distinct(rng, pool, k):
    """k values from pool with no two neighbours equal (a literal run)"""
    out = []
    while len(out) < k:
        x = rng.choice(pool)
        if not out or out[-1] != x:
            out.append(x)
    return out


def _str_pool(rng):
    base = "".join(rng.choice("abcdefghij") for _ in range(64))
    pool = ["", "a", "é", "€", "😀"]
    for n in STR_LENS:
        pool.append("".join(rng.choice("klmnopqrst") for _ in range(n)))
    # agree on the first 64 bytes; differ at byte 64, or at byte 65
    pool += [base + "a", base + "b", base + "ca", base + "cb", base]
    return pool


def _rle_values(rng, pool, budget=None):
    vals = []
    cost = 0
    while len(vals) < MAXV and rng.random() < (0.9 if vals else 1.0):
        kind = rng.choice("nrl")
        if kind == "n":
            seg = [None] * rng.choice(NULL_RUNS)
        elif kind == "r":
            seg = [rng.choice(pool)] * rng.choice(RUNS)
        else:
            seg = _distinct(rng, pool, rng.choice(RUNS))
        if budget is not None:
            keep = []
            for s in seg:
                cost += len(s) if s else 0
                if cost > budget:
                    break
                keep.append(s)
            seg = keep
        vals += seg
    return vals[:MAXV]


def _delta_values(rng, pool):
    vals, cur = [], 0
    for d in _rle_values(rng, pool):
        if d is None:
            vals.append(None)
            continue
        if abs(cur + d) > MAX53:
            d = -d
        if abs(cur + d) > MAX53:
            d = -cur  # back to zero: |cur| <= MAX53 is itself a valid delta
        cur += d
        vals.append(cur)
    return vals


def _bool_values(rng):
    vals, cur = [], rng.random() < 0.5  # True first: a zero-length first run
    while len(vals) < MAXV and rng.random() < (0.9 if vals else 1.0):
        vals += [cur] * rng.choice(BOOL_RUNS)
        cur = not cur
    return vals[:MAXV]


def _generated(seed=20240611, per_type=520):
    rng = random.Random(seed)
    upool, ipool = _int_pool(False), _int_pool(True)
    out = []
    for _ in range(per_type):
        out.append(("uint", _rle_values(rng, upool)))
        out.append(("int", _rle_values(rng, ipool)))
        out.append(("utf8", _rle_values(rng, _str_pool(rng), budget=12000)))
        out.append(("delta", _delta_values(rng, ipool)))
        out.append(("bool", _bool_values(rng)))
    # every edge at least once, on its own
    for n in RUNS:
        out.append(("uint", [2 ** 28] * n))
        out.append(("int", list(range(-n, 0))))
        out.append(("delta", [2 ** 31 - n + i * i for i in range(n)]))
        out.append(("utf8", ["k%d" % i for i in range(n)]))
    for n in NULL_RUNS:
        out.append(("uint", [7] + [None] * n + [7]))
        out.append(("utf8", [None] * n + ["x"]))
        out.append(("delta", [1] + [None] * n + [2, None]))
    for n in BOOL_RUNS:
        out.append(("bool", [True] * n + [False] * n + [True]))
    for x in upool:
        out.append(("uint", [x]))
    for x in ipool:
        out.append(("int", [x, x]))
        out.append(("delta", [x]))
    return out


def test_generated_streams():
    gen = _generated()
    per = {}
    for t, v in gen:
        assert len(v) <= MAXV
        per[t] = per.get(t, 0) + 1
    assert all(per[t] >= 500 for t in DT), per
    items = [(t, O.col_encode(t, v)) for t, v in gen]
    got = decode_streams(items, MAXV + 1)  # one launch; one value of room shows a decoder that overruns
    bad = [(i, t, v[:8], got[i][0], got[i][1][:8]) for i, (t, v) in enumerate(gen) if got[i] != (0, _expect(t, v))]
    assert not bad, (len(bad), bad[:3])
    print("generated streams decoded:", per)
