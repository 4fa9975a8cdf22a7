"""Small hand-shaped change histories that put every column-codec edge through the engine: integer
sizes at the LEB128 and 2^31 / 2^32 / 2^53 boundaries, opIds that cross a varint or envelope
boundary, run / null-stretch / literal-group lengths around 64, 128 and 256 values, key and value
string lengths at 64 / 256 / 1024 bytes, succ counts and the fast kernel's 64-row limits.

Plain Python, no GPU. cases() returns [Case]; a Case is a name, a list of JSON changes in the form
backend.encodeChange takes (their `deps` are indices of earlier changes of the same case, resolved
by encode_case), and what the document must show afterwards:
  root   {key: value}  the visible value of a root key (counters: the running sum)
  lists  {key: [values]}  the visible elements of the list / text object under a root key
  half   how many changes the reload test saves as its base, where the later changes must depend
         on the base's heads only (a loaded document knows no more of its hash graph)
`fast` says whether the small-document kernel (k_doc_fast) must take the whole history as one
batch document -- derived by reading fast_eligible and the Dec32 rules (am_doc_fast.h), not by
running: FD_MAX = 64 op rows / pred-succ entries / changes / actor references, opIds and deltas
inside 31 bits, key strings of at most 255 bytes whose bytes stay below 0xEE, no value column
outside 31 bits, and a merged document that fits the kernel's output image.
"""
import math

ACT = ["%02x" % (0xa0 + i) * 16 for i in range(80)]
A, B = ACT[0], ACT[1]
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
MAX53 = 2 ** 53 - 1


class Case:
    def __init__(self, name, fast):
        self.name, self.fast = name, fast
        self.changes, self.root, self.lists = [], {}, {}
        self.half = None  # changes in the reload's base; default: half of them

    def change(self, actor=A, start=None, deps=None, time=0, seq=None, message=None):
        """opens a change; by default it follows the case's last change"""
        n = len(self.changes)
        if seq is None:
            seq = 1 + sum(1 for c in self.changes if c["actor"] == actor)
        if start is None:
            start = 1 + max([c["startOp"] + _nops(c) - 1 for c in self.changes] + [0])
        if deps is None:
            deps = [n - 1] if n else []
        ch = {"actor": actor, "seq": seq, "startOp": start, "time": time, "deps": deps, "ops": []}
        if message is not None:
            ch["message"] = message
        self.changes.append(ch)
        return Chg(ch)

    def __repr__(self):
        return "Case(%s)" % self.name


def _nops(c):
    return sum(len(o["values"]) if "values" in o else 1 for o in c["ops"])


class Chg:
    def __init__(self, ch):
        self.ch = ch

    def _id(self):
        return "%d@%s" % (self.ch["startOp"] + _nops(self.ch), self.ch["actor"])

    def op(self, **kw):
        i = self._id()
        kw.setdefault("pred", [])
        self.ch["ops"].append(kw)
        return i

    def set(self, key, value, datatype=None, pred=(), obj="_root"):
        kw = {"action": "set", "obj": obj, "key": key, "value": value, "pred": list(pred)}
        if datatype:
            kw["datatype"] = datatype
        return self.op(**kw)

    def inc(self, key, by, pred, obj="_root"):
        return self.op(action="inc", obj=obj, key=key, value=by, pred=list(pred))

    def make(self, key, kind="makeText", obj="_root"):
        return self.op(action=kind, obj=obj, key=key)

    def ins(self, obj, after, value, datatype=None):
        kw = {"action": "set", "obj": obj, "elemId": after, "insert": True, "value": value}
        if datatype:
            kw["datatype"] = datatype
        return self.op(**kw)

    def upd(self, obj, elem, value, pred):
        return self.op(action="set", obj=obj, elemId=elem, value=value, pred=list(pred))

    def rm(self, obj, elem, pred=None):
        return self.op(action="del", obj=obj, elemId=elem, pred=[elem] if pred is None else list(pred))


def _leb_edges():
    out = set()
    for k in range(1, 8):
        for b in (2 ** (7 * k - 1), 2 ** (7 * k)):
            out |= {b - 1, b, b + 1}
    return sorted(x for x in out if x <= MAX53)


INT_EDGES = sorted(set([2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, MAX53] + _leb_edges()))


def _value_cases():
    out = []
    for dt in ("int", "uint", "counter", "timestamp"):
        vals = list(INT_EDGES)
        if dt != "uint":
            vals += [-v for v in INT_EDGES] + [-2 ** 31 - 1]
        # values live in valRaw (bytes), not in a 32-bit column: inside the fast envelope. 30 ops a
        # case keep the rows within FD_MAX.
        for part, chunk in enumerate([vals[i:i + 30] for i in range(0, len(vals), 30)]):
            c = Case("value/%s/%d" % (dt, part), fast=True)
            ch = c.change()
            for i, v in enumerate(chunk):
                k = "k%03d" % i
                ch.set(k, v, None if dt == "int" else dt)
                c.root[k] = v
            out.append(c)
    # counters whose running sum crosses 2^31 and 2^32 in both directions; increments by
    # null / false / true count +0 / +0 / +1 (the reference adds them as numbers)
    c = Case("value/counter-sums", fast=True)
    ch = c.change()
    steps = {"up31": (2 ** 31 - 2, [1, 1, 5]), "down31": (2 ** 31 + 1, [-1, -1, -7]),
             "up32": (2 ** 32 - 1, [1, 2 ** 31]), "down32": (2 ** 32, [-1, -2 ** 32 - 3]),
             "neg31": (-2 ** 31 + 1, [-1, -1, 3]), "big": (MAX53 - 3, [1, 2, -MAX53])}
    ids = {}
    for k, (v0, _) in steps.items():
        ids[k] = ch.set(k, v0, "counter")
        c.root[k] = v0
    ch = c.change()
    for k, (_, incs) in steps.items():
        for by in incs:
            ch.inc(k, by, [ids[k]])
            c.root[k] += by
    out.append(c)
    c = Case("value/counter-inc-null-false-true", fast=True)
    ch = c.change()
    cid = ch.set("c", 10, "counter")
    ch = c.change()
    for by in (None, False, True, 4):
        ch.inc("c", by, [cid])
    c.root["c"] = 15
    out.append(c)
    # other scalars
    c = Case("value/scalars", fast=True)
    ch = c.change()
    sc = {"null": None, "true": True, "false": False, "negzero": -0.0, "inf": math.inf, "ninf": -math.inf,
          "subnormal": 5e-324, "subnormal2": -2.2250738585072009e-308, "f": 1.5, "pi": math.pi}
    for k, v in sc.items():
        ch.set(k, v, "float64" if isinstance(v, float) else None)
        c.root[k] = v
    out.append(c)
    # string and bytes values at the valLen varint / tag boundaries. k_doc_fast builds the merged
    # document in its cells region, the columns after 9 + 10 + 10 + actors + 10 + 32 * heads + 620
    # bytes kept for the header (about 710 here), and the region holds max(1024, 4 * (13 rows +
    # 2 entries), 446 + input bytes): once the values dominate the input the image no longer fits
    # and the document goes to k_doc (fast_layout's comment says so). Short values stay inside.
    for name, fast, sizes in (("short", True, (0, 7, 8)), ("long", False, (127, 128, 1023, 1024))):
        c = Case("value/strings-" + name, fast)
        ch = c.change()
        for n in sizes:
            s_ = "".join(chr(97 + (i * 7 + n) % 26) for i in range(n))
            b_ = bytes((i * 31 + n) & 255 for i in range(n))
            ch.set("s%d" % n, s_)
            ch.set("b%d" % n, b_)
            c.root["s%d" % n] = s_
            c.root["b%d" % n] = b_
        out.append(c)
    return out


def _opid_cases():
    """opIds that cross a boundary inside one change; preds and elemIds point below and above it"""
    out = []
    # 2^28 is the wave window's 4-to-5-byte varint; 2^31 is Dec32's envelope (ids >= 2^31 leave the
    # fast kernel); 2^32 wraps a 32-bit decoder
    for name, bound, fast in (("2p7", 2 ** 7, True), ("2p14", 2 ** 14, True), ("2p21", 2 ** 21, True),
                              ("2p28", 2 ** 28, True), ("2p31-below", 2 ** 31 - 12, True), ("2p31", 2 ** 31, False),
                              ("2p32", 2 ** 32, False), ("2p53", MAX53 - 40, False)):
        c = Case("opid/" + name, fast)
        ch = c.change()
        low = ch.set("low", 1)
        t = ch.make("t")
        e0 = ch.ins(t, "_head", "a")
        ch = c.change(start=bound - 4)  # ids bound-4 .. bound+7
        ids, el = [], e0
        for i in range(4):
            ids.append(ch.set("k%d" % i, i))
        el1 = ch.ins(t, el, "b")            # bound
        el2 = ch.ins(t, el1, "c")           # bound+1
        ids.append(ch.set("k4", 4))
        ch.set("low", 2, pred=[low])         # pred far below
        ch.set("k0", 10, pred=[ids[0]])      # pred just below the boundary
        ch.set("k4", 14, pred=[ids[4]])      # pred above it
        ch.ins(t, el2, "d")                  # elemId above
        ch.ins(t, e0, "e")                   # elemId far below
        ch = c.change()
        ch.upd(t, el1, "B", [el1])
        ch.rm(t, el2)
        c.root.update({"low": 2, "k0": 10, "k1": 1, "k2": 2, "k3": 3, "k4": 14})
        c.lists["t"] = ["a", "e", "B", "d"]
        out.append(c)
    # seq of a few thousand: empty changes of one actor, one op at the end
    c = Case("seq/2100", fast=False)  # 2100 changes > FD_MAX
    for i in range(2099):
        c.change(time=i)
    c.change().set("x", 1)
    c.root["x"] = 1
    out.append(c)
    for name, t in (("neg", -1), ("neg-2p31", -2 ** 31 - 1), ("2p53", MAX53), ("neg-2p53", -MAX53), ("2p32", 2 ** 32)):
        c = Case("time/" + name, fast=True)  # times are change-header / 64-bit column values
        c.change(time=t).set("x", 1)
        c.change(time=0).set("y", 2)
        c.change(time=-t).set("z", 3)
        c.root.update({"x": 1, "y": 2, "z": 3})
        out.append(c)
    return out


def _run_cases():
    out = []
    for n in SIZES:
        # N sequential appends (+ makeText): n + 1 rows
        c = Case("run/append/%d" % n, fast=n + 1 <= 64)
        ch = c.change()
        t = ch.make("t")
        el, vals = "_head", []
        for i in range(n):
            v = chr(0x61 + i % 26)
            el = ch.ins(t, el, v)
            vals.append(v)
        c.lists["t"] = vals
        out.append(c)
        # N inserts at _head
        c = Case("run/head/%d" % n, fast=n + 1 <= 64)
        ch = c.change()
        t = ch.make("t")
        vals = []
        for i in range(n):
            v = chr(0x41 + i % 26)
            ch.ins(t, "_head", v)
            vals.insert(0, v)
        c.lists["t"] = vals
        out.append(c)
        # strictly alternating insert / update: boolean runs all of length 1
        c = Case("run/alternate/%d" % n, fast=2 * n + 1 <= 64)
        ch = c.change()
        t = ch.make("t", "makeList")
        el, vals = "_head", []
        for i in range(n):
            el = ch.ins(t, el, i)
            ch.upd(t, el, i + 1000, [el])
            vals.append(i + 1000)
        c.lists["t"] = vals
        out.append(c)
        # N appends, then N deletes in descending elemId order (negative deltas)
        c = Case("run/delete-desc/%d" % n, fast=2 * n + 1 <= 64)  # the del ops are rows of their change
        ch = c.change()
        t = ch.make("t")
        el, els = "_head", []
        for i in range(n):
            el = ch.ins(t, el, "x")
            els.append(el)
        ch = c.change()
        for el in reversed(els):
            ch.rm(t, el)
        c.lists["t"] = []
        out.append(c)
        # deltas that alternate in sign and size: updates that hop between the ends of the list
        c = Case("run/zigzag/%d" % n, fast=2 * n + 1 <= 64)
        ch = c.change()
        t = ch.make("t", "makeList")
        el, els = "_head", []
        for i in range(n):
            el = ch.ins(t, el, i)
            els.append(el)
        ch = c.change()
        order = []
        lo, hi = 0, n - 1
        while lo <= hi:
            order.append(lo)
            if hi != lo:
                order.append(hi)
            lo, hi = lo + 1, hi - 1
        vals = list(range(n))
        for j, i in enumerate(order):
            ch.upd(t, els[i], -j, [els[i]])
            vals[i] = -j
        c.lists["t"] = vals
        out.append(c)
    # blocks of k map ops, m list ops, k map ops: keyStr, keyCtr / keyActor and obj carry null runs
    for k, m in ((1, 1), (2, 63), (3, 64), (63, 2), (64, 65), (65, 1), (127, 129), (128, 128), (129, 3), (255, 2),
                 (2, 255), (256, 1), (1, 256), (257, 3), (3, 257), (20, 20), (30, 2)):
        c = Case("run/blocks/%d-%d" % (k, m), fast=2 * k + m + 1 <= 64)
        ch = c.change()
        t = ch.make("t")
        for i in range(k):
            ch.set("a%03d" % i, i)
            c.root["a%03d" % i] = i
        el, vals = "_head", []
        for i in range(m):
            el = ch.ins(t, el, "z")
            vals.append("z")
        for i in range(k):
            ch.set("b%03d" % i, -i)
            c.root["b%03d" % i] = -i
        c.lists["t"] = vals
        out.append(c)
    # a literal run of more than 64 distinct 1-byte varints: 70 actors set one root key each, so the
    # document's idActor column (uint) is the literal run 0..69
    c = Case("run/literal/1byte", fast=False)  # 70 rows, changes and actors > FD_MAX
    for i in range(70):
        c.change(ACT[i]).set("k%02d" % i, i)
        c.root["k%02d" % i] = i
    out.append(c)
    # ... of distinct 2-byte and of distinct 4-byte varints: every list element is updated by a change
    # at an opId stride of its own, so the document's idCtr column (delta; insert and update rows
    # alternate) is a literal run of 140 distinct deltas, +d_i then -(d_i - 1), with d_i in
    # 140..7316 (2-byte signed varints) and in 2^21..2^21 + 1.2M (4-byte ones)
    for name, base, step in (("2byte", 2 ** 7, 70), ("4byte", 2 ** 21, 2 ** 14 + 3)):
        n = 70
        c = Case("run/literal/" + name, fast=False)  # 2n + 1 rows > FD_MAX
        ch = c.change()
        t = ch.make("t", "makeList")
        els = []
        ch = c.change(start=base + 1)
        el = "_head"
        for i in range(n):
            el = ch.ins(t, el, i)
            els.append(el)
        vals = list(range(n))
        prev_start = base + 1 + n
        for i in range(n):
            prev_start += step + i
            ch = c.change(start=prev_start)
            ch.upd(t, els[i], i + 500, [els[i]])
            vals[i] = i + 500
        c.lists["t"] = vals
        out.append(c)
    return out


def _string_cases():
    out = []
    for n in (1, 63, 64, 65, 127, 128, 129, 255, 256):
        c = Case("key/len/%d" % n, fast=n <= 255)  # d32_raw takes strings of at most 255 bytes
        ch = c.change()
        k = "k" * n
        a = ch.set(k, 1)
        ch = c.change()
        ch.set(k, 2, pred=[a])  # consecutive equal keys across changes
        ch.set(k[:-1] + "l", 3)
        c.root[k] = 2
        c.root[k[:-1] + "l"] = 3
        out.append(c)
    # k_doc_fast ranks keys bytewise, which is UTF-16 order only while every byte is below 0xEE
    # (U+E000 and up, and the supplementary planes, reorder): such keys leave it
    for name, fast, keys in (("below-ee", True, ["é", "ß" * 32, "€", "€" * 21 + "a", "a€é", "\ud7ff", "\ud7ff" * 9]),
                             ("from-ee", False, ["\ue000", "😀", "😀" * 16, "a😀é€", "\uffff", "\uffff😀", "😀\uffff"])):
        c = Case("key/multibyte-" + name, fast)
        ch = c.change()
        for i, k in enumerate(keys):
            ch.set(k, i)
            c.root[k] = i
        out.append(c)
    # UTF-16 order (the reference's key sort) differs from UTF-8 byte order for these two
    c = Case("key/utf16-order", fast=False)
    c.change(A).set("￿", 1)
    smile = c.change(B).set("😀", 2)
    c.change(A).set("😀", 3, pred=[smile])
    c.root.update({"￿": 1, "😀": 3})
    out.append(c)
    # keys equal through byte 64 and different after it (and at it)
    c = Case("key/common-prefix-64", fast=True)
    ch = c.change()
    p = "p" * 64
    keys = [p, p + "a", p + "b", p + "ba", p + "bb", "p" * 63 + "q", p * 2 + "a", p * 2 + "b"]
    ids = {}
    for i, k in enumerate(keys):
        ids[k] = ch.set(k, i)
    ch = c.change()
    for i, k in enumerate(keys):
        ch.set(k, 100 + i, pred=[ids[k]])
        c.root[k] = 100 + i
    out.append(c)
    return out


def _succ_cases():
    out = []
    for k in (1, 2, 63, 64, 65):
        # k actors overwrite one key concurrently, one more change resolves them: succNum = k.
        # k + 2 changes, actors and rows; 2k pred entries
        c = Case("succ/%d" % k, fast=2 * k <= 64)  # 2k pred entries
        c.half = 1
        first = c.change(A).set("x", 0)
        ids = []
        for i in range(k):
            ids.append(c.change(ACT[2 + i], start=2, deps=[0]).set("x", i + 1, pred=[first]))
        ch = c.change(B, start=3, deps=list(range(1, k + 1)))
        ch.set("x", "done", pred=ids)
        c.root["x"] = "done"
        out.append(c)
    for n in (64, 65):
        # op rows
        c = Case("limit/rows/%d" % n, fast=n <= 64)
        ch = c.change()
        for i in range(n):
            ch.set("r%02d" % i, i)
            c.root["r%02d" % i] = i
        out.append(c)
        # pred / succ entries with few rows, one actor and no further dependencies: one op, 32
        # ops that each name it as their pred (32 entries), one op that names those 32 (32 more):
        # 64 entries over 34 rows; a further overwrite makes 65
        c = Case("limit/preds/%d" % n, fast=n <= 64)
        ch = c.change()
        first = ch.set("x", 0)
        ids = [ch.set("x", i + 1, pred=[first]) for i in range(32)]
        last = ch.set("x", "done", pred=ids)
        c.root["x"] = "done"
        if n == 65:
            c.change().set("x", "again", pred=[last])
            c.root["x"] = "again"
        out.append(c)
        # changes (one actor)
        c = Case("limit/changes/%d" % n, fast=n <= 64)
        for i in range(n):
            c.change().set("c", i)
        c.root["c"] = n - 1  # no preds: all n values conflict, the last opId wins the key
        out.append(c)
        # actors
        c = Case("limit/actors/%d" % n, fast=n <= 64)
        c.change(ACT[0]).set("a00", 0)
        c.root["a00"] = 0
        for i in range(1, n):
            c.change(ACT[i], start=i + 1, deps=[i - 1]).set("a%02d" % i, i)
            c.root["a%02d" % i] = i
        out.append(c)
    return out


def rejected_cases():
    """Histories every path must refuse with the reference's error: a pred or an elemId whose counter
    is 2^32 plus the counter of an op that exists. A decoder that keeps only 32 bits of the delta
    would find that op and accept the change. -> [(Case, the counter the error names)]"""
    out = []
    for kind in ("pred", "elemId"):
        c = Case("rejected/%s-2p32-alias" % kind, fast=False)
        ch = c.change()
        x = ch.set("x", 1)
        t = ch.make("t")
        e = ch.ins(t, "_head", "a")
        ch = c.change()
        ch.set("y", 2)
        big = lambda opid: "%d@%s" % (2 ** 32 + int(opid.split("@")[0]), A)
        if kind == "pred":
            ch.set("x", 3, pred=[big(x)])
            out.append((c, 2 ** 32 + 1))
        else:
            ch.ins(t, big(e), "b")
            out.append((c, 2 ** 32 + 3))
    return out


def cases():
    out = _value_cases() + _opid_cases() + _run_cases() + _string_cases() + _succ_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


# ---- helpers of the tests (need the built library / oracle; the generator above does not) ----
_encoded = {}


def encode_case(case):
    """the case's binary changes (backend.encodeChange), deps resolved to hashes in order"""
    if case.name not in _encoded:
        import oracle_ffi as O
        from automerge_amd import backend as B
        out, hashes = [], []
        for ch in case.changes:
            js = dict(ch, deps=sorted(hashes[i] for i in ch["deps"]))
            b = B.encodeChange(js)
            out.append(b)
            hashes.append(O.change_meta(b)["hash"])
        _encoded[case.name] = (out, hashes)
    return _encoded[case.name]
