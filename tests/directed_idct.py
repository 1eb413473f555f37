"""Directed IDCT batches (plain Python, no GPU): an int64 model of the reference's
inverse_dct_template<add> with every node named, named mutants of it, range bounds, a seeded
witness search and batches that place the witnesses in every kernel path.

The model's input is the QFS block after mismatch control (directed_dequant.model_qfs), in the
reference's transposed layout: F[i * 8 + j] is horizontal frequency i of coefficient row j.  Pass 1
transforms over i for the eight rows j (a kernel lane holds rows v, v + 1 as one packed pair), pass 2
over the rows for the eight columns x (a lane holds columns x, x + 2 for x in 0, 1, 4, 5), then
>> 6 and packus (put) or packus(adds(pred, res)) (add).

Legal domain, as mp2vg_batch_upload's validation (runtime.cpp plan_batch) leaves it: the upload
checks a word's tag bits, that DC / '1s' words sit at scan position 0, that the block is coded and
the words contiguous; it puts no bound on a level.  The bounds are therefore those of the dequant
arithmetic (directed_dequant.model_qfs): every AC value is clamped to [-2048, 2047]; QFS[63] takes
the mismatch toggle of its bit 0 inside that range; a non-intra QFS[0] is an AC value or the
unclamped '1s' value, |v| <= 2677 = (3 * 255 * 112) >> 5; an intra QFS[0] is the DC word's level as
it stands, any int16.

Mutants are (name, pass, node, rail) tuples; a witness applies one to a single line of its pass (a
row in pass 1, a column in pass 2 and in the output stage), so that each half of the packed pair and
each of an item's four lanes has its own witness.  A witness counts only when a final byte changes.
What the search cannot hit must be excluded by bound(): affine forms of the eight inputs with
floor-error intervals (exact while nothing upstream can saturate, plain intervals after), and
exhaustive sweeps where a term depends on one input.  The search draws its blocks from what quantiser
matrices 16 and quantiser scale 1 reach (dequant is the identity there: AC values and a non-intra
QFS[0] in [-2047, 2047], an intra QFS[0] any int16) and kills every mutant the bounds leave inside it;
the bounds are taken over the whole legal domain, -2048 and the '1s' value 2677 included.

tests/test_idct_directed_cpu.py asserts model == oracle == the reference's fixture, the kills, the
bounds and the batches' coverage; tests/test_gpu_idct.py decodes the batches."""
import os

import numpy as np

import _oracle
import directed_dequant as Q
from directed import NB, _Builder
from tiny_mp2v_dec_amd._lib import COEF_DC, COEF_FIRST1S, MB_BWD, MB_DCT_FIELD, MB_FWD, MB_INTRA

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "idct_directed.npz")
SEED = 20261


# ---------------------------------------------------------------------------------------------
# 16-bit SSE2 semantics on int64
# ---------------------------------------------------------------------------------------------
def _sat(x):
    return np.clip(x, -32768, 32767)


def _wrap(x):
    return ((x + 32768) % 65536) - 32768


def _wrap32(x):
    return ((x + 2 ** 31) % 2 ** 32) - 2 ** 31


# the pair partner of a line: pass 1 rows (v, v + 1), pass 2 / output columns (x, x + 2)
def is_high(ps, line):
    return bool(line & 1) if ps == 0 else bool(line & 2)


def partner(ps, line):
    return line ^ 1 if ps == 0 else line ^ 2


def lane_of(ps, line):
    """The item's lane (0-3) that holds the line: rows 2q, 2q + 1; columns x, x + 2 with
    x = (q & 1) | ((q & 2) << 1)."""
    return line >> 1 if ps == 0 else (line & 1) | ((line & 4) >> 1)


class _Num:
    """Numeric node operations on arrays [..., 8 lines] with one optional mutant, and a record of
    which node saturates where."""

    def __init__(self, ps, mut=None, rec=None, wrap32=False):
        self.ps, self.rec, self.wrap32 = ps, rec, wrap32
        self.mut = mut if mut is not None and mut[1] == ps else None

    def _satn(self, name, t):
        r = _sat(t)
        if self.rec is not None:
            self.rec[(self.ps, name, "+")] = t > 32767
            self.rec[(self.ps, name, "-")] = t < -32768
        m = self.mut
        if m is not None and m[0] == "wrap" and m[2] == name:
            return np.where(t > 32767 if m[3] == "+" else t < -32768, _wrap(t), r)
        return r

    def adds(self, name, a, b):
        return self._satn(name, a + b)

    def subs(self, name, a, b):
        return self._satn(name, a - b)

    def shl(self, name, a, n):
        t = a * (1 << n)
        r = _wrap(t)
        if self.rec is not None:
            self.rec[(self.ps, name, "o")] = t != r
        m = self.mut
        if m is not None and m[0] == "shlsat" and m[2] == name:
            return _sat(t)
        return r

    def mulhi(self, a, c):
        p = a * c
        if self.wrap32:
            p = _wrap32(p)
        else:
            assert np.abs(p).max(initial=0) < 2 ** 31
        m = self.mut
        if m is not None and m[0] == "mulhi_round":
            return _wrap((p + 32768) >> 16)
        r = _wrap(p >> 16)
        if m is not None and m[0] == "mulhi_borrow":  # the high half's product loses the low half's borrow
            neg = (p < 0).astype(np.int64)
            b = np.zeros_like(r)
            for h in range(8):
                if is_high(self.ps, h):
                    b[..., h] = neg[..., partner(self.ps, h)]
            return _wrap(r - b)
        return r

    def mulhi_x2(self, name, a, c):
        m = self.mut
        if m is not None and m[0] == "x2_bit0":  # high half of a * 2c with bit 0 kept
            return _wrap((a * 2 * c) >> 16)
        return self.shl(name + ".x2", self.mulhi(a, c), 1)

    # the kernel's folded forms: one mulhi of a wider constant (32-bit products)
    def fold(self, a, c):
        return self.mulhi(a, c)

    def fold_x2(self, a, c):
        p = a * 2 * c
        if self.wrap32:
            p = _wrap32(p)
        else:
            assert np.abs(p).max(initial=0) < 2 ** 31
        return _wrap((p >> 16) & ~1)


def idct_1d(s, p1=False, ops=None):
    """idct_sse2.hpp:23-65 on eight inputs; p1: the kernel's pass-1 fold form (idct_1d<true>)."""
    if ops is None:
        ops = _Num(0)
        s = [np.asarray(x, dtype=np.int64) for x in s]
    o = ops
    m = getattr(o, "mut", None)
    if m is not None and m[0] == "fold_s0":
        v15 = o.fold_x2(s[0], 27145 + 65536)
    else:
        v15 = o.adds("v15", o.mulhi_x2("v15", s[0], 27145), o.shl("v15.shl", s[0], 1))
    if p1:
        v26 = o.fold(s[1], -5037 + 262144)
        v21 = o.fold(s[2], -19954 + 262144)
        v28 = o.fold_x2(s[3], -22089 + 131072)
        v16 = o.fold_x2(s[4], 27145 + 65536)
        v25 = o.fold(s[5], 14567 + 131072)
    else:
        v26 = o.adds("v26", o.mulhi(s[1], -5037), o.shl("v26.shl", s[1], 2))
        v21 = o.adds("v21", o.mulhi(s[2], -19954), o.shl("v21.shl", s[2], 2))
        v28 = o.adds("v28", o.mulhi_x2("v28", s[3], -22089), o.shl("v28.shl", s[3], 2))
        v16 = o.adds("v16", o.mulhi_x2("v16", s[4], 27145), o.shl("v16.shl", s[4], 1))
        v25 = o.adds("v25", o.mulhi(s[5], 14567), o.shl("v25.shl", s[5], 1))
    v22 = o.adds("v22", o.mulhi_x2("v22", s[6], 17391), s[6])
    v27 = o.mulhi_x2("v27", s[7], 25570)
    v19, v20 = o.subs("v19", v25, v28), o.subs("v20", v26, v27)
    v23, v24 = o.adds("v23", v26, v27), o.adds("v24", v25, v28)
    v7, v11 = o.adds("v7", v23, v24), o.adds("v11", v21, v22)
    v13, v17 = o.subs("v13", v23, v24), o.subs("v17", v21, v22)
    v8, v9 = o.adds("v8", v15, v16), o.subs("v9", v15, v16)
    v18 = o.mulhi(o.subs("v18.sub", v19, v20), 25079)
    v12 = o.subs("v12", v18, o.fold(v19, 20090 + 65536) if p1 else o.adds("v12.op3", v19, o.mulhi(v19, 20090)))
    v14 = o.subs("v14", o.subs("v14.op1", v20, o.mulhi(v20, 30068)), v18)
    v6 = o.subs("v6", o.shl("v6.shl", v14, 1), v7)
    v5 = o.subs("v5", o.fold(v13, 27145 + 65536) if p1 else o.adds("v5.op0", v13, o.mulhi(v13, 27145)), v6)
    v4 = o.adds("v4", v5, o.shl("v4.shl", v12, 1))
    v10 = o.subs("v10", o.fold(v17, 27145 + 65536) if p1 else o.adds("v10.op0", v17, o.mulhi(v17, 27145)), v11)
    v0, v1 = o.adds("v0", v8, v11), o.adds("v1", v9, v10)
    v2, v3 = o.subs("v2", v9, v10), o.subs("v3", v8, v11)
    out = [o.adds("o0", v0, v7), o.adds("o1", v1, v6), o.adds("o2", v2, v5), o.subs("o3", v3, v4),
           o.adds("o4", v3, v4), o.subs("o5", v2, v5), o.subs("o6", v1, v6), o.subs("o7", v0, v7)]
    return out if isinstance(o, _Bound) else np.stack(out)


SAT_NODES = ("v15", "v26", "v21", "v28", "v16", "v25", "v22", "v19", "v20", "v23", "v24", "v7", "v11", "v13", "v17",
             "v8", "v9", "v18.sub", "v12.op3", "v12", "v14.op1", "v14", "v6", "v5.op0", "v5", "v4", "v10.op0", "v10",
             "v0", "v1", "v2", "v3", "o0", "o1", "o2", "o3", "o4", "o5", "o6", "o7")
SHL_NODES = ("v15.shl", "v26.shl", "v21.shl", "v28.shl", "v16.shl", "v25.shl", "v6.shl", "v4.shl",
             "v15.x2", "v28.x2", "v16.x2", "v22.x2", "v27.x2")

# mutants of the arithmetic, (kind, pass, node, rail); each is witnessed per (form, line)
ARITH = ([("wrap", ps, n, r) for ps in (0, 1) for n in SAT_NODES for r in "+-"] +
         [("shlsat", ps, n, None) for ps in (0, 1) for n in SHL_NODES] +
         [(k, ps, None, None) for k in ("mulhi_round", "x2_bit0", "mulhi_borrow") for ps in (0, 1)] +
         [("fold_p2", 1, None, None), ("fold_s0", 0, None, None)])
# ... of the output stage (pass-2 lanes: the line is a column) and of the pair's order
OUTPUT = [(k, 2, None, None) for k in ("shr_logical", "shr_round", "add_wrap", "add_carry", "cols_swapped")] + \
         [("rows_swapped", 0, None, None)]
# ... of the block's form, and of where it lands and what it leaves (whole batches only)
FORM = [("put_for_add", 2, None, None), ("add_for_put", 2, None, None)]
BATCH_MUTANTS = ("field_step_ignored", "chunk_unzeroed")
MUTANTS = ARITH + OUTPUT + FORM
MUTANT_TEXT = {
    "wrap": "adds/subs node wraps instead of saturating at the rail", "shlsat": "slli saturates instead of wrapping",
    "mulhi_round": "mulhi rounds to nearest", "x2_bit0": "slli(mulhi, 1) keeps bit 0 of the doubled product",
    "mulhi_borrow": "mulhi of the high half takes the borrow of the low half's product",
    "fold_p2": "the pass-1 fold form used in pass 2", "fold_s0": "the fold form used for s[0] in pass 1",
    "shr_logical": ">> 6 logical", "shr_round": ">> 6 with rounding",
    "add_wrap": "adds(pred, res) as a plain 16-bit add", "add_carry": "pred + res as one 32-bit add of the pair",
    "cols_swapped": "columns x / x + 2 swapped", "rows_swapped": "rows v / v + 1 swapped",
    "put_for_add": "put instead of add", "add_for_put": "add instead of put",
    "field_step_ignored": "field-DCT row step ignored", "chunk_unzeroed": "pass 2 leaves one 16-B chunk unzeroed",
}


def mutant_name(m):
    if m[0] in ("wrap", "shlsat"):
        return "p%d.%s.%s%s" % (m[1] + 1, m[0], m[2], m[3] or "")
    return "p%d.%s" % (m[1] + 1, m[0]) if m in ARITH and m[0] not in ("fold_p2", "fold_s0") else m[0]


NAMES = [mutant_name(m) for m in MUTANTS]
assert len(set(NAMES)) == len(NAMES)


def _pass(X, ps, mut, line, rec=None):
    """One pass over X[n, i, line] -> [n, out, line]; the mutant on one line (None: all)."""
    def run(m):
        fold = m is not None and m[0] == "fold_p2" and ps == 1
        ops = _Num(ps, m, rec if m is None else None, wrap32=m is not None and m[0] in ("fold_p2", "fold_s0"))
        return np.stack(idct_1d([X[:, i, :] for i in range(8)], fold, ops), 1)
    good = run(None)
    if mut is None or mut[1] != ps or mut[0] == "rows_swapped":
        return good
    bad = run(mut)
    if line is None:
        return bad
    # (the borrow mutant's critical line is the low half, its effect in the high half: the pair)
    for c in (line, partner(ps, line)) if mut[0] == "mulhi_borrow" else (line,):
        good[:, :, c] = bad[:, :, c]
    return good


def model_idct(F, pred=None, mut=None, line=None, rec=None):
    """F: int[n, 64] (QFS after mismatch control), pred: None (put) or int[n] / int[n, 64] -> uint8
    [n, 64] (row y, column x), with one optional mutant on one optional line."""
    X = np.asarray(F, np.int64).reshape(-1, 8, 8).copy()
    n = len(X)
    if mut is not None and mut[0] == "rows_swapped":
        for v in range(0, 8, 2):
            if line is None or line >> 1 == v >> 1:
                X[:, :, [v, v + 1]] = X[:, :, [v + 1, v]]
    o = _pass(X, 0, mut, line, rec)           # [n, x, v]
    r = _pass(o.transpose(0, 2, 1), 1, mut, line, rec)  # [n, y, x]
    k = mut[0] if mut is not None and mut[1] == 2 else None
    add = pred is not None
    if k == "put_for_add":
        add = False
    P = np.zeros((n, 8, 8), np.int64)
    if pred is not None:
        P[:] = np.asarray(pred, np.int64).reshape(n, -1, 1) if np.ndim(pred) < 2 else np.asarray(pred).reshape(n, 8, 8)
    if k == "add_for_put":
        add = True

    def finish(kk):
        res = r >> 6
        if kk == "shr_logical":
            res = (r & 0xFFFF) >> 6
        elif kk == "shr_round":
            res = (r + 32) >> 6
        if not add:
            out = res
        elif kk == "add_wrap":
            out = _wrap(P + res)
        else:
            out = _sat(P + res)
            if kk == "add_carry":  # the low half's unsigned carry lands in the high half
                c = ((res < 0) & (P + res >= 0)).astype(np.int64)
                for h in (2, 3, 6, 7):
                    out[:, :, h] = _wrap(out[:, :, h] + c[:, :, h - 2])
        out = np.clip(out, 0, 255)
        if kk == "cols_swapped":
            out = out[:, :, [2, 3, 0, 1, 6, 7, 4, 5]]
        return out
    out = finish(None)
    if k is not None and k not in ("put_for_add", "add_for_put"):
        bad = finish(k)
        if line is None:
            out = bad
        else:
            for c in (line, partner(1, line)) if k in ("cols_swapped", "add_carry") else (line,):
                out[:, :, c] = bad[:, :, c]
    return out.reshape(n, 64).astype(np.uint8)


def oracle_idct(F, pred=None):
    F = np.asarray(F, np.int16).reshape(-1, 64)
    if pred is not None:
        pred = np.broadcast_to(np.asarray(pred, np.uint8).reshape(len(F), -1), (len(F), 64))
    return np.stack([_oracle.idct(F[k], None if pred is None else pred[k]) for k in range(len(F))])


# ---------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------
class _Aff:
    """sum(c[i] * s[i]) + e with e in [elo, ehi]; s[i] in [lo[i], hi[i]]."""
    __slots__ = ("c", "elo", "ehi", "src")

    def __init__(self, c, elo=0.0, ehi=0.0, src=None):
        self.c, self.elo, self.ehi, self.src = np.asarray(c, float), elo, ehi, src


class _Bound:
    """The node operations on affine forms.  may[(node, rail)]: the unsaturated value can pass the
    rail; a node that can is a plain interval from there on."""

    def __init__(self, lo, hi):
        self.lo, self.hi = np.asarray(lo, float), np.asarray(hi, float)
        self.may, self.range = {}, {}

    def rng(self, a):
        lo = np.minimum(a.c * self.lo, a.c * self.hi).sum() + a.elo
        hi = np.maximum(a.c * self.lo, a.c * self.hi).sum() + a.ehi
        return int(np.ceil(lo - 1e-6)), int(np.floor(hi + 1e-6))

    def _node(self, name, t, rails):
        lo, hi = self.rng(t)
        self.range[name] = (lo, hi)
        for r in rails:
            self.may[(name, r)] = hi > 32767 if r == "+" else (lo < -32768 if r == "-" else hi > 32767 or lo < -32768)
        if hi > 32767 or lo < -32768:
            return _Aff(np.zeros(8), max(lo, -32768), min(hi, 32767))
        return t

    def _own(self, a, b, sign):
        """a +- mulhi(a, c) of a plain interval a: one variable, swept exhaustively."""
        if b.src is None or b.src[0] is not a or a.c.any():
            return None
        x = np.arange(int(a.elo), int(a.ehi) + 1, dtype=np.int64)
        t = x + sign * ((x * b.src[1]) >> 16)
        return _Aff(np.zeros(8), float(t.min()), float(t.max()))

    def adds(self, name, a, b):
        return self._node(name, self._own(a, b, 1) or _Aff(a.c + b.c, a.elo + b.elo, a.ehi + b.ehi), "+-")

    def subs(self, name, a, b):
        return self._node(name, self._own(a, b, -1) or _Aff(a.c - b.c, a.elo - b.ehi, a.ehi - b.elo), "+-")

    def shl(self, name, a, n):
        return self._node(name, _Aff(a.c * (1 << n), a.elo * (1 << n), a.ehi * (1 << n)), "o")

    def mulhi(self, a, c):
        k = c / 65536.0
        e = sorted((a.elo * k, a.ehi * k))
        return _Aff(a.c * k, e[0] - 1.0, e[1], (a, c))

    def mulhi_x2(self, name, a, c):
        return self.shl(name + ".x2", self.mulhi(a, c), 1)


_bounds = {}


def bound(ps, intra, line):
    """The _Bound of one line of a pass: pass 1 over the legal domain (row 0's s[0] is QFS[0]), pass
    2 over all int16."""
    key = (ps, intra and line == 0, line == 0) if ps == 0 else (1,)
    if key not in _bounds:
        lo, hi = [-2048.0] * 8, [2047.0] * 8
        if ps == 1:
            lo, hi = [-32768.0] * 8, [32767.0] * 8
        elif line == 0:
            lo[0], hi[0] = (-32768.0, 32767.0) if intra else (-2677.0, 2677.0)
        b = _Bound(lo, hi)
        idct_1d([_Aff(np.eye(8)[i]) for i in range(8)], False, b)
        _bounds[key] = b
    return _bounds[key]


_sweeps = {}


def sweep_unreachable(m, intra, line):
    """Exhaustive single-variable sweeps.  slli(mulhi(a, c), 1) never leaves int16 for any int16 a;
    the fold of s[0] equals the exact form wherever |s[0]| <= 8191; adds(pred, res) cannot leave
    int16 with |res| <= 512."""
    a = np.arange(-32768, 32768, dtype=np.int64)
    if m[0] == "shlsat" and m[2].endswith(".x2"):
        c = {"v15.x2": 27145, "v28.x2": -22089, "v16.x2": 27145, "v22.x2": 17391, "v27.x2": 25570}[m[2]]
        if c not in _sweeps:
            _sweeps[c] = bool((np.abs(((a * c) >> 16) * 2) <= 32767).all())
        return _sweeps[c]
    if m[0] == "fold_s0":
        if "fold" not in _sweeps:
            o = _Num(0, wrap32=True)
            exact = o.adds("v15", o.mulhi_x2("v15", a, 27145), o.shl("v15.shl", a, 1))
            _sweeps["fold"] = a[exact != o.fold_x2(a, 27145 + 65536)]
        bad = _sweeps["fold"]
        lim = 32768 if intra and line == 0 else (2677 if line == 0 else 2048)
        return not ((bad >= -lim) & (bad <= lim)).any()
    if m[0] == "add_wrap":
        return (-32768 >> 6) + 0 >= -32768 and (32767 >> 6) + 255 <= 32767
    return False


def bounded(m, intra, line):
    """True when the bound code proves that mutant m cannot change anything on this line."""
    if m[0] == "wrap":
        return not bound(m[1], intra, line).may[(m[2], m[3])]
    if m[0] == "shlsat" and not m[2].endswith(".x2"):
        return not bound(m[1], intra, line).may[(m[2], "o")]
    return sweep_unreachable(m, intra, line)


# the kernel's comment bounds on the pass-1 folds (recon.hip idct_1d)
KERNEL_BOUNDS = {"v19": 11363, "v13": 20998, "v17": 10703}


# ---------------------------------------------------------------------------------------------
# the witness search
# ---------------------------------------------------------------------------------------------
P_VALUES = (0, 128, 255)        # flat predictions of the add form
P_DC = {0: 0, 128: Q.ANCHOR_DC, 255: 2047}  # the DC of a DC-only intra block that renders them


def mismatch(Q0, intra):
    """Mismatch control on blocks [n, 64] (intra: QFS[0], the DC, outside the sum)."""
    F = np.array(Q0, np.int64)
    s = F.sum(1) - (F[:, 0] if intra else 0)
    F[s % 2 == 0, 63] ^= 1
    return F


def _pool(rng, intra, n):
    """Candidate blocks of the W = 16, quantiser scale 1 domain (dequant is the identity: AC values
    in [-2047, 2047], non-intra QFS[0] too, an intra QFS[0] any int16)."""
    edge = np.array([-2047, -2046, -1024, -1, 0, 1, 1024, 2046, 2047])

    def amp(k):  # log-uniform amplitudes in (1/64, 1]
        return np.exp(rng.uniform(np.log(1 / 64), 0, (k, 1)))
    fam = []
    b = np.zeros((n, 8, 8), np.int64)  # one coefficient row (a pass-1 line) carries the weight
    j = rng.integers(0, 8, n)
    b[np.arange(n), :, j] = np.where(rng.random((n, 8)) < 0.5, rng.choice(edge, (n, 8)), rng.integers(-2047, 2048, (n, 8)))
    b += (rng.random((n, 8, 8)) < 0.05) * rng.integers(-300, 301, (n, 8, 8))
    fam.append(np.clip(b.reshape(n, 64), -2047, 2047))
    fam.append(rng.integers(-2047, 2048, (n, 64)))
    fam.append(np.rint(rng.choice([-2047, 2047], (n, 64)) * amp(n)).astype(np.int64))
    b = np.zeros((n, 64), np.int64)
    for k in range(n):
        pos = rng.choice(64, int(rng.integers(1, 7)), replace=False)
        b[k, pos] = rng.choice(edge, len(pos))
    fam.append(b)
    # separable blocks: pass 2 sees one profile scaled per column, so single nodes can just saturate
    a, c = rng.choice([-1, 0, 1], (n, 8, 1), p=[.4, .2, .4]), rng.choice([-1, 0, 1], (n, 1, 8), p=[.4, .2, .4])
    fam.append(np.rint(a * c * 2047 * amp(n).reshape(n, 1, 1)).astype(np.int64).reshape(n, 64))
    a, c = rng.integers(-2047, 2048, (n, 8, 1)), rng.integers(-2047, 2048, (n, 1, 8))
    fam.append((a * c // 2047).reshape(n, 64))
    # the corner of every pass-1 output: the inputs of one coefficient row at the signs of the
    # output's impulse responses, at a few amplitudes, alone or beside a second row
    imp = np.stack([idct_1d(list(1024 * np.eye(8, dtype=np.int64)[i]))[:, ] for i in range(8)], 1)  # [out, in]
    b = []
    for k in range(8):
        for sg in (1, -1):
            for j in range(8):
                for a in (1.0, 0.97, 0.9, 0.8, 0.7, 0.6):
                    blk = np.zeros((8, 8), np.int64)
                    blk[:, j] = np.rint(sg * np.sign(imp[k]) * 2047 * a)
                    b.append(blk.reshape(64))
                    blk = blk.copy()
                    blk[:, (j + 1 + int(rng.integers(7))) % 8] = rng.integers(-2047, 2048, 8)
                    b.append(blk.reshape(64))
    fam.append(np.array(b))
    Q0 = np.concatenate(fam)
    m = len(Q0)
    if intra:
        dc = np.where(rng.random(m) < 0.5, rng.integers(-32768, 32768, m),
                      rng.choice([-32768, -32767, -11586, -11585, -11584, 0, 1024, 11584, 11585, 11586, 32767], m))
        Q0[:, 0] = np.where(rng.random(m) < 0.35, rng.integers(0, 2048, m), dc)
    F = mismatch(Q0, intra)
    F = F[F[:, 63] != -2048]
    return F, (None if intra else rng.choice(P_VALUES, len(F)))


class Vectors:
    """The witness vectors: F[n, 64], form[n] (0 put, 1 add), p[n]; conds: (mutant name, form,
    line or -1, vector); bounded and unkilled: (mutant name, form, line)."""

    def __init__(self, F, form, p, conds, bounded_, unkilled):
        self.F, self.form, self.p = np.asarray(F, np.int16), np.asarray(form, np.uint8), np.asarray(p, np.uint8)
        self.conds, self.bounded, self.unkilled = conds, bounded_, unkilled
        self._kills = {}

    def pred(self):
        return np.repeat(self.p[:, None], 64, 1)

    def witnesses(self, name):
        return sorted({c[3] for c in self.conds if c[0] == name})

    def expected(self):
        out = model_idct(self.F, None)
        a = self.form == 1
        out[a] = model_idct(self.F[a], self.p[a].astype(np.int64))
        return out

    def killed_by(self, m):
        """Vectors whose bytes mutant m (on all lines) changes."""
        if m not in self._kills:
            base = self.expected()
            out = model_idct(self.F, None, m)
            a = self.form == 1
            out[a] = model_idct(self.F[a], self.p[a].astype(np.int64), m)
            if m[0] == "add_for_put":  # an intra block of a P or B picture, over the prediction under it
                out[~a] = model_idct(self.F[~a], np.full((~a).sum(), 128), m)
            self._kills[m] = (out != base).any(1)
        return self._kills[m]


def conditions():
    out = []
    for m in ARITH + OUTPUT:
        for form in (0, 1):
            if m[0] in ("add_wrap", "add_carry") and form == 0:
                continue
            out += [(m, form, line) for line in range(8)]
    return out + [(FORM[0], 1, -1), (FORM[1], 0, -1)]


def search(seed=SEED, n=5000, chunk=192, tries=12):
    """Deterministic from the seed: per condition (mutant, form, line) the first vector already
    chosen that kills it, else the first pool block that does."""
    rng = np.random.default_rng(seed)
    pools, recs, base, chosen = [], [], [], [[], []]
    for form in (0, 1):
        F, p = _pool(rng, form == 0, n)
        rec = {}
        pools.append((F, p))
        base.append(model_idct(F, p, rec=rec))
        recs.append(rec)
    conds, bnd, unk = [], [], []

    def kills(m, form, line, idx):
        F, p = pools[form]
        pp = None if p is None else p[idx]
        if m[0] == "add_for_put":
            pp = np.full(len(idx), 128)
        out = model_idct(F[idx], pp, m, None if line < 0 else line)
        return (out != base[form][idx]).any(1)

    for m, form, line in conditions():
        name = mutant_name(m)
        if line >= 0 and bounded(m, form == 0, line):
            bnd.append((name, form, line))
            continue
        flag = None
        if m[0] == "wrap":
            flag = recs[form][(m[1], m[2], m[3])][:, line]
        elif m[0] == "shlsat":
            flag = recs[form][(m[1], m[2], "o")][:, line]
        got = None
        ch = np.array(chosen[form], np.int64)
        if flag is not None and len(ch):
            ch = ch[flag[ch]]
        if len(ch):
            k = kills(m, form, line, ch)
            if k.any():
                got = int(ch[np.argmax(k)])
        if got is None:
            cand = np.nonzero(flag)[0] if flag is not None else np.arange(len(pools[form][0]))
            for a in range(0, min(len(cand), chunk * tries), chunk):
                k = kills(m, form, line, cand[a:a + chunk])
                if k.any():
                    got = int(cand[a + np.argmax(k)])
                    chosen[form].append(got)
                    break
        if got is None:
            unk.append((name, form, line))
        else:
            conds.append((name, form, line, got))
    # pool indices -> vector indices, put vectors first
    order = [sorted(set(chosen[0])), sorted(set(chosen[1]))]
    at = [{g: i for i, g in enumerate(order[0])}, {g: len(order[0]) + i for i, g in enumerate(order[1])}]
    F = np.concatenate([pools[0][0][order[0]], pools[1][0][order[1]]])
    form = np.array([0] * len(order[0]) + [1] * len(order[1]))
    p = np.concatenate([np.zeros(len(order[0]), np.int64), pools[1][1][order[1]]])
    return Vectors(F, form, p, [(nm, f, ln, at[f][g]) for nm, f, ln, g in conds], bnd, unk)


# ---------------------------------------------------------------------------------------------
# the corners of the legal domain that matrices 16 and quantiser scale 1 do not reach
# ---------------------------------------------------------------------------------------------
CORNER_KINDS = ("intra qs 2", "inter qs 2", "inter 1s")
W_ONES = 255     # the non-intra matrices' entry 0 in a corner picture: '1s' = (3 * 255 * 112) >> 5 = 2677
QS_OF = {"intra qs 2": 2, "inter qs 2": 2, "inter 1s": 112}


def corner_matrices():
    W = np.full((4, 64), 16, np.int64)
    W[1][0] = W[3][0] = W_ONES
    return W


def corner_blocks(seed=SEED + 1):
    """[(kind, words)]: blocks defined by their words, for MBs of quantiser scale 2 (intra: the even
    values, -2048 = level -1024; non-intra: the odd values, level -1024 clamped to -2048) and 112
    with the '1s' word at +-2677 (AC values +-(2 L + 1) * 56, |L| >= 18 clamped to 2047 / -2048)."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(12):
        n = (63, 63, 40, 12, 3, 1)[t % 6]
        pos = sorted(rng.choice(np.arange(1, 64), n, replace=False).tolist())
        dc = (-32768, 32767, 0, 1024, -1, 2047)[t % 6]
        lv = [-1024 if t < 2 or rng.random() < 0.5 else int(rng.integers(-1024, 1024)) or 1 for _ in pos]
        out.append(("intra qs 2", [(dc, 0, COEF_DC)] + list(zip(lv, pos, [0] * n))))
    for t in range(8):
        n = (63, 40, 12, 2)[t % 4]
        pos = sorted(rng.choice(np.arange(1, 64), n, replace=False).tolist())
        lv = [-1024 if t < 1 or rng.random() < 0.5 else int(rng.integers(-1023, 1024)) or 1 for _ in pos]
        out.append(("inter qs 2", list(zip(lv, pos, [0] * n))))
    for t in range(12):
        n = (63, 63, 30, 8, 1, 0)[t % 6]
        pos = sorted(rng.choice(np.arange(1, 64), n, replace=False).tolist())
        lv = [(-18 if t % 2 else 18) if t < 2 or rng.random() < 0.3 else int(rng.integers(-19, 19)) or 1 for _ in pos]
        out.append(("inter 1s", [(-1 if (t // 6 + t) % 2 else 1, 0, COEF_FIRST1S)] + list(zip(lv, pos, [0] * n))))
    return out


def corner_qfs(kind, words):
    W = corner_matrices()[0 if kind.startswith("intra") else 1].tolist()
    return Q.model_qfs([Q._pack(l, pos, 0, fl) for l, pos, fl in words], W, QS_OF[kind], kind.startswith("intra"), 0)


_vectors = None


def vectors():
    """The committed witness vectors (tests/golden/idct_directed.npz, made by
    tests/golden/make_idct_directed.py from search())."""
    global _vectors
    if _vectors is None:
        z = np.load(FIXTURE)
        names = [str(x) for x in z["names"]]
        conds = [(names[a], int(b), int(c), int(d)) for a, b, c, d in z["conds"]]
        bnd = [(names[a], int(b), int(c)) for a, b, c in z["bounded"]]
        _vectors = Vectors(z["F"], z["form"], z["pred"][:, 0], conds, bnd, [])
        _vectors.put, _vectors.add = z["put"], z["add"]
        _vectors.corner = {k: z["corner_" + k] for k in ("F", "pred", "put", "add")}
    return _vectors


# ---------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------
KINDS = {"I": ("intra I",), "P": ("intra P", "inter P"), "B": ("intra B", "inter B"),
         "mixed": ("intra mixed", "inter mixed")}
MAX_PICTURES = Q.MAX_PICTURES
SCAN = Q.QFS_OF_POS[0]
WAVE_STRIDES = (4, 2)  # recon_kernel: a wave's next group is `step` MBs on, step = 4 waves * G, or
#                        (4 / 2 slices per workgroup) * G when the workgroup runs two slices (wpos, step)


def uni_rounds(gsize, nb=6):
    """The 4:2:0 I kernel's shared IDCT rounds (run_slice, UNI) for a group of gsize MBs, restated:
    n4 = 4 * slots items per pass, pass 2 starts at item max(n4, 64), rounds of 64 items, and a
    round takes the folded form iff base + 64 <= n4.  [(base, form, pass-1 slots, pass-2 slots)]."""
    n4 = gsize * nb * 4
    p2b = max(n4, 64)
    out = []
    for base in range(0, p2b + n4, 64):
        t = range(base, base + 64)
        s1 = sorted({u >> 2 for u in t if u < n4})
        s2 = sorted({(u - p2b) >> 2 for u in t if u >= p2b and u - p2b < n4})
        out.append((base, "fold" if base + 64 <= n4 else "exact", s1, s2))
    return out


def vec_words(F, intra):
    """The coefficient words (level, scan position, flags) of QFS block F at W = 16, quantiser
    scale 1: every value is its own level, and F's odd sum keeps mismatch control from toggling."""
    F = [int(v) for v in F]
    assert (sum(F) - (F[0] if intra else 0)) % 2 == 1 and all(abs(v) <= 2047 for v in F[1:])
    ws = [(F[0], 0, COEF_DC)] if intra else []
    for i in range(1 if intra else 0, 64):
        if F[SCAN[i]]:
            ws.append((F[SCAN[i]], i, 0))
    return ws


def placement(cf, b, dctf):
    """(plane, x0, y0, row step) of block b in its MB (mb_decoder.cpp:176-195)."""
    plane, x0, y0 = Q.block_origin(cf, b)
    if dctf and (plane == 0 or cf != 1):
        return plane, x0, (1 if y0 else 0), 2
    return plane, x0, y0, 1


class IdctBatch:
    def __init__(self, name, width, height, cf, launch, pics, mbs, coefs, first_case_pic):
        self.name, self.width, self.height, self.cf, self.launch = name, width, height, cf, launch
        self.pics, self.mbs, self.coefs, self.first_case_pic = pics, mbs, coefs, first_case_pic
        self._blocks = None

    def key(self):
        return (self.name, self.width, self.height, self.cf, self.launch)


def _anchors(B, launch):
    """Flat anchors per prediction value: an I picture of DC-only blocks and, for B pictures, a P
    picture that copies it (zero vector, nothing coded).  {p: (forward slot, backward slot)}."""
    zero = np.zeros((2, 2, 2), np.int16)
    out = {}
    n = B.mbw * B.mbh
    for p in P_VALUES if launch != "I" else ():
        i = B.picture(1)
        for _ in range(n):
            B.mb(MB_INTRA, {b: [(P_DC[p], 0, COEF_DC)] for b in range(B.nb)}, 1)
        j = -1
        if launch in ("B", "mixed"):
            j = B.picture(2, i)
            for _ in range(n):
                B.mb(MB_FWD, {}, 1, zero)
        out[p] = (i, j)
    return out


def _case_picture(B, launch, anchors, q, qmat=16):
    """Case picture q: (picture, its flat prediction, inter MB flags)."""
    p = P_VALUES[q % 3]
    if launch == "I":
        return B.picture(1, qmat=qmat), None, 0
    f, b = anchors[p]
    if launch == "P":
        return B.picture(2, f, qmat=qmat), p, MB_FWD
    one_dir = launch == "mixed" and q % 2 == 0
    return B.picture(3, -1 if one_dir else f, b, qmat), p, (MB_BWD if one_dir else MB_FWD | MB_BWD)


_batches = {}


def idct_batch(width, height, cf, launch, seed=7300):
    """launch I: I pictures.  P / B / mixed: the flat anchors, then P pictures, two-direction B
    pictures, or backward-only and two-direction B pictures in turn (one mixed launch), each
    predicted from the anchors of one prediction value; every third MB intra, every second one field
    DCT (4:2:0, 4:2:2), the inter MBs' cbp full, drawn, full, a single block in turn (every third
    group: all full, for the last slots).  Blocks are
    filled with the witness vectors (quantiser matrices 16, quantiser scale 1) until every vector
    has been in every MB kind and every cell of needs() has its witness.  Then the corner pictures:
    corner_blocks() in MBs of quantiser scale 2 and 112 under corner_matrices()."""
    ck = (width, height, cf, launch, seed)
    if ck in _batches:
        return _batches[ck]
    V = vectors()
    B = _Builder(width, height, cf, seed + 100 * cf + width + height + sum(map(ord, launch)))
    rng, nb, mbw = B.rng, B.nb, B.mbw
    zero = np.zeros((2, 2, 2), np.int16)
    anchors = _anchors(B, launch)
    first = len(B.pics)
    cls = vector_classes(V)
    left = {kind: {v for v in range(len(V.F)) if (V.form[v] == 1) == kind.startswith("inter")} for kind in KINDS[launch]}
    cells = needs(width, cf, launch)
    words = {}
    q = gcount = 0
    # (a mixed launch needs a backward-only and a two-direction picture per prediction value)
    while any(left.values()) or cells or (launch == "mixed" and q < 6):
        assert len(B.pics) < MAX_PICTURES, ("needs no picture could meet", launch, sorted(cells)[:8])
        _, p, inter_flags = _case_picture(B, launch, anchors, q)
        for y in range(B.mbh):
            for g0 in range(0, mbw, 4):
                gsize, slot = min(4, mbw - g0), 0
                gcount += 1
                for k in range(gsize):
                    t = B.k + q
                    intra = launch == "I" or t % 3 == 0
                    kind = ("intra " if intra else "inter ") + launch
                    dctf = cf != 3 and t % 2 == 1
                    coded = list(range(nb))
                    if gcount % 3 == 0:  # a group with every block coded: the last slots
                        pass
                    elif not intra and t % 4 == 1:
                        coded = [b for b in coded if rng.random() < 0.5] or [int(rng.integers(nb))]
                    elif not intra and t % 4 == 3:
                        coded = [int(rng.integers(nb))]
                    blocks = {}
                    for b in coded:
                        here = [c for c in block_cells(launch, gsize, slot, b, dctf, intra) if c in cells]
                        ok = [v for v in range(len(V.F)) if (V.form[v] == 0) == intra and (intra or V.p[v] == p)]
                        best = max(ok, key=lambda v: (sum(c[0] in cls[v] for c in here), v in left[kind], -v))
                        if not here and not any(v in left[kind] for v in ok):
                            best = ok[int(rng.integers(len(ok)))]
                        left[kind].discard(best)
                        cells.difference_update(c for c in here if c[0] in cls[best])
                        if (best, intra) not in words:
                            words[(best, intra)] = vec_words(V.F[best], intra)
                        blocks[b] = words[(best, intra)]
                        slot += 1
                    B.mb((MB_INTRA if intra else inter_flags) | (MB_DCT_FIELD if dctf else 0), blocks, 1,
                         None if intra else zero)
        q += 1
    # the corner pictures: their own matrices, an MB's quantiser scale by its kind, every block coded
    corners = corner_blocks()
    at = {kind: 0 for kind in CORNER_KINDS}
    for _ in range(2 if launch == "I" else 6):
        _, p, inter_flags = _case_picture(B, launch, anchors, q, corner_matrices())
        for _ in range(mbw * B.mbh):
            kind = CORNER_KINDS[0 if launch == "I" else (B.k + q) % 3]
            mine = [wds for kd, wds in corners if kd == kind]
            blocks = {}
            for b in range(nb):
                blocks[b] = mine[at[kind] % len(mine)]
                at[kind] += 1
            intra = kind.startswith("intra")
            B.mb(MB_INTRA if intra else inter_flags, blocks, QS_OF[kind], None if intra else zero)
        q += 1
    pics, mbs, coefs = B.finish()
    _batches[ck] = IdctBatch("idct", width, height, cf, launch, pics, mbs, coefs, first)
    return _batches[ck]


def stale_batch(cf, launch, seed=7400):
    """512x16: rows of eight groups.  Groups 0-3 of a row hold dense blocks (all 64 positions at
    +-2047), groups 4-7 single-coefficient blocks (position 0 only and position 63 only in turn,
    per picture), every block coded: whichever of WAVE_STRIDES the launch runs with, a wave meets a
    sparse block after a dense one in every slot."""
    ck = (cf, launch, seed)
    if ck in _batches:
        return _batches[ck]
    B = _Builder(512, 16, cf, seed + cf + sum(map(ord, launch)))
    rng, nb = B.rng, B.nb
    zero = np.zeros((2, 2, 2), np.int16)
    anchors = _anchors(B, launch)
    first = len(B.pics)
    for q in range(6):
        _, p, inter_flags = _case_picture(B, launch, anchors, q)
        for x in range(B.mbw):
            intra = launch == "I" or (x + q) % 5 == 0
            blocks = {}
            for b in range(nb):
                if x < 16:
                    F = rng.choice([-2047, 2047], 64)
                    F[63] -= np.sign(F[63]) * int((F.sum() - (F[0] if intra else 0)) % 2 == 0)
                elif q % 2 == 0:
                    F = np.zeros(64, np.int64)  # (an intra block: its DC word alone)
                    F[0] = 1031 + 2 * b if intra else (-1) ** b * (301 + 2 * x)
                else:
                    F = np.zeros(64, np.int64)
                    F[63] = (-1) ** (b + x) * 2047
                    F[0] = 1024 if intra else 0
                blocks[b] = vec_words(F, intra) if (F[1:] != 0).any() or not intra else [(int(F[0]), 0, COEF_DC)]
            B.mb(MB_INTRA if intra else inter_flags, blocks, 1, None if intra else zero)
    pics, mbs, coefs = B.finish()
    _batches[ck] = IdctBatch("stale", 512, 16, cf, launch, pics, mbs, coefs, first)
    return _batches[ck]


# ---------------------------------------------------------------------------------------------
# what a finished batch holds, from its records
# ---------------------------------------------------------------------------------------------
def vector_classes(V):
    """Per vector the witness classes the cells ask for: a saturating pass-1 / pass-2 node, the
    two fold mutants, and output rows that differ (a wrong row step shows)."""
    out = [set() for _ in V.F]
    for name, _, _, v in V.conds:
        for c, pre in (("sat1", "p1.wrap."), ("sat2", "p2.wrap."), ("fold_p2", "fold_p2"), ("fold_s0", "fold_s0")):
            if name.startswith(pre):
                out[v].add(c)
    e = V.expected().reshape(-1, 8, 8)
    for v in np.nonzero((e != e[:, :1]).any((1, 2)))[0]:
        out[v].add("rows")
    return out


def block_cells(launch, gsize, slot, b, dctf, intra):
    """The (class, cell) pairs a block of this place can serve."""
    out = [("rows", "block %d %s DCT" % (b, "field" if dctf else "frame"))]
    if launch == "I":
        out += [(c, "group of %d slot %d" % (gsize, slot)) for c in ("fold_p2", "fold_s0")]
    else:
        out += [(c, "slot %d" % slot) for c in ("sat1", "sat2")]
    return out


def needs(width, cf, launch):
    nb, mbw = NB[cf], width // 16
    out = {("rows", "block %d %s DCT" % (b, d)) for b in range(nb) for d in (("frame", "field") if cf != 3 else ("frame",))}
    if launch == "I":
        for gsize in {4} | ({mbw % 4} - {0}):
            out |= {(c, "group of %d slot %d" % (gsize, s)) for s in range(gsize * nb) for c in ("fold_p2", "fold_s0")}
    else:
        out |= {(c, "slot %d" % s) for s in range(4 * nb) for c in ("sat1", "sat2")}
    return out


class Block:
    __slots__ = ("p", "mb", "x", "y", "b", "k", "gsize", "group", "slot", "dctf", "intra", "kind", "F", "pred", "vec", "pos",
                 "corner")


def flat_values(batch):
    """Per picture the value of a flat anchor (an I picture of equal DC-only blocks, or a P picture
    that copies one), else None."""
    pics, mbs, coefs = batch.pics, batch.mbs, batch.coefs
    n = (batch.width // 16) * (batch.height // 16)
    out = []
    for p in range(len(pics)):
        a = int(pics[p]["mb_first"])
        t = int(pics[p]["picture_coding_type"])
        nc = int(mbs["ncoef"][a:a + n].sum())
        w = coefs[int(mbs["coef_off"][a]):int(mbs["coef_off"][a]) + nc]
        val = None
        if t == 1 and nc == n * NB[batch.cf] and len(set((w & 0xFFFF).tolist())) == 1 and (w & COEF_DC).all():
            val = int(model_idct(np.eye(1, 64, 0, dtype=np.int64) * int(w[0] & 0xFFFF))[0, 0])
        elif t == 2 and nc == 0 and not mbs["mv"][a:a + n].any() and not (mbs["flags"][a:a + n] & MB_INTRA).any():
            val = out[int(pics[p]["fwd_slot"])]
        out.append(val)
    return out


def batch_blocks(batch):
    """Every coded block of the case pictures, with its place in the kernel (MB k of a group of
    gsize, coded-block slot) and the model's QFS; vec: the witness vector it equals, or -1."""
    if batch._blocks is not None:
        return batch._blocks
    V = vectors()
    lookup = {(V.F[v].tobytes(), int(V.form[v]), int(V.p[v]) if V.form[v] else 0): v for v in range(len(V.F))}
    corner = {(V.corner["F"][c].tobytes(), kd.startswith("intra")): c for c, (kd, _) in enumerate(corner_blocks())}
    pics, mbs, cl = batch.pics, batch.mbs, batch.coefs.tolist()
    mbw, mbh, nb = batch.width // 16, batch.height // 16, NB[batch.cf]
    flat = flat_values(batch)
    out = []
    for p in range(batch.first_case_pic, len(pics)):
        first = int(pics[p]["mb_first"])
        refs = [flat[int(pics[p][s])] for s in ("fwd_slot", "bwd_slot") if int(pics[p][s]) >= 0]
        assert len(set(refs)) <= 1 and None not in refs, (p, refs)
        for y in range(mbh):
            for g0 in range(0, mbw, 4):
                gsize, slot = min(4, mbw - g0), 0
                for k in range(gsize):
                    i = first + y * mbw + g0 + k
                    fl, cbp = int(mbs["flags"][i]), int(mbs["cbp"][i])
                    off, nc = int(mbs["coef_off"][i]), int(mbs["ncoef"][i])
                    ws = cl[off:off + nc]
                    intra = bool(fl & MB_INTRA)
                    for b in range(nb):
                        if not cbp >> b & 1:
                            continue
                        bl = Block()
                        bl.p, bl.mb, bl.x, bl.y, bl.b, bl.k, bl.gsize, bl.group = p, i, g0 + k, y, b, k, gsize, g0 // 4
                        bl.slot, bl.dctf, bl.intra = slot, bool(fl & MB_DCT_FIELD), intra
                        bl.kind = ("intra " if intra else "inter ") + batch.launch
                        wb = [w for w in ws if (w >> 22) & 15 == b]
                        bl.pos = tuple((w >> 16) & 63 for w in wb)  # the words' scan positions
                        W = pics[p]["W"][Q.block_row(b, intra)].tolist()
                        bl.F = Q.model_qfs(wb, W, int(mbs["qscale"][i]), intra, 0)
                        bl.pred = None if intra else refs[0]
                        fb = np.array(bl.F, np.int16).tobytes()
                        bl.vec = lookup.get((fb, int(not intra), 0 if intra else bl.pred), -1)
                        bl.corner = corner.get((fb, intra), -1) if bl.vec < 0 else -1
                        out.append(bl)
                        slot += 1
    batch._blocks = out
    return out


def coverage(batch):
    """From the records: {MB kind: vectors present} and the (class, cell) pairs served."""
    V = vectors()
    cls = vector_classes(V)
    kinds, cells = {}, set()
    for bl in batch_blocks(batch):
        if bl.vec < 0:
            continue
        kinds.setdefault(bl.kind, set()).add(bl.vec)
        cells |= {c for c in block_cells(batch.launch, bl.gsize, bl.slot, bl.b, bl.dctf, bl.intra) if c[0] in cls[bl.vec]}
    return kinds, cells


def stale_successions(batch, stride):
    """{slot: count} of (dense block, then sparse block in the same slot of the same wave's next
    group of the row) for waves `stride` groups apart."""
    at = {(bl.p, bl.y, bl.group, bl.slot): len(bl.pos) for bl in batch_blocks(batch)}
    out = {}
    for (p, y, g, s), n in at.items():
        if n == 64 and 0 < at.get((p, y, g + stride, s), 0) <= 2:
            out[s] = out.get(s, 0) + 1
    return out


def coverage_table(batch):
    kinds, cells = coverage(batch)
    want = needs(batch.width, batch.cf, batch.launch)
    lines = ["%-12s %d vectors" % (k, len(v)) for k, v in sorted(kinds.items())]
    for c in ("rows", "sat1", "sat2", "fold_p2", "fold_s0"):
        w = {x for x in want if x[0] == c}
        if w:
            lines.append("%-8s %3d/%d cells" % (c, len(w & cells), len(w)))
    return "\n".join(lines)


def model_frames(batch, mut=None):
    """The batch's frames from the model alone: flat anchors, the flat prediction under every
    inter MB, every coded block's bytes at its placement.  mut: None, a model mutant (applied to every
    block) or a batch mutant: 'field_step_ignored', ('chunk_unzeroed', chunk, stride)."""
    w, h, cf = batch.width, batch.height, batch.cf
    from directed import plane_dims
    pw, ph, bw, bh = plane_dims(w, h, cf)
    flat = flat_values(batch)
    frames = []
    for p in range(len(batch.pics)):
        v = flat[p]
        if v is None:
            refs = [flat[int(batch.pics[p][s])] for s in ("fwd_slot", "bwd_slot") if int(batch.pics[p][s]) >= 0]
            v = refs[0] if refs else 0
        frames.append([np.full((ph[k], pw[k]), v, np.uint8) for k in range(3)])
    blocks = batch_blocks(batch)
    F = np.array([bl.F for bl in blocks], np.int64)
    if isinstance(mut, tuple) and mut[0] == "chunk_unzeroed":
        F = stale_qfs(blocks, F, mut[1], mut[2])
    mm = mut if isinstance(mut, tuple) and mut[0] != "chunk_unzeroed" else None
    out = np.zeros((len(blocks), 64), np.uint8)
    intra = np.array([bl.intra for bl in blocks])
    pred = np.array([bl.pred or 0 for bl in blocks], np.int64)
    if intra.any():
        out[intra] = model_idct(F[intra], None, mm)
    if (~intra).any():
        out[~intra] = model_idct(F[~intra], pred[~intra], mm)
    for bl, o in zip(blocks, out):
        plane, x0, y0, ys = placement(cf, bl.b, bl.dctf and mut != "field_step_ignored")
        X, Y = bl.x * bw[plane] + x0, bl.y * bh[plane] + y0
        frames[bl.p][plane][Y:Y + 8 * ys:ys, X:X + 8] = o.reshape(8, 8)
    return frames


def stale_qfs(blocks, F, chunk, stride):
    """chunk_unzeroed: pass 2 leaves 16-B chunk `chunk` of every block as it read it (pass 1's output
    column `chunk`, rows 0-7).  The wave's next group (stride groups on in the row) writes its words
    over it, in the pair-interleaved layout: element e of the chunk is coefficient (row 2 * (chunk >> 1)
    + (e & 1), column 4 * (chunk & 1) + (e >> 1)); positions without a word keep the stale value, and
    the parity is taken over what the block then holds."""
    at = {(bl.p, bl.y, bl.group, bl.slot): n for n, bl in enumerate(blocks)}
    o1 = _pass(F.reshape(-1, 8, 8), 0, None, None)  # [n, x, v]
    out = F.copy()
    for n, bl in enumerate(blocks):
        prev = at.get((bl.p, bl.y, bl.group - stride, bl.slot))
        if prev is None:
            continue
        Q0 = F[n].copy()  # (the records' blocks have odd sums: F is what the words wrote)
        for e in range(8):
            row, col = 2 * (chunk >> 1) + (e & 1), 4 * (chunk & 1) + (e >> 1)
            if Q0[col * 8 + row] == 0:
                Q0[col * 8 + row] = o1[prev, chunk, e]
        out[n] = mismatch(Q0[None], bl.intra)[0]
    return out
