"""Vectors and integer expectations for lib/arith_check (csrc/tools/arith_check.cpp),
shared by tests/test_gpu_arith.py (runs them on the device) and
tests/test_arith_vectors_cpu.py (checks on the CPU that they reach the branches
they are meant to reach).  TEST INFRASTRUCTURE ONLY.

A record is (op, operand words, kind, want).  Words are the raw 256-bit machine
values the device function takes and returns (Montgomery representatives
included); every expectation is computed here with Python integers, the
oracle's curves and oracle/pairing_tower.py.  `kind` says how the result words
are normalised before the exact comparison with `want`:
  raw        the words themselves
  jac:<c>    (X, Y, Z) Montgomery on curve c -> affine canonical point, None at Z == 0
  xyzz       (X, Y, ZZ, ZZZ) Montgomery on BN254 -> the same (ZZ^3 == ZZZ^2 asserted)
"""
import functools
import os
import random
import re

from oracle import bn254 as bn, ecdsa_p256 as p256o, idemix as OI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "fabric-token-sdk_amd", "csrc", "device")
RR = 1 << 256  # the Montgomery radix of every field here

MODS = {"fp": bn.P, "fr": bn.R, "p256p": p256o.P, "p256n": p256o.N, "fbnp": OI.FP256BNC.p, "fbnr": OI.FP256BNC.r}
WIDE = ("p256p", "p256n", "fbnp", "fbnr")       # full-width moduli (p256.hpp's code)
WIDE_MUL = ("p256p", "p256n", "fbnp")           # fbn::RM has no Montgomery constants: add/sub/cond_sub only
PRODUCT_OPS = [("fp_mul", "fp"), ("fp_mulg", "fp"), ("fr_mul", "fr"), ("fr_mulg", "fr")] + \
              [(m + "_mul", m) for m in WIDE_MUL]

_TOWER = [("f2_mul", 4, 2), ("f2_sqr", 2, 2), ("f2_inv", 2, 2), ("f2_mul_xi", 2, 2), ("f6_mul", 12, 6),
          ("f6_mul01", 10, 6), ("f6_mul_v", 6, 6), ("f6_inv", 6, 6), ("f12_mul", 24, 12), ("f12_sqr", 12, 12),
          ("f12_cyc_sqr", 12, 12), ("f12_inv", 12, 12), ("f12_conj", 12, 12), ("f12_frob1", 12, 12),
          ("f12_frob2", 12, 12), ("f12_frob3", 12, 12), ("line_mul", 18, 12)]


def _catalogue():
    c = []
    for m in ("fp", "fr"):
        c += [(m + "_add", 2, 1), (m + "_sub", 2, 1), (m + "_neg", 1, 1), (m + "_dbl", 1, 1), (m + "_mul", 2, 1),
              (m + "_to_mont", 1, 1), (m + "_from_mont", 1, 1), (m + "_reduce_once", 1, 1), (m + "_lt_mod", 1, 1),
              (m + "_mulg", 2, 1), (m + "_inv", 1, 1)]
    for m in WIDE:
        c += [(m + "_add", 2, 1), (m + "_sub", 2, 1), (m + "_cond_sub", 2, 1)]
        if m in WIDE_MUL:
            c += [(m + "_mul", 2, 1), (m + "_to_mont", 1, 1), (m + "_from_mont", 1, 1), (m + "_inv", 1, 1)]
    c += [("lt256", 2, 1),
          ("g1j_dbl", 3, 3), ("g1j_add_affine", 5, 3), ("g1j_add", 6, 3), ("madd_inl", 5, 3), ("add_inl", 6, 3),
          ("g1j_to_affine", 3, 2), ("g1j_eq", 6, 1), ("xmadd_inl", 6, 4), ("xadd_inl", 8, 4), ("g1x_dbl", 4, 4),
          ("g1x_to_jac", 4, 3), ("var_base_mul", 3, 3), ("glv_mul", 3, 3), ("vb128j", 4, 3), ("straus2_128", 8, 3),
          ("glv_decompose_bn", 1, 4), ("glv_decompose_fbn", 1, 4)]
    for c_ in ("p256", "fbn"):
        c += [(c_ + "_pj_dbl", 3, 3), (c_ + "_pj_add", 6, 3), (c_ + "_pj_madd", 5, 3), (c_ + "_on_curve", 2, 1)]
    for t in ("bn", "fbn"):
        c += [(t + "_" + n, ni, no) for n, ni, no in _TOWER]
    return c


CATALOGUE = _catalogue()
# the FP256BN chain's op, listed by `arith_check --list-glv`: apart from the primitives' catalogue, which
# stays as it is (as the com chain's and the fixed-base ops are)
GLV_CATALOGUE = [("fbn_glv_mul", 3, 3)]
ARITY = {n: (ni, no) for n, ni, no in CATALOGUE + GLV_CATALOGUE}


# ------------------------------------------------------------ Montgomery helpers
def to_mont(x, M):
    return x * RR % M


def from_mont(x, M):
    return x * pow(RR, -1, M) % M


def mont_mul(a, b, M):
    """the Montgomery product of two representatives: a b R^-1 mod M"""
    return a * b * pow(RR, -1, M) % M


def mont_t(a, b, M):
    """the product's value before its conditional subtraction: t = (a b + m M) / R with
    m = -a b M^-1 mod R, so t = a b R^-1 (mod M) and t < 2M"""
    m = (-a * b * pow(M, -1, RR)) % RR
    t, rem = divmod(a * b + m * M, RR)
    assert rem == 0
    return t


# ------------------------------------------------------------------ field vectors
def edge_set(M):
    """values < M where multi-limb code goes wrong, closed under negation"""
    ones7 = ((M >> 224) << 224) | ((1 << 224) - 1)
    if ones7 >= M:
        ones7 -= 1 << 224
    alt = sum(0xffffffff << (64 * i) for i in range(4))

    def mask(v):  # clear top bits until v < M
        while v >= M:
            v &= (1 << (v.bit_length() - 1)) - 1
        return v
    e = [0, 1, 2, M - 1, M - 2, (M - 1) // 2, (M + 1) // 2, RR % M, (-RR) % M, (1 << 32) - 1, 1 << 32,
         (1 << 64) - 1, 1 << 128, 1 << 224, ones7, ((M - 1) >> 32) << 32, mask(alt), mask(alt << 32)]
    out = []
    for v in e + [(-v) % M for v in e]:
        assert 0 <= v < M
        if v not in out:
            out.append(v)
    return out


def binary_pairs(M, seed):
    E = edge_set(M)
    rng = random.Random(seed)
    out = [(a, b) for a in E for b in E] + [(rng.randrange(M), rng.randrange(M)) for _ in range(512)]
    # sums that are 2^256 exactly (full-width moduli only: both operands must stay below M)
    xs = [M - 1, M - 2, 1 << 255, (1 << 255) + 1, (1 << 255) - 1] + [rng.randrange(1 << 255, RR) for _ in range(8)]
    return out + [(x, RR - x) for x in xs if x < M and RR - x < M]


def unary_values(M, seed):
    rng = random.Random(seed)
    out = list(edge_set(M))
    out += [1 << k for k in range(256) if (1 << k) < M]
    out += [(1 << k) - 1 for k in range(1, 257) if (1 << k) - 1 < M]
    return out + [rng.randrange(M) for _ in range(256)]


def inv_values(M, seed):
    """non-zero values with the zero at lane 17 of the first wave"""
    v = [x for x in unary_values(M, seed) if x != 0]
    return v[:17] + [0] + v[17:]


def _seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


@functools.lru_cache(maxsize=None)
def field_records():
    recs = []
    for m, M in MODS.items():
        wide = m in WIDE
        pairs = binary_pairs(M, _seed(m))
        for a, b in pairs:
            recs.append((m + "_add", [a, b], "raw", [(a + b) % M]))
            recs.append((m + "_sub", [a, b], "raw", [(a - b) % M]))
        muls = [op for op, mm in PRODUCT_OPS if mm == m]
        for op in muls:
            recs += [(op, [a, b], "raw", [mont_mul(a, b, M)]) for a, b in pairs]
        if not wide or m in WIDE_MUL:
            un = unary_values(M, _seed(m) + 1)
            recs += [(m + "_to_mont", [a], "raw", [to_mont(a, M)]) for a in un]
            recs += [(m + "_from_mont", [a], "raw", [from_mont(a, M)]) for a in un]
            # inverse of the value whose representative is A: A^-1 R^2 mod M; inv(0) = 0
            recs += [(m + "_inv", [a], "raw", [pow(a, -1, M) * RR * RR % M if a else 0])
                     for a in inv_values(M, _seed(m) + 2)]
        rng = random.Random(_seed(m) + 3)
        if not wide:
            un = unary_values(M, _seed(m) + 1)
            recs += [(m + "_neg", [a], "raw", [(-a) % M]) for a in un]
            recs += [(m + "_dbl", [a], "raw", [2 * a % M]) for a in un]
            E = edge_set(M)
            lt2m = E + [M + x for x in E] + [rng.randrange(2 * M) for _ in range(128)]
            recs += [(m + "_reduce_once", [a], "raw", [a - M if a >= M else a]) for a in lt2m]
            words = E + [M, M + 1, RR - 1, RR - 2, 1 << 255] + [M + (1 << (32 * i)) for i in range(8)] + \
                    [M - (1 << (32 * i)) for i in range(8)] + [rng.randrange(RR) for _ in range(128)]
            recs += [(m + "_lt_mod", [a], "raw", [int(a < M)]) for a in words]
        else:
            E = edge_set(M)
            xs0 = E + [M, M + 1, RR - 1, RR - 2] + [rng.randrange(RR) for _ in range(128)] + \
                  [M + x for x in E if M + x < RR] + [rng.randrange(M, RR) for _ in range(64)]
            top = 2 * M - RR  # carry set: x + 2^256 < 2M
            xs1 = [0, 1, top - 1, top - 2, top // 2, (1 << 32) - 1, 1 << 32] + [rng.randrange(top) for _ in range(128)]
            for c, xs in ((0, xs0), (1, xs1)):
                for x in xs:
                    v = x + c * RR
                    assert v < 2 * M
                    recs.append((m + "_cond_sub", [x, c], "raw", [v - M if v >= M else v]))
    rng = random.Random(99)
    ws = [0, 1, RR - 1, RR - 2, 1 << 255, (1 << 255) - 1] + [1 << (32 * i) for i in range(8)] + \
         [(1 << (32 * i)) - 1 for i in range(1, 8)]
    pairs = [(a, b) for a in ws for b in ws]
    for _ in range(128):
        a = rng.randrange(RR)
        pairs += [(a, a), (a, a ^ (1 << rng.randrange(256))), (a, rng.randrange(RR))]
    recs += [("lt256", [a, b], "raw", [int(a < b)]) for a, b in pairs]
    return recs


# -------------------------------------------------------------------------- GLV
def header_consts(header, struct):
    """the limb arrays of `struct NAME { ... }` in a device header, as integers"""
    src = open(os.path.join(DEVICE, header)).read()
    body = src[src.index("struct " + struct):]
    body = body[:body.index("\n};")]
    out = {}
    for name, vals in re.findall(r"(\w+)\[\d+\] = \{([^}]*)\}", body):
        limbs = [int(v.strip().rstrip("u"), 16) for v in vals.split(",")]
        out[name] = sum(l << (32 * i) for i, l in enumerate(limbs))
    return out


GLV_SETS = {"bn": ("glv.hpp", "Glv", bn.R, bn.P), "fbn": ("fp256bn.hpp", "GlvK", OI.FP256BNC.r, OI.FP256BNC.p)}
# what the consuming chain can recode: 32 signed 4-bit windows with no carry out of the
# top one (vb128j, straus2_128) / fbn::glv_mul_tab's 33 windows, the 33rd taking the carry
GLV_BOUND = {"bn": 1 << 127, "fbn": 1 << 128}


def glv_lambda(tag):
    """the eigenvalue the lattice basis belongs to: (a1, b1) = (A1, -NB1) has a1 + b1 lambda = 0 (mod r)"""
    hdr, st, r, _ = GLV_SETS[tag]
    c = header_consts(hdr, st)
    return c["A1"] * pow(c["NB1"], -1, r) % r


def glv_decompose(k, c):
    """the integer Babai step (tests/test_fbn_glv.py _decompose): signed k1, k2"""
    c1 = (k * c["G1"] + (1 << 383)) >> 384
    c2 = (k * c["G2"] + (1 << 383)) >> 384
    return k - c1 * c["A1"] - c2 * c["A2"], c1 * c["NB1"] - c2 * c["A1"]


def scalar_edges(r, lam):
    def nib(d):  # 0xddd...d with as many digits as stay below r
        n = 64
        while int(d * n, 16) >= r:
            n -= 1
        return int(d * n, 16)
    return [0, 1, 2, 8, 9, 15, 16, r - 1, r - 2, lam, lam + 1, lam - 1, r - lam, (r - 1) // 2, nib("8"), nib("9")]


def scalars(r, lam, seed, n=32):
    rng = random.Random(seed)
    return scalar_edges(r, lam) + [rng.randrange(r) for _ in range(n)]


def glv_scalars(tag):
    _, _, r, _ = GLV_SETS[tag]
    ks = scalars(r, glv_lambda(tag), 5, n=2000)
    for k in list(range(0, 257, 32)) + [125, 126, 127, 128, 253, 254, 255]:
        ks += [v for v in (1 << k, (1 << k) - 1) if 0 <= v < r]
    return ks


@functools.lru_cache(maxsize=None)
def glv_records():
    recs = []
    for tag, (hdr, st, r, _) in GLV_SETS.items():
        c = header_consts(hdr, st)
        for k in glv_scalars(tag):
            k1, k2 = glv_decompose(k, c)
            recs.append(("glv_decompose_" + tag, [k], "raw", [abs(k1), int(k1 < 0), abs(k2), int(k2 < 0)]))
    return recs


# ------------------------------------------------------------------ group laws
class Curve:
    """y^2 = x^3 + a x + b over Fp in affine integers; None is the identity"""

    def __init__(self, p, a, b, gen):
        self.p, self.a, self.b, self.gen = p, a, b, gen

    def on(self, P):
        return P is None or (P[1] * P[1] - P[0] ** 3 - self.a * P[0] - self.b) % self.p == 0

    def neg(self, P):
        return None if P is None else (P[0], (-P[1]) % self.p)

    def add(self, P, Q):
        p = self.p
        if P is None:
            return Q
        if Q is None:
            return P
        if P[0] == Q[0]:
            if (P[1] + Q[1]) % p == 0:
                return None
            lam = (3 * P[0] * P[0] + self.a) * pow(2 * P[1], -1, p) % p
        else:
            lam = (Q[1] - P[1]) * pow(Q[0] - P[0], -1, p) % p
        x = (lam * lam - P[0] - Q[0]) % p
        return (x, (lam * (P[0] - x) - P[1]) % p)

    def mul(self, k, P):
        acc = None
        for bit in bin(k)[2:] if k else "":
            acc = self.add(acc, acc)
            if bit == "1":
                acc = self.add(acc, P)
        return acc


CURVES = {"bn": Curve(bn.P, 0, 3, (1, 2)), "p256": Curve(p256o.P, p256o.P - 3, p256o.B, p256o.G),
          "fbn": Curve(OI.FP256BNC.p, 0, 3, (1, 2))}


def jac_words(C, P, z, xy=None):
    """(x z^2, y z^3, z) in Montgomery form; the identity is z = 0 with the given (or unit) x, y"""
    p = C.p
    if P is None:
        x, y = xy if xy else (1, 1)
        return [to_mont(x, p), to_mont(y, p), 0]
    return [to_mont(P[0] * z * z % p, p), to_mont(P[1] * z ** 3 % p, p), to_mont(z, p)]


def xyzz_words(C, P, z, xy=None):
    """(x zz, y zzz, zz, zzz) with zz = z^2, zzz = z^3"""
    p = C.p
    if P is None:
        x, y = xy if xy else (1, 1)
        return [to_mont(x, p), to_mont(y, p), 0, 0]
    zz, zzz = z * z % p, z ** 3 % p
    return [to_mont(P[0] * zz % p, p), to_mont(P[1] * zzz % p, p), to_mont(zz, p), to_mont(zzz, p)]


def aff_words(C, P):
    """affine Montgomery; BN254's G1A encodes the identity as (0, 0)"""
    return [0, 0] if P is None else [to_mont(P[0], C.p), to_mont(P[1], C.p)]


def norm_jac(C, w):
    p = C.p
    assert all(v < p for v in w), "unreduced coordinate"
    x, y, z = (from_mont(v, p) for v in w)
    if z == 0:
        return None
    zi = pow(z, -1, p)
    return (x * zi * zi % p, y * zi ** 3 % p)


def norm_xyzz(C, w):
    p = C.p
    assert all(v < p for v in w), "unreduced coordinate"
    x, y, zz, zzz = (from_mont(v, p) for v in w)
    assert pow(zz, 3, p) == zzz * zzz % p, "ZZ^3 != ZZZ^2"
    if zz == 0:
        return None
    return (x * pow(zz, -1, p) % p, y * pow(zzz, -1, p) % p)


def normalise(kind, words):
    if kind == "raw":
        return list(words)
    if kind == "xyzz":
        return norm_xyzz(CURVES["bn"], words)
    assert kind.startswith("jac:")
    return norm_jac(CURVES[kind[4:]], words)


def _points(C, seed):
    rng = random.Random(seed)
    n = 1 << 200
    return [C.mul(rng.randrange(1, n), C.gen) for _ in range(3)], rng


def add_cases(C, seed, q_identity, both_identity):
    """(P, zP, Q, zQ, xyP, xyQ): operand pairs every addition formula must get right;
    z in {1, M-1, random}; xy: coordinates of an identity operand"""
    (A, B, D), rng = _points(C, seed)
    p = C.p
    zs = [1, p - 1, rng.randrange(2, p)]
    out = []
    for za in zs:
        for zb in zs:
            out.append((A, za, B, zb))
            out.append((D, za, A, zb))
    z1, z2 = rng.randrange(2, p), rng.randrange(2, p)
    A2 = C.add(A, A)
    for za, zb in ((1, 1), (z1, z2), (p - 1, z1), (z2, 1), (z1, p - 1)):
        out.append((A, za, A, zb))          # P + P
        out.append((A, za, C.neg(A), zb))   # P + (-P)
        out.append((A, za, A2, zb))         # P + 2P
        out.append((A2, za, A, zb))
    out = [c + (None, None) for c in out]
    junk = (rng.randrange(1, p), rng.randrange(1, p))
    for xy in (None, junk):
        for zb in zs:
            out.append((None, 0, B, zb, xy, None))  # identity + P
        if q_identity:
            for za in zs:
                out.append((A, za, None, 0, None, xy))  # P + identity
        if both_identity:
            out.append((None, 0, None, 0, xy, xy))
            out.append((None, 0, None, 0, xy, None))
    return out


@functools.lru_cache(maxsize=None)
def group_records():
    recs = []
    bnc = CURVES["bn"]
    # op, curve, P's form, Q's form, Q may be the identity, both may be
    forms = {"J": jac_words, "X": xyzz_words}
    table = [("g1j_add_affine", "bn", "J", "A", True), ("g1j_add", "bn", "J", "J", True),
             ("madd_inl", "bn", "J", "A", False), ("add_inl", "bn", "J", "J", True),
             ("xmadd_inl", "bn", "X", "A", False), ("xadd_inl", "bn", "X", "X", True),
             ("p256_pj_add", "p256", "J", "J", True), ("p256_pj_madd", "p256", "J", "A", False),
             ("fbn_pj_add", "fbn", "J", "J", True), ("fbn_pj_madd", "fbn", "J", "A", False)]
    for op, cn, fp_, fq, qid in table:
        C = CURVES[cn]
        kind = "xyzz" if fp_ == "X" else "jac:" + cn
        for P, zp, Q, zq, xyp, xyq in add_cases(C, _seed(op), qid, qid):
            if fq == "A":
                qw = aff_words(C, Q)  # an affine operand has no denominator: zq unused
            else:
                qw = forms[fq](C, Q, zq, xyq)
            recs.append((op, forms[fp_](C, P, zp, xyp) + qw, kind, C.add(P, Q)))
    # doublings
    for op, cn, form in (("g1j_dbl", "bn", "J"), ("g1x_dbl", "bn", "X"), ("p256_pj_dbl", "p256", "J"),
                         ("fbn_pj_dbl", "fbn", "J")):
        C = CURVES[cn]
        pts, rng = _points(C, _seed(op))
        kind = "xyzz" if form == "X" else "jac:" + cn
        for P in pts + [C.gen]:
            for z in (1, C.p - 1, rng.randrange(2, C.p)):
                recs.append((op, forms[form](C, P, z), kind, C.add(P, P)))
        junk = (rng.randrange(1, C.p), rng.randrange(1, C.p))
        recs.append((op, forms[form](C, None, 0), kind, None))
        recs.append((op, forms[form](C, None, 0, junk), kind, None))
    # g1j_dbl's y == 0 branch (no such point on the curve): the identity
    recs.append(("g1j_dbl", [to_mont(5, bn.P), 0, to_mont(7, bn.P)], "jac:bn", None))
    # conversions
    pts, rng = _points(bnc, 77)
    for P in pts + [bnc.gen]:
        for z in (1, bn.P - 1, rng.randrange(2, bn.P)):
            recs.append(("g1j_to_affine", jac_words(bnc, P, z), "raw", aff_words(bnc, P)))
            recs.append(("g1x_to_jac", xyzz_words(bnc, P, z), "jac:bn", P))
    junk = (rng.randrange(1, bn.P), rng.randrange(1, bn.P))
    for xy in (None, junk):
        recs.append(("g1j_to_affine", jac_words(bnc, None, 0, xy), "raw", [0, 0]))
        recs.append(("g1x_to_jac", xyzz_words(bnc, None, 0, xy), "jac:bn", None))
    # equality of Jacobian points as group elements
    A, B, _ = pts
    zs = [1, bn.P - 1, rng.randrange(2, bn.P), rng.randrange(2, bn.P)]
    for za in zs:
        for zb in zs:
            recs.append(("g1j_eq", jac_words(bnc, A, za) + jac_words(bnc, A, zb), "raw", [1]))
            recs.append(("g1j_eq", jac_words(bnc, A, za) + jac_words(bnc, bnc.neg(A), zb), "raw", [0]))
            recs.append(("g1j_eq", jac_words(bnc, A, za) + jac_words(bnc, B, zb), "raw", [0]))
    for xy1 in (None, junk):
        for xy2 in (None, junk, (junk[1], junk[0])):
            recs.append(("g1j_eq", jac_words(bnc, None, 0, xy1) + jac_words(bnc, None, 0, xy2), "raw", [1]))
        for z in zs[:3]:
            recs.append(("g1j_eq", jac_words(bnc, None, 0, xy1) + jac_words(bnc, A, z), "raw", [0]))
            recs.append(("g1j_eq", jac_words(bnc, A, z) + jac_words(bnc, None, 0, xy1), "raw", [0]))
    # curve membership of affine Montgomery coordinates
    for cn in ("p256", "fbn"):
        C = CURVES[cn]
        pts, rng = _points(C, _seed(cn) + 9)
        cand = []
        for P in pts + [C.gen]:
            cand += [P, C.neg(P), (P[0], (P[1] + 1) % C.p), ((P[0] + 1) % C.p, P[1]), (P[1], P[0])]
        cand += [(0, 0), (C.p - 1, C.p - 1), (0, 1), (1, 0)] + \
                [(rng.randrange(C.p), rng.randrange(C.p)) for _ in range(16)]
        for x, y in cand:
            want = int((y * y - x ** 3 - C.a * x - C.b) % C.p == 0)
            recs.append((cn + "_on_curve", [to_mont(x, C.p), to_mont(y, C.p)], "raw", [want]))
    return recs


MAGS = [0, 1, (1 << 127) - 1, 0x7fff << 112, int("08" + "8" * 30, 16), int("7" + "9" * 31, 16)]


@functools.lru_cache(maxsize=None)
def scalar_records():
    recs = []
    C = CURVES["bn"]
    rng = random.Random(4242)
    lam = glv_lambda("bn")
    bases = [C.gen, C.mul(rng.randrange(1, bn.R), C.gen), C.mul(rng.randrange(1, bn.R), C.gen)]
    ks = scalars(bn.R, lam, 31)
    for P in bases:
        for k in ks:
            want = bn.g1_mul(P, k) if k else None
            recs.append(("var_base_mul", aff_words(C, P) + [k], "jac:bn", want))
            recs.append(("glv_mul", aff_words(C, P) + [k], "jac:bn", want))
    for k in ks[:20]:
        recs.append(("var_base_mul", [0, 0, k], "jac:bn", None))
    mags = MAGS + [rng.randrange(1 << 127) for _ in range(24)]
    zs = [1, bn.P - 1, rng.randrange(2, bn.P)]
    for i, P in enumerate(bases):
        for j, m in enumerate(mags):
            z = zs[(i + j) % 3]
            recs.append(("vb128j", jac_words(C, P, z) + [m], "jac:bn", bn.g1_mul(P, m) if m else None))
    recs.append(("vb128j", jac_words(C, None, 0) + [mags[7]], "jac:bn", None))
    A, B = bases[1], bases[2]
    pairs = [(a, b) for a in MAGS for b in MAGS] + [(rng.randrange(1 << 127), rng.randrange(1 << 127)) for _ in range(24)]
    for j, (a, b) in enumerate(pairs):
        want = C.add(bn.g1_mul(A, a) if a else None, bn.g1_mul(B, b) if b else None)
        recs.append(("straus2_128", jac_words(C, A, zs[j % 3]) + [a] + jac_words(C, B, zs[(j + 1) % 3]) + [b],
                     "jac:bn", want))
    for a, b in pairs[-8:] + [(1, 1), (MAGS[2], MAGS[2])]:
        # Q = P, Q = -P and identity operands: the exceptional branches inside the chain
        for Q, z in ((A, zs[2]), (C.neg(A), zs[1]), (None, 0)):
            want = C.add(bn.g1_mul(A, a) if a else None, bn.g1_mul(Q, b) if (b and Q) else None)
            recs.append(("straus2_128", jac_words(C, A, zs[0]) + [a] + jac_words(C, Q, z) + [b], "jac:bn", want))
        want = bn.g1_mul(B, b) if b else None
        recs.append(("straus2_128", jac_words(C, None, 0) + [a] + jac_words(C, B, zs[2]) + [b], "jac:bn", want))
    return recs


# fbn::glv_mul_tab (fbn_glv.hpp, the FP256BN nym kernels' variable-base product): the
# scalars by the property each has under glv_decompose.  The chain recodes |k1| and |k2|
# into 33 signed 4-bit windows, the 33rd taking a carry out of nibble 31.  No k < r sends
# one there: |k1| <= (A1 + A2) / 2 and |k2| <= (NB1 + A1) / 2, both 0x7fffffffffff3c33...
# < 2^127, so nibble 31 is at most 7 and 7 + carry = 8 is kept as the digit +8.  A
# magnitude whose nibbles are all 0xf does not exist (fbn_glv_search(0): no k among 10^6
# seeded draws has 0xf in nibble 31 either), so in its place stand the two closest:
# nibble 31 = 7 over the longest run of 0xf below it, which carries all the way up to
# that digit +8.
FBN_GLV_KS = [
    (0, "zero: the identity"),
    (1, "k1 = 1, k2 = 0"),
    (2, "k1 = 2, k2 = 0"),
    ("r-1", "k1 = -1, k2 = 0"),
    ("lam", "k1 = 0, k2 = 1: phi(Q) alone"),
    ("lam-1", "k1 = -1, k2 = 1"),
    (0xaae8812bd2a9068a982e5c91f91ecb2b62bcfc1ea1b66a0cc3a24c99162c17a8,
     "|k1| = 0x7ffff1...: the longest run of 0xf below nibble 31 = 7 in random.Random(128)'s first 10^6 "
     "draws below r (fbn_glv_search(1)); k1 < 0 < k2"),
    (0x7fffffffffff00000000000000000000,
     "k1 = k, k2 = 0, eleven 0xf below nibble 31 = 7: the longest such run with k2 = 0 (constructed, no draw)"),
    (5 << 100, "k2 = 0 with k1 of 103 bits: windows 26..32 of k1 and all of k2 are zero"),
]


def fbn_glv_search(below):
    """the seeded search behind FBN_GLV_KS (seconds; not run by any test): the draw with the
    longest run of 0xf nibbles of |k1| from nibble 31 - below downwards, nibble 31 largest first"""
    hdr, st, r, _ = GLV_SETS["fbn"]
    c = header_consts(hdr, st)
    rng = random.Random(128)
    best = (-1, -1, None)
    for _ in range(10 ** 6):
        k = rng.randrange(r)
        key = _f_run(abs(glv_decompose(k, c)[0]), below)
        if key > best[:2]:
            best = key + (k,)
    return best


def _f_run(mag, below):
    n, i = 0, 31 - below
    while i >= 0 and (mag >> (4 * i)) & 15 == 15:
        n, i = n + 1, i - 1
    return (mag >> 124 if below else 0, n)


def fbn_glv_scalars():
    r, lam = OI.FP256BNC.r, glv_lambda("fbn")
    named = {"r-1": r - 1, "lam": lam, "lam-1": lam - 1}
    rng = random.Random(33)
    return [named.get(k, k) for k, _ in FBN_GLV_KS] + [rng.randrange(r) for _ in range(8)]


@functools.lru_cache(maxsize=None)
def fbn_glv_records():
    """operands Qx Qy (affine Montgomery, on the curve) and k < r; want: the oracle's k * Q"""
    F, C = OI.FP256BNC, CURVES["fbn"]
    recs = []
    for P in (C.gen, F.mul((1, 2), 0x1f2e3d4c5b6a79880123456789abcdef)):
        for k in fbn_glv_scalars():
            recs.append(("fbn_glv_mul", aff_words(C, P) + [k], "jac:fbn", F.mul(P, k) if k else None))
    return recs


# ------------------------------------------------------------------------ tower
def _tower(tag):
    from oracle import pairing as PR, pairing_tower as PT
    return PT.Tower(PR.BN254 if tag == "bn" else PR.FP256BN)


def f2_elems(p, rng, n=32):
    e = [(0, 0), (1, 0), (0, 1), (p - 1, 0), (0, p - 1), (p - 1, p - 1), (1, p - 1), (p - 1, 1)]
    return e + [(rng.randrange(p), rng.randrange(p)) for _ in range(n - len(e))]


def tower_elems(p, rng, nc, n=32):
    """n elements of nc Fp2 coefficients: 0, 1, one non-zero coefficient each, all coefficients
    M-1, one coefficient M-1, and random ones"""
    Z = (0, 0)
    out = [[Z] * nc, [(1, 0)] + [Z] * (nc - 1), [(p - 1, p - 1)] * nc]
    for i in range(nc):
        c = (rng.randrange(p), rng.randrange(p))
        out.append([c if j == i else Z for j in range(nc)])
    for i in range(nc):
        out.append([(p - 1, p - 1) if j == i else (rng.randrange(p), rng.randrange(p)) for j in range(nc)])
    while len(out) < n:
        out.append([(rng.randrange(p), rng.randrange(p)) for _ in range(nc)])
    return out[:n]


def _t6(z):
    return tuple(z)


def _t12(z):
    return (tuple(z[:3]), tuple(z[3:]))


def _flat(p, *els):
    """Montgomery words of Fp2 coefficients in struct order"""
    out = []
    for e in els:
        for a, b in e:
            out += [to_mont(a, p), to_mont(b, p)]
    return out


def _l6(a):
    return list(a)


def _l12(a):
    return list(a[0]) + list(a[1])


def t12_pow(T, a, e):
    r = T.one()
    for bit in bin(e)[2:]:
        r = T.m12(r, r)
        if bit == "1":
            r = T.m12(r, a)
    return r


def embed_line(T, lam, mu, xP, yP):
    """the line as a dense Fp12 element, placed as device/pairing.hpp's header comment says:
    D-type l = yP + (-lam xP) w + mu v w; M-type l w^3 = mu + (-lam xP) v + yP v w"""
    Z = (0, 0)
    A = T.n2(T.sc2(lam, xP))
    if T.C.twist == "M":
        return ((mu, A, Z), (Z, (yP, 0), Z))
    return (((yP, 0), Z, Z), (A, mu, Z))


@functools.lru_cache(maxsize=None)
def tower_records():
    recs = []
    for tag in ("bn", "fbn"):
        T = _tower(tag)
        p = T.p
        rng = random.Random(_seed(tag) + 1000)
        R = lambda op, ins, want: recs.append((tag + "_" + op, ins, "raw", want))  # noqa: E731
        e2, f2 = f2_elems(p, rng), f2_elems(p, rng)
        rng.shuffle(f2)
        for a, b in zip(e2, f2):
            R("f2_mul", _flat(p, [a, b]), _flat(p, [T.m2(a, b)]))
        for a in e2:
            R("f2_sqr", _flat(p, [a]), _flat(p, [T.m2(a, a)]))
            R("f2_inv", _flat(p, [a]), _flat(p, [T.inv2(a)]))
            R("f2_mul_xi", _flat(p, [a]), _flat(p, [T.m2(a, tuple(T.C.xi))]))
        e6, g6 = tower_elems(p, rng, 3), tower_elems(p, rng, 3)
        rng.shuffle(g6)
        Z = (0, 0)
        for a, b in zip(e6, g6):
            R("f6_mul", _flat(p, a, b), _flat(p, _l6(T.m6(_t6(a), _t6(b)))))
            R("f6_mul01", _flat(p, a, b[:2]), _flat(p, _l6(T.m6(_t6(a), (b[0], b[1], Z)))))
        for a in e6:
            R("f6_mul_v", _flat(p, a), _flat(p, _l6(T.m6(_t6(a), (Z, (1, 0), Z)))))
            R("f6_inv", _flat(p, a), _flat(p, _l6(T.inv6(_t6(a)))))
        e12, g12 = tower_elems(p, rng, 6), tower_elems(p, rng, 6)
        rng.shuffle(g12)
        for a, b in zip(e12, g12):
            R("f12_mul", _flat(p, a, b), _flat(p, _l12(T.m12(_t12(a), _t12(b)))))
        for a in e12:
            ta = _t12(a)
            R("f12_sqr", _flat(p, a), _flat(p, _l12(T.m12(ta, ta))))
            R("f12_inv", _flat(p, a), _flat(p, _l12(T.inv12(ta))))
            R("f12_conj", _flat(p, a), _flat(p, _l12((ta[0], T.n6(ta[1])))))
            x = ta
            for n in (1, 2, 3):  # a^(p^n) = (a^(p^(n-1)))^p, square-and-multiply with m12
                x = t12_pow(T, x, p)
                R("f12_frob%d" % n, _flat(p, a), _flat(p, _l12(x)))
            # cyclotomic input: f^(p^6 - 1) = conj(f) / f, then times its p^2-th power
            if any(c != Z for c in a):
                g = T.m12(T.cj12(ta), T.inv12(ta))
                g = T.m12(T.frob(g, 2), g)
            else:
                g = T.one()
            R("f12_cyc_sqr", _flat(p, _l12(g)), _flat(p, _l12(T.m12(g, g))))
        for a, (lam, mu) in zip(e12, zip(f2_elems(p, rng), reversed(f2_elems(p, rng)))):
            xP, yP = rng.randrange(p), rng.randrange(p)
            want = T.m12(_t12(a), embed_line(T, lam, mu, xP, yP))
            R("line_mul", _flat(p, a, [lam, mu]) + [to_mont(xP, p), to_mont(yP, p)], _flat(p, _l12(want)))
    return recs


def all_records():
    return field_records() + glv_records() + group_records() + scalar_records() + tower_records()


def format_records(recs):
    return "".join("%s %s\n" % (op, " ".join("%x" % w for w in ins)) for op, ins, _, _ in recs)


def parse_results(text):
    return [[int(w, 16) for w in line.split()] for line in text.splitlines()]
