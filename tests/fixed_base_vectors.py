"""Vectors for the fixed-base code of device/fixed_base.hpp, as lib/arith_check runs
it (ops listed by `arith_check --list-fb`):

  fb_digits_16 / _w16 / _20 / _22    the NW signed digits and the carry out of a scalar
                       (fb_next_digit, fb_next_digit_w<W>), called as the products call them
  fb_sum_W, fb_mul_W   fb_sum_w<W> (XYZZ), fb_mul_w<W> (Jacobian), W = 16, 20, 22
  fb_mul2              ka A + kb B over two 16-bit tables; fb_mul2_same and fb_mul2_neg:
                       the same function with B's table a table of A, resp. of -A
  fb_mul_acc, fb_mul_acc_jac    acc += k B over a 16-bit table

The tool does no arithmetic: a product's record carries, after its device operands,
for each table and window the entry this file's integer recoding selects -- |d| and
the affine Montgomery point |d| 2^(W w) B, or 0 0 0 for a zero digit.  The tool
scatters them into a table of the production size that is otherwise 0xFF bytes
(guard windows included), so a device whose digit or index differs from the integer
recoding reads poison.  Expectations are k B by oracle/bn254.py's g1_mul on the whole
scalar: they do not go through the digits.

The scalars (`scalars(W)`) sit on the recoding's edges at every window: the digits 0,
+-1, E - 1, E (kept positive: the last entry of a window), -(E - 1) (from E + 1, the
first that carries), the two-level build's seam S - 1, S, S + 1, 2S, the top window's
maximum (from r - 1), carry chains 2^(W j) - 1 and all-E digits, and single entries
2^(W j).  tests/test_fixed_base_vectors_cpu.py recodes every vector and asserts that
each class is reached at every width; tests/test_gpu_fixed_base.py runs them.

Records have the shape of com_chain_vectors': (op, words, result kind, expected, tag)."""
import random

from oracle import bn254 as bn

import arith_vectors as AV

C = AV.CURVES["bn"]
WIDTHS = (16, 20, 22)


def cfg(W):
    """NW windows, E entries per window, S small multiples (FbCfg<W>)"""
    return (255 + W - 1) // W, 1 << (W - 1), 1 << (W // 2)


def recode(k, W):
    """the signed digits of k, least significant first, and the carry out: digit =
    window + carry in, and a digit above E becomes digit - 2E with a carry"""
    NW, E, _ = cfg(W)
    ds, carry = [], 0
    for _ in range(NW):
        d = (k & (2 * E - 1)) + carry
        k >>= W
        carry = int(d > E)
        ds.append(d - 2 * E if carry else d)
    return ds, carry


def from_digits(ds, W):
    return sum(d << (W * w) for w, d in enumerate(ds))


def top_max(W):
    return recode(bn.R - 1, W)[0][-1]


def edge_digits(W):
    _, E, S = cfg(W)
    return [0, 1, -1, E - 1, E, -(E - 1), S - 1, S, S + 1, 2 * S]


_SCALARS = {}


def scalars(W):
    """[(tag, k)], k < r, in a fixed order"""
    if W in _SCALARS:
        return _SCALARS[W]
    NW, E, S = cfg(W)
    rng = random.Random(0xFB00 + W)
    tmax = top_max(W)

    def rand_digits():
        # any digit string with entries in (-E, E] below a positive top digit is the
        # recoding of its own sum; top <= tmax - 2 keeps the sum below r
        return [rng.randrange(-(E - 1), E + 1) for _ in range(NW - 1)] + [rng.randrange(1, tmax - 1)]

    out = []
    for w in range(NW - 1):
        for t in edge_digits(W):
            ds = rand_digits()
            ds[w] = t
            out.append(("w%d_d%d" % (w, t), from_digits(ds, W)))
    # the top window: its maximum (r - 1), 0 (the digit below positive, so k > 0) and 1
    out.append(("top_max", bn.R - 1))
    for t in (0, 1):
        ds = rand_digits()
        ds[NW - 1] = t
        ds[NW - 2] = rng.randrange(1, E + 1)
        out.append(("top_%d" % t, from_digits(ds, W)))
    # carry chains: 2^(W j) - 1 is -1, then j - 1 zero digits made by carries, then 1
    for j in range(1, NW):
        out.append(("chain_%d" % j, (1 << (W * j)) - 1))
    out.append(("all_E", from_digits([E] * (NW - 1) + [0], W)))
    out.append(("all_E_top", from_digits([E] * (NW - 1) + [tmax - 1], W)))
    # the first digit that carries, in every window at once
    out.append(("all_E1", from_digits([E + 1] * (NW - 1) + [0], W)))
    # one entry, no addition
    for j in range(NW):
        out.append(("single_%d" % j, 1 << (W * j)))
    out += [("zero", 0), ("one", 1), ("r_minus_2W", bn.R - (1 << W))]
    out += [("random_%d" % i, rng.randrange(bn.R)) for i in range(32)]
    assert all(0 <= k < bn.R for _, k in out)
    _SCALARS[W] = out
    return out


# ------------------------------------------------------------------- tables
_BASES = {}
_ENTRIES = {}


def base(name):
    """the bases of the sparse tables: one point per name, fixed"""
    if name not in _BASES:
        if name.startswith("-"):
            _BASES[name] = bn.g1_neg(base(name[1:]))
        else:
            _BASES[name] = bn.g1_mul(bn.GEN, random.Random("fb base " + name).randrange(1, bn.R))
    return _BASES[name]


def mul(name, k):
    """k B of base `name`, from the whole scalar"""
    key = (name, k % bn.R)
    if key not in _ENTRIES:
        _ENTRIES[key] = bn.g1_mul(base(name), k)
    return _ENTRIES[key]


def entry(name, W, w, ad):
    """T[w][ad - 1] = ad 2^(W w) B of base `name` (affine), 1 <= ad <= E"""
    key = (name, W, w, ad)
    if key not in _ENTRIES:
        wb = (name, W, w, 0)  # the window's base 2^(W w) B
        if wb not in _ENTRIES:
            _ENTRIES[wb] = bn.g1_mul(base(name), 1 << (W * w))
        _ENTRIES[key] = bn.g1_mul(_ENTRIES[wb], ad)
    return _ENTRIES[key]


def entry_words(name, W, k):
    """the 3 NW words |d| x y of the entries k selects in base `name`'s table"""
    ds, carry = recode(k, W)
    assert carry == 0
    ws = []
    for w, d in enumerate(ds):
        ws += [abs(d)] + AV.aff_words(C, entry(name, W, w, abs(d))) if d else [0, 0, 0]
    return ws


# ------------------------------------------------------------------ records
def _u32(d):
    return d & 0xFFFFFFFF


def s32(w):
    """a digit word as the int the device stored"""
    assert w < (1 << 32)
    return w - (1 << 32) if w >> 31 else w


DIGIT_OPS = {"fb_digits_16": 16, "fb_digits_w16": 16, "fb_digits_20": 20, "fb_digits_22": 22}


def digit_records():
    recs = []
    for op, W in DIGIT_OPS.items():
        for tag, k in scalars(W):
            ds, carry = recode(k, W)
            recs.append((op, [k], "raw", [_u32(d) for d in ds] + [carry], tag))
    return recs


def product_records():
    """fb_sum_w<W> and fb_mul_w<W> on every scalar of their width"""
    recs = []
    for W in WIDTHS:
        name = "B%d" % W
        for tag, k in scalars(W):
            want = mul(name, k)
            ent = entry_words(name, W, k)
            recs.append(("fb_sum_%d" % W, [k] + ent, "xyzz", want, tag))
            recs.append(("fb_mul_%d" % W, [k] + ent, "jac:bn", want, tag))
    return recs


def mul2_records():
    """fb_mul2: generic pairs of the 16-bit scalars over tables of A and B; then the second
    table a table of A with ka = kb (the second addition of the first non-zero window meets
    the accumulator's own point: the doubling branch, in every window across the records)
    and a table of -A (that addition gives the identity, and the later windows start from
    it again), each also with scalars that differ only above the lowest windows"""
    W = 16
    NW, E, _ = cfg(W)
    sc = scalars(W)
    rng = random.Random(0xFB02)
    recs = []
    for i, (tag, ka) in enumerate(sc):
        tb, kb = sc[(7 * i + 3) % len(sc)]
        want = bn.g1_add(mul("A", ka), mul("B", kb))
        recs.append(("fb_mul2", [ka, kb] + entry_words("A", W, ka) + entry_words("B", W, kb), "jac:bn", want,
                     tag + "+" + tb))
    for op, other, sign in (("fb_mul2_same", "A", 1), ("fb_mul2_neg", "-A", -1)):
        ks = []
        for j in range(NW):  # the first non-zero digit at window j
            ds = [0] * j + [rng.randrange(-(E - 1), E + 1) or 1 for _ in range(NW - 1 - j)] + [rng.randrange(1, 1000)]
            ks.append(("first_%d" % j, from_digits(ds, W)))
        ks += [(t, k) for t, k in sc if t in ("one", "top_max", "all_E", "all_E1", "chain_3", "random_0", "random_1")]
        for tag, k in ks:
            want = bn.g1_mul(base("A"), (1 + sign) * k)
            recs.append((op, [k, k] + entry_words("A", W, k) + entry_words(other, W, k), "jac:bn", want, "eq_" + tag))
        for j in (1, 2, NW - 1):  # equal digits below window j, then different ones
            ka = rng.randrange(bn.R >> 1)
            kb = (ka % (1 << (W * j))) + (rng.randrange(1 << 200) >> (W * j) << (W * j))
            want = bn.g1_mul(base("A"), ka + sign * kb)
            recs.append((op, [ka, kb] + entry_words("A", W, ka) + entry_words(other, W, kb), "jac:bn", want,
                         "low_eq_%d" % j))
    return recs


ACC_KINDS = ("identity", "neg_kB", "kB", "first_entry", "neg_first_entry", "random")


def acc_records():
    """fb_mul_acc (XYZZ sum, one full addition) and fb_mul_acc_jac (every entry added into
    the Jacobian accumulator): every 16-bit scalar with a random accumulator; a sample with
    the accumulator the identity, -(k B) (the last addition gives the identity), k B (the
    full addition doubles), the first entry the product adds (fb_mul_acc_jac's first addition
    doubles) and its negative (its first addition gives the identity)"""
    W = 16
    sc = scalars(W)
    rng = random.Random(0xFB03)
    sample = [(t, k) for t, k in sc if t in ("w0_d1", "w0_d%d" % (1 << 15), "w3_d-1", "w5_d%d" % -((1 << 15) - 1),
                                            "top_max", "chain_2", "all_E", "single_0", "single_4", "one", "random_0",
                                            "random_1")]
    assert len(sample) == 12
    recs = []

    def rec(tag, k, kind):
        ds, _ = recode(k, W)
        first = next(((w, d) for w, d in enumerate(ds) if d), None)
        fe = None
        if first:
            fe = entry("B16", W, first[0], abs(first[1]))
            fe = bn.g1_neg(fe) if first[1] < 0 else fe
        kB = mul("B16", k)
        acc = {"identity": None, "neg_kB": bn.g1_neg(kB), "kB": kB, "first_entry": fe, "neg_first_entry": bn.g1_neg(fe),
               "random": bn.g1_mul(bn.GEN, rng.randrange(1, bn.R))}[kind]
        z = rng.randrange(2, bn.P)
        xy = (rng.randrange(bn.P), rng.randrange(bn.P))  # an identity's x, y are arbitrary
        ins = AV.jac_words(C, acc, z, xy) + [k] + entry_words("B16", W, k)
        for op in ("fb_mul_acc", "fb_mul_acc_jac"):
            recs.append((op, ins, "jac:bn", bn.g1_add(acc, kB), "%s:%s" % (kind, tag)))

    for tag, k in sc:
        rec(tag, k, "random")
    for tag, k in sample + [("zero", 0)]:
        for kind in ACC_KINDS[:-1]:
            rec(tag, k, kind)
    return recs


ARITY = {}
for _op, _W in DIGIT_OPS.items():
    ARITY[_op] = (1, cfg(_W)[0] + 1)
for _W in WIDTHS:
    ARITY["fb_sum_%d" % _W] = (1 + 3 * cfg(_W)[0], 4)
    ARITY["fb_mul_%d" % _W] = (1 + 3 * cfg(_W)[0], 3)
for _op in ("fb_mul2", "fb_mul2_same", "fb_mul2_neg"):
    ARITY[_op] = (2 + 2 * 3 * 16, 3)
for _op in ("fb_mul_acc", "fb_mul_acc_jac"):
    ARITY[_op] = (4 + 3 * 16, 3)

_CACHE = {}


def all_records():
    """computed once per process (a few thousand short oracle products)"""
    if "all" not in _CACHE:
        _CACHE["all"] = digit_records() + product_records() + mul2_records() + acc_records()
    return _CACHE["all"]


def format_records(recs):
    return AV.format_records([r[:4] for r in recs])
