"""CPU: the vectors tests/test_gpu_fixed_base.py feeds to lib/arith_check
(tests/fixed_base_vectors.py) are consistent with the oracle's integers on their own
and reach every class of digit the recoding and the table consumers have an edge at,
at every window of every width.  The recoding's invariants (sum d_w 2^(W w) = k,
|d_w| <= E, no carry out for k < r) hold for every vector in integers, so that a
device that differs from it is the device's finding.  `arith_check --list-fb` (no
device) names the ops with the arities the vectors use, and the tool refuses records
that break a table's contract before it launches anything."""
import os
import subprocess

import pytest

from conftest import ROOT

from oracle import bn254 as bn

import arith_vectors as AV
import fixed_base_vectors as FV

EXE = os.path.join(ROOT, "fabric-token-sdk_amd", "lib", "arith_check")


def _aff(x, y):
    return (AV.from_mont(x, bn.P), AV.from_mont(y, bn.P))


def test_list_fb_names_the_ops():
    out = subprocess.run([EXE, "--list-fb"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = {n: (int(a), int(b)) for n, a, b in (l.split() for l in out.stdout.splitlines())}
    assert got == FV.ARITY
    # the primitives' catalogue and the chain's are listed apart and unchanged
    for flag in ("--list", "--list-chain"):
        out = subprocess.run([EXE, flag], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and not set(FV.ARITY) & {l.split()[0] for l in out.stdout.splitlines()}
    assert {r[0] for r in FV.all_records()} == set(FV.ARITY)


def test_window_constants_match_the_header():
    """FbCfg<W> as device/fixed_base.hpp states it, and the top window's range for k < r"""
    with open(os.path.join(AV.DEVICE, "fixed_base.hpp")) as f:
        src = f.read()
    for line in ("static constexpr int NW = (255 + W - 1) / W;", "static constexpr int E = 1 << (W - 1);",
                 "static constexpr int S = 1 << (W / 2);", "constexpr int FB_W = 16;"):
        assert line in src, line
    assert [FV.cfg(W) for W in FV.WIDTHS] == [(16, 1 << 15, 1 << 8), (13, 1 << 19, 1 << 10), (12, 1 << 21, 1 << 11)]
    assert [FV.top_max(W) for W in FV.WIDTHS] == [12388, 12388, 3097]
    for W in FV.WIDTHS:
        NW, E, _ = FV.cfg(W)
        # the largest top digit any k < r has, with the largest carry into it
        assert ((bn.R - 1) >> (W * (NW - 1))) + 1 <= E


@pytest.mark.parametrize("W", FV.WIDTHS)
def test_scalars_reach_every_digit_class(W):
    NW, E, S = FV.cfg(W)
    sc = dict(FV.scalars(W))
    assert len(sc) == len(FV.scalars(W))  # tags are unique
    seen = [set() for _ in range(NW)]
    carries_in = [set() for _ in range(NW)]
    for tag, k in sc.items():
        assert 0 <= k < bn.R
        ds, carry = FV.recode(k, W)
        assert carry == 0 and FV.from_digits(ds, W) == k and all(-E < d <= E for d in ds), tag
        c = 0
        for w, d in enumerate(ds):
            seen[w].add(d)
            carries_in[w].add(c)
            c = int(((k >> (W * w)) & (2 * E - 1)) + c > E)
    for w in range(NW - 1):
        for t in FV.edge_digits(W):
            assert FV.recode(sc["w%d_d%d" % (w, t)], W)[0][w] == t
        assert set(FV.edge_digits(W)) <= seen[w]
        # E stays positive (raw window E, no carry in; and E - 1 with a carry in), E + 1 carries
        assert (sc["w%d_d%d" % (w, E)] >> (W * w)) & (2 * E - 1) in (E, E - 1)
        assert carries_in[w + 1] == {0, 1}
    assert {0, 1, FV.top_max(W)} <= seen[NW - 1] and max(seen[NW - 1]) == FV.top_max(W) and min(seen[NW - 1]) == 0
    # carry chains: -1, zeros made by a carry into an all-ones window, then 1
    for j in range(1, NW):
        ds, _ = FV.recode(sc["chain_%d" % j], W)
        assert ds == [-1] + [0] * (j - 1) + [1] + [0] * (NW - 1 - j)
    assert FV.recode(sc["all_E"], W)[0] == [E] * (NW - 1) + [0]
    assert FV.recode(sc["all_E1"], W)[0] == [-(E - 1)] + [-(E - 2)] * (NW - 2) + [1]
    for j in range(NW):
        assert FV.recode(sc["single_%d" % j], W)[0] == [0] * j + [1] + [0] * (NW - 1 - j)
    assert sc["zero"] == 0 and sc["one"] == 1 and sc["top_max"] == bn.R - 1 and sc["r_minus_2W"] == bn.R - (1 << W)
    assert sum(t.startswith("random_") for t in sc) == 32
    # E reached with no carry in (the raw window is E) at every window below the top
    for w in range(NW - 1):
        assert any((k >> (W * w)) & (2 * E - 1) == E and FV.recode(k, W)[0][w] == E for k in sc.values())


def _entries(words, W):
    """[(|d|, point or None)] per window of one table's 3 NW words"""
    NW = FV.cfg(W)[0]
    assert len(words) == 3 * NW
    out = []
    for w in range(NW):
        ad, x, y = words[3 * w:3 * w + 3]
        out.append((ad, _aff(x, y) if ad else None))
        assert ad or (x, y) == (0, 0)
    return out


_WINDOW_BASE, _CHECKED = {}, set()


def _table_sum(words, W, k, B):
    """sum of the supplied entries with the recoding's signs; every entry is |d| (2^(W w) B),
    recomputed here once per position"""
    ds, _ = FV.recode(k, W)
    acc = None
    for w, ((ad, pt), d) in enumerate(zip(_entries(words, W), ds)):
        assert ad == abs(d) and ad <= FV.cfg(W)[1]
        if d:
            if (B, W, w) not in _WINDOW_BASE:
                _WINDOW_BASE[(B, W, w)] = bn.g1_mul(B, 1 << (W * w))
            if (B, W, w, ad, pt) not in _CHECKED:
                assert pt == bn.g1_mul(_WINDOW_BASE[(B, W, w)], ad)
                _CHECKED.add((B, W, w, ad, pt))
            acc = bn.g1_add(acc, pt if d > 0 else bn.g1_neg(pt))
    return acc


def test_records_are_self_consistent():
    """every expectation (k B from the whole scalar) is the signed sum of the entries the
    record supplies, each of which is |d| 2^(W w) B; no two records of an op place different
    points at one position; digit records restate the integer recoding"""
    by = {}
    for r in FV.all_records():
        by.setdefault(r[0], []).append(r)
    for op, W in FV.DIGIT_OPS.items():
        assert [r[1][0] for r in by[op]] == [k for _, k in FV.scalars(W)]
        for _, (k,), kind, want, _ in by[op]:
            assert kind == "raw" and ([FV.s32(x) for x in want[:-1]], want[-1]) == FV.recode(k, W)
    placed = {}

    def place(op, t, W, words):
        for w, (ad, pt) in enumerate(_entries(words, W)):
            if ad:
                assert placed.setdefault((op, t, w, ad), pt) == pt

    for W in FV.WIDTHS:
        B = FV.base("B%d" % W)
        for op, kind in (("fb_sum_%d" % W, "xyzz"), ("fb_mul_%d" % W, "jac:bn")):
            assert [r[1][0] for r in by[op]] == [k for _, k in FV.scalars(W)]
            for _, ins, knd, want, tag in by[op][::7 if op.startswith("fb_mul") else 1]:
                assert knd == kind and _table_sum(ins[1:], W, ins[0], B) == want, (op, tag)
            for r in by[op]:
                place(op, 0, W, r[1][1:])
    A, B = FV.base("A"), FV.base("B")
    for op, other in (("fb_mul2", B), ("fb_mul2_same", A), ("fb_mul2_neg", bn.g1_neg(A))):
        for _, ins, _, want, tag in by[op][::5 if op == "fb_mul2" else 1]:
            assert bn.g1_add(_table_sum(ins[2:50], 16, ins[0], A), _table_sum(ins[50:], 16, ins[1], other)) == want, tag
        for r in by[op]:
            place(op, 0, 16, r[1][2:50])
            place(op, 1, 16, r[1][50:])
    B = FV.base("B16")
    for op in ("fb_mul_acc", "fb_mul_acc_jac"):
        for _, ins, _, want, tag in by[op][::5]:
            acc = AV.norm_jac(FV.C, ins[:3])
            assert bn.g1_add(acc, _table_sum(ins[4:], 16, ins[3], B)) == want, tag
        for r in by[op]:
            place(op, 0, 16, r[1][4:])


def test_exceptional_branches_are_present():
    by = {}
    for r in FV.all_records():
        by.setdefault(r[0], []).append(r)
    W, NW = 16, 16
    # fb_mul2 over a table of the same base, ka = kb: the first non-zero window's second
    # addition doubles, at every window across the records; over -A it gives the identity
    for op, want_of in (("fb_mul2_same", lambda k: bn.g1_mul(FV.base("A"), 2 * k)), ("fb_mul2_neg", lambda k: None)):
        eq = [r for r in by[op] if r[1][0] == r[1][1]]
        firsts = {next(w for w, d in enumerate(FV.recode(r[1][0], W)[0]) if d) for r in eq}
        assert firsts == set(range(NW))
        assert all(r[3] == want_of(r[1][0]) for r in eq)
        assert all(r[1][2:50] == r[1][50:] for r in eq) == (op == "fb_mul2_same")
        low = [r for r in by[op] if r[4].startswith("low_eq_")]
        assert len(low) == 3 and all(r[3] is not None and r[1][0] != r[1][1] and r[1][0] % (1 << W) == r[1][1] % (1 << W)
                                     for r in low)
    # accumulators: identity, -(k B), k B, the first entry, its negative, on 12 scalars and 0
    for op in ("fb_mul_acc", "fb_mul_acc_jac"):
        kinds = {}
        for _, ins, _, want, tag in by[op]:
            kinds.setdefault(tag.split(":")[0], []).append((AV.norm_jac(FV.C, ins[:3]), ins, want))
        assert set(kinds) == set(FV.ACC_KINDS) and all(len(kinds[k]) == 13 for k in FV.ACC_KINDS[:-1])
        B = FV.base("B16")
        assert all(acc is None and ins[2] == 0 and want == bn.g1_mul(B, ins[3]) for acc, ins, want in kinds["identity"])
        assert all(want is None and acc == bn.g1_neg(bn.g1_mul(B, ins[3])) for acc, ins, want in kinds["neg_kB"])
        assert all(acc == bn.g1_mul(B, ins[3]) and want == bn.g1_mul(B, 2 * ins[3]) for acc, ins, want in kinds["kB"])
        for sign, kind in ((1, "first_entry"), (-1, "neg_first_entry")):
            for acc, ins, want in kinds[kind]:
                ds = FV.recode(ins[3], W)[0]
                first = next(((w, d) for w, d in enumerate(ds) if d), None)
                assert acc == (bn.g1_mul(B, sign * first[1] << (W * first[0])) if first else None)
        # the accumulator reaches the device with a denominator other than 1
        assert all(ins[2] != AV.to_mont(1, bn.P) for _, ins, _ in kinds["random"])


def test_contract_violations_end_the_tool_before_any_launch(tmp_path):
    k = dict(FV.scalars(16))["w0_d1"]
    good = [k] + FV.entry_words("B16", 16, k)
    other = [k] + FV.entry_words("A", 16, k)  # the same positions, another base's points
    off = list(good)
    off[3] = (off[3] + 1) % bn.P  # y of window 0: not on the curve
    big = list(good)
    big[1] = (1 << 15) + 1  # |d| > E
    zero_d = list(good)
    zero_d[1] = 0  # a point under digit 0
    bad = [[("fb_mul_16", good), ("fb_mul_16", other)], [("fb_mul_16", off)], [("fb_mul_16", big)],
           [("fb_mul_16", zero_d)], [("fb_mul_16", good[:-1])], [("fb_mul_16", good + [0])],
           [("fb_mul_16", [bn.R] + good[1:])], [("fb_digits_20", [bn.R])]]
    for recs in bad:
        inp = tmp_path / "in.txt"
        inp.write_text(AV.format_records([(op, ins, "raw", None) for op, ins in recs]))
        out = subprocess.run([EXE, str(inp), str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2, (recs[0][0], out.returncode, out.stderr)
        assert not (tmp_path / "out.txt").exists()


def test_table_entries_hook_refuses_a_context_without_tables(host_pp):
    """fts_debug_table_entries on a host-only context (no device, no tables) and on no context"""
    import ctypes as C
    from fts_gpu import _lib as L
    w, d, out = (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(1), C.create_string_buffer(64)
    for wide in (0, 1):
        assert L.lib.fts_debug_table_entries(host_pp(8)._ctx, wide, 0, 1, w, d, out) == -1  # FTS_API_EINVAL
        assert L.lib.fts_debug_table_entries(None, wide, 0, 1, w, d, out) == -1
