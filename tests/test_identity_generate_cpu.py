"""CPU: the host side of identity generation (csrc/host/identity_write.hpp) -- the draws of
one identity, the identity writer and the credential / revocation-information parsers --
through the library's host-only entry points and through lib/idgen_check (a stand-alone
program built with the host address and undefined-behaviour sanitizers)."""
import os
import random
import subprocess

import pytest

from conftest import PKG

import idgen_common as G
from oracle import idemix as OI, idemix_identity as ID

CHECK = os.path.join(PKG, "lib", "idgen_check")
TAGS = ["bn254", "fp256bn"]
SEEDS = [0, 1, 77, (1 << 63) + 5, (1 << 64) - 3]


def run(lines):
    p = subprocess.run([CHECK], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return out


def _ints(hexline):
    b = bytes.fromhex(hexline)
    return [int.from_bytes(b[32 * k:32 * k + 32], "big") for k in range(len(b) // 32)]


@pytest.mark.parametrize("tag", TAGS)
def test_draws_deterministic_below_r_and_shifted(tag):
    from fts_gpu import idemix as I
    _, cid, C, _ = G.CURVES[tag]
    for seed in SEEDS[:4]:
        d = [I.identity_draws(cid, seed, i) for i in range(6)]
        assert d == [I.identity_draws(cid, seed, i) for i in range(6)]
        for i, v in enumerate(d):
            assert len(v) == 18 and all(0 <= x < C.r for x in v) and v[1] != 0
            assert len(set(v)) == 18
        for i in range(5):
            assert d[i] != d[i + 1] and not set(d[i]) & set(d[i + 1])
            # item i + 1 at `seed` is item i at seed + 1
            assert d[i + 1] == I.identity_draws(cid, seed + 1, i)
    # uniform by rejection over four stream words: both halves of [0, r) turn up
    top = [v >> (C.r.bit_length() - 1) for i in range(40) for v in I.identity_draws(cid, 5, i)]
    assert 0 < sum(top) < len(top)


@pytest.mark.parametrize("tag", TAGS)
def test_draws_of_the_check_program_equal_the_library(tag):
    from fts_gpu import idemix as I
    cid = G.CURVES[tag][1]
    cases = [(s, i) for s in SEEDS[:3] for i in (0, 1, 129)]
    out = run(["draws %d %d %d" % (cid, s, i) for s, i in cases])
    assert [_ints(o) for o in out] == [I.identity_draws(cid, s, i) for s, i in cases]


def test_draws_reject_the_os_seed_and_bad_curves():
    from fts_gpu import idemix as I, _lib as L
    with pytest.raises(L.FtsError):
        I.identity_draws(1, (1 << 64) - 1, 0)
    with pytest.raises(L.FtsError):
        I.identity_draws(2, 1, 0)


def _synthetic(C, PC, rng, small=False):
    """a signature dict of arbitrary field values (the writer copies, it does not check)"""
    def z():
        return rng.randrange(1 << 8) if small else rng.randrange(C.r)

    def pt():
        return (rng.randrange(1 << 16), rng.randrange(C.p)) if small else (rng.randrange(C.p), rng.randrange(C.p))
    s = {k: pt() for k in ("APrime", "ABar", "BPrime", "Nym", "EidNym", "RhNym")}
    s.update({k: z() for k in ("c", "sSk", "sE", "sR2", "sR3", "sSPrime", "sRNym", "sEid", "sRh", "nonce")})
    s["sAttrs"] = [z() for _ in range(4)]
    s.update(rev_alg=0, epoch=0, epoch_pk=PC.g2_gen)
    return s


@pytest.mark.parametrize("tag", TAGS)
def test_writer_equals_oracle_encoding(tag):
    from fts_gpu import idemix as I
    _, cid, C, PC = G.CURVES[tag]
    rng = random.Random(1600 + cid)
    sigs = [_synthetic(C, PC, rng), _synthetic(C, PC, rng, small=True)]
    if tag == "bn254":  # a real signature too (the FP256BN oracle takes seconds per signature)
        ipk, cred, _ = G.oracle_key(tag)
        sigs.append(G.oracle_sign(tag, ipk, cred, I.identity_draws(cid, 9, 0))[0])
    lines, want = [], []
    for s in sigs:
        for epoch in (0, 1, 127, 128, (1 << 63) - 1):
            s = dict(s, epoch=epoch)
            pts, sc, nonce = G.writer_inputs(s)
            w = ID.serialize_identity(C.g1_bytes(s["Nym"]), ID.encode_signature(s, PC))
            assert I.write_identity(cid, pts, sc, nonce, epoch=epoch) == w
            want.append(w.hex())
            lines.append("write %d %d %s %s %064x -" % (
                cid, epoch, "".join("%064x%064x" % p for p in pts), "".join("%064x" % v for v in sc), nonce))
    assert run(lines) == want
    # another epoch key: copied as given
    epk = bytes(range(128))
    got = I.write_identity(cid, pts, sc, nonce, epoch_pk=epk, epoch=0)
    key = b"".join(OI.pb_bytes_field(k + 1, epk[32 * k:32 * k + 32]) for k in range(4))
    assert OI.pb_bytes_field(14, key) in got and len(got) == len(bytes.fromhex(want[0]))
    assert run(["write %d 0 %s %s %064x %s" % (cid, "".join("%064x%064x" % p for p in pts),
                                              "".join("%064x" % v for v in sc), nonce, epk.hex())]) == [got.hex()]


@pytest.mark.parametrize("tag", TAGS)
def test_identity_length(tag):
    _, cid, C, PC = G.CURVES[tag]
    s = _synthetic(C, PC, random.Random(3))
    for epoch in (0, 1, 300):
        w = ID.serialize_identity(C.g1_bytes(s["Nym"]), ID.encode_signature(dict(s, epoch=epoch), PC))
        assert run(["len %d %d" % (cid, epoch)]) == [str(len(w))]
    assert run(["len %d 0" % cid]) == ["1113" if tag == "bn254" else "1114"]


def test_writer_size_check():
    import ctypes as C
    from fts_gpu import _lib as L
    n = C.c_size_t()
    buf = (C.c_uint8 * 1113)(*([0xAA] * 1113))
    args = (1, bytes(384), bytes(416), bytes(32), None, 0)
    assert L.lib.fts_debug_idemix_identity_write(*args, buf, 1112, C.byref(n)) == -5  # FTS_API_ESIZE
    assert n.value == 1113 and bytes(buf) == b"\xaa" * 1113
    assert L.lib.fts_debug_idemix_identity_write(*args, buf, 1113, C.byref(n)) == 0 and bytes(buf)[:2] == b"\x0a\x40"


@pytest.mark.parametrize("tag", TAGS)
def test_credential_and_cri_parsers(tag):
    from fts_gpu import idemix as I
    _, cid, C, PC = G.CURVES[tag]
    _, cred, _ = G.oracle_key(tag)
    cred_raw, sk, cri = I.parse_signer_config(G.raw(tag, "SignerConfig"))
    assert int.from_bytes(sk, "big") == cred["sk"] and cri == cred["cri"]
    want = "ok " + "".join("%064x%064x" % p for p in (cred["A"], cred["B"])) + \
        "".join("%064x" % v for v in [cred["E"], cred["S"]] + cred["attrs"])
    f = OI.pb_fields(cred_raw)

    def enc(fields):
        return b"".join(OI.pb_bytes_field(k, v) for k, _, v in fields)
    three = [x for x in f if x[0] != 5] + [x for x in f if x[0] == 5][:3]
    five = f + [x for x in f if x[0] == 5][:1]
    big_e = [(k, wt, C.r.to_bytes(32, "big") if k == 3 else v) for k, wt, v in f]
    out = run(["cred %d %s" % (cid, r.hex()) for r in
               (cred_raw, enc(three), enc(five), enc(big_e), cred_raw[:-1], cred_raw[:40])])
    assert out == [want, "bad", "bad", "bad", "bad", "bad"]
    # the revocation information: the fixture's, none, an algorithm set, no epoch key, truncated
    g2 = b"".join(v for _, _, v in OI.pb_fields(ID.ecp2(PC, PC.g2_gen)))
    epoch = dict((k, v) for k, wt, v in OI.pb_fields(cri) if wt == 0).get(1, 0)
    with_alg = cri + ID._varint_field(4, 1)
    no_key = b"".join(OI.pb_bytes_field(k, v) for k, wt, v in OI.pb_fields(cri) if k == 3)
    out = run(["cri %d %s" % (cid, r) for r in ("-", cri.hex(), with_alg.hex(), no_key.hex(), cri[:-2].hex())])
    assert out == ["ok 0 " + g2.hex(), "ok %d %s" % (epoch, g2.hex()), "bad", "bad", "bad"]


def test_size_t_entry_points_are_bound():
    """the header's functions that return a size_t (test_lib_cpu's list holds the int, void and
    string ones): each is exported and bound with that return type"""
    import ctypes as C
    import re
    from conftest import ROOT
    from fts_gpu import _lib as L
    with open(os.path.join(ROOT, "include", "fts_gpu.h")) as f:
        names = sorted(set(re.findall(r"^size_t\s+(fts_\w+)\s*\(", f.read(), re.M)))
    assert names == ["fts_idemix_identity_len"]
    for n in names:
        assert getattr(L.lib, n).restype is C.c_size_t and n not in L.EXPORTED
    assert L.lib.fts_idemix_identity_len(None) == 0
