"""CPU: the audit-info matcher's fixtures, restatement, host parser and C-ABI
surface (no device): tests/golden/idemix_audit_golden.json against
tests/idemix_audit_ref.py, the attribute encoding pinned by the reference's own
SignerConfig files, lib/idemix_parse_check on `audit` inputs under the host
sanitizers, the new status strings and the argument check that needs no handle."""
import ctypes as C
import json
import os
import subprocess

import pytest

from conftest import ROOT

import idemix_audit_ref as REF
from oracle import idemix as I, idemix_identity as ID, pairing as PR

GOLD = os.path.join(ROOT, "tests", "golden")
CURVES = {"bn254": (I.BN254C, PR.BN254), "fp256bn": (I.FP256BNC, PR.FP256BN)}
# FP256BN: Python products take ~80 ms each, so one case per status and the honest ones
FBN_SUBSET = ("honest_0", "honest_1", "honest_2", "r_eid_equals_r", "wrong_r_eid", "wrong_rh", "no_eidnym",
              "no_rhnym", "eidnym_all_zero", "rhnym_off_curve", "attr_len_64", "s_sk_31_bytes", "garbage_proof")


@pytest.fixture(scope="module")
def doc():
    with open(os.path.join(GOLD, "idemix_audit_golden.json")) as f:
        return json.load(f)


def _raw(*p):
    with open(os.path.join(GOLD, "idemix", *p), "rb") as f:
        return f.read()


def _verdict(ipk, Cv, c):
    return REF.audit_match(ipk, Cv, bytes.fromhex(c["identity"]), bytes.fromhex(c["eid"]), int(c["r_eid"], 16),
                           bytes.fromhex(c["rh"]), int(c["r_rh"], 16))


def test_fixture_verdicts_bn254(doc):
    d = doc["bn254"]
    ipk = I.parse_ipk(_raw(d["issuer"], "IssuerPublicKey"), I.BN254C)
    assert len(d["cases"]) >= 49
    assert {c["name"]: _verdict(ipk, I.BN254C, c) for c in d["cases"]} == {c["name"]: c["error"] for c in d["cases"]}
    assert {c["error"] for c in d["cases"]} == set(REF.STATUS)


def test_fixture_verdicts_fp256bn_subset(doc):
    d = doc["fp256bn"]
    ipk = I.parse_ipk(_raw(d["issuer"], "IssuerPublicKey"), I.FP256BNC)
    by = {c["name"]: c for c in d["cases"]}
    assert {n: _verdict(ipk, I.FP256BNC, by[n]) for n in FBN_SUBSET} == {n: by[n]["error"] for n in FBN_SUBSET}
    # one case per status among them, and the two curves differ only where their point rules do
    assert {by[n]["error"] for n in FBN_SUBSET} == set(REF.STATUS)
    bn = {c["name"]: c["error"] for c in doc["bn254"]["cases"]}
    diff = {n for n in bn if bn[n] != by[n]["error"]}
    assert diff == {"eidnym_all_zero"} and bn["eidnym_all_zero"] == REF.E_EID_MISMATCH
    assert by["eidnym_all_zero"]["error"] == REF.E_EID_POINT


@pytest.mark.parametrize("tag,eid,rh", [("bn254", b"charlie.ExtraId2", b"1"), ("fp256bn", b"alice", b"150")])
def test_attribute_encoding_pinned_by_signer_configs(doc, tag, eid, rh):
    """the credential's attributes 2 and 3 are HashToZr of the SignerConfig's enrollment
    id and revocation handle: the encoding Match recomputes from AuditInfo.Attributes"""
    Cv, _ = CURVES[tag]
    sc = _raw(doc[tag]["issuer"], "SignerConfig")
    assert REF.signer_strings(sc) == (eid, rh)
    cred = ID.parse_signer_config(sc, Cv)
    assert Cv.hash_to_zr(eid) == cred["attrs"][2]
    assert Cv.hash_to_zr(rh) == cred["attrs"][3]
    honest = {c["name"]: c for c in doc[tag]["cases"]}["honest_0"]
    assert (bytes.fromhex(honest["eid"]), bytes.fromhex(honest["rh"])) == (eid, rh)


def test_honest_fixture_identity_verifies(doc):
    d = doc["bn254"]
    raw = _raw(d["issuer"], "IssuerPublicKey")
    ipk = I.parse_ipk(raw, I.BN254C)
    honest = {c["name"]: c for c in d["cases"]}["honest_1"]
    ID.verify_identity(ipk, PR.BN254, ID.ipk_w(PR.BN254, raw), bytes.fromhex(honest["identity"]))


def test_audit_parser_under_sanitizers(doc, tmp_path):
    """lib/idemix_parse_check on `audit` lines: every fixture identity as it is, as every
    strict prefix, with single-byte corruptions and in the null / zero-length forms
    (the tool does all of these for each input); no sanitizer report, and the host's
    statuses of the fixture cases are what the stored verdicts imply"""
    lines, want = [], []
    for tag in ("bn254", "fp256bn"):
        for c in doc[tag]["cases"]:
            lines.append("audit %s %s %s\n" % (tag, c["identity"] or "-", "honest" if c["name"].startswith("honest_") else ""))
            want.append((tag, c["name"], c["error"]))
    inp = tmp_path / "audit_inputs.txt"
    inp.write_text("".join(lines))
    exe = os.path.join(ROOT, "fabric-token-sdk_amd", "lib", "idemix_parse_check")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "idemix_parse_check: ok" in out.stdout
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
    got = {}
    for ln in out.stdout.splitlines():
        if ln.startswith("audit "):
            _, idx, pre, rh_pre = ln.split()
            got[int(idx)] = (int(pre), int(rh_pre))
    assert len(got) == len(want)
    S = REF.STATUS
    host_final = (REF.E_MALFORMED, REF.E_NO_EIDNYM)
    for k, (tag, name, err) in enumerate(want):
        pre, rh_pre = got[k]
        if err in host_final:
            assert pre == S[err], (tag, name)
        elif name == "eidnym_31_byte_coordinate":  # G1FromProto's length rule is the host's
            assert (pre, err) == (S[REF.E_EID_POINT], REF.E_EID_POINT), (tag, name)
        elif err == REF.E_NO_RHNYM:  # counts only after the EID half has passed on the device
            assert (pre, rh_pre) == (0, S[err]), (tag, name)
        else:  # goes to the device
            assert (pre, rh_pre) == (0, 0), (tag, name)


def test_status_strings_and_null_handle():
    from fts_gpu import _lib as L
    from fts_gpu import idemix as X
    codes = [L.FTS_E_AUDIT_MALFORMED, L.FTS_E_AUDIT_NO_EIDNYM, L.FTS_E_AUDIT_EID_POINT, L.FTS_E_AUDIT_EID_MISMATCH,
             L.FTS_E_AUDIT_NO_RHNYM, L.FTS_E_AUDIT_RH_POINT, L.FTS_E_AUDIT_RH_MISMATCH]
    assert codes == list(range(L.FTS_E_ID_ZK + 1, L.FTS_E_ID_ZK + 8))
    by_status = {v: k for k, v in REF.STATUS.items()}
    for c in codes:
        assert L.status_str(c) == by_status[c] == X.message(c)
    assert X.message(L.FTS_OK) is None
    st = (C.c_int32 * 1)()
    items = (L.AuditItem * 1)()
    assert L.lib.fts_idemix_audit_match_batch(None, 1, items, st) == -1  # FTS_API_EINVAL
    assert L.lib.fts_idemix_audit_match_batch(None, 0, None, None) == -1
    ms = C.c_float()
    assert L.lib.fts_idemix_audit_last_timings(None, C.byref(ms)) == -1
