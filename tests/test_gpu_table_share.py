"""GPU: fixed-base tables shared between the contexts of one device (the table cache,
csrc/host/table_cache.hpp; fts_ctx_table_info / fts_table_cache_stats).

Bit lengths 8 and 16 are the smallest shapes that still have every table kind
(22 / 38 narrow bases, 10 / 18 wide ones); several contexts live at once, so they
run one lane each (FTS_LANES=1).

Other tests' contexts may be alive in the session (conftest's per-bit-length
contexts) and may hold the very entries a test here asks for.  So every statement
about the cache's books is a DELTA over the test's own steps, and a reference count
is stated against the entry's count before the step.  What an entry adds to the
books is decided by its `built` flag: a context that found its entry held by an
outsider adds nothing for it.  With nobody else alive these reduce to the plain
figures: refs 2 for two contexts, resident_bytes == table_bytes, builds 2 / hits 14
for eight creators."""
import base64
import json
import os
import threading

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "rp_golden.json")) as f:
    RP_GOLDEN = json.load(f)
with open(os.path.join(GOLDEN, "transfer_golden.json")) as f:
    TRANSFERS = json.load(f)
STATUS_OF = {None: 0, "invalid range proof": 3, "invalid IPA": 6, "invalid range proof: nil elements": 2,
             "invalid IPA proof: nil elements": 4, "invalid IPA proof": 5}
KNOBS = ("FTS_LANES", "FTS_TABLE_SHARE", "FTS_WIDE_BITS")


def _ctx(pp_raw, bits, env=None, **kw):
    """a context created under exactly the given table knobs (FTS_LANES=1 unless said)"""
    import fts_gpu
    env = dict({"FTS_LANES": 1}, **(env or {}))
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return fts_gpu.PublicParams(pp_raw, bit_length=bits, **dict({"device": 0}, **kw))
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _golden_ok(pp, bits):
    """the golden range-proof verdicts (honest and tampered) at this bit length"""
    cases = [c for c in RP_GOLDEN if c["bits"] == bits]
    assert cases
    st = pp.verify_range_proofs([bytes.fromhex(c["proof"]) for c in cases],
                                [bytes.fromhex(c["commitment"]) for c in cases])
    assert [int(s) for s in st] == [STATUS_OF[c["expect"]] for c in cases]


def _stats():
    import fts_gpu
    return fts_gpu.table_cache_stats(0)


def _delta(after, before):
    return type(after)(*(a - b for a, b in zip(after, before)))


def _added(info):
    """(bytes, entries) a context's creation added to the books"""
    return (info.narrow_bytes * info.narrow_built + info.wide_bytes * info.wide_built,
            info.narrow_built + info.wide_built)


def _check_builder(info):
    """an entry this context built was held by nobody before; one it found, by somebody"""
    assert info.narrow_built in (0, 1) and info.wide_built in (0, 1)
    assert (info.narrow_refs == 1) == (info.narrow_built == 1), info
    assert (info.wide_refs == 1) == (info.wide_built == 1), info


def test_same_pp_twice_shares_and_outlives_the_builder(pp_raw):
    s0 = _stats()
    a = _ctx(pp_raw, 8, wide_bits=20)
    b = None
    try:
        ia = a.table_info()
        _check_builder(ia)
        assert ia.narrow_bytes + ia.wide_bytes == a.table_bytes
        add_bytes, add_entries = _added(ia)
        b = _ctx(pp_raw, 8, wide_bits=20)
        ib, ia2 = b.table_info(), a.table_info()
        assert (ib.narrow_built, ib.wide_built) == (0, 0)
        assert (ib.narrow_id, ib.wide_id) == (ia.narrow_id, ia.wide_id)
        assert ib.narrow_refs == ia2.narrow_refs == ia.narrow_refs + 1
        assert ib.wide_refs == ia2.wide_refs == ia.wide_refs + 1
        assert a.table_bytes == b.table_bytes == (2 * 8 + 6) * 32 * (1 << 20) + (8 + 2) * 13 * (1 << 19) * 64
        d = _delta(_stats(), s0)
        assert (d.resident_bytes, d.entries) == (add_bytes, add_entries)
        assert d.builds == add_entries and d.hits == 4 - add_entries
        _golden_ok(a, 8)
        _golden_ok(b, 8)
        a.close()  # the builder goes first: b keeps reading the same memory
        _golden_ok(b, 8)
        ib = b.table_info()
        assert (ib.narrow_id, ib.wide_id) == (ia.narrow_id, ia.wide_id)
        assert (ib.narrow_refs, ib.wide_refs) == (ia.narrow_refs, ia.wide_refs)
        d = _delta(_stats(), s0)
        assert (d.resident_bytes, d.entries) == (add_bytes, add_entries)
        b.close()
        d = _delta(_stats(), s0)
        assert (d.resident_bytes, d.entries) == (0, 0)  # nothing is kept alive
    finally:
        a.close()
        if b is not None:
            b.close()


def test_different_bit_lengths_share_nothing(pp_raw):
    s0 = _stats()
    a = _ctx(pp_raw, 8, wide_bits=20)
    b = None
    try:
        b = _ctx(pp_raw, 16, wide_bits=20)
        ia, ib = a.table_info(), b.table_info()
        assert len({ia.narrow_id, ia.wide_id, ib.narrow_id, ib.wide_id}) == 4
        assert ia.narrow_bytes + ia.wide_bytes == a.table_bytes
        assert ib.narrow_bytes + ib.wide_bytes == b.table_bytes and b.table_bytes > a.table_bytes
        d = _delta(_stats(), s0)
        assert d.resident_bytes == _added(ia)[0] + _added(ib)[0]
        assert d.entries == _added(ia)[1] + _added(ib)[1]
        _golden_ok(a, 8)
        _golden_ok(b, 16)
    finally:
        a.close()
        if b is not None:
            b.close()
    assert _delta(_stats(), s0)[:2] == (0, 0)


def _varint(b, i):
    v = shift = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << shift
        shift += 7
        if not c & 0x80:
            return v, i


def _swap_pedersen_1_2(pp_raw):
    """the fixture PP with the byte strings of PedersenGenerators[1] and [2] (field 4 of
    nogh.PublicParameters, length-delimited) exchanged; equal lengths, valid points"""
    c = json.loads(pp_raw)
    raw = base64.b64decode(c["raw"])
    spans, i = [], 0
    while i < len(raw):
        key, i = _varint(raw, i)
        wt = key & 7
        if wt == 2:
            ln, i = _varint(raw, i)
            if key >> 3 == 4:
                spans.append((i, i + ln))
            i += ln
        elif wt == 0:
            _, i = _varint(raw, i)
        else:
            i += 8 if wt == 1 else 4
    assert len(spans) == 3
    (a0, a1), (b0, b1) = spans[1], spans[2]
    assert a1 - a0 == b1 - b0 and raw[a0:a1] != raw[b0:b1]
    out = raw[:a0] + raw[b0:b1] + raw[a1:b0] + raw[a0:a1] + raw[b1:]
    c["raw"] = base64.b64encode(out).decode()
    return json.dumps(c).encode()


def test_other_pedersen_generators_share_the_wide_set(pp_raw):
    var_raw = _swap_pedersen_1_2(pp_raw)
    f = _ctx(pp_raw, 8, wide_bits=20)
    v = None
    try:
        v = _ctx(var_raw, 8, wide_bits=20)
        fi, vi = f.table_info(), v.table_info()
        assert vi.wide_id == fi.wide_id and vi.wide_built == 0 and vi.wide_refs == fi.wide_refs
        assert vi.narrow_id != fi.narrow_id and vi.narrow_built == 1 and vi.narrow_refs == 1
        assert v.table_bytes == f.table_bytes
        vals = [0, 1, 77, 255]
        made = [v.prove_range(x, (900 + j).to_bytes(32, "big"), 40 + j) for j, x in enumerate(vals)]
        proofs, coms = [p for p, _ in made], [c for _, c in made]
        assert [int(s) for s in v.verify_range_proofs(proofs, coms)] == [0] * len(vals)
        assert all(int(s) != 0 for s in f.verify_range_proofs(proofs, coms))
        _golden_ok(f, 8)  # the fixture's own proofs are untouched by the neighbour
    finally:
        f.close()
        if v is not None:
            v.close()


def test_widths_forced_and_inherited(pp_raw):
    s0 = _stats()
    a = _ctx(pp_raw, 8, wide_bits=22)
    b = c = None
    try:
        ia = a.table_info()
        assert a.wide_bits == 22 and ia.wide_bytes == (8 + 2) * 12 * (1 << 21) * 64
        b = _ctx(pp_raw, 8, wide_bits=20)
        ib = b.table_info()
        assert b.wide_bits == 20 and ib.narrow_id == ia.narrow_id and ib.narrow_built == 0
        assert ib.wide_id != ia.wide_id and ib.wide_bytes == (8 + 2) * 13 * (1 << 19) * 64
        # no width, no budget, no FTS_WIDE_BITS: A's 22-bit set is there for the taking
        c = _ctx(pp_raw, 8)
        ic = c.table_info()
        assert c.wide_bits == 22 and ic.wide_id == ia.wide_id and ic.wide_built == 0
        assert ic.narrow_id == ia.narrow_id and c.table_bytes == a.table_bytes
        assert a.table_info().wide_refs == ia.wide_refs + 1
        assert a.table_info().narrow_refs == ia.narrow_refs + 2
        for pp in (a, b, c):
            _golden_ok(pp, 8)
    finally:
        for pp in (a, b, c):
            if pp is not None:
                pp.close()
    assert _delta(_stats(), s0)[:2] == (0, 0)


def _check_single_flight(infos, d, n):
    """n creators of one narrow and one wide key: one build per key nobody held, every
    other creator a hit, one buffer per key held by all n"""
    assert len({i.narrow_id for i in infos}) == 1 and len({i.wide_id for i in infos}) == 1
    nb, wb = sum(i.narrow_built for i in infos), sum(i.wide_built for i in infos)
    assert nb in (0, 1) and wb in (0, 1)
    assert d.builds == nb + wb and d.hits == 2 * n - (nb + wb)
    assert d.entries == nb + wb
    assert d.resident_bytes == nb * infos[0].narrow_bytes + wb * infos[0].wide_bytes
    for i in infos:  # built by one of the n: held by the n alone
        assert (i.narrow_refs == n) if nb else (i.narrow_refs > n), i
        assert (i.wide_refs == n) if wb else (i.wide_refs > n), i


def test_eight_shards_on_one_device_build_once(pp_raw):
    import fts_gpu
    s0 = _stats()
    multi = _ctx(pp_raw, 16, env={"FTS_WIDE_BITS": 20}, device=None, devices=[0] * 8)
    single = None
    try:
        assert multi.devices == [0] * 8
        infos = [multi.table_info(j) for j in range(8)]
        _check_single_flight(infos, _delta(_stats(), s0), 8)
        assert multi.table_bytes == 8 * (infos[0].narrow_bytes + infos[0].wide_bytes)
        with pytest.raises(fts_gpu.FtsError):
            multi.table_info(8)
        single = _ctx(pp_raw, 16, wide_bits=20)
        assert single.table_info().narrow_id == infos[0].narrow_id
        assert single.table_info().wide_id == infos[0].wide_id
        # the golden transfers (16-bit honest and wrong-sum ones, and the 8-bit one, whose
        # range proofs do not fit 16-bit parameters), tiled over all eight shards
        items = [([bytes.fromhex(h) for h in c["inputs"]], [bytes.fromhex(h) for h in c["outputs"]],
                  bytes.fromhex(c["proof"])) for c in TRANSFERS] * 13
        assert len(items) >= 64
        s1, f1 = single.verify_transfers(items)
        s2, f2 = multi.verify_transfers(items)
        assert [(int(s), int(i)) for s, i in zip(s2, f2)] == [(int(s), int(i)) for s, i in zip(s1, f1)]
        want = [c["expect"] for c in TRANSFERS if c["bits"] == 16]
        got = [fts_gpu.transfer_message(int(s), int(i)) for s, i, c in zip(s2, f2, TRANSFERS) if c["bits"] == 16]
        assert got == want and any(w is not None for w in want)
    finally:
        multi.close()
        if single is not None:
            single.close()
    assert _delta(_stats(), s0)[:2] == (0, 0)


def test_eight_threads_build_once(pp_raw):
    import fts_gpu
    s0 = _stats()
    ctxs, errs = [None] * 8, []

    def create(t):
        try:
            ctxs[t] = fts_gpu.PublicParams(pp_raw, bit_length=8, device=0, wide_bits=20)
        except Exception as e:  # noqa: BLE001 (reported below)
            errs.append(e)

    # the environment is set once, around all eight creators
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ["FTS_LANES"] = "1"
    try:
        th = [threading.Thread(target=create, args=(t,)) for t in range(8)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
        _check_single_flight([c.table_info() for c in ctxs], _delta(_stats(), s0), 8)
        for c in (ctxs[0], ctxs[7]):
            _golden_ok(c, 8)
    finally:
        os.environ.pop("FTS_LANES", None)
        for k in KNOBS:
            if old[k] is not None:
                os.environ[k] = old[k]
        for c in ctxs:
            if c is not None:
                c.close()
    assert _delta(_stats(), s0)[:2] == (0, 0)


def test_knob_table_share_off(pp_raw):
    """FTS_TABLE_SHARE=0: private tables, outside the cache's books"""
    a = _ctx(pp_raw, 8, wide_bits=20)
    b = None
    try:
        ia, s1 = a.table_info(), _stats()
        b = _ctx(pp_raw, 8, env={"FTS_TABLE_SHARE": 0}, wide_bits=20)
        ib = b.table_info()
        assert (ib.narrow_built, ib.wide_built, ib.narrow_refs, ib.wide_refs) == (1, 1, 1, 1)
        assert len({ia.narrow_id, ia.wide_id, ib.narrow_id, ib.wide_id}) == 4
        assert (ib.narrow_bytes, ib.wide_bytes) == (ia.narrow_bytes, ia.wide_bytes)
        assert b.table_bytes == a.table_bytes and b.wide_bits == 20
        assert _stats() == s1  # not a build, not a hit, not resident
        assert a.table_info() == ia
        _golden_ok(b, 8)
        a.close()
        _golden_ok(b, 8)
        b.close()
        assert _delta(_stats(), s1)[:2] == tuple(-x for x in _added(ia))
    finally:
        a.close()
        if b is not None:
            b.close()
