"""GPU: batched token commitments (fts_token_commit_batch_gpu, k_token_commit) and
whole actions generated on the device (fts_transfer_generate_batch_gpu,
fts_issue_generate_batch_gpu).

The commit kernel is compared byte for byte with the host's token_commit at the
batch sizes around a wave and around one launch width (lanes x tokens per lane,
read from the binding), the digit edges of the 16-bit windows, blinding factors
around r, and types that cross the SHA-256 padding edges, mixed within a wave.
Device generation equals host generation action by action (seed + i), and what it
emits goes through the request verifier and the metadata opening check as is."""
import random

import pytest

import generate_cases as gc

pytestmark = pytest.mark.gpu

VALUES = [0, 1, 0xFFFF, 0x10000, 1 << 32, (1 << 64) - 1]
BFS = [0, 1, gc.R - 1, gc.R, gc.R + 1, (1 << 256) - 1]
TYPES = [b"", b"ABC", b"t" * 55, b"u" * 56, b"v" * 64, b"w" * 200]


def _items(n):
    """item i: value / blinding factor / type edges on coprime strides, so every pair meets
    and neighbouring lanes hold different types"""
    rng = random.Random(n)
    out = []
    for i in range(n):
        v = VALUES[i % 6] if i % 7 else rng.randrange(1 << 64)
        b = BFS[(i // 6) % 6] if i % 11 else rng.randrange(1 << 256)
        out.append((TYPES[(i + i // 36) % 6], v, b.to_bytes(32, "big")))
    return out


@pytest.fixture(scope="module")
def host_commits(host_pp):
    """token_commit of _items(n), computed once per item (the host tables do not depend on the bit length)"""
    pp = host_pp(16)
    memo = {}

    def get(items):
        return [memo.setdefault(it, pp.token_commit(*it)) for it in items]
    return get


def test_commit_kernel_matches_token_commit(gpu_pp, host_commits):
    import fts_gpu as F
    pp = gpu_pp(16)
    width = F.token_commit_batch_width()
    assert width % 64 == 0
    for n in sorted({1, 2, 63, 64, 65, width - 1, width + 1}):
        items = _items(n)
        dev = pp.token_commit_batch_gpu(items)
        want = host_commits(items)
        assert dev == want, n
        if n == width + 1:
            st = pp.check_openings([(c, t, v.to_bytes(32, "big"), b) for c, (t, v, b) in zip(dev, items)])
            assert [int(s) for s in st] == [F.FTS_OK] * n


def test_commit_kernel_every_edge_pair(gpu_pp, host_commits):
    """every (value, blinding factor, type) edge combination in one batch"""
    pp = gpu_pp(16)
    items = [(t, v, b.to_bytes(32, "big")) for v in VALUES for b in BFS for t in TYPES]
    assert pp.token_commit_batch_gpu(items) == host_commits(items)


def test_device_transfer_generation_equals_host(gpu_pp):
    pp = gpu_pp(64)
    rng = gc.rng_for("gpu-t")
    cases = [gc.transfer_case(pp, rng, nin, nout, ttype=b"ABC" if nin % 2 else b"USD", redeem_last=(nin == 3))
             for nin, nout in [(2, 2), (1, 1), (1, 2), (3, 1), (2, 3)]]
    dev = pp.generate_transfers_gpu(cases, seed=8000)
    for i, case in enumerate(cases):
        assert dev[i] == pp.generate_transfer(*case, seed=8000 + i), i
    gc.check_transfer_parts(pp, cases[0], dev[0], 8000)


def test_device_issue_generation_equals_host(gpu_pp):
    pp = gpu_pp(32)
    rng = gc.rng_for("gpu-i")
    cases = [gc.issue_case(pp, rng, m) for m in (1, 4, 16)]
    dev = pp.generate_issues_gpu(cases, seed=8100)
    for i, case in enumerate(cases):
        assert dev[i] == pp.generate_issue(*case, seed=8100 + i), i
    gc.check_issue_parts(pp, cases[1], dev[1], 8101)


def test_generated_actions_round_trip_through_the_verifier(gpu_pp):
    """130 generated 2-in/2-out transfers (across the 64- and 128-lane edges of the
    thread-per-action kernel) and a few issues, as TokenRequests; one transfer's sums
    differ and is the only one rejected"""
    import fts_gpu as F
    pp = gpu_pp(16)
    rng = gc.rng_for("gpu-rt")
    bad = 77
    trs = [gc.transfer_case(pp, rng, 2, 2, extra=1 if i == bad else 0) for i in range(130)]
    iss = [gc.issue_case(pp, rng, m) for m in (1, 2, 3)]
    gt = pp.generate_transfers_gpu(trs, seed=8200)
    gi = pp.generate_issues_gpu(iss, seed=8400)
    reqs = [F.request.token_request([(F.request.TRANSFER, g[0])], [b"sig"]) for g in gt]
    reqs += [F.request.token_request([(F.request.ISSUE, g[0])], [b"sig"]) for g in gi]
    reqs.append(F.request.token_request([(F.request.ISSUE, gi[0][0]), (F.request.TRANSFER, gt[0][0])], [b"sig"]))
    st, fa, fi = pp.verify_requests(reqs)
    want = [F.FTS_OK] * len(reqs)
    want[bad] = F.FTS_E_TAS_INVALID
    assert [int(s) for s in st] == want
    assert int(fa[bad]) == 0
    coms = [c for g in gt + gi for c in g[2]]
    metas = [m for g in gt + gi for m in g[1]]
    assert [int(s) for s in pp.check_metadata_openings(coms, metas)] == [F.FTS_OK] * len(coms)
    rot = metas[1:] + metas[:1]
    assert [int(s) for s in pp.check_metadata_openings(coms, rot)] == [F.FTS_E_OPEN_MISMATCH] * len(coms)
