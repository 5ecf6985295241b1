"""Builders of the SerializedIdemixIdentity wire edge cases, shared by the GPU
test of the identity verifier (test_idemix_identity.py) and the host-only check
of its parser (test_lib_cpu.py)."""
from oracle import idemix as OI


def _key(f, wt):
    k, out = (f << 3) | wt, b""
    while True:
        c = k & 0x7F
        k >>= 7
        out += bytes([c | (0x80 if k else 0)])
        if not k:
            return out


def _overlong(f, wt, last):
    """the key of (f, wt) as a 10-byte varint whose last byte is `last`"""
    k = (f << 3) | wt
    body = [(k >> (7 * i)) & 0x7F for i in range(9)]
    return bytes(b | 0x80 for b in body) + bytes([last])


def wire_edge_cases(raw, malformed):
    """eight re-encodings of the honest identity `raw` as (bytes, wanted status):
    0 where the encoding parses, `malformed` where it does not"""
    fields = OI.pb_fields(raw)
    rebuilt = b"".join(OI.pb_bytes_field(f, v) for f, wt, v in fields)
    assert rebuilt == raw and all(wt == 2 for _, wt, _ in fields)

    def with_key(i, key):
        out = b""
        for j, (f, wt, v) in enumerate(fields):
            enc = OI.pb_bytes_field(f, v)
            out += (key + enc[len(_key(f, 2)):]) if j == i else enc
        return out
    group = _key(100, 3) + _key(1, 0) + b"\x05" + _key(2, 2) + b"\x01Z" + _key(100, 4)
    return [
        (with_key(0, _overlong(fields[0][0], 2, 0x00)), 0),                        # overlong, no overflow
        (with_key(0, _overlong(fields[0][0], 2, 0x02)), malformed),                # 10th byte > 1: overflow
        (with_key(len(fields) - 1, _overlong(fields[-1][0], 2, 0x7F)), malformed),
        (raw + group, 0),                                                          # unknown group skipped
        (group + raw, 0),
        (raw + _key(100, 3) + _key(1, 0) + b"\x05", malformed),                    # group without its end
        (raw + _key(100, 3) + _key(101, 4), malformed),                            # mismatched end group
        (raw + _key(100, 4), malformed),                                           # end group alone
    ]
