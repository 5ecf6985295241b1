// Minimal protobuf wire reader shared by the idemix host code (nym signatures,
// identity proofs): Go proto.Unmarshal failure modes -- truncation, varint
// overflow (protowire.ConsumeVarint), field 0 / numbers above 2^29 - 1, wire
// types 6 and 7, an end-group marker without its start.  Unknown groups
// (wire type 3 ... matching 4) are skipped as protowire.ConsumeFieldValue
// does; a known field with the wrong wire type is rejected by the callers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace fts {

struct Pb {
  const uint8_t* p;
  size_t n, o = 0;
  // protowire.ConsumeVarint: at most 10 bytes, and the 10th may only carry bit 63
  bool varint(uint64_t& v) {
    v = 0;
    for (int sh = 0; sh < 64; sh += 7) {
      if (o >= n) return false;
      const uint8_t c = p[o++];
      if (sh == 63 && c > 1) return false;  // overflow
      v |= (uint64_t)(c & 0x7f) << sh;
      if (!(c & 0x80)) return true;
    }
    return false;
  }
  // the value of a field with wire type wt (key already read); groups nest up to
  // `depth` levels (protowire's recursion limit is far above any real message)
  bool skip_value(uint32_t f, uint32_t wt, int depth = 0) {
    uint64_t x;
    switch (wt) {
      case 0: return varint(x);
      case 1: if (n - o < 8) return false; o += 8; return true;
      case 5: if (n - o < 4) return false; o += 4; return true;
      case 2: if (!varint(x) || x > n - o) return false; o += (size_t)x; return true;
      case 3: {  // start group: fields until the end group of the same number
        if (depth >= 64) return false;
        for (;;) {
          uint64_t key;
          if (!varint(key)) return false;
          const uint32_t gf = (uint32_t)(key >> 3), gw = (uint32_t)(key & 7);
          if (gf == 0 || (key >> 3) > 0x1fffffff) return false;
          if (gw == 4) return gf == f;
          if (!skip_value(gf, gw, depth + 1)) return false;
        }
      }
      default: return false;  // 4 (end group without a start), 6, 7
    }
  }
  // next field: number, wire type, value span (bytes) / varint; groups are skipped
  // (v = nullptr, vl = 0) and reported with wt = 3
  struct Field {
    uint32_t f, wt;
    const uint8_t* v;
    size_t vl;
    uint64_t iv;
  };
  bool next(Field& d) {
    uint64_t key;
    if (!varint(key)) return false;
    d.f = (uint32_t)(key >> 3), d.wt = (uint32_t)(key & 7);
    if (d.f == 0 || (key >> 3) > 0x1fffffff) return false;
    d.v = nullptr, d.vl = 0, d.iv = 0;
    switch (d.wt) {
      case 0: return varint(d.iv);
      case 1: if (n - o < 8) return false; d.v = p + o, d.vl = 8, o += 8; return true;
      case 5: if (n - o < 4) return false; d.v = p + o, d.vl = 4, o += 4; return true;
      case 2: {
        uint64_t l;
        if (!varint(l) || l > n - o) return false;
        d.v = p + o, d.vl = (size_t)l, o += (size_t)l;
        return true;
      }
      case 3: return skip_value(d.f, 3);
      default: return false;
    }
  }
};

// a length-delimited field's bytes, and whether the field was seen
struct Span {
  const uint8_t* p = nullptr;
  size_t n = 0;
  bool set = false;
};

// ECP{1 x, 2 y} -> X || Y (64 raw bytes); false if the field is absent, the message
// malformed or a coordinate not 32 bytes.  x or y with the wrong wire type: rejected
// if `strict` (the Signature's points), otherwise ignored (the issuer key's bases)
inline bool ecp_xy(const Span& s, uint8_t out[64], bool strict) {
  if (!s.set) return false;
  Pb pb{s.p, s.n};
  Pb::Field d;
  Span c[3];
  while (pb.o < pb.n) {
    if (!pb.next(d)) return false;
    if (d.f != 1 && d.f != 2) continue;
    if (d.wt == 2) c[d.f] = Span{d.v, d.vl, true};
    else if (strict) return false;
  }
  if (c[1].n != 32 || c[2].n != 32) return false;
  memcpy(out, c[1].p, 32);
  memcpy(out + 32, c[2].p, 32);
  return true;
}
// ECP2{1..4: four 32-byte coordinates} -> 128 raw bytes, strict as above
inline bool ecp2_raw(const Span& s, uint8_t out[128]) {
  if (!s.set) return false;
  Pb pb{s.p, s.n};
  Pb::Field d;
  Span c[5];
  while (pb.o < pb.n) {
    if (!pb.next(d)) return false;
    if (d.f < 1 || d.f > 4) continue;
    if (d.wt != 2) return false;
    c[d.f] = Span{d.v, d.vl, true};
  }
  for (int q = 1; q <= 4; q++) {
    if (c[q].n != 32) return false;
    memcpy(out + 32 * (q - 1), c[q].p, 32);
  }
  return true;
}

}  // namespace fts
