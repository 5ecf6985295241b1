// Range-proof batch verification: the transcripts.  The x / y / x_j transcripts
// (k_rp_hash_small), the batch affine normalisation (it writes the H' records of the x0
// messages) and the x0 transcript (ipa.go:200-213).  launch_x0 is also the prover's entry
// to the transcript kernels (prove_kernels.hip).
// k_rp_hash_small is here and not with the other head kernels (rp_exact.hip) for the code
// the compiler emits: how it selects the inlined hex digits (transcript.hpp hex2) of
// k_rp_x0_build and k_rp_normalize depends on whether the unit also holds hash_raw_points;
// with it, all three compile as they did in one unit (tools/kernel_resources.py), without
// it k_rp_normalize takes 2 more SGPRs and 176 bytes.
#include "device/g1.hpp"
#include "device/fixed_base.hpp"
#include "device/glv.hpp"
#include "device/rp_kernels.hpp"
#include "device/rp_decls.hpp"
#include "device/transcript.hpp"
#include "device/helpers.hpp"
#include "../../include/fts_gpu.h"

namespace fts {

// -------------------------------------------------------------- challenges
// thread per (proof, message): message 0 = Arr(T1, T2) -> x; 1 = Arr(C, D, V)
// -> y; 2 + j = Arr(L_j, R_j) -> x_j  (bulletproof.go:266-281, ipa.go:230-235).
// Digests (canonical Fr) land in the challenge block, converted later.
__global__ void __launch_bounds__(64) k_rp_hash_small(int B, int n, int k, const uint8_t* __restrict__ raw,
                                                      const int32_t* __restrict__ status, uint32_t* __restrict__ ch,
                                                      uint8_t* __restrict__ small_msgs) {
  wave_prio<PS_HEAD>();
  const int nm = 2 + k;
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= B * nm) return;
  const int b = gid / nm, m = gid % nm;
  if (status[b] != 0) return;
  const uint8_t* P = raw + (size_t)b * rp_npts(k) * 64;
  uint8_t* slot = small_msgs + (size_t)gid * SMALL_SLOT;
  uint32_t* C = ch + (size_t)b * rp_nch(k) * 8;
  Fr h;
  int dst;
  if (m == 0) {
    const uint8_t* px[2] = {P + RP_PT_T1 * 64, P + RP_PT_T2 * 64};
    h = hash_raw_points(slot, px, 2);
    store_f(reinterpret_cast<uint32_t*>(slot), h);  // canonical x for k_rp_xd (runs beside k_rp_chal_fr)
    dst = CH_X;
  } else if (m == 1) {
    const uint8_t* py[3] = {P + RP_PT_C * 64, P + RP_PT_D * 64, P + RP_PT_V * 64};
    h = hash_raw_points(slot, py, 3);
    dst = CH_Y;
  } else {
    const int j = m - 2;
    const uint8_t* pl[2] = {P + (RP_PT_L + j) * 64, P + (RP_PT_L + k + j) * 64};
    h = hash_raw_points(slot, pl, 2);
    dst = CH_XJ + j;
  }
  store_f(C + dst * 8, h);  // canonical for now
}

// Batch affine normalisation (Montgomery's trick), E points per lane and ONE
// inversion per lane (point g of group g / per lives at index
// (g / per) * stride + g % per + first; points of proofs with status[g / per]
// != 0 are skipped, identities map to (0, 0)).  Lane l of wave w owns the points
// (w E + j) 64 + l, j < E (every load / store coalesced across the wave):
//   1. forward: the exclusive prefix product of the lane's z's, stored in the
//      point's own affine slot (scratch until step 2 overwrites it);
//   2. one inversion of the lane's product (f_inv_gcd, branch-free);
//   3. back-sweep: z_j^-1 = inv * prefix_j, inv *= z_j; then x z^-2, y z^-3.
// 7 products per point + one inversion per E points, no LDS and no barrier
// (round 5; the round-1..4 kernel scanned the lanes' totals across a 256-lane
// block in LDS and inverted once per block: ~13 products per point, 8 barrier
// levels and one lane inverting while the block waited -- 0.05-0.11 of the MAD
// peak beside the com chain).  Writes affine Montgomery (aff, 16 words) and,
// when be != nullptr, the canonical 64-byte BE encoding.
// x0 record r of a proof's message (ipa.go:200-213): hex(H'_r) + "||" at byte
// 8 + 130 r of its slot (bytes < 64 cb0 sit at their own offset), from the point's
// 16 BE words; 33 stores (4-byte ones where the record's parity allows)
FTS_DEV void x0_put_record(uint8_t* msg, uint32_t r, const uint32_t pw[16]) {
  uint8_t* d = msg + 8u + 130u * r;
  auto hx = [&](int i) -> uint32_t { return hex2((pw[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu); };  // byte i
  if ((r & 1u) == 0) {  // 4-byte aligned
    uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
#pragma unroll
    for (int i = 0; i < 32; i++) d4[i] = hx(2 * i) | (hx(2 * i + 1) << 16);
    reinterpret_cast<uint16_t*>(d)[64] = 0x7c7cu;
  } else {  // 2 mod 4: one 2-byte store, 31 aligned words, then hex(byte 63) "||"
    reinterpret_cast<uint16_t*>(d)[0] = (uint16_t)hx(0);
    uint32_t* d4 = reinterpret_cast<uint32_t*>(d + 2);
#pragma unroll
    for (int i = 0; i < 31; i++) d4[i] = hx(2 * i + 1) | (hx(2 * i + 2) << 16);
    d4[31] = hx(63) | (0x7c7cu << 16);
  }
}

template <int E>
__global__ void __launch_bounds__(NORM_BS) k_rp_normalize(int total, int per, int stride, int first,
                                                          const int32_t* __restrict__ status,
                                                          const uint32_t* __restrict__ jac, uint32_t* __restrict__ aff,
                                                          uint8_t* __restrict__ be, uint8_t* __restrict__ x0msgs) {
  wave_prio<PS_NORM>();
  const size_t gid = (size_t)blockIdx.x * NORM_BS + threadIdx.x;
  const size_t g0 = (gid >> 6) * (size_t)E * 64 + (gid & 63);
  auto slot = [&](int j) {
    const size_t g = g0 + (size_t)j * 64;
    return (g / per) * stride + g % per + first;
  };
  // liveness is read ONCE per point: status may change while this kernel runs
  // (k_sig_exclude on the batch-check stream marks excluded proofs NOT_RUN), and
  // the forward pass and the back-sweep must skip exactly the same points
  uint32_t livem = 0;
#pragma unroll
  for (int j = 0; j < E; j++) {
    const size_t g = g0 + (size_t)j * 64;
    if (g < (size_t)total && !(status && status[g / per] != 0)) livem |= 1u << j;
  }
  if (!livem) return;
  Fp run = f_one<FpP>();
#pragma unroll
  for (int j = 0; j < E; j++) {
    if (!((livem >> j) & 1u)) continue;
    const size_t q = slot(j);
    store_fp(aff + q * 16, run);  // exclusive prefix (scratch)
    Fp z;
    load_fp(jac + q * 24 + 16, z);
    if (!f_is_zero(z)) run = fp_mul(run, z);
  }
  Fp inv = nl_fp_inv(run);
#pragma unroll
  for (int j = E - 1; j >= 0; j--) {
    if (!((livem >> j) & 1u)) continue;
    const size_t q = slot(j);
    const G1J p = load_g1j(jac + q * 24);
    Fp pre;
    load_fp(aff + q * 16, pre);
    G1A r;
    if (f_is_zero(p.z)) {
      r.x = f_zero<FpP>();
      r.y = f_zero<FpP>();
    } else {
      const Fp zi = fp_mul(inv, pre);
      inv = fp_mul(inv, p.z);
      const Fp zi2 = fp_sqr(zi);
      r.x = fp_mul(p.x, zi2);
      r.y = fp_mul(fp_mul(p.y, zi2), zi);
    }
    store_g1a(aff + q * 16, r);
    if (be || x0msgs) {
      uint32_t pw[16];
      g1_mont_to_be_words(r.x, r.y, pw);
      if (be) {
        uint4* d = reinterpret_cast<uint4*>(be + q * 64);
#pragma unroll
        for (int w = 0; w < 4; w++)
          d[w] = make_uint4(__builtin_bswap32(pw[4 * w]), __builtin_bswap32(pw[4 * w + 1]),
                            __builtin_bswap32(pw[4 * w + 2]), __builtin_bswap32(pw[4 * w + 3]));
      }
      // the x0 prefix's hex record of this point (H'_r of proof g / per)
      if (x0msgs) {
        const size_t g = g0 + (size_t)j * 64;
        x0_put_record(x0msgs + (g / per) * x0_var_bytes(per), (uint32_t)(g % per), pw);
      }
    }
  }
}

// ------------------------------------------------------------ host launch
void launch_normalize(size_t total, int per, int stride, int first, const int32_t* status, const uint32_t* jac,
                      uint32_t* aff, uint8_t* be, hipStream_t s, uint8_t* x0msgs) {
  // lanes: one per E points, rounded to whole waves (E * 64 points per wave)
  if (total >= NORM_BIG)
    FTS_LAUNCH(k_rp_normalize<16>, (total + 16 * 64 - 1) / (16 * 64) * 64, NORM_BS, s, (int)total, per, stride, first,
               status, jac, aff, be, x0msgs);
  else
    FTS_LAUNCH(k_rp_normalize<4>, (total + 4 * 64 - 1) / (4 * 64) * 64, NORM_BS, s, (int)total, per, stride, first,
               status, jac, aff, be, x0msgs);
}

void launch_normalize_all(int total, const uint32_t* jac, uint32_t* aff, hipStream_t s) {
  launch_normalize(total, 1, 1, 0, (const int32_t*)nullptr, jac, aff, (uint8_t*)nullptr, s);
}

// --------------------------------------------------------- x0 transcript
// The x0 message DER(SEQUENCE{OCTET(Arr(H'_0..H'_{n-1}, G_0..G_{n-1}, Q, com)),
// OCTET("||"), OCTET(Zb(ip))}) + SHA-256 padding (ipa.go:200-213) as 16-bit
// units (2 hex chars, "||", DER bytes, padding; first byte in the low half).
struct X0Src {
  const uint8_t* hp;     // this proof's n+1 canonical BE points (H'..., com)
  const uint16_t* cst;   // hex(G_0) "||" ... hex(Q) "||"
  const uint32_t* ip;    // Zb(ip): canonical LE limbs
  uint32_t A, len, end;  // array length, message length, padded length (bytes)
  int n;
};
FTS_DEV uint32_t x0_unit(const X0Src& m, uint32_t u) {
  const uint32_t pos = 2u * u;
  if (pos < 8) {  // 30 82 L L 04 82 A A
    const uint32_t L = m.A + 42u;
    return pos == 0 ? 0x8230u : pos == 2 ? ((L >> 8) | ((L & 0xffu) << 8)) : pos == 4 ? 0x8204u
                                                                           : ((m.A >> 8) | ((m.A & 0xffu) << 8));
  }
  uint32_t off = pos - 8u;
  if (off < m.A) {
    const uint32_t r = off / 130u, o = off - 130u * r;
    if (r >= (uint32_t)m.n && r <= 2u * m.n) return m.cst[(130u * (r - m.n) + o) >> 1];
    if (o == 128u) return 0x7c7cu;
    return hex2(m.hp[(r < (uint32_t)m.n ? r : (uint32_t)m.n) * 64u + (o >> 1)]);
  }
  off -= m.A;
  if (off < 38u) {  // 04 02 "||" 04 20 Zb(ip)
    if (off < 6u) return off == 0 ? 0x0204u : off == 2 ? 0x7c7cu : 0x2004u;
    const uint32_t k = off - 6u;  // even byte index into Zb(ip)
    const uint32_t wd = m.ip[7 - (k >> 2)];
    return (k & 2u) ? (((wd >> 8) & 0xffu) | ((wd & 0xffu) << 8)) : ((wd >> 24) | (((wd >> 16) & 0xffu) << 8));
  }
  if (pos == m.len) return 0x0080u;
  if (pos >= m.end - 8u) {  // 64-bit big-endian bit length
    const uint64_t bits = (uint64_t)m.len * 8u;
    const uint32_t k = pos - (m.end - 8u);  // 0, 2, 4, 6
    const uint32_t b0 = (uint32_t)(bits >> (56 - 8 * k)) & 0xffu, b1 = (uint32_t)(bits >> (48 - 8 * k)) & 0xffu;
    return b0 | (b1 << 8);
  }
  return 0u;
}

// One wave per proof, X0_PPB proofs per block: the proof's variable message
// blocks (everything but the shared template blocks) are assembled in the
// wave's LDS region -- hex records of H'_i and com (one 16-byte quarter of a
// point per work item), the DER header, the constant bytes that share a block
// with variable ones, Zb(ip) and the SHA-256 padding -- then written to the
// compact slot with coalesced uint4 stores.  (One 256-thread block per proof,
// rounds 1-3, launched 4x the waves for the same work: at 81,920 proofs the
// launch's span beside the com chain was 5.8-6.8 ms.)
// LDS offset of message byte `pos` (outside the template blocks):
FTS_DEV uint32_t x0_lds_off(uint32_t pos, uint32_t cb0, uint32_t cb1) {
  return pos < 64u * cb0 ? pos : pos - 64u * (cb1 - cb0);
}
// part: 2 = every variable block; 0 = the blocks before the shared template
// (header, H'_0..H'_{n-1}: available right after their normalisation); 1 = the
// blocks after it (com, DER tail, Zb(ip), padding).  Parts 0 and 1 write
// disjoint byte ranges of the proof's slot.
__global__ void __launch_bounds__(64 * X0_PPB) k_rp_x0_build(int B, int n, const int32_t* __restrict__ status,
                                                            const uint8_t* __restrict__ hp_be,
                                                            const uint8_t* __restrict__ x0_const,
                                                            const uint32_t* __restrict__ sc, uint8_t* __restrict__ msgs,
                                                            int part) {
  wave_prio<PS_X0TAIL>();
  extern __shared__ uint4 x0_lds[];
  const uint32_t A = x0_array_len(n), len = x0_msg_len(n), end = x0_slot_bytes(n);
  const uint32_t cb0 = x0_cb0(n), cb1 = x0_cb1(n), var = x0_var_bytes(n);
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * X0_PPB + wv;
  const bool live = b < B && status[b] == 0;  // uniform per wave
  // part 1 assembles only bytes >= 64 cb0 (its LDS region starts there)
  const uint32_t lbase = part == 1 ? 64u * cb0 : 0u;
  uint4* L4 = x0_lds + (size_t)wv * ((var - lbase) / 16u);
  uint8_t* Lb = reinterpret_cast<uint8_t*>(L4) - lbase;
  const uint32_t c_off = x0_const_off(n), c_end = x0_const_end(n);
  const uint8_t* hp = hp_be + (size_t)b * (n + 1) * 64;
  // hex records: H'_0..H'_{n-1} (records 0..n-1) and com (record 2n+1, no "||")
  const int r_lo = part == 1 ? n : 0, r_hi = part == 0 ? n : n + 1;  // records of this part
  for (int it = lane + 4 * r_lo; live && it < r_hi * 4; it += 64) {
    const int r = it >> 2, q = it & 3;
    const uint4 v = *reinterpret_cast<const uint4*>(hp + r * 64 + q * 16);
    const uint32_t rec = r < n ? (uint32_t)r : 2u * n + 1u;
    uint16_t* d = reinterpret_cast<uint16_t*>(Lb + x0_lds_off(8u + 130u * rec + 32u * q, cb0, cb1));
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; j++) d[j] = hex2((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
    if (q == 3 && r < n) d[16] = 0x7c7cu;
  }
  // header, constant bytes in variable blocks, trailer (DER tail, Zb(ip), padding, length)
  const uint32_t* ip = sc + ((size_t)(live ? b : 0) * RP_NSC + RP_SC_IP) * 8;
  const uint32_t t0 = 8u + A;
  auto put = [&](uint32_t pos) {
    uint32_t v;
    if (pos < 8u) {  // 30 82 L L 04 82 A A
      const uint32_t L = A + 42u;
      const uint8_t h[8] = {0x30, 0x82, (uint8_t)(L >> 8), (uint8_t)L, 0x04, 0x82, (uint8_t)(A >> 8), (uint8_t)A};
      v = h[pos];
    } else if (pos >= c_off && pos < c_end) {
      v = x0_const[pos - c_off];
    } else if (pos < t0 + 6u) {  // 04 02 "||" 04 20
      const uint8_t h[6] = {0x04, 0x02, 0x7c, 0x7c, 0x04, 0x20};
      v = h[pos - t0];
    } else if (pos < len) {  // Zb(ip): big-endian bytes of the canonical LE limbs
      const uint32_t k = pos - t0 - 6u;
      v = (ip[7 - (k >> 2)] >> (24 - 8 * (k & 3u))) & 0xffu;
    } else if (pos == len) {
      v = 0x80u;
    } else if (pos >= end - 8u) {
      v = (uint32_t)(((uint64_t)len * 8u) >> (8 * (end - 1u - pos))) & 0xffu;
    } else {
      v = 0u;
    }
    Lb[x0_lds_off(pos, cb0, cb1)] = (uint8_t)v;
  };
  const uint32_t nh = 8u, nc0 = 64u * cb0 - c_off, nc1 = c_end - 64u * cb1, nt = end - t0;
  // part 0: header + constants before the template; part 1: constants after it + trailer
  const uint32_t i_lo = part == 1 ? nh + nc0 : 0u, i_hi = part == 0 ? nh + nc0 : nh + nc0 + nc1 + nt;
  for (uint32_t it = lane + i_lo; live && it < i_hi; it += 64) {
    uint32_t pos;
    if (it < nh) pos = it;
    else if (it < nh + nc0) pos = c_off + (it - nh);
    else if (it < nh + nc0 + nc1) pos = 64u * cb1 + (it - nh - nc0);
    else pos = t0 + (it - nh - nc0 - nc1);
    put(pos);
  }
  __syncthreads();
  if (!live) return;
  uint4* dst = reinterpret_cast<uint4*>(msgs + (size_t)b * var);
  const uint32_t c_lo = part == 1 ? 4u * cb0 : 0u, c_hi = part == 0 ? 4u * cb0 : var / 16u;
  for (uint32_t c = lane + c_lo; c < c_hi; c += 64) dst[c] = L4[c - lbase / 16u];
}

// The bytes of part 0 of the x0 message that are not H' records (the DER header
// and the constant bytes sharing block cb0 - 1 with the last record), lane per
// proof; the records themselves are written by k_rp_normalize (x0msgs) as it
// normalises H' (round 5: a separate LDS-assembled build of part 0 waited for CU
// slots beside the com chain, and the x0 prefix it feeds became the pass's
// critical path, 0.4 -> 5.2 ms)
__global__ void __launch_bounds__(256) k_rp_x0_hdr(int B, int n, const int32_t* __restrict__ status,
                                                   const uint8_t* __restrict__ x0_const, uint8_t* __restrict__ msgs) {
  wave_prio<PS_NORM>();
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || status[b] != 0) return;
  uint8_t* msg = msgs + (size_t)b * x0_var_bytes(n);
  const uint32_t A = x0_array_len(n), L = A + 42u;
  const uint8_t h[8] = {0x30, 0x82, (uint8_t)(L >> 8), (uint8_t)L, 0x04, 0x82, (uint8_t)(A >> 8), (uint8_t)A};
#pragma unroll
  for (int i = 0; i < 8; i++) msg[i] = h[i];
  const uint32_t c_off = x0_const_off(n), c_end = 64u * x0_cb0(n);
  for (uint32_t pos = c_off; pos < c_end; pos++) msg[pos] = x0_const[pos - c_off];
}

// SHA-256 over message blocks [b0, b1) of each proof's x0 message: b0 == 0
// starts from the initial state, else from mid[b]; b1 == every block finishes
// (x0 = HashToZr -> ch), else the state is left in mid[b].  The whole hash
// (0, all) or its prefix (0, cb1: H' records + the shared template, started
// while com is still being computed) and suffix (cb1, all).
__global__ void __launch_bounds__(256) k_rp_x0_hash(int B, int n, int k, const int32_t* __restrict__ status,
                                                   const uint8_t* __restrict__ msgs, const uint8_t* __restrict__ tmpl,
                                                   uint32_t b0, uint32_t b1, uint32_t* __restrict__ mid,
                                                   uint32_t* __restrict__ ch) {
  // the suffix is the pass's short tail; the prefix runs beside the com chain
  if (b0 != 0)
    wave_prio<PS_X0TAIL>();
  else
    wave_prio<PS_X0PRE>();
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || status[b] != 0) return;
  const uint32_t cb0 = x0_cb0(n), cb1 = x0_cb1(n), nb = sha_blocks(x0_msg_len(n));
  const uint32_t hi = b1 < nb ? b1 : nb;
  const uint4* own = reinterpret_cast<const uint4*>(msgs + (size_t)b * x0_var_bytes(n));
  uint32_t st[8];
  if (b0 == 0) {
    sha256_init(st);
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = mid[(size_t)b * 8 + i];
  }
  // one block ahead: the next block's 64 bytes are loaded before this block's
  // 64 rounds, so the load's latency (L2 / HBM, ~1 us under load) is hidden
  // behind them instead of exposed once per block
  const uint4* shared = reinterpret_cast<const uint4*>(tmpl);
  auto block_ptr = [&](uint32_t blk) {
    return blk < cb0 ? own + 4u * blk : blk < cb1 ? shared + 4u * (blk - cb0) : own + 4u * (blk - (cb1 - cb0));
  };
  uint4 nx[4];
  if (b0 < hi) {
    const uint4* m = block_ptr(b0);
#pragma unroll
    for (int i = 0; i < 4; i++) nx[i] = m[i];
  }
  for (uint32_t blk = b0; blk < hi; blk++) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      w[4 * i + 0] = __builtin_bswap32(nx[i].x);
      w[4 * i + 1] = __builtin_bswap32(nx[i].y);
      w[4 * i + 2] = __builtin_bswap32(nx[i].z);
      w[4 * i + 3] = __builtin_bswap32(nx[i].w);
    }
    if (blk + 1 < hi) {
      const uint4* m = block_ptr(blk + 1);
#pragma unroll
      for (int i = 0; i < 4; i++) nx[i] = m[i];
    }
    sha256_compress(st, w);
  }
  if (hi < nb) {
#pragma unroll
    for (int i = 0; i < 8; i++) mid[(size_t)b * 8 + i] = st[i];
    return;
  }
  store_f(ch + ((size_t)b * rp_nch(k) + CH_X0) * 8, f_to_mont(digest_to_fr(st)));
}

// x0 = Hz(DER(Arr(H'..., G..., Q, com), "||", Zb(ip))) for B proofs whose
// H'/com BE points are in hp_be and ip in sc (RP_SC_IP): the prover's entry
// to the same transcript kernels (prove_kernels.hip)
void launch_x0(int B, int n, int k, const int32_t* status, const uint8_t* hp_be, const uint8_t* x0_const,
               const uint8_t* x0_tmpl, const uint32_t* sc, uint8_t* msgs, uint32_t* ch, hipStream_t s) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_rp_x0_build, dim3(x0_build_grid(B)), dim3(64 * X0_PPB), x0_build_lds(n), s, B, n, status, hp_be, x0_const, sc, msgs, 2);
  FTS_LAUNCH(k_rp_x0_hash, B, g_lat_bs, s, B, n, k, status, msgs, x0_tmpl, 0u, 0xffffffffu, (uint32_t*)nullptr, ch);
}

hipError_t upload_wave_prio_rp_x0(const int* p) { return upload_wave_prio(p); }

}  // namespace fts
