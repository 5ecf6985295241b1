// C-ABI (include/fts_gpu.h): the idemix verifiers -- pseudonym signatures
// (fts_idemix_ipk, idemix_kernels.hip), the identities' association proofs
// (fts_idemix_idv, idemix_identity_{bn,fbn}.hip) and, on the same handle, credentials
// (idemix_cred_{bn,fbn}.hip).  Handles, slots and staging; the untrusted bytes are parsed
// by host/idemix_parse.hpp and host/identity_write.hpp, the kernels are reached through
// device/launch.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/fts_gpu.h"
#include "device/launch.hpp"
#include "host/bn254_host.hpp"
#include "host/hip_owned.hpp"
#include "host/host_pool.hpp"
#include "host/idemix_parse.hpp"
#include "host/identity_write.hpp"  // parse_credential
#include "host/prover.hpp"  // Rng, RngSource: the signer's nonces
#include "host/sign_encode.hpp"

using namespace fts;
using namespace idv;

#define ICHK(x)                                    \
  do {                                             \
    if ((x) != hipSuccess) return FTS_API_EDEVICE; \
  } while (0)

namespace {

constexpr int NYM_NSLOT = 3;
// items per nym-kernel launch (the GLV lane tables are sized for one tile)
constexpr size_t NYM_TILE = 262144;
struct NymSlot {
  Stream stream;
  DevBuf d_buf;  // rec | nym | moff | mlen | status | vtab | messages
  PinBuf h_buf;  // pinned staging of everything above but vtab
  Event ev[2];
  float ms = 0.f;
  float sign_ms = 0.f;
};

constexpr int IDV_NSLOT = 8;  // calls in flight per handle (each slot: its own stream and buffers, grown on first use;
                              // 12 concurrent calls hit HSA_STATUS_ERROR_OUT_OF_RESOURCES dispatching the
                              // scratch-using pairing kernels, gpurun_out/ns)
struct IdvSlot {
  Stream stream;
  DevBuf d_buf;
  PinBuf h_buf;
  Event ev[3];
  float ms[2] = {0.f, 0.f};
  uint32_t stats[2] = {0u, 0u};
  // credential calls take these slots too (one bound on the pairing stages in flight) and
  // keep their figures apart from the identity calls'
  float cred_ms[2] = {0.f, 0.f};
  uint32_t cred_stats[2] = {0u, 0u};
};
// credentials per kernel sequence of fts_idemix_cred_verify_batch: bounds what a call asks a
// slot for (2.5 KB of device memory per credential, 42 MB) and still puts 1,792 waves on
// the device in k_cred_var
constexpr size_t CRV_TILE = 16384;

constexpr int AUD_NSLOT = 3;  // audit-match calls in flight per handle, beside the identity slots
struct AuditSlot {
  Stream stream;
  DevBuf d_buf;  // pts | rnd | aoff | alen | pre | rh_pre | strings | half_st
  PinBuf h_buf;  // pinned staging of the same layout
  Event ev[2];
  float ms = 0.f;
};

// 32 bytes -> 8 big-endian words
void be_words(const uint8_t h[32], uint32_t hw[8]) {
  for (int q = 0; q < 8; q++)
    hw[q] = ((uint32_t)h[4 * q] << 24) | ((uint32_t)h[4 * q + 1] << 16) | ((uint32_t)h[4 * q + 2] << 8) | h[4 * q + 3];
}

// nb issuer bases (X || Y, 64 raw bytes each) -> 16 words each for the table build: BN254
// Montgomery (decoded and on-curve checked here, not the identity); FP256BN plain LE limbs
// (checked on the device)
bool base_words(bool bn, const uint8_t (*raw)[64], int nb, uint32_t* bases) {
  for (int b = 0; b < nb; b++) {
    if (bn) {
      host::G1A a;
      if (!host::g1_from_bytes(raw[b], 64, a) || a.inf) return false;
      memcpy(&bases[b * 16], a.x.v, 32);
      memcpy(&bases[b * 16 + 8], a.y.v, 32);
    } else {
      u256::be_limbs(raw[b], 32, &bases[b * 16]);
      u256::be_limbs(raw[b] + 32, 32, &bases[b * 16 + 8]);
    }
  }
  return true;
}

// Fr (Montgomery) -> canonical LE limbs
void fr_canon(const host::Fr& a, uint32_t out[8]) {
  uint64_t c[4];
  host::from_mont(a, c);
  for (int i = 0; i < 4; i++) out[2 * i] = (uint32_t)c[i], out[2 * i + 1] = (uint32_t)(c[i] >> 32);
}

}  // namespace

struct fts_idemix_ipk {
  int device = -1;
  int curve = 1;                 // mathlib CurveID: 1 BN254, 0 FP256BN_AMCL
  DevBuf d_tables;               // HSk, HRand (FB_W-bit windows)
  DevBuf d_hash;                 // ipk.Hash as 8 big-endian words
  uint8_t hash[32];
  SlotRing<NymSlot, NYM_NSLOT> ring;
  float last_ms = 0.f;     // under ring.mu
  float last_sign_ms = 0.f;  // under ring.mu
  size_t tile = NYM_TILE;  // items per launch (FTS_NYM_TILE overrides, for tests)
  ~fts_idemix_ipk() {
    if (device >= 0) (void)hipSetDevice(device);
  }
};

struct fts_idemix_idv {
  int device = -1;
  int curve = 1;
  DevBuf d_tables;  // HSk, HRand, HAttrs[0..3], g1
  DevBuf d_lines;   // lines of W, then of g2
  DevBuf d_hash;    // ipk.Hash as 8 big-endian words, then HSk as X || Y (16): the credential-request transcript
  // BarG1 then BarG2 of the key as X || Y (an issuer handle checks its secret against them)
  uint8_t bar[128];
  bool has_bar = false;
  CredReqState* creq = nullptr;  // slots of the credential-request calls (api_credissue.cpp)
  SlotRing<IdvSlot, IDV_NSLOT> ring;  // its lock also guards last_* and g2_seen
  float last_ms[2] = {0.f, 0.f};
  // batch pairing check (k_idv_bp_*; FTS_IDV_BATCH=0 pairs every identity, the A/B
  // and pre-round-6 path); last call's groups and identities paired one by one
  bool batch = true;
  uint32_t last_stats[2] = {0u, 0u};
  // the last credential batch (fts_idemix_cred_verify_batch), under the ring's lock
  float last_cred_ms[2] = {0.f, 0.f};
  uint32_t last_cred_stats[2] = {0u, 0u};
  // BN254 epoch keys already subgroup-checked by this context (128 raw bytes ->
  // verdict): an honest stream carries one key per epoch, and k_idv_g2_check is
  // one 254-step G2 chain on one lane (7.7 ms, on the call's critical path)
  std::unordered_map<std::string, int32_t> g2_seen;
  // audit info matching (fts_idemix_audit_match_batch): slots of its own, so a match
  // never waits for (or holds) an identity-verification slot
  SlotRing<AuditSlot, AUD_NSLOT> aud;
  float aud_ms = 0.f;  // under aud.mu
  ~fts_idemix_idv() {
    if (device >= 0) (void)hipSetDevice(device);
    credreq_state_free(creq);
  }
};

// what a credential handle borrows from its identity verifier (api_idgen.cpp), and an issuer
// handle and the credential-request calls (api_credissue.cpp)
namespace idv {
IdvView idv_view(const fts_idemix_idv* k) {
  return IdvView{k->device, k->curve, k->d_tables.as<uint32_t>(), k->d_hash.as<uint32_t>()};
}
IssuerView idv_issuer_view(const fts_idemix_idv* k) {
  return IssuerView{idv_view(k), k->creq, k->has_bar ? k->bar : nullptr};
}
}  // namespace idv

extern "C" {

// ---------------------------------------------------------------------------
// Pseudonym signatures
// ---------------------------------------------------------------------------
int fts_idemix_ipk_create(int device, const uint8_t* ipk, size_t ipk_len, int curve_id, fts_idemix_ipk** out) {
  if (!out || !ipk || !ipk_len || (curve_id != FTS_CURVE_BN254 && curve_id != FTS_CURVE_FP256BN_AMCL))
    return FTS_API_EINVAL;
  *out = nullptr;
  const bool bn = curve_id == FTS_CURVE_BN254;
  IpkFields f;  // this verifier needs h_sk and h_rand only
  uint8_t raw[2][64];
  uint32_t hb[32];
  if (!parse_ipk(ipk, ipk_len, f) || !ecp_xy(f.h_sk, raw[0], false) || !ecp_xy(f.h_rand, raw[1], false) ||
      !base_words(bn, raw, 2, hb))
    return FTS_API_EPP;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FTS_API_EDEVICE;
  std::unique_ptr<fts_idemix_ipk> k(new fts_idemix_ipk());
  k->device = device;
  k->curve = curve_id;
  if (const char* e = getenv("FTS_NYM_TILE")) k->tile = (size_t)std::max(64L, std::min((long)NYM_TILE, atol(e)));
  ipk_hash32(f, k->hash);
  if (hipSetDevice(device) != hipSuccess) return FTS_API_EDEVICE;
  uint32_t hw[8];
  be_words(k->hash, hw);
  DevBuf bases_buf, scr_buf;
  Stream s0;
  const size_t tab_b = 2 * (bn ? fb_words_per_base() : fbn_words_per_base()) * 4;
  const size_t scr_b = bn ? table_build_scratch_bytes(2) : 2 * 16 * 4 + 64;
  bool ok = s0.create() == hipSuccess && k->d_tables.reserve(tab_b) && k->d_hash.reserve(32) &&
            bases_buf.reserve(sizeof(hb)) && scr_buf.reserve(scr_b);
  uint32_t* const d_tables = k->d_tables.as<uint32_t>();
  uint32_t* const d_bases = bases_buf.as<uint32_t>();
  uint32_t* const d_scr = scr_buf.as<uint32_t>();
  ok = ok && hipMemcpyAsync(d_bases, hb, sizeof(hb), hipMemcpyHostToDevice, s0) == hipSuccess &&
       hipMemcpyAsync(k->d_hash.p, hw, 32, hipMemcpyHostToDevice, s0) == hipSuccess;
  bool on_curve = true;
  if (ok && bn) {
    launch_build_tables(d_bases, 2, d_tables, d_scr, s0);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s0) == hipSuccess;
  } else if (ok) {
    // plain -> Montgomery + on-curve flags (into the scratch), then the window tables
    int32_t* flags = reinterpret_cast<int32_t*>(d_scr + 32);
    int32_t hf[2] = {0, 0};
    fbn_build_tables(d_bases, 2, d_scr, flags, d_tables, s0);
    ok = hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, s0) == hipSuccess &&
         hipStreamSynchronize(s0) == hipSuccess;
    on_curve = hf[0] == 1 && hf[1] == 1;
  }
  if (s0) (void)hipStreamSynchronize(s0);  // an error path may leave copies queued on s0
  if (ok && !on_curve) return FTS_API_EPP;
  for (auto& S : k->ring.slot) {
    ok = ok && S.stream.create() == hipSuccess;
    for (auto& e : S.ev) ok = ok && e.create() == hipSuccess;
  }
  if (!ok) return FTS_API_EDEVICE;
  *out = k.release();
  return FTS_API_OK;
}

void fts_idemix_ipk_destroy(fts_idemix_ipk* k) { delete k; }

int fts_idemix_identity_nym(const uint8_t* id, size_t len, const uint8_t** nym, size_t* nym_len) {
  if (!id || !nym || !nym_len) return FTS_API_EINVAL;
  Pb pb{id, len};
  Pb::Field d;
  *nym = nullptr, *nym_len = 0;
  while (pb.o < pb.n) {
    if (!pb.next(d)) return FTS_API_EINVAL;
    if (d.f == 1) {
      if (d.wt != 2) return FTS_API_EINVAL;
      *nym = d.v, *nym_len = d.vl;
    }
  }
  return *nym_len ? FTS_API_OK : FTS_API_EINVAL;  // crypto/deserializer.go:45-47: empty nym rejected
}

int fts_nym_verify_batch(fts_idemix_ipk* K, size_t n, const fts_nym_item* items, int32_t* status) {
  if (!K || n > (size_t)(1u << 24) || (n && (!items || !status))) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  // message words per item (nym_stream_words): BN254 the message alone; FP256BN the
  // whole hashed stream
  const bool bn = K->curve == FTS_CURVE_BN254;
  size_t mtot_w = 0;
  for (size_t i = 0; i < n; i++) {
    if (items[i].msg_len > 0xffffff00u || (items[i].msg_len && !items[i].msg)) return FTS_API_EINVAL;
    mtot_w += nym_stream_words(bn, items[i].msg_len);
  }
  auto guard = K->ring.acquire([K](NymSlot& S) { K->last_ms = S.ms; });
  NymSlot& D = guard.slot();
  ICHK(hipSetDevice(K->device));
  // layout: rec | nym | moff | mlen | status | messages (| vtab on the device only)
  const size_t rec_b = n * NREC * 4, nym_b = n * 64, off_b = n * 8, len_b = n * 4, st_b = n * 4;
  const size_t o_nym = rec_b, o_off = o_nym + nym_b, o_len = o_off + off_b, o_st = o_len + len_b,
               o_msg = (o_st + st_b + 255) & ~size_t(255), h_need = o_msg + mtot_w * 4;
  // GLV lane tables (16 Jacobian entries, 1,536 B per lane) for one tile of NYM_TILE
  // items: bounded at 384 MiB per slot whatever n is; a call above NYM_TILE items
  // runs one launch per tile on the slot's stream (a 2^24-item call
  // asked for ~38 GB here)
  const size_t tile = std::min<size_t>(n, K->tile);
  const size_t vt_b = tile * 16 * 24 * 4, o_vt = (h_need + 255) & ~size_t(255), d_need = o_vt + vt_b;
  if (D.h_buf.cap < h_need && !D.h_buf.reserve(h_need + h_need / 2)) return FTS_API_ENOMEM;
  if (D.d_buf.cap < d_need && !D.d_buf.reserve(d_need + d_need / 2)) return FTS_API_ENOMEM;
  uint8_t* h = D.h_buf.as<uint8_t>();
  uint64_t* hoff = reinterpret_cast<uint64_t*>(h + o_off);
  {
    uint64_t o = 0;
    for (size_t i = 0; i < n; i++) hoff[i] = o, o += nym_stream_words(bn, items[i].msg_len);
  }
  auto pack = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      const fts_nym_item& it = items[i];
      int32_t st = parse_nym_sig(it.sig, it.sig_len, bn, reinterpret_cast<uint32_t*>(h) + i * NREC);
      // NymPublicKey import precedes Verify: a key of the wrong length / form fails first
      if (!pack_nym_item(bn, it.nym, it.nym_len, K->hash, it.msg, it.msg_len, h + o_nym + i * 64,
                         h + o_msg + hoff[i] * 4, reinterpret_cast<uint32_t*>(h + o_len) + i))
        st = FTS_E_NYM_BADKEY;
      reinterpret_cast<int32_t*>(h + o_st)[i] = st;
    }
  };
  const size_t CH = 2048, nch = (n + CH - 1) / CH;
  host_parallel_for(nch, [&](size_t c) { pack(c * CH, std::min(n, (c + 1) * CH)); });
  uint8_t* d = D.d_buf.as<uint8_t>();
  ICHK(hipMemcpyAsync(d, h, h_need, hipMemcpyHostToDevice, D.stream));
  ICHK(hipEventRecord(D.ev[0], D.stream));
  for (size_t base = 0; base < n; base += tile)
    launch_nym_verify(bn, (int)n, reinterpret_cast<const uint32_t*>(d), d + o_nym,
                      reinterpret_cast<const uint32_t*>(d + o_msg), reinterpret_cast<const uint64_t*>(d + o_off),
                      reinterpret_cast<const uint32_t*>(d + o_len), K->d_tables.as<uint32_t>(),
                      K->d_hash.as<uint32_t>(), reinterpret_cast<uint32_t*>(d + o_vt),
                      reinterpret_cast<int32_t*>(d + o_st), (int)base, (int)tile, D.stream);
  ICHK(hipGetLastError());
  ICHK(hipEventRecord(D.ev[1], D.stream));
  ICHK(hipMemcpyAsync(h + o_st, d + o_st, st_b, hipMemcpyDeviceToHost, D.stream));
  ICHK(hipStreamSynchronize(D.stream));
  memcpy(status, h + o_st, st_b);
  ICHK(hipEventElapsedTime(&D.ms, D.ev[0], D.ev[1]));
  return FTS_API_OK;
}

int fts_nym_last_timings(fts_idemix_ipk* K, float* ms) {
  if (!K || !ms) return FTS_API_EINVAL;
  std::lock_guard<std::mutex> l(K->ring.mu);
  *ms = K->last_ms;
  return FTS_API_OK;
}

int fts_nym_sign_batch(fts_idemix_ipk* K, size_t n, const fts_nym_sign_item* items, uint64_t seed, uint8_t* sig,
                       int32_t* status) {
  if (!K || n > (size_t)(1u << 24) || (n && (!items || !sig || !status))) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  const bool bn = K->curve == FTS_CURVE_BN254;
  const uint32_t* const rmod = bn ? u256::kRbn : u256::kRfbn;
  size_t mtot_w = 0;  // the hashed stream, laid out as for fts_nym_verify_batch
  for (size_t i = 0; i < n; i++) {
    if (items[i].msg_len > 0xffffff00u || (items[i].msg_len && !items[i].msg)) return FTS_API_EINVAL;
    mtot_w += nym_stream_words(bn, items[i].msg_len);
  }
  const host::RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  auto guard = K->ring.acquire([K](NymSlot& S) { K->last_sign_ms = S.sign_ms; });
  NymSlot& D = guard.slot();
  ICHK(hipSetDevice(K->device));
  // layout: secrets | nym | moff | mlen | status | c, s_sk, s_r (device -> host) | messages
  const size_t sec_b = n * NSREC * 4, nym_b = n * 64, off_b = n * 8, len_b = n * 4, st_b = n * 4, out_b = n * NSOUT * 4;
  const size_t o_nym = sec_b, o_off = o_nym + nym_b, o_len = o_off + off_b, o_st = o_len + len_b, o_out = o_st + st_b,
               o_msg = (o_out + out_b + 255) & ~size_t(255), need = o_msg + mtot_w * 4;
  if (D.h_buf.cap < need && !D.h_buf.reserve(need + need / 2)) return FTS_API_ENOMEM;
  if (D.d_buf.cap < need && !D.d_buf.reserve(need + need / 2)) return FTS_API_ENOMEM;
  uint8_t* h = D.h_buf.as<uint8_t>();
  uint8_t* d = D.d_buf.as<uint8_t>();
  SecretWipe wipe(D.stream);
  wipe.host = h, wipe.bytes = sec_b;
  uint64_t* hoff = reinterpret_cast<uint64_t*>(h + o_off);
  {
    uint64_t o = 0;
    for (size_t i = 0; i < n; i++) hoff[i] = o, o += nym_stream_words(bn, items[i].msg_len);
  }
  // uniform below r by rejection: Rng::fr() on BN254, the same construction over the
  // 256-bit r of FP256BN (four words, no mask)
  auto draw = [&](host::Rng& rng, uint32_t out[8]) {
    if (bn) return fr_canon(rng.fr(), out);
    do {
      for (int k = 0; k < 4; k++) {
        const uint64_t v = rng.next();
        out[2 * k] = (uint32_t)v, out[2 * k + 1] = (uint32_t)(v >> 32);
      }
    } while (u256::ge(out, u256::kRfbn));
  };
  const size_t CH = 2048, nch = (n + CH - 1) / CH;
  host_parallel_for(nch, [&](size_t c) {
    for (size_t i = c * CH; i < std::min(n, (c + 1) * CH); i++) {
      const fts_nym_sign_item& it = items[i];
      uint32_t* R = reinterpret_cast<uint32_t*>(h) + i * NSREC;
      memset(R, 0, NSREC * 4);
      int32_t st = FTS_OK;
      // secrets below r, decided here; then the key checks of verification (the point
      // checks run on the device)
      if (!it.sk32 || !it.rnym32 || !u256::be_limbs(it.sk32, 32, R) || !u256::be_limbs(it.rnym32, 32, R + 8) ||
          u256::ge(R, rmod) || u256::ge(R + 8, rmod))
        st = FTS_E_SIGN_BADKEY;
      const bool key_ok = pack_nym_item(bn, it.nym, it.nym_len, K->hash, it.msg, it.msg_len, h + o_nym + i * 64,
                                        h + o_msg + hoff[i] * 4, reinterpret_cast<uint32_t*>(h + o_len) + i);
      if (st == FTS_OK && !key_ok) st = FTS_E_NYM_BADKEY;
      if (st == FTS_OK) {
        host::Rng rng = src.at(i);
        uint32_t nonce[8];
        draw(rng, nonce);
        draw(rng, R + 16);
        draw(rng, R + 24);
        for (int k = 0; k < 8; k++) R[32 + k] = nonce[7 - k];  // big-endian words, as hashed
      } else {
        memset(R, 0, NSREC * 4);
      }
      reinterpret_cast<int32_t*>(h + o_st)[i] = st;
    }
  });
  wipe.dev = d;
  ICHK(hipMemcpyAsync(d, h, o_out, hipMemcpyHostToDevice, D.stream));
  ICHK(hipMemcpyAsync(d + o_msg, h + o_msg, mtot_w * 4, hipMemcpyHostToDevice, D.stream));
  ICHK(hipEventRecord(D.ev[0], D.stream));
  launch_nym_sign(bn, (int)n, reinterpret_cast<const uint32_t*>(d), d + o_nym,
                  reinterpret_cast<const uint32_t*>(d + o_msg), reinterpret_cast<const uint64_t*>(d + o_off),
                  reinterpret_cast<const uint32_t*>(d + o_len), K->d_tables.as<uint32_t>(), K->d_hash.as<uint32_t>(),
                  reinterpret_cast<int32_t*>(d + o_st), reinterpret_cast<uint32_t*>(d + o_out), D.stream);
  ICHK(hipGetLastError());
  ICHK(hipEventRecord(D.ev[1], D.stream));
  // the nonce words are read back from the staging copy before it is wiped
  ICHK(hipMemcpyAsync(h + o_st, d + o_st, st_b + out_b, hipMemcpyDeviceToHost, D.stream));
  ICHK(hipMemsetAsync(d, 0, sec_b, D.stream));
  wipe.dev = nullptr;  // queued
  ICHK(hipStreamSynchronize(D.stream));
  host_parallel_for(nch, [&](size_t c) {
    for (size_t i = c * CH; i < std::min(n, (c + 1) * CH); i++) {
      const int32_t st = reinterpret_cast<const int32_t*>(h + o_st)[i];
      status[i] = st;
      uint8_t* o = sig + i * FTS_NYM_SIG_LEN;
      if (st != FTS_OK) {
        memset(o, 0, FTS_NYM_SIG_LEN);
        continue;
      }
      const uint32_t* O = reinterpret_cast<const uint32_t*>(h + o_out) + i * NSOUT;
      const uint32_t* R = reinterpret_cast<const uint32_t*>(h) + i * NSREC;
      uint8_t f[4][32];
      for (int q = 0; q < 3; q++)
        for (int k = 0; k < 8; k++)
          for (int b = 0; b < 4; b++) f[q][4 * k + b] = (uint8_t)(O[8 * q + 7 - k] >> (24 - 8 * b));
      for (int k = 0; k < 8; k++)
        for (int b = 0; b < 4; b++) f[3][4 * k + b] = (uint8_t)(R[32 + k] >> (24 - 8 * b));
      host::nym_sig_proto(f[0], f[1], f[2], f[3], o);
    }
  });
  memset(h, 0, sec_b);
  wipe.host = nullptr;
  ICHK(hipEventElapsedTime(&D.sign_ms, D.ev[0], D.ev[1]));
  return FTS_API_OK;
}

int fts_nym_sign_last_timings(fts_idemix_ipk* K, float* ms) {
  if (!K || !ms) return FTS_API_EINVAL;
  std::lock_guard<std::mutex> l(K->ring.mu);
  *ms = K->last_sign_ms;
  return FTS_API_OK;
}

// ---------------------------------------------------------------------------
// Identity association proofs
// ---------------------------------------------------------------------------
int fts_idemix_idv_create(int device, const uint8_t* ipk, size_t ipk_len, int curve_id, fts_idemix_idv** out) {
  if (!out || !ipk || !ipk_len || (curve_id != FTS_CURVE_BN254 && curve_id != FTS_CURVE_FP256BN_AMCL))
    return FTS_API_EINVAL;
  *out = nullptr;
  const bool bn = curve_id == FTS_CURVE_BN254;
  IpkFields f;
  if (!parse_ipk(ipk, ipk_len, f) || f.n_attrs != 4) return FTS_API_EPP;  // OU, Role, EnrollmentID, RevocationHandle
  uint8_t raw[NB][64], wraw[128];
  if (!ecp_xy(f.h_sk, raw[B_HSK], true) || !ecp_xy(f.h_rand, raw[B_HRAND], true) || !ecp2_raw(f.w, wraw))
    return FTS_API_EPP;
  for (int a = 0; a < 4; a++)
    if (!ecp_xy(f.h_attrs[a], raw[B_HA + a], true)) return FTS_API_EPP;
  memset(raw[B_G1], 0, 64);  // g1 = (1, 2) on both curves
  raw[B_G1][31] = 1, raw[B_G1][63] = 2;
  uint32_t bases[NB * 16];
  if (!base_words(bn, raw, NB, bases)) return FTS_API_EPP;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FTS_API_EDEVICE;
  std::unique_ptr<fts_idemix_idv> k(new fts_idemix_idv());
  k->device = device;
  k->curve = curve_id;
  if (const char* e = getenv("FTS_IDV_BATCH")) k->batch = atoi(e) != 0;
  if (hipSetDevice(device) != hipSuccess) return FTS_API_EDEVICE;
  uint8_t h32[32];
  uint32_t hw[24];  // ipk.Hash, then HSk as X || Y
  ipk_hash32(f, h32);
  be_words(h32, hw);
  be_words(raw[B_HSK], hw + 8), be_words(raw[B_HSK] + 32, hw + 16);
  k->has_bar = ecp_xy(f.bar_g1, k->bar, false) && ecp_xy(f.bar_g2, k->bar + 64, false);
  const size_t wpb = bn ? fb_words_per_base() : fbn_words_per_base();
  const size_t nl = line_words(bn);
  Stream s0;
  DevBuf bases_buf, scr_buf, w_buf, ok_buf;
  const size_t scr_b = bn ? table_build_scratch_bytes(NB) : (size_t)NB * 16 * 4;
  bool ok = s0.create() == hipSuccess && k->d_tables.reserve((size_t)NB * wpb * 4) &&
            k->d_lines.reserve(2 * nl * 4) && k->d_hash.reserve(sizeof hw) && bases_buf.reserve(sizeof bases) &&
            scr_buf.reserve(scr_b) && w_buf.reserve(128) && ok_buf.reserve(64);
  uint32_t* const d_tables = k->d_tables.as<uint32_t>();
  uint32_t* const d_lines = k->d_lines.as<uint32_t>();
  uint32_t *const d_bases = bases_buf.as<uint32_t>(), *const d_scr = scr_buf.as<uint32_t>();
  uint8_t* const d_w = w_buf.as<uint8_t>();
  int32_t* const d_ok = ok_buf.as<int32_t>();
  ok = ok && hipMemcpyAsync(d_bases, bases, sizeof bases, hipMemcpyHostToDevice, s0) == hipSuccess &&
       hipMemcpyAsync(d_w, wraw, 128, hipMemcpyHostToDevice, s0) == hipSuccess &&
       hipMemcpyAsync(k->d_hash.p, hw, sizeof hw, hipMemcpyHostToDevice, s0) == hipSuccess &&
       hipMemsetAsync(d_ok, 0, 64, s0) == hipSuccess;
  int32_t hok[NB + 1] = {0};
  if (ok) {
    if (bn) {
      launch_build_tables(d_bases, NB, d_tables, d_scr, s0);
      launch_lines<BnCurve>(d_w, d_lines, d_ok + NB, s0);
    } else {
      fbn_build_tables(d_bases, NB, d_scr, d_ok, d_tables, s0);
      launch_lines<FbnCurve>(d_w, d_lines, d_ok + NB, s0);
    }
    ok = hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(hok, d_ok, sizeof hok, hipMemcpyDeviceToHost, s0) == hipSuccess &&
         hipStreamSynchronize(s0) == hipSuccess;
  }
  if (s0) (void)hipStreamSynchronize(s0);  // an error path may leave copies queued on s0
  if (!ok) return FTS_API_EDEVICE;
  bool valid = hok[NB] == 1;  // W on the twist
  if (!bn)
    for (int b = 0; b < NB; b++) valid = valid && hok[b] == 1;
  if (!valid) return FTS_API_EPP;
  for (auto& S : k->ring.slot) {
    ok = ok && S.stream.create() == hipSuccess;
    for (auto& e : S.ev) ok = ok && e.create() == hipSuccess;
  }
  for (auto& S : k->aud.slot) {
    ok = ok && S.stream.create() == hipSuccess;
    for (auto& e : S.ev) ok = ok && e.create() == hipSuccess;
  }
  ok = ok && (k->creq = credreq_state_new()) != nullptr;
  if (!ok) return FTS_API_EDEVICE;
  *out = k.release();
  return FTS_API_OK;
}

void fts_idemix_idv_destroy(fts_idemix_idv* k) { delete k; }

int fts_idemix_identity_verify_batch(fts_idemix_idv* K, size_t n, const uint8_t* const* ids, const size_t* id_len,
                                     int32_t* status) {
  if (!K || n > (size_t)(1u << 22) || (n && (!ids || !id_len || !status))) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  const bool bn = K->curve == FTS_CURVE_BN254;
  auto guard = K->ring.acquire([K](IdvSlot& S) {
    K->last_ms[0] = S.ms[0], K->last_ms[1] = S.ms[1];
    K->last_stats[0] = S.stats[0], K->last_stats[1] = S.stats[1];
  });
  IdvSlot& D = guard.slot();
  ICHK(hipSetDevice(K->device));
  // staged (host + device): rec | pts | epk | status | eidx | distinct epoch keys (BN254);
  // device only: zk | pin | scratch | msg | g2ok
  const size_t rec_b = n * REC_STRIDE * 4, pts_b = n * NPT * 64, epk_b = n * 128, st_b = n * 4;
  const size_t o_pts = rec_b, o_epk = o_pts + pts_b, o_st = o_epk + epk_b, o_eidx = o_st + st_b,
               o_uk = o_eidx + n * 4;
  // host only: the distinct keys' verdicts (cached or read back) and the indices to check
  const size_t o_gk = (o_uk + epk_b + 255) & ~size_t(255), o_miss = o_gk + n * 4;
  const size_t o_cnt = o_miss + n * 4;  // the batch check's list length, read back
  const size_t h_need = (o_cnt + 4 + 255) & ~size_t(255);
  const size_t o_zk = h_need, o_pin = (o_zk + n * 4 + 255) & ~size_t(255), o_scr = o_pin + n * 32 * 4;
  const size_t scr_w = std::max(idv_scratch_words(n), bp_scratch_words(n));
  const size_t o_msg = (o_scr + scr_w * 4 + 255) & ~size_t(255);
  const size_t o_g2ok = (o_msg + (size_t)MSG_MAX * n + 255) & ~size_t(255);
  const size_t d_need = o_g2ok + 2 * n * 4;  // U verdicts, then the M key indices to check
  if (D.h_buf.cap < h_need && !D.h_buf.reserve(h_need + h_need / 2)) return FTS_API_ENOMEM;
  if (D.d_buf.cap < d_need && !D.d_buf.reserve(d_need + d_need / 2)) return FTS_API_ENOMEM;
  uint8_t* h = D.h_buf.as<uint8_t>();
  const size_t CH = 1024, nch = (n + CH - 1) / CH;
  host_parallel_for(nch, [&](size_t c) {
    for (size_t i = c * CH; i < std::min(n, (c + 1) * CH); i++)
      reinterpret_cast<int32_t*>(h + o_st)[i] =
          parse_identity(ids[i], id_len[i], bn, reinterpret_cast<uint32_t*>(h) + i * REC_STRIDE,
                         h + o_pts + i * NPT * 64, h + o_epk + i * 128);
  });
  // BN254 epoch keys: one subgroup check per DISTINCT key (honest batches carry one)
  size_t U = 0;
  int32_t* eidx = reinterpret_cast<int32_t*>(h + o_eidx);
  if (bn) {
    const uint8_t* E = h + o_epk;
    uint8_t* UK = h + o_uk;
    std::atomic<bool> same{true};
    host_parallel_for(nch, [&](size_t c) {
      for (size_t i = c * CH; i < std::min(n, (c + 1) * CH) && same.load(std::memory_order_relaxed); i++)
        if (memcmp(E + i * 128, E, 128) != 0) same = false;
    });
    if (same) {
      memcpy(UK, E, 128);
      std::fill(eidx, eidx + n, 0);
      U = 1;
    } else {  // sort by (hash, bytes), then one entry per run of equal keys
      std::vector<std::pair<uint64_t, uint32_t>> hk(n);
      for (size_t i = 0; i < n; i++) {
        uint64_t x = 0x9e3779b97f4a7c15ull;
        for (int q = 0; q < 16; q++) {
          uint64_t w;
          memcpy(&w, E + i * 128 + 8 * q, 8);
          x = (x ^ w) * 0xff51afd7ed558ccdull;
          x ^= x >> 29;
        }
        hk[i] = {x, (uint32_t)i};
      }
      std::sort(hk.begin(), hk.end(), [&](const std::pair<uint64_t, uint32_t>& a, const std::pair<uint64_t, uint32_t>& b) {
        if (a.first != b.first) return a.first < b.first;
        return memcmp(E + (size_t)a.second * 128, E + (size_t)b.second * 128, 128) < 0;
      });
      for (size_t j = 0; j < n; j++) {
        const uint32_t i = hk[j].second;
        if (j == 0 || hk[j].first != hk[j - 1].first ||
            memcmp(E + (size_t)i * 128, E + (size_t)hk[j - 1].second * 128, 128) != 0)
          memcpy(UK + 128 * U++, E + (size_t)i * 128, 128);
        eidx[i] = (int32_t)(U - 1);
      }
    }
  }
  // cached key verdicts; the misses are checked on the device and cached after the call
  int32_t* gk = reinterpret_cast<int32_t*>(h + o_gk);
  int32_t* miss = reinterpret_cast<int32_t*>(h + o_miss);
  size_t M = 0;
  if (bn) {
    std::lock_guard<std::mutex> l(K->ring.mu);
    for (size_t j = 0; j < U; j++) {
      const auto it = K->g2_seen.find(std::string(reinterpret_cast<const char*>(h + o_uk + 128 * j), 128));
      if (it != K->g2_seen.end()) {
        gk[j] = it->second;
      } else {
        gk[j] = 0;
        miss[M++] = (int32_t)j;
      }
    }
  }
  uint8_t* d = D.d_buf.as<uint8_t>();
  ICHK(hipMemcpyAsync(d, h, o_uk + U * 128, hipMemcpyHostToDevice, D.stream));
  ICHK(hipEventRecord(D.ev[0], D.stream));
  // batch pairing check: group sums, one pairing product per group, the identities
  // of failing groups listed for k_idv_pairing
  uint32_t* scr = reinterpret_cast<uint32_t*>(d + o_scr);
  const size_t ng = (n + BP_G - 1) / BP_G;
  Chain c;
  c.s = D.stream, c.n = (int)n, c.rec = reinterpret_cast<const uint32_t*>(d), c.pts = d + o_pts, c.epk = d + o_epk;
  c.scr = scr, c.pin = reinterpret_cast<uint32_t*>(d + o_pin);
  c.zk = reinterpret_cast<int32_t*>(d + o_zk), c.st = reinterpret_cast<int32_t*>(d + o_st);
  int32_t* g2ok = reinterpret_cast<int32_t*>(d + o_g2ok);
  c.eidx = bn ? reinterpret_cast<const int32_t*>(d + o_eidx) : nullptr, c.g2ok = bn ? g2ok : nullptr;
  c.tables = K->d_tables.as<uint32_t>(), c.hash = K->d_hash.as<uint32_t>(), c.lines = K->d_lines.as<uint32_t>(), c.msg = d + o_msg;
  c.gok = reinterpret_cast<int32_t*>(scr + bp_gok_off(n, ng));
  c.cnt = reinterpret_cast<int32_t*>(scr + bp_cnt_off(n, ng));
  c.list = reinterpret_cast<int32_t*>(scr + bp_list_off(n, ng));
  if (K->batch && getrandom(c.key.k, sizeof c.key.k, 0) != (ssize_t)sizeof c.key.k) return FTS_API_EDEVICE;
  if (bn) {
    ICHK(hipMemcpyAsync(g2ok, gk, U * 4, hipMemcpyHostToDevice, D.stream));
    if (M) {
      ICHK(hipMemcpyAsync(g2ok + U, miss, M * 4, hipMemcpyHostToDevice, D.stream));
      launch_g2_check((int)M, g2ok + U, d + o_uk, g2ok, D.stream);
    }
  }
  bn ? launch_tvals<BnCurve>(c) : launch_tvals<FbnCurve>(c);
  ICHK(hipEventRecord(D.ev[1], D.stream));
  unsigned nlist = 0;  // identities of failing groups (read back after k_idv_bp_sel)
  if (K->batch) {
    bn ? launch_batch<BnCurve>(c) : launch_batch<FbnCurve>(c);
    ICHK(hipMemcpyAsync(h + o_cnt, c.cnt, 4, hipMemcpyDeviceToHost, D.stream));
    ICHK(hipStreamSynchronize(D.stream));
    nlist = *reinterpret_cast<const uint32_t*>(h + o_cnt);
    // exact grid: idle pairing waves (256 VGPRs and scratch each) would still queue
    // behind the other slots' kernels
    if (nlist) bn ? launch_pairing<BnCurve>(c, nlist, true) : launch_pairing<FbnCurve>(c, nlist, true);
  } else {
    bn ? launch_pairing<BnCurve>(c, (unsigned)n, false) : launch_pairing<FbnCurve>(c, (unsigned)n, false);
  }
  ICHK(hipGetLastError());
  ICHK(hipEventRecord(D.ev[2], D.stream));
  ICHK(hipMemcpyAsync(h + o_st, d + o_st, st_b, hipMemcpyDeviceToHost, D.stream));
  if (M) ICHK(hipMemcpyAsync(gk, g2ok, U * 4, hipMemcpyDeviceToHost, D.stream));
  ICHK(hipStreamSynchronize(D.stream));
  memcpy(status, h + o_st, st_b);
  D.stats[0] = K->batch ? (uint32_t)ng : 0u;
  D.stats[1] = K->batch ? nlist : (uint32_t)n;
  if (M) {
    std::lock_guard<std::mutex> l(K->ring.mu);
    if (K->g2_seen.size() + M > 4096) K->g2_seen.clear();  // bounded: a new epoch's keys refill it
    for (size_t q = 0; q < M; q++) {
      const size_t j = (size_t)miss[q];
      K->g2_seen.emplace(std::string(reinterpret_cast<const char*>(h + o_uk + 128 * j), 128), gk[j]);
    }
  }
  ICHK(hipEventElapsedTime(&D.ms[0], D.ev[0], D.ev[1]));
  ICHK(hipEventElapsedTime(&D.ms[1], D.ev[1], D.ev[2]));
  return FTS_API_OK;
}

int fts_idemix_identity_last_timings(fts_idemix_idv* K, float* ms) {
  if (!K || !ms) return FTS_API_EINVAL;
  std::lock_guard<std::mutex> l(K->ring.mu);
  ms[0] = K->last_ms[0], ms[1] = K->last_ms[1];
  return FTS_API_OK;
}

int fts_idemix_identity_last_stats(fts_idemix_idv* K, uint32_t* out) {
  if (!K || !out) return FTS_API_EINVAL;
  std::lock_guard<std::mutex> l(K->ring.mu);
  out[0] = K->last_stats[0], out[1] = K->last_stats[1];
  return FTS_API_OK;
}

// ---------------------------------------------------------------------------
// Credentials (Credential.Ver, pairing equation included)
// ---------------------------------------------------------------------------
int fts_idemix_cred_verify_batch(fts_idemix_idv* K, size_t n, const fts_idemix_cred_item* items, int32_t* status) {
  if (!K || n > (size_t)(1u << 22) || (n && (!items || !status))) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  const bool bn = K->curve == FTS_CURVE_BN254;
  const uint32_t* const rmod = bn ? u256::kRbn : u256::kRfbn;
  // a slot of the identity ring: identity and credential calls share the bound on pairing
  // stages in flight (IDV_NSLOT)
  auto guard = K->ring.acquire([K](IdvSlot& S) {
    K->last_cred_ms[0] = S.cred_ms[0], K->last_cred_ms[1] = S.cred_ms[1];
    K->last_cred_stats[0] = S.cred_stats[0], K->last_cred_stats[1] = S.cred_stats[1];
  });
  IdvSlot& D = guard.slot();
  ICHK(hipSetDevice(K->device));
  const size_t T = std::min(n, CRV_TILE);
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  // staged (host + device): rec | pts | status; host only: the batch check's list length,
  // read back; device only: zk | pin | scratch
  const size_t rec_b = T * CRV_REC_WORDS * 4;
  const size_t o_pts = al(rec_b), o_st = al(o_pts + T * CRV_PTS_BYTES), o_cnt = al(o_st + T * 4), h_need = o_cnt + 256;
  const size_t o_zk = h_need, o_pin = al(o_zk + T * 4), o_scr = al(o_pin + T * 32 * 4);
  const size_t scr_w = std::max(cred_scratch_words(T), bp_scratch_words(T));
  const size_t d_need = o_scr + scr_w * 4;
  if (D.h_buf.cap < h_need && !D.h_buf.reserve(h_need)) return FTS_API_ENOMEM;
  if (D.d_buf.cap < d_need && !D.d_buf.reserve(d_need)) return FTS_API_ENOMEM;
  uint8_t* h = D.h_buf.as<uint8_t>();
  uint8_t* d = D.d_buf.as<uint8_t>();
  // sk (with E, S and the attributes) staged on the host and the device, then HSk sk, the
  // lane tables and the pairing inputs: wiped on every way out
  SecretWipe wipe_rec(D.stream), wipe_scr(D.stream);
  wipe_rec.host = h, wipe_rec.dev = d, wipe_rec.bytes = rec_b;
  wipe_scr.dev = d + o_pin, wipe_scr.bytes = d_need - o_pin;
  uint32_t* scr = reinterpret_cast<uint32_t*>(d + o_scr);
  CredChain cc;
  cc.s = D.stream, cc.rec = reinterpret_cast<const uint32_t*>(d), cc.pts = d + o_pts, cc.scr = scr;
  cc.pin = reinterpret_cast<uint32_t*>(d + o_pin), cc.zk = reinterpret_cast<int32_t*>(d + o_zk);
  cc.st = reinterpret_cast<int32_t*>(d + o_st), cc.tables = K->d_tables.as<uint32_t>();
  // the pairing stage of the identity verifier, on (A, E A - B) instead of (A', -ABar)
  Chain c{};
  c.s = D.stream, c.scr = scr, c.pin = cc.pin, c.zk = cc.zk, c.st = cc.st, c.lines = K->d_lines.as<uint32_t>();
  float ms[2] = {0.f, 0.f};
  uint32_t stats[2] = {0u, 0u};
  const size_t CH = 512;
  for (size_t base = 0; base < n; base += T) {
    const size_t m = std::min(T, n - base), nch = (m + CH - 1) / CH, ng = (m + BP_G - 1) / BP_G;
    host_parallel_for(nch, [&](size_t ch) {
      struct Parsed {
        idgen::CredFields f;
        ~Parsed() {
          volatile uint8_t* p = reinterpret_cast<volatile uint8_t*>(this);
          for (size_t q = 0; q < sizeof(Parsed); q++) p[q] = 0;
        }
      } pc;
      for (size_t j = ch * CH; j < std::min(m, (ch + 1) * CH); j++) {
        const fts_idemix_cred_item& it = items[base + j];
        uint32_t* R = reinterpret_cast<uint32_t*>(h) + j * CRV_REC_WORDS;  // E S sk attrs[0..3]
        uint8_t* P = h + o_pts + j * CRV_PTS_BYTES;
        const bool good = it.cred && it.cred_len && it.sk32 && idgen::parse_credential(it.cred, it.cred_len, bn, pc.f) &&
                          u256::be_limbs(it.sk32, 32, R + 16) && !u256::ge(R + 16, rmod);
        if (good) {
          memcpy(R, pc.f.e, 32), memcpy(R + 8, pc.f.s, 32), memcpy(R + 24, pc.f.attrs, 128);
          memcpy(P, pc.f.a, 64), memcpy(P + 64, pc.f.b, 64);
        } else {
          memset(R, 0, CRV_REC_WORDS * 4), memset(P, 0, CRV_PTS_BYTES);
        }
        reinterpret_cast<int32_t*>(h + o_st)[j] = good ? FTS_OK : FTS_E_CRED_MALFORMED;
      }
    });
    cc.n = c.n = (int)m;
    c.gok = reinterpret_cast<int32_t*>(scr + bp_gok_off(m, ng));
    c.cnt = reinterpret_cast<int32_t*>(scr + bp_cnt_off(m, ng));
    c.list = reinterpret_cast<int32_t*>(scr + bp_list_off(m, ng));
    if (K->batch && getrandom(c.key.k, sizeof c.key.k, 0) != (ssize_t)sizeof c.key.k) return FTS_API_EDEVICE;
    ICHK(hipMemcpyAsync(d, h, o_st + m * 4, hipMemcpyHostToDevice, D.stream));
    ICHK(hipEventRecord(D.ev[0], D.stream));
    bn ? launch_cred_prep<BnCurve>(cc) : launch_cred_prep<FbnCurve>(cc);
    ICHK(hipEventRecord(D.ev[1], D.stream));
    unsigned nlist = 0;
    if (K->batch) {
      bn ? launch_batch<BnCurve>(c) : launch_batch<FbnCurve>(c);
      ICHK(hipMemcpyAsync(h + o_cnt, c.cnt, 4, hipMemcpyDeviceToHost, D.stream));
      ICHK(hipStreamSynchronize(D.stream));
      nlist = *reinterpret_cast<const uint32_t*>(h + o_cnt);
      if (nlist > m) return FTS_API_EDEVICE;
      if (nlist) bn ? launch_pairing<BnCurve>(c, nlist, true) : launch_pairing<FbnCurve>(c, nlist, true);
    } else {
      bn ? launch_pairing<BnCurve>(c, (unsigned)m, false) : launch_pairing<FbnCurve>(c, (unsigned)m, false);
    }
    ICHK(hipGetLastError());
    ICHK(hipEventRecord(D.ev[2], D.stream));
    ICHK(hipMemcpyAsync(h + o_st, d + o_st, m * 4, hipMemcpyDeviceToHost, D.stream));
    ICHK(hipStreamSynchronize(D.stream));
    // the pairing kernels write the identity verifier's verdict
    const int32_t* hst = reinterpret_cast<const int32_t*>(h + o_st);
    for (size_t j = 0; j < m; j++) status[base + j] = hst[j] == FTS_E_ID_PAIRING ? FTS_E_CRED_PAIRING : hst[j];
    float a = 0.f, b = 0.f;
    ICHK(hipEventElapsedTime(&a, D.ev[0], D.ev[1]));
    ICHK(hipEventElapsedTime(&b, D.ev[1], D.ev[2]));
    ms[0] += a, ms[1] += b;
    stats[0] += K->batch ? (uint32_t)ng : 0u;
    stats[1] += K->batch ? nlist : (uint32_t)m;
  }
  D.cred_ms[0] = ms[0], D.cred_ms[1] = ms[1];
  D.cred_stats[0] = stats[0], D.cred_stats[1] = stats[1];
  return FTS_API_OK;
}

int fts_idemix_cred_verify_last_timings(fts_idemix_idv* K, float* ms2) {
  if (!K || !ms2) return FTS_API_EINVAL;
  std::lock_guard<std::mutex> l(K->ring.mu);
  ms2[0] = K->last_cred_ms[0], ms2[1] = K->last_cred_ms[1];
  return FTS_API_OK;
}

int fts_idemix_cred_verify_last_stats(fts_idemix_idv* K, uint32_t* out2) {
  if (!K || !out2) return FTS_API_EINVAL;
  std::lock_guard<std::mutex> l(K->ring.mu);
  out2[0] = K->last_cred_stats[0], out2[1] = K->last_cred_stats[1];
  return FTS_API_OK;
}

// ---------------------------------------------------------------------------
// Audit info against owner identities (AuditInfo.Match)
// ---------------------------------------------------------------------------
int fts_idemix_audit_match_batch(fts_idemix_idv* K, size_t n, const fts_idemix_audit_item* items, int32_t* status) {
  if (!K || n > (size_t)(1u << 22) || (n && (!items || !status))) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  const bool bn = K->curve == FTS_CURVE_BN254;
  // a lane's string: its bytes padded to whole words + 1 (as the nym messages)
  auto words = [](size_t len) { return (len + 3) / 4 + 1; };
  size_t atot_w = 0;
  for (size_t i = 0; i < n; i++) {
    const fts_idemix_audit_item& it = items[i];
    if (it.eid_len > 0xffffff00u || it.rh_len > 0xffffff00u || (it.eid_len && !it.eid) || (it.rh_len && !it.rh))
      return FTS_API_EINVAL;
    atot_w += words(it.eid_len) + words(it.rh_len);
  }
  auto guard = K->aud.acquire([K](AuditSlot& S) { K->aud_ms = S.ms; });
  AuditSlot& D = guard.slot();
  ICHK(hipSetDevice(K->device));
  // half-major lanes g = half * n + i: pts | rnd | aoff | alen (2n each) | pre | rh_pre (n each) |
  // strings (the EID strings, then the RH strings) | half_st (2n, written by the device)
  const size_t o_rnd = 2 * n * 64, o_off = o_rnd + 2 * n * 32, o_len = o_off + 2 * n * 8, o_pre = o_len + 2 * n * 4,
               o_rhp = o_pre + n * 4, o_str = (o_rhp + n * 4 + 255) & ~size_t(255),
               o_hst = (o_str + atot_w * 4 + 255) & ~size_t(255), need = o_hst + 2 * n * 4;
  if (D.h_buf.cap < need && !D.h_buf.reserve(need + need / 2)) return FTS_API_ENOMEM;
  if (D.d_buf.cap < need && !D.d_buf.reserve(need + need / 2)) return FTS_API_ENOMEM;
  uint8_t* h = D.h_buf.as<uint8_t>();
  uint64_t* hoff = reinterpret_cast<uint64_t*>(h + o_off);
  {
    uint64_t o = 0;
    for (size_t i = 0; i < n; i++) hoff[i] = o, o += words(items[i].eid_len);
    for (size_t i = 0; i < n; i++) hoff[n + i] = o, o += words(items[i].rh_len);
  }
  auto pack = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      const fts_idemix_audit_item& it = items[i];
      int32_t rh_pre = FTS_OK;
      int32_t pre = parse_audit_identity(it.id, it.id_len, bn, h + i * 64, h + (n + i) * 64, rh_pre);
      if (!it.r_eid32 || !it.r_rh32) pre = FTS_E_AUDIT_MALFORMED;  // the reference dereferences a nil Rand
      reinterpret_cast<int32_t*>(h + o_pre)[i] = pre;
      reinterpret_cast<int32_t*>(h + o_rhp)[i] = rh_pre;
      const uint8_t* const rnd[2] = {it.r_eid32, it.r_rh32};
      const uint8_t* const str[2] = {it.eid, it.rh};
      const size_t slen[2] = {it.eid_len, it.rh_len};
      for (int half = 0; half < 2; half++) {
        const size_t g = (size_t)half * n + i;
        uint8_t* r = h + o_rnd + g * 32;
        if (rnd[half]) memcpy(r, rnd[half], 32);
        else memset(r, 0, 32);
        reinterpret_cast<uint32_t*>(h + o_len)[g] = (uint32_t)slen[half];
        uint8_t* sw = h + o_str + hoff[g] * 4;
        if (slen[half]) memcpy(sw, str[half], slen[half]);
        memset(sw + slen[half], 0, words(slen[half]) * 4 - slen[half]);
      }
    }
  };
  const size_t CH = 2048, nch = (n + CH - 1) / CH;
  host_parallel_for(nch, [&](size_t c) { pack(c * CH, std::min(n, (c + 1) * CH)); });
  uint8_t* d = D.d_buf.as<uint8_t>();
  ICHK(hipMemcpyAsync(d, h, o_hst, hipMemcpyHostToDevice, D.stream));
  ICHK(hipEventRecord(D.ev[0], D.stream));
  launch_idv_audit(bn, (int)n, d, reinterpret_cast<const uint32_t*>(d + o_rnd),
                   reinterpret_cast<const uint32_t*>(d + o_str), reinterpret_cast<const uint64_t*>(d + o_off),
                   reinterpret_cast<const uint32_t*>(d + o_len), reinterpret_cast<const int32_t*>(d + o_pre),
                   reinterpret_cast<const int32_t*>(d + o_rhp), K->d_tables.as<uint32_t>(),
                   reinterpret_cast<int32_t*>(d + o_hst), D.stream);
  ICHK(hipGetLastError());
  ICHK(hipEventRecord(D.ev[1], D.stream));
  ICHK(hipMemcpyAsync(h + o_hst, d + o_hst, 2 * n * 4, hipMemcpyDeviceToHost, D.stream));
  ICHK(hipStreamSynchronize(D.stream));
  // the reference's order: what ends the match on the host, every EID check, every RH check
  const int32_t* pre = reinterpret_cast<const int32_t*>(h + o_pre);
  const int32_t* hst = reinterpret_cast<const int32_t*>(h + o_hst);
  for (size_t i = 0; i < n; i++) status[i] = pre[i] ? pre[i] : hst[i] ? hst[i] : hst[n + i];
  ICHK(hipEventElapsedTime(&D.ms, D.ev[0], D.ev[1]));
  return FTS_API_OK;
}

int fts_idemix_audit_last_timings(fts_idemix_idv* K, float* ms) {
  if (!K || !ms) return FTS_API_EINVAL;
  std::lock_guard<std::mutex> l(K->aud.mu);
  *ms = K->aud_ms;
  return FTS_API_OK;
}

int fts_idemix_pairing_debug(fts_idemix_idv* K, int which, const uint8_t* p64, int final_exp, uint32_t* out192) {
  if (!K || !p64 || !out192 || (which != 0 && which != 1)) return FTS_API_EINVAL;
  // P: 64 raw BE bytes -> 16 words as base_words() hands points over: BN254 affine Montgomery
  // (decoded and on-curve checked here), FP256BN canonical limbs < p (converted on the device)
  const bool bn = K->curve == FTS_CURVE_BN254;
  uint32_t pm[16];
  if (bn) {
    host::G1A a;
    if (!host::g1_from_bytes(p64, 64, a) || a.inf) return FTS_API_EINVAL;
    memcpy(pm, a.x.v, 32);
    memcpy(pm + 8, a.y.v, 32);
  } else {
    u256::be_limbs(p64, 32, pm);
    u256::be_limbs(p64 + 32, 32, pm + 8);
    if (u256::ge(pm, u256::kPfbn) || u256::ge(pm + 8, u256::kPfbn)) return FTS_API_EINVAL;
  }
  std::lock_guard<std::mutex> l(K->ring.mu);
  ICHK(hipSetDevice(K->device));
  // private stream and buffers, released on every exit path
  struct Res {
    Stream s;
    DevBuf p, o;
    ~Res() {
      if (s) (void)hipStreamSynchronize(s);
    }
  } r;
  ICHK(r.s.create());
  if (!r.p.reserve(64) || !r.o.reserve(192 * 4)) return FTS_API_EDEVICE;
  ICHK(hipMemcpyAsync(r.p.p, pm, 64, hipMemcpyHostToDevice, r.s));
  if (bn) launch_pairing_debug<BnCurve>(K->d_lines.as<uint32_t>(), which, r.p.as<uint32_t>(), r.o.as<uint32_t>(), final_exp, r.s);
  else launch_pairing_debug<FbnCurve>(K->d_lines.as<uint32_t>(), which, r.p.as<uint32_t>(), r.o.as<uint32_t>(), final_exp, r.s);
  ICHK(hipGetLastError());
  ICHK(hipMemcpyAsync(out192, r.o.p, 192 * 4, hipMemcpyDeviceToHost, r.s));
  ICHK(hipStreamSynchronize(r.s));
  return FTS_API_OK;
}

}  // extern "C"
