// C-ABI (include/fts_gpu.h): idemix enrolment on the device -- credential requests made and
// checked on a verifier's handle (fts_idemix_cred_request_batch, _request_verify_batch) and
// fts_idemix_issuer (one issuer secret; fts_idemix_cred_issue_batch).  Handles, slots, tiles
// and staging on the host pool; the draws, the request parser and the two writers are
// host/credreq_write.hpp; the kernels are reached through device/launch.hpp
// (idemix_credissue_{bn,fbn}.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <memory>
#include <mutex>

#include "../../include/fts_gpu.h"
#include "device/launch.hpp"
#include "host/credreq_write.hpp"
#include "host/hip_owned.hpp"
#include "host/host_pool.hpp"
#include "host/prover.hpp"  // Rng, RngSource

using namespace fts;
using namespace idv;

#define CCHK(x)                                    \
  do {                                             \
    if ((x) != hipSuccess) return FTS_API_EDEVICE; \
  } while (0)

namespace {

constexpr int CI_NSLOT = 3;         // calls in flight per handle
constexpr size_t CI_TILE = 16384;   // items per kernel sequence: bounds a slot's buffers (2.7 KB per item, 45 MB per
                                    // slot) and still puts 1,792 waves on the device in k_ci_var
constexpr size_t CI_MAX = (size_t)1 << 22;
struct CiSlot {
  Stream stream;
  DevBuf d_buf;  // rec (the secret region) | pts | status | out | scratch | transcript
  PinBuf h_buf;  // rec | pts | status | out
  Event ev[3];
  float ms[2] = {0.f, 0.f};
  double host_s[2] = {0., 0.};
};

double now_s() {
  timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}
bool make_slots(SlotRing<CiSlot, CI_NSLOT>& ring) {
  bool ok = true;
  for (auto& S : ring.slot) {
    ok = ok && S.stream.create() == hipSuccess;
    for (auto& e : S.ev) ok = ok && e.create() == hipSuccess;
  }
  return ok;
}
void wipe_bytes(void* p, size_t n) {
  volatile uint8_t* q = reinterpret_cast<volatile uint8_t*>(p);
  for (size_t i = 0; i < n; i++) q[i] = 0;
}
size_t al(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

namespace idv {
struct CredReqState {
  SlotRing<CiSlot, CI_NSLOT> ring;
  float last_ms[2] = {0.f, 0.f};  // under ring.mu: the last request batch, the last request-verification batch
};
CredReqState* credreq_state_new() {
  std::unique_ptr<CredReqState> s(new CredReqState());
  return make_slots(s->ring) ? s.release() : nullptr;
}
void credreq_state_free(CredReqState* s) { delete s; }
}  // namespace idv

struct fts_idemix_issuer {
  IssuerView iv{};
  bool bn = true;
  DevBuf d_isk;        // the secret, canonical limbs
  uint32_t avoid[8];   // r - isk: the E that has no inverse
  SlotRing<CiSlot, CI_NSLOT> ring;
  float last_ms[2] = {0.f, 0.f};     // under ring.mu
  double last_host_s[2] = {0., 0.};  // under ring.mu
  // the secret this handle holds is zeroed before it is freed
  void wipe() {
    wipe_bytes(avoid, sizeof avoid);
    if (iv.v.device < 0 || hipSetDevice(iv.v.device) != hipSuccess) return;
    if (d_isk.p) (void)hipMemset(d_isk.p, 0, d_isk.cap);
    (void)hipDeviceSynchronize();
  }
  ~fts_idemix_issuer() { wipe(); }
};

namespace {

// One call of the request check (K = nullptr) or of issuance on the slot D: tiles of CI_TILE,
// request i = get(i).  status (and for an issue creds, cred_len) are written for every item.
template <class Get>
int check_or_issue(const IdvView& v, CiSlot& D, size_t n, Get get, const fts_idemix_issuer* K,
                   const fts_idemix_issue_item* items, const host::RngSource* src, uint8_t* creds, size_t stride,
                   uint32_t* cred_len, int32_t* status) {
  const bool bn = v.curve == FTS_CURVE_BN254, issue = K != nullptr;
  const uint32_t* const rmod = bn ? u256::kRbn : u256::kRfbn;
  CCHK(hipSetDevice(v.device));
  const size_t T = std::min(n, CI_TILE);
  const size_t rec_b = T * CI_REC_WORDS * 4, out_b = T * CI_OUT_WORDS * 4;
  const size_t o_pts = al(rec_b), o_st = al(o_pts + T * 64), o_out = al(o_st + T * 4), h_need = al(o_out + out_b);
  const size_t o_scr = h_need, o_msg = al(o_scr + credissue_scratch_words(T) * 4),
               d_need = o_msg + (size_t)CI_MSG_BYTES * T;
  if (D.h_buf.cap < h_need && !D.h_buf.reserve(h_need)) return FTS_API_ENOMEM;
  if (D.d_buf.cap < d_need && !D.d_buf.reserve(d_need)) return FTS_API_ENOMEM;
  uint8_t* h = D.h_buf.as<uint8_t>();
  uint8_t* d = D.d_buf.as<uint8_t>();
  // an issue stages E and S on the host and the device and leaves (isk + E)^-1, the products
  // and the lane tables in the scratch: wiped on every way out
  SecretWipe wipe_rec(D.stream), wipe_scr(D.stream);
  if (issue) {
    wipe_rec.host = h, wipe_rec.dev = d, wipe_rec.bytes = rec_b;
    wipe_scr.dev = d + o_scr, wipe_scr.bytes = d_need - o_scr;
  }
  CredReqChain c;
  c.s = D.stream, c.ev_mid = D.ev[1];
  c.rec = reinterpret_cast<const uint32_t*>(d), c.pts = d + o_pts, c.st = reinterpret_cast<int32_t*>(d + o_st);
  c.out = reinterpret_cast<uint32_t*>(d + o_out), c.scr = reinterpret_cast<uint32_t*>(d + o_scr), c.msg = d + o_msg;
  c.tables = v.tables, c.hk = v.hash, c.isk = issue ? K->d_isk.as<uint32_t>() : nullptr;
  float ms[2] = {0.f, 0.f};
  double host_s[2] = {0., 0.};
  const size_t CH = 512;
  for (size_t base = 0; base < n; base += T) {
    const size_t m = std::min(T, n - base), nch = (m + CH - 1) / CH;
    const double t0 = now_s();
    host_parallel_for(nch, [&](size_t ch) {
      credis::ReqFields f;
      for (size_t j = ch * CH; j < std::min(m, (ch + 1) * CH); j++) {
        const size_t i = base + j;
        const auto rq = get(i);
        uint32_t* R = reinterpret_cast<uint32_t*>(h) + j * CI_REC_WORDS;
        memset(R, 0, CI_REC_WORDS * 4);
        int32_t st = credis::parse_request(rq.first, rq.second, bn, f);
        if (issue) {
          // a value the caller holds out of range is the caller's error, whatever the request says
          const uint8_t* at = items[i].attrs4x32;
          for (int a = 0; a < 4 && at; a++)
            if (!u256::be_limbs(at + 32 * a, 32, R + CI_R_ATTR + 8 * a) || u256::ge(R + CI_R_ATTR + 8 * a, rmod))
              at = nullptr;
          if (!at) st = FTS_E_SIGN_BADKEY;
          // the item's own stream: E, then S, whatever becomes of the other items
          credis::issue_draws(bn, src->at(i), K->avoid, R + CI_R_E, R + CI_R_BIGS);
        }
        if (st == FTS_OK) {
          memcpy(R + CI_R_CCMP, f.c_cmp, 32), memcpy(R + CI_R_CMUL, f.c_mul, 32);
          memcpy(R + CI_R_S, f.s, 32), memcpy(R + CI_R_NONCE, f.nonce_be, 32);
          memcpy(h + o_pts + j * 64, f.nym, 64);
        } else {
          memset(R, 0, CI_REC_WORDS * 4), memset(h + o_pts + j * 64, 0, 64);
        }
        reinterpret_cast<int32_t*>(h + o_st)[j] = st;
      }
    });
    host_s[0] += now_s() - t0;
    c.n = (int)m;
    CCHK(hipMemcpyAsync(d, h, o_st + m * 4, hipMemcpyHostToDevice, D.stream));
    CCHK(hipEventRecord(D.ev[0], D.stream));
    CCHK(bn ? launch_credissue<BnCurve>(c, issue) : launch_credissue<FbnCurve>(c, issue));
    CCHK(hipGetLastError());
    CCHK(hipEventRecord(D.ev[2], D.stream));
    CCHK(hipMemcpyAsync(h + o_st, d + o_st, m * 4, hipMemcpyDeviceToHost, D.stream));
    if (issue) CCHK(hipMemcpyAsync(h + o_out, d + o_out, m * CI_OUT_WORDS * 4, hipMemcpyDeviceToHost, D.stream));
    CCHK(hipStreamSynchronize(D.stream));
    const double t1 = now_s();
    const int32_t* hst = reinterpret_cast<const int32_t*>(h + o_st);
    if (!issue) {
      memcpy(status + base, hst, m * 4);
    } else {
      host_parallel_for(nch, [&](size_t ch) {
        for (size_t j = ch * CH; j < std::min(m, (ch + 1) * CH); j++) {
          const size_t i = base + j;
          status[i] = hst[j];
          uint8_t* o = creds + i * stride;
          if (hst[j] != FTS_OK) {
            memset(o, 0, credis::CRED_LEN);
            cred_len[i] = 0;
            continue;
          }
          const uint32_t* R = reinterpret_cast<const uint32_t*>(h) + j * CI_REC_WORDS;
          const uint8_t* O = h + o_out + j * CI_OUT_WORDS * 4;
          uint8_t es[2][32];
          idgen::limbs_to_be32(R + CI_R_E, es[0]);
          idgen::limbs_to_be32(R + CI_R_BIGS, es[1]);
          credis::write_credential(O, O + 64, es[0], es[1], items[i].attrs4x32, o);
          wipe_bytes(es, sizeof es);
          cred_len[i] = (uint32_t)credis::CRED_LEN;
        }
      });
    }
    host_s[1] += now_s() - t1;
    float a = 0.f, b = 0.f;
    if (issue) {
      CCHK(hipEventElapsedTime(&a, D.ev[0], D.ev[1]));
      CCHK(hipEventElapsedTime(&b, D.ev[1], D.ev[2]));
    } else {
      CCHK(hipEventElapsedTime(&a, D.ev[0], D.ev[2]));
    }
    ms[0] += a, ms[1] += b;
  }
  D.ms[0] = ms[0], D.ms[1] = ms[1];
  D.host_s[0] = host_s[0], D.host_s[1] = host_s[1];
  return FTS_API_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// The wallet's side: NewCredRequest
// ---------------------------------------------------------------------------
int fts_idemix_cred_request_batch(fts_idemix_idv* idvh, size_t n, const uint8_t* sk32, const uint8_t* nonce32,
                                  uint64_t seed, uint8_t* out, size_t stride, uint32_t* len, int32_t* status) {
  if (!idvh || n > CI_MAX) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  if (!out || !len || !status) return FTS_API_EINVAL;
  if (stride < credis::REQ_LEN) return FTS_API_ESIZE;
  const IssuerView iv = idv_issuer_view(idvh);
  const IdvView& v = iv.v;
  const bool bn = v.curve == FTS_CURVE_BN254;
  const uint32_t* const rmod = bn ? u256::kRbn : u256::kRfbn;
  const host::RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  CredReqState* const Q = iv.rq;
  auto guard = Q->ring.acquire([Q](CiSlot& S) { Q->last_ms[0] = S.ms[0]; });
  CiSlot& D = guard.slot();
  CCHK(hipSetDevice(v.device));
  const size_t T = std::min(n, CI_TILE);
  // host: rec | status | out; device: rec | status | out | transcript
  const size_t rec_b = T * CIQ_REC_WORDS * 4, out_b = T * CI_OUT_WORDS * 4;
  const size_t o_st = al(rec_b), o_out = al(o_st + T * 4), h_need = al(o_out + out_b);
  const size_t o_msg = h_need, d_need = o_msg + (size_t)CI_MSG_BYTES * T;
  if (D.h_buf.cap < h_need && !D.h_buf.reserve(h_need)) return FTS_API_ENOMEM;
  if (D.d_buf.cap < d_need && !D.d_buf.reserve(d_need)) return FTS_API_ENOMEM;
  uint8_t* h = D.h_buf.as<uint8_t>();
  uint8_t* d = D.d_buf.as<uint8_t>();
  // sk and rSk staged on the host and the device; t = HSk rSk in the transcript: wiped on every way out
  SecretWipe wipe_rec(D.stream), wipe_msg(D.stream);
  wipe_rec.host = h, wipe_rec.dev = d, wipe_rec.bytes = rec_b;
  wipe_msg.dev = d + o_msg, wipe_msg.bytes = d_need - o_msg;
  CredReqChain c{};
  c.s = D.stream, c.rec = reinterpret_cast<const uint32_t*>(d), c.st = reinterpret_cast<int32_t*>(d + o_st);
  c.out = reinterpret_cast<uint32_t*>(d + o_out), c.msg = d + o_msg, c.tables = v.tables, c.hk = v.hash;
  float ms = 0.f;
  const size_t CH = 512;
  for (size_t base = 0; base < n; base += T) {
    const size_t m = std::min(T, n - base), nch = (m + CH - 1) / CH;
    host_parallel_for(nch, [&](size_t ch) {
      for (size_t j = ch * CH; j < std::min(m, (ch + 1) * CH); j++) {
        const size_t i = base + j;
        uint32_t* R = reinterpret_cast<uint32_t*>(h) + j * CIQ_REC_WORDS;
        uint32_t nonce[8];
        int32_t st = FTS_OK;
        if (!sk32 || !nonce32 || !u256::be_limbs(sk32 + 32 * i, 32, R) || u256::ge(R, rmod)) st = FTS_E_SIGN_BADKEY;
        credis::request_draw(bn, src.at(i), R + 8);
        if (st == FTS_OK) {
          u256::be_limbs(nonce32 + 32 * i, 32, nonce);
          for (int k = 0; k < 8; k++) R[16 + k] = nonce[7 - k];
        } else {
          memset(R, 0, CIQ_REC_WORDS * 4);
        }
        reinterpret_cast<int32_t*>(h + o_st)[j] = st;
      }
    });
    c.n = (int)m;
    CCHK(hipMemcpyAsync(d, h, o_st + m * 4, hipMemcpyHostToDevice, D.stream));
    CCHK(hipEventRecord(D.ev[0], D.stream));
    bn ? launch_credreq_make<BnCurve>(c) : launch_credreq_make<FbnCurve>(c);
    CCHK(hipGetLastError());
    CCHK(hipEventRecord(D.ev[2], D.stream));
    CCHK(hipMemcpyAsync(h + o_out, d + o_out, m * CI_OUT_WORDS * 4, hipMemcpyDeviceToHost, D.stream));
    CCHK(hipStreamSynchronize(D.stream));
    const int32_t* hst = reinterpret_cast<const int32_t*>(h + o_st);
    host_parallel_for(nch, [&](size_t ch) {
      for (size_t j = ch * CH; j < std::min(m, (ch + 1) * CH); j++) {
        const size_t i = base + j;
        status[i] = hst[j];
        uint8_t* o = out + i * stride;
        if (hst[j] != FTS_OK) {
          memset(o, 0, credis::REQ_LEN);
          len[i] = 0;
          continue;
        }
        const uint8_t* O = h + o_out + j * CI_OUT_WORDS * 4;  // Nym (X || Y), c, s
        credis::write_request(O, nonce32 + 32 * i, O + 64, O + 96, o);
        len[i] = (uint32_t)credis::REQ_LEN;
      }
    });
    float a = 0.f;
    CCHK(hipEventElapsedTime(&a, D.ev[0], D.ev[2]));
    ms += a;
  }
  D.ms[0] = ms;
  return FTS_API_OK;
}

// ---------------------------------------------------------------------------
// CredRequest.Check
// ---------------------------------------------------------------------------
int fts_idemix_cred_request_verify_batch(fts_idemix_idv* idvh, size_t n, const fts_idemix_credreq_item* items,
                                         int32_t* status) {
  if (!idvh || n > CI_MAX || (n && (!items || !status))) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  const IssuerView iv = idv_issuer_view(idvh);
  CredReqState* const Q = iv.rq;
  auto guard = Q->ring.acquire([Q](CiSlot& S) { Q->last_ms[1] = S.ms[1]; });
  CiSlot& D = guard.slot();
  const int r = check_or_issue(
      iv.v, D, n, [items](size_t i) { return std::make_pair(items[i].req, items[i].req_len); }, nullptr, nullptr,
      nullptr, nullptr, 0, nullptr, status);
  D.ms[1] = D.ms[0];  // this ring's [0] is the request generator's
  return r;
}

int fts_idemix_cred_request_last_timings(fts_idemix_idv* idvh, float* ms2) {
  if (!idvh || !ms2) return FTS_API_EINVAL;
  CredReqState* const Q = idv_issuer_view(idvh).rq;
  std::lock_guard<std::mutex> l(Q->ring.mu);
  ms2[0] = Q->last_ms[0], ms2[1] = Q->last_ms[1];
  return FTS_API_OK;
}

// ---------------------------------------------------------------------------
// The issuer: CredRequest.Check, then NewCredential
// ---------------------------------------------------------------------------
int fts_idemix_issuer_create(fts_idemix_idv* idvh, const uint8_t* isk32, fts_idemix_issuer** out) {
  if (!out) return FTS_API_EINVAL;
  *out = nullptr;
  if (!idvh || !isk32) return FTS_API_EINVAL;
  std::unique_ptr<fts_idemix_issuer> k(new fts_idemix_issuer());
  k->iv.v.device = -1;
  memset(k->avoid, 0, sizeof k->avoid);
  const IssuerView iv = idv_issuer_view(idvh);
  const bool bn = iv.v.curve == FTS_CURVE_BN254;
  const uint32_t* const rmod = bn ? u256::kRbn : u256::kRfbn;
  // host staging of the secret, wiped on every way out
  struct Stage {
    uint32_t isk[8];
    ~Stage() { wipe_bytes(this, sizeof(Stage)); }
  } st;
  if (!u256::be_limbs(isk32, 32, st.isk) || u256::ge(st.isk, rmod) || idgen::is_zero8(st.isk) || !iv.bar)
    return FTS_API_EPP;
  CCHK(hipSetDevice(iv.v.device));
  k->iv = iv, k->bn = bn;  // from here on the destructor wipes the device buffer
  memcpy(k->avoid, rmod, 32);
  u256::sub(k->avoid, st.isk);
  Stream s0;
  DevBuf bar_buf, ok_buf;
  bool ok = s0.create() == hipSuccess && k->d_isk.reserve(64) && bar_buf.reserve(128) && ok_buf.reserve(64);
  int32_t hok = 0;
  ok = ok && hipMemcpyAsync(k->d_isk.p, st.isk, 32, hipMemcpyHostToDevice, s0) == hipSuccess &&
       hipMemcpyAsync(bar_buf.p, iv.bar, 128, hipMemcpyHostToDevice, s0) == hipSuccess &&
       hipMemsetAsync(ok_buf.p, 0, 64, s0) == hipSuccess;
  if (ok) {
    if (bn) launch_credissue_key<BnCurve>(bar_buf.as<uint8_t>(), k->d_isk.as<uint32_t>(), ok_buf.as<int32_t>(), s0);
    else launch_credissue_key<FbnCurve>(bar_buf.as<uint8_t>(), k->d_isk.as<uint32_t>(), ok_buf.as<int32_t>(), s0);
    ok = hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(&hok, ok_buf.p, sizeof hok, hipMemcpyDeviceToHost, s0) == hipSuccess;
  }
  if (s0) ok = hipStreamSynchronize(s0) == hipSuccess && ok;
  if (!ok) return FTS_API_EDEVICE;
  if (hok != 1) return FTS_API_EPP;
  if (!make_slots(k->ring)) return FTS_API_EDEVICE;
  *out = k.release();
  return FTS_API_OK;
}

void fts_idemix_issuer_destroy(fts_idemix_issuer* k) { delete k; }

int fts_idemix_cred_issue_batch(fts_idemix_issuer* K, size_t n, const fts_idemix_issue_item* items, uint64_t seed,
                                uint8_t* creds, size_t stride, uint32_t* cred_len, int32_t* status) {
  if (!K || n > CI_MAX) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  if (!items || !creds || !cred_len || !status) return FTS_API_EINVAL;
  if (stride < credis::CRED_LEN) return FTS_API_ESIZE;
  const host::RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  auto guard = K->ring.acquire([K](CiSlot& S) {
    K->last_ms[0] = S.ms[0], K->last_ms[1] = S.ms[1];
    K->last_host_s[0] = S.host_s[0], K->last_host_s[1] = S.host_s[1];
  });
  return check_or_issue(
      K->iv.v, guard.slot(), n, [items](size_t i) { return std::make_pair(items[i].req, items[i].req_len); }, K, items,
      &src, creds, stride, cred_len, status);
}

int fts_idemix_cred_issue_last_timings(fts_idemix_issuer* K, float* ms2, double* host_s2) {
  if (!K || !ms2) return FTS_API_EINVAL;
  std::lock_guard<std::mutex> l(K->ring.mu);
  ms2[0] = K->last_ms[0], ms2[1] = K->last_ms[1];
  if (host_s2) host_s2[0] = K->last_host_s[0], host_s2[1] = K->last_host_s[1];
  return FTS_API_OK;
}

// ---------------------------------------------------------------------------
// Host-only entries (tests)
// ---------------------------------------------------------------------------
int fts_debug_idemix_cred_issue_draws(int curve_id, uint64_t seed, uint64_t i, const uint8_t* avoid_e32,
                                      uint8_t* out3x32) {
  if (!out3x32 || seed == FTS_SEED_OS_RANDOM || (curve_id != FTS_CURVE_BN254 && curve_id != FTS_CURVE_FP256BN_AMCL))
    return FTS_API_EINVAL;
  const bool bn = curve_id == FTS_CURVE_BN254;
  uint32_t avoid[8], d[3][8];
  if (avoid_e32 && !u256::be_limbs(avoid_e32, 32, avoid)) return FTS_API_EINVAL;
  credis::issue_draws(bn, host::Rng(seed + i), avoid_e32 ? avoid : nullptr, d[0], d[1]);
  credis::request_draw(bn, host::Rng(seed + i), d[2]);
  for (int k = 0; k < 3; k++) idgen::limbs_to_be32(d[k], out3x32 + 32 * k);
  return FTS_API_OK;
}

int fts_debug_idemix_credreq_parse(int curve_id, const uint8_t* req, size_t req_len, int32_t* status,
                                   uint8_t* out160) {
  if (!status || !out160 || (curve_id != FTS_CURVE_BN254 && curve_id != FTS_CURVE_FP256BN_AMCL)) return FTS_API_EINVAL;
  credis::ReqFields f;
  *status = credis::parse_request(req, req_len, curve_id == FTS_CURVE_BN254, f);
  memcpy(out160, f.nym, 64);
  for (int k = 0; k < 8; k++)
    for (int b = 0; b < 4; b++) out160[64 + 4 * k + b] = (uint8_t)(f.nonce_be[k] >> (24 - 8 * b));
  idgen::limbs_to_be32(f.c_cmp, out160 + 96);
  idgen::limbs_to_be32(f.s, out160 + 128);
  return FTS_API_OK;
}

int fts_debug_idemix_credreq_write(const uint8_t* nym64, const uint8_t* nonce32, const uint8_t* c32, const uint8_t* s32,
                                   uint8_t* out) {
  if (!nym64 || !nonce32 || !c32 || !s32 || !out) return FTS_API_EINVAL;
  credis::write_request(nym64, nonce32, c32, s32, out);
  return FTS_API_OK;
}

int fts_debug_idemix_credential_write(const uint8_t* a64, const uint8_t* b64, const uint8_t* e32, const uint8_t* s32,
                                      const uint8_t* attrs4x32, uint8_t* out) {
  if (!a64 || !b64 || !e32 || !s32 || !attrs4x32 || !out) return FTS_API_EINVAL;
  credis::write_credential(a64, b64, e32, s32, attrs4x32, out);
  return FTS_API_OK;
}

}  // extern "C"
