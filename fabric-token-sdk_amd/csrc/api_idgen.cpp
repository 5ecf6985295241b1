// C-ABI (include/fts_gpu.h): idemix owner identities generated on the device --
// fts_idemix_cred (one wallet's credential: tables of A and B, its constant points) and
// fts_idemix_identity_generate_batch.  The draws, the parsers and the identity writer are
// host/identity_write.hpp; the kernels are reached through device/launch.hpp
// (idemix_idgen_{bn,fbn}.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <memory>
#include <mutex>

#include "../../include/fts_gpu.h"
#include "device/launch.hpp"
#include "host/bn254_host.hpp"
#include "host/hip_owned.hpp"
#include "host/host_pool.hpp"
#include "host/identity_write.hpp"
#include "host/idemix_parse.hpp"
#include "host/prover.hpp"  // Rng, RngSource

using namespace fts;
using namespace idv;

#define GCHK(x)                                    \
  do {                                             \
    if ((x) != hipSuccess) return FTS_API_EDEVICE; \
  } while (0)

namespace {

constexpr int GEN_NSLOT = 3;           // calls in flight per credential
constexpr size_t GEN_TILE = 16384;     // identities per kernel sequence: bounds a slot's buffers (4.4 KB per identity,
                                       // 72 MB per slot) and still puts 2,816 waves on the device in k_idg_points
constexpr size_t GEN_MAX = (size_t)1 << 22;
struct GenSlot {
  Stream stream;
  DevBuf d_buf;  // draws | scalar slots (the secret region) | points | prefix products | transcript | out | status
  PinBuf h_buf;  // draws | out | status
  Event ev[3];
  float ms[2] = {0.f, 0.f};
  double host_s[2] = {0., 0.};
};

double now_s() {
  timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

}  // namespace

struct fts_idemix_cred {
  fts_idemix_idv* idv = nullptr;  // borrowed: device, issuer tables, ipk.Hash
  IdvView v{};
  bool bn = true;
  DevBuf d_tables;  // A, B
  DevBuf d_sec;     // sk E S attrs | HSk sk, HAttrs[2] a_eid, HAttrs[3] a_rh, mask
  idgen::CriFields cri;
  size_t id_len = 0;
  SlotRing<GenSlot, GEN_NSLOT> ring;
  float last_ms[2] = {0.f, 0.f};       // under ring.mu
  double last_host_s[2] = {0., 0.};    // under ring.mu: draws + staging, serialisation
  // the secrets this handle holds on the device are zeroed before they are freed
  void wipe() {
    if (v.device < 0 || hipSetDevice(v.device) != hipSuccess) return;
    if (d_sec.p) (void)hipMemset(d_sec.p, 0, d_sec.cap);
    if (d_tables.p) (void)hipMemset(d_tables.p, 0, d_tables.cap);
    (void)hipDeviceSynchronize();
  }
  ~fts_idemix_cred() { wipe(); }
};

extern "C" {

int fts_idemix_cred_create(fts_idemix_idv* idvh, const uint8_t* cred, size_t cred_len, const uint8_t* sk32,
                           const uint8_t* cri, size_t cri_len, fts_idemix_cred** out) {
  if (!out) return FTS_API_EINVAL;
  *out = nullptr;
  if (!idvh || !cred || !cred_len || !sk32 || (!cri && cri_len)) return FTS_API_EINVAL;
  std::unique_ptr<fts_idemix_cred> k(new fts_idemix_cred());
  k->v.device = -1;
  const IdvView v = idv_view(idvh);
  const bool bn = v.curve == FTS_CURVE_BN254;
  // host staging of the secrets, wiped on every way out
  struct Stage {
    idgen::CredFields f;
    uint32_t sec[IDG_SEC_WORDS];
    uint32_t bases[32];  // A and B as the table builders take them
    host::G1A pt;
    ~Stage() {
      volatile uint8_t* p = reinterpret_cast<volatile uint8_t*>(this);
      for (size_t i = 0; i < sizeof(Stage); i++) p[i] = 0;
    }
  } st;
  if (!idgen::parse_credential(cred, cred_len, bn, st.f) || !idgen::parse_cri(cri, cri_len, bn, k->cri))
    return FTS_API_EPP;
  uint32_t* const sec = st.sec;
  if (!u256::be_limbs(sk32, 32, sec) || u256::ge(sec, bn ? u256::kRbn : u256::kRfbn)) return FTS_API_EPP;
  memcpy(sec + 8, st.f.e, 32);
  memcpy(sec + 16, st.f.s, 32);
  memcpy(sec + 24, st.f.attrs, 128);
  // A and B as the table builders take them: BN254 Montgomery (decoded and on-curve checked
  // here; the identity is rejected), FP256BN plain limbs (checked on the device)
  uint32_t* const bases = st.bases;
  const uint8_t* const raw[2] = {st.f.a, st.f.b};
  for (int b = 0; b < 2; b++) {
    if (bn) {
      host::G1A& a = st.pt;
      if (!host::g1_from_bytes(raw[b], 64, a) || a.inf) return FTS_API_EPP;
      memcpy(&bases[b * 16], a.x.v, 32);
      memcpy(&bases[b * 16 + 8], a.y.v, 32);
    } else {
      u256::be_limbs(raw[b], 32, &bases[b * 16]);
      u256::be_limbs(raw[b] + 32, 32, &bases[b * 16 + 8]);
    }
  }
  GCHK(hipSetDevice(v.device));
  k->idv = idvh, k->v = v, k->bn = bn;  // from here on the destructor wipes the device buffers
  k->id_len = idgen::identity_len(bn, k->cri.epoch);
  const size_t wpb = bn ? fb_words_per_base() : fbn_words_per_base();
  Stream s0;
  DevBuf bases_buf, scr_buf, ok_buf;
  const size_t scr_b = bn ? table_build_scratch_bytes(2) : 2 * 16 * 4;
  bool ok = s0.create() == hipSuccess && k->d_tables.reserve(2 * wpb * 4) &&
            k->d_sec.reserve((IDG_SEC_WORDS + IDG_CPT_WORDS) * 4) && bases_buf.reserve(sizeof st.bases) &&
            scr_buf.reserve(scr_b) && ok_buf.reserve(64);
  uint32_t* const d_sec = k->d_sec.as<uint32_t>();
  uint32_t* const d_bases = bases_buf.as<uint32_t>();
  int32_t* const d_ok = ok_buf.as<int32_t>();
  ok = ok && hipMemcpyAsync(d_bases, bases, sizeof st.bases, hipMemcpyHostToDevice, s0) == hipSuccess &&
       hipMemcpyAsync(d_sec, sec, IDG_SEC_WORDS * 4, hipMemcpyHostToDevice, s0) == hipSuccess &&
       hipMemsetAsync(d_ok, 0, 64, s0) == hipSuccess;
  int32_t hok[3] = {0, 0, 0};  // A, B on the curve (FP256BN), the B check
  if (ok) {
    if (bn) {
      launch_build_tables(d_bases, 2, k->d_tables.as<uint32_t>(), scr_buf.as<uint32_t>(), s0);
      launch_idgen_cred<BnCurve>(v.tables, d_bases, d_sec, d_sec + IDG_SEC_WORDS, d_ok + 2, s0);
    } else {
      fbn_build_tables(d_bases, 2, scr_buf.as<uint32_t>(), d_ok, k->d_tables.as<uint32_t>(), s0);
      launch_idgen_cred<FbnCurve>(v.tables, scr_buf.as<uint32_t>(), d_sec, d_sec + IDG_SEC_WORDS, d_ok + 2, s0);
    }
    ok = hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(hok, d_ok, sizeof hok, hipMemcpyDeviceToHost, s0) == hipSuccess;
  }
  // the staged copies of A and B go with the call, zeroed
  if (bases_buf.p) (void)hipMemsetAsync(bases_buf.p, 0, sizeof st.bases, s0);
  if (scr_buf.p && !bn) (void)hipMemsetAsync(scr_buf.p, 0, scr_b, s0);
  if (s0) ok = hipStreamSynchronize(s0) == hipSuccess && ok;
  if (!ok) return FTS_API_EDEVICE;
  if (hok[2] != 1 || (!bn && (hok[0] != 1 || hok[1] != 1))) return FTS_API_EPP;
  for (auto& S : k->ring.slot) {
    ok = ok && S.stream.create() == hipSuccess;
    for (auto& e : S.ev) ok = ok && e.create() == hipSuccess;
  }
  if (!ok) return FTS_API_EDEVICE;
  *out = k.release();
  return FTS_API_OK;
}

void fts_idemix_cred_destroy(fts_idemix_cred* k) { delete k; }

size_t fts_idemix_identity_len(const fts_idemix_cred* c) { return c ? c->id_len : 0; }

int fts_debug_idemix_identity_draws(int curve_id, uint64_t seed, uint64_t i, uint8_t* out18x32) {
  if (!out18x32 || seed == FTS_SEED_OS_RANDOM || (curve_id != FTS_CURVE_BN254 && curve_id != FTS_CURVE_FP256BN_AMCL))
    return FTS_API_EINVAL;
  uint32_t d[idgen::ND][8];
  idgen::identity_draws(curve_id == FTS_CURVE_BN254, host::Rng(seed + i), d);
  for (int k = 0; k < idgen::ND; k++) idgen::limbs_to_be32(d[k], out18x32 + 32 * k);
  return FTS_API_OK;
}

int fts_debug_idemix_identity_write(int curve_id, const uint8_t* pts6x64, const uint8_t* sc13x32,
                                    const uint8_t* nonce32, const uint8_t* epoch_pk128, uint64_t epoch, uint8_t* out,
                                    size_t out_cap, size_t* out_len) {
  if (!pts6x64 || !sc13x32 || !nonce32 || !out_len || (int64_t)epoch < 0 ||
      (curve_id != FTS_CURVE_BN254 && curve_id != FTS_CURVE_FP256BN_AMCL))
    return FTS_API_EINVAL;
  const bool bn = curve_id == FTS_CURVE_BN254;
  *out_len = idgen::identity_len(bn, epoch);
  if (!out || out_cap < *out_len) return FTS_API_ESIZE;
  const idgen::IdentityParts v{pts6x64, sc13x32, nonce32, epoch_pk128 ? epoch_pk128 : (bn ? idgen::kG2Bn : idgen::kG2Fbn),
                               epoch};
  idgen::write_identity(bn, v, out);
  return FTS_API_OK;
}

int fts_idemix_identity_generate_batch(fts_idemix_cred* K, size_t n, uint64_t seed, const uint8_t* r_eid_in32,
                                       const uint8_t* r_rh_in32, uint8_t* ids, size_t id_stride, uint32_t* id_len,
                                       uint8_t* rnym32, uint8_t* r_eid32, uint8_t* r_rh32, int32_t* status) {
  if (!K || n > GEN_MAX) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  if (!ids || !id_len || !rnym32 || !r_eid32 || !r_rh32 || !status) return FTS_API_EINVAL;
  if (id_stride < K->id_len) return FTS_API_ESIZE;
  const bool bn = K->bn;
  const uint32_t* const rmod = bn ? u256::kRbn : u256::kRfbn;
  const host::RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  auto guard = K->ring.acquire([K](GenSlot& S) {
    K->last_ms[0] = S.ms[0], K->last_ms[1] = S.ms[1];
    K->last_host_s[0] = S.host_s[0], K->last_host_s[1] = S.host_s[1];
  });
  GenSlot& D = guard.slot();
  GCHK(hipSetDevice(K->v.device));
  const size_t T = std::min(n, GEN_TILE);
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  // host: draws | out | status; device: draws | scalar slots | points | prefix | transcript | out | status
  const size_t draws_b = T * IDG_ND * 32, out_b = T * IDG_OUT_WORDS * 4, st_b = T * 4;
  const size_t ho_out = al(draws_b), ho_st = al(ho_out + out_b), h_need = ho_st + st_b;
  const size_t do_sc = al(draws_b), sec_b = al(do_sc + T * IDG_NSC * 32), do_pts = sec_b,
               do_pre = al(do_pts + T * IDG_NPT * 24 * 4), do_msg = al(do_pre + T * IDG_NPT * 32),
               do_out = al(do_msg + T * MSG_MAX), do_st = al(do_out + out_b), d_need = do_st + st_b;
  if (D.h_buf.cap < h_need && !D.h_buf.reserve(h_need)) return FTS_API_ENOMEM;
  if (D.d_buf.cap < d_need && !D.d_buf.reserve(d_need)) return FTS_API_ENOMEM;
  uint8_t* h = D.h_buf.as<uint8_t>();
  uint8_t* d = D.d_buf.as<uint8_t>();
  // the staged draws and the scalars derived from them are wiped on every way out
  SecretWipe wipe_h(D.stream), wipe_d(D.stream);
  wipe_h.host = h, wipe_h.bytes = draws_b;
  wipe_d.dev = d, wipe_d.bytes = sec_b;
  GenChain c;
  c.s = D.stream, c.ev_mid = D.ev[1];
  c.draws = reinterpret_cast<const uint32_t*>(d), c.sec = K->d_sec.as<uint32_t>(), c.cpt = c.sec + IDG_SEC_WORDS;
  c.sc = reinterpret_cast<uint32_t*>(d + do_sc), c.pts = reinterpret_cast<uint32_t*>(d + do_pts);
  c.pre = reinterpret_cast<uint32_t*>(d + do_pre), c.msg = d + do_msg;
  c.itab = K->v.tables, c.ctab = K->d_tables.as<uint32_t>(), c.hash = K->v.hash;
  c.out = reinterpret_cast<uint32_t*>(d + do_out), c.st = reinterpret_cast<const int32_t*>(d + do_st);
  float ms[2] = {0.f, 0.f};
  double host_s[2] = {0., 0.};
  const size_t CH = 512;
  for (size_t base = 0; base < n; base += T) {
    const size_t m = std::min(T, n - base), nch = (m + CH - 1) / CH;
    const double t0 = now_s();
    host_parallel_for(nch, [&](size_t ch) {
      for (size_t j = ch * CH; j < std::min(m, (ch + 1) * CH); j++) {
        const size_t i = base + j;
        uint32_t(*R)[8] = reinterpret_cast<uint32_t(*)[8]>(h + j * IDG_ND * 32);
        idgen::identity_draws(bn, src.at(i), R);
        int32_t st = FTS_OK;
        // fixed audit randoms: the drawn value is consumed above, then replaced
        if (r_eid_in32 && (!u256::be_limbs(r_eid_in32 + 32 * i, 32, R[idgen::D_REID]) || u256::ge(R[idgen::D_REID], rmod)))
          st = FTS_E_SIGN_BADKEY;
        if (r_rh_in32 && (!u256::be_limbs(r_rh_in32 + 32 * i, 32, R[idgen::D_RRH]) || u256::ge(R[idgen::D_RRH], rmod)))
          st = FTS_E_SIGN_BADKEY;
        if (st != FTS_OK) memset(R, 0, IDG_ND * 32);
        reinterpret_cast<int32_t*>(h + ho_st)[j] = st;
      }
    });
    host_s[0] += now_s() - t0;
    c.n = (int)m;
    GCHK(hipMemcpyAsync(d, h, m * IDG_ND * 32, hipMemcpyHostToDevice, D.stream));
    GCHK(hipMemcpyAsync(d + do_st, h + ho_st, m * 4, hipMemcpyHostToDevice, D.stream));
    GCHK(hipEventRecord(D.ev[0], D.stream));
    GCHK(bn ? launch_idgen<BnCurve>(c) : launch_idgen<FbnCurve>(c));
    GCHK(hipGetLastError());
    GCHK(hipEventRecord(D.ev[2], D.stream));
    GCHK(hipMemcpyAsync(h + ho_out, d + do_out, m * IDG_OUT_WORDS * 4, hipMemcpyDeviceToHost, D.stream));
    GCHK(hipStreamSynchronize(D.stream));
    const double t1 = now_s();
    host_parallel_for(nch, [&](size_t ch) {
      for (size_t j = ch * CH; j < std::min(m, (ch + 1) * CH); j++) {
        const size_t i = base + j;
        const int32_t st = reinterpret_cast<const int32_t*>(h + ho_st)[j];
        status[i] = st;
        uint8_t* o = ids + i * id_stride;
        if (st != FTS_OK) {
          memset(o, 0, K->id_len);
          memset(rnym32 + 32 * i, 0, 32), memset(r_eid32 + 32 * i, 0, 32), memset(r_rh32 + 32 * i, 0, 32);
          id_len[i] = 0;
          continue;
        }
        const uint32_t(*R)[8] = reinterpret_cast<const uint32_t(*)[8]>(h + j * IDG_ND * 32);
        const uint8_t* O = h + ho_out + j * IDG_OUT_WORDS * 4;
        uint8_t nonce[32];
        idgen::limbs_to_be32(R[idgen::D_NONCE], nonce);
        const idgen::IdentityParts v{O, O + 6 * 64, nonce, K->cri.epoch_pk, K->cri.epoch};
        idgen::write_identity(bn, v, o);
        id_len[i] = (uint32_t)K->id_len;
        idgen::limbs_to_be32(R[idgen::D_RNYM], rnym32 + 32 * i);
        idgen::limbs_to_be32(R[idgen::D_REID], r_eid32 + 32 * i);
        idgen::limbs_to_be32(R[idgen::D_RRH], r_rh32 + 32 * i);
      }
    });
    host_s[1] += now_s() - t1;
    float a = 0.f, b = 0.f;
    GCHK(hipEventElapsedTime(&a, D.ev[0], D.ev[1]));
    GCHK(hipEventElapsedTime(&b, D.ev[1], D.ev[2]));
    ms[0] += a, ms[1] += b;
  }
  D.ms[0] = ms[0], D.ms[1] = ms[1];
  D.host_s[0] = host_s[0], D.host_s[1] = host_s[1];
  return FTS_API_OK;
}

int fts_idemix_identity_generate_last_timings(fts_idemix_cred* K, float* ms2, double* host_s2) {
  if (!K || !ms2) return FTS_API_EINVAL;
  std::lock_guard<std::mutex> l(K->ring.mu);
  ms2[0] = K->last_ms[0], ms2[1] = K->last_ms[1];
  if (host_s2) host_s2[0] = K->last_host_s[0], host_s2[1] = K->last_host_s[1];
  return FTS_API_OK;
}

}  // extern "C"
