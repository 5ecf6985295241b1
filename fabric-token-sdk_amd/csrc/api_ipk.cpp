// C-ABI (include/fts_gpu.h): idemix issuer keys on the device -- IssuerPublicKey.Check for a
// batch of keys (fts_idemix_ipk_check_batch) and NewIssuerKey (fts_idemix_issuer_keygen_batch).
// Neither takes a handle: they run when a key is imported or made, so each call owns its stream
// and buffers.  The reading of the untrusted key, the draws and the writer are
// host/ipk_write.hpp; the kernels are reached through device/launch.hpp
// (idemix_ipk_{bn,fbn}.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "../../include/fts_gpu.h"
#include "device/launch.hpp"
#include "host/hip_owned.hpp"
#include "host/host_pool.hpp"
#include "host/ipk_write.hpp"
#include "host/prover.hpp"  // Rng, RngSource

using namespace fts;
using namespace idv;

#define KCHK(x)                                    \
  do {                                             \
    if ((x) != hipSuccess) return FTS_API_EDEVICE; \
  } while (0)

namespace {

constexpr size_t IPK_MAX = (size_t)1 << 22;
constexpr size_t IPK_TILE = 4096;  // keys per kernel sequence: bounds a call's buffers (1.3 KB per key and its HAttrs)
std::atomic<float> g_last_ms[2];   // the process's last check call, last keygen call

size_t al(size_t x) { return (x + 255) & ~size_t(255); }
void wipe_bytes(void* p, size_t n) {
  volatile uint8_t* q = reinterpret_cast<volatile uint8_t*>(p);
  for (size_t i = 0; i < n; i++) q[i] = 0;
}
bool curve_ok(int id) { return id == FTS_CURVE_BN254 || id == FTS_CURVE_FP256BN_AMCL; }
int pick_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FTS_API_EDEVICE;
  return hipSetDevice(device) == hipSuccess ? FTS_API_OK : FTS_API_EDEVICE;
}

}  // namespace

extern "C" {

int fts_idemix_ipk_check_batch(int device, int curve_id, size_t n, const uint8_t* const* ipk, const size_t* ipk_len,
                               int32_t* status, uint8_t* hash32_out) {
  if (!curve_ok(curve_id) || n > IPK_MAX) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  if (!ipk || !ipk_len || !status) return FTS_API_EINVAL;
  if (pick_device(device) != FTS_API_OK) return FTS_API_EDEVICE;
  const bool bn = curve_id == FTS_CURVE_BN254;
  Stream s;
  Event ev[2];
  KCHK(s.create());
  for (auto& e : ev) KCHK(e.create());
  DevBuf d_buf;
  PinBuf h_buf;
  // an error path may leave a copy or a kernel queued that still reads the buffers: drained before they go
  struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{s};
  const size_t T = std::min(n, IPK_TILE), CH = 64;
  std::vector<ipkw::CheckFields> F(T);
  std::vector<size_t> goff(T + 1);
  std::vector<int32_t> st0(T);
  float ms = 0.f;
  for (size_t base = 0; base < n; base += T) {
    const size_t m = std::min(T, n - base), nch = (m + CH - 1) / CH;
    host_parallel_for(nch, [&](size_t ch) {
      for (size_t j = ch * CH; j < std::min(m, (ch + 1) * CH); j++) {
        const size_t i = base + j;
        st0[j] = ipkw::parse_for_check(ipk[i], ipk_len[i], bn, F[j]);
        if (hash32_out) (void)ipkw::hash_without_field10(ipk[i], ipk[i] ? ipk_len[i] : 0, bn, hash32_out + 32 * i);
      }
    });
    goff[0] = 0;
    for (size_t j = 0; j < m; j++) goff[j + 1] = goff[j] + (st0[j] == FTS_OK ? 2 + F[j].n_attrs : 0);
    const size_t G = goff[m];
    // host and device: rec | status | bar | w | g2 | the G1 list; device only: wdec | t1 | t2 | transcript
    const size_t o_st = al(m * IPK_REC_WORDS * 4), o_bar = al(o_st + m * 4), o_w = al(o_bar + m * 128),
                 o_g2 = al(o_w + m * 128), o_g1 = al(o_g2 + 128), h_need = al(o_g1 + G * 64);
    const size_t o_wdec = h_need, o_t1 = al(o_wdec + m * 128), o_t2 = al(o_t1 + m * 128), o_msg = al(o_t2 + m * 64),
                 d_need = o_msg + (size_t)IPK_MSG_BYTES * m;
    if (!h_buf.grow(h_need) || !d_buf.grow(d_need)) return FTS_API_ENOMEM;
    uint8_t* h = h_buf.as<uint8_t>();
    uint8_t* d = d_buf.as<uint8_t>();
    memcpy(h + o_g2, bn ? idgen::kG2Bn : idgen::kG2Fbn, 128);
    host_parallel_for(nch, [&](size_t ch) {
      for (size_t j = ch * CH; j < std::min(m, (ch + 1) * CH); j++) {
        const size_t i = base + j;
        uint32_t* R = reinterpret_cast<uint32_t*>(h) + j * IPK_REC_WORDS;
        memset(R, 0, IPK_REC_WORDS * 4);
        memset(h + o_bar + j * 128, 0, 128), memset(h + o_w + j * 128, 0, 128);
        if (st0[j] == FTS_OK) {
          uint8_t* g1 = h + o_g1 + goff[j] * 64;
          memcpy(g1, F[j].h_sk, 64), memcpy(g1 + 64, F[j].h_rand, 64);
          if (!ipkw::hattrs(ipk[i], ipk_len[i], g1 + 128, F[j].n_attrs)) {
            st0[j] = FTS_E_IPK_MALFORMED;
            memset(g1, 0, (2 + F[j].n_attrs) * 64);
          }
        }
        if (st0[j] == FTS_OK) {
          memcpy(R + IPK_R_CCMP, F[j].c_cmp, 32), memcpy(R + IPK_R_A, F[j].s, 32), memcpy(R + IPK_R_B, F[j].neg_c, 32);
          R[IPK_R_OFF] = (uint32_t)goff[j], R[IPK_R_CNT] = (uint32_t)(2 + F[j].n_attrs);
          memcpy(h + o_bar + j * 128, F[j].bar, 128), memcpy(h + o_w + j * 128, F[j].w, 128);
        }
        reinterpret_cast<int32_t*>(h + o_st)[j] = st0[j];
      }
    });
    IpkChain c{};
    c.s = s, c.n = (int)m, c.rec = reinterpret_cast<const uint32_t*>(d), c.st = reinterpret_cast<int32_t*>(d + o_st);
    c.bar = d + o_bar, c.w = d + o_w, c.g2 = d + o_g2, c.g1 = d + o_g1;
    c.wdec = reinterpret_cast<uint32_t*>(d + o_wdec), c.t1 = reinterpret_cast<uint32_t*>(d + o_t1);
    c.t2 = reinterpret_cast<uint32_t*>(d + o_t2), c.msg = d + o_msg;
    KCHK(hipMemcpyAsync(d, h, h_need, hipMemcpyHostToDevice, s));
    KCHK(hipEventRecord(ev[0], s));
    bn ? launch_ipk_check<BnCurve>(c) : launch_ipk_check<FbnCurve>(c);
    KCHK(hipGetLastError());
    KCHK(hipEventRecord(ev[1], s));
    KCHK(hipMemcpyAsync(h + o_st, d + o_st, m * 4, hipMemcpyDeviceToHost, s));
    KCHK(hipStreamSynchronize(s));
    memcpy(status + base, h + o_st, m * 4);
    float a = 0.f;
    KCHK(hipEventElapsedTime(&a, ev[0], ev[1]));
    ms += a;
  }
  g_last_ms[0].store(ms);
  return FTS_API_OK;
}

int fts_idemix_issuer_keygen_batch(int device, int curve_id, size_t n, uint64_t seed, uint8_t* isk32_out,
                                   uint8_t* ipk_out, size_t ipk_stride, uint32_t* ipk_len) {
  if (!curve_ok(curve_id) || n > IPK_MAX) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  if (!isk32_out || !ipk_out || !ipk_len) return FTS_API_EINVAL;
  if (ipk_stride < ipkw::IPK_LEN) return FTS_API_ESIZE;
  const host::RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  if (pick_device(device) != FTS_API_OK) return FTS_API_EDEVICE;
  const bool bn = curve_id == FTS_CURVE_BN254;
  Stream s;
  Event ev[2];
  KCHK(s.create());
  for (auto& e : ev) KCHK(e.create());
  const size_t T = std::min(n, IPK_TILE), CH = 64;
  // host and device: draws | status | g2; then out (c, s) | W, t1 | the nine points; device only: transcript
  const size_t draw_b = T * IPK_ND * 32;
  const size_t o_st = al(draw_b), o_g2 = al(o_st + T * 4), o_out = al(o_g2 + 128), o_t1 = al(o_out + T * 64),
               o_pts = al(o_t1 + 2 * T * 128), h_need = al(o_pts + T * IPK_NPT * 64);
  const size_t o_msg = h_need, d_need = o_msg + (size_t)IPK_MSG_BYTES * T;
  DevBuf d_buf;
  PinBuf h_buf;
  if (!h_buf.reserve(h_need) || !d_buf.reserve(d_need)) return FTS_API_ENOMEM;
  uint8_t* h = h_buf.as<uint8_t>();
  uint8_t* d = d_buf.as<uint8_t>();
  // isk, r and the other draws staged on the host and the device: wiped on every way out
  SecretWipe wipe(s);
  wipe.host = h, wipe.dev = d, wipe.bytes = draw_b;
  memset(h + o_st, 0, T * 4);
  memcpy(h + o_g2, bn ? idgen::kG2Bn : idgen::kG2Fbn, 128);
  float ms = 0.f;
  for (size_t base = 0; base < n; base += T) {
    const size_t m = std::min(T, n - base), nch = (m + CH - 1) / CH;
    host_parallel_for(nch, [&](size_t ch) {
      for (size_t j = ch * CH; j < std::min(m, (ch + 1) * CH); j++) {
        host::Rng rng = src.at(base + j);
        ipkw::keygen_draws(bn, rng, reinterpret_cast<uint32_t(*)[8]>(h) + j * IPK_ND);
      }
    });
    IpkChain c{};
    c.s = s, c.n = (int)m, c.rec = reinterpret_cast<const uint32_t*>(d), c.st = reinterpret_cast<int32_t*>(d + o_st);
    c.g2 = d + o_g2, c.out = reinterpret_cast<uint32_t*>(d + o_out), c.t1 = reinterpret_cast<uint32_t*>(d + o_t1);
    c.t2 = reinterpret_cast<uint32_t*>(d + o_pts), c.msg = d + o_msg;
    KCHK(hipMemcpyAsync(d, h, o_out, hipMemcpyHostToDevice, s));
    KCHK(hipEventRecord(ev[0], s));
    bn ? launch_ipk_keygen<BnCurve>(c) : launch_ipk_keygen<FbnCurve>(c);
    KCHK(hipGetLastError());
    KCHK(hipEventRecord(ev[1], s));
    KCHK(hipMemcpyAsync(h + o_out, d + o_out, h_need - o_out, hipMemcpyDeviceToHost, s));
    KCHK(hipStreamSynchronize(s));
    host_parallel_for(nch, [&](size_t ch) {
      for (size_t j = ch * CH; j < std::min(m, (ch + 1) * CH); j++) {
        const size_t i = base + j;
        const uint8_t* cs = h + o_out + j * 64;
        const uint8_t* W = h + o_t1 + j * 128;  // the first plane of [2][m][128]
        ipkw::write_ipk(bn, h + o_pts + j * IPK_NPT * 64, W, cs, cs + 32, ipk_out + i * ipk_stride);
        ipk_len[i] = (uint32_t)ipkw::IPK_LEN;
        idgen::limbs_to_be32(reinterpret_cast<const uint32_t*>(h) + (j * IPK_ND + IPK_D_ISK) * 8, isk32_out + 32 * i);
      }
    });
    float a = 0.f;
    KCHK(hipEventElapsedTime(&a, ev[0], ev[1]));
    ms += a;
  }
  g_last_ms[1].store(ms);
  return FTS_API_OK;
}

int fts_idemix_issuer_key_last_timings(float* ms2) {
  if (!ms2) return FTS_API_EINVAL;
  ms2[0] = g_last_ms[0].load(), ms2[1] = g_last_ms[1].load();
  return FTS_API_OK;
}

// ---------------------------------------------------------------------------
// Host-only entries (tests)
// ---------------------------------------------------------------------------
int fts_debug_idemix_keygen_draws(int curve_id, uint64_t seed, uint64_t i, uint8_t* out10x32) {
  if (!out10x32 || seed == FTS_SEED_OS_RANDOM || !curve_ok(curve_id)) return FTS_API_EINVAL;
  uint32_t dr[10][8];
  host::Rng rng(seed + i);
  ipkw::keygen_draws(curve_id == FTS_CURVE_BN254, rng, dr, 10);
  for (int k = 0; k < 10; k++) idgen::limbs_to_be32(dr[k], out10x32 + 32 * k);
  wipe_bytes(dr, sizeof dr);
  return FTS_API_OK;
}

int fts_debug_idemix_ipk_parse(int curve_id, const uint8_t* ipk, size_t ipk_len, int32_t* status, uint8_t* hash32) {
  if (!status || !hash32 || !curve_ok(curve_id)) return FTS_API_EINVAL;
  ipkw::CheckFields f;
  const bool bn = curve_id == FTS_CURVE_BN254;
  *status = ipkw::parse_for_check(ipk, ipk_len, bn, f);
  (void)ipkw::hash_without_field10(ipk, ipk ? ipk_len : 0, bn, hash32);
  return FTS_API_OK;
}

}  // extern "C"
