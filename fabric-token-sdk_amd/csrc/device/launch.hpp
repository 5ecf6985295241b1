// Everything one translation unit defines and another uses: the kernel
// launchers, their size functions and the process-wide launch knobs.  Included
// by the unit that defines a name and by every unit that uses it, so a changed
// parameter, default argument or variable type fails to compile instead of
// surfacing at link time (or never).  The structures are only named here (but
// idv::Chain, at the end); a unit includes the header that defines the ones it touches.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <atomic>

namespace fts {

struct MsmPlan;
struct PvDev;
struct PvStage;
struct RlcDev;
struct RpBatchDev;
struct RpGather;
struct SigBatchDev;
struct SpDev;
struct Timeline;

// ---- the host API (api_ctx.cpp)
// "fb:" + nm, interned (Timeline marks after fallback())
const char* fallback_name(const char* nm);

// thread-per-item launch: ceil(nthreads / bs) blocks of bs threads, nothing for zero items
#define FTS_LAUNCH(kern, nthreads, bs, stream, ...)                                   \
  do {                                                                                \
    size_t nt_ = (size_t)(nthreads);                                                  \
    if (nt_) hipLaunchKernelGGL(kern, dim3((unsigned)((nt_ + (bs)-1) / (bs))), dim3(bs), 0, stream, __VA_ARGS__); \
  } while (0)

// ---- rp_pass.cpp
extern int g_lat_bs;                // block size of the latency-bound per-proof kernels
extern std::atomic<int> g_work_bs;  // FTS_WORK_BS: written by context creation while other lanes launch
void launch_rp_batch(const RpBatchDev& d, const RlcDev& r, const uint32_t* tables, const uint32_t* wtables,
                     const uint8_t* x0_const, const uint8_t* x0_tmpl, hipStream_t s, hipStream_t s2, hipStream_t s3,
                     hipStream_t s4, Timeline* tl, int wbits);
void launch_rp_gather(const RpGather& g, int k, uint8_t* raw, uint32_t* sc, int32_t* status, int32_t* ipa,
                      hipStream_t s);
// wave priority table (wave_prio.hpp PrioSlot) of every unit whose kernels call wave_prio<>()
hipError_t set_wave_prio(const int* p);

// ---- rp_tables.hip
size_t fb_words_per_base();
size_t fbw_words_per_base(int wbits);
size_t table_build_scratch_bytes(int nb);
size_t wide_build_scratch_bytes(int nb, int wbits);
void launch_build_tables(const uint32_t* bases, int nb, uint32_t* tables, uint32_t* scratch, hipStream_t s);
void launch_build_wide_tables(const uint32_t* bases, int nb, uint32_t* tables, uint32_t* scratch, hipStream_t s,
                              int wbits);
void launch_msm_gen_points(int N, const uint8_t* raw_k, const uint8_t* raw_s, const uint32_t* table, uint32_t* jac,
                           uint32_t* pts, uint32_t* sc, hipStream_t s);

// ---- rp_x0.hip
void launch_normalize(size_t total, int per, int stride, int first, const int32_t* status, const uint32_t* jac,
                      uint32_t* aff, uint8_t* be, hipStream_t s, uint8_t* x0msgs = nullptr);
void launch_normalize_all(int total, const uint32_t* jac, uint32_t* aff, hipStream_t s);
void launch_x0(int B, int n, int k, const int32_t* status, const uint8_t* hp_be, const uint8_t* x0_const,
               const uint8_t* x0_tmpl, const uint32_t* sc, uint8_t* msgs, uint32_t* ch, hipStream_t s);

// ---- rp_rlc.hip
// column Q of the ungrouped combination (after x0): partial sums, their sum, its product -> r.fixed
void launch_rlc_q_column(const RpBatchDev& d, const RlcDev& r, const uint32_t* tables, hipStream_t s, Timeline* tl);
void launch_rlc_group_test(const RpBatchDev& d, const RlcDev& r, const uint32_t* tables, const MsmPlan& p,
                           const int32_t* sel, int G, int gs, uint32_t* gcol, uint32_t* gfix, int32_t* next,
                           uint32_t* next_count, hipStream_t s, Timeline* tl);
void launch_rlc_locate(const RpBatchDev& d, const RlcDev& r, const uint32_t* tables, uint32_t* save, int32_t* loc,
                       hipStream_t s, Timeline* tl);
void launch_rlc_accept_except(int B, int skip, int32_t* status, const int32_t* ipa_flag, hipStream_t s);

// ---- rp_fallback.hip
size_t rp_scratch_words(int B, int n, int k);
size_t rp_terms_words(int B, int n, int k);
void launch_rp_fallback(const RpBatchDev& d, const uint32_t* tables, const int32_t* sel, int nsel, hipStream_t s,
                        Timeline* tl);

// ---- msm.hip
// ev_stage (optional): recorded on s after the counting sort (stage 1) or the bucket
// accumulation (stage 2)
void launch_msm(const MsmPlan& p, const uint32_t* points, const uint32_t* scalars, const uint32_t* extra, int nextra,
                uint32_t* scratch, hipStream_t s, hipStream_t s_extra, Timeline* tl, hipEvent_t ev_stage = nullptr,
                int stage = 0);
void launch_msm_small(const MsmPlan& p, const uint32_t* points, const uint32_t* scalars, const uint32_t* extra,
                      int nextra, hipStream_t s, Timeline* tl);
void launch_msm_sort(const MsmPlan& p, const uint32_t* scalars, hipStream_t s, Timeline* tl);
void launch_msm_reduce(const MsmPlan& p, const uint32_t* points, const uint32_t* extra, int nextra, uint32_t* scratch,
                       hipStream_t s, hipStream_t s_extra, Timeline* tl);
void launch_msm_load(int N, const uint8_t* raw_pts, const uint8_t* raw_sc, uint32_t* pts, uint32_t* sc, uint32_t* bad,
                     hipStream_t s);
void launch_msm_to_bytes(const uint32_t* jac, uint8_t* out, hipStream_t s);
void launch_msm_pts_to_bytes(int n, const uint32_t* pts, uint8_t* out, hipStream_t s);

// ---- sigma_kernels.hip
void launch_sig_prep(const SigBatchDev& d, hipStream_t s);
void launch_sig_finish(const SigBatchDev& d, const uint32_t* tables, int n, hipStream_t s);
void launch_sig_exclude(const SigBatchDev& d, int32_t* rp_excl, hipStream_t s);

// ---- prove_kernels.hip
void launch_rp_prove(const PvDev& d, const PvStage* stages, const uint8_t* x0_const, const uint8_t* x0_tmpl,
                     hipStream_t s, Timeline* tl);
void launch_sigma_prove(const SpDev& d, hipStream_t s);

// ---- audit_kernels.hip
void launch_open_check(int n, const uint8_t* raw, const uint32_t* sc, const uint32_t* tables, int nb,
                       int32_t* status, hipStream_t s);
// tokens per lane of k_token_commit (they share one inversion).  1: at 65,536 tokens a lane
// per token is one wave per SIMD, and every further token per lane only takes waves
// off the chip (0.40 ms against 0.70 / 1.32 / 2.49 / 4.85 ms for 2 / 4 / 8 / 16; at 2^20 tokens
// 2 and 4 gain 4 %); the launcher takes 2 / 4 / 8 / 16 for that A/B
constexpr int TOKEN_COMMIT_PER_LANE = 1;
// sc: [n][24] staged scalars; zs, pre: [n][8] scratch; out: [n][64] (16-byte aligned)
void launch_token_commit(int n, int per_lane, const uint32_t* sc, const uint32_t* tables, int nb, uint32_t* zs,
                         uint32_t* pre, uint8_t* out, hipStream_t s);

// ---- idemix_kernels.hip (nym signatures; the FP256BN fixed-base tables also serve the identity proofs)
void fbn_build_tables(const uint32_t* plain, int nb, uint32_t* mont, int32_t* ok, uint32_t* tables, hipStream_t s);
size_t fbn_words_per_base();
// one tile of k_nym_verify (bn; msgw = the messages) or k_nym_verify<FbnCurve> (msgw = the hashed streams, ipk_hash unused)
void launch_nym_verify(bool bn, int n, const uint32_t* rec, const uint8_t* nym, const uint32_t* msgw,
                       const uint64_t* moff, const uint32_t* mlen, const uint32_t* tables, const uint32_t* ipk_hash,
                       uint32_t* vtab, int32_t* status, int base, int tile, hipStream_t s);
// k_nym_sign<BnCurve> (bn) or k_nym_sign<FbnCurve> over all n items: srec idv::NSREC words per item, out idv::NSOUT
void launch_nym_sign(bool bn, int n, const uint32_t* srec, const uint8_t* nym, const uint32_t* msgw,
                     const uint64_t* moff, const uint32_t* mlen, const uint32_t* tables, const uint32_t* ipk_hash,
                     int32_t* status, uint32_t* out, hipStream_t s);

}  // namespace fts

// ---- idemix_identity_<cv>.hip, idemix_pairing_<cv>.hip, idemix_bp_<cv>.hip, cv = bn | fbn (device/idv_kernels.hpp)
struct fts_idemix_idv;
namespace idv {
struct BnCurve;
struct FbnCurve;
constexpr int MSG_MAX = 832;  // transcript bytes per identity: 13 SHA-256 blocks (FP256BN: 19 + 11 * 65 + 36 = 770)
constexpr int BP_G = 256;     // identities per group of the batch pairing check
struct Key8 {
  uint32_t k[8];
};
// one call's buffers (the only structure defined here: the host fills it and must not see the kernels)
struct Chain {
  hipStream_t s;
  int n;
  const uint32_t* rec;
  const uint8_t *pts, *epk;
  uint32_t *scr, *pin;
  int32_t *zk, *st;
  const int32_t *eidx, *g2ok;  // BN254 epoch keys (FP256BN: null)
  const uint32_t *tables, *hash, *lines;
  uint8_t* msg;
  int32_t *gok, *cnt, *list;
  Key8 key;
};
// per curve, instantiated in that curve's units
template <class CV>
void launch_tvals(const Chain& c);
template <class CV>
void launch_batch(const Chain& c);
template <class CV>
void launch_pairing(const Chain& c, unsigned lanes, bool list);
template <class CV>
void launch_lines(const uint8_t* w, uint32_t* lines, int32_t* ok, hipStream_t s);
// debug pairing; p16: affine P as 16 words, BN254 Montgomery / FP256BN canonical limbs < p
template <class CV>
void launch_pairing_debug(const uint32_t* lines, int which, const uint32_t* p16, uint32_t* out, int final_exp,
                          hipStream_t s);
// BN254 only
void launch_g2_check(int M, const int32_t* idx, const uint8_t* keys, int32_t* ok, hipStream_t s);
// sizes (words): pairing lines per G2 point, the t-value kernels' scratch, the batch check's layout in it
size_t line_words(bool bn);
size_t idv_scratch_words(size_t n);
size_t bp_part_off(size_t n);
size_t bp_gok_off(size_t n, size_t ng);
size_t bp_cnt_off(size_t n, size_t ng);
size_t bp_list_off(size_t n, size_t ng);
size_t bp_scratch_words(size_t n);

// ---- idemix_audit.hip (device/idv_audit.hpp): k_idv_audit of either curve, 2n lanes
// (pts, rnd, aoff, alen and half_st are [2][n], half-major; pre and rh_pre [n])
void launch_idv_audit(bool bn, int n, const uint8_t* pts, const uint32_t* rnd, const uint32_t* attrw,
                      const uint64_t* aoff, const uint32_t* alen, const int32_t* pre, const int32_t* rh_pre,
                      const uint32_t* tables, int32_t* half_st, hipStream_t s);

// ---- idemix_idgen_<cv>.hip (device/idgen_kernels.hpp): identity generation
// per identity: draws staged (IDG_ND x 8 words), scalar slots of k_idg_prep, output points
// (Jacobian), words written back; per credential: secrets (sk E S attrs), constant points + mask
constexpr int IDG_ND = 18, IDG_NPROD = 19, IDG_NSC = IDG_NPROD + 2, IDG_NPT = 11, IDG_OUT_WORDS = 6 * 16 + 13 * 8;
constexpr int IDG_SEC_WORDS = 7 * 8, IDG_CPT_WORDS = 3 * 16 + 1;
struct GenChain {
  hipStream_t s;
  hipEvent_t ev_mid;  // recorded between k_idg_points and k_idg_finish
  int n;
  const uint32_t *draws, *sec, *cpt;  // [n][IDG_ND][8]; the credential's
  uint32_t *sc, *pts, *pre;           // [IDG_NSC][n][8]; [IDG_NPT][24][n]; [IDG_NPT * 8][n]
  uint8_t* msg;                       // [MSG_MAX][n]
  const uint32_t *itab, *ctab, *hash;  // issuer tables, the tables of A and B, ipk.Hash
  uint32_t* out;                      // [n][IDG_OUT_WORDS]
  const int32_t* st;
};
// api_idemix.cpp: the verifier handle's device, curve, seven fixed-base tables and ipk.Hash words
struct IdvView {
  int device, curve;
  const uint32_t *tables, *hash;
};
IdvView idv_view(const ::fts_idemix_idv* k);
template <class CV>
void launch_idgen_cred(const uint32_t* tables, const uint32_t* ab, const uint32_t* sec, uint32_t* cpt, int32_t* ok,
                       hipStream_t s);
template <class CV>
hipError_t launch_idgen(const GenChain& c);

// ---- idemix_cred_<cv>.hip (device/cred_kernels.hpp): credential verification up to the
// pairing stage's inputs (launch_batch / launch_pairing above then run on pin, zk and st)
// per credential: E S sk attrs[0..3] as canonical limbs; A then B, X || Y raw
constexpr int CRV_NPROD = 7, CRV_REC_WORDS = CRV_NPROD * 8, CRV_PTS_BYTES = 2 * 64;
struct CredChain {
  hipStream_t s;
  int n;
  const uint32_t* rec;  // [n][CRV_REC_WORDS]
  const uint8_t* pts;   // [n][CRV_PTS_BYTES]
  uint32_t *scr, *pin;  // cred_scratch_words(n); [n][32]
  int32_t *zk, *st;
  const uint32_t* tables;  // the issuer's seven
};
template <class CV>
void launch_cred_prep(const CredChain& c);
size_t cred_scratch_words(size_t n);

// ---- idemix_credissue_<cv>.hip (device/credissue_kernels.hpp): credential requests made and
// checked, credentials issued
// per request checked (CI_REC_WORDS, canonical limbs): proof_c as sent (compared), proof_c and
// proof_s mod r, the nonce as big-endian words, then for an issue S, attrs[0..3], E
constexpr int CI_R_CCMP = 0, CI_R_CMUL = 8, CI_R_S = 16, CI_R_NONCE = 24, CI_R_BIGS = 32, CI_R_ATTR = 40, CI_R_E = 72;
constexpr int CI_REC_WORDS = 80, CI_NPROD = 7;
// per request made: sk, rSk, the nonce as big-endian words; words written back by
// k_ci_request (Nym c s) and k_ci_sign (A B); transcript bytes per lane (five SHA-256 blocks)
constexpr int CIQ_REC_WORDS = 24, CI_OUT_WORDS = 32, CI_MSG_BYTES = 320;
struct CredReqChain {
  hipStream_t s;
  hipEvent_t ev_mid;    // an issue: recorded between k_ci_check and k_ci_sign
  int n;
  const uint32_t* rec;  // [n][CI_REC_WORDS] (made: [n][CIQ_REC_WORDS])
  const uint8_t* pts;   // [n][64] Nym, X || Y
  uint32_t* scr;        // credissue_scratch_words(n)
  uint8_t* msg;         // [CI_MSG_BYTES][n]
  uint32_t* out;        // [n][CI_OUT_WORDS]
  int32_t* st;
  const uint32_t *tables, *hk, *isk;  // the issuer's seven; ipk.Hash then HSk (X || Y), big-endian words; the secret
};
template <class CV>
void launch_credreq_make(const CredReqChain& c);
template <class CV>
hipError_t launch_credissue(const CredReqChain& c, bool issue);
template <class CV>
void launch_credissue_key(const uint8_t* bar, const uint32_t* isk, int32_t* ok, hipStream_t s);
size_t credissue_scratch_words(size_t n);
// api_idemix.cpp / api_credissue.cpp: the slots of the credential-request calls that run on a
// verifier's handle, and what an issuer handle borrows from it
struct CredReqState;
CredReqState* credreq_state_new();  // nullptr: a stream or an event could not be created
void credreq_state_free(CredReqState* s);
struct IssuerView {
  IdvView v;
  CredReqState* rq;
  const uint8_t* bar;  // BarG1 then BarG2 of the key as X || Y (128 bytes); nullptr: the key carries none
};
IssuerView idv_issuer_view(const ::fts_idemix_idv* k);

// ---- idemix_ipk_<cv>.hip (device/ipk_kernels.hpp): issuer keys checked and generated
// per key checked (IPK_REC_WORDS): ProofC as sent (compared), ProofS mod r, -ProofC mod r
// (canonical limbs), then where the key's HSk, HRand and HAttrs start in the G1 list and how many
constexpr int IPK_R_CCMP = 0, IPK_R_A = 8, IPK_R_B = 16, IPK_R_OFF = 24, IPK_R_CNT = 25, IPK_REC_WORDS = 28;
// per key generated: the draws isk, HSk, HRand, HAttrs[0..3], BarG1, r (canonical limbs); the
// points k_ipk_points writes (the first seven draws' after isk, BarG2, t2); transcript bytes
// per lane (ten SHA-256 blocks)
constexpr int IPK_ND = 9, IPK_D_ISK = 0, IPK_D_BAR = 7, IPK_D_R = 8, IPK_NPT = 9, IPK_MSG_BYTES = 640;
struct IpkChain {
  hipStream_t s;
  int n;
  const uint32_t* rec;  // check: [n][IPK_REC_WORDS]; keygen: [n][IPK_ND][8]
  const uint8_t *g1, *bar, *w;  // check: the G1 list; [n][128] BarG1 BarG2; [n][128] W
  const uint8_t* g2;    // the generator's 128 bytes, proto order
  uint32_t *wdec, *t1, *t2, *out;  // [n][32]; [n][32] (keygen [2][n][32]); [n][16] (keygen [n][IPK_NPT][16]); [n][16]
  uint8_t* msg;         // [IPK_MSG_BYTES][n]
  int32_t* st;
};
template <class CV>
void launch_ipk_check(const IpkChain& c);
template <class CV>
void launch_ipk_keygen(const IpkChain& c);
}  // namespace idv
