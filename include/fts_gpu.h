/*
 * fts_gpu.h — C-ABI of the MI355X batch verifier for zkatdlog ("nogh" v1)
 * token proofs on BN254.
 *
 * This is the drop-in boundary: a Go validator binds these symbols through
 * cgo.  Only plain pointers and sizes cross it; the
 * library owns all device memory, streams and tables per context.
 *
 * Reference interfaces each entry point replaces (paths relative to
 * token/core/zkatdlog/nogh/v1/ in murongshaozong/fabric-token-sdk):
 *   fts_ctx_create            crypto/setup.go:319-372   PublicParams.Deserialize
 *                             + driver/base.go:39-46     DefaultValidator (context build)
 *   fts_rp_verify_batch       crypto/rp/bulletproof.go:184-205,252-333
 *                                                       NewRangeVerifier + (*rangeVerifier).Verify
 *                             crypto/rp/ipa.go:190-262  (*ipaVerifier).Verify (called from it)
 *   fts_transfer_verify_batch crypto/transfer/transfer.go:49-60,153-197
 *                                                       transfer.NewVerifier + (*Verifier).Verify
 *                             (validator/validator_transfer.go:96-110 TransferZKProofValidate)
 *   fts_issue_verify_batch    crypto/issue/verifier.go:24-57 issue.NewVerifier + Verify
 *                             (validator/validator_issue.go:28-32 IssueValidate)
 *   fts_status_str            the reference's error strings (bulletproof.go:255-323,
 *                             ipa.go:193-258, rangecorrectness.go:139-159,
 *                             typeandsum.go:232-274, sametype.go:180, transfer.go:192-196)
 *   fts_*_prove               crypto/rp/bulletproof.go:209-249, transfer/transfer.go:69-150,
 *                             issue/prover.go:46-112 (host prover: synthetic inputs)
 *
 * Return values: every function returns FTS_API_OK (0) or a negative
 * FTS_API_* code for API/driver errors (bad argument, HIP failure).
 * Per-item verdicts go to caller-owned int32 arrays as fts_status values.
 * Thread safety: every verify entry point may be called concurrently.  Calls queue
 * at one dispatcher per context; a free lane (FTS_LANES, default 4: its own HIP
 * streams and workspace) takes the queue's head calls as ONE device pass -- the
 * range proofs of staged batches, transfer, issue, mixed and request calls are
 * verified together (up to FTS_COALESCE_MAX proofs), each call's sigma proofs beside
 * them -- and every call gets exactly the verdicts it would get alone.
 */
#ifndef FTS_GPU_H
#define FTS_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-item verdicts (1:1 with the reference's distinct error strings) ---- */
enum fts_status {
  FTS_OK = 0,
  FTS_E_MALFORMED = 1,      /* deserialization error, or input on which the reference panics */
  FTS_E_RP_NIL = 2,         /* "invalid range proof: nil elements"   bulletproof.go:255-264 */
  FTS_E_RP_INVALID = 3,     /* "invalid range proof"                 bulletproof.go:323 */
  FTS_E_IPA_NIL = 4,        /* "invalid IPA proof: nil elements"     ipa.go:193,227 */
  FTS_E_IPA_LEN = 5,        /* "invalid IPA proof"                   ipa.go:197 */
  FTS_E_IPA_INVALID = 6,    /* "invalid IPA"                         ipa.go:258 */
  FTS_E_RC_COUNT = 7,       /* "invalid range proof" (#proofs != #commitments) rangecorrectness.go:139 */
  FTS_E_TAS_INVALID = 8,    /* "invalid sum and type proof"          typeandsum.go:232,274 */
  FTS_E_ST_INVALID = 9,     /* "invalid same type proof"             sametype.go:180 */
  FTS_E_NOT_RUN = 10,       /* item not evaluated (batch aborted by an API error) */
  FTS_E_ACTION_INVALID = 11, /* action fails its structural Validate() before the ZK proof:
                               issue/action.go:161-185,273-282; transfer/action.go:244-283 */
  FTS_E_OPEN_MISMATCH = 12, /* "output at index [%d] does not match the provided opening"
                               audit/auditor.go:236-238; "... output does not match provided
                               opening" token/token.go:78-80 */
  FTS_E_SIG_MALFORMED = 13, /* asn1.Unmarshal of the ECDSA signature failed   validator/ecdsa/ecdsa.go:84-87 */
  FTS_E_SIG_NOT_LOW_S = 14, /* "signature is not in lowS"                     validator/ecdsa/ecdsa.go:103-105 */
  FTS_E_SIG_INVALID = 15,   /* "signature not valid" (ecdsa.Verify false)     validator/ecdsa/ecdsa.go:107-110 */
  FTS_E_NYM_MALFORMED = 16, /* idemix nym signature empty / proto.Unmarshal failed (bccsp NymSigner.Verify) */
  FTS_E_NYM_BADKEY = 17,    /* nym public key import failed (idemix/crypto/deserializer.go:49-56) */
  FTS_E_NYM_INVALID = 18,   /* "pseudonym signature invalid: zero-knowledge proof is invalid"
                               (NymSignature.Ver, via idemix/crypto/id.go:151-161) */
  /* idemix identity validity (crypto/id.go:74-108 -> IBM/idemix Signature.Ver), in the order checked: */
  FTS_E_ID_MALFORMED = 19,  /* empty identity, SerializedIdemixIdentity / Signature proto or a point
                               encoding does not parse (crypto/deserializer.go:37-47) */
  FTS_E_ID_BADNYM = 20,     /* nym public key import failed (crypto/deserializer.go:49-56) */
  FTS_E_ID_NO_EIDNYM = 21,  /* "no EidNym provided but ExpectEidNym required" */
  FTS_E_ID_NO_RHNYM = 22,   /* "no RhNym provided but ExpectEidNymRhNym required" */
  FTS_E_ID_REVOCATION = 23, /* revocation algorithm other than ALG_NO_REVOCATION */
  FTS_E_ID_APRIME = 24,     /* "signature invalid: APrime = 1" */
  FTS_E_ID_PAIRING = 25,    /* "signature invalid: APrime and ABar don't have the expected structure" */
  FTS_E_ID_ZK = 26,         /* "signature invalid: zero-knowledge proof is invalid" */
  /* idemix audit info against an owner identity (services/identity/idemix/crypto/audit.go:40-84
     AuditInfo.Match -> IBM/idemix AuditNymEid / AuditNymRh), in the order checked: */
  FTS_E_AUDIT_MALFORMED = 27,    /* SerializedIdemixIdentity or its Signature proto does not unmarshal,
                                    empty proof, or a nil rand */
  FTS_E_AUDIT_NO_EIDNYM = 28,    /* "no EidNym provided" */
  FTS_E_AUDIT_EID_POINT = 29,    /* EidNym does not decode (G1FromProto) */
  FTS_E_AUDIT_EID_MISMATCH = 30, /* "eid nym does not match" */
  FTS_E_AUDIT_NO_RHNYM = 31,     /* "no RhNym provided" */
  FTS_E_AUDIT_RH_POINT = 32,     /* RhNym does not decode */
  FTS_E_AUDIT_RH_MISMATCH = 33,  /* "rh nym does not match" */
  /* signing (fts_ecdsa_sign_batch, fts_nym_sign_batch): no reference string, a signer holding
   * such a key cannot exist there */
  FTS_E_SIGN_BADKEY = 34,        /* private scalar out of range: ECDSA d = 0 or d >= n; nym sk or rnym >= r */
  /* idemix credential validity (services/identity/idemix/km.go:117-133 -> IBM/idemix Credential.Ver),
   * in the order checked.  35 stays unassigned: fts_status_str(35) is "unknown status", which callers
   * have been able to rely on as the first code past the table */
  FTS_E_CRED_MALFORMED = 36,     /* NULL or empty input, Credential proto does not parse, attributes other
                                    than four, a scalar >= r, A or B off the curve or the identity */
  FTS_E_CRED_B = 37,             /* "b-value from credential does not match the attribute values" */
  FTS_E_CRED_PAIRING = 38,       /* "credential is not cryptographically valid" */
  /* idemix credential requests (IBM/idemix CredRequest.Check), in the order checked.  39 stays
   * unassigned, as 35 does: fts_status_str(39) has been "unknown status", the first code past the table */
  FTS_E_CREDREQ_MALFORMED = 40,  /* "one of the proof values is undefined": NULL or empty input, the proto
                                    does not parse, a missing field, a scalar or nonce not of 32 bytes,
                                    a Nym that does not decode or is the identity */
  FTS_E_CREDREQ_INVALID = 41,    /* "zero knowledge proof is invalid": the challenge differs */
  /* idemix issuer public keys (IBM/idemix IssuerPublicKey.Check; fts_idemix_ipk_check_batch).  The
   * wording of the three messages is restated from the published idemix code.  42 stays
   * unassigned, as 35 and 39 do: fts_status_str(42) has been "unknown status" */
  FTS_E_IPK_MALFORMED = 43,      /* NULL or empty input, the proto does not parse, a point that does not
                                    decode on the curve (W: on the twist), ProofC or ProofS not of 32 bytes */
  FTS_E_IPK_UNDEFINED = 44,      /* "some part of the public key is undefined": HSk, HRand, W, BarG1, BarG2,
                                    ProofC or ProofS missing, BarG1 the identity, fewer HAttrs than names */
  FTS_E_IPK_PROOF = 45           /* "zero knowledge proof in public key invalid": the challenge differs */
};

/* ---- API return codes ---- */
#define FTS_API_OK 0
#define FTS_API_EINVAL (-1)   /* bad argument / NULL pointer */
#define FTS_API_EPP (-2)      /* public parameters rejected (setup.go:319-372,444-489) */
#define FTS_API_EDEVICE (-3)  /* HIP runtime / device failure */
#define FTS_API_ENOMEM (-4)
#define FTS_API_ESIZE (-5)    /* unsupported bit length / batch shape */

/* device argument of fts_ctx_create*: host-only context (parsing + prover, no GPU) */
#define FTS_DEVICE_NONE (-2)

typedef struct fts_ctx fts_ctx;
typedef struct fts_rp_batch fts_rp_batch;

typedef struct fts_pp_info {
  uint32_t bit_length;      /* RangeProofParams.BitLength (8/16/32/64) */
  uint32_t rounds;          /* RangeProofParams.NumberOfRounds */
  uint32_t curve_id;        /* always 1 (BN254) */
  int32_t device;           /* HIP device ordinal the context runs on */
  uint64_t max_token;
  uint64_t table_bytes;     /* device bytes of fixed-base tables */
  uint32_t wide_bits;       /* window width of the per-proof bases' tables: 22 (11 additions per
                               product, 1.5 GiB per base) or 20 (12, 436 MiB); fts_ctx_opts */
  uint32_t lanes;           /* concurrent device passes (execution lanes) */
} fts_pp_info;

/* Context options (fts_ctx_create_opts); zero-initialise, then set what you need. */
typedef struct fts_ctx_opts {
  uint32_t bit_length;      /* 0: the PP's own (else as fts_ctx_create_bits) */
  int32_t wide_bits;        /* 20 or 22: force the per-proof bases' window width; 0: by budget */
  uint64_t table_budget;    /* with wide_bits 0: the most device bytes this context's fixed-base
                               tables may take -- 22-bit tables only when all of them fit (at
                               n = 64: 104 GiB; 20-bit: 33 GiB).  0: 22-bit only when the free
                               HBM at creation exceeds them + 8 GiB per lane + 128 GiB (the first
                               context on an empty MI355X), falling back to 20-bit if the
                               allocation fails.  FTS_WIDE_BITS overrides the budget. */
  int32_t lanes;            /* 0: FTS_LANES or 4 */
  int32_t reserved;
} fts_ctx_opts;

/* One transfer action: commitments as 64-byte X||Y big-endian (G1.Bytes()). */
typedef struct fts_transfer_item {
  const uint8_t* inputs;    /* n_in  * 64 bytes */
  size_t n_in;
  const uint8_t* outputs;   /* n_out * 64 bytes */
  size_t n_out;
  const uint8_t* proof;     /* transfer.Proof DER (transfer.go:29-40) */
  size_t proof_len;
} fts_transfer_item;

/* One issue action. */
typedef struct fts_issue_item {
  const uint8_t* tokens;    /* n_tok * 64 bytes */
  size_t n_tok;
  const uint8_t* proof;     /* issue.Proof DER (issue/prover.go:27-37) */
  size_t proof_len;
} fts_issue_item;

/* ---- context ---- */
/* pp: PublicParams.Serialize() bytes (JSON container {"identifier","raw"}).
 * device: HIP device ordinal (-1: current device, FTS_DEVICE_NONE: host-only). */
int fts_ctx_create(const uint8_t* pp, size_t pp_len, int device, fts_ctx** out);
/* Same generators, range proofs truncated to bit_length (Setup(bit_length) semantics,
 * setup.go:388-406: labels do not depend on the bit length). */
int fts_ctx_create_bits(const uint8_t* pp, size_t pp_len, uint32_t bit_length, int device, fts_ctx** out);
/* Same, with explicit options (table budget, window width, lanes); opts may be NULL. */
int fts_ctx_create_opts(const uint8_t* pp, size_t pp_len, int device, const fts_ctx_opts* opts, fts_ctx** out);
/* Multi-device context (SURVEY §8b device_mask; the reference verifies every action
 * independently, core/common/validator.go:215-224): one child context per device (its
 * own lanes and streams; children on one device share its tables, see below).  Every batch entry point below splits the caller's batch
 * into contiguous shards balanced by cost (fts_shard_plan: range proofs per action),
 * runs the shards on their devices concurrently and returns the verdicts in the
 * caller's order; fts_msm_g1 sums the devices' partial MSM points on the host.
 * The device provers, fts_token_commit_batch_gpu and the generators split the same way
 * (proofs and tokens equally, actions by the verify side's weights) and write their
 * results in the caller's order.  Their randomness keeps its GLOBAL index: one source per
 * call, item g of the caller's batch draws from stream g on whichever device it runs, so
 * a seeded call gives the single-device bytes and a secure call never uses one
 * (key, stream) pair for two items.  The whole batch is checked before any device starts;
 * the first error in shard order is returned.
 * Not sharded, first device only: staged MSMs (fts_msm_stage*, fts_msm_run,
 * fts_msm_points: a handle would have to span devices), fts_last_timings* and the debug
 * hooks.  The randomness draws and the DER / protobuf writers run on the one host pool
 * for all devices.  The ECDSA, nym and identity calls take a device ordinal or a
 * per-device handle; their callers shard them.  devices[] may
 * repeat an ordinal (several shards on one device).  bit_length 0: the PP's own. */
int fts_ctx_create_devices(const uint8_t* pp, size_t pp_len, uint32_t bit_length, const int32_t* devices, int ndev,
                           fts_ctx** out);
/* bit d of device_mask = HIP device d */
int fts_ctx_create_mask(const uint8_t* pp, size_t pp_len, uint32_t bit_length, uint64_t device_mask, fts_ctx** out);
/* devices of the context (up to cap written); returns their number (0: host-only) */
int fts_ctx_devices(const fts_ctx* ctx, int32_t* devices, int cap);
/* contiguous split of n items into nshards shards of (near) equal total weight
 * (weights NULL: equal weights): shard j = [bounds[j], bounds[j+1]), bounds[0] = 0,
 * bounds[nshards] = n.  Host-only; the split every multi-device entry point uses. */
int fts_shard_plan(size_t n, const double* weights, int nshards, size_t* bounds);
void fts_ctx_destroy(fts_ctx* ctx);
int fts_ctx_info(const fts_ctx* ctx, fts_pp_info* out);

/* ---- shared fixed-base tables ----
 * The tables are a function of the generator bytes alone, so the contexts of one
 * process that have the same bases on the same device read ONE device buffer: a
 * process-wide, per-device, reference-counted cache hands it out.  Two kinds of entry:
 *   narrow  the 16-bit tables of all 2n+6 bases; key = (device, SHA-256 of the bases)
 *   wide    the 20/22-bit tables of [H_0..H_{n-1}, K, P]; key = (device, width,
 *           SHA-256 of those n+2 bases) -- the Pedersen generators are not part of it,
 *           so public parameters that differ only in them share the wide set
 * Different bit lengths share nothing (K and the layout depend on n).  Contexts created
 * concurrently with the same key build it once; the others wait.  Each context holds a
 * counted reference; the last one destroyed frees the buffer, and the cache keeps
 * nothing alive by itself.  A built table is never written again.
 * Width: with no explicit width (fts_ctx_opts.wide_bits, FTS_WIDE_BITS) and no
 * table_budget, a context takes 22-bit tables without looking at the free HBM when a
 * live context on the device already has (or is building) its wide set at 22 bits.
 * fts_pp_info.table_bytes stays the size of the tables the context READS (summed over
 * the shards of a multi-device context), shared or not; table_budget compares against
 * the same figure.
 * FTS_TABLE_SHARE=0 (read at context creation): the context builds private tables. */
typedef struct fts_table_info {
  uint64_t narrow_id, wide_id;       /* opaque; equal ids on one device = the same device memory */
  uint64_t narrow_bytes, wide_bytes;
  uint32_t narrow_refs, wide_refs;   /* contexts holding the entry now */
  uint32_t narrow_built, wide_built; /* 1: this context's creation built it; 0: found in the cache */
} fts_table_info;
/* shard: index into the context's devices (0 for a single-device context).  A private
 * context (FTS_TABLE_SHARE=0) reports refs 1, built 1 and ids of its own.
 * FTS_API_EINVAL for a host-only context or a shard out of range. */
int fts_ctx_table_info(const fts_ctx* ctx, int shard, fts_table_info* out);

/* The cache's books for one device.  Private contexts' tables are not in them.
 * (The struct shares its name with the call, like stat: write `struct
 * fts_table_cache_stats`.) */
struct fts_table_cache_stats {
  uint64_t resident_bytes;           /* bytes of all live entries on the device */
  uint32_t entries;
  uint64_t builds, hits;             /* since process start */
};
int fts_table_cache_stats(int device, struct fts_table_cache_stats* out);

/* ---- verification (host buffers in, verdicts out) ---- */
/* n standalone range proofs: rp_der[i] = RangeProof.Serialize() (bulletproof.go:93-95),
 * com64 = n * 64-byte commitments V_i.  status[i] <- fts_status. */
int fts_rp_verify_batch(fts_ctx* ctx, size_t n, const uint8_t* const* rp_der, const size_t* rp_len,
                        const uint8_t* com64, int32_t* status);
/* status[i] <- fts_status; fail_index[i] <- index of the failing range proof (-1 if none). */
int fts_transfer_verify_batch(fts_ctx* ctx, size_t n, const fts_transfer_item* items, int32_t* status,
                              int32_t* fail_index);
int fts_issue_verify_batch(fts_ctx* ctx, size_t n, const fts_issue_item* items, int32_t* status,
                           int32_t* fail_index);

/* Transfers and issues of many token requests in ONE device pass (BASELINE config C5):
 * verdicts identical to fts_transfer_verify_batch / fts_issue_verify_batch on the same
 * items.  fail_tr / fail_is may be NULL. */
int fts_actions_verify_batch(fts_ctx* ctx, size_t n_tr, const fts_transfer_item* transfers, size_t n_is,
                             const fts_issue_item* issues, int32_t* status_tr, int32_t* fail_tr, int32_t* status_is,
                             int32_t* fail_is);

/* ---- raw TokenRequest ingest (replaces the deserialisation + ZK half of
 * Validator.VerifyTokenRequestFromRaw, core/common/validator.go:78-130) ----
 * req[i] = TokenRequest.Bytes() (driver/request.go:38-53, protos request.proto:95-100).
 * Every request is decoded on the host (TokenRequest.FromBytes, DeserializeActions:
 * validator/validator.go:27-47, the actions' Deserialize + Validate), then the ZK proofs
 * of ALL actions of ALL n requests are verified in ONE device pass.
 *   status[i]      <- FTS_OK, or the verdict of the request's first failing action in
 *                     the reference's order (every issue, then every transfer), or
 *                     FTS_E_MALFORMED when the request / an action does not deserialise
 *   fail_action[i] <- index in TokenRequest.actions of that action (-1: request level
 *                     or OK)
 *   fail_index[i]  <- index of the failing range proof inside that action (-1 if none)
 * Not evaluated here (stay with the caller's Go code): signatures, auditor signature,
 * issuer allow-list, upgrade-witness commitment, HTLC scripts, ledger lookups.
 * fail_action / fail_index may be NULL. */
int fts_request_verify_batch(fts_ctx* ctx, size_t n, const uint8_t* const* req, const size_t* req_len,
                             int32_t* status, int32_t* fail_action, int32_t* fail_index);
/* Host-only decode of one request (no device, ctx not needed): the deserialisation verdict
 * (status, fail_action as above), the action counts, and the first action (reference order)
 * whose structural check fails before its proof (pre_status FTS_E_ACTION_INVALID /
 * FTS_E_MALFORMED, pre_action its index; FTS_OK / -1 if none). */
int fts_request_inspect(const uint8_t* req, size_t req_len, int32_t* status, int32_t* fail_action,
                        int32_t* n_issue, int32_t* n_transfer, int32_t* pre_status, int32_t* pre_action);

/* ---- device-resident batches (parse + upload once, verify many times) ---- */
int fts_rp_batch_stage(fts_ctx* ctx, size_t n, const uint8_t* const* rp_der, const size_t* rp_len,
                       const uint8_t* com64, fts_rp_batch** out);
/* runs the whole GPU verification of a staged batch; status may be NULL.
 * Thread-safe: concurrent calls on DIFFERENT batches run on different lanes
 * (stream pairs, FTS_LANES env, default 4) and overlap on the device; batches
 * submitted while every lane is busy are coalesced into one device pass of
 * up to FTS_COALESCE_MAX proofs (default 81920).  Verdicts are per proof and
 * independent of the grouping. */
int fts_rp_batch_verify(fts_ctx* ctx, fts_rp_batch* b, int32_t* status);
/* pre-allocate every lane's workspace for device passes of up to max_pass_proofs
 * range proofs (0: FTS_COALESCE_MAX) so that no allocation -- and no device-wide
 * synchronisation -- happens once batches flow; call once after fts_ctx_create */
int fts_ctx_reserve(fts_ctx* ctx, size_t max_pass_proofs);
/* number of staged batches (including b) in the device pass that verified b last */
int fts_rp_batch_merged(const fts_rp_batch* b);
/* Test hook: no device pass starts until n calls (staged batches and action calls of any
 * entry point) are queued, then the queue forms passes as usual (one-shot; n = 0 releases).
 * Makes "these calls share one pass" deterministic in tests. */
int fts_debug_hold(fts_ctx* ctx, int n);
/* Host cost of an action call's staging (DER parse into the device layout, no device;
 * ctx must be host-only: FTS_DEVICE_NONE): ms_avg[0..3] <- mean wall ms over reps of the
 * whole staging and of its three steps (shapes, layout, decode). */
int fts_debug_stage_actions(fts_ctx* ctx, size_t n_tr, const fts_transfer_item* transfers, size_t n_is,
                            const fts_issue_item* issues, int reps, float* ms_avg);
/* dispatcher counters since context creation: out[0] device passes, out[1] calls served,
 * out[2] most calls in one pass, out[3] action calls (transfer / issue / actions / request) */
int fts_debug_dispatch_stats(const fts_ctx* ctx, int64_t* out);
/* range-proof pass counters since context creation, summed over the devices of a
 * multi-device context: out[0] passes finished, out[1] passes whose batch check's
 * combination did not close (a fallback decided them), out[2] single-fault locator
 * hits, out[3] proofs handed to the per-proof final equations.  An honest pass adds
 * (1, 0, 0, 0): a fallback gives the right verdicts whatever the main path computed,
 * so only out[1] shows that the main path is sound. */
int fts_debug_pass_stats(const fts_ctx* ctx, int64_t out[4]);
/* prover-side work of ONE child of a multi-device context since context creation (shard:
 * index into the context's devices; a single-device context is shard 0 of itself):
 * out[0] range proofs proved on it, out[1] sigma proofs (actions), out[2] tokens
 * committed, out[3] prover or commit passes started.  Shows that a call ran on every
 * device, which equal output bytes cannot.  FTS_API_EINVAL for a host-only context or a
 * shard out of range. */
int fts_debug_shard_work(const fts_ctx* ctx, int shard, int64_t out[4]);
/* fts_last_timings of ONE child (fts_last_timings itself reads the first): the kernel
 * classes and the host phases (host_prep: randomness staged, host_wait_flag: device,
 * host_parse: DER) of the pass that finished last on it; returns the count filled, 0 for a
 * shard out of range.  tools/prove_multi_bench.py reads the host share per device here. */
int fts_debug_shard_timings(const fts_ctx* ctx, int shard, const char** names, float* ms, int cap);
/* per-kernel device time (ms) and algorithmic u32 MADs of b's last verification */
int fts_rp_batch_timings(const fts_rp_batch* b, const char** names, float* ms, double* mads, int cap);
void fts_rp_batch_free(fts_rp_batch* b);
/* device time of the last fts_rp_batch_verify, per kernel class (ms); returns count filled */
int fts_last_timings(const fts_ctx* ctx, const char** names, float* ms, int cap);
/* same, plus the algorithmic u32 MAD count of each launch (DESIGN.md cost model; 0 for
 * kernels without field products, e.g. SHA-256) */
int fts_last_timings_ex(const fts_ctx* ctx, const char** names, float* ms, double* mads, int cap);

/* parity/debug hook: exact intermediates of proof i of the last range-proof run
 * (ch_out: (8+2k) x 32-byte BE Fr [x, x^2, y, y^-1, z, z^2, polEval, x0, x_j..., x_j^-1...],
 *  com_out: 64-byte com, hp_out: n x 64-byte H'_i); any pointer may be NULL */
int fts_debug_rp_intermediates(fts_ctx* ctx, size_t i, uint8_t* ch_out, uint8_t* com_out, uint8_t* hp_out);

/* debug: `count` entries T[w[j]][d[j] - 1] = d 2^(W w) B of one base's fixed-base table as
 * the device holds them, out64: count x 64-byte X||Y BE.  wide = 0: the 16-bit set, bases
 * [G_0.., H_0.., ped1, ped2, P, Q, K, ped0] (2n + 6); wide != 0: the set of
 * fts_pp_info.wide_bits, bases [H_0.., K, P] (n + 2).  1 <= d <= 2^(W-1), w < ceil(255 / W);
 * EINVAL otherwise, and on a host-only context */
int fts_debug_table_entries(fts_ctx* ctx, int wide, int base, size_t count, const uint32_t* w, const uint32_t* d,
                            uint8_t* out64);

/* debug: bucket occupancy of the last RLC MSM: out[0] max bucket count, out[1] its index,
 * out[2] total buckets, out[3] non-empty buckets */
int fts_debug_msm_stats(fts_ctx* ctx, int64_t* out);

/* ---- standalone BN254 G1 multi-scalar multiplication (BASELINE config C3) ----
 * out64 <- sum_i k_i P_i as 64-byte X||Y BE (identity: 64 zero bytes), the value
 * gnark-crypto's G1 MultiExp / mathlib G1.Mul + Add return.
 * points64: n x 64-byte X||Y BE, each checked like NewG1FromBytes (asn1.go:148): flag
 * bits, canonical coordinates, on the curve; 64 zero bytes = identity.  A rejected
 * point makes the call return FTS_API_EINVAL.
 * scalars32: n x 32-byte BE integers, used mod r (G1.Mul semantics).
 * Device Pippenger MSM (GLV split, signed windows, counting-sort buckets; msm.hip). */
typedef struct fts_msm_batch fts_msm_batch;
int fts_msm_g1(fts_ctx* ctx, size_t n, const uint8_t* points64, const uint8_t* scalars32, uint8_t* out64);
/* device-resident variant: upload + validate once, run many times */
int fts_msm_stage(fts_ctx* ctx, size_t n, const uint8_t* points64, const uint8_t* scalars32, fts_msm_batch** out);
int fts_msm_run(fts_ctx* ctx, fts_msm_batch* b, uint8_t* out64);
/* config C3 at scale (points k_i G with uniform k_i): n DISTINCT points
 * P_i = k_i * ped1 (the PP's ped[1], a generator of G1) computed on the device from the
 * context's fixed-base table, k32 / scalars32: n x 32-byte BE integers used mod r.  The
 * result of fts_msm_run is then (sum_i s_i k_i mod r) * ped1 (closed form for tests). */
int fts_msm_stage_multiples(fts_ctx* ctx, size_t n, const uint8_t* k32, const uint8_t* scalars32, fts_msm_batch** out);
/* the staged points [lo, lo + count) of b as 64-byte X||Y BE (identity = 64 zero bytes):
 * the C3 CPU baseline runs its Pippenger over the same distinct points */
int fts_msm_points(fts_ctx* ctx, const fts_msm_batch* b, size_t lo, size_t count, uint8_t* out64);
/* per-kernel device time (ms) and algorithmic u32 MADs of b's last run */
int fts_msm_timings(const fts_msm_batch* b, const char** names, float* ms, double* mads, int cap);
void fts_msm_free(fts_msm_batch* b);

/* ---- token opening checks (auditor / wallet) ----
 * Replaces the per-token commit() + Equals of Auditor.InspectOutput
 * (crypto/audit/auditor.go:226-238, reached from CheckIssueRequests / CheckTransferRequests
 * :178-210) and of Token.ToClear (crypto/token/token.go:69-83):
 *   status[i] <- FTS_OK iff HashToZr(type_i)*ped0 + value_i*ped1 + bf_i*ped2 == com_i
 *                FTS_E_OPEN_MISMATCH otherwise
 * com64:   token.Data as 64 B X||Y BE (G1.Bytes()), checked like NewG1FromBytes (flag bits,
 *          canonical coordinates, on the curve; 64 zero bytes = identity) -> FTS_E_MALFORMED
 * type:    metadata.Type bytes (HashToZr = SHA-256 mod r)
 * value32, bf32: Zr.Bytes() 32 B BE, used mod r (G1.Mul semantics)
 * A NULL com64 / value32 / bf32 -> FTS_E_MALFORMED (the reference returns "invalid output at
 * index [%d]" / "cannot commit a nil element", or panics on a nil Zr in the auditor's commit).
 * One device pass: three fixed-base products per token (audit_kernels.hip). */
typedef struct {
  const uint8_t* com64;
  const uint8_t* type;
  size_t type_len;
  const uint8_t* value32;
  const uint8_t* bf32;
} fts_token_opening;
int fts_token_open_batch(fts_ctx* ctx, size_t n, const fts_token_opening* items, int32_t* status);
/* The same check from the serialized form the auditor receives: meta[i] = driver.Metadata
 * bytes of output i (ASN.1 TypedToken{2, proto TokenMetadata}), decoded as
 * token.Metadata.Deserialize does (crypto/token/token.go:136-158; audit/auditor.go:296-300,
 * :370-374 call it), com64 = n x 64 B token.Data.  A metadata that does not decode, or
 * carries a nil value / blinding factor -> FTS_E_MALFORMED. */
int fts_token_metadata_open_batch(fts_ctx* ctx, size_t n, const uint8_t* com64, const uint8_t* const* meta,
                                  const size_t* meta_len, int32_t* status);
/* Host-only decode of one driver.Metadata (no device): status FTS_OK / FTS_E_MALFORMED, the
 * type as (offset, length) into meta, value / bf mod r as 32 B BE, has bit 0 / bit 1 = value /
 * bf present (non-nil). */
int fts_token_metadata_decode(const uint8_t* meta, size_t meta_len, int32_t* status, size_t* type_off,
                              size_t* type_len, uint8_t* value32, uint8_t* bf32, int32_t* has);

/* ---- error strings ---- */
const char* fts_status_str(int32_t status);

/* ---- host prover (reference prover semantics) ----
 * seed selects the prover randomness of every fts_*_prove* entry point:
 *   FTS_SEED_OS_RANDOM  secure: ChaCha20 keystreams under a fresh 256-bit getrandom() key
 *                       per call, one per proof / action (the role of crypto/rand in
 *                       Curve.NewRandomZr, rp/bulletproof.go:336-466).  Use this for real tokens.
 *   any other value     deterministic, FOR TESTS AND BENCHMARKS ONLY: item i draws from
 *                       xoshiro256**(seed + i).  Two calls whose seed ranges overlap reuse
 *                       nonces across different witnesses, which reveals the committed
 *                       values and blinding factors.
 * i is the item's index in the caller's batch.  A multi-device context keeps it: its
 * shards read the call's one source (one getrandom() key in secure mode) at the global
 * index, never at the index inside the shard. */
#define FTS_SEED_OS_RANDOM UINT64_MAX
/* value < 2^bit_length expected (larger values produce a proof that fails, as in the
 * reference).  bf32: blinding factor (BE, reduced mod r).  seed: deterministic RNG seed.
 * out_der: caller buffer of out_cap bytes; *out_len <- bytes written. com64_out: V. */
int fts_rp_prove(const fts_ctx* ctx, uint64_t value, const uint8_t* bf32, uint64_t seed, uint8_t* out_der,
                 size_t out_cap, size_t* out_len, uint8_t* com64_out);
/* batch helper: n proofs with values[i], blinding factors bfs[i*32], seeds seed+i,
 * written into one buffer (offsets[i], lens[i]); uses `threads` host threads */
int fts_rp_prove_batch(const fts_ctx* ctx, size_t n, const uint64_t* values, const uint8_t* bfs, uint64_t seed,
                       int threads, uint8_t* out, size_t out_cap, size_t* offsets, size_t* lens,
                       uint8_t* com64_out);
/* Batched range-proof prover on the device: rangeProver.Prove
 * (rp/bulletproof.go:209-249, preprocess :336-466, IPA prover ipa.go:158-186,267-322) for n
 * proofs in device passes of up to 16,384 (prove_kernels.hip).  Same arguments and output as
 * fts_rp_prove_batch -- byte-identical proofs for the same seed (proof i uses seed + i; the
 * host draws the randomness, the device computes every group element, transcript and
 * Fiat-Shamir challenge).  Needs a device context.  A multi-device context proves an equal
 * share on every device, proof i still from seed + i (its index in this call), and packs the
 * proofs in the caller's order: the same bytes, offsets and lengths as on one device. */
int fts_rp_prove_batch_gpu(fts_ctx* ctx, size_t n, const uint64_t* values, const uint8_t* bfs, uint64_t seed,
                           uint8_t* out, size_t out_cap, size_t* offsets, size_t* lens, uint8_t* com64_out);
/* Whole transfer / issue proofs on the device: the TypeAndSum
 * (transfer/typeandsum.go:189-227,280-356) or SameType (issue/sametype.go:103-149) sigma
 * proof in one kernel (thread per action), then the range proofs of every output of every
 * action in one fts_rp_prove_batch_gpu-style pass.  Action i is seeded with seed + i and the
 * output is byte-identical to fts_transfer_prove / fts_issue_prove.  Issues ignore n_in /
 * in_values / in_bfs (their tokens are the outputs).  A multi-device context splits the
 * actions as the verify entry points do (by range proofs per action); i stays the action's
 * index in this call, so the output does not depend on the devices.  Every witness is
 * checked before any device starts (FTS_API_EINVAL, no device work). */
typedef struct {
  const uint8_t* type;
  size_t type_len;
  size_t n_in;
  const uint64_t* in_values;
  const uint8_t* in_bfs;  /* n_in x 32 B BE */
  size_t n_out;
  const uint64_t* out_values;
  const uint8_t* out_bfs; /* n_out x 32 B BE */
} fts_action_witness;
int fts_transfer_prove_batch_gpu(fts_ctx* ctx, size_t n, const fts_action_witness* w, uint64_t seed, uint8_t* out,
                                 size_t out_cap, size_t* offsets, size_t* lens);
int fts_issue_prove_batch_gpu(fts_ctx* ctx, size_t n, const fts_action_witness* w, uint64_t seed, uint8_t* out,
                              size_t out_cap, size_t* offsets, size_t* lens);
/* Token commitments (token.go:208-217): tok = H(type)*ped0 + value*ped1 + bf*ped2 */
int fts_token_commit(const fts_ctx* ctx, const uint8_t* type, size_t type_len, uint64_t value,
                     const uint8_t* bf32, uint8_t* com64_out);
/* transfer.NewProver(...).Prove(): n_in inputs / n_out outputs with witnesses */
int fts_transfer_prove(const fts_ctx* ctx, const uint8_t* type, size_t type_len, size_t n_in,
                       const uint64_t* in_values, const uint8_t* in_bfs, size_t n_out, const uint64_t* out_values,
                       const uint8_t* out_bfs, uint64_t seed, uint8_t* out_der, size_t out_cap, size_t* out_len);
/* issue.NewProver(...).Prove() */
int fts_issue_prove(const fts_ctx* ctx, const uint8_t* type, size_t type_len, size_t n_tok, const uint64_t* values,
                    const uint8_t* bfs, uint64_t seed, uint8_t* out_der, size_t out_cap, size_t* out_len);

/* Token commitments for a batch on the device (audit_kernels.hip k_token_commit): replaces the
 * per-token commit() of token.GetTokensWithWitness (crypto/token/token.go:109-133, commit :208-217).
 *   com64_out[i] <- G1.Bytes() of HashToZr(type_i)*ped0 + value_i*ped1 + bf_i*ped2
 * byte-identical to fts_token_commit on the same arguments (bf32: 32 B BE, used mod r; the
 * identity comes out as 64 zero bytes).  Three fixed-base products per token into one
 * accumulator, then the exact affine point.  Needs a device context (FTS_API_EDEVICE
 * otherwise); a multi-device context commits an equal share of the tokens on every device. */
typedef struct {
  const uint8_t* type;
  size_t type_len;
  uint64_t value;
  const uint8_t* bf32;
} fts_commit_item;
int fts_token_commit_batch_gpu(fts_ctx* ctx, size_t n, const fts_commit_item* items, uint8_t* com64_out);
/* tokens per wave of that kernel: 64 lanes x the tokens a lane commits and normalises with
 * one inversion (1 by default: DESIGN.md section 5.3) */
int fts_token_commit_batch_width(void);

/* ---- whole transfer / issue actions (prover side of the TokenRequest) ----
 * Replaces Sender.GenerateZKTransfer (crypto/transfer/sender.go:54-107) and
 * Issuer.GenerateZKIssue (crypto/issue/issuer.go:39-84): draw the output blinding factors,
 * commit the outputs (token.GetTokensWithWitness, token.go:109-133), prove
 * (transfer.go:69-150 / issue/prover.go:46-112), build the action (NewTransfer
 * transfer/action.go:127-153 / NewAction issue/action.go:62-77) and serialize it
 * (Action.Serialize transfer/action.go:290-323 / issue/action.go:192-229: fields in number
 * order, proto3 empty values omitted, no metadata map), and serialize the token.Metadata of
 * every output (token.go:161-180: TypedToken{2, TokenMetadata{type, value, blinding_factor,
 * issuer}}; issues carry the issuer, transfers the empty Identity written for a nil issuer).
 * The checks are those of the reference and of the provers: a transfer whose sums differ,
 * or a value above the range, yields an action whose proof fails; input commitments are not
 * checked against their openings.
 * Randomness: action i's prover draws are those of fts_transfer_prove / fts_issue_prove at
 * seed + i; its output blinding factors come from stream 2^63 + i of the same source
 * (secure: that ChaCha20 nonce under the call's key; seeded: xoshiro256**(seed + 2^63 + i)),
 * drawn uniformly below r in output order.  So commitment = fts_token_commit(type, v_j, bf_j)
 * and proof = fts_transfer_prove(type, in..., out_values, those bfs, seed + i). */
typedef struct {
  const uint8_t* tx_id;  /* token id (token.ID{TxId, Index}) */
  size_t tx_id_len;
  uint64_t index;
  const uint8_t* owner;
  size_t owner_len;
  const uint8_t* com64;  /* token.Data, 64 B X||Y BE */
  uint64_t value;        /* its opening */
  const uint8_t* bf32;
} fts_gen_input;
typedef struct {
  uint64_t value;
  const uint8_t* owner;  /* owner_len == 0: a redeem (no owner field is written) */
  size_t owner_len;
} fts_gen_output;
typedef struct {
  const uint8_t* type;
  size_t type_len;
  const fts_gen_input* inputs;  /* transfers; ignored by issues */
  size_t n_in;
  const fts_gen_output* outputs;
  size_t n_out;
  const uint8_t* issuer;  /* issues; ignored by transfers */
  size_t issuer_len;
} fts_gen_action;
/* Caller buffers.  Outputs are numbered across the call in action order (T = sum of n_out):
 * action i is actions[action_off[i] .. + action_len[i]), output t's metadata
 * meta[meta_off[t] .. + meta_len[t]), its commitment com64[64 t] and blinding factor
 * bf32[32 t] (com64 / bf32: T x 64 / T x 32 bytes).  Every length is computed before
 * anything is written: when actions_cap or meta_cap is too small the call returns
 * FTS_API_ESIZE with the offset and length arrays filled and the buffers untouched. */
typedef struct {
  uint8_t* actions;
  size_t actions_cap;
  size_t* action_off;
  size_t* action_len;
  uint8_t* meta;
  size_t meta_cap;
  size_t* meta_off;
  size_t* meta_len;
  uint8_t* com64;
  uint8_t* bf32;
} fts_gen_result;
/* one action on the host (works on a host-only context, like fts_transfer_prove) */
int fts_transfer_generate(const fts_ctx* ctx, const fts_gen_action* action, uint64_t seed, fts_gen_result* out);
int fts_issue_generate(const fts_ctx* ctx, const fts_gen_action* action, uint64_t seed, fts_gen_result* out);
/* n actions on the device: commitments by k_token_commit, proofs by the passes of
 * fts_transfer_prove_batch_gpu / fts_issue_prove_batch_gpu, serialization on the host pool.
 * Action i equals the host call at seed + i.  Needs a device context (FTS_API_EDEVICE).
 * A multi-device context splits the actions as the action provers do; action i (its index
 * in this call) keeps prover stream i and blinding-factor stream 2^63 + i and its outputs
 * their numbers across the call, every device writes com64 / bf32 at those offsets, and the
 * actions and metadata are packed once: output and FTS_API_ESIZE behaviour are those of one
 * device. */
int fts_transfer_generate_batch_gpu(fts_ctx* ctx, size_t n, const fts_gen_action* actions, uint64_t seed,
                                    fts_gen_result* out);
int fts_issue_generate_batch_gpu(fts_ctx* ctx, size_t n, const fts_gen_action* actions, uint64_t seed,
                                 fts_gen_result* out);

/* ---- ECDSA P-256 owner signatures (x509 identities) ----
 * Replaces, per item, ecdsa.Verifier.Verify(message, sigma)
 * (validator/ecdsa/ecdsa.go:82-113; identical logic in
 * services/identity/x509/crypto/ecdsa.go:46-77), called by
 * TransferSignatureValidate (validator/validator_transfer.go:29-62) once per
 * input owner.  Independent of the zkatdlog public parameters: takes a device
 * ordinal, not an fts_ctx. */
typedef struct {
  const uint8_t* msg;  /* signed message; SHA-256 is computed on the device */
  size_t msg_len;
  const uint8_t* sig;  /* DER ECDSA-Sig-Value SEQUENCE{INTEGER r, INTEGER s} */
  size_t sig_len;
  const uint8_t* pk64; /* public key X||Y, 32 B big-endian each (see fts_p256_pubkey_from_pkix) */
} fts_ecdsa_item;
/* status[i] <- FTS_OK | FTS_E_SIG_MALFORMED | FTS_E_SIG_NOT_LOW_S | FTS_E_SIG_INVALID
 * (an off-curve / non-canonical public key is FTS_E_SIG_INVALID, as in Go's ecdsa.Verify). */
int fts_ecdsa_verify_batch(int device, size_t n, const fts_ecdsa_item* items, int32_t* status);
/* Host-only: the asn1.Unmarshal + IsLowS + range part of Verify; r32/s32 <- 32 B big-endian
 * (valid when *status == FTS_OK). */
int fts_ecdsa_sig_parse(const uint8_t* sig, size_t sig_len, uint8_t* r32, uint8_t* s32, int32_t* status);
/* Host-only: DER SubjectPublicKeyInfo of a P-256 key (x509.MarshalPKIXPublicKey, the body of
 * the PEM "PUBLIC KEY" block of ecdsa.Verifier.Serialize, ecdsa.go:115-150) -> X||Y.
 * FTS_API_EINVAL for anything else. */
int fts_p256_pubkey_from_pkix(const uint8_t* der, size_t len, uint8_t* pk64);
/* HIP-event durations (ms) of the last fts_ecdsa_verify_batch on `device`:
 * ms2[0] = k_ecdsa_digest, ms2[1] = k_ecdsa_verify. */
int fts_ecdsa_last_timings(int device, float* ms2);

/* ---- ECDSA P-256 signing (x509 owners) ----
 * Per item what ecdsa.Signer.Sign(message) returns (validator/ecdsa/ecdsa.go:49-63): the
 * digest is SHA-256 of the message, s is normalised to s <= n/2 (ToLowS) and (r, s) is written
 * as utils.MarshalECDSASignature does (minimal DER).  The nonce is NOT Go's (crypto/ecdsa.Sign is
 * randomised): it is RFC 6979 HMAC-DRBG over SHA-256, derived on the device, so signature
 * values differ from a Go signer's and every verifier accepts them.
 *   FTS_NONCE_RFC6979  deterministic; `seed` is ignored
 *   FTS_NONCE_HEDGED   RFC 6979 section 3.6: 32 bytes of additional data per item, the four
 *                      Rng::next() words of RngSource(seed).at(i), each big-endian
 *                      (FTS_SEED_OS_RANDOM: the secure ChaCha20 source, as for the provers)
 * In neither mode can two different messages under one key share a nonce, whatever the seed.
 * The kernels are not hardened against timing or cache side channels: sign on a device the
 * key owner controls.  The private scalars are wiped from the staging slot before it is
 * released. */
typedef struct {
  const uint8_t* msg; /* message; SHA-256 is computed on the device */
  size_t msg_len;
  const uint8_t* d32; /* private scalar, 32 B big-endian, 0 < d < n */
} fts_ecdsa_sign_item;
#define FTS_ECDSA_SIG_MAX 72
#define FTS_NONCE_RFC6979 0
#define FTS_NONCE_HEDGED 1
/* sig: n * FTS_ECDSA_SIG_MAX bytes, signature i at sig + i * FTS_ECDSA_SIG_MAX, sig_len[i] long.
 * status[i] <- FTS_OK | FTS_E_SIGN_BADKEY (d = 0, d >= n or a NULL d32: sig_len[i] = 0; the other
 * items are not affected).  Argument errors, n = 0, n > 2^24 and a missing device as
 * fts_ecdsa_verify_batch; a nonce_mode other than the two above is FTS_API_EINVAL. */
int fts_ecdsa_sign_batch(int device, size_t n, const fts_ecdsa_sign_item* items, int nonce_mode, uint64_t seed,
                         uint8_t* sig, uint32_t* sig_len, int32_t* status);
/* Host-only: (r, s), 32 B big-endian each -> minimal DER in out72 (at most FTS_ECDSA_SIG_MAX
 * bytes), *len <- its length. */
int fts_ecdsa_sig_encode(const uint8_t* r32, const uint8_t* s32, uint8_t* out72, uint32_t* len);
/* HIP-event durations (ms) of the last fts_ecdsa_sign_batch on `device`:
 * ms2[0] = k_ecdsa_digest, ms2[1] = k_ecdsa_sign (the nonce derivation runs inside it). */
int fts_ecdsa_sign_last_timings(int device, float* ms2);

/* ---- idemix pseudonym signatures (idemix owner identities, BN254 issuer keys) ----
 * Replaces, per item, crypto.NymSignatureVerifier.Verify(message, sigma)
 * (services/identity/idemix/crypto/id.go:145-161 -> IBM/idemix NymSignature.Ver),
 * the owner verifier that services/identity/idemix/deserializer.go:82-105 returns
 * for an idemix identity; called by TransferSignatureValidate
 * (validator/validator_transfer.go:29-62) once per input owner.
 * One handle per issuer public key (the idemix IssuerPublicKey proto, as held in
 * PublicParams.IdemixIssuerPublicKeys): HSk / HRand fixed-base tables in HBM
 * (BN254: 2 x 32 MiB; FP256BN_AMCL: 2 x 64 MiB).  FTS_API_EPP for a key that does not
 * parse or whose HSk / HRand are not on the curve. */
typedef struct fts_idemix_ipk fts_idemix_ipk;
/* curve_id: mathlib CurveID of the key (PublicParams.IdemixIssuerPublicKeys[i].Curve) */
#define FTS_CURVE_FP256BN_AMCL 0
#define FTS_CURVE_BN254 1
int fts_idemix_ipk_create(int device, const uint8_t* ipk, size_t ipk_len, int curve_id, fts_idemix_ipk** out);
void fts_idemix_ipk_destroy(fts_idemix_ipk* ipk);
typedef struct {
  const uint8_t* nym; /* NymPublicKey bytes: G1.Bytes() (BN254: 64 B raw X||Y; FP256BN: 65 B 0x04||X||Y),
                         see fts_idemix_identity_nym */
  size_t nym_len;
  const uint8_t* sig; /* NymSignature proto (proof_c, proof_s_sk, proof_s_r_nym, nonce) */
  size_t sig_len;
  const uint8_t* msg; /* signed message; hashed on the device */
  size_t msg_len;
} fts_nym_item;
/* status[i] <- FTS_OK | FTS_E_NYM_MALFORMED | FTS_E_NYM_BADKEY | FTS_E_NYM_INVALID */
int fts_nym_verify_batch(fts_idemix_ipk* ipk, size_t n, const fts_nym_item* items, int32_t* status);
/* Host-only: SerializedIdemixIdentity.nym_public_key (idemix/crypto/protos/idemix_config.proto,
 * crypto/deserializer.go:41-56); *nym points into `id`. FTS_API_EINVAL if absent or malformed. */
int fts_idemix_identity_nym(const uint8_t* id, size_t len, const uint8_t** nym, size_t* nym_len);
/* HIP-event duration (ms) of k_nym_verify (BN254) / k_nym_verify<FbnCurve> in the last finished fts_nym_verify_batch on `ipk`. */
int fts_nym_last_timings(fts_idemix_ipk* ipk, float* ms);

/* ---- idemix pseudonym signing ----
 * Per item what the nym signer of services/identity/idemix/crypto/id.go produces (IBM/idemix
 * NewNymSignature), with the randomness of RngSource(seed).at(i) drawn on the host in the order
 * nonce, r_sk, r_r (uniform below the key's r; FTS_SEED_OS_RANDOM: the secure source):
 *   t = r_sk HSk + r_r HRand;  c = HashToZr(HashToZr("sign" || t || Nym || ipk.Hash || msg) || nonce);
 *   s_sk = r_sk + c sk;  s_r = r_r + c rnym  (mod r)
 * written as the NymSignature proto (proof_c, proof_s_sk, proof_s_r_nym, nonce: 4 x 34 bytes).
 * Not hardened against timing or cache side channels, secrets wiped from the slot before it is
 * released: as fts_ecdsa_sign_batch. */
typedef struct {
  const uint8_t* sk32;   /* user secret, 32 B big-endian, < r */
  const uint8_t* rnym32; /* nym randomness, 32 B big-endian, < r */
  const uint8_t* nym;    /* G1.Bytes() of Nym = HSk^sk HRand^rnym (64 B / 65 B, as fts_nym_item) */
  size_t nym_len;
  const uint8_t* msg;
  size_t msg_len;
} fts_nym_sign_item;
#define FTS_NYM_SIG_LEN 136
/* sig: n * FTS_NYM_SIG_LEN bytes.  status[i] <- FTS_OK | FTS_E_SIGN_BADKEY (sk or rnym >= r, or
 * NULL) | FTS_E_NYM_BADKEY (nym of the wrong length / form or not on the curve, as in
 * verification); a rejected item's 136 bytes are zero and the other items are not affected.
 * FTS_API_EINVAL for a NULL handle or argument, n > 2^24 or a NULL msg with a length. */
int fts_nym_sign_batch(fts_idemix_ipk* ipk, size_t n, const fts_nym_sign_item* items, uint64_t seed, uint8_t* sig,
                       int32_t* status);
/* HIP-event duration (ms) of k_nym_sign<BnCurve> / k_nym_sign<FbnCurve> in the last finished fts_nym_sign_batch. */
int fts_nym_sign_last_timings(fts_idemix_ipk* ipk, float* ms);

/* ---- idemix identity validity (idemix half) ----
 * Replaces the validity check of idemix Deserializer.Deserialize(raw, true)
 * (services/identity/idemix/deserializer.go:82-93 -> crypto/deserializer.go:36-86 ->
 * crypto/id.go:74-108 verifyProof -> IBM/idemix Signature.Ver with ExpectEidNymRhNym),
 * which TransferSignatureValidate reaches for every input through
 * GetOwnerVerifier (validator/validator_transfer.go:46, core/common/deserializer.go:63-64).
 * One handle per issuer public key: fixed-base tables of HSk, HRand, HAttrs[0..3] and
 * g1 (BN254: 7 x 32 MiB; FP256BN_AMCL: 7 x 64 MiB) and the Miller-loop lines of W and g2.
 * FTS_API_EPP for a key that does not parse, lacks four attributes, or has a point off
 * its curve. */
typedef struct fts_idemix_idv fts_idemix_idv;
int fts_idemix_idv_create(int device, const uint8_t* ipk, size_t ipk_len, int curve_id, fts_idemix_idv** out);
void fts_idemix_idv_destroy(fts_idemix_idv* idv);
/* ids[i] = a serialized idemix owner identity (SerializedIdemixIdentity proto, the token's
 * Owner); status[i] <- FTS_OK or FTS_E_ID_* (the first failing check).  Thread-safe: up to
 * 8 calls on one handle run concurrently (one device slot each); more callers wait for a
 * slot.  The pairing equation is checked per group of 256 identities as one randomised
 * product (fresh getrandom weights per call, soundness 2^-128); the identities of a
 * failing group are paired one by one, so status[i] is the per-identity verdict. */
int fts_idemix_identity_verify_batch(fts_idemix_idv* idv, size_t n, const uint8_t* const* ids, const size_t* id_len,
                                     int32_t* status);
/* HIP-event durations (ms) of the last batch: [0] decode + t-values + transcript, [1] pairings
 * (the batch check and the one-by-one pairings of the identities of failing groups). */
int fts_idemix_identity_last_timings(fts_idemix_idv* idv, float* ms);
/* The last batch's pairing check: out[0] = groups of 256 identities checked with one
 * randomised pairing product each (0 with FTS_IDV_BATCH=0), out[1] = identities paired one
 * by one (those of the groups whose product was not 1; every identity with the batch off). */
int fts_idemix_identity_last_stats(fts_idemix_idv* idv, uint32_t* out);
/* Debug (tests): e(Q, P) on the handle's curve (BN254 or FP256BN) for Q = W (which 0) or
 * g2 (1) and P = X || Y, 64 raw BE bytes (FP256BN too: no 0x04 prefix), after the final
 * exponentiation (final_exp != 0) or the Miller value; out192 = 6 Fp2 coefficients of
 * w^0..w^5, Montgomery, little-endian limbs.  BN254: P must decode as a G1 point other than
 * the identity; FP256BN: coordinates below p (curve membership is the caller's business). */
int fts_idemix_pairing_debug(fts_idemix_idv* idv, int which, const uint8_t* p64, int final_exp, uint32_t* out192);

/* ---- idemix audit info against owner identities ----
 * Replaces AuditInfo.Match (services/identity/idemix/crypto/audit.go:40-84), which the
 * auditor reaches through InspectIdentity for every output, input and issuer
 * (crypto/audit/auditor.go:225-282): the two Csp.Verify calls with EidNymAuditOpts and
 * RhNymAuditOpts, each recomputing HAttrs[idx] * HashToZr(attr) + HRand * rand and comparing
 * it with the EidNym / RhNym point of the identity's proof (audit type AuditExpectSignature).
 * The proof itself is NOT verified (that is fts_idemix_identity_verify_batch) and the nym
 * public key is not read; the Signature proto must unmarshal as a whole.  The caller decodes
 * the AuditInfo JSON and passes Attributes[2], Attributes[3] and the two Rand.Bytes(). */
typedef struct {
  const uint8_t* id;  size_t id_len;   /* SerializedIdemixIdentity (the token's Owner) */
  const uint8_t* eid; size_t eid_len;  /* AuditInfo.Attributes[2] (may be empty) */
  const uint8_t* r_eid32;              /* EidNymAuditData.Rand, Zr.Bytes(), 32 B BE (used mod r) */
  const uint8_t* rh;  size_t rh_len;   /* AuditInfo.Attributes[3] */
  const uint8_t* r_rh32;               /* RhNymAuditData.Rand */
} fts_idemix_audit_item;
/* status[i] <- FTS_OK or FTS_E_AUDIT_* (the first failing check: every EID check precedes
 * every RH check; a NULL rand is FTS_E_AUDIT_MALFORMED).  FTS_API_EINVAL for a NULL handle,
 * NULL arrays with n > 0, an attribute with a NULL pointer and a non-zero length or longer
 * than 0xffffff00 bytes, or n above 2^22.  Thread-safe: up to 3 calls on one handle run
 * concurrently on slots of their own, beside identity-verification calls. */
int fts_idemix_audit_match_batch(fts_idemix_idv* idv, size_t n, const fts_idemix_audit_item* items, int32_t* status);
/* HIP-event duration (ms) of the last batch's kernel (k_idv_audit). */
int fts_idemix_audit_last_timings(fts_idemix_idv* idv, float* ms);

/* ---- idemix owner identities generated on the device ----
 * Per identity what KeyManager.Identity produces (services/identity/idemix/km.go:173-290):
 * a fresh nym, Csp.Sign with IdemixSignerOpts{4 hidden attributes, RhIndex 3, EidIndex 2,
 * SigType EidNymRhNym} (IBM/idemix NewSignature, no message) and the randomness of the audit
 * info, serialized as SerializedIdemixIdentity{1 nym_public_key, 4 proof} -- what
 * SigningIdentity.Serialize yields and fts_idemix_identity_verify_batch /
 * fts_idemix_audit_match_batch take.
 *
 * One handle per credential.  cred: the idemix Credential proto (IdemixSignerConfig.Cred: A, B,
 * E, S, attributes); sk32: the user secret, 32 B big-endian; cri: the
 * CredentialRevocationInformation proto, or NULL (cri_len 0) for epoch 0 and the curve's G2
 * generator as epoch_pk, as ALG_NO_REVOCATION writes it.  The handle BORROWS idv -- its device,
 * its seven fixed-base tables and ipk.Hash -- so idv must outlive it.  It holds fixed-base
 * tables of A and B (BN254: 2 x 32 MiB; FP256BN_AMCL: 2 x 64 MiB) and the constant points
 * HSk sk, HAttrs[2] attrs[2], HAttrs[3] attrs[3].
 * Checked at creation (FTS_API_EPP): exactly four attributes; A and B on the curve, A != O;
 * sk, E, S and the attributes below r; B = g1 + HRand S + HSk sk + sum HAttrs[i] attrs[i]
 * (Credential.Ver's B check); a CRI that does not parse, lacks its epoch key or names a
 * revocation algorithm other than ALG_NO_REVOCATION.  FTS_API_EINVAL for a NULL argument.
 * NOT checked here: the credential's pairing equation e(W + g2 E, A) = e(g2, B).  By
 * bilinearity it is e(W, A) e(g2, E A - B) = 1, which fts_idemix_cred_verify_batch checks
 * on the verifier's handle; without that call a forged A only yields identities that the
 * verifier rejects.
 * Secrets the handle holds on the device are zeroed before they are freed, on destroy and on
 * every error path of create.  Not hardened against timing or cache side channels (table
 * indices and branches depend on secrets), as the other signers. */
typedef struct fts_idemix_cred fts_idemix_cred;
int fts_idemix_cred_create(fts_idemix_idv* idv, const uint8_t* cred, size_t cred_len, const uint8_t* sk32,
                           const uint8_t* cri, size_t cri_len, fts_idemix_cred** out);
void fts_idemix_cred_destroy(fts_idemix_cred* c);
/* Exact length of every identity the handle writes: a function of the curve and the CRI's epoch
 * (BN254 1113 bytes, FP256BN_AMCL 1114, at epoch 0). */
size_t fts_idemix_identity_len(const fts_idemix_cred* c);
/* n identities.  Identity i is written at ids + i * id_stride, id_len[i] <- its length;
 * rnym32 <- the nym's randomness (what fts_nym_sign_batch takes), r_eid32 / r_rh32 <-
 * EidNymAuditData.Rand / RhNymAuditData.Rand of the audit info (n x 32 B big-endian each).
 * r_eid_in32 / r_rh_in32 (n x 32 B each, or NULL): the Identity(auditInfo) case of
 * km.go:199-209, the caller fixes the audit randoms so that EidNym / RhNym equal an earlier
 * identity's.  An in-value >= r gives status[i] = FTS_E_SIGN_BADKEY, zero outputs
 * (id_len[i] = 0) and leaves the other items alone; every other status is FTS_OK.
 * Randomness: item i draws from RngSource(seed).at(i) on the host (seeded: the stream of
 * seed + i, tests only; FTS_SEED_OS_RANDOM: the secure source), uniform below r by rejection,
 * in this order:
 *   rnym, r1, r2, nonce, rSk, rE, rR2, rR3, rS', rRNym, rAttrs[0..3], r_eid, r_rh, rr_eid, rr_rh
 * (rnym, then the order of IBM/idemix NewSignature as oracle/idemix_identity.py sign restates
 * it); r1 = 0 is redrawn; with r_*_in32 the drawn value is consumed, then replaced.
 * FTS_API_ESIZE, before a byte is written, if id_stride < fts_idemix_identity_len; n = 0 is
 * FTS_API_OK; FTS_API_EINVAL for a NULL handle or output array or n > 2^22; FTS_API_EDEVICE
 * for a device failure or a failure of the OS random source (getrandom), as the other
 * signers.  Thread-safe: up to 3 calls on one handle run concurrently (a slot each; the staged
 * draws are wiped from the slot on every way out).  A call above 16,384 identities runs in
 * tiles of that size, so a slot holds at most 72 MB of device memory.
 * The device hands back six points and thirteen scalars per identity (c and the twelve
 * responses); the nonce is written from the host's draws. */
int fts_idemix_identity_generate_batch(fts_idemix_cred* c, size_t n, uint64_t seed, const uint8_t* r_eid_in32,
                                       const uint8_t* r_rh_in32, uint8_t* ids, size_t id_stride, uint32_t* id_len,
                                       uint8_t* rnym32, uint8_t* r_eid32, uint8_t* r_rh32, int32_t* status);
/* The last finished call: ms2[0] = k_idg_prep + k_idg_points, ms2[1] = k_idg_finish (HIP events);
 * host_s2 (may be NULL): seconds of the host pool drawing + staging, and serialising. */
int fts_idemix_identity_generate_last_timings(fts_idemix_cred* c, float* ms2, double* host_s2);
/* Host-only (tests): the 18 scalars above of item i at `seed` (not FTS_SEED_OS_RANDOM),
 * 18 x 32 B big-endian.  r1 cannot be recovered from A', so a byte-exact comparison with the
 * oracle's signer needs them. */
int fts_debug_idemix_identity_draws(int curve_id, uint64_t seed, uint64_t i, uint8_t* out18x32);
/* Host-only (tests): the identity writer on given values.  pts6x64: A' ABar B' Nym EidNym RhNym
 * (X || Y); sc13x32: c sSk sE sR2 sR3 sS' sAttrs[0..3] sRNym sEid sRh; epoch_pk128 NULL: the
 * generator.  *out_len <- the length; FTS_API_ESIZE (nothing written) if out_cap is below it. */
int fts_debug_idemix_identity_write(int curve_id, const uint8_t* pts6x64, const uint8_t* sc13x32,
                                    const uint8_t* nonce32, const uint8_t* epoch_pk128, uint64_t epoch, uint8_t* out,
                                    size_t out_cap, size_t* out_len);

/* ---- idemix credentials verified on the device ----
 * Replaces the check KeyManager construction makes of a signer config
 * (services/identity/idemix/km.go:117-133: Csp.Verify(userKey, cred, ..., IdemixCredentialSignerOpts)
 * -> IBM/idemix Credential.Ver), pairing equation included, for n credentials under the handle's
 * issuer key.  cred: the idemix Credential proto (IdemixSignerConfig.Cred); sk32: the user
 * secret, 32 B big-endian -- the inputs of fts_idemix_cred_create.
 * status[i] <- FTS_OK or the first failing check:
 *   FTS_E_CRED_MALFORMED  a NULL cred or sk32; an empty proto or one that does not parse;
 *                         attributes other than four; E, S, an attribute or sk >= r; A or B that
 *                         does not decode on the handle's curve (BN254: flag bits clear, canonical
 *                         coordinates, on the curve; FP256BN_AMCL: coordinates below p, on the
 *                         curve) or is the identity
 *   FTS_E_CRED_B          B != g1 + HRand S + HSk sk + sum HAttrs[i] attrs[i]
 *   FTS_E_CRED_PAIRING    e(W + g2 E, A) != e(g2, B), checked as e(W, A) e(g2, E A - B) = 1:
 *                         the shape of the identity verifier's equation, on the same Miller-loop
 *                         lines, per group of 256 credentials as one randomised product (fresh
 *                         getrandom weights per call, soundness 2^-128; G1 has cofactor 1 on both
 *                         curves, so every decoded point has order r); the credentials of a
 *                         failing group are paired one by one (all of them with FTS_IDV_BATCH=0)
 * CRI and revocation are not looked at.  FTS_API_EINVAL for a NULL handle, NULL arrays with
 * n > 0 or n > 2^22; n = 0 is FTS_API_OK; FTS_API_EDEVICE for a device failure or a failure of
 * getrandom; FTS_API_ENOMEM.  Thread-safe: a call takes one of the handle's 8 identity-
 * verification slots, so identity and credential calls together never have more than 8
 * pairing stages in flight on a handle.  A call above 16,384 credentials runs in tiles of that
 * size, so it asks a slot for at most 42 MB of device memory.  sk, HSk sk and the lane tables
 * of E A are wiped from the slot's host and device buffers on every way out.  Not hardened
 * against timing or cache side channels, as the signers. */
typedef struct {
  const uint8_t* cred;
  size_t cred_len;
  const uint8_t* sk32;
} fts_idemix_cred_item;
int fts_idemix_cred_verify_batch(fts_idemix_idv* idv, size_t n, const fts_idemix_cred_item* items, int32_t* status);
/* HIP-event durations (ms) of the last credential batch, summed over its tiles: [0] the prep
 * kernels (decode, the seven products, the B check and E A - B), [1] the pairing stage.
 * fts_idemix_identity_last_timings keeps reporting the last identity batch. */
int fts_idemix_cred_verify_last_timings(fts_idemix_idv* idv, float* ms2);
/* The last credential batch's pairing check, summed over its tiles: out2[0] = groups checked
 * with one randomised pairing product each (0 with FTS_IDV_BATCH=0), out2[1] = credentials
 * paired one by one. */
int fts_idemix_cred_verify_last_stats(fts_idemix_idv* idv, uint32_t* out2);

/* ---- idemix enrolment on the device: credential requests and issuance ----
 * The user's NewCredRequest and the issuer's CredRequest.Check and NewCredential (IBM/idemix
 * bccsp/schemes/dlog/crypto credrequest.go, credential.go; the reference reaches them through
 * idemixgen and its CA).  With C the curve of the handle's issuer key, points as G1.Bytes() and
 * scalars as 32 B big-endian:
 *   request  Nym = HSk sk; t = HSk rSk;
 *            c = HashToZr("credRequest" || t || HSk || Nym || IssuerNonce || ipk.Hash); s = rSk + c sk
 *            -> CredRequest{1 nym: ECP{1 x, 2 y}, 2 issuer_nonce, 3 proof_c, 4 proof_s}
 *   check    t = HSk s - Nym c; accept iff c == HashToZr(the same bytes), as integers
 *   issue    the check; B = g1 + Nym + HRand S + sum HAttrs[i] attrs[i]; A = B (isk + E)^-1
 *            -> Credential{1 a, 2 b, 3 e, 4 s, 5 attrs x 4}, what fts_idemix_cred_verify_batch
 *            and fts_idemix_cred_create take
 * UNPINNED: the reference holds no credential-request vector, so the label "credRequest" and
 * the field order of the transcript are restated from the published idemix code.  The
 * credential equation is pinned: an issued credential is accepted by Credential.Ver, which the
 * reference's signer configs pin and fts_idemix_cred_verify_batch runs.
 * Both protos have one fixed length on both curves. */
#define FTS_IDEMIX_CRED_REQUEST_LEN 172
#define FTS_IDEMIX_CREDENTIAL_LEN 344
/* The wallet's side, on the verifier's handle (it needs HSk's table and ipk.Hash only).
 * sk32, nonce32: n x 32 B (the user secrets, the issuer's nonces).  Item i draws rSk from
 * RngSource(seed).at(i) (`seed` + i, tests only; FTS_SEED_OS_RANDOM: the secure source), uniform
 * below r by rejection, on the host pool.  out + i * stride <- the request
 * (FTS_IDEMIX_CRED_REQUEST_LEN bytes), len[i] <- its length.  status[i] <- FTS_OK |
 * FTS_E_SIGN_BADKEY (sk >= r, or a NULL sk32 or nonce32: zero bytes, len[i] = 0, the other items
 * are not affected).  FTS_API_ESIZE, before a byte is written, for a stride below the length;
 * n = 0 is FTS_API_OK; FTS_API_EINVAL for a NULL handle or output array or n > 2^22.  Thread-
 * safe (three slots per handle, shared with the request verifier; tiles of 16,384).  sk and rSk
 * are wiped from the slot on every way out.  Not hardened against timing side channels. */
int fts_idemix_cred_request_batch(fts_idemix_idv* idv, size_t n, const uint8_t* sk32, const uint8_t* nonce32,
                                  uint64_t seed, uint8_t* out, size_t stride, uint32_t* len, int32_t* status);
/* CredRequest.Check alone: holds no secret.  status[i] <- FTS_OK or
 *   FTS_E_CREDREQ_MALFORMED  a NULL or empty input; a proto that does not parse; a missing field;
 *                            proof_c, proof_s or issuer_nonce not of 32 bytes; a Nym that does not
 *                            decode on the handle's curve or is the identity
 *   FTS_E_CREDREQ_INVALID    the challenge differs
 * proof_s >= r is used mod r; proof_c >= r can never equal the recomputed challenge and is
 * FTS_E_CREDREQ_INVALID (the conventions of fts_nym_verify_batch).  Divergences from the
 * reference: a nonce of another length, and the identity as Nym on BN254. */
typedef struct {
  const uint8_t* req;
  size_t req_len;
} fts_idemix_credreq_item;
int fts_idemix_cred_request_verify_batch(fts_idemix_idv* idv, size_t n, const fts_idemix_credreq_item* items,
                                         int32_t* status);
/* HIP-event durations (ms) of the handle's last request batch ([0], k_ci_request) and last
 * request-verification batch ([1], decode, the two products and the check), summed over tiles. */
int fts_idemix_cred_request_last_timings(fts_idemix_idv* idv, float* ms2);

/* One handle per issuer secret.  Borrows idv's device, its seven tables and ipk.Hash, as
 * fts_idemix_cred does: destroy it before idv.  FTS_API_EPP for isk = 0, isk >= r, a key
 * without BarG1 / BarG2 or BarG2 != isk BarG1 (a G1 check on the device; the key's own proof of
 * knowledge, not checked here, ties W to it: fts_idemix_ipk_check_batch checks it).  isk is
 * zeroed on the device and the host before it is freed, on destroy and on every error path. */
typedef struct fts_idemix_issuer fts_idemix_issuer;
int fts_idemix_issuer_create(fts_idemix_idv* idv, const uint8_t* isk32, fts_idemix_issuer** out);
void fts_idemix_issuer_destroy(fts_idemix_issuer* issuer);
/* Check each request, then issue.  attrs4x32: the four attribute values, 32 B big-endian each.
 * Item i draws E, then S from RngSource(seed).at(i) on the host pool; an E with E + isk = 0
 * mod r is drawn again.  creds + i * stride <- the credential (FTS_IDEMIX_CREDENTIAL_LEN bytes),
 * cred_len[i] <- its length.  status[i] <- FTS_OK | FTS_E_SIGN_BADKEY (an attribute >= r or NULL
 * attrs4x32) | FTS_E_CREDREQ_MALFORMED | FTS_E_CREDREQ_INVALID; a rejected item writes zeros and
 * cred_len[i] = 0 and moves no other item's draws or bytes.  FTS_API_ESIZE, before a byte is
 * written, for a stride below the length; n = 0 is FTS_API_OK; FTS_API_EINVAL for a NULL handle
 * or array or n > 2^22.  Thread-safe: three slots per handle; a call above 16,384 items runs in
 * tiles of that size.  (isk + E)^-1, E and S are wiped from the slot on every way out.  Not
 * hardened against timing side channels (table indices and branches depend on secrets). */
typedef struct {
  const uint8_t* req;
  size_t req_len;
  const uint8_t* attrs4x32;
} fts_idemix_issue_item;
int fts_idemix_cred_issue_batch(fts_idemix_issuer* issuer, size_t n, const fts_idemix_issue_item* items,
                                uint64_t seed, uint8_t* creds, size_t stride, uint32_t* cred_len, int32_t* status);
/* The last issue batch: ms2[0] decode, the seven products and the check, ms2[1] A = inv B
 * (HIP events); host_s2 (optional): [0] parsing, draws and staging, [1] serialisation. */
int fts_idemix_cred_issue_last_timings(fts_idemix_issuer* issuer, float* ms2, double* host_s2);
/* Host-only (tests): item i's draws at `seed` (not FTS_SEED_OS_RANDOM), 32 B big-endian each:
 * E, S of fts_idemix_cred_issue_batch, then rSk of fts_idemix_cred_request_batch.
 * avoid_e32 (optional): the value r - isk that E is drawn again on. */
int fts_debug_idemix_cred_issue_draws(int curve_id, uint64_t seed, uint64_t i, const uint8_t* avoid_e32,
                                      uint8_t* out3x32);
/* Host-only (tests): the parser and the writers of host/credreq_write.hpp.  _parse: status of
 * the host's part of the check, out160 <- Nym (X || Y), issuer_nonce, proof_c as sent, proof_s
 * mod r.  The writers fill exactly FTS_IDEMIX_CRED_REQUEST_LEN / FTS_IDEMIX_CREDENTIAL_LEN bytes. */
int fts_debug_idemix_credreq_parse(int curve_id, const uint8_t* req, size_t req_len, int32_t* status, uint8_t* out160);
int fts_debug_idemix_credreq_write(const uint8_t* nym64, const uint8_t* nonce32, const uint8_t* c32, const uint8_t* s32,
                                   uint8_t* out);
int fts_debug_idemix_credential_write(const uint8_t* a64, const uint8_t* b64, const uint8_t* e32, const uint8_t* s32,
                                      const uint8_t* attrs4x32, uint8_t* out);

/* ---- idemix issuer keys on the device: IssuerPublicKey.Check and NewIssuerKey (IBM/idemix
 * bccsp/schemes/dlog/crypto issuerkey.go; the reference runs Check whenever it imports a key and
 * makes keys through idemixgen's CA), on both curves.  The key's proof of knowledge of isk:
 *   check    t1 = g2 s - W c; t2 = BarG1 s - BarG2 c;
 *            accept iff c == HashToZr(t1 || t2 || g2 || BarG1 || W || BarG2), as integers
 *   keygen   W = g2 isk; BarG2 = BarG1 isk; t1 = g2 r; t2 = BarG1 r; c as above; s = r + c isk
 * G1 points are hashed as G1.Bytes(), G2 points as the four 32-byte coordinates of the ECP2
 * proto in field order (1, 2, 3, 4) on both curves.  PINNED: the reference's four issuer keys
 * (two per curve) verify under this reading and under no other coordinate order.
 *
 * IssuerPublicKey.Check for n keys, no handle needed.  status[i] <- FTS_OK or
 *   FTS_E_IPK_MALFORMED  a NULL or empty item; a proto that does not parse; HSk, HRand, an
 *                        HAttrs, BarG1 or BarG2 that does not decode on the curve, or W that does
 *                        not (the rules of fts_idemix_idv_create: canonical coordinates of 32
 *                        bytes, on the curve, the bases not the identity; W on the twist, not
 *                        the identity and, on BN254, in the subgroup); ProofC or ProofS not of
 *                        32 bytes.  BarG2 is not one of the bases: on BN254 its identity
 *                        encoding (64 zero bytes) decodes, as in the reference, its term of t2
 *                        vanishes and the key ends as FTS_E_IPK_PROOF; on FP256BN x = 0, y = 1
 *                        is off the curve and the key is malformed
 *   FTS_E_IPK_UNDEFINED  "some part of the public key is undefined": HSk, HRand, W, BarG1, BarG2,
 *                        ProofC or ProofS missing; fewer HAttrs than attribute names; BarG1 the
 *                        identity (BN254: 64 zero bytes; FP256BN: x = 0, y = 1, AMCL's)
 *   FTS_E_IPK_PROOF      "zero knowledge proof in public key invalid": the challenge differs
 * in this order on the host (parse, missing parts, lengths), then on the device (HSk, HRand,
 * HAttrs and BarG1 decode; BarG1 the identity; BarG2 and W decode; the proof).  The wording of
 * the messages is restated from the published idemix code.  ProofS >= r is used mod r; ProofC
 * >= r can never equal the recomputed challenge and is FTS_E_IPK_PROOF (the conventions of
 * fts_idemix_cred_request_verify_batch and fts_nym_verify_batch).  Unlike the handles, the call
 * does not require four attributes: it checks the key as given.  hash32_out (optional, n x 32
 * B) <- HashToZr of the key's bytes without field 10 (zeros where the proto does not parse);
 * the stored hash field is not compared, as with the handles.  An item's defect does not affect
 * the others.  n = 0 is FTS_API_OK; FTS_API_EINVAL for a NULL array, an unknown curve or n >
 * 2^22; FTS_API_EDEVICE for a device that does not exist or fails.  Each call owns its stream
 * and buffers (one lane per key, tiles of 4,096): meant for key import, not for bulk traffic.
 *
 * fts_idemix_ipk_create, fts_idemix_idv_create and fts_idemix_issuer_create do not run this
 * check and keep accepting what they accepted: a caller that wants the reference's import
 * semantics calls fts_idemix_ipk_check_batch first. */
int fts_idemix_ipk_check_batch(int device, int curve_id, size_t n, const uint8_t* const* ipk, const size_t* ipk_len,
                               int32_t* status, uint8_t* hash32_out);
/* NewIssuerKey with the four attribute names the handles require (OU, Role, EnrollmentID,
 * RevocationHandle); the key has one fixed length on both curves. */
#define FTS_IDEMIX_IPK_LEN 843
/* Key i draws from RngSource(seed).at(i) (`seed` + i, tests only; FTS_SEED_OS_RANDOM: the secure
 * source), each value uniform in [1, r) by rejection, in this order: isk, HSk, HRand,
 * HAttrs[0..3], BarG1, r.  On the device: the bases = their draws times g1, W, BarG2, t1, t2, c
 * and s as above; the host writes fields 1..9 in number order and field 10 = HashToZr of those
 * bytes.  ipk_out + i * ipk_stride <- the key (FTS_IDEMIX_IPK_LEN bytes), ipk_len[i] <- its
 * length, isk32_out + 32 i <- isk (big-endian).  FTS_API_ESIZE, before a byte is written, for a
 * stride below the length; n = 0 is FTS_API_OK; FTS_API_EINVAL for a NULL array, an unknown
 * curve or n > 2^22.  isk, r and every draw are wiped from the call's host and device staging
 * on every way out (isk32_out is the caller's).  Not hardened against timing side channels. */
int fts_idemix_issuer_keygen_batch(int device, int curve_id, size_t n, uint64_t seed, uint8_t* isk32_out,
                                   uint8_t* ipk_out, size_t ipk_stride, uint32_t* ipk_len);
/* HIP-event durations (ms) of this process's last check call ([0]) and last keygen call ([1]),
 * kernels only, summed over tiles. */
int fts_idemix_issuer_key_last_timings(float* ms2);
/* Host-only (tests): key i's draws at `seed` (not FTS_SEED_OS_RANDOM), 32 B big-endian each, in
 * the order above: the nine that key generation consumes, then the stream's next value, which
 * it does not (ten values). */
int fts_debug_idemix_keygen_draws(int curve_id, uint64_t seed, uint64_t i, uint8_t* out10x32);
/* Host-only (tests): the host's part of the check (host/ipk_write.hpp): *status as
 * fts_idemix_ipk_check_batch would leave it before the device runs, hash32 as hash32_out. */
int fts_debug_idemix_ipk_parse(int curve_id, const uint8_t* ipk, size_t ipk_len, int32_t* status, uint8_t* hash32);

#ifdef __cplusplus
}
#endif
#endif /* FTS_GPU_H */
