// C-ABI (include/fts_gpu.h): the auditor's checks -- token openings and token
// metadata (audit_kernels.hip).
#include "host/api_internal.hpp"

// ---------------------------------------------------------------------------
// Token opening checks (crypto/audit/auditor.go:226-238, crypto/token/token.go:69-83)
// ---------------------------------------------------------------------------
namespace {
constexpr size_t OPEN_REC = 64 + 96 + 4;       // staged bytes per token
constexpr double OPEN_PRODUCTS = 48.0 * 11 + 4;  // Fp products: <= 48 mixed additions + the projective compare
}  // namespace

extern "C" {

int fts_token_open_batch(fts_ctx* c, size_t n, const fts_token_opening* items, int32_t* status) {
  if (!c || n > (size_t)(1u << 26) || (n && (!items || !status))) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  if (!c->shards.empty())
    return run_shards(plan(n, nullptr, (int)c->shards.size()), [&](int j, size_t lo, size_t hi) {
      return fts_token_open_batch(c->shards[j], hi - lo, items + lo, status + lo);
    });
  if (c->device < 0) return FTS_API_EDEVICE;
  HIP_OK(hipSetDevice(c->device));
  LaneGuard lg(c);
  Lane& L = *lg.L;
  const double t0 = now_ms();
  uint8_t* st = L.stage_buf(n * OPEN_REC);
  if (!st || !L.ws.open_rec.grow(n * OPEN_REC)) return FTS_API_ENOMEM;
  uint8_t* h_raw = st;
  uint32_t* h_sc = reinterpret_cast<uint32_t*>(st + n * 64);
  int32_t* h_st = reinterpret_cast<int32_t*>(st + n * 160);
  // host: HashToZr(type) (one SHA-256 per distinct type within a chunk), scalars mod r
  const size_t CH = 512, nch = (n + CH - 1) / CH;
  parallel_for(nch, 2, [&](size_t ch) {
    // HashToZr of the last few distinct types (a batch carries few token types)
    constexpr int NC = 8;
    std::string key[NC];
    uint32_t val[NC][8];
    int nc = 0, rr = 0;
    for (size_t i = ch * CH; i < std::min(n, (ch + 1) * CH); i++) {
      const fts_token_opening& it = items[i];
      uint32_t* S = h_sc + i * 24;
      if (!it.com64 || !it.value32 || !it.bf32 || (it.type_len && !it.type)) {
        h_st[i] = FTS_E_MALFORMED;
        memset(h_raw + i * 64, 0, 64);
        memset(S, 0, 96);
        continue;
      }
      h_st[i] = FTS_OK;
      memcpy(h_raw + i * 64, it.com64, 64);
      int hit = -1;
      for (int q = 0; q < nc && hit < 0; q++)
        if (key[q].size() == it.type_len && !memcmp(key[q].data(), it.type, it.type_len)) hit = q;
      if (hit < 0) {
        hit = nc < NC ? nc++ : (rr++ % NC);
        key[hit].assign((const char*)it.type, it.type_len);
        fr_canon_words(hash_to_zr(key[hit]), val[hit]);
      }
      memcpy(S, val[hit], 32);
      zr_canon_words(it.value32, S + 8);
      zr_canon_words(it.bf32, S + 16);
    }
  });
  const double t1 = now_ms();
  uint8_t* d = L.ws.open_rec.as<uint8_t>();
  L.tl.begin(L.s);
  HIP_OK(hipMemcpyAsync(d, st, n * OPEN_REC, hipMemcpyHostToDevice, L.s));
  L.tl.mark("h2d_open", L.s, 0);
  launch_open_check((int)n, d, reinterpret_cast<const uint32_t*>(d + n * 64), c->d_tables.as<uint32_t>(), c->n,
                    reinterpret_cast<int32_t*>(d + n * 160), L.s);
  L.tl.mark("k_open_check", L.s, OPEN_PRODUCTS * (double)n);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(h_st, d + n * 160, n * 4, hipMemcpyDeviceToHost, L.s));
  const double t2 = now_ms();
  HIP_OK(L.sync());
  memcpy(status, h_st, n * 4);
  L.host_parse_ms = (float)(t1 - t0);
  L.host_stage_ms = 0;
  L.host_prep_ms = 0;
  L.host_enqueue_ms = (float)(t2 - t1);
  L.host_wait_ms = (float)(now_ms() - t2);
  collect_timings(c, L, nullptr);
  return FTS_API_OK;
}

}  // extern "C"

extern "C" {
// token.Metadata.Deserialize + the opening check (auditor GetAuditInfoFor* + InspectOutput)
int fts_token_metadata_open_batch(fts_ctx* c, size_t n, const uint8_t* com64, const uint8_t* const* meta,
                                  const size_t* meta_len, int32_t* status) {
  if (!c || n > (size_t)(1u << 26) || (n && (!com64 || !meta || !meta_len || !status))) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  if (!c->shards.empty())
    return run_shards(plan(n, nullptr, (int)c->shards.size()), [&](int j, size_t lo, size_t hi) {
      return fts_token_metadata_open_batch(c->shards[j], hi - lo, com64 + 64 * lo, meta + lo, meta_len + lo, status + lo);
    });
  std::vector<req::TokenMeta> md(n);
  std::vector<fts_token_opening> items(n);
  parallel_for(n, 1024, [&](size_t i) {
    fts_token_opening& it = items[i];
    memset(&it, 0, sizeof it);
    req::TokenMeta& m = md[i];
    if (!meta[i] || !req::token_metadata(meta[i], meta_len[i], m)) return;  // NULL com64 -> FTS_E_MALFORMED
    it.com64 = com64 + 64 * i;
    it.type = m.type;
    it.type_len = m.type_len;
    it.value32 = m.has_value ? m.value : nullptr;
    it.bf32 = m.has_bf ? m.bf : nullptr;
  });
  return fts_token_open_batch(c, n, items.data(), status);
}

int fts_token_metadata_decode(const uint8_t* meta, size_t meta_len, int32_t* status, size_t* type_off,
                              size_t* type_len, uint8_t* value32, uint8_t* bf32, int32_t* has) {
  if (!status || !type_off || !type_len || !value32 || !bf32 || !has) return FTS_API_EINVAL;
  req::TokenMeta m;
  *status = meta && req::token_metadata(meta, meta_len, m) ? FTS_OK : FTS_E_MALFORMED;
  *type_off = m.type ? (size_t)(m.type - meta) : 0;
  *type_len = m.type_len;
  memcpy(value32, m.has_value ? m.value : req::kZero64, 32);
  memcpy(bf32, m.has_bf ? m.bf : req::kZero64, 32);
  *has = (m.has_value ? 1 : 0) | (m.has_bf ? 2 : 0);
  return FTS_API_OK;
}
}  // extern "C"
