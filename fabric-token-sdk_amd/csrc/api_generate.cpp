// C-ABI (include/fts_gpu.h): batched token commitments on the device
// (audit_kernels.hip k_token_commit) and whole transfer / issue actions --
// Sender.GenerateZKTransfer (crypto/transfer/sender.go:54-107) and
// Issuer.GenerateZKIssue (crypto/issue/issuer.go:39-84) -- on the host
// (host/generate.hpp) and on the device: commitments by k_token_commit, proofs by
// actions_prove_core, serialization by host/action_write.hpp on the host pool.
#include "host/api_internal.hpp"
#include "host/generate.hpp"

namespace {
constexpr size_t COMMIT_CHUNK = (size_t)1 << 20;  // tokens per device pass (224 B of arena each)
constexpr size_t COMMIT_REC = 96 + 64 + 32 + 32;  // scalars, output, z, prefix product
// <= 48 mixed additions, and per token of a lane's shared inversion 3 products forward and back + 4 to scale
constexpr double COMMIT_PRODUCTS = 48.0 * 11 + 7;

// tokens per lane: TOKEN_COMMIT_PER_LANE; FTS_COMMIT_PER_LANE = 1 / 2 / 4 / 8 / 16 for the A/B of DESIGN.md §5.3
int commit_per_lane() {
  static const int v = [] {
    const char* e = getenv("FTS_COMMIT_PER_LANE");
    const int x = e ? atoi(e) : 0;
    return x == 1 || x == 2 || x == 4 || x == 8 || x == 16 ? x : TOKEN_COMMIT_PER_LANE;
  }();
  return v;
}
}  // namespace

int token_commit_device(fts_ctx* c, size_t n, const CommitItem& item, uint8_t* com64_out) {
  if (n == 0) return FTS_API_OK;
  if (c->device < 0) return FTS_API_EDEVICE;
  HIP_OK(hipSetDevice(c->device));
  LaneGuard lg(c);
  Lane& L = *lg.L;
  const size_t B0 = std::min(n, COMMIT_CHUNK);
  uint8_t* st = L.stage_buf(B0 * (96 + 64));
  if (!st || !L.ws.open_rec.grow(B0 * COMMIT_REC)) return FTS_API_ENOMEM;
  uint32_t* h_sc = reinterpret_cast<uint32_t*>(st);
  uint8_t* h_out = st + B0 * 96;
  uint8_t* d = L.ws.open_rec.as<uint8_t>();
  for (size_t p0 = 0; p0 < n; p0 += B0) {
    const size_t B = std::min(B0, n - p0);
    const double t0 = now_ms();
    // host: HashToZr(type) once per distinct type within a chunk (fts_token_open_batch's staging)
    const size_t CH = 512, nch = (B + CH - 1) / CH;
    parallel_for(nch, 2, [&](size_t ch) {
      constexpr int NC = 8;
      std::string key[NC];
      uint32_t val[NC][8];
      int nc = 0, rr = 0;
      for (size_t i = ch * CH; i < std::min(B, (ch + 1) * CH); i++) {
        const uint8_t *type = nullptr, *bf32 = nullptr;
        size_t type_len = 0;
        uint64_t value = 0;
        item(p0 + i, type, type_len, value, bf32);
        uint32_t* S = h_sc + i * 24;
        int hit = -1;
        for (int q = 0; q < nc && hit < 0; q++)
          if (key[q].size() == type_len && !memcmp(key[q].data(), type, type_len)) hit = q;
        if (hit < 0) {
          hit = nc < NC ? nc++ : (rr++ % NC);
          key[hit].assign((const char*)type, type_len);
          fr_canon_words(hash_to_zr(key[hit]), val[hit]);
        }
        memcpy(S, val[hit], 32);
        S[8] = (uint32_t)value, S[9] = (uint32_t)(value >> 32);
        memset(S + 10, 0, 24);
        zr_canon_words(bf32, S + 16);
      }
    });
    const double t1 = now_ms();
    L.tl.begin(L.s);
    HIP_OK(hipMemcpyAsync(d, h_sc, B * 96, hipMemcpyHostToDevice, L.s));
    L.tl.mark("h2d_commit", L.s, 0);
    c->st_pv_tokens += (int64_t)B, c->st_pv_passes++;
    launch_token_commit((int)B, commit_per_lane(), reinterpret_cast<const uint32_t*>(d), c->d_tables.as<uint32_t>(),
                        c->n, reinterpret_cast<uint32_t*>(d + B0 * 160), reinterpret_cast<uint32_t*>(d + B0 * 192),
                        d + B0 * 96, L.s);
    L.tl.mark("k_token_commit", L.s, COMMIT_PRODUCTS * (double)B);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h_out, d + B0 * 96, B * 64, hipMemcpyDeviceToHost, L.s));
    const double t2 = now_ms();
    HIP_OK(L.sync());
    memcpy(com64_out + 64 * p0, h_out, B * 64);
    L.host_parse_ms = (float)(t1 - t0);
    L.host_stage_ms = 0;
    L.host_prep_ms = 0;
    L.host_enqueue_ms = (float)(t2 - t1);
    L.host_wait_ms = (float)(now_ms() - t2);
    collect_timings(c, L, nullptr);
  }
  return FTS_API_OK;
}

namespace {
// whole actions on the host, action i from src.at(i) and src.at(2^63 + i)
int generate_host(const fts_ctx* c, const fts_gen_action* a, bool issue, uint64_t seed, fts_gen_result* out) {
  if (!c || !a || !gen_result_valid(out) || !gen_valid(*a, issue)) return FTS_API_EINVAL;
  const ProverTables& T = prover_tables(c);
  RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  return gen_host_one(T, c->pp, c->n, c->k, *a, issue, src.at(0), src.at(GEN_BF_STREAM), *out);
}

// Steps 1-3 of generation for actions [lo, hi) of a call on one device context: action i
// (its index in the caller's batch) draws its blinding factors from src.at(GEN_BF_STREAM + i)
// and its prover scalars from src.at(i), whichever device it runs on.  Blinding factors and
// commitments go into the caller's arrays at the outputs' offsets in the call (first[i]),
// proofs[i] <- the action's proof.
int generate_slice(fts_ctx* c, size_t lo, size_t hi, const fts_gen_action* acts, bool issue, const RngSource& src,
                   const std::vector<size_t>& first, const std::vector<size_t>& in_first, fts_gen_result* out,
                   std::string* proofs) {
  const size_t A = hi - lo, t0 = first[lo], T = first[hi] - t0, q0 = in_first[lo], Q = in_first[hi] - q0;
  // 1. blinding factors (into the caller's array) and the provers' witnesses
  std::vector<uint64_t> ov(T), iv(Q);
  std::vector<uint8_t> ib(32 * Q);
  std::vector<uint32_t> owner_of(T);
  std::vector<fts_action_witness> w(A);
  parallel_for(A, 256, [&](size_t s) {
    const size_t i = lo + s, f = first[i] - t0, fi = in_first[i] - q0;
    const fts_gen_action& a = acts[i];
    gen_draw_bfs(src.at(GEN_BF_STREAM + i), a.n_out, out->bf32 + 32 * first[i]);
    for (size_t j = 0; j < a.n_out; j++) ov[f + j] = a.outputs[j].value, owner_of[f + j] = (uint32_t)i;
    const size_t nin = issue ? 0 : a.n_in;
    for (size_t q = 0; q < nin; q++) {
      iv[fi + q] = a.inputs[q].value;
      memcpy(ib.data() + 32 * (fi + q), a.inputs[q].bf32, 32);
    }
    w[s] = fts_action_witness{a.type, a.type_len, nin, iv.data() + fi, ib.data() + 32 * fi,
                              a.n_out, ov.data() + f, out->bf32 + 32 * first[i]};
  });
  // 2. the outputs' commitments (into the caller's array)
  int rc = token_commit_device(c, T, [&](size_t t, const uint8_t*& type, size_t& type_len, uint64_t& value,
                                         const uint8_t*& bf32) {
    const fts_gen_action& a = acts[owner_of[t]];
    type = a.type, type_len = a.type_len, value = ov[t], bf32 = out->bf32 + 32 * (t0 + t);
  }, out->com64 + 64 * t0);
  if (rc) return rc;
  // 3. the proofs
  return actions_prove_core(c, lo, A, w.data(), issue ? 1 : 0, src, proofs + lo);
}

// The parent checks the whole batch, makes the call's one source, lets every device
// generate its slice (split as the action provers split) and packs once.
int generate_device(fts_ctx* c, size_t A, const fts_gen_action* acts, bool issue, uint64_t seed, fts_gen_result* out) {
  if (!c || A > GEN_MAX_ACTIONS || (A && (!acts || !gen_result_valid(out)))) return FTS_API_EINVAL;
  if (A == 0) return FTS_API_OK;
  if (c->device < 0) return FTS_API_EDEVICE;
  std::vector<size_t> first(A + 1, 0), in_first(A + 1, 0);
  for (size_t i = 0; i < A; i++) {
    if (!gen_valid(acts[i], issue)) return FTS_API_EINVAL;
    first[i + 1] = first[i] + acts[i].n_out;
    in_first[i + 1] = in_first[i] + (issue ? 0 : acts[i].n_in);
  }
  const RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  std::vector<double> wt;
  if (!c->shards.empty()) {  // no weight for the commitments: 3 fixed-base products per output
    wt.resize(A);
    for (size_t i = 0; i < A; i++) wt[i] = action_weight(issue ? 0 : acts[i].n_in, acts[i].n_out, !issue);
  }
  std::vector<std::string> proofs(A);
  int rc = over_devices(c, A, c->shards.empty() ? nullptr : &wt, [&](fts_ctx* ch, size_t lo, size_t hi) {
    return generate_slice(ch, lo, hi, acts, issue, src, first, in_first, out, proofs.data());
  });
  if (rc) return rc;
  // 4. actions and metadata
  return gen_emit(A, acts, issue, proofs, out->com64, out->bf32, *out,
                  [](size_t m, auto&& f) { parallel_for(m, 64, f); });
}
}  // namespace

extern "C" {

int fts_token_commit_batch_gpu(fts_ctx* c, size_t n, const fts_commit_item* items, uint8_t* com64_out) {
  if (!c || n > (size_t)(1u << 26) || (n && (!items || !com64_out))) return FTS_API_EINVAL;
  if (c->device < 0) return FTS_API_EDEVICE;
  for (size_t i = 0; i < n; i++)
    if (!items[i].bf32 || (items[i].type_len && !items[i].type)) return FTS_API_EINVAL;
  return over_devices(c, n, nullptr, [&](fts_ctx* ch, size_t lo, size_t hi) {
    return token_commit_device(ch, hi - lo, [&](size_t i, const uint8_t*& type, size_t& type_len, uint64_t& value,
                                                const uint8_t*& bf32) {
      const fts_commit_item& it = items[lo + i];
      type = it.type, type_len = it.type_len, value = it.value, bf32 = it.bf32;
    }, com64_out + 64 * lo);
  });
}

int fts_token_commit_batch_width(void) { return commit_per_lane() * 64; }

int fts_transfer_generate(const fts_ctx* c, const fts_gen_action* a, uint64_t seed, fts_gen_result* out) {
  return generate_host(c, a, false, seed, out);
}
int fts_issue_generate(const fts_ctx* c, const fts_gen_action* a, uint64_t seed, fts_gen_result* out) {
  return generate_host(c, a, true, seed, out);
}
int fts_transfer_generate_batch_gpu(fts_ctx* c, size_t n, const fts_gen_action* a, uint64_t seed, fts_gen_result* out) {
  return generate_device(c, n, a, false, seed, out);
}
int fts_issue_generate_batch_gpu(fts_ctx* c, size_t n, const fts_gen_action* a, uint64_t seed, fts_gen_result* out) {
  return generate_device(c, n, a, true, seed, out);
}

}  // extern "C"
