// Whole transfer / issue actions (no HIP): Sender.GenerateZKTransfer
// (crypto/transfer/sender.go:54-107) and Issuer.GenerateZKIssue
// (crypto/issue/issuer.go:39-84) around the host prover, and the packing of
// generated actions into caller buffers that the host and the device entry points
// (api_generate.cpp) share.
#pragma once
#include <atomic>
#include <string>
#include <vector>

#include "action_write.hpp"
#include "prover.hpp"

namespace fts {
namespace host {

// index of the blinding-factor stream of action i in its call's RngSource: prover
// streams are [0, 2^22) (the batch limit), so the two never meet
constexpr uint64_t GEN_BF_STREAM = 1ULL << 63;
constexpr size_t GEN_MAX_ACTIONS = (size_t)1 << 22, GEN_MAX_TOKENS = 4096;

// the argument checks of the provers (actions_prove_device) on the generators' input
inline bool gen_valid(const fts_gen_action& a, bool issue) {
  if (!a.n_out || !a.outputs || a.n_out > GEN_MAX_TOKENS || (a.type_len && !a.type)) return false;
  for (size_t j = 0; j < a.n_out; j++)
    if (a.outputs[j].owner_len && !a.outputs[j].owner) return false;
  if (issue) return !(a.issuer_len && !a.issuer);
  if (!a.n_in || !a.inputs || a.n_in > GEN_MAX_TOKENS) return false;
  for (size_t i = 0; i < a.n_in; i++) {
    const fts_gen_input& in = a.inputs[i];
    if (!in.com64 || !in.bf32 || (in.tx_id_len && !in.tx_id) || (in.owner_len && !in.owner)) return false;
  }
  return true;
}

// the output blinding factors of one action, in output order (sender.go:70 /
// issuer.go:44 through token.GetTokensWithWitness: one NewRandomZr per output)
inline void gen_draw_bfs(Rng bf_rng, size_t n_out, uint8_t* bf32) {
  for (size_t j = 0; j < n_out; j++) fr_to_be(bf_rng.fr(), bf32 + 32 * j);
}

// one action on the host: commitments (coms: n_out x 64 B) and the proof, from the
// blinding factors drawn by gen_draw_bfs; prover_rng is the action's prover stream
inline std::string gen_prove_host(const ProverTables& T, const PublicParams& pp, int n, int k, const fts_gen_action& a,
                                  bool issue, const uint8_t* bf32, Rng& prover_rng, uint8_t* coms) {
  const Fr type = type_to_zr(a.type, a.type_len);
  std::vector<uint64_t> ov(a.n_out);
  std::vector<Fr> ob(a.n_out);
  for (size_t j = 0; j < a.n_out; j++) {
    ov[j] = a.outputs[j].value;
    ob[j] = fr_from_be(bf32 + 32 * j);
    g1_to_bytes(token_commit(T, type, ov[j], ob[j]), coms + 64 * j);
  }
  if (issue) return prove_issue(T, pp, n, k, type, ov, ob, prover_rng);
  std::vector<uint64_t> iv(a.n_in);
  std::vector<Fr> ib(a.n_in);
  for (size_t i = 0; i < a.n_in; i++) iv[i] = a.inputs[i].value, ib[i] = fr_from_be(a.inputs[i].bf32);
  return prove_transfer(T, pp, n, k, type, iv, ib, ov, ob, prover_rng);
}

// Pack n generated actions into the caller's buffers: proofs[i], and per output (numbered
// across the call) coms / bfs.  Lengths and offsets first -- FTS_API_ESIZE before a byte
// is written when a buffer is too small -- then the writers, action by action under
// `loop(n, f)` (the device path passes the host pool).  coms / bfs may be r.com64 / r.bf32.
template <class Loop>
int gen_emit(size_t n, const fts_gen_action* acts, bool issue, const std::vector<std::string>& proofs,
             const uint8_t* coms, const uint8_t* bfs, const fts_gen_result& r, Loop&& loop) {
  std::vector<size_t> first(n + 1, 0);
  size_t aoff = 0, moff = 0;
  for (size_t i = 0; i < n; i++) {
    const fts_gen_action& a = acts[i];
    first[i + 1] = first[i] + a.n_out;
    r.action_off[i] = aoff;
    r.action_len[i] = issue ? aw::issue_action_len(a, proofs[i].size()) : aw::transfer_action_len(a, proofs[i].size());
    aoff += r.action_len[i];
    for (size_t j = 0; j < a.n_out; j++) {
      r.meta_off[first[i] + j] = moff;
      r.meta_len[first[i] + j] = aw::metadata_len(a.type_len, issue ? a.issuer_len : 0);
      moff += r.meta_len[first[i] + j];
    }
  }
  if (aoff > r.actions_cap || moff > r.meta_cap) return FTS_API_ESIZE;
  std::atomic<bool> ok{true};
  loop(n, [&](size_t i) {
    const fts_gen_action& a = acts[i];
    const size_t t0 = first[i];
    uint8_t* p = r.actions + r.action_off[i];
    const uint8_t* pr = (const uint8_t*)proofs[i].data();
    uint8_t* e = issue ? aw::write_issue_action(p, a, coms + 64 * t0, pr, proofs[i].size())
                       : aw::write_transfer_action(p, a, coms + 64 * t0, pr, proofs[i].size());
    if (e != p + r.action_len[i]) ok = false;
    for (size_t j = 0; j < a.n_out; j++) {
      uint8_t* m = r.meta + r.meta_off[t0 + j];
      e = aw::write_metadata(m, a.type, a.type_len, a.outputs[j].value, bfs + 32 * (t0 + j), issue ? a.issuer : nullptr,
                             issue ? a.issuer_len : 0);
      if (e != m + r.meta_len[t0 + j]) ok = false;
    }
  });
  if (coms != r.com64) memcpy(r.com64, coms, 64 * first[n]);
  if (bfs != r.bf32) memcpy(r.bf32, bfs, 32 * first[n]);
  return ok ? FTS_API_OK : FTS_API_EINVAL;
}

inline bool gen_result_valid(const fts_gen_result* r) {
  return r && r->actions && r->action_off && r->action_len && r->meta && r->meta_off && r->meta_len && r->com64 &&
         r->bf32;
}

// GenerateZKTransfer / GenerateZKIssue for one action from its two streams
inline int gen_host_one(const ProverTables& T, const PublicParams& pp, int n, int k, const fts_gen_action& a,
                        bool issue, Rng prover_rng, Rng bf_rng, const fts_gen_result& r) {
  std::vector<uint8_t> bfs(32 * a.n_out), coms(64 * a.n_out);
  gen_draw_bfs(bf_rng, a.n_out, bfs.data());
  std::vector<std::string> proof(1);
  proof[0] = gen_prove_host(T, pp, n, k, a, issue, bfs.data(), prover_rng, coms.data());
  return gen_emit(1, &a, issue, proof, coms.data(), bfs.data(), r, [](size_t m, auto&& f) {
    for (size_t i = 0; i < m; i++) f(i);
  });
}

}  // namespace host
}  // namespace fts
