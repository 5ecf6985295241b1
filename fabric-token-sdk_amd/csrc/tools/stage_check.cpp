// Stand-alone check of host/action_stage.hpp, the untrusted-input parser of the
// action path, built with the host address and undefined-behaviour sanitizers
// (any report is fatal).  No device, no library: it makes its own proofs with the
// host prover at bit length 8, and stages honest, truncated and corrupted ones.
// Every proof lives in a heap block of exactly its length and the records in a
// block of exactly the laid-out size, so a read or write past either is a report.
//   stage_check <public parameters json>      exit status 0 iff every check holds
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../host/action_stage.hpp"
#include "../host/pp_parse.hpp"
#include "../host/prover.hpp"

using namespace fts;
using namespace fts::host;

static int g_failed = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      if (g_failed++ < 20) fprintf(stderr, "stage_check: %s (line %d)\n", #x, __LINE__); \
    }                                                             \
  } while (0)

constexpr int N = 8, K = 3;  // bit length, rounds

static const auto serial = [](size_t n, auto&& f) {
  for (size_t i = 0; i < n; i++) f(i);
};
// chunks on four threads (the parser keeps per-thread buffers)
static const auto threaded = [](size_t n, auto&& f) {
  std::vector<std::thread> th;
  for (size_t t = 0; t < 4; t++)
    th.emplace_back([&, t] {
      for (size_t i = t; i < n; i += 4) f(i);
    });
  for (auto& x : th) x.join();
};

// one action of a call: its tokens and an exactly-sized copy of its proof
struct Item {
  int kind = SIG_TAS;
  size_t n_in = 0, n_out = 0;
  const uint8_t *in = nullptr, *out = nullptr;
  std::unique_ptr<uint8_t[]> proof;  // null: a null proof pointer
  size_t len = 0;
  bool honest = false, prefix = false;
};

static Item make_item(const Item& of, const std::string& proof, bool null_proof = false) {
  Item it;
  it.kind = of.kind, it.n_in = of.n_in, it.n_out = of.n_out, it.in = of.in, it.out = of.out;
  if (!null_proof) {
    it.proof.reset(new uint8_t[proof.size()]);
    memcpy(it.proof.get(), proof.data(), proof.size());
    it.len = proof.size();
  }
  return it;
}

struct Staged {
  std::vector<ActionState> st;
  StageLayout lay;
  std::vector<uint8_t> buf;
};

template <class Loop>
static void stage(const std::vector<Item>& items, Staged& s, Loop&& loop) {
  std::vector<ActionIn> acts;
  for (const Item& it : items)
    acts.push_back(ActionIn{it.kind, it.in, it.kind == SIG_TAS ? it.n_in : 0, it.out, it.n_out,
                            der::Span{it.proof.get(), it.proof ? it.len : 0}});
  stage_layout(K, acts, s.st, s.lay, loop);
  s.buf.assign(std::max<size_t>(s.lay.pin_end, 256), 0xa5);
  stage_decode(K, acts, s.st, s.lay, s.buf.data(), loop);
  CHECK(s.st.size() == items.size());
}

// every action is decided on the host, or its records lie inside the laid-out regions
static void check_inside(const std::vector<Item>& items, const Staged& s) {
  const StageLayout& lay = s.lay;
  const StageRun& tot = lay.tot;
  const SigAction* hact = reinterpret_cast<const SigAction*>(s.buf.data() + lay.o_act);
  const int32_t* haffo = reinterpret_cast<const int32_t*>(s.buf.data() + lay.o_affoff);
  CHECK(lay.o_act <= lay.o_raw && lay.o_raw <= lay.o_owner && lay.o_owner <= lay.o_sc && lay.o_sc <= lay.o_work &&
        lay.o_work <= lay.o_affoff && lay.o_affoff <= lay.o_sst && lay.o_sst <= lay.o_rraw && lay.o_rraw <= lay.o_rsc &&
        lay.o_rsc <= lay.o_rst && lay.o_rst <= lay.o_ripa && lay.o_ripa <= lay.in_end && lay.in_end <= lay.o_res &&
        lay.o_res <= lay.pin_end && lay.in_end <= lay.dev_end);
  int nsig = 0;
  for (size_t i = 0; i < items.size(); i++) {
    const ActionState& a = s.st[i];
    if (a.sig < 0) {
      CHECK(a.host_final >= 0);
      continue;
    }
    nsig++;
    CHECK(a.sig < tot.sa);
    const SigAction& sa = hact[a.sig];
    const int n_in = items[i].kind == SIG_TAS ? (int)items[i].n_in : 0, n_out = (int)items[i].n_out;
    CHECK(sa.kind == items[i].kind && sa.n_in == n_in && sa.n_out == n_out);
    CHECK(sa.pt_off >= 0 && sa.pt_off + 1 + n_in + n_out <= tot.pt);
    CHECK(sa.sc_off >= 0 && sa.sc_off + sig_nscalars(sa.kind, n_in) <= tot.sc);
    CHECK(sa.term_off >= 0 && sa.term_off + sig_nterms(sa.kind, n_in) <= tot.term);
    CHECK(sa.msg_off >= 0 && (uint32_t)sa.msg_off + sig_msg_slot(sa.kind, n_in, n_out) <= tot.msg);
    CHECK(haffo[a.sig] >= 0 && haffo[a.sig] + sig_naff(sa.kind, n_in, n_out) <= tot.aff);
    CHECK(sa.rp_base == a.rp_base && sa.rp_count == a.rp_count && a.rp_count >= 0);
    if (a.rp_base >= 0) CHECK(a.rc_applicable && a.rp_base + a.rp_count <= tot.rp);
  }
  CHECK(nsig == tot.sa);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: stage_check <public parameters json>\n");
    return 2;
  }
  std::ifstream f(argv[1], std::ios::binary);
  const std::string raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  PublicParams pp;
  std::string err;
  if (!parse_public_params((const uint8_t*)raw.data(), raw.size(), pp, err) || pp.bit_length < (uint64_t)N) {
    fprintf(stderr, "stage_check: public parameters rejected: %s\n", err.c_str());
    return 2;
  }
  pp.left.resize(N), pp.right.resize(N);
  pp.bit_length = N, pp.rounds = K, pp.max_token = (1ULL << N) - 1, pp.precision = N;
  ProverTables T;  // prover.hpp's table order
  {
    std::vector<G1A> bases(pp.left.begin(), pp.left.end());
    bases.insert(bases.end(), pp.right.begin(), pp.right.end());
    bases.insert(bases.end(), pp.ped.begin(), pp.ped.begin() + 3);
    bases.push_back(pp.P);
    bases.push_back(pp.Q);
    T.n = N;
    T.fb.resize(bases.size());
    for (size_t i = 0; i < bases.size(); i++) T.fb[i].build(bases[i]);
  }

  // ---- the honest actions: a 2-in/2-out transfer, a 1-in/1-out transfer, a 2-token issue
  const Fr type = type_to_zr((const uint8_t*)"ABC", 3);
  auto commit = [&](const std::vector<uint64_t>& v, const std::vector<Fr>& bf) {
    std::vector<uint8_t> o(v.size() * 64);
    for (size_t i = 0; i < v.size(); i++) g1_to_bytes(token_commit(T, type, v[i], bf[i]), o.data() + 64 * i);
    return o;
  };
  auto bfs = [](uint64_t a, uint64_t b) { return std::vector<Fr>{fr_u64(a), fr_u64(b)}; };
  Rng r0(11), r1(12), r2(13);
  const std::vector<uint64_t> in22{3, 4}, out22{5, 2}, in11{7}, out11{7}, tok{9, 200};
  const std::vector<uint8_t> c_in22 = commit(in22, bfs(101, 102)), c_out22 = commit(out22, bfs(103, 104)),
                             c_in11 = commit(in11, {fr_u64(105)}), c_out11 = commit(out11, {fr_u64(106)}),
                             c_tok = commit(tok, bfs(107, 108));
  const std::string p22 = prove_transfer(T, pp, N, K, type, in22, bfs(101, 102), out22, bfs(103, 104), r0),
                    p11 = prove_transfer(T, pp, N, K, type, in11, {fr_u64(105)}, out11, {fr_u64(106)}, r1),
                    pis = prove_issue(T, pp, N, K, type, tok, bfs(107, 108), r2);
  Item t22, t11, is2;
  t22.kind = SIG_TAS, t22.n_in = 2, t22.n_out = 2, t22.in = c_in22.data(), t22.out = c_out22.data();
  t11.kind = SIG_TAS, t11.n_in = 1, t11.n_out = 1, t11.in = c_in11.data(), t11.out = c_out11.data();
  is2.kind = SIG_ST, is2.n_in = 0, is2.n_out = 2, is2.out = c_tok.data();
  const Item* shape[3] = {&t22, &t11, &is2};
  const std::string* proof[3] = {&p22, &p11, &pis};

  // ---- (a) the three honest actions
  {
    std::vector<Item> items;
    for (int q = 0; q < 3; q++) items.push_back(make_item(*shape[q], *proof[q]));
    Staged s;
    stage(items, s, serial);
    StageRun want;
    for (int q = 0; q < 3; q++) {
      const ActionState& a = s.st[q];
      const int n_in = (int)items[q].n_in, n_out = (int)items[q].n_out;
      CHECK(a.host_final < 0);
      CHECK(a.rc_applicable == (q != 1));
      // the prover sends no range proofs with a 1-in/1-out transfer (transfer.go:85-87)
      CHECK(a.rp_count == (q != 1 ? n_out : 0));
      CHECK(!a.rc_count_bad);
      want.add(items[q].kind, n_in, n_out, q != 1 ? n_out : 0);
    }
    const StageRun& tot = s.lay.tot;
    CHECK(tot.sa == want.sa && tot.pt == want.pt && tot.sc == want.sc && tot.term == want.term &&
          tot.nfix == want.nfix && tot.aff == want.aff && tot.rp == want.rp && tot.msg == want.msg);
    CHECK(tot.sa == 3 && tot.rp == 4);
    check_inside(items, s);
  }

  // ---- (b) every strict prefix, and a null proof pointer: the parser alone rejects them
  for (int q : {0, 2}) {
    std::vector<Item> items;
    for (size_t l = 0; l < proof[q]->size(); l++) items.push_back(make_item(*shape[q], proof[q]->substr(0, l)));
    items.push_back(make_item(*shape[q], std::string(), true));
    Staged s;
    stage(items, s, serial);
    size_t kept = 0;
    for (const ActionState& a : s.st) kept += a.host_final != FTS_E_MALFORMED;
    if (kept) fprintf(stderr, "stage_check: %zu prefixes of proof %d not rejected as malformed\n", kept, q);
    CHECK(kept == 0);
    check_inside(items, s);
  }

  // ---- (c) every single byte replaced by 0x00, by 0xff, by its value + 1: staging returns,
  // and whatever is not decided on the host lies inside the layout
  for (int q : {0, 2})
    for (int m = 0; m < 3; m++) {
      std::vector<Item> items;
      for (size_t i = 0; i < proof[q]->size(); i++) {
        std::string p = *proof[q];
        p[i] = m == 0 ? (char)0x00 : m == 1 ? (char)0xff : (char)(p[i] + 1);
        items.push_back(make_item(*shape[q], p));
      }
      Staged s;
      stage(items, s, serial);
      check_inside(items, s);
    }

  // ---- (d) one call of 300 actions (more than two chunks) cycling through all of the above
  {
    std::vector<Item> items;
    for (size_t i = 0; i < 300; i++) {
      const int q = (int)(i % 3), how = (int)((i / 3) % 4);
      const std::string& p = *proof[q];
      const size_t at = (i * 37) % p.size();
      if (how == 0) {
        items.push_back(make_item(*shape[q], p));
        items.back().honest = true;
      } else if (how == 1) {
        items.push_back(make_item(*shape[q], p.substr(0, at), i % 5 == 0));
        items.back().prefix = true;
      } else {
        std::string m = p;
        m[at] = how == 2 ? (char)0xff : (char)(m[at] + 1);
        items.push_back(make_item(*shape[q], m));
      }
    }
    Staged s;
    stage(items, s, threaded);
    for (size_t i = 0; i < items.size(); i++) {
      if (items[i].honest) CHECK(s.st[i].host_final < 0);
      if (items[i].prefix) CHECK(s.st[i].host_final == FTS_E_MALFORMED);
    }
    CHECK(s.lay.base.size() == 3);
    check_inside(items, s);
    // the same call on one thread lays out and decodes the same records
    Staged s1;
    stage(items, s1, serial);
    CHECK(s1.lay.pin_end == s.lay.pin_end && s1.lay.dev_end == s.lay.dev_end);
    for (size_t i = 0; i < items.size(); i++)
      CHECK(s1.st[i].host_final == s.st[i].host_final && s1.st[i].sig == s.st[i].sig);
  }

  if (g_failed) {
    fprintf(stderr, "stage_check: %d check(s) failed\n", g_failed);
    return 1;
  }
  printf("stage_check: ok\n");
  return 0;
}
