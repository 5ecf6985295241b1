// Stand-alone check of the action generators (host/generate.hpp) and their
// serializers (host/action_write.hpp), built with the host address and
// undefined-behaviour sanitizers (any report is fatal).  No device, no library: the
// host prover at bit length 8.  Every output buffer is a heap block of exactly the
// size under test, so a write past it is a report.
//   generate_check <public parameters json>      exit status 0 iff every check holds
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../host/generate.hpp"
#include "../host/pb.hpp"
#include "../host/pp_parse.hpp"
#include "../host/request_parse.hpp"

using namespace fts;
using namespace fts::host;

static int g_failed = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      if (g_failed++ < 20) fprintf(stderr, "generate_check: %s (line %d)\n", #x, __LINE__); \
    }                                                             \
  } while (0)

constexpr int N = 8, K = 3;  // bit length, rounds

static const auto serial = [](size_t n, auto&& f) {
  for (size_t i = 0; i < n; i++) f(i);
};

// caller buffers of exactly the given sizes, each in its own heap block
struct Bufs {
  std::unique_ptr<uint8_t[]> actions, meta, com, bf;
  std::vector<size_t> aoff, alen, moff, mlen;
  fts_gen_result r;
  Bufs(size_t n_act, size_t n_out, size_t acap, size_t mcap)
      : actions(new uint8_t[acap]), meta(new uint8_t[mcap]), com(new uint8_t[64 * n_out]), bf(new uint8_t[32 * n_out]),
        aoff(n_act), alen(n_act), moff(n_out), mlen(n_out) {
    r = fts_gen_result{actions.get(), acap, aoff.data(), alen.data(), meta.get(), mcap,
                       moff.data(),   mlen.data(), com.get(), bf.get()};
  }
};

// an independent reading of one length-delimited field list: (field, wire type, bytes / varint)
struct Rec {
  uint32_t f, wt;
  std::string v;
  uint64_t iv;
};
static bool fields(const std::string& m, std::vector<Rec>& out) {
  Pb pb{(const uint8_t*)m.data(), m.size()};
  Pb::Field d;
  out.clear();
  while (pb.o < pb.n) {
    if (!pb.next(d)) return false;
    out.push_back(Rec{d.f, d.wt, d.v ? std::string((const char*)d.v, d.vl) : std::string(), d.iv});
  }
  return true;
}
static std::string b64(const std::string& s) {
  std::string o(aw::b64_len(s.size()), '\0');
  aw::put_b64((uint8_t*)&o[0], (const uint8_t*)s.data(), s.size());
  return o;
}
static std::string json_of(const uint8_t* b, size_t n) {
  return "{\"curve\":1,\"element\":\"" + b64(std::string((const char*)b, n)) + "\"}";
}

// Token{owner, G1{json}} as the fields of `tok`
static void check_token(const std::string& tok, const std::string& owner, const uint8_t* com64) {
  std::vector<Rec> f, g;
  CHECK(fields(tok, f));
  size_t q = 0;
  if (!owner.empty()) {
    CHECK(f.size() == 2 && f[0].f == 1 && f[0].wt == 2 && f[0].v == owner);
    q = 1;
  } else {
    CHECK(f.size() == 1);
  }
  if (f.size() != q + 1) return;
  CHECK(f[q].f == 2 && f[q].wt == 2 && fields(f[q].v, g) && g.size() == 1 && g[0].f == 1 &&
        g[0].v == json_of(com64, 64));
}

static void check_action(const fts_gen_action& a, bool issue, const std::string& act, const uint8_t* coms,
                         const std::string& proof) {
  std::vector<Rec> f, g, h;
  CHECK(fields(act, f));
  const size_t want = (issue ? 1 : a.n_in) + a.n_out + 1;
  CHECK(f.size() == want);
  if (f.size() != want) return;
  size_t q = 0;
  if (issue) {
    CHECK(f[0].f == 1 && f[0].wt == 2 && fields(f[0].v, g));
    if (a.issuer_len) CHECK(g.size() == 1 && g[0].f == 1 && g[0].v == std::string((const char*)a.issuer, a.issuer_len));
    else CHECK(g.empty());
    q = 1;
  } else {
    for (size_t i = 0; i < a.n_in; i++, q++) {
      const fts_gen_input& in = a.inputs[i];
      CHECK(f[q].f == 1 && f[q].wt == 2 && fields(f[q].v, g) && g.size() == 2 && g[0].f == 1 && g[1].f == 2);
      if (g.size() != 2) continue;
      CHECK(fields(g[0].v, h));
      size_t e = 0;
      if (in.tx_id_len) {
        CHECK(h.size() > e && h[e].f == 1 && h[e].v == std::string((const char*)in.tx_id, in.tx_id_len));
        e++;
      }
      if (in.index) {
        CHECK(h.size() > e && h[e].f == 2 && h[e].wt == 0 && h[e].iv == in.index);
        e++;
      }
      CHECK(h.size() == e);
      check_token(g[1].v, std::string((const char*)in.owner, in.owner_len), in.com64);
    }
  }
  for (size_t j = 0; j < a.n_out; j++, q++) {
    CHECK(f[q].f == (issue ? 3u : 2u) && f[q].wt == 2 && fields(f[q].v, g) && g.size() == 1 && g[0].f == 1);
    if (g.size() == 1)
      check_token(g[0].v, std::string((const char*)a.outputs[j].owner, a.outputs[j].owner_len), coms + 64 * j);
  }
  CHECK(f[q].f == (issue ? 4u : 3u) && f[q].wt == 2 && fields(f[q].v, g) && g.size() == 1 && g[0].f == 1 &&
        g[0].v == proof);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: generate_check <public parameters json>\n");
    return 2;
  }
  std::ifstream f(argv[1], std::ios::binary);
  const std::string raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  PublicParams pp;
  std::string err;
  if (!parse_public_params((const uint8_t*)raw.data(), raw.size(), pp, err) || pp.bit_length < (uint64_t)N) {
    fprintf(stderr, "generate_check: public parameters rejected: %s\n", err.c_str());
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

  // owners across the one- to two-byte varint and DER length edges
  const size_t owner_len[5] = {0, 1, 127, 128, 300};
  std::vector<std::string> owner;
  for (size_t l : owner_len) {
    std::string o(l, '\0');
    for (size_t i = 0; i < l; i++) o[i] = (char)(i * 7 + l);
    owner.push_back(o);
  }
  auto op = [&](int i) { return owner[i].empty() ? nullptr : (const uint8_t*)owner[i].data(); };
  uint8_t in_bf[3][32] = {{0}};
  in_bf[0][31] = 101, in_bf[1][31] = 102, in_bf[2][0] = 0xff;  // the last one is above r: used mod r
  uint8_t in_com[3][64];
  const std::string types[3] = {"ABC", "", std::string(200, 't')};
  const std::string tx = "tx-0123456789abcdef";
  uint64_t seed = 40;

  for (int ti = 0; ti < 3; ti++) {
    const std::string& ty = types[ti];
    const uint8_t* typ = ty.empty() ? nullptr : (const uint8_t*)ty.data();
    const Fr tz = type_to_zr(typ, ty.size());
    const uint64_t in_val[3] = {3, 4, 5};
    for (int i = 0; i < 3; i++) g1_to_bytes(token_commit(T, tz, in_val[i], fr_from_be(in_bf[i])), in_com[i]);
    // shapes: (n_in, n_out); n_in == 0 marks an issue; values sum up for the transfers
    const int shapes[6][2] = {{2, 2}, {1, 1}, {1, 2}, {3, 1}, {0, 1}, {0, 4}};
    for (int sh = 0; sh < 6; sh++) {
      const bool issue = shapes[sh][0] == 0;
      const size_t n_in = shapes[sh][0], n_out = shapes[sh][1];
      std::vector<fts_gen_input> ins(n_in);
      uint64_t total = 0;
      for (size_t i = 0; i < n_in; i++) {
        const int o = (int)((i + sh + ti) % 5);
        // an empty tx id, index 0 against 2^63
        const bool empty_tx = (i + sh) % 3 == 1;
        ins[i] = fts_gen_input{empty_tx ? nullptr : (const uint8_t*)tx.data(), empty_tx ? 0 : tx.size(),
                               i % 2 ? 0 : (1ULL << 63), op(o), owner[o].size(), in_com[i], in_val[i], in_bf[i]};
        total += in_val[i];
      }
      std::vector<fts_gen_output> outs(n_out);
      for (size_t j = 0; j < n_out; j++) {
        const int o = sh == 3 ? 0 : (int)((j + 2 * sh + ti) % 5);  // the 3-in/1-out transfer redeems
        const uint64_t v = issue ? 7 + j : (j + 1 == n_out ? total : 1);
        if (!issue) total -= v;
        outs[j] = fts_gen_output{v, op(o), owner[o].size()};
      }
      const int io = (sh + ti) % 5;
      const fts_gen_action a{typ, ty.size(), ins.data(), n_in, outs.data(), n_out, issue ? op(io) : nullptr,
                             issue ? owner[io].size() : 0};
      CHECK(gen_valid(a, issue));
      seed += 3;
      // sizes: a first call into roomy buffers
      Bufs big(1, n_out, 1 << 16, 1 << 14);
      CHECK(gen_host_one(T, pp, N, K, a, issue, Rng(seed), Rng(seed + GEN_BF_STREAM), big.r) == FTS_API_OK);
      const size_t alen = big.alen[0];
      size_t mtot = 0;
      for (size_t j = 0; j < n_out; j++) {
        CHECK(big.moff[j] == mtot);
        mtot += big.mlen[j];
      }
      // exactly the needed size: the same bytes
      Bufs fit(1, n_out, alen, mtot);
      CHECK(gen_host_one(T, pp, N, K, a, issue, Rng(seed), Rng(seed + GEN_BF_STREAM), fit.r) == FTS_API_OK);
      CHECK(fit.alen[0] == alen && !memcmp(fit.actions.get(), big.actions.get(), alen));
      CHECK(!memcmp(fit.meta.get(), big.meta.get(), mtot));
      CHECK(!memcmp(fit.com.get(), big.com.get(), 64 * n_out) && !memcmp(fit.bf.get(), big.bf.get(), 32 * n_out));
      // one byte short, either buffer: FTS_API_ESIZE, lengths reported, nothing written
      {
        Bufs sa(1, n_out, alen - 1, mtot);
        CHECK(gen_host_one(T, pp, N, K, a, issue, Rng(seed), Rng(seed + GEN_BF_STREAM), sa.r) == FTS_API_ESIZE);
        CHECK(sa.alen[0] == alen);
        Bufs sm(1, n_out, alen, mtot - 1);
        CHECK(gen_host_one(T, pp, N, K, a, issue, Rng(seed), Rng(seed + GEN_BF_STREAM), sm.r) == FTS_API_ESIZE);
        CHECK(sm.mlen[n_out - 1] == big.mlen[n_out - 1]);
      }
      // the parts: blinding factors of the bf stream, commitments and proof of the host prover
      std::vector<uint8_t> bfs(32 * n_out), coms(64 * n_out);
      gen_draw_bfs(Rng(seed + GEN_BF_STREAM), n_out, bfs.data());
      CHECK(!memcmp(bfs.data(), fit.bf.get(), 32 * n_out));
      Rng pr(seed);
      const std::string proof = gen_prove_host(T, pp, N, K, a, issue, bfs.data(), pr, coms.data());
      CHECK(!memcmp(coms.data(), fit.com.get(), 64 * n_out));
      // a 1-in/1-out transfer carries no range proofs (transfer.go:85-87): its proof is short
      if (n_in == 1 && n_out == 1) CHECK(proof.size() < 700);
      else CHECK(proof.size() > 700);
      check_action(a, issue, std::string((const char*)fit.actions.get(), alen), coms.data(), proof);
      // every metadata decodes (token.Metadata.Deserialize) to the type, value and bf
      for (size_t j = 0; j < n_out; j++) {
        req::TokenMeta m;
        const uint8_t* mp = fit.meta.get() + fit.moff[j];
        CHECK(req::token_metadata(mp, fit.mlen[j], m));
        CHECK(m.type_len == ty.size() && (ty.empty() || !memcmp(m.type, ty.data(), ty.size())));
        uint8_t v32[32] = {0};
        for (int b = 0; b < 8; b++) v32[31 - b] = (uint8_t)(outs[j].value >> (8 * b));
        CHECK(m.has_value && !memcmp(m.value, v32, 32));
        CHECK(m.has_bf && !memcmp(m.bf, bfs.data() + 32 * j, 32));
      }
    }
  }

  // a batch through gen_emit: offsets are the running sums, and the short buffer is caught
  {
    const fts_gen_output o2[2] = {{1, op(1), 1}, {2, op(4), 300}};
    const fts_gen_action acts[2] = {{(const uint8_t*)"ABC", 3, nullptr, 0, o2, 2, op(2), 127},
                                    {(const uint8_t*)"ABC", 3, nullptr, 0, o2, 1, nullptr, 0}};
    std::vector<uint8_t> bfs(96), coms(192);
    std::vector<std::string> proofs(2);
    for (int i = 0; i < 2; i++) {
      gen_draw_bfs(Rng(900 + i + GEN_BF_STREAM), acts[i].n_out, bfs.data() + 64 * i);
      Rng pr(900 + i);
      proofs[i] = gen_prove_host(T, pp, N, K, acts[i], true, bfs.data() + 64 * i, pr, coms.data() + 128 * i);
    }
    Bufs big(2, 3, 1 << 16, 1 << 14);
    CHECK(gen_emit(2, acts, true, proofs, coms.data(), bfs.data(), big.r, serial) == FTS_API_OK);
    CHECK(big.aoff[0] == 0 && big.aoff[1] == big.alen[0]);
    const size_t atot = big.alen[0] + big.alen[1], mtot = big.mlen[0] + big.mlen[1] + big.mlen[2];
    Bufs fit(2, 3, atot, mtot);
    CHECK(gen_emit(2, acts, true, proofs, coms.data(), bfs.data(), fit.r, serial) == FTS_API_OK);
    CHECK(!memcmp(fit.actions.get(), big.actions.get(), atot) && !memcmp(fit.meta.get(), big.meta.get(), mtot));
    Bufs shrt(2, 3, atot - 1, mtot);
    CHECK(gen_emit(2, acts, true, proofs, coms.data(), bfs.data(), shrt.r, serial) == FTS_API_ESIZE);
    for (int i = 0; i < 2; i++)
      check_action(acts[i], true, std::string((const char*)fit.actions.get() + fit.aoff[i], fit.alen[i]),
                   coms.data() + 128 * i, proofs[i]);
  }

  // invalid arguments are refused before anything is drawn
  {
    fts_gen_output o{1, nullptr, 5};
    fts_gen_action a{nullptr, 0, nullptr, 0, &o, 1, nullptr, 0};
    CHECK(!gen_valid(a, true));
    o.owner_len = 0;
    CHECK(gen_valid(a, true) && !gen_valid(a, false));
    a.n_out = 0;
    CHECK(!gen_valid(a, true));
  }

  if (g_failed) {
    fprintf(stderr, "generate_check: %d check(s) failed\n", g_failed);
    return 1;
  }
  printf("generate_check: ok\n");
  return 0;
}
