// C-ABI (include/fts_gpu.h): the provers.  Host entry points over
// host/prover.hpp, and the batched provers on the device (prove_kernels.hip):
// range proofs (rp_prove_device) and whole transfer / issue proofs
// (actions_prove_device).
#include "host/api_internal.hpp"

namespace fts {
namespace host {
RngSource::RngSource(uint64_t sd) : secure(sd == FTS_SEED_OS_RANDOM), seed(sd) {
  if (secure) ok = getrandom(key, sizeof key, 0) == (ssize_t)sizeof key;
}
}  // namespace host
}  // namespace fts

const ProverTables& prover_tables(const fts_ctx* cc) {
  fts_ctx* c = const_cast<fts_ctx*>(cc);
  std::call_once(c->prover_once, [&]() { build_prover_tables(c->pp, c->n, c->ptab); });
  return c->ptab;
}

extern "C" {

int fts_token_commit(const fts_ctx* c, const uint8_t* type, size_t type_len, uint64_t value, const uint8_t* bf32,
                     uint8_t* com64_out) {
  Fr bf;
  if (!c || !com64_out || !fr_arg(bf32, bf)) return FTS_API_EINVAL;
  const ProverTables& T = prover_tables(c);
  G1A t = token_commit(T, type_to_zr(type, type_len), value, bf);
  g1_to_bytes(t, com64_out);
  return FTS_API_OK;
}

int fts_rp_prove(const fts_ctx* c, uint64_t value, const uint8_t* bf32, uint64_t seed, uint8_t* out_der,
                 size_t out_cap, size_t* out_len, uint8_t* com64_out) {
  Fr bf;
  if (!c || !out_der || !out_len || !fr_arg(bf32, bf)) return FTS_API_EINVAL;
  const ProverTables& T = prover_tables(c);
  Msm vm;
  vm.add_fb(T.ped(1), fr_u64(value));
  vm.add_fb(T.ped(2), bf);
  G1A V = vm.aff();
  RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  Rng rng = src.at(0);
  RangeProofOut rp = prove_range(T, c->pp, c->n, c->k, V, value, bf, rng);
  std::string s = rp.serialize();
  *out_len = s.size();
  if (s.size() > out_cap) return FTS_API_ESIZE;
  memcpy(out_der, s.data(), s.size());
  if (com64_out) g1_to_bytes(V, com64_out);
  return FTS_API_OK;
}

int fts_rp_prove_batch(const fts_ctx* c, size_t n, const uint64_t* values, const uint8_t* bfs, uint64_t seed,
                       int threads, uint8_t* out, size_t out_cap, size_t* offsets, size_t* lens,
                       uint8_t* com64_out) {
  if (!c || !values || !bfs || !out || !offsets || !lens || !com64_out) return FTS_API_EINVAL;
  const ProverTables& T = prover_tables(c);
  RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  std::vector<std::string> res(n);
  std::atomic<size_t> next{0};
  int nth = threads > 0 ? threads : (int)host_threads();
  std::vector<std::thread> th;
  for (int t = 0; t < nth; t++)
    th.emplace_back([&]() {
      for (size_t i; (i = next++) < n;) {
        Fr bf = fr_from_be(bfs + 32 * i);
        Msm vm;
        vm.add_fb(T.ped(1), fr_u64(values[i]));
        vm.add_fb(T.ped(2), bf);
        G1A V = vm.aff();
        Rng rng = src.at(i);
        res[i] = prove_range(T, c->pp, c->n, c->k, V, values[i], bf, rng).serialize();
        g1_to_bytes(V, com64_out + 64 * i);
      }
    });
  for (auto& t : th) t.join();
  size_t off = 0;
  for (size_t i = 0; i < n; i++) {
    if (off + res[i].size() > out_cap) return FTS_API_ESIZE;
    memcpy(out + off, res[i].data(), res[i].size());
    offsets[i] = off;
    lens[i] = res[i].size();
    off += res[i].size();
  }
  return FTS_API_OK;
}

int fts_transfer_prove(const fts_ctx* c, const uint8_t* type, size_t type_len, size_t n_in, const uint64_t* in_values,
                       const uint8_t* in_bfs, size_t n_out, const uint64_t* out_values, const uint8_t* out_bfs,
                       uint64_t seed, uint8_t* out_der, size_t out_cap, size_t* out_len) {
  if (!c || !out_der || !out_len || !n_in || !n_out) return FTS_API_EINVAL;
  const ProverTables& T = prover_tables(c);
  std::vector<uint64_t> iv(in_values, in_values + n_in), ov(out_values, out_values + n_out);
  std::vector<Fr> ib(n_in), ob(n_out);
  for (size_t i = 0; i < n_in; i++) ib[i] = fr_from_be(in_bfs + 32 * i);
  for (size_t i = 0; i < n_out; i++) ob[i] = fr_from_be(out_bfs + 32 * i);
  RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  Rng rng = src.at(0);
  std::string s = prove_transfer(T, c->pp, c->n, c->k, type_to_zr(type, type_len), iv, ib, ov, ob, rng);
  *out_len = s.size();
  if (s.size() > out_cap) return FTS_API_ESIZE;
  memcpy(out_der, s.data(), s.size());
  return FTS_API_OK;
}

int fts_issue_prove(const fts_ctx* c, const uint8_t* type, size_t type_len, size_t n_tok, const uint64_t* values,
                    const uint8_t* bfs, uint64_t seed, uint8_t* out_der, size_t out_cap, size_t* out_len) {
  if (!c || !out_der || !out_len || !n_tok) return FTS_API_EINVAL;
  const ProverTables& T = prover_tables(c);
  std::vector<uint64_t> v(values, values + n_tok);
  std::vector<Fr> b(n_tok);
  for (size_t i = 0; i < n_tok; i++) b[i] = fr_from_be(bfs + 32 * i);
  RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  Rng rng = src.at(0);
  std::string s = prove_issue(T, c->pp, c->n, c->k, type_to_zr(type, type_len), v, b, rng);
  *out_len = s.size();
  if (s.size() > out_cap) return FTS_API_ESIZE;
  memcpy(out_der, s.data(), s.size());
  return FTS_API_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Batched range-proof prover on the device (prove_kernels.hip)
// ---------------------------------------------------------------------------
namespace {
constexpr size_t PV_CHUNK = 16384;  // proofs per device pass (~54 KB of arena each at n = 64)

struct PvArena {
  size_t off = 0;
  template <class T>
  size_t take(size_t count) {
    size_t o = off;
    off += (count * sizeof(T) + 255) & ~(size_t)255;
    return o;
  }
};

// stage tables: per-term table slot, groups {t0, t1, seg} of <= PV_TPG terms, segments {g0, g1}
struct PvStageHost {
  std::vector<int32_t> base;
  std::vector<int32_t> grp;  // 4 per group
  std::vector<int32_t> seg;  // 2 per segment
  void segment(int t0, int t1) {  // terms [t0, t1) form the next output point
    const int s = (int)seg.size() / 2, g0 = (int)grp.size() / 4;
    for (int t = t0; t < t1; t += PV_TPG) grp.insert(grp.end(), {t, std::min(t1, t + PV_TPG), s, 0});
    seg.insert(seg.end(), {g0, (int)grp.size() / 4});
  }
};

std::vector<PvStageHost> pv_stage_tables(int n, int k) {
  std::vector<PvStageHost> st(3 + k);
  PvStageHost& s1 = st[0];  // V | C (rho P) | D
  s1.base = {tb_G(n), tb_H(n), tb_P(n)};
  for (int i = 0; i < n; i++) s1.base.insert(s1.base.end(), {i, n + i});
  s1.base.push_back(tb_P(n));
  s1.segment(0, 2);
  s1.segment(2, 3);
  s1.segment(3, 2 * n + 4);
  PvStageHost& s2 = st[1];  // T1 | T2
  s2.base = {tb_G(n), tb_H(n), tb_G(n), tb_H(n)};
  s2.segment(0, 2);
  s2.segment(2, 4);
  PvStageHost& s3 = st[2];  // H'_0 | ... | H'_{n-1} | com
  for (int i = 0; i < n; i++) s3.base.push_back(n + i);
  for (int i = 0; i < n; i++) s3.base.insert(s3.base.end(), {i, n + i});
  for (int i = 0; i < n; i++) s3.segment(i, i + 1);
  s3.segment(n, 3 * n);
  for (int j = 0; j < k; j++) {  // L_j | R_j
    PvStageHost& r = st[3 + j];
    const int m = n >> (j + 1);
    for (int t = 0; t < n; t++) r.base.push_back((t % (2 * m)) >= m ? t : n + t);
    r.base.push_back(tb_Q(n));
    for (int t = 0; t < n; t++) r.base.push_back((t % (2 * m)) < m ? t : n + t);
    r.base.push_back(tb_Q(n));
    r.segment(0, n + 1);
    r.segment(n + 1, 2 * n + 2);
  }
  return st;
}
}  // namespace

// N range proofs on the device: input(i, value, bf8, rnd) supplies proof i's value, its
// blinding factor and its 2n + 4 random scalars (canonical limbs, pv_nrnd order);
// der[i] (N strings) <- the serialized proof, com64_out[i] (optional) <- V
using PvInput = std::function<void(size_t, uint64_t&, uint32_t*, uint32_t*)>;
static int rp_prove_device(fts_ctx* c, Lane& L, size_t N, const PvInput& input, std::string* der,
                           uint8_t* com64_out) {
  const int n = c->n, k = c->k;
  // stage tables (proof-independent), uploaded once per call
  const std::vector<PvStageHost> sth = pv_stage_tables(n, k);
  std::vector<int32_t> tab;
  std::vector<size_t> tb_off;
  for (const PvStageHost& s : sth)
    for (const std::vector<int32_t>* v : {&s.base, &s.grp, &s.seg}) {
      while (tab.size() % 4) tab.push_back(0);  // int4 alignment of the group arrays
      tb_off.push_back(tab.size());
      tab.insert(tab.end(), v->begin(), v->end());
    }
  const size_t B0 = std::min(N, PV_CHUNK);
  PvArena ar;
  const size_t o_tab = ar.take<int32_t>(tab.size()), o_val = ar.take<uint64_t>(B0),
               o_rnd = ar.take<uint32_t>(B0 * pv_nrnd(n) * 8), o_bf = ar.take<uint32_t>(B0 * 8),
               o_st = ar.take<uint32_t>(B0 * pv_nst(n) * 8), o_terms = ar.take<uint32_t>(B0 * pv_tmax(n) * 8),
               o_part = ar.take<uint32_t>(B0 * pv_gmax(n) * 24), o_jac = ar.take<uint32_t>(B0 * (n + 1) * 24),
               o_aff = ar.take<uint32_t>(B0 * (n + 1) * 16), o_hp = ar.take<uint8_t>(B0 * (n + 1) * 64),
               o_out = ar.take<uint8_t>(B0 * pv_npts(k) * 64), o_fr = ar.take<uint32_t>(B0 * PV_NFR * 8),
               o_ch = ar.take<uint32_t>(B0 * rp_nch(k) * 8), o_sc = ar.take<uint32_t>(B0 * RP_NSC * 8),
               o_status = ar.take<int32_t>(B0), o_x0 = ar.take<uint8_t>(B0 * x0_var_bytes(n)),
               o_hs = ar.take<uint8_t>(B0 * PV_HSLOT);
  if (!L.ws.pv.grow(ar.off)) return FTS_API_ENOMEM;
  uint8_t* base = L.ws.pv.as<uint8_t>();
  // pinned staging: inputs [values | rnd | bf], outputs [points | scalars]
  const size_t in_bytes = B0 * (8 + pv_nrnd(n) * 32 + 32), out_pts_b = B0 * pv_npts(k) * 64,
               out_fr_b = B0 * PV_NFR * 32;
  uint8_t* stg = L.stage_buf(in_bytes + out_pts_b + out_fr_b);
  if (!stg) return FTS_API_ENOMEM;
  HIP_OK(hipMemcpyAsync(base + o_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, L.s));
  HIP_OK(hipMemsetAsync(base + o_status, 0, B0 * 4, L.s));
  PvStage stages[3 + 16];
  for (size_t s = 0; s < sth.size(); s++) {
    const int32_t* tb = reinterpret_cast<const int32_t*>(base + o_tab);
    stages[s].T = (int)sth[s].base.size();
    stages[s].G = (int)sth[s].grp.size() / 4;
    stages[s].S = (int)sth[s].seg.size() / 2;
    stages[s].base = tb + tb_off[3 * s];
    stages[s].grp = reinterpret_cast<const int4*>(tb + tb_off[3 * s + 1]);
    stages[s].seg = reinterpret_cast<const int2*>(tb + tb_off[3 * s + 2]);
  }
  for (size_t p0 = 0; p0 < N; p0 += B0) {
    const size_t B = std::min(B0, N - p0);
    uint64_t* h_val = reinterpret_cast<uint64_t*>(stg);
    uint32_t* h_rnd = reinterpret_cast<uint32_t*>(stg + B0 * 8);
    uint32_t* h_bf = reinterpret_cast<uint32_t*>(stg + B0 * 8 + B0 * pv_nrnd(n) * 32);
    // randomness in the host prover's draw order (prove_range): rho, eta, (rl_i, rr_i), tau1, tau2
    const double h0 = now_ms();
    parallel_for(B, 256, [&](size_t i) { input(p0 + i, h_val[i], h_bf + i * 8, h_rnd + i * pv_nrnd(n) * 8); });
    HIP_OK(hipMemcpyAsync(base + o_val, h_val, B * 8, hipMemcpyHostToDevice, L.s));
    HIP_OK(hipMemcpyAsync(base + o_rnd, h_rnd, B * pv_nrnd(n) * 32, hipMemcpyHostToDevice, L.s));
    HIP_OK(hipMemcpyAsync(base + o_bf, h_bf, B * 32, hipMemcpyHostToDevice, L.s));
    PvDev d;
    d.B = (int)B, d.n = n, d.k = k;
    d.tables = c->d_tables.as<uint32_t>();
    d.values = reinterpret_cast<const uint64_t*>(base + o_val);
    d.rnd = reinterpret_cast<const uint32_t*>(base + o_rnd);
    d.bf = reinterpret_cast<const uint32_t*>(base + o_bf);
    d.st = reinterpret_cast<uint32_t*>(base + o_st);
    d.terms = reinterpret_cast<uint32_t*>(base + o_terms);
    d.partial = reinterpret_cast<uint32_t*>(base + o_part);
    d.jac = reinterpret_cast<uint32_t*>(base + o_jac);
    d.aff = reinterpret_cast<uint32_t*>(base + o_aff);
    d.hp_be = base + o_hp;
    d.out_pts = base + o_out;
    d.out_fr = reinterpret_cast<uint32_t*>(base + o_fr);
    d.ch = reinterpret_cast<uint32_t*>(base + o_ch);
    d.sc_ip = reinterpret_cast<uint32_t*>(base + o_sc);
    d.status = reinterpret_cast<int32_t*>(base + o_status);
    d.x0_msgs = base + o_x0;
    d.hslot = base + o_hs;
    const double h1 = now_ms();
    L.tl.begin(L.s);
    c->st_pv_proofs += (int64_t)B, c->st_pv_passes++;
    launch_rp_prove(d, stages, c->d_x0const.as<uint8_t>(), c->d_x0tmpl.as<uint8_t>(), L.s, &L.tl);
    HIP_OK(hipGetLastError());
    uint8_t* h_pts = stg + in_bytes;
    uint32_t* h_fr = reinterpret_cast<uint32_t*>(stg + in_bytes + out_pts_b);
    HIP_OK(hipMemcpyAsync(h_pts, base + o_out, B * pv_npts(k) * 64, hipMemcpyDeviceToHost, L.s));
    HIP_OK(hipMemcpyAsync(h_fr, base + o_fr, B * PV_NFR * 32, hipMemcpyDeviceToHost, L.s));
    const double h2 = now_ms();
    HIP_OK(L.sync());
    const double h3 = now_ms();
    bool bad = false;
    parallel_for(B, 256, [&](size_t i) {
      const uint8_t* P = h_pts + i * pv_npts(k) * 64;
      const uint32_t* F = h_fr + i * PV_NFR * 8;
      auto pt = [&](int slot) {
        G1A a;
        if (!g1_from_bytes(P + slot * 64, 64, a)) bad = true;
        return a;
      };
      auto fr = [&](int slot) {
        uint64_t w[4];
        for (int q = 0; q < 4; q++) w[q] = (uint64_t)F[slot * 8 + 2 * q] | ((uint64_t)F[slot * 8 + 2 * q + 1] << 32);
        return to_mont<ModR>(w);
      };
      RangeProofOut ro;
      ro.T1 = pt(PV_T1), ro.T2 = pt(PV_T2), ro.C = pt(PV_C), ro.D = pt(PV_D);
      ro.tau = fr(PV_F_TAU), ro.delta = fr(PV_F_DELTA), ro.ip = fr(PV_F_IP), ro.a = fr(PV_F_A), ro.b = fr(PV_F_B);
      for (int j = 0; j < k; j++) {
        ro.L.push_back(pt(PV_L(j)));
        ro.R.push_back(pt(PV_R(j)));
      }
      der[p0 + i] = ro.serialize();
      if (com64_out) memcpy(com64_out + 64 * (p0 + i), P + PV_V * 64, 64);
    });
    if (bad) return FTS_API_EDEVICE;  // a device point failed its own encoding check
    L.host_prep_ms = (float)(h1 - h0);         // randomness draw
    L.host_enqueue_ms = (float)(h2 - h1);
    L.host_wait_ms = (float)(h3 - h2);         // device
    L.host_parse_ms = (float)(now_ms() - h3);  // DER serialisation
    L.host_stage_ms = 0;
    collect_timings(c, L, nullptr);
  }
  return FTS_API_OK;
}

extern "C" {

int fts_rp_prove_batch_gpu(fts_ctx* c, size_t N, const uint64_t* values, const uint8_t* bfs, uint64_t seed,
                           uint8_t* out, size_t out_cap, size_t* offsets, size_t* lens, uint8_t* com64_out) {
  if (!c || !values || !bfs || !out || !offsets || !lens || !com64_out || N > (size_t)(1u << 24))
    return FTS_API_EINVAL;
  if (N == 0) return FTS_API_OK;
  if (c->device < 0) return FTS_API_EDEVICE;
  // one source per call, read by every shard: proof g of the call draws from src.at(g)
  const RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  const int nr = pv_nrnd(c->n);
  std::vector<std::string> der(N);
  int rc = over_devices(c, N, nullptr, [&](fts_ctx* ch, size_t lo, size_t hi) {
    if (ch->device < 0) return FTS_API_EDEVICE;
    HIP_OK(hipSetDevice(ch->device));
    LaneGuard lg(ch);
    return rp_prove_device(ch, *lg.L, hi - lo, [&](size_t i, uint64_t& v, uint32_t* bf8, uint32_t* R) {
      const size_t g = lo + i;
      v = values[g];
      Rng rng = src.at(g);  // the host prover's draw order (prove_range)
      for (int r = 0; r < nr; r++) fr_canon_words(rng.fr(), R + r * 8);
      fr_canon_words(fr_from_be(bfs + 32 * g), bf8);
    }, der.data() + lo, com64_out + 64 * lo);
  });
  if (rc) return rc;
  size_t off = 0;
  for (size_t i = 0; i < N; i++) {
    offsets[i] = off;
    lens[i] = der[i].size();
    if (off + der[i].size() > out_cap) return FTS_API_ESIZE;
    memcpy(out + off, der[i].data(), der[i].size());
    off += der[i].size();
  }
  return FTS_API_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Whole transfer / issue proofs on the device: sigma prover (k_sp_prove) + the
// range proofs of every output (rp_prove_device), byte-identical to
// fts_transfer_prove / fts_issue_prove for the same seeds
// ---------------------------------------------------------------------------
bool action_witness_valid(const fts_action_witness& x, int issue) {
  const size_t nin = issue ? 0 : x.n_in;
  return !((!issue && (!nin || !x.in_values || !x.in_bfs)) || !x.n_out || !x.out_values || !x.out_bfs ||
           (x.type_len && !x.type) || nin > 4096 || x.n_out > 4096);
}

int actions_prove_core(fts_ctx* c, size_t g0, size_t A, const fts_action_witness* w, int issue,
                       const RngSource& src, std::string* der) {
  if (!c || !w || !der || A > (size_t)(1u << 22)) return FTS_API_EINVAL;
  if (A == 0) return FTS_API_OK;
  if (c->device < 0 || !src.ok) return FTS_API_EDEVICE;
  const int n = c->n, nr = pv_nrnd(n), kind = issue ? 1 : 0;
  HIP_OK(hipSetDevice(c->device));
  LaneGuard lg(c);
  Lane& L = *lg.L;
  // layout: offsets of every action's scalars / points / transcript / outputs / range proofs
  std::vector<SpAction> act(A);
  std::vector<size_t> rp_first(A + 1, 0);
  size_t nsc = 0, npt = 0, nmsg = 0, nout = 0;
  for (size_t a = 0; a < A; a++) {
    const int nin = issue ? 0 : (int)w[a].n_in, no = (int)w[a].n_out;
    const int m = sp_npts(kind, nin, no);
    act[a] = SpAction{kind, nin, no, (int32_t)nsc, (int32_t)npt, (int32_t)nmsg, (int32_t)nout,
                      kind == 0 ? 2 * nin + no + 2 : 0};
    nsc += sp_nsc(kind, nin, no);
    npt += m;
    nmsg += sp_msg_slot(m);
    nout += sp_nout(kind, nin);
    const bool has_rc = issue || nin != 1 || no != 1;  // transfer.go:85-87 (1-in/1-out: no range proof)
    rp_first[a + 1] = rp_first[a] + (has_rc ? no : 0);
  }
  const size_t NR = rp_first[A];
  std::vector<uint32_t> h_sc(nsc * 8);
  std::vector<uint64_t> rp_val(NR);
  std::vector<uint32_t> rp_bf(NR * 8), rp_rnd(NR * nr * 8);
  // host: the draws of the host prover, in its order (prove_transfer / prove_issue)
  parallel_for(A, 64, [&](size_t a) {
    const fts_action_witness& x = w[a];
    const SpAction& ac = act[a];
    uint32_t* S = h_sc.data() + (size_t)ac.sc_off * 8;
    Rng rng = src.at(g0 + a);  // the action's index in the caller's batch
    const Fr type = type_to_zr(x.type, x.type_len);
    const Fr tbf = rng.fr();
    fr_canon_words(type, S);
    fr_canon_words(tbf, S + 8);
    auto rp_draw = [&](size_t q, uint64_t v, const uint8_t* bf32) {
      const size_t r = rp_first[a] + q;
      rp_val[r] = v;
      fr_canon_words(sub(fr_from_be(bf32), tbf), rp_bf.data() + r * 8);  // V = Out - CT
      for (int t = 0; t < nr; t++) fr_canon_words(rng.fr(), rp_rnd.data() + (r * nr + t) * 8);
    };
    const int N = ac.n_in, M = ac.n_out;
    if (!issue) {
      if (rp_first[a + 1] > rp_first[a])
        for (int j = 0; j < M; j++) rp_draw(j, x.out_values[j], x.out_bfs + 32 * j);
      fr_canon_words(rng.fr(), S + 2 * 8);  // r_t
      fr_canon_words(rng.fr(), S + 3 * 8);  // r_tbf
      for (int i = 0; i < N; i++) {
        fr_canon_words(rng.fr(), S + (5 + 2 * N + i) * 8);  // r_iv_i
        fr_canon_words(rng.fr(), S + (5 + 3 * N + i) * 8);  // r_ibf_i
      }
      fr_canon_words(rng.fr(), S + 4 * 8);  // r_sum
      for (int i = 0; i < N; i++) {
        fr_canon_words(fr_u64(x.in_values[i]), S + (5 + i) * 8);
        fr_canon_words(fr_from_be(x.in_bfs + 32 * i), S + (5 + N + i) * 8);
      }
      for (int j = 0; j < M; j++) {
        fr_canon_words(fr_u64(x.out_values[j]), S + (5 + 4 * N + j) * 8);
        fr_canon_words(fr_from_be(x.out_bfs + 32 * j), S + (5 + 4 * N + M + j) * 8);
      }
    } else {
      fr_canon_words(rng.fr(), S + 2 * 8);  // r_t
      fr_canon_words(rng.fr(), S + 3 * 8);  // r_bf
      for (int j = 0; j < M; j++) rp_draw(j, x.out_values[j], x.out_bfs + 32 * j);
    }
  });
  // device: sigma proofs
  PvArena ar;
  const size_t o_act = ar.take<SpAction>(A), o_sc = ar.take<uint32_t>(nsc * 8), o_jac = ar.take<uint32_t>(npt * 24),
               o_aff = ar.take<uint32_t>(npt * 16), o_be = ar.take<uint8_t>(npt * 64), o_msg = ar.take<uint8_t>(nmsg),
               o_out = ar.take<uint32_t>(nout * 8);
  if (!L.ws.sp.grow(ar.off)) return FTS_API_ENOMEM;
  uint8_t* base = L.ws.sp.as<uint8_t>();
  std::vector<uint8_t> h_be(npt * 64);
  std::vector<uint32_t> h_out(nout * 8);
  HIP_OK(hipMemcpyAsync(base + o_act, act.data(), A * sizeof(SpAction), hipMemcpyHostToDevice, L.s));
  HIP_OK(hipMemcpyAsync(base + o_sc, h_sc.data(), nsc * 32, hipMemcpyHostToDevice, L.s));
  SpDev d;
  d.A = (int)A, d.tables = c->d_tables.as<uint32_t>(), d.n = n;
  d.act = reinterpret_cast<const SpAction*>(base + o_act);
  d.sc = reinterpret_cast<const uint32_t*>(base + o_sc);
  d.jac = reinterpret_cast<uint32_t*>(base + o_jac);
  d.aff = reinterpret_cast<uint32_t*>(base + o_aff);
  d.be = base + o_be;
  d.msgs = base + o_msg;
  d.out = reinterpret_cast<uint32_t*>(base + o_out);
  c->st_pv_actions += (int64_t)A, c->st_pv_passes++;
  launch_sigma_prove(d, L.s);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(h_be.data(), base + o_be, npt * 64, hipMemcpyDeviceToHost, L.s));
  HIP_OK(hipMemcpyAsync(h_out.data(), base + o_out, nout * 32, hipMemcpyDeviceToHost, L.s));
  HIP_OK(L.sync());
  // device: every range proof of the batch
  std::vector<std::string> rps(NR);
  if (NR) {
    int rc = rp_prove_device(c, L, NR, [&](size_t r, uint64_t& v, uint32_t* bf8, uint32_t* R) {
      v = rp_val[r];
      memcpy(bf8, rp_bf.data() + r * 8, 32);
      memcpy(R, rp_rnd.data() + r * nr * 8, (size_t)nr * 32);
    }, rps.data(), nullptr);
    if (rc) return rc;
  }
  // host: DER (transfer.go:140-149 / issue/prover.go:100-111)
  bool bad = false;
  parallel_for(A, 64, [&](size_t a) {
    const SpAction& ac = act[a];
    const uint32_t* O = h_out.data() + (size_t)ac.out_off * 8;
    auto fr = [&](int i) {
      uint64_t q[4];
      for (int t = 0; t < 4; t++) q[t] = (uint64_t)O[i * 8 + 2 * t] | ((uint64_t)O[i * 8 + 2 * t + 1] << 32);
      return to_mont<ModR>(q);
    };
    G1A ct;
    if (!g1_from_bytes(h_be.data() + ((size_t)ac.pt_off + ac.ct_idx) * 64, 64, ct)) bad = true;
    std::vector<std::string> proofs;
    for (size_t r = rp_first[a]; r < rp_first[a + 1]; r++) proofs.push_back(rps[r]);
    if (!issue) {
      const int N = ac.n_in;
      std::vector<Fr> pibf(N), piv(N);
      for (int i = 0; i < N; i++) pibf[i] = fr(i), piv[i] = fr(N + i);
      std::string tas = der::values({el_g1(ct), el_fr_array(pibf), el_fr_array(piv), el_fr(fr(2 * N)),
                                     el_fr(fr(2 * N + 1)), el_fr(fr(2 * N + 2)), el_fr(fr(2 * N + 3))});
      der[a] = der::values({tas, proofs.empty() ? std::string() : rc_serialize(proofs)});
    } else {
      std::string st = der::values({el_fr(fr(0)), el_fr(fr(1)), el_fr(fr(2)), el_g1(ct)});
      der[a] = der::values({st, rc_serialize(proofs)});
    }
  });
  if (bad) return FTS_API_EDEVICE;
  return FTS_API_OK;
}

// The whole batch is checked before any device starts; a multi-device context then splits it
// by the verify side's action weights, every child proving its slice into der at the slice's
// offset with the call's one source, and the parent packs once.
static int actions_prove_device(fts_ctx* c, size_t A, const fts_action_witness* w, int issue, uint64_t seed,
                                uint8_t* out, size_t out_cap, size_t* offsets, size_t* lens) {
  if (!c || !w || !out || !offsets || !lens || A > (size_t)(1u << 22)) return FTS_API_EINVAL;
  if (A == 0) return FTS_API_OK;
  if (c->device < 0) return FTS_API_EDEVICE;
  for (size_t a = 0; a < A; a++)
    if (!action_witness_valid(w[a], issue)) return FTS_API_EINVAL;
  const RngSource src(seed);
  if (!src.ok) return FTS_API_EDEVICE;
  std::vector<double> wt;
  if (!c->shards.empty()) {
    wt.resize(A);
    for (size_t a = 0; a < A; a++) wt[a] = action_weight(issue ? 0 : w[a].n_in, w[a].n_out, !issue);
  }
  std::vector<std::string> der(A);
  int rc = over_devices(c, A, c->shards.empty() ? nullptr : &wt, [&](fts_ctx* ch, size_t lo, size_t hi) {
    return actions_prove_core(ch, lo, hi - lo, w + lo, issue, src, der.data() + lo);
  });
  if (rc) return rc;
  size_t off = 0;
  for (size_t a = 0; a < A; a++) {
    offsets[a] = off;
    lens[a] = der[a].size();
    if (off + der[a].size() > out_cap) return FTS_API_ESIZE;
    memcpy(out + off, der[a].data(), der[a].size());
    off += der[a].size();
  }
  return FTS_API_OK;
}

extern "C" {
int fts_transfer_prove_batch_gpu(fts_ctx* c, size_t n, const fts_action_witness* w, uint64_t seed, uint8_t* out,
                                 size_t out_cap, size_t* offsets, size_t* lens) {
  return actions_prove_device(c, n, w, 0, seed, out, out_cap, offsets, lens);
}
int fts_issue_prove_batch_gpu(fts_ctx* c, size_t n, const fts_action_witness* w, uint64_t seed, uint8_t* out,
                              size_t out_cap, size_t* offsets, size_t* lens) {
  return actions_prove_device(c, n, w, 1, seed, out, out_cap, offsets, lens);
}
}  // extern "C"
