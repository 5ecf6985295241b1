// Host half of action staging: the untrusted-input parser of the transfer /
// issue / request path.  Turns a call's actions (attacker-controlled DER proofs)
// into the sigma batch + range-proof records of the device layout, in a
// caller-given buffer.  No HIP call and no context: api_actions.cpp's act_stage
// runs it on a slot's pinned memory and uploads the result,
// fts_debug_stage_actions and tools/stage_check.cpp run it on plain host memory.
// Three steps:
//   1. (parallel) the proofs' outer structure: which actions reach the device and
//      how many range proofs each carries -- the layout's only inputs;
//   2. (serial) offsets of every action's records (integer prefix sums);
//   3. (parallel) the full decode into those offsets.  An action rejected here keeps
//      its records in the layout, marked so every kernel skips them (sigma status
//      FTS_E_MALFORMED, its range proofs FTS_E_NOT_RUN); its verdict is the host's.
// The per-action checks and their order are the reference's deserialisation
// (transfer.go:29-40, typeandsum.go:37-93,230-251, sametype.go:32-64,167-171,
// rangecorrectness.go:19-40, bulletproof.go:37-101, ipa.go:33-67).
// Steps 1 and 2 are stage_layout, step 3 is stage_decode; `loop(n, f)` runs f(i)
// for i in [0, n), in parallel if it likes (the host pool's parallel_for).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../../include/fts_gpu.h"
#include "../device/rp_kernels.hpp"
#include "../device/sigma.hpp"
#include "bn254_host.hpp"
#include "der.hpp"
#include "host_pool.hpp"
#include "proofs.hpp"

namespace fts {
namespace host {

struct ActionIn {
  int kind;                    // SIG_TAS / SIG_ST
  const uint8_t* in;           // n_in * 64
  size_t n_in;
  const uint8_t* out;          // n_out * 64 (issue: tokens)
  size_t n_out;
  der::Span proof;
};

struct ActionState {
  int32_t host_final = -1;     // verdict decided on the host (MALFORMED / TAS_INVALID)
  int sig = -1;                // index in the call's sigma batch (-1: decided before the layout)
  bool rc_applicable = false;
  int rp_base = -1, rp_count = 0;
  bool rc_count_bad = false;
};

// record counts of a run of actions: a chunk's totals, its base, or the call's totals
struct StageRun {
  int sa = 0, pt = 0, sc = 0, term = 0, nfix = 0, aff = 0, rp = 0;
  uint32_t msg = 0;
  // advance past action (kind, n_in, n_out) with nrp slotted range proofs
  void add(int kind, int n_in, int n_out, int nrp) {
    sa++;
    pt += 1 + n_in + n_out;
    sc += sig_nscalars(kind, n_in);
    term += sig_nterms(kind, n_in);
    nfix += sig_nfixed(kind, n_in);
    aff += sig_naff(kind, n_in, n_out);
    msg += sig_msg_slot(kind, n_in, n_out);
    rp += nrp;
  }
};

// Steps 1 and 3 run over chunks of STAGE_CH consecutive actions; step 2 scans the
// chunks' totals only (a serial pass over every action re-read the per-action
// state the parse threads had just written: ~0.1 us per action of cache-line
// transfers), and step 3 lays its chunk out from the chunk's base.
constexpr size_t STAGE_CH = 128;

// Byte offsets of a call's regions (256-byte aligned): the uploaded part [0, in_end)
// (one copy), then the pinned verdict download [o_res, pin_end); on the device the
// workspace [in_end, dev_end) follows the uploaded part instead.
struct StageLayout {
  std::vector<StageRun> base;  // per chunk: the counts before it
  StageRun tot;
  size_t o_act = 0, o_raw = 0, o_owner = 0, o_sc = 0, o_work = 0, o_affoff = 0, o_sst = 0, o_rraw = 0, o_rsc = 0,
         o_rst = 0, o_ripa = 0, in_end = 0, o_res = 0, pin_end = 0;
  size_t w_pts = 0, w_terms = 0, w_aff = 0, w_jac = 0, w_msgs = 0, w_scratch = 0, dev_end = 0;
  double t_shapes = 0;  // now_ms() between steps 1 and 2
};

template <class Loop>
void stage_layout(int k, const std::vector<ActionIn>& acts, std::vector<ActionState>& st, StageLayout& lay,
                  Loop&& loop) {
  const int npts_rp = rp_npts(k);
  const size_t A = acts.size();
  st.assign(A, ActionState{});
  constexpr size_t CH = STAGE_CH;
  const size_t nch = (A + CH - 1) / CH;
  std::vector<StageRun>& base = lay.base;
  base.assign(nch, StageRun{});
  // ---- 1. shapes, and each chunk's totals
  loop(nch, [&](size_t q) {
    thread_local std::vector<der::Span> vals, rps;
    StageRun t;
    for (size_t i = q * CH; i < std::min(A, (q + 1) * CH); i++) {
      const ActionIn& ai = acts[i];
      ActionState& s = st[i];
      if (!der::unmarshal_values(ai.proof, vals) || vals.size() != 2) {
        s.host_final = FTS_E_MALFORMED;
        continue;
      }
      s.rc_applicable = ai.kind == SIG_ST || ai.n_in != 1 || ai.n_out != 1;
      rps.clear();
      if (vals[1].n && !parse_range_correctness(vals[1], rps)) {
        s.host_final = FTS_E_MALFORMED;
        continue;
      }
      s.rp_count = (int)rps.size();
      const int n_in = ai.kind == SIG_TAS ? (int)ai.n_in : 0;
      t.add(ai.kind, n_in, (int)ai.n_out, s.rc_applicable ? s.rp_count : 0);
    }
    base[q] = t;
  });
  lay.t_shapes = now_ms();
  // ---- 2. chunk bases (exclusive scan) and the totals
  StageRun tot;
  for (size_t q = 0; q < nch; q++) {
    const StageRun t = base[q];
    base[q] = tot;
    tot.sa += t.sa, tot.pt += t.pt, tot.sc += t.sc, tot.term += t.term, tot.nfix += t.nfix, tot.aff += t.aff;
    tot.rp += t.rp, tot.msg += t.msg;
  }
  lay.tot = tot;
  const int SA = tot.sa, pt_off = tot.pt, sc_off = tot.sc, aff_off = tot.aff, rp_total = tot.rp;
  const uint32_t msg_off = tot.msg;
  const size_t nwork = (size_t)tot.term;
  size_t o = 0;
  auto region = [&](size_t bytes) {  // 256-byte aligned regions
    size_t r = o;
    o += (bytes + 255) & ~size_t(255);
    return r;
  };
  // uploaded part (one copy), then the pinned verdict download, then device workspace
  lay.o_act = region((size_t)SA * sizeof(SigAction)), lay.o_raw = region((size_t)pt_off * 64),
  lay.o_owner = region((size_t)pt_off * 4), lay.o_sc = region((size_t)sc_off * 32),
  lay.o_work = region(nwork * sizeof(int2)), lay.o_affoff = region((size_t)SA * 4), lay.o_sst = region((size_t)SA * 4),
  lay.o_rraw = region((size_t)rp_total * npts_rp * 64), lay.o_rsc = region((size_t)rp_total * RP_NSC * 32),
  lay.o_rst = region((size_t)rp_total * 4), lay.o_ripa = region((size_t)rp_total * 4);
  lay.in_end = o;
  lay.o_res = region((size_t)SA * 4), lay.pin_end = o;
  o = lay.in_end;
  lay.w_pts = region((size_t)pt_off * 64), lay.w_terms = region(nwork * 96), lay.w_aff = region((size_t)aff_off * 64),
  lay.w_jac = region((size_t)aff_off * 96), lay.w_msgs = region(msg_off),
  lay.w_scratch = region(sig_scratch_words(nwork) * 4), lay.dev_end = o;
}

// hp: at least max(lay.pin_end, 256) writable bytes, 256-byte aligned
template <class Loop>
void stage_decode(int k, const std::vector<ActionIn>& acts, std::vector<ActionState>& st, const StageLayout& lay,
                  uint8_t* hp, Loop&& loop) {
  const int npts_rp = rp_npts(k), nfix_total = lay.tot.nfix;
  const size_t A = acts.size();
  constexpr size_t CH = STAGE_CH;
  const size_t o_raw = lay.o_raw, o_sc = lay.o_sc, o_rraw = lay.o_rraw, o_rsc = lay.o_rsc;
  SigAction* hact = reinterpret_cast<SigAction*>(hp + lay.o_act);
  int32_t* hsst = reinterpret_cast<int32_t*>(hp + lay.o_sst);
  int32_t* hrst = reinterpret_cast<int32_t*>(hp + lay.o_rst);
  int32_t* hripa = reinterpret_cast<int32_t*>(hp + lay.o_ripa);
  int32_t* howner = reinterpret_cast<int32_t*>(hp + lay.o_owner);
  int32_t* haffo = reinterpret_cast<int32_t*>(hp + lay.o_affoff);
  int2* hwork = reinterpret_cast<int2*>(hp + lay.o_work);
  // one action: its records at the running offsets, then its decode
  auto decode_one = [&](size_t i, StageRun& run) {
    thread_local std::vector<der::Span> vals, rps, ubuf, ibf, iv;
    ActionState& s = st[i];
    if (s.host_final >= 0) return;
    const ActionIn& ai = acts[i];
    const int g = run.sa;
    s.sig = g;
    const int n_in = ai.kind == SIG_TAS ? (int)ai.n_in : 0;
    SigAction& sa = hact[g];
    sa = SigAction{};
    sa.kind = ai.kind;
    sa.n_in = n_in;
    sa.n_out = (int)ai.n_out;
    sa.pt_off = run.pt;
    sa.sc_off = run.sc;
    sa.term_off = run.term;
    sa.msg_off = (int32_t)run.msg;
    s.rp_base = s.rc_applicable && s.rp_count > 0 ? run.rp : -1;
    sa.rp_base = s.rp_base;
    sa.rp_count = s.rp_count;
    hsst[g] = 0;
    haffo[g] = run.aff;
    const int npt = 1 + sa.n_in + sa.n_out;
    for (int q = 0; q < npt; q++) howner[sa.pt_off + q] = g;
    // work list: every fixed-base term first, then every variable-base (GLV) term,
    // so each kind has its own kernel (k_sig_fixed, k_sig_var)
    for (int t = 0, nt = sig_nterms(sa.kind, sa.n_in), fi = run.nfix, vi = nfix_total + run.term - run.nfix; t < nt; t++)
      hwork[sig_term_var(sa.kind, sa.n_in, t) ? vi++ : fi++] = make_int2(g, t);
    run.add(ai.kind, n_in, (int)ai.n_out, s.rc_applicable ? s.rp_count : 0);
    // a rejected action keeps its records, skipped by every kernel
    auto fail = [&](int32_t v) {
      s.host_final = v;
      hsst[g] = FTS_E_MALFORMED;
      for (int j = 0; j < s.rp_count && s.rp_base >= 0; j++) {
        hrst[s.rp_base + j] = FTS_E_NOT_RUN;
        hripa[s.rp_base + j] = 0;
      }
    };
    (void)der::unmarshal_values(ai.proof, vals);  // held in step 1
    rps.clear();
    if (vals[1].n) (void)parse_range_correctness(vals[1], rps);
    // ---- range proofs (deserialised together with the sigma proof)
    thread_local std::vector<uint8_t> tpts;
    thread_local std::vector<uint32_t> tsc;
    for (size_t j = 0; j < rps.size(); j++) {
      uint8_t* pts;
      uint32_t* scp;
      int32_t tst = 0, tipa = 0;
      int32_t *pst = &tst, *pipa = &tipa;
      if (s.rp_base >= 0) {
        const size_t r = (size_t)s.rp_base + j;
        pts = hp + o_rraw + r * npts_rp * 64;
        scp = reinterpret_cast<uint32_t*>(hp + o_rsc) + r * RP_NSC * 8;
        pst = hrst + r;
        pipa = hripa + r;
      } else {  // not verified (1-in/1-out transfer), but must deserialise
        tpts.resize((size_t)npts_rp * 64);
        tsc.resize(RP_NSC * 8);
        pts = tpts.data();
        scp = tsc.data();
      }
      parse_range_proof(rps[j], k, pts, scp, *pst, *pipa);
      filler_point(pts + RP_PT_V * 64);
      if (*pst == FTS_E_MALFORMED) return fail(FTS_E_MALFORMED);
      if (!s.rc_applicable) {  // its points decode on the host (no device slot)
        G1A tmp;
        for (int q = 0; q < npts_rp; q++)
          if (q != RP_PT_V && !g1_from_bytes(pts + q * 64, 64, tmp)) return fail(FTS_E_MALFORMED);
      }
    }
    if (s.rc_applicable) s.rc_count_bad = rps.size() != ai.n_out;
    // ---- sigma proof: points [CT, in..., out...], scalars
    uint8_t* raw = hp + o_raw + (size_t)sa.pt_off * 64;
    memset(raw, 0, 64);
    if (sa.n_in) memcpy(raw + 64, ai.in, (size_t)sa.n_in * 64);
    if (ai.n_out) memcpy(raw + (size_t)(1 + sa.n_in) * 64, ai.out, ai.n_out * 64);
    uint32_t* sc = reinterpret_cast<uint32_t*>(hp + o_sc) + (size_t)sa.sc_off * 8;
    memset(sc, 0, (size_t)sig_nscalars(sa.kind, sa.n_in) * 32);
    bool nil_fields = false, panic = false;
    Elem e[7];
    const int ne = ai.kind == SIG_TAS ? 7 : 4;
    if (vals[0].n) {
      Unmarshaller u(vals[0], ubuf);
      if (!u.ok) return fail(FTS_E_MALFORMED);
      for (int f = 0; f < ne; f++)
        if (!u.next(e[f])) return fail(FTS_E_MALFORMED);
    }
    // element kinds: TAS [CT g1, ibf arr, iv arr, Type, TBF, EqSum, Chal]; ST [Type, BF, Chal, CT g1]
    const int ct_idx = ai.kind == SIG_TAS ? 0 : 3;
    if (e[ct_idx].present) {
      if (e[ct_idx].raw.n != 64) return fail(FTS_E_MALFORMED);
      memcpy(raw, e[ct_idx].raw.p, 64);
    }
    if (ai.kind == SIG_TAS) {
      ibf.clear();
      iv.clear();
      if (e[1].present && !der::unmarshal_values(e[1].raw, ibf, true)) return fail(FTS_E_MALFORMED);
      if (e[2].present && !der::unmarshal_values(e[2].raw, iv, true)) return fail(FTS_E_MALFORMED);
      // typeandsum.go:231: nil TBF/Type/CT/EqSum -> "invalid sum and type proof"
      nil_fields = !e[4].present || !e[3].present || !e[0].present || !e[5].present;
      // :242-251 would panic on a nil challenge or short/nil InputValues / InputBlindingFactors
      if (!nil_fields && (!e[6].present || !e[2].present || !e[1].present || iv.size() < ai.n_in || ibf.size() < ai.n_in))
        panic = true;
      // transfer.go:175: the range goroutine dereferences CommitmentToType
      if (s.rc_applicable && !e[0].present) panic = true;
      if (!nil_fields && !panic) {
        scalar_from_bytes(e[3].raw, sc + TAS_SC_TYPE * 8, nullptr);
        scalar_from_bytes(e[4].raw, sc + TAS_SC_TBF * 8, nullptr);
        scalar_from_bytes(e[5].raw, sc + TAS_SC_EQ * 8, nullptr);
        bool canon;
        scalar_from_bytes(e[6].raw, sc + TAS_SC_CHAL * 8, &canon);
        sa.chal_canonical = canon;
        for (size_t j = 0; j < ai.n_in; j++) {
          scalar_from_bytes(iv[j], sc + (TAS_SC_IV + j) * 8, nullptr);
          scalar_from_bytes(ibf[j], sc + (TAS_SC_IV + ai.n_in + j) * 8, nullptr);
        }
      }
    } else if (!e[0].present || !e[1].present || !e[2].present || !e[3].present) {
      panic = true;  // sametype.go:169-171 dereferences every field
    } else {
      scalar_from_bytes(e[0].raw, sc + ST_SC_TYPE * 8, nullptr);
      scalar_from_bytes(e[1].raw, sc + ST_SC_BF * 8, nullptr);
      bool canon;
      scalar_from_bytes(e[2].raw, sc + ST_SC_CHAL * 8, &canon);
      sa.chal_canonical = canon;
    }
    if (panic) return fail(FTS_E_MALFORMED);
    if (nil_fields) {
      // element arrays / CT must still decode even when the proof is rejected for nil fields
      G1A tmp;
      if (e[0].present && !g1_from_bytes(raw, 64, tmp)) return fail(FTS_E_MALFORMED);
      // the range proofs' slotted points too (the unslotted ones decoded above)
      for (int j = 0; j < s.rp_count && s.rp_base >= 0; j++)
        for (int q = 0; q < npts_rp; q++)
          if (q != RP_PT_V && !g1_from_bytes(hp + o_rraw + ((size_t)(s.rp_base + j) * npts_rp + q) * 64, 64, tmp))
            return fail(FTS_E_MALFORMED);
      return fail(FTS_E_TAS_INVALID);
    }
  };
  // ---- 3. lay out and decode, chunk by chunk from its base
  loop((A + CH - 1) / CH, [&](size_t q) {
    StageRun run = lay.base[q];
    for (size_t i = q * CH; i < std::min(A, (q + 1) * CH); i++) decode_one(i, run);
  });
}

}  // namespace host
}  // namespace fts
