// Primitive-level conformance tool: runs the device field, curve, GLV and tower
// functions of device/*.hpp on operands read from a file and writes their raw
// results, for tests/test_gpu_arith.py to compare with integer arithmetic.
//
//   arith_check IN OUT   one record per line of IN: "op operand operand ...";
//                        one result line per record in OUT, in input order
//   arith_check --list   the op catalogue ("name operands results"), no device
//   arith_check --list-chain   the same for the com chain's op (straus4_ctab:
//                        tests/com_chain_vectors.py), kept apart from the primitives' list
//   arith_check --list-glv     the same for the FP256BN GLV chain's op (fbn_glv_mul: tests/arith_vectors.py
//                        FBN_GLV_KS)
//   arith_check --list-fb      the same for the fixed-base ops (tests/fixed_base_vectors.py):
//                        the signed-digit recoding and the table products of fixed_base.hpp
//
// A fixed-base product's record carries, after its device operands, the table entries
// its scalar selects: per table and window three words |d| x y, the affine Montgomery
// point |d| * 2^(W w) * B that the test computed, or 0 0 0 for a zero digit.  The tool
// scatters them to (w * E + |d| - 1) * 16 of a table of the production size that is
// otherwise 0xFF bytes, guard windows before and after included (SparseTable below),
// so a device that looks anywhere else reads poison, inside the allocation.  All
// records of an op share its table(s): two that place different points at one position
// violate the contract.
//
// An operand or result is one 256-bit word in hex (most significant digit first):
// the 8 little-endian uint32 limbs exactly as the device function takes and
// returns them, Montgomery representatives included.  A bool result is the word
// 0 or 1; a 128-bit magnitude, a sign or a carry is a word with the upper limbs 0.
// Points are their coordinates in struct order (G1A x y; G1J/PJ x y z; G1X x y zz
// zzz), tower elements their base-field coefficients in struct order (F2 a b;
// F6 c0 c1 c2; F12 c0 c1).  The tool does no arithmetic on operands or results:
// Montgomery conversion and normalisation are the test's business.
//
// One record per lane, one launch per op, records of an op laid out in the
// order given.  Every record is validated against its op's contract on the
// host before anything is launched (exit 2 on a violation); every HIP call is
// checked (exit 1).  Ops with a data-dependent trip count (f_inv_bin) and the
// experimental products of lib/int_peak are not in the catalogue.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <array>
#include <map>
#include <string>
#include <vector>
#include "../device/glv.hpp"
#include "../device/fbn_glv.hpp"
#include "../device/pairing.hpp"
#include "../host/bn254_host.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1);} } while (0)

struct Aux {  // lane tables of the scalar products (sized as in glv_check.cpp)
  uint32_t* tab;  // [16 entries][24 words][n lanes], or one CTab of n proofs (straus4_ctab)
  uint32_t* scr;  // 10 * 24 words per lane
  size_t n;
};

// ------------------------------------------------------------ loads and stores
template <class T>
FTS_DEV T ld(const uint32_t* a, int w) {
  T r;
#pragma unroll
  for (int q = 0; q < 8; q++) r.v[q] = a[w * 8 + q];
  return r;
}
template <class T>
FTS_DEV void st(uint32_t* r, int w, const T& x) {
#pragma unroll
  for (int q = 0; q < 8; q++) r[w * 8 + q] = x.v[q];
}
FTS_DEV void stw(uint32_t* r, int w, uint32_t x) { r[w * 8] = x; }
FTS_DEV void st4(uint32_t* r, int w, const uint32_t x[4]) {
#pragma unroll
  for (int q = 0; q < 4; q++) r[w * 8 + q] = x[q];
}
FTS_DEV fts::G1A lda(const uint32_t* a, int w) { return {ld<fts::Fp>(a, w), ld<fts::Fp>(a, w + 1)}; }
FTS_DEV fts::G1J ldj(const uint32_t* a, int w) { return {ld<fts::Fp>(a, w), ld<fts::Fp>(a, w + 1), ld<fts::Fp>(a, w + 2)}; }
FTS_DEV fts::G1X ldx(const uint32_t* a, int w) {
  return {ld<fts::Fp>(a, w), ld<fts::Fp>(a, w + 1), ld<fts::Fp>(a, w + 2), ld<fts::Fp>(a, w + 3)};
}
FTS_DEV void sta(uint32_t* r, const fts::G1A& p) { st(r, 0, p.x), st(r, 1, p.y); }
FTS_DEV void stj(uint32_t* r, const fts::G1J& p) { st(r, 0, p.x), st(r, 1, p.y), st(r, 2, p.z); }
FTS_DEV void stx(uint32_t* r, const fts::G1X& p) { st(r, 0, p.x), st(r, 1, p.y), st(r, 2, p.zz), st(r, 3, p.zzz); }
template <class PJ>
FTS_DEV PJ ldpj(const uint32_t* a, int w) {
  PJ p;
  p.x = ld<decltype(p.x)>(a, w), p.y = ld<decltype(p.x)>(a, w + 1), p.z = ld<decltype(p.x)>(a, w + 2);
  return p;
}
template <class PJ>
FTS_DEV void stpj(uint32_t* r, const PJ& p) {
  st(r, 0, p.x), st(r, 1, p.y), st(r, 2, p.z);
}
template <class B>
FTS_DEV pair::F2<B> ld2(const uint32_t* a, int w) {
  return {ld<typename B::F>(a, w), ld<typename B::F>(a, w + 1)};
}
template <class B>
FTS_DEV pair::F6<B> ld6(const uint32_t* a, int w) {
  return {ld2<B>(a, w), ld2<B>(a, w + 2), ld2<B>(a, w + 4)};
}
template <class B>
FTS_DEV pair::F12<B> ld12(const uint32_t* a, int w) {
  return {ld6<B>(a, w), ld6<B>(a, w + 6)};
}
template <class B>
FTS_DEV void st2(uint32_t* r, int w, const pair::F2<B>& x) {
  st(r, w, x.a), st(r, w + 1, x.b);
}
template <class B>
FTS_DEV void st6(uint32_t* r, int w, const pair::F6<B>& x) {
  st2<B>(r, w, x.c0), st2<B>(r, w + 2, x.c1), st2<B>(r, w + 4, x.c2);
}
template <class B>
FTS_DEV void st12(uint32_t* r, int w, const pair::F12<B>& x) {
  st6<B>(r, w, x.c0), st6<B>(r, w + 6, x.c1);
}

// ------------------------------------------------------------------------ ops
// struct Name { ni operand words, no result words, run(a, r, aux, lane) }
#define OP(NAME, NI, NO, ...)                                                                      \
  struct NAME {                                                                                    \
    static constexpr int ni = NI, no = NO;                                                         \
    static FTS_DEV void run(const uint32_t* a, uint32_t* r, const Aux& x, size_t i) { __VA_ARGS__ } \
  }
#define TOP(T, NAME, NI, NO, ...) template <class T> OP(NAME, NI, NO, __VA_ARGS__)
#define TOP_W(W, NAME, NI, NO, ...) template <int W> OP(NAME, NI, NO, __VA_ARGS__)

// BN254 Fp / Fr (field.hpp)
TOP(P, FAdd, 2, 1, using F = fts::Field<P>; st(r, 0, fts::f_add(ld<F>(a, 0), ld<F>(a, 1))););
TOP(P, FSub, 2, 1, using F = fts::Field<P>; st(r, 0, fts::f_sub(ld<F>(a, 0), ld<F>(a, 1))););
TOP(P, FNeg, 1, 1, using F = fts::Field<P>; st(r, 0, fts::f_neg(ld<F>(a, 0))););
TOP(P, FDbl, 1, 1, using F = fts::Field<P>; st(r, 0, fts::f_dbl(ld<F>(a, 0))););
TOP(P, FMul, 2, 1, using F = fts::Field<P>; st(r, 0, fts::f_mul(ld<F>(a, 0), ld<F>(a, 1))););
TOP(P, FToMont, 1, 1, using F = fts::Field<P>; st(r, 0, fts::f_to_mont(ld<F>(a, 0))););
TOP(P, FFromMont, 1, 1, using F = fts::Field<P>; st(r, 0, fts::f_from_mont(ld<F>(a, 0))););
TOP(P, FReduceOnce, 1, 1, using F = fts::Field<P>; F t = ld<F>(a, 0); fts::f_reduce_once(t); st(r, 0, t););
TOP(P, FLtMod, 1, 1, stw(r, 0, fts::limbs_lt_mod<P>(a) ? 1u : 0u););
OP(FpMulG, 2, 1, st(r, 0, fts::fp_mul(ld<fts::Fp>(a, 0), ld<fts::Fp>(a, 1))););
OP(FrMulG, 2, 1, st(r, 0, fts::fr_mul(ld<fts::Fr>(a, 0), ld<fts::Fr>(a, 1))););
OP(FpInv, 1, 1, st(r, 0, fts::nl_fp_inv(ld<fts::Fp>(a, 0))););
OP(FrInv, 1, 1, st(r, 0, fts::nl_fr_inv(ld<fts::Fr>(a, 0))););

// full-width Montgomery code (p256.hpp) over P-256's p, n and FP256BN's p, r
TOP(P, WAdd, 2, 1, using F = p256::F<P>; st(r, 0, p256::add(ld<F>(a, 0), ld<F>(a, 1))););
TOP(P, WSub, 2, 1, using F = p256::F<P>; st(r, 0, p256::sub(ld<F>(a, 0), ld<F>(a, 1))););
TOP(P, WMul, 2, 1, using F = p256::F<P>; st(r, 0, p256::mul(ld<F>(a, 0), ld<F>(a, 1))););
TOP(P, WToMont, 1, 1, using F = p256::F<P>; st(r, 0, p256::to_mont(ld<F>(a, 0))););
TOP(P, WFromMont, 1, 1, using F = p256::F<P>; st(r, 0, p256::from_mont(ld<F>(a, 0))););
TOP(P, WInv, 1, 1, using F = p256::F<P>; st(r, 0, p256::inv(ld<F>(a, 0))););
TOP(P, WCondSub, 2, 1, using F = p256::F<P>; F t = ld<F>(a, 0); p256::cond_sub(t, a[8]); st(r, 0, t););
OP(Lt256, 2, 1, stw(r, 0, p256::lt256(a, a + 8) ? 1u : 0u););

// BN254 G1 (g1.hpp, fixed_base.hpp)
OP(JDbl, 3, 3, stj(r, fts::g1j_dbl(ldj(a, 0))););
OP(JAddAffine, 5, 3, stj(r, fts::g1j_add_affine(ldj(a, 0), lda(a, 3))););
OP(JAdd, 6, 3, stj(r, fts::g1j_add(ldj(a, 0), ldj(a, 3))););
OP(MaddInl, 5, 3, fts::G1J p = ldj(a, 0); fts::madd_inl(p, lda(a, 3)); stj(r, p););
OP(AddInl, 6, 3, fts::G1J p = ldj(a, 0); fts::add_inl(p, ldj(a, 3)); stj(r, p););
OP(JToAffine, 3, 2, sta(r, fts::g1j_to_affine(ldj(a, 0))););
OP(JEq, 6, 1, stw(r, 0, fts::g1j_eq(ldj(a, 0), ldj(a, 3)) ? 1u : 0u););
OP(XMaddInl, 6, 4, fts::G1X p = ldx(a, 0); fts::xmadd_inl(p, lda(a, 4)); stx(r, p););
OP(XAddInl, 8, 4, fts::G1X p = ldx(a, 0); fts::xadd_inl(p, ldx(a, 4)); stx(r, p););
OP(XDbl, 4, 4, stx(r, fts::g1x_dbl(ldx(a, 0))););
OP(XToJac, 4, 3, stj(r, fts::g1x_to_jac(ldx(a, 0))););
OP(VarBaseMul, 3, 3, stj(r, fts::var_base_mul(lda(a, 0), ld<fts::Scalar>(a, 2), x.scr + i * 10 * 24)););
OP(GlvMul, 3, 3, stj(r, fts::glv_mul(lda(a, 0), ld<fts::Scalar>(a, 2), x.tab, x.n, i)););
OP(Vb128j, 4, 3, stj(r, fts::vb128j(ldj(a, 0), a + 24, x.tab, x.n, i)););
OP(Straus2, 8, 3, stj(r, fts::straus2_128(ldj(a, 0), a + 24, ldj(a, 4), a + 56, x.tab, x.n, i)););
// the com chain (glv.hpp).  straus4_ctab: D (affine), S (Jacobian), then
// |a1| s1 |a2| s2 |b1| t1 |b2| t2; the lane builds its proof's CTab (D's rows as
// k_rp_com_tab does, then S's) in the table buffer and runs the chain over it
OP(Straus4Ctab, 13, 3, const fts::CTab T{x.tab, x.n, i}; const fts::G1A D = lda(a, 0); const fts::G1J S = ldj(a, 2);
   const bool idD = fts::g1a_is_identity(D); const bool idS = fts::f_is_zero(S.z);
   fts::ctab_build8<true>(T, 0, fts::g1j_from_affine(D), idD); fts::ctab_build8<false>(T, 8, S, idS);
   stj(r, fts::straus4_ctab(T, a + 40, a[48] != 0, a + 56, a[64] != 0, a + 72, a[80] != 0, a + 88, a[96] != 0, idD, idS)););

// fixed-base digits and table products (fixed_base.hpp).  The digit ops call the
// recoding as the products do (a copy of k shifted in place, carry 0 in) and return
// the NW digits, each as the int's 32 bits in limb 0, then the carry out.  The
// products read the op's sparse table(s), x.tab and for fb_mul2's second base x.scr
template <int W>
struct FbDigitsW {
  static constexpr int ni = 1, no = fts::FbCfg<W>::NW + 1;
  static FTS_DEV void run(const uint32_t* a, uint32_t* r, const Aux&, size_t) {
    uint32_t s[8];
#pragma unroll
    for (int q = 0; q < 8; q++) s[q] = a[q];
    int carry = 0;
#pragma unroll
    for (int w = 0; w < fts::FbCfg<W>::NW; w++) stw(r, w, (uint32_t)fts::fb_next_digit_w<W>(s, carry));
    stw(r, fts::FbCfg<W>::NW, (uint32_t)carry);
  }
};
struct FbDigits16 {  // fb_next_digit, the 16-bit tables' own copy (fb_mul2, fb_mul_acc_jac)
  static constexpr int ni = 1, no = fts::FB_NW + 1;
  static FTS_DEV void run(const uint32_t* a, uint32_t* r, const Aux&, size_t) {
    uint32_t s[8];
#pragma unroll
    for (int q = 0; q < 8; q++) s[q] = a[q];
    int carry = 0;
#pragma unroll
    for (int w = 0; w < fts::FB_NW; w++) stw(r, w, (uint32_t)fts::fb_next_digit(s, carry));
    stw(r, fts::FB_NW, (uint32_t)carry);
  }
};
TOP_W(W, FbSumW, 1, 4, stx(r, fts::fb_sum_w<W>(x.tab, ld<fts::Scalar>(a, 0))););
TOP_W(W, FbMulW, 1, 3, stj(r, fts::fb_mul_w<W>(x.tab, ld<fts::Scalar>(a, 0))););
OP(FbMul2, 2, 3, stj(r, fts::fb_mul2(x.tab, ld<fts::Scalar>(a, 0), x.scr, ld<fts::Scalar>(a, 1))););
OP(FbMulAcc, 4, 3, fts::G1J p = ldj(a, 0); fts::fb_mul_acc(p, x.tab, ld<fts::Scalar>(a, 3)); stj(r, p););
OP(FbMulAccJac, 4, 3, fts::G1J p = ldj(a, 0); fts::fb_mul_acc_jac(p, x.tab, ld<fts::Scalar>(a, 3)); stj(r, p););

// GLV decomposition (glv.hpp): k -> |k1|, s1, |k2|, s2
TOP(K, GlvDec, 1, 4, uint32_t k1[4]; uint32_t k2[4]; uint32_t s1; uint32_t s2; fts::glv_decompose<K>(a, k1, s1, k2, s2);
    st4(r, 0, k1); stw(r, 1, s1); st4(r, 2, k2); stw(r, 3, s2););

// the FP256BN nym kernels' variable-base product (fbn_glv.hpp) over the lane tables of glv_mul
OP(FbnGlvMul, 3, 3, stpj(r, fbn::glv_mul_tab(ld<fbn::Fp>(a, 0), ld<fbn::Fp>(a, 1), a + 16, x.tab, x.n, i)););

// P-256 and FP256BN points (p256.hpp, fp256bn.hpp)
OP(P256Dbl, 3, 3, stpj(r, p256::pj_dbl(ldpj<p256::PJ>(a, 0))););
OP(P256Add, 6, 3, stpj(r, p256::pj_add(ldpj<p256::PJ>(a, 0), ldpj<p256::PJ>(a, 3))););
OP(P256Madd, 5, 3, stpj(r, p256::pj_madd(ldpj<p256::PJ>(a, 0), ld<p256::Fp>(a, 3), ld<p256::Fp>(a, 4))););
OP(P256OnCurve, 2, 1, stw(r, 0, p256::on_curve(ld<p256::Fp>(a, 0), ld<p256::Fp>(a, 1)) ? 1u : 0u););
OP(FbnDbl, 3, 3, stpj(r, fbn::pj_dbl(ldpj<fbn::PJ>(a, 0))););
OP(FbnAdd, 6, 3, stpj(r, fbn::pj_add(ldpj<fbn::PJ>(a, 0), ldpj<fbn::PJ>(a, 3))););
OP(FbnMadd, 5, 3, stpj(r, fbn::pj_madd(ldpj<fbn::PJ>(a, 0), ld<fbn::Fp>(a, 3), ld<fbn::Fp>(a, 4))););
OP(FbnOnCurve, 2, 1, stw(r, 0, fbn::on_curve(ld<fbn::Fp>(a, 0), ld<fbn::Fp>(a, 1)) ? 1u : 0u););

// tower (pairing.hpp) over pair::BnField / pair::FbnField
TOP(B, T2Mul, 4, 2, st2<B>(r, 0, pair::mul(ld2<B>(a, 0), ld2<B>(a, 2))););
TOP(B, T2Sqr, 2, 2, st2<B>(r, 0, pair::sqr(ld2<B>(a, 0))););
TOP(B, T2Inv, 2, 2, st2<B>(r, 0, pair::inv(ld2<B>(a, 0))););
TOP(B, T2MulXi, 2, 2, st2<B>(r, 0, pair::mul_xi(ld2<B>(a, 0))););
TOP(B, T6Mul, 12, 6, st6<B>(r, 0, pair::mul6_i(ld6<B>(a, 0), ld6<B>(a, 6))););
TOP(B, T6Mul01, 10, 6, st6<B>(r, 0, pair::mul01_i(ld6<B>(a, 0), ld2<B>(a, 6), ld2<B>(a, 8))););
TOP(B, T6MulV, 6, 6, st6<B>(r, 0, pair::mul_v(ld6<B>(a, 0))););
TOP(B, T6Inv, 6, 6, st6<B>(r, 0, pair::inv(ld6<B>(a, 0))););
TOP(B, T12Mul, 24, 12, st12<B>(r, 0, pair::mul12_i(ld12<B>(a, 0), ld12<B>(a, 12))););
TOP(B, T12Sqr, 12, 12, st12<B>(r, 0, pair::sqr12_i(ld12<B>(a, 0))););
TOP(B, T12CycSqr, 12, 12, st12<B>(r, 0, pair::cyc_sqr_i(ld12<B>(a, 0))););
TOP(B, T12Inv, 12, 12, st12<B>(r, 0, pair::inv(ld12<B>(a, 0))););
TOP(B, T12Conj, 12, 12, st12<B>(r, 0, pair::conj(ld12<B>(a, 0))););
TOP(B, T12Frob1, 12, 12, st12<B>(r, 0, pair::frob<B, 1>(ld12<B>(a, 0))););
TOP(B, T12Frob2, 12, 12, st12<B>(r, 0, pair::frob<B, 2>(ld12<B>(a, 0))););
TOP(B, T12Frob3, 12, 12, st12<B>(r, 0, pair::frob<B, 3>(ld12<B>(a, 0))););
// f, line (lam, mu: 32 words as precompute_lines stores them), xP, yP
TOP(B, TLineMul, 18, 12, pair::F12<B> f = ld12<B>(a, 0);
    pair::line_mul_i<B>(f, a + 12 * 8, ld<typename B::F>(a, 16), ld<typename B::F>(a, 17)); st12<B>(r, 0, f););

template <class Op>
__global__ void __launch_bounds__(64) k_op(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n, Aux x) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t a[Op::ni * 8], r[Op::no * 8];
#pragma unroll
  for (int q = 0; q < Op::ni * 8; q++) a[q] = in[(size_t)i * Op::ni * 8 + q];
#pragma unroll
  for (int q = 0; q < Op::no * 8; q++) r[q] = 0;
  Op::run(a, r, x, (size_t)i);
#pragma unroll
  for (int q = 0; q < Op::no * 8; q++) out[(size_t)i * Op::no * 8 + q] = r[q];
}
template <class Op>
void launch(const uint32_t* in, uint32_t* out, int n, Aux x) {
  k_op<Op><<<(n + 63) / 64, 64>>>(in, out, n, x);
}

// ------------------------------------------------------------- host: contracts
static const uint32_t* const MODS[6] = {fts::FpP::M, fts::FrP::M, p256::PM::M, p256::NM::M, fbn::PM::M, fbn::RM::M};

static bool lt8(const uint32_t* a, const uint32_t* b) {  // a < b
  for (int i = 7; i >= 0; i--)
    if (a[i] != b[i]) return a[i] < b[i];
  return false;
}
// a + carry * 2^256 < 2 m
static bool lt_2m(const uint32_t* a, uint32_t carry, const uint32_t* m) {
  uint32_t m2[9], a9[9];
  m2[0] = m[0] << 1;
  for (int i = 1; i < 8; i++) m2[i] = (m[i] << 1) | (m[i - 1] >> 31);
  m2[8] = m[7] >> 31;
  memcpy(a9, a, 32);
  a9[8] = carry;
  for (int i = 8; i >= 0; i--)
    if (a9[i] != m2[i]) return a9[i] < m2[i];
  return false;
}
static bool upper_zero(const uint32_t* a, int from) {
  for (int i = from; i < 8; i++)
    if (a[i]) return false;
  return true;
}
// one character per operand word:
//   '0'..'5'  < M of MODS[.]         'a', 'b'  < 2M of MODS[0], MODS[1]
//   'w'       any 256-bit word       'c'       0 or 1
//   'm'       < 2^127
static bool word_ok(char c, const uint32_t* w) {
  if (c >= '0' && c <= '5') return lt8(w, MODS[c - '0']);
  if (c == 'a' || c == 'b') return lt_2m(w, 0, MODS[c - 'a']);
  if (c == 'w') return true;
  if (c == 'c') return w[0] <= 1 && upper_zero(w, 1);
  if (c == 'm') return upper_zero(w, 4) && w[3] < 0x80000000u;
  return false;
}

// BN254 curve membership of Montgomery coordinates (host/bn254_host.hpp): Y^2 = X^3 + 3 Z^6
static fts::host::Fp hfp(const uint32_t* w) {
  fts::host::Fp f;
  for (int i = 0; i < 4; i++) f.v[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
  return f;
}
static bool jac_on_curve(const fts::host::Fp& X, const fts::host::Fp& Y, const fts::host::Fp& Z) {
  using namespace fts::host;
  if (Z.is_zero()) return true;
  const Fp z2 = sqr(Z), z6 = mul(sqr(z2), z2);
  return sqr(Y) == add(mul(sqr(X), X), mul(from_u64<ModP>(3), z6));
}
// affine point: on the curve, or the identity encoding (0, 0)
static bool chk_affine0(const uint32_t* a) {
  const fts::host::Fp X = hfp(a), Y = hfp(a + 8);
  return (X.is_zero() && Y.is_zero()) || jac_on_curve(X, Y, fts::host::Fp::one());
}
static bool chk_jac0(const uint32_t* a) { return jac_on_curve(hfp(a), hfp(a + 8), hfp(a + 16)); }
static bool chk_jac0_jac4(const uint32_t* a) { return chk_jac0(a) && chk_jac0(a + 32); }
static bool chk_aff0_jac2(const uint32_t* a) { return chk_affine0(a) && chk_jac0(a + 16); }
// cond_sub<P>(x, carry): x + carry 2^256 < 2M
template <int MI>
static bool chk_cond_sub(const uint32_t* a) {
  return lt_2m(a, a[8], MODS[MI]);
}

struct Entry {
  const char* name;
  int ni, no;
  const char* spec;              // per-word contract, ni characters
  bool (*check)(const uint32_t*);  // whole-record contract, or null
  bool aux;                      // uses the lane tables
  void (*fn)(const uint32_t*, uint32_t*, int, Aux);
  int fbw = 0, fbt = 0;          // fixed-base op: window width and tables (0: none)
  // a record's words: the ni device operands, then per table and window the entry |d| x y
  int nwords() const { return ni + (fbw ? 3 * ((255 + fbw - 1) / fbw) * fbt : 0); }
};
template <class Op>
static Entry E(const char* name, const char* spec, bool (*check)(const uint32_t*) = nullptr, bool aux = false) {
  return {name, Op::ni, Op::no, spec, check, aux, &launch<Op>};
}

template <class P>
static void bn_field(std::vector<Entry>& c, const char* pfx, char m, char m2) {
  auto nm = [&](const char* s) { return strdup((std::string(pfx) + "_" + s).c_str()); };
  const std::string s1(1, m), s2(2, m), t1(1, m2);
  c.push_back(E<FAdd<P>>(nm("add"), strdup(s2.c_str())));
  c.push_back(E<FSub<P>>(nm("sub"), strdup(s2.c_str())));
  c.push_back(E<FNeg<P>>(nm("neg"), strdup(s1.c_str())));
  c.push_back(E<FDbl<P>>(nm("dbl"), strdup(s1.c_str())));
  c.push_back(E<FMul<P>>(nm("mul"), strdup(s2.c_str())));
  c.push_back(E<FToMont<P>>(nm("to_mont"), strdup(s1.c_str())));
  c.push_back(E<FFromMont<P>>(nm("from_mont"), strdup(s1.c_str())));
  c.push_back(E<FReduceOnce<P>>(nm("reduce_once"), strdup(t1.c_str())));
  c.push_back(E<FLtMod<P>>(nm("lt_mod"), "w"));
}
template <class P, int MI, bool MUL>
static void wide_field(std::vector<Entry>& c, const char* pfx) {
  auto nm = [&](const char* s) { return strdup((std::string(pfx) + "_" + s).c_str()); };
  const std::string s1(1, (char)('0' + MI)), s2(2, (char)('0' + MI));
  c.push_back(E<WAdd<P>>(nm("add"), strdup(s2.c_str())));
  c.push_back(E<WSub<P>>(nm("sub"), strdup(s2.c_str())));
  c.push_back(E<WCondSub<P>>(nm("cond_sub"), "wc", &chk_cond_sub<MI>));
  if constexpr (MUL) {
    c.push_back(E<WMul<P>>(nm("mul"), strdup(s2.c_str())));
    c.push_back(E<WToMont<P>>(nm("to_mont"), strdup(s1.c_str())));
    c.push_back(E<WFromMont<P>>(nm("from_mont"), strdup(s1.c_str())));
    c.push_back(E<WInv<P>>(nm("inv"), strdup(s1.c_str())));
  }
}
template <class B>
static void tower(std::vector<Entry>& c, const char* pfx, char m) {
  auto nm = [&](const char* s) { return strdup((std::string(pfx) + "_" + s).c_str()); };
  auto sp = [&](int n) { return strdup(std::string((size_t)n, m).c_str()); };
  c.push_back(E<T2Mul<B>>(nm("f2_mul"), sp(4)));
  c.push_back(E<T2Sqr<B>>(nm("f2_sqr"), sp(2)));
  c.push_back(E<T2Inv<B>>(nm("f2_inv"), sp(2)));
  c.push_back(E<T2MulXi<B>>(nm("f2_mul_xi"), sp(2)));
  c.push_back(E<T6Mul<B>>(nm("f6_mul"), sp(12)));
  c.push_back(E<T6Mul01<B>>(nm("f6_mul01"), sp(10)));
  c.push_back(E<T6MulV<B>>(nm("f6_mul_v"), sp(6)));
  c.push_back(E<T6Inv<B>>(nm("f6_inv"), sp(6)));
  c.push_back(E<T12Mul<B>>(nm("f12_mul"), sp(24)));
  c.push_back(E<T12Sqr<B>>(nm("f12_sqr"), sp(12)));
  c.push_back(E<T12CycSqr<B>>(nm("f12_cyc_sqr"), sp(12)));
  c.push_back(E<T12Inv<B>>(nm("f12_inv"), sp(12)));
  c.push_back(E<T12Conj<B>>(nm("f12_conj"), sp(12)));
  c.push_back(E<T12Frob1<B>>(nm("f12_frob1"), sp(12)));
  c.push_back(E<T12Frob2<B>>(nm("f12_frob2"), sp(12)));
  c.push_back(E<T12Frob3<B>>(nm("f12_frob3"), sp(12)));
  c.push_back(E<TLineMul<B>>(nm("line_mul"), sp(18)));
}

static std::vector<Entry> catalogue() {
  std::vector<Entry> c;
  // fields: the four full-width moduli share p256.hpp's code; FP256BN's r has no
  // Montgomery constants in fp256bn.hpp (nothing multiplies modulo it), so add/sub/cond_sub only
  bn_field<fts::FpP>(c, "fp", '0', 'a');
  c.push_back(E<FpMulG>("fp_mulg", "00"));
  c.push_back(E<FpInv>("fp_inv", "0"));
  bn_field<fts::FrP>(c, "fr", '1', 'b');
  c.push_back(E<FrMulG>("fr_mulg", "11"));
  c.push_back(E<FrInv>("fr_inv", "1"));
  wide_field<p256::PM, 2, true>(c, "p256p");
  wide_field<p256::NM, 3, true>(c, "p256n");
  wide_field<fbn::PM, 4, true>(c, "fbnp");
  wide_field<fbn::RM, 5, false>(c, "fbnr");
  c.push_back(E<Lt256>("lt256", "ww"));
  // BN254 G1: coordinates < p; the scalar products take points on the curve
  c.push_back(E<JDbl>("g1j_dbl", "000"));
  c.push_back(E<JAddAffine>("g1j_add_affine", "00000"));
  c.push_back(E<JAdd>("g1j_add", "000000"));
  c.push_back(E<MaddInl>("madd_inl", "00000"));
  c.push_back(E<AddInl>("add_inl", "000000"));
  c.push_back(E<JToAffine>("g1j_to_affine", "000"));
  c.push_back(E<JEq>("g1j_eq", "000000"));
  c.push_back(E<XMaddInl>("xmadd_inl", "000000"));
  c.push_back(E<XAddInl>("xadd_inl", "00000000"));
  c.push_back(E<XDbl>("g1x_dbl", "0000"));
  c.push_back(E<XToJac>("g1x_to_jac", "0000"));
  c.push_back(E<VarBaseMul>("var_base_mul", "001", &chk_affine0, true));
  c.push_back(E<GlvMul>("glv_mul", "001", &chk_affine0, true));
  c.push_back(E<Vb128j>("vb128j", "000m", &chk_jac0, true));
  c.push_back(E<Straus2>("straus2_128", "000m000m", &chk_jac0_jac4, true));
  c.push_back(E<GlvDec<fts::Glv>>("glv_decompose_bn", "1"));
  c.push_back(E<GlvDec<fbn::GlvK>>("glv_decompose_fbn", "5"));
  c.push_back(E<P256Dbl>("p256_pj_dbl", "222"));
  c.push_back(E<P256Add>("p256_pj_add", "222222"));
  c.push_back(E<P256Madd>("p256_pj_madd", "22222"));
  c.push_back(E<P256OnCurve>("p256_on_curve", "22"));
  c.push_back(E<FbnDbl>("fbn_pj_dbl", "444"));
  c.push_back(E<FbnAdd>("fbn_pj_add", "444444"));
  c.push_back(E<FbnMadd>("fbn_pj_madd", "44444"));
  c.push_back(E<FbnOnCurve>("fbn_on_curve", "44"));
  tower<pair::BnField>(c, "bn", '0');
  tower<pair::FbnField>(c, "fbn", '4');
  return c;
}
// the com chain's op: run by name like the catalogue's, listed by --list-chain.  It has
// a list of its own only because tests/test_arith_vectors_cpu.py compares `--list` with
// the catalogue tests/arith_vectors.py states, op for op, and that catalogue stays as it is
static std::vector<Entry> chain_ops() {
  std::vector<Entry> c;
  c.push_back(E<Straus4Ctab>("straus4_ctab", "00000mcmcmcmc", &chk_aff0_jac2, true));
  return c;
}

// the FP256BN chain's op, listed by --list-glv, apart for the reason chain_ops gives.  Q on
// the curve is the test's business (there is no host code for this p)
static std::vector<Entry> glv_ops() {
  std::vector<Entry> c;
  c.push_back(E<FbnGlvMul>("fbn_glv_mul", "445", nullptr, true));
  return c;
}

// the fixed-base ops: listed by --list-fb (tests/fixed_base_vectors.py), apart from the
// primitives' catalogue for the reason chain_ops gives.  fb_mul2_same and fb_mul2_neg are
// fb_mul2 under names of their own, so that each has tables of its own (the second a
// table of the first's base, resp. of its negative: the vectors' business)
template <class Op>
static Entry FB(const char* name, const char* spec, int w, int tabs, bool (*check)(const uint32_t*) = nullptr) {
  Entry e = E<Op>(name, spec, check);
  e.fbw = w, e.fbt = tabs;
  return e;
}
static std::vector<Entry> fb_ops() {
  std::vector<Entry> c;
  c.push_back(E<FbDigits16>("fb_digits_16", "1"));
  c.push_back(E<FbDigitsW<16>>("fb_digits_w16", "1"));
  c.push_back(E<FbDigitsW<20>>("fb_digits_20", "1"));
  c.push_back(E<FbDigitsW<22>>("fb_digits_22", "1"));
  c.push_back(FB<FbSumW<16>>("fb_sum_16", "1", 16, 1));
  c.push_back(FB<FbSumW<20>>("fb_sum_20", "1", 20, 1));
  c.push_back(FB<FbSumW<22>>("fb_sum_22", "1", 22, 1));
  c.push_back(FB<FbMulW<16>>("fb_mul_16", "1", 16, 1));
  c.push_back(FB<FbMulW<20>>("fb_mul_20", "1", 20, 1));
  c.push_back(FB<FbMulW<22>>("fb_mul_22", "1", 22, 1));
  c.push_back(FB<FbMul2>("fb_mul2", "11", 16, 2));
  c.push_back(FB<FbMul2>("fb_mul2_same", "11", 16, 2));
  c.push_back(FB<FbMul2>("fb_mul2_neg", "11", 16, 2));
  c.push_back(FB<FbMulAcc>("fb_mul_acc", "0001", 16, 1, &chk_jac0));
  c.push_back(FB<FbMulAccJac>("fb_mul_acc_jac", "0001", 16, 1, &chk_jac0));
  return c;
}

// a sparse fixed-base table on the device: the production size and layout of one base
// (FbCfg<W>::WORDS_PER_BASE) between two guard windows, every byte 0xFF but the entries
// the records supply, so a lookup at any other (window, digit) reads poison -- inside
// the allocation -- and the result differs
struct SparseTable {
  int W, NW;
  size_t E;
  std::map<size_t, std::array<uint32_t, 16>> rows;  // row w * E + |d| - 1
  uint32_t* dev = nullptr;
  explicit SparseTable(int w) : W(w), NW((255 + w - 1) / w), E((size_t)1 << (w - 1)) {}
  // false: another record placed a different point there
  bool put(int w, uint32_t d, const uint32_t* xy) {
    std::array<uint32_t, 16> v;
    memcpy(v.data(), xy, 64);
    auto it = rows.emplace((size_t)w * E + d - 1, v);
    return it.second || it.first->second == v;
  }
  size_t bytes() const { return ((size_t)NW + 2) * E * 64; }
  uint32_t* upload() {  // the table proper starts one window in
    CK(hipMalloc(&dev, bytes()));
    CK(hipMemset(dev, 0xFF, bytes()));
    for (const auto& kv : rows)
      CK(hipMemcpy(dev + (E + kv.first) * 16, kv.second.data(), 64, hipMemcpyHostToDevice));
    return dev + E * 16;
  }
  void release() { CK(hipFree(dev)); }
};

// ------------------------------------------------------------------- host: io
static bool parse_word(const char* s, uint32_t w[8]) {
  const size_t len = strlen(s);
  if (len == 0 || len > 64) return false;
  memset(w, 0, 32);
  for (size_t k = 0; k < len; k++) {
    const char ch = s[len - 1 - k];
    uint32_t d;
    if (ch >= '0' && ch <= '9') d = (uint32_t)(ch - '0');
    else if (ch >= 'a' && ch <= 'f') d = (uint32_t)(ch - 'a' + 10);
    else if (ch >= 'A' && ch <= 'F') d = (uint32_t)(ch - 'A' + 10);
    else return false;
    w[k / 8] |= d << (4 * (k % 8));
  }
  return true;
}

struct Batch {
  std::vector<uint32_t> in;
  std::vector<SparseTable> tabs;  // fixed-base ops: filled from the records' entries
  std::vector<size_t> rec;  // output position of each record
};

int main(int argc, char** argv) {
  std::vector<Entry> cat = catalogue();
  const std::vector<Entry> chain = chain_ops(), fb = fb_ops(), glv = glv_ops();
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const Entry& e : cat) printf("%s %d %d\n", e.name, e.ni, e.no);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "--list-chain")) {
    for (const Entry& e : chain) printf("%s %d %d\n", e.name, e.ni, e.no);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "--list-fb")) {
    for (const Entry& e : fb) printf("%s %d %d\n", e.name, e.nwords(), e.no);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "--list-glv")) {
    for (const Entry& e : glv) printf("%s %d %d\n", e.name, e.ni, e.no);
    return 0;
  }
  cat.insert(cat.end(), chain.begin(), chain.end());
  cat.insert(cat.end(), glv.begin(), glv.end());
  cat.insert(cat.end(), fb.begin(), fb.end());
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT | --list | --list-chain | --list-fb | --list-glv\n", argv[0]);
    return 2;
  }
  FILE* fi = fopen(argv[1], "r");
  if (!fi) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<Batch> batches(cat.size());
  size_t nrec = 0;
  {
    std::vector<char> line(64 * 1024);
    for (size_t ln = 1; fgets(line.data(), (int)line.size(), fi); ln++) {
      char* save = nullptr;
      const char* op = strtok_r(line.data(), " \t\r\n", &save);
      if (!op) continue;
      size_t ei = 0;
      while (ei < cat.size() && strcmp(cat[ei].name, op)) ei++;
      if (ei == cat.size()) {
        fprintf(stderr, "line %zu: unknown op %s\n", ln, op);
        return 2;
      }
      const Entry& e = cat[ei];
      Batch& b = batches[ei];
      const size_t base = b.in.size();
      b.in.resize(base + (size_t)e.ni * 8);
      for (int w = 0; w < e.ni; w++) {
        const char* tok = strtok_r(nullptr, " \t\r\n", &save);
        if (!tok || !parse_word(tok, &b.in[base + (size_t)w * 8])) {
          fprintf(stderr, "line %zu: %s takes %d operand words\n", ln, op, e.ni);
          return 2;
        }
        if (!word_ok(e.spec[w], &b.in[base + (size_t)w * 8])) {
          fprintf(stderr, "line %zu: %s operand %d violates the contract '%c'\n", ln, op, w, e.spec[w]);
          return 2;
        }
      }
      if (e.fbw && b.tabs.empty()) b.tabs.assign((size_t)e.fbt, SparseTable(e.fbw));
      for (SparseTable& t : b.tabs)
        for (int w = 0; w < t.NW; w++) {
          uint32_t ent[24];  // |d| x y: d = 0 with x = y = 0, or 1 <= d <= E with a curve point
          for (int q = 0; q < 3; q++) {
            const char* tok = strtok_r(nullptr, " \t\r\n", &save);
            if (!tok || !parse_word(tok, ent + 8 * q)) {
              fprintf(stderr, "line %zu: %s takes %d words\n", ln, op, e.nwords());
              return 2;
            }
          }
          const bool none = upper_zero(ent, 0) && upper_zero(ent + 8, 0) && upper_zero(ent + 16, 0);
          if (none) continue;
          if (!upper_zero(ent, 1) || ent[0] == 0 || ent[0] > t.E || !word_ok('0', ent + 8) || !word_ok('0', ent + 16) ||
              !jac_on_curve(hfp(ent + 8), hfp(ent + 16), fts::host::Fp::one())) {
            fprintf(stderr, "line %zu: %s window %d: not a table entry\n", ln, op, w);
            return 2;
          }
          if (!t.put(w, ent[0], ent + 8)) {
            fprintf(stderr, "line %zu: %s window %d digit %u: another record placed a different point there\n", ln, op,
                    w, ent[0]);
            return 2;
          }
        }
      if (strtok_r(nullptr, " \t\r\n", &save)) {
        fprintf(stderr, "line %zu: %s takes %d words\n", ln, op, e.nwords());
        return 2;
      }
      if (e.check && !e.check(&b.in[base])) {
        fprintf(stderr, "line %zu: %s record violates the op's contract\n", ln, op);
        return 2;
      }
      b.rec.push_back(nrec++);
    }
  }
  fclose(fi);

  std::vector<std::vector<uint32_t>> results(nrec);
  for (size_t ei = 0; ei < cat.size(); ei++) {
    const Entry& e = cat[ei];
    const Batch& b = batches[ei];
    const size_t n = b.rec.size();
    if (n == 0) continue;
    if (n > (size_t)(1 << 20)) {
      fprintf(stderr, "%s: too many records\n", e.name);
      return 2;
    }
    uint32_t *din = nullptr, *dout = nullptr;
    Aux x{nullptr, nullptr, n};
    const size_t out_words = n * (size_t)e.no * 8;
    CK(hipMalloc(&din, b.in.size() * 4));
    CK(hipMalloc(&dout, out_words * 4));
    if (e.aux) {
      CK(hipMalloc(&x.tab, n * (size_t)fts::CTAB_WORDS * 4));  // >= 16 * 24 words per lane
      CK(hipMalloc(&x.scr, n * 10 * 24 * 4));
    }
    std::vector<SparseTable> tabs = b.tabs;
    if (tabs.size() > 0) x.tab = tabs[0].upload();
    if (tabs.size() > 1) x.scr = tabs[1].upload();
    CK(hipMemcpy(din, b.in.data(), b.in.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dout, 0, out_words * 4));
    e.fn(din, dout, (int)n, x);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> h(out_words);
    CK(hipMemcpy(h.data(), dout, out_words * 4, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; k++)
      results[b.rec[k]].assign(h.begin() + (ptrdiff_t)(k * e.no * 8), h.begin() + (ptrdiff_t)((k + 1) * e.no * 8));
    CK(hipFree(din));
    CK(hipFree(dout));
    if (e.aux) {
      CK(hipFree(x.tab));
      CK(hipFree(x.scr));
    }
    for (SparseTable& t : tabs) t.release();
  }

  FILE* fo = fopen(argv[2], "w");
  if (!fo) {
    fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  for (const std::vector<uint32_t>& r : results) {
    for (size_t w = 0; w * 8 < r.size(); w++) {
      if (w) fputc(' ', fo);
      for (int q = 7; q >= 0; q--) fprintf(fo, "%08x", r[w * 8 + q]);
    }
    fputc('\n', fo);
  }
  if (fclose(fo) != 0) return 2;
  return 0;
}
