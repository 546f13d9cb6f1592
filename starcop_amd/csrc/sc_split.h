// The split arithmetic of the 16-bit matrix-core kernels (conv_bx3, conv_sp, conv_spw, conv_pw3, conv_irb, conv_irt): every fp32 MFMA
// operand is split EXACTLY into 16-bit terms while it is staged, and the leading partial products are accumulated in fp32.  This header
// is the single home of the splits, the product chains and the power-of-two range scales; everything is __device__ __forceinline__.
#pragma once
#include "sc_common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float floatx2;
typedef __attribute__((ext_vector_type(4))) unsigned int uintx4;
typedef __attribute__((ext_vector_type(8))) _Float16 halfx8;
typedef __attribute__((ext_vector_type(2))) _Float16 halfx2;

// ---- three bf16 terms ("fp32-x3"; the pointwise, inverted-residual and fused-training kernels) ----
// exact three-term bf16 split of two floats (a = t0 + t1 + t2 up to 2^-24 |a|); returns packed pairs (low half = first value)
__device__ __forceinline__ void split3x2(float a, float b, unsigned& t0, unsigned& t1, unsigned& t2) {
  floatx2 v = {a, b};
  const bf16x2 h0 = __builtin_convertvector(v, bf16x2);
  v -= __builtin_convertvector(h0, floatx2);
  const bf16x2 h1 = __builtin_convertvector(v, bf16x2);
  v -= __builtin_convertvector(h1, floatx2);
  const bf16x2 h2 = __builtin_convertvector(v, bf16x2);
  t0 = __builtin_bit_cast(unsigned, h0);
  t1 = __builtin_bit_cast(unsigned, h1);
  t2 = __builtin_bit_cast(unsigned, h2);
}
__device__ __forceinline__ void split8(const float (&v)[8], uintx4 (&t)[3]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned t0, t1, t2;
    split3x2(v[2 * q], v[2 * q + 1], t0, t1, t2);
    t[0][q] = t0; t[1][q] = t1; t[2][q] = t2;
  }
}
__device__ __forceinline__ floatx16 mfma_bf16(const uintx4& a, const uintx4& b, const floatx16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// the six products of weight >= 2^-24, smallest first
__device__ __forceinline__ floatx16 mfma6(const uintx4 (&a)[3], const uintx4 (&b)[3], floatx16 c) {
  c = mfma_bf16(a[1], b[1], c);
  c = mfma_bf16(a[2], b[0], c);
  c = mfma_bf16(a[0], b[2], c);
  c = mfma_bf16(a[1], b[0], c);
  c = mfma_bf16(a[0], b[1], c);
  c = mfma_bf16(a[0], b[0], c);
  return c;
}

// ---- two fp16 terms ("H" mode, terms code SC_TERMS_F16X2 = 4) ----
// a*s = h0 + h1 exactly to 22 significand bits (round-to-nearest conversions), products h0*g0 + h0*g1 + h1*g0: the dropped
// h1*g1 is 2^-22 |a||b|, below the fp32 accumulation error of a K >= 288 reduction.  fp16 has 5 exponent bits, so every
// operand is brought into range by an exact power-of-two scale that the epilogue divides out again:
//   filters     x 2^8  (|w| < 255; the absolute error 2^-25 of a sub-normal second term is 2^-33 in filter units)
//   activations x 2    (BatchNorm-normalised, ReLU6-clipped or ReLU: |x| < 32752; absolute error floor 2^-26)
//   gradients   x 2^(5-e), 2^e >= the tensor's max |A_c g| from the BatchNorm-backward reduction (args->absmax): the
//               prologue output A g + B y + D is bounded by (2 + max|x_hat|) times that, so anything up to
//               max|x_hat| = 2045 (the most a 4M-sample channel can reach is 2048) fits; error floor 2^-30 of the maximum
// Values beyond the range are clamped to +-65504 (a finite error, never an inf/NaN); the three-term bf16 split
// ("fp32-x3") has fp32's exponent range and no such limits.
constexpr float SC_H_SW = 256.f, SC_H_SX = 2.f, SC_H_MAX = 65504.f;
constexpr float SC_H_XMAX = 32752.f;      // the activation limit: SC_H_SX * SC_H_XMAX = SC_H_MAX
// E0: target exponent, M * s in [2^(E0-1), 2^E0).  Default 5: [16, 32), fallback 1; the 2x2 box sums of conv_spw.hip use 3 (/ 4 for
// the four addends: fallback 0.25).
template <int E0 = 5>
__device__ __forceinline__ float h_grad_scale(const float* absmax) {
  const float M = absmax ? *absmax : 0.f;
  if (!(M > 0.f) || !(M < 3.0e38f)) return ldexpf(1.f, E0 - 5);
  int e;
  (void)frexpf(M, &e);                                  // M = m * 2^e, m in [0.5, 1)
  e = E0 - e;
  e = e < -100 ? -100 : (e > 100 ? 100 : e);
  return ldexpf(1.f, e);                                // M * s in [16, 32) for E0 = 5
}
// Activation operand scale (round 5: range-safe by construction).  xb0 / xb1: device floats >= max |activation| of the staged
// source(s) -- in training the bound |gamma| sqrt(n - 1) + |beta| that sc_bn_finalize leaves per BatchNorm'd tensor (no normalised
// sample of n can exceed sqrt(n - 1)), for residual sums the maximum sc_add_srcs_absmax records in every forward, in inference
// the sticky record of the streamed maxima; NULL: bounded by ReLU6 / unknown -> the default.  The scale is the default 2 whenever
// 2 M <= 32752 (bit-identical to the fixed scale of rounds 1-4) and the largest power of two with s M <= 32752 otherwise.
__device__ __forceinline__ float h_act_scale(const float* xb0, const float* xb1) {
  float M = fmaxf(xb0 ? *xb0 : 0.f, xb1 ? *xb1 : 0.f);
  if (!(M * SC_H_SX > SC_H_XMAX)) return SC_H_SX;
  M = fminf(M, 3.0e38f);
  int e;
  (void)frexpf(SC_H_XMAX / M, &e);                      // 32752 / M = m * 2^e, m in [0.5, 1)  ->  2^(e-1) <= 32752 / M
  e = e - 1 < -120 ? -120 : e - 1;
  return ldexpf(1.f, e);
}
// The operand scale s and (forward sources) the clamp are folded into the prologue constants by the callers: s is a power of
// two, so  clamp(s * min(max(x*sc + sh, lo), hi))  ==  med3(x*(s*sc) + s*sh, max(s*lo, -65504), min(s*hi, 65504))  bit for bit
// (h_lo / h_hi / sc_pro_affine_h), and  s * (A g + B y + D)  ==  (sA) g + (sB) y + sD  -- 3 resp. 1 VALU less per staged value.
__device__ __forceinline__ float h_lo(float lo, float s) { return fmaxf(lo * s, -SC_H_MAX); }
__device__ __forceinline__ float h_hi(float hi, float s) { return fminf(hi * s, SC_H_MAX); }
__device__ __forceinline__ float sc_pro_affine_h(float x, float sc, float sh, float lo, float hi) {
  return __builtin_amdgcn_fmed3f(fmaf(x, sc, sh), lo, hi);
}
// The remainder a - h0 is ONE v_fma_mix_f32 per value (f16 half of the packed first term x -1 + a, the same single rounding as
// convert-back-and-subtract): a pair costs cvt_pk, 2 x fma_mix, cvt_pk instead of cvt_pk, 2 x cvt, (pk_)sub, cvt_pk.  The
// compiler does not form it by itself (it rewrites fma(h, -1, a) into the subtraction), hence the inline assembly.
#ifndef SC_SPLIT_MIX
#define SC_SPLIT_MIX 1
#endif
template <bool CLAMP = true>
__device__ __forceinline__ void split2h(float a, float b, unsigned& t0, unsigned& t1) {
  floatx2 v = {a, b};
  if constexpr (CLAMP) v = floatx2{__builtin_amdgcn_fmed3f(a, -SC_H_MAX, SC_H_MAX), __builtin_amdgcn_fmed3f(b, -SC_H_MAX, SC_H_MAX)};
  const halfx2 h0 = __builtin_convertvector(v, halfx2);
  t0 = __builtin_bit_cast(unsigned, h0);
#if SC_SPLIT_MIX
  float ra, rb;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(ra) : "v"(t0), "v"(v[0]));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rb) : "v"(t0), "v"(v[1]));
  v = floatx2{ra, rb};
#else
  v -= __builtin_convertvector(h0, floatx2);
#endif
  const halfx2 h1 = __builtin_convertvector(v, halfx2);
  t1 = __builtin_bit_cast(unsigned, h1);
}
// The split for the producer waves of k_conv3_ws.  Without the fma_mix form it keeps its remainders scalar: beside the MFMAs
// of the consumer wave on the same SIMD a v_pk_add_f32 costs several issue slots (MI355X_MICROARCH.md: packed f32 VALU is "an
// anti-lever beside MFMAs"; measured -7 % there), while in the single-role kernels, whose staging phases are VALU-bound, the
// packed subtraction was the faster one (weight gradients +3-6 %, thin forward +2-5 % with the scalar form).
template <bool CLAMP = true>
__device__ __forceinline__ void split2h_scalar(float a, float b, unsigned& t0, unsigned& t1) {
#if SC_SPLIT_MIX
  split2h<CLAMP>(a, b, t0, t1);
#else
  if constexpr (CLAMP) {
    a = __builtin_amdgcn_fmed3f(a, -SC_H_MAX, SC_H_MAX);
    b = __builtin_amdgcn_fmed3f(b, -SC_H_MAX, SC_H_MAX);
  }
  const _Float16 ha = (_Float16)a, hb = (_Float16)b;
  const float ra = a - (float)ha, rb = b - (float)hb;
  const _Float16 la = (_Float16)ra, lb = (_Float16)rb;
  t0 = (unsigned)__builtin_bit_cast(unsigned short, ha) | ((unsigned)__builtin_bit_cast(unsigned short, hb) << 16);
  t1 = (unsigned)__builtin_bit_cast(unsigned short, la) | ((unsigned)__builtin_bit_cast(unsigned short, lb) << 16);
#endif
}
// one value, clamped, to two separate halves (the operand writers of conv_spw.hip store 2-byte terms)
__device__ __forceinline__ void split2h_one(float a, unsigned short& h0, unsigned short& h1) {
  a = __builtin_amdgcn_fmed3f(a, -SC_H_MAX, SC_H_MAX);
  const _Float16 t0 = (_Float16)a;
  const _Float16 t1 = (_Float16)(a - (float)t0);
  h0 = __builtin_bit_cast(unsigned short, t0); h1 = __builtin_bit_cast(unsigned short, t1);
}
template <bool HF>
__device__ __forceinline__ floatx16 mfma_split(const bf16x8& a, const bf16x8& b, const floatx16& c) {
  if constexpr (HF) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(halfx8, a), __builtin_bit_cast(halfx8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
