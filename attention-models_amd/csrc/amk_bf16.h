// bf16 vector types and matrix-pipe helpers shared by the bf16 and the split-bf16 ("bf16x6") kernels (gfx950 only).
#pragma once
#include "amk_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// v_mfma_f32_32x32x16_bf16: D(32x32) += A(32x16) * B(16x32), f32 accumulation.
//   lane l supplies A[l & 31][8 (l >> 5) + (0..7)] and B[8 (l >> 5) + (0..7)][l & 31]; the accumulator as for mfma32.
__device__ __forceinline__ f32x16 mfmab(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// transposing LDS read (ds_read_b64_tr_b16): this lane's 4 elements = one column of a 4-row x 16-column block of 16-bit
// values.  p must be a multiple of 8 bytes.
__device__ __forceinline__ bf16x4 tr_read(const __bf16* p) {
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
  return __builtin_bit_cast(bf16x4, v);
}

// 32x32x16 operand whose contraction index is the ROW of the LDS tile img [row][STRIDE], rows in natural order:
// lane (col = c0 + (l & 31), half) gets rows r0 + 8 half + (0..7)
template <int STRIDE>
__device__ __forceinline__ bf16x8 tr_frag(const __bf16* img, int r0, int c0, int lane) {
  const int hf = lane >> 5, grp = (lane >> 4) & 1, q = (lane & 15) >> 2, pp = lane & 3;
  const __bf16* a = img + (r0 + 8 * hf + q) * STRIDE + c0 + 16 * grp + 4 * pp;
  const bf16x4 lo = tr_read(a), hi = tr_read(a + 4 * STRIDE);
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) { r[i] = lo[i]; r[4 + i] = hi[i]; }
  return r;
}

// The same operand with the rows in PACKED-ACCUMULATOR order, for a product that sums over the rows of a 32x32
// accumulator whose registers 8t .. 8t+7 were packed into the other operand's k-slot t (acc_row order):
// lane (col = c0 + (l & 31), half) gets rows 16 t + 4 half + (0..3) and + 8
template <int STRIDE>
__device__ __forceinline__ bf16x8 tr_frag_packed(const __bf16* img, int t, int c0, int lane) {
  const int hf = lane >> 5, grp = (lane >> 4) & 1, q = (lane & 15) >> 2, pp = lane & 3;
  const __bf16* a = img + (16 * t + 4 * hf + q) * STRIDE + c0 + 16 * grp + 4 * pp;
  const bf16x4 lo = tr_read(a), hi = tr_read(a + 8 * STRIDE);
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) { r[i] = lo[i]; r[4 + i] = hi[i]; }
  return r;
}

// ---- helpers of the bf16 attention kernels (attn_bf16.hip, attn_bf16_hd.hip) -----------------------------------
typedef float f32x4v __attribute__((ext_vector_type(4)));

// a * b - c with two roundings.  HIP contracts a plain a * b - c into one FMA (__fmul_rn / __fsub_rn included: they are
// a * b and a - b), and an FMA leaves the rounding error of c = m * c2 in the exponent -- up to +-64 at the fill value's
// 1.4e9, so a fully masked row lost its uniform weights (and overflowed to NaN over a long row of rescales)
__device__ __forceinline__ float mul_sub_rn(float a, float b, float c) {
#pragma clang fp contract(off)
  return a * b - c;
}
// v_max3_f32 (in files built with -fno-honor-nans -mno-amdgpu-ieee, see the Makefile: no canonicalising v_max in front)
__device__ __forceinline__ float max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }

__device__ __forceinline__ bf16x8 cat4(bf16x4 a, bf16x4 b) {
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) { r[i] = a[i]; r[4 + i] = b[i]; }
  return r;
}
// registers 8t .. 8t+7 of a 32x32 accumulator as the 8 bf16 of a k-slot (the B operand of a product that sums over
// the accumulator's rows)
__device__ __forceinline__ bf16x8 pack8(const f32x16& s, int t) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (__bf16)s[8 * t + j];
  return r;
}

// v_mfma_f32_16x16x32_bf16: D(16x16) += A(16x32) * B(32x16); lane l supplies A[l & 15][8 (l >> 4) + (0..7)] and
// B[8 (l >> 4) + (0..7)][l & 15], accumulator register r of lane l is D[4 (l >> 4) + r][l & 15]
__device__ __forceinline__ f32x4v mfma16(bf16x8 a, bf16x8 b, f32x4v c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// 16x16x32 operand out of an LDS tile X [row][col] by transposing reads, for a product that sums over X's ROWS in
// natural order: lane (col = c0 + (l & 15), kq = l >> 4) gets rows r0 + 8 kq + (0..7)
__device__ __forceinline__ bf16x8 tr_frag16(const __bf16* img, int stride, int r0, int c0, int lane) {
  const int kq = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  const __bf16* a = img + (r0 + 8 * kq + q) * stride + c0 + 4 * pp;
  return cat4(tr_read(a), tr_read(a + 4 * stride));
}

// ---- the split-bf16 contract ------------------------------------------------------------------------------------
// An f32 x is three bf16 parts, x = h + m + l: h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m), every conversion
// round-to-nearest-even and every residual exact in f32 (24 mantissa bits in all).  Planes are indexed 0 = h, 1 = m,
// 2 = l.  A product a * b is six partial products accumulated in f32 SMALLEST FIRST, in this order of (a part, b part):
//   m.m, l.h, h.l, m.h, h.m, h.h     (the terms m.l, l.m and l.l, below 2^-24 of the product, are dropped).
// The error bounds of the x6 tests and the bitwise guarantees (reproducible dq, fixed-order chunk sums) hold for exactly
// this split and this order: every split-bf16 kernel takes both from here.
__device__ __forceinline__ void split1(float x, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)x;
  const float r1 = x - (float)h;
  m = (__bf16)r1;
  l = (__bf16)(r1 - (float)m);
}
__device__ __forceinline__ void split4(const float4& x, bf16x4 (&pl)[3]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    __bf16 h, m, l;
    split1(f4(x, j), h, m, l);
    pl[0][j] = h; pl[1][j] = m; pl[2][j] = l;
  }
}
// x[o] .. x[o + 7] of an array or a vector (o = 8 t: registers 8t .. 8t+7 of a 32x32 accumulator as the three planes of
// k-slot t, the B operand of a product that sums over the accumulator's rows)
template <class X>
__device__ __forceinline__ void split8(const X& x, int o, bf16x8 (&pl)[3]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 h, m, l;
    split1(x[o + j], h, m, l);
    pl[0][j] = h; pl[1][j] = m; pl[2][j] = l;
  }
}
// planes of the A and of the B operand in partial product q = 0..5
__device__ constexpr int x6_pa(int q) { constexpr int t[6] = {1, 2, 0, 1, 0, 0}; return t[q]; }
__device__ constexpr int x6_pb(int q) { constexpr int t[6] = {1, 0, 2, 0, 1, 0}; return t[q]; }

__device__ __forceinline__ f32x16 mfma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16 c) {
#pragma unroll
  for (int q = 0; q < 6; ++q) c = mfmab(a[x6_pa(q)], b[x6_pb(q)], c);
  return c;
}
// two independent products, c0 += a0 b0 and c1 += a1 b1 (which may share an operand), their MFMAs alternating so that
// no MFMA waits on its predecessor
__device__ __forceinline__ void mfma6x2(const bf16x8 (&a0)[3], const bf16x8 (&b0)[3], f32x16& c0,
                                        const bf16x8 (&a1)[3], const bf16x8 (&b1)[3], f32x16& c1) {
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    c0 = mfmab(a0[x6_pa(q)], b0[x6_pb(q)], c0);
    c1 = mfmab(a1[x6_pa(q)], b1[x6_pb(q)], c1);
  }
}
