// The gate and the LayerNorm of the transformer FFN under bf16 autocast as one row-wise pass each way
// (models/transformer.py:22-43: Linear(dim, 2 inner) -> gate * gelu(val) -> LayerNorm(inner) -> Linear(inner, dim)).
// The LayerNorm sits between the gate and the second Linear, so the gate cannot ride in a GEMM epilogue (as the SwiGLU
// FFN's does, gemm_bf16.hip); the row is the unit instead:
//   geglu_ln_fwd   ab (M, 2H) bf16 = (val | gate) -> g = gelu(val) * gate in f32 registers (exact erf, as
//                  elementwise.hip:gelu_; never rounded to bf16, never written), two-pass mean / variance of g on the
//                  centred values, y = (g - mean) rstd gamma + beta rounded to bf16 once; mean, rstd f32.
//                  Traffic: one read of ab, one write of y.
//   geglu_ln_bwd   recomputes g and xhat from ab, mean and rstd;  dg = rstd (dy gamma - mean_j(dy gamma)
//                  - xhat mean_j(dy gamma xhat));  d_ab = (dg gate gelu'(val) | dg gelu(val)) rounded to bf16 once;
//                  dgamma / dbeta as f32 partial sums per workgroup, no atomics (the caller sums them in a fixed order).
//                  Traffic: one read of ab and dy, one write of d_ab, plus the partials.
// Structure (ln_mixed_* of mixed_bf16.hip, with 16-byte bf16 loads: 8 elements per lane and chunk): a row belongs to one
// wave up to H = 1024 (4 rows per workgroup) and to the whole workgroup of 4 waves above (the backward at H = 4096 would
// need > 300 registers per lane on one wave); the widths dispatch as
//   H <= 512: 1 chunk, wave   | H <= 1024: 2 chunks, wave   | H <= 2048: 1 chunk, workgroup   | H <= 4096: 2 chunks, workgroup.
// Rows are walked grid-stride.  Loads in the row loop are unconditional: a lane past the row's end reads chunk 0 of the
// same row and its values are zeroed by a select; only the stores are predicated per lane.
// Partials: the backward runs at most 512 workgroups (two per CU) and each writes one (2, H) partial, so at the decoder's
// shape (M 8192, H 4096) the partials are 16.8 MB written + 16.8 MB re-read against 335 MB of ab, dy and d_ab (10 %);
// ln_mixed_bwd's 2048 rows would be 134 MB.
#include "amk_bf16.h"

namespace amk_gln {

constexpr int WAVES = 4;
constexpr int MAX_PARTS = 512;
constexpr int MAX_FWD_GRID = 2048;

__device__ __forceinline__ bf16x8 ldb8(const __bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ void st4_array(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void ld8f(const float* p, float* v) {
  const float4 a = ld4(p), b = ld4(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void stb8(__bf16* p, const float* v) {
  bf16x8 w;
#pragma unroll
  for (int e = 0; e < 8; ++e) w[e] = (__bf16)v[e];
  *reinterpret_cast<bf16x8*>(p) = w;
}
// Sum over the row's threads: the wave's, or the four waves' in a fixed order through `slot` (4 floats of LDS).  The
// callers alternate slots so that one barrier per sum suffices.
template <int WPR>
__device__ __forceinline__ float row_sum(float s, float* slot, int lane, int wave) {
  s = wave_sum(s);
  if (WPR == 1) return s;
  if (lane == 0) slot[wave] = s;
  __syncthreads();
  return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}

// elementwise.hip:gelu_ / gelu_grad_ from one erf
__device__ __forceinline__ float erf_arg_(float x) { return erff(x * 0.70710678118654752f); }
__device__ __forceinline__ float gelu_of_(float x, float e) { return 0.5f * x * (1.f + e); }
__device__ __forceinline__ float gelu_grad_of_(float x, float e) {
  return 0.5f * (1.f + e) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}

// WPR: waves per row (1: a wave per row, 4 rows per workgroup; 4: the workgroup per row).  NCH: 8-element chunks per thread.
template <int NCH, int WPR>
__global__ __launch_bounds__(64 * WAVES) void geglu_ln_fwd_kernel(const __bf16* __restrict__ ab, int64_t lda,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  int64_t M, int H, float eps, __bf16* __restrict__ y,
                                                                  float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  __shared__ float red[2][WAVES];
  constexpr int RPW = WAVES / WPR, T = 64 * WPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = WPR == 1 ? lane : (int)threadIdx.x;
  const int nch = H >> 3;
  int col[NCH];
  bool ok[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = t + T * j;
    ok[j] = c < nch;
    col[j] = ok[j] ? 8 * c : 0;
  }
  const float inv_h = 1.f / (float)H;
  for (int64_t row = (int64_t)blockIdx.x * RPW + (WPR == 1 ? wave : 0); row < M; row += (int64_t)gridDim.x * RPW) {
    const __bf16* a = ab + row * lda;
    float g[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const bf16x8 v = ldb8(a + col[j]), w = ldb8(a + H + col[j]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = (float)v[e];
        const float gv = gelu_of_(x, erf_arg_(x)) * (float)w[e];
        g[j][e] = ok[j] ? gv : 0.f;
        s += g[j][e];
      }
    }
    const float mean = row_sum<WPR>(s, red[0], lane, wave) * inv_h;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        g[j][e] = ok[j] ? g[j][e] - mean : 0.f;
        q += g[j][e] * g[j][e];
      }
    const float rstd = rsqrtf(row_sum<WPR>(q, red[1], lane, wave) * inv_h + eps);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      float gm[8], bt[8], o[8];
      ld8f(gamma + col[j], gm);
      ld8f(beta + col[j], bt);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = g[j][e] * rstd * gm[e] + bt[e];
      if (ok[j]) stb8(y + row * H + col[j], o);
    }
    if (t == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
  }
}

template <int NCH, int WPR>
__global__ __launch_bounds__(64 * WAVES) void geglu_ln_bwd_kernel(const __bf16* __restrict__ ab, int64_t lda, const __bf16* __restrict__ dy,
                                                                  const float* __restrict__ gamma, const float* __restrict__ mean_in,
                                                                  const float* __restrict__ rstd_in, int64_t M, int H,
                                                                  __bf16* __restrict__ d_ab, float* __restrict__ part) {
  __shared__ float red[2][2][WAVES];
  __shared__ __attribute__((aligned(16))) float acc[WPR == 1 ? WAVES * NCH * 512 : 4];  // (WAVES, <= NCH * 512): dgamma then dbeta
  constexpr int RPW = WAVES / WPR, T = 64 * WPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = WPR == 1 ? lane : (int)threadIdx.x;
  const int nch = H >> 3;
  int col[NCH];
  bool ok[NCH];
  float gm[NCH][8], dgm[NCH][8], dbt[NCH][8];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = t + T * j;
    ok[j] = c < nch;
    col[j] = ok[j] ? 8 * c : 0;
    ld8f(gamma + col[j], gm[j]);
#pragma unroll
    for (int e = 0; e < 8; ++e) dgm[j][e] = dbt[j][e] = 0.f;
  }
  const float inv_h = 1.f / (float)H;
  int flip = 0;
  for (int64_t row = (int64_t)blockIdx.x * RPW + (WPR == 1 ? wave : 0); row < M; row += (int64_t)gridDim.x * RPW, flip ^= 1) {
    const __bf16* a = ab + row * lda;
    const float mean = mean_in[row], rstd = rstd_in[row];
    float xh[NCH][8], gy[NCH][8], da[NCH][8], db[NCH][8];   // xhat, dy gamma, gate gelu'(val), gelu(val)
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const bf16x8 v = ldb8(a + col[j]), w = ldb8(a + H + col[j]), d = ldb8(dy + row * H + col[j]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = (float)v[e], gate = (float)w[e];
        const float er = erf_arg_(x);
        const float ge = gelu_of_(x, er);
        const float dyv = ok[j] ? (float)d[e] : 0.f;   // a lane past the end contributes nothing to any sum
        db[j][e] = ge;
        da[j][e] = gate * gelu_grad_of_(x, er);
        xh[j][e] = (ge * gate - mean) * rstd;
        gy[j][e] = dyv * gm[j][e];
        dgm[j][e] += dyv * xh[j][e];
        dbt[j][e] += dyv;
        s1 += gy[j][e];
        s2 += gy[j][e] * xh[j][e];
      }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (WPR > 1) {   // both sums behind one barrier; the slots alternate from row to row
      if (lane == 0) { red[flip][0][wave] = s1; red[flip][1][wave] = s2; }
      __syncthreads();
      s1 = ((red[flip][0][0] + red[flip][0][1]) + red[flip][0][2]) + red[flip][0][3];
      s2 = ((red[flip][1][0] + red[flip][1][1]) + red[flip][1][2]) + red[flip][1][3];
    }
    const float c1 = s1 * inv_h, c2 = s2 * inv_h;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      float o1[8], o2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float dg = rstd * (gy[j][e] - c1 - xh[j][e] * c2);
        o1[e] = dg * da[j][e];
        o2[e] = dg * db[j][e];
      }
      if (ok[j]) {
        stb8(d_ab + row * 2 * H + col[j], o1);
        stb8(d_ab + row * 2 * H + H + col[j], o2);
      }
    }
  }
  float* p = part + (int64_t)blockIdx.x * 2 * H;
  if (WPR > 1) {   // every thread owns its columns
#pragma unroll
    for (int j = 0; j < NCH; ++j)
      if (ok[j]) {
        st4_array(p + col[j], dgm[j]); st4_array(p + col[j] + 4, dgm[j] + 4);
        st4_array(p + H + col[j], dbt[j]); st4_array(p + H + col[j] + 4, dbt[j] + 4);
      }
  } else {         // the four waves hold four rows' worth of the same columns: sum them in wave order
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
      for (int j = 0; j < NCH; ++j)
        if (ok[j]) {
          st4_array(&acc[wave * NCH * 512 + col[j]], pass == 0 ? dgm[j] : dbt[j]);
          st4_array(&acc[wave * NCH * 512 + col[j] + 4], (pass == 0 ? dgm[j] : dbt[j]) + 4);
        }
      __syncthreads();
      for (int i = threadIdx.x; i < H; i += 64 * WAVES) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += acc[w * NCH * 512 + i];
        p[pass * H + i] = s;
      }
      __syncthreads();
    }
  }
}

}  // namespace amk_gln

using namespace amk_gln;

static bool a4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
static int64_t rows_per_wg(int H) { return H <= 1024 ? WAVES : 1; }

#define AMK_GLN_DISPATCH(H_, CALL)                    \
  do {                                                \
    if ((H_) <= 512) { CALL(1, 1); }                  \
    else if ((H_) <= 1024) { CALL(2, 1); }            \
    else if ((H_) <= 2048) { CALL(1, 4); }            \
    else { CALL(2, 4); }                              \
  } while (0)

extern "C" int amk_geglu_ln_bf16_num_partials(int64_t M, int H) {
  if (M <= 0 || H <= 0) return 0;
  const int64_t wg = (M + rows_per_wg(H) - 1) / rows_per_wg(H);
  return (int)(wg < MAX_PARTS ? wg : MAX_PARTS);
}

extern "C" int amk_geglu_ln_bf16_fwd(const void* ab, int64_t ab_stride, int64_t M, int H, const float* gamma, const float* beta,
                                     float eps, void* y, float* mean, float* rstd, void* stream) {
  AMK_CHECK_ARG(ab && gamma && beta && y && mean && rstd, "amk_geglu_ln_bf16_fwd: null pointer");
  AMK_CHECK_ARG(M > 0 && H > 0, "amk_geglu_ln_bf16_fwd: non-positive size");
  AMK_CHECK_SUPPORTED(H % 8 == 0 && H <= 4096, "amk_geglu_ln_bf16_fwd: width %d not supported (multiple of 8, <= 4096)", H);
  AMK_CHECK_ARG(ab_stride >= 2 * (int64_t)H && ab_stride % 8 == 0,
                "amk_geglu_ln_bf16_fwd: ab_stride %lld must be a multiple of 8 and at least 2 H", (long long)ab_stride);
  AMK_CHECK_ARG(a16(ab) && a16(gamma) && a16(beta) && a16(y) && a4(mean) && a4(rstd), "amk_geglu_ln_bf16_fwd: misaligned pointer");
  const int64_t wg = (M + rows_per_wg(H) - 1) / rows_per_wg(H);
  const dim3 grid((unsigned)(wg < MAX_FWD_GRID ? wg : MAX_FWD_GRID)), block(64 * WAVES);
#define CALL(NCH, WPR)                                                                                                   \
  hipLaunchKernelGGL((geglu_ln_fwd_kernel<NCH, WPR>), grid, block, 0, static_cast<hipStream_t>(stream),                  \
                     static_cast<const __bf16*>(ab), ab_stride, gamma, beta, M, H, eps, static_cast<__bf16*>(y), mean, rstd)
  AMK_GLN_DISPATCH(H, CALL);
#undef CALL
  AMK_CHECK_LAUNCH("amk_geglu_ln_bf16_fwd");
  return AMK_OK;
}

extern "C" int amk_geglu_ln_bf16_bwd(const void* ab, int64_t ab_stride, const void* dy, const float* gamma, const float* mean,
                                     const float* rstd, int64_t M, int H, void* d_ab, float* dgb_part, void* stream) {
  AMK_CHECK_ARG(ab && dy && gamma && mean && rstd && d_ab && dgb_part, "amk_geglu_ln_bf16_bwd: null pointer");
  AMK_CHECK_ARG(M > 0 && H > 0, "amk_geglu_ln_bf16_bwd: non-positive size");
  AMK_CHECK_SUPPORTED(H % 8 == 0 && H <= 4096, "amk_geglu_ln_bf16_bwd: width %d not supported (multiple of 8, <= 4096)", H);
  AMK_CHECK_ARG(ab_stride >= 2 * (int64_t)H && ab_stride % 8 == 0,
                "amk_geglu_ln_bf16_bwd: ab_stride %lld must be a multiple of 8 and at least 2 H", (long long)ab_stride);
  AMK_CHECK_ARG(a16(ab) && a16(dy) && a16(gamma) && a4(mean) && a4(rstd) && a16(d_ab) && a16(dgb_part),
                "amk_geglu_ln_bf16_bwd: misaligned pointer");
  const dim3 grid((unsigned)amk_geglu_ln_bf16_num_partials(M, H)), block(64 * WAVES);
#define CALL(NCH, WPR)                                                                                                   \
  hipLaunchKernelGGL((geglu_ln_bwd_kernel<NCH, WPR>), grid, block, 0, static_cast<hipStream_t>(stream),                  \
                     static_cast<const __bf16*>(ab), ab_stride, static_cast<const __bf16*>(dy), gamma, mean, rstd, M, H, \
                     static_cast<__bf16*>(d_ab), dgb_part)
  AMK_GLN_DISPATCH(H, CALL);
#undef CALL
  AMK_CHECK_LAUNCH("amk_geglu_ln_bf16_bwd");
  return AMK_OK;
}
