// A few rows times a weight matrix on bf16 MFMA (include/amk.h: amk_gemm_rows_bf16):
//     Y (M, N) = X (M, K) . W (N, K)^T + bias,   X and W bf16, bias f32 or NULL, f32 accumulation, Y f32 or bf16.
// Built for M = the batch of a KV-cached decode step (models/transformer.py:22-43 and models/softmax_attention.py:30-44,
// :78-81 for one new row per sequence; models/parti.py:135-152 is the loop): the product is a read of W, so the kernel
// streams W once per block of 16 rows at full width and the rows ride along.
//
//   * rows come in blocks of 16: one v_mfma_f32_16x16x32_bf16 tile holds all rows of a block (A = X, rows past M are exact
//     zeros) against 16 rows of W (B = W^T).  Grid: (ceil(N / 16), ceil(M / 16)), one workgroup of four waves per tile.
//   * the four waves split K: wave w takes the 32-element steps w, w + 4, ...  Lane l of a wave loads the 16 bytes
//     W[n0 + (l & 15)][k + 8 (l >> 4) .. + 8) straight into the VGPRs of its B fragment -- together the waves read 256
//     contiguous bytes of each of the 16 rows per round -- and X[m0 + (l & 15)][the same k] into its A fragment.  Nothing of
//     W goes through LDS.  Two steps are loaded before their MFMAs are issued.
//   * the four partial tiles are added through LDS IN WAVE ORDER, ((t0 + t1) + t2) + t3, then the f32 bias, then the one
//     rounding (to nearest even) where the output is bf16.  No atomics, no split across workgroups.
//   * tails are PREDICATES, not padding: a 16-byte load is issued only where all 8 of its elements lie inside the row's K
//     elements and the row exists; the one piece that straddles K is read element by element up to K and zero-filled; columns
//     n >= N and rows m >= M load nothing and are not stored.  No byte past a row's K elements is read, whatever ldx / ldw hold.
//   * row m of Y depends on row m of X alone: an MFMA accumulates each output element from its own row and column, the step
//     order does not depend on M, and the rows of a block that do not exist contribute zeros to no element but their own.
//     So a row's result is bitwise the same at M = 1 and in any batch.
// The longest addition path of one element: ceil(ceil(K / 32) / 4) MFMAs of 32 products each in a wave, three additions of
// partial tiles and the bias (tests/gemm_rows_bf16_ref.py derives the bound from it).
#include "amk_bf16.h"

namespace amk_rows {

constexpr int WAVES = 4;
constexpr int TILE = 16;
constexpr int KSTEP = 32;

// 8 elements of a row at k .. k + 8: a 16-byte load where they all exist, element loads up to K where the piece
// straddles the end, zeros where the row does not exist or k >= K
__device__ __forceinline__ bf16x8 load8(const __bf16* row, bool row_ok, int k, int K) {
  bf16x8 v = {};
  if (row_ok) {
    if (k + 8 <= K) {
      v = *reinterpret_cast<const bf16x8*>(row + k);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (k + e < K) v[e] = row[k + e];
    }
  }
  return v;
}

template <bool OUT_BF16>
__global__ __launch_bounds__(64 * WAVES) void gemm_rows_bf16_kernel(const __bf16* __restrict__ x, int64_t ldx,
                                                                    const __bf16* __restrict__ w, int64_t ldw,
                                                                    const float* __restrict__ bias, void* __restrict__ y,
                                                                    int64_t ldy, int M, int N, int K) {
  __shared__ float part[WAVES][TILE * TILE];
  const int n0 = blockIdx.x * TILE, m0 = blockIdx.y * TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kq = 8 * (lane >> 4);
  const bool w_ok = n0 + r < N, x_ok = m0 + r < M;
  const __bf16* wrow = w + (int64_t)(w_ok ? n0 + r : 0) * ldw;
  const __bf16* xrow = x + (int64_t)(x_ok ? m0 + r : 0) * ldx;
  const int steps = (K + KSTEP - 1) / KSTEP;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int s = wave;
  for (; s + WAVES < steps; s += 2 * WAVES) {   // two of this wave's steps per trip: four loads in flight
    const int k0 = s * KSTEP + kq, k1 = (s + WAVES) * KSTEP + kq;
    const bf16x8 b0 = load8(wrow, w_ok, k0, K), b1 = load8(wrow, w_ok, k1, K);
    const bf16x8 a0 = load8(xrow, x_ok, k0, K), a1 = load8(xrow, x_ok, k1, K);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc, 0, 0, 0);
  }
  if (s < steps) {
    const int k0 = s * KSTEP + kq;
    const bf16x8 b0 = load8(wrow, w_ok, k0, K);
    const bf16x8 a0 = load8(xrow, x_ok, k0, K);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc, 0, 0, 0);
  }
  // accumulator register i of lane l is the tile's element (row 4 (l >> 4) + i, column l & 15)
#pragma unroll
  for (int i = 0; i < 4; ++i) part[wave][(4 * (lane >> 4) + i) * TILE + r] = acc[i];
  __syncthreads();

  const int row = tid >> 4, col = tid & 15;
  const int m = m0 + row, n = n0 + col;
  if (m < M && n < N) {
    float v = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    if (bias) v += bias[n];
    if (OUT_BF16)
      static_cast<__bf16*>(y)[(int64_t)m * ldy + n] = (__bf16)v;   // the one rounding, to nearest even
    else
      static_cast<float*>(y)[(int64_t)m * ldy + n] = v;
  }
}

}  // namespace amk_rows

using namespace amk_rows;

extern "C" int amk_gemm_rows_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias,
                                  void* y, int64_t ldy, int M, int N, int K, int out_bf16, void* stream) {
  AMK_CHECK_ARG(x && w && y, "amk_gemm_rows_bf16: null pointer");
  AMK_CHECK_ARG(M > 0 && N > 0 && K > 0, "amk_gemm_rows_bf16: bad sizes M=%d N=%d K=%d", M, N, K);
  AMK_CHECK_ARG(ldx >= K && ldw >= K && ldy >= N, "amk_gemm_rows_bf16: a leading dimension is below the row length");
  AMK_CHECK_ARG(ldx % 8 == 0 && ldw % 8 == 0 && ldy % 4 == 0,
                "amk_gemm_rows_bf16: ldx and ldw must be multiples of 8 elements, ldy of 4");
  AMK_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w)) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(y) & (out_bf16 ? 1 : 3)) == 0 && (reinterpret_cast<uintptr_t>(bias) & 3) == 0,
                "amk_gemm_rows_bf16: x and w must be 16-byte aligned (y and bias: to their element)");
  const int64_t nb = ((int64_t)N + TILE - 1) / TILE, mb = ((int64_t)M + TILE - 1) / TILE;
  AMK_CHECK_SUPPORTED(mb <= 65535, "amk_gemm_rows_bf16: M=%d beyond the grid", M);
  const dim3 grid((unsigned)nb, (unsigned)mb);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const __bf16* xp = static_cast<const __bf16*>(x);
  const __bf16* wp = static_cast<const __bf16*>(w);
  if (out_bf16)
    hipLaunchKernelGGL(gemm_rows_bf16_kernel<true>, grid, dim3(64 * WAVES), 0, st, xp, ldx, wp, ldw, bias, y, ldy, M, N, K);
  else
    hipLaunchKernelGGL(gemm_rows_bf16_kernel<false>, grid, dim3(64 * WAVES), 0, st, xp, ldx, wp, ldw, bias, y, ldy, M, N, K);
  AMK_CHECK_LAUNCH("amk_gemm_rows_bf16");
  return AMK_OK;
}
