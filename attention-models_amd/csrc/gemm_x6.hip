// C (M, N) = A (M, K) B (N, K)^T (+ bias[N]) for f32 operands with SPLIT-BF16 products ("bf16x6").
//
// The projection / FFN GEMMs of the ViT-VQGAN step (x W^T of every nn.Linear, and dY W for its input
// gradient with W pre-transposed) are 36 % of the step on the vendor library's exact-f32 path, which
// already runs at 0.79 of the f32 MFMA peak: an exact-f32 kernel of our own cannot win there (SURVEY.md
// section 8f rank 1).  What can: every f32 operand x is split into three bf16 parts x = h + m + l
// (24 mantissa bits) and a product is the sum of six exact partial products accumulated in f32 by
// v_mfma_f32_32x32x16_bf16 -- the scheme of attn_fwd_x6.hip, with the same measured f32-level error
// (tools/ubench_bf16x6.hip) -- at 6 / 16 of the f32 MFMA's matrix-pipe time.  Its roofline is the bf16
// MFMA peak / 6 (417 TFLOP/s), NOT the 157.3 TFLOP/s f32 peak; bench.py reports it as a variant.
//
// B is the WEIGHT: small and shared by every row tile, so it is split ONCE per call (or once per optimizer
// step, split_table_kernel) into three bf16 planes ([plane][row][K rounded up to 32], zero padded) and the
// GEMM streams those; A (the activations) is split inside the GEMM.  Two kernels share the arithmetic -- one
// f32 accumulator per output element, k-blocks of 16 in ascending order, the six products in the order of
// x6_pa / x6_pb, then the epilogue -- and so agree bit for bit:
//
// gemm_x6_nt_kernel (every K, two contraction segments, the gate's backward): one workgroup per 128 x 128
// output tile, 8 waves as 2 (m) x 4 (n), each 64 x 32 = two MFMA tiles; K in steps of 32; two workgroups per
// CU.  A is split on the fly between its global load and its LDS store, by EVERY column tile of a row block.
// LDS: three bf16 planes per operand, [row][32 k] with 80-byte rows (conflict-free 16-byte fragment reads),
// 60 KB.  The loads of step k+1 are in flight under the MFMAs of step k.  125-168 TFLOP/s = 0.30-0.40 of the
// bf16x6 bound at the ViT-VQGAN shapes (tools/kbench_gemm.py).  Three other structures were built and
// measured within 8 % of it: 4 waves x (64 x 64) with both operands split on the fly; a 256 x 128 tile with
// the split hoisted out of the barrier window; two LDS stages with one barrier per step.  At K = 256 a
// workgroup lives for eight steps and its cost is per tile (the split, the prologue, the epilogue), not in
// the K loop.
//
// gemm_x6_short_k_kernel (K <= 256, one segment, PLAIN and GATE; taken by x6_launch unless
// amk_gemm_x6_short_k(0)): the row block owns the contraction.  A workgroup of 4 waves loads its 128 rows
// of A once, splits them once and keeps the planes in registers as MFMA fragments for the whole K; it then
// walks every column tile of the row block streaming only the weight planes through a double-buffered LDS
// stage, and a tile's stores drain under the next tile's MFMAs.  Details at the kernel.
#include <atomic>

#include "amk_bf16.h"

namespace amk_gemm {

constexpr int BM = 128, BN = 128, BK = 32, NTHR = 512;
constexpr int RS = BK + 8;            // bf16 per LDS row: 80 bytes
constexpr int PLANE = 128 * RS;       // one plane of a 128-row tile

// planes[p][r][kp] = part p of W[r][k] (k < K), 0 for K <= kp < Kp
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ W, int64_t ldw, int R, int K, int Kp,
                                                           __bf16* __restrict__ planes) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one thread per 4 consecutive k
  const int kq = Kp / 4;
  if (i >= (int64_t)R * kq) return;
  const int r = (int)(i / kq), k = (int)(i % kq) * 4;
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
  if (k < K) x = *reinterpret_cast<const float4*>(W + (int64_t)r * ldw + k);  // K % 4 == 0
  bf16x4 pl[3];
  split4(x, pl);
#pragma unroll
  for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x4*>(planes + ((int64_t)p * R + r) * Kp + k) = pl[p];
}

enum { X6_PLAIN = 0, X6_GATE = 1, X6_GATE_BWD = 2 };

struct Args {
  const float *A, *A2, *bias, *AB;
  const __bf16 *Bp, *Bp2;   // [3][NR][Kp] (and [3][NR][Kp2] against A2)
  float *C, *G;
  int M, N, K, Kp, K2, Kp2, NR;
  int64_t lda, lda2, ldc, ldg, ldab;
};

// EPI: X6_PLAIN     C = A B^T (+ bias)
//      X6_GATE      B = w12 in the gate order (plane rows 128 t + j: column 64 t + j of a for j < 64, of b for j >= 64,
//                   zero rows past H); a tile is 128 rows x 64 gate columns, 8 waves as 4 (m) x 2 (n), and a wave's two
//                   MFMA tiles are the a and the b columns of the SAME 32 gate columns: the pair meets in one lane.
//                   G = silu(a) b with the bias added; (a | b) goes to C only when C is given.
//      X6_GATE_BWD  N = H, the product is dGate; reads (a | b) from AB, writes (dA | dB) to C.
// TWO: the contraction runs over (A, Bp) and then (A2, Bp2): dX = dq Wq + dkv Wkv in one launch.
template <int EPI, bool TWO>
__global__ __launch_bounds__(NTHR, 4) void gemm_x6_nt_kernel(Args g) {
  constexpr bool GATE = EPI == X6_GATE;
  constexpr int TN = GATE ? 64 : BN;   // output columns of a tile (its plane rows are always 128)
  __shared__ __attribute__((aligned(16))) __bf16 Ap[3 * PLANE];
  __shared__ __attribute__((aligned(16))) __bf16 Bs[3 * PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  // PLAIN: 2 x 4 waves, rows 64 wm .., columns 32 wn ..; GATE: 4 x 2 waves, rows 32 wm .., gate columns 32 wn ..
  const int wm = GATE ? wave >> 1 : wave >> 2, wn = GATE ? wave & 1 : wave & 3;
  // tiles: consecutive logical ids walk the N tiles of one M tile (they share the A rows): one XCD
  const int ntn = (g.N + TN - 1) / TN;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (wg / ntn) * BM, n0 = (wg % ntn) * TN, p0 = (wg % ntn) * BN;

  // A staging: thread -> rows ar + 64 j (j < 2), 4 floats at column ac
  const int ar = tid >> 3, ac = (tid & 7) * 4;
  const __amdgpu_buffer_rsrc_t a_rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)g.A, 0, (int)(((int64_t)(g.M - 1) * g.lda + g.K) * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t a2_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(TWO ? g.A2 : g.A), 0, TWO ? (int)(((int64_t)(g.M - 1) * g.lda2 + g.K2) * 4) : 0, 0x00020000);
  int aoff[2], aoff2[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ra = m0 + ar + 64 * j;
    aoff[j] = ra < g.M ? (int)(((int64_t)ra * g.lda + ac) * 4) : 0x7ffffff0;  // past the buffer: zeros
    aoff2[j] = TWO && ra < g.M ? (int)(((int64_t)ra * g.lda2 + ac) * 4) : 0x7ffffff0;
  }
  // B staging: 3 planes x 128 rows x 4 pieces of 16 B: plane p, row tid / 4, piece tid % 4
  const int br = tid >> 2, bc = (tid & 3) * 8;
  const __amdgpu_buffer_rsrc_t b_rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)g.Bp, 0, (int)((int64_t)3 * g.NR * g.Kp * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t b2_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(TWO ? g.Bp2 : g.Bp), 0, TWO ? (int)((int64_t)3 * g.NR * g.Kp2 * 2) : 0, 0x00020000);
  int boff[3], boff2[3];
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    boff[p] = p0 + br < g.NR ? (int)((((int64_t)p * g.NR + p0 + br) * g.Kp + bc) * 2) : 0x7ffffff0;
    boff2[p] = TWO && p0 + br < g.NR ? (int)((((int64_t)p * g.NR + p0 + br) * g.Kp2 + bc) * 2) : 0x7ffffff0;
  }

  const int nk1 = (g.K + BK - 1) / BK;
  const int nk = nk1 + (TWO ? (g.K2 + BK - 1) / BK : 0);
  float4 ast[2];
  uint4 bst[3];
  auto prefetch = [&](int kt) {
    if (TWO && kt >= nk1) {
      const int k0 = (kt - nk1) * BK;
      const bool kin = k0 + ac < g.K2;
#pragma unroll
      for (int j = 0; j < 2; ++j)
        ast[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(a2_rsrc, kin ? aoff2[j] + k0 * 4 : 0x7ffffff0, 0, 0));
#pragma unroll
      for (int p = 0; p < 3; ++p)
        bst[p] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(b2_rsrc, boff2[p] + k0 * 2, 0, 0));
    } else {
      const int k0 = kt * BK;
      const bool kin = k0 + ac < g.K;  // columns past K (the last, partial step) must read zeros, not the next row
#pragma unroll
      for (int j = 0; j < 2; ++j)
        ast[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, kin ? aoff[j] + k0 * 4 : 0x7ffffff0, 0, 0));
#pragma unroll
      for (int p = 0; p < 3; ++p)
        bst[p] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, boff[p] + k0 * 2, 0, 0));  // Kp is padded
    }
  };
  auto commit = [&]() {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bf16x4 pa[3];
      split4(ast[j], pa);
#pragma unroll
      for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x4*>(&Ap[p * PLANE + (ar + 64 * j) * RS + ac]) = pa[p];
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4*>(&Bs[p * PLANE + br * RS + bc]) = bst[p];
  };

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[i][t] = 0.f;

  prefetch(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();  // every wave is done with the previous tile's fragments
    commit();
    __syncthreads();
    prefetch(min(kt + 1, nk - 1));      // unconditional (the last step re-reads its own tile, unused)
    __builtin_amdgcn_sched_barrier(0);  // issued HERE, under the MFMAs below (the compiler sinks them otherwise)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      // six partial products per output tile, smallest first; the two tiles' chains interleave
      if constexpr (GATE) {
        bf16x8 a[3], b[2][3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          a[p] = *reinterpret_cast<const bf16x8*>(&Ap[p * PLANE + (32 * wm + r) * RS + 16 * s + 8 * h]);
#pragma unroll
          for (int i = 0; i < 2; ++i)
            b[i][p] = *reinterpret_cast<const bf16x8*>(&Bs[p * PLANE + (64 * i + 32 * wn + r) * RS + 16 * s + 8 * h]);
        }
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
          for (int i = 0; i < 2; ++i) acc[i] = mfmab(a[x6_pa(q)], b[i][x6_pb(q)], acc[i]);
      } else {
        bf16x8 a[2][3], b[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          b[p] = *reinterpret_cast<const bf16x8*>(&Bs[p * PLANE + (32 * wn + r) * RS + 16 * s + 8 * h]);
#pragma unroll
          for (int i = 0; i < 2; ++i)
            a[i][p] = *reinterpret_cast<const bf16x8*>(&Ap[p * PLANE + (64 * wm + 32 * i + r) * RS + 16 * s + 8 * h]);
        }
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
          for (int i = 0; i < 2; ++i) acc[i] = mfmab(a[i][x6_pa(q)], b[x6_pb(q)], acc[i]);
      }
    }
  }
  const int n = n0 + 32 * wn + r;
  if (n >= g.N) return;
  if constexpr (GATE) {
    // register t of lane (r, h): a (acc[0]) and b (acc[1]) of row m0 + 32 wm + acc_row(t, h), gate column n
    const float ba = g.bias ? g.bias[n] : 0.f, bb = g.bias ? g.bias[g.N + n] : 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int m = m0 + 32 * wm + acc_row(t, h);
      if (m < g.M) {
        const float av = acc[0][t] + ba, bv = acc[1][t] + bb;
        g.G[(int64_t)m * g.ldg + n] = av * sigmoidf_(av) * bv;
        if (g.C) { g.C[(int64_t)m * g.ldc + n] = av; g.C[(int64_t)m * g.ldc + g.N + n] = bv; }
      }
    }
  } else {
    // register t of lane (r, h) is C[m0 + 64 wm + 32 i + acc_row(t, h)][n0 + 32 wn + r]
    const float bv = (EPI == X6_PLAIN && g.bias) ? g.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int m = m0 + 64 * wm + 32 * i + acc_row(t, h);
        if (m < g.M) {
          if constexpr (EPI == X6_GATE_BWD) {
            const float dg = acc[i][t], a_ = g.AB[(int64_t)m * g.ldab + n], b_ = g.AB[(int64_t)m * g.ldab + g.N + n];
            const float sg = sigmoidf_(a_);
            g.C[(int64_t)m * g.ldc + n] = dg * b_ * (sg * (1.f + a_ * (1.f - sg)));
            g.C[(int64_t)m * g.ldc + g.N + n] = dg * (a_ * sg);
          } else {
            g.C[(int64_t)m * g.ldc + n] = acc[i][t] + bv;
          }
        }
      }
  }
}

// ---- the short-K kernel: the whole contraction (K <= 256) of a row block stays in registers.
// Workgroup: 4 waves, one per SIMD, 128 rows; wave w owns rows 32 w .. 32 w + 31 and holds their three planes as MFMA
// A fragments for all 16 k-blocks (192 registers), loaded and split ONCE.  The workgroup then walks every column tile of
// its row block -- 64 plane rows: 64 output columns (PLAIN), or the a and the b rows of 32 gate columns (GATE) -- in
// stages of 64 k: the weight planes of stage s + 2 are in flight to registers and those of stage s + 1 go to the other
// LDS buffer while the MFMAs of stage s run, with one LDS-only barrier per stage (48 MFMAs per wave).  The stores of a
// tile are issued in the first stage of the next tile, behind that stage's loads, and drain under its products (neither
// the barrier nor the wait for the next planes waits for them).
// PLAIN walks the tiles of a second weight (Bp2 -> C2, no bias) behind those of the first: q | kv in one launch.
// Every output element is one accumulator that takes its k-blocks in ascending order and the six products in the order
// of x6_pa / x6_pb, then the epilogue arithmetic of gemm_x6_nt_kernel: the two kernels agree bit for bit.
constexpr int SK_THR = 256, SK_BM = 128, SK_KC = 64, SK_ROWS = 64, SK_MAXK = 256;
constexpr int SK_RS = SK_KC + 8;             // bf16 per LDS row: 144 bytes (conflict-free 16-byte fragment reads)
constexpr int SK_PLANE = SK_ROWS * SK_RS;    // one plane of a stage
constexpr int SK_STAGE = 3 * SK_PLANE;

struct SkArgs {
  const float *A, *bias;
  const __bf16 *Bp, *Bp2;    // [3][NR][Kp], [3][NR2][Kp]
  float *C, *C2, *G;
  int M, K, Kp, N, N2, NR, NR2, nt1, ntiles;
  int64_t lda, ldc, ldc2, ldg;
};

// FULL: Kp == 256 (every k-block and every stage exists: no guards in the stage loop)
// KEEP (GATE): (a | b) is written to C
template <int EPI, bool FULL, bool KEEP>
__global__ __launch_bounds__(SK_THR) void gemm_x6_short_k_kernel(SkArgs g) {
  constexpr bool GATE = EPI == X6_GATE;
  __shared__ __attribute__((aligned(16))) __bf16 Bs[2 * SK_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * SK_BM;
  const int nkb = FULL ? 16 : g.Kp / 16, nst = FULL ? 4 : (nkb + 3) / 4;   // Kp is a multiple of 32: nkb is even
  const int S = g.ntiles * nst;

  // B staging: a stage is 3 planes x 64 rows x 8 pieces of 16 B; thread -> rows tid / 8 and + 32, piece tid % 8
  const int srow = tid >> 3, spc = (tid & 7) * 8;
  const __amdgpu_buffer_rsrc_t b_rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)g.Bp, 0, (int)((int64_t)3 * g.NR * g.Kp * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t b2_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(g.Bp2 ? g.Bp2 : g.Bp), 0, g.Bp2 ? (int)((int64_t)3 * g.NR2 * g.Kp * 2) : 0, 0x00020000);
  uint4 bst[6];
  int pt = 0, pc = 0;   // the stage the next prefetch() loads: tile pt, k chunk pc
  auto prefetch = [&]() {
    if (pt < g.ntiles) {
      const bool second = !GATE && pt >= g.nt1;
      const int tl = second ? pt - g.nt1 : pt, NR = second ? g.NR2 : g.NR;
      const int k = SK_KC * pc + spc;
      int off[6];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int prow = GATE ? 128 * (tl >> 1) + 32 * (tl & 1) + 64 * jj + srow : 64 * tl + 32 * jj + srow;
        const bool ok = prow < NR && k < g.Kp;   // rows past the planes, chunks past Kp: zeros
#pragma unroll
        for (int p = 0; p < 3; ++p) off[2 * p + jj] = ok ? (int)((((int64_t)p * NR + prow) * g.Kp + k) * 2) : 0x7ffffff0;
      }
      if (second) {
#pragma unroll
        for (int i = 0; i < 6; ++i) bst[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(b2_rsrc, off[i], 0, 0));
      } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) bst[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, off[i], 0, 0));
      }
    }
    if (++pc == nst) { pc = 0; ++pt; }
  };
  auto commit = [&](int par) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
        *reinterpret_cast<uint4*>(&Bs[par * SK_STAGE + p * SK_PLANE + (32 * jj + srow) * SK_RS + spc]) = bst[2 * p + jj];
  };

  prefetch();   // stage 0, in flight under the A loads

  // the row block's A: lane (r, h) holds A[m0 + 32 wave + r][16 kb + 8 h + (0..7)] of every k-block, split once
  bf16x8 a[16][3];
  {
    const __amdgpu_buffer_rsrc_t a_rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void*)g.A, 0, (int)(((int64_t)(g.M - 1) * g.lda + g.K) * 4), 0x00020000);
    const int row = m0 + 32 * wave + r;
    const bool rin = row < g.M;
    const int abase = rin ? (int)(((int64_t)row * g.lda + 8 * h) * 4) : 0;
#pragma unroll
    for (int kb = 0; kb < 16; ++kb) {
      bf16x4 lo[3], hi[3];
      const int col = 16 * kb + 8 * h;   // columns past K (and rows past M) read zeros
      const float4 x0 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, rin && col < g.K ? abase + 64 * kb : 0x7ffffff0, 0, 0));
      const float4 x1 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, rin && col + 4 < g.K ? abase + 64 * kb + 16 : 0x7ffffff0, 0, 0));
      split4(x0, lo);
      split4(x1, hi);
#pragma unroll
      for (int p = 0; p < 3; ++p) a[kb][p] = cat4(lo[p], hi[p]);
    }
  }

  commit(0);
  prefetch();   // stage 1
  lds_barrier();

  // Outputs and bias go through buffer resources: a column past N, a row past M (beyond the resource's range: the host
  // checks that the offsets fit) and "no tile" are offsets out of range, which the hardware drops or reads as 0.  So the
  // stage loop has NO branch around a load or a store, and the compiler's s_waitcnt vmcnt(n) counts exactly: the wait for
  // the next stage's planes leaves the younger stores in flight (behind a branch it would have to assume none were issued).
  const auto out_rsrc = [&](float* p, int64_t ld, int width) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, p ? (int)(((int64_t)(g.M - 1) * ld + width) * 4) : 0, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t c_rsrc = out_rsrc(g.C, g.ldc, GATE ? 2 * g.N : g.N);
  const __amdgpu_buffer_rsrc_t c2_rsrc = out_rsrc(GATE ? g.G : g.C2, GATE ? g.ldg : g.ldc2, GATE ? g.N : g.N2);   // GATE: the gate
  const __amdgpu_buffer_rsrc_t bias_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(g.bias ? g.bias : g.A), 0, g.bias ? (GATE ? 2 * g.N : g.N) * 4 : 0, 0x00020000);
  const int mrow = m0 + 32 * wave + 4 * h;   // register e of lane (r, h): row mrow + (e & 3) + 8 (e >> 2)
  auto st = [&](__amdgpu_buffer_rsrc_t rs, int off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs, off, 0, 0);
  };

  // a finished tile: its accumulators and its bias, stored under the first stage of the NEXT tile (t < 0: nothing)
  f32x16 out[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) out[i][e] = 0.f;
  float ob0 = 0.f, ob1 = 0.f;
  auto store_tile = [&](int t) {
    const bool second = !GATE && t >= g.nt1;
    const int tl = second ? t - g.nt1 : t;
    const int Nt = second ? g.N2 : g.N;
    const int n = GATE ? 32 * tl + r : 64 * tl + r;
    if constexpr (GATE) {
      const bool ok = t >= 0 && n < Nt;
      const int goff = ok ? (int)(((int64_t)mrow * g.ldg + n) * 4) : 0x7ffffff0, gstep = (int)g.ldg * 4;
      const int coff = ok ? (int)(((int64_t)mrow * g.ldc + n) * 4) : 0x7ffffff0, cstep = (int)g.ldc * 4;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int re = (e & 3) + 8 * (e >> 2);
        const float av = out[0][e] + ob0, bv = out[1][e] + ob1;
        st(c2_rsrc, goff + re * gstep, av * sigmoidf_(av) * bv);
        if constexpr (KEEP) {
          st(c_rsrc, coff + re * cstep, av);
          st(c_rsrc, coff + re * cstep + Nt * 4, bv);
        }
      }
    } else {
      const int64_t ldt = second ? g.ldc2 : g.ldc;
      const int step = (int)ldt * 4;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int off = t >= 0 && n + 32 * i < Nt ? (int)(((int64_t)mrow * ldt + n + 32 * i) * 4) : 0x7ffffff0;
        const float bv = i ? ob1 : ob0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int re = (e & 3) + 8 * (e >> 2);
          if (second) st(c2_rsrc, off + re * step, out[i][e] + bv);   // (a uniform choice of the resource, both arms store)
          else st(c_rsrc, off + re * step, out[i][e] + bv);
        }
      }
    }
  };

  f32x16 acc[2];
  float b0 = 0.f, b1 = 0.f;   // GATE: the bias of a and of b; PLAIN: of columns n and n + 32
  int par = 0, s = 0;
  for (int t = 0; t < g.ntiles; ++t) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (FULL || c < nst) {
        if (s + 1 < S) commit(par ^ 1);   // stage s + 1: its buffer was last read before the previous barrier
        prefetch();                       // stage s + 2
        __builtin_amdgcn_sched_barrier(0);   // issued HERE, under the MFMAs below
        if (c == 0) {
          // this tile's bias (used when the tile is stored), then the previous tile's stores: all BEHIND this stage's
          // loads, so that the next stage waits for the loads alone; they drain under this tile's MFMAs
          const bool second = !GATE && t >= g.nt1;
          const int n = GATE ? 32 * t + r : 64 * t + r;
          const int N1 = g.N;
          b0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(bias_rsrc, !second && n < N1 ? n * 4 : 0x7ffffff0, 0, 0));
          b1 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                             bias_rsrc, GATE ? (n < N1 ? (N1 + n) * 4 : 0x7ffffff0) : (!second && n + 32 < N1 ? (n + 32) * 4 : 0x7ffffff0), 0, 0));
          store_tile(t - 1);
        }
        const __bf16* bs = Bs + par * SK_STAGE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (FULL || 4 * c + j < nkb) {
            bf16x8 b[2][3];
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
              for (int i = 0; i < 2; ++i)
                b[i][p] = *reinterpret_cast<const bf16x8*>(&bs[p * SK_PLANE + (32 * i + r) * SK_RS + 16 * j + 8 * h]);
#pragma unroll
            for (int q = 0; q < 6; ++q)
#pragma unroll
              for (int i = 0; i < 2; ++i) acc[i] = mfmab(a[4 * c + j][x6_pa(q)], b[i][x6_pb(q)], acc[i]);
          }
        }
        if (FULL ? c == 3 : c == nst - 1) {
          out[0] = acc[0];
          out[1] = acc[1];
          ob0 = b0;
          ob1 = b1;
        }
        lds_barrier();   // LDS only: stores and the loads of stage s + 2 stay in flight
        par ^= 1;
        ++s;
      }
    }
  }
  store_tile(g.ntiles - 1);
}

// ---- the plane shadow: every weight of a flat parameter buffer split in ONE launch, driven by a table.
// Entry e (SPLIT_ENT int64 each): {src, R, K, H, blk0, dst_w, dst_wt, NR}: W = flat + src is (R, K) row-major;
// its planes go to planes + dst_w as [3][NR][K padded to 32] -- row r of W at plane row r (H == 0), or in the gate
// order of X6_GATE (H > 0, R == 2 H) -- and the planes of W^T to planes + dst_wt as [3][K][R padded to 32] (dst_wt
// < 0: none).  Workgroups blk0 .. of the grid own the 32 x 32 tiles of W, row tiles outermost; the transposed planes
// go through an LDS tile.  Rows and columns of padding inside a tile are written as zeros; plane rows no tile owns
// (the gate order's rows past H) are never written: the buffer is allocated zeroed.
constexpr int SPLIT_ENT = 8;

__global__ __launch_bounds__(256) void split_table_kernel(const float* __restrict__ flat, int64_t flat_elems,
                                                          const int64_t* __restrict__ table, int n_ent,
                                                          __bf16* __restrict__ planes, int64_t planes_elems) {
  __shared__ __bf16 T[3][32][36];
  const int tid = threadIdx.x;
  int e = 0;
  while (e + 1 < n_ent && (int64_t)blockIdx.x >= table[(e + 1) * SPLIT_ENT + 4]) ++e;
  const int64_t* t = table + e * SPLIT_ENT;
  const int64_t src = t[0], dst_w = t[5], dst_wt = t[6];
  const int R = (int)t[1], K = (int)t[2], H = (int)t[3], NR = (int)t[7];
  const int Kp = (K + 31) / 32 * 32, Rp = (R + 31) / 32 * 32, tk_n = Kp / 32;
  const int tile = (int)((int64_t)blockIdx.x - t[4]);
  const int tr = tile / tk_n, tk = tile - tr * tk_n;
  // a table that does not fit its buffers writes nothing (uniform per workgroup)
  if (tile < 0 || tr >= Rp / 32 || src < 0 || src + (int64_t)R * K > flat_elems || dst_w < 0 ||
      dst_w + (int64_t)3 * NR * Kp > planes_elems || (dst_wt >= 0 && dst_wt + (int64_t)3 * K * Rp > planes_elems) ||
      (H > 0 ? (R != 2 * H || NR < (H + 63) / 64 * 128) : NR < R))
    return;
  const int lr = tid >> 3, lc = (tid & 7) * 4;
  const int rr = 32 * tr + lr, k = 32 * tk + lc;
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
  if (rr < R && k < K) x = *reinterpret_cast<const float4*>(flat + src + (int64_t)rr * K + k);  // K % 4 == 0
  bf16x4 pl[3];
  split4(x, pl);
  if (rr < R) {
    int pr = rr;
    if (H > 0) { const int j = rr < H ? rr : rr - H; pr = 128 * (j >> 6) + (j & 63) + (rr < H ? 0 : 64); }
#pragma unroll
    for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x4*>(planes + dst_w + ((int64_t)p * NR + pr) * Kp + k) = pl[p];
  }
  if (dst_wt < 0) return;
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) T[p][lc + j][lr] = pl[p][j];
  __syncthreads();
  const int kk = 32 * tk + lr, rc = 32 * tr + lc;   // row kk of W^T, columns rc .. rc + 3
  if (kk < K) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      bf16x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = T[p][lr][lc + j];
      *reinterpret_cast<bf16x4*>(planes + dst_wt + ((int64_t)p * K + kk) * Rp + rc) = v;
    }
  }
}

}  // namespace amk_gemm

using namespace amk_gemm;

static int padded_k(int K) { return (K + BK - 1) / BK * BK; }

extern "C" int64_t amk_gemm_x6_planes_bytes(int N, int K) {
  if (N <= 0 || K <= 0) return 0;
  return (int64_t)3 * N * padded_k(K) * 2;
}

extern "C" int amk_gemm_x6_split(const float* W, int64_t ldw, int N, int K, void* planes, void* stream) {
  AMK_CHECK_ARG(W && planes, "amk_gemm_x6_split: null pointer");
  AMK_CHECK_ARG(N > 0 && K > 0, "amk_gemm_x6_split: non-positive size");
  AMK_CHECK_SUPPORTED(K % 4 == 0 && ldw % 4 == 0 && ((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(planes)) & 15) == 0,
                      "amk_gemm_x6_split: K, ldw multiples of 4 and 16-byte aligned pointers");
  const int Kp = padded_k(K);
  const int64_t n = (int64_t)N * (Kp / 4);
  AMK_CHECK_SUPPORTED((n + 255) / 256 < (1ll << 31), "amk_gemm_x6_split: grid too large");
  hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     W, ldw, N, K, Kp, static_cast<__bf16*>(planes));
  AMK_CHECK_LAUNCH("amk_gemm_x6_split");
  return AMK_OK;
}

// A/B switch: 1 = the forms with K <= 256 and one contraction segment run gemm_x6_short_k_kernel; 0 = every launch is
// gemm_x6_nt_kernel
static std::atomic<int> g_short_k{1};

extern "C" int amk_gemm_x6_short_k(int on) {
  const int prev = g_short_k.load(std::memory_order_relaxed);
  if (on >= 0) g_short_k.store(on != 0, std::memory_order_relaxed);
  return prev;
}

// The short-K kernel addresses its outputs with 32-bit byte offsets (rows up to a block past M included)
static bool sk_out_ok(const float* p, int64_t ld, int M, int width) {
  return !p || (ld >= width && ((int64_t)(M + SK_BM) * ld + width) * 4 < 0x7ffffff0ll);
}

// The short-K kernel over one weight (N2 == 0) or two (PLAIN only); the caller has made the checks of x6_launch.
static int sk_launch(const char* who, int epi, const float* A, int64_t lda, const void* planes, const void* planes2, int K,
                     const float* bias, float* C, int64_t ldc, float* C2, int64_t ldc2, float* G, int64_t ldg, int M, int N,
                     int N2, void* stream) {
  SkArgs g;
  g.A = A; g.bias = bias; g.C = C; g.C2 = C2; g.G = G;
  g.Bp = static_cast<const __bf16*>(planes); g.Bp2 = static_cast<const __bf16*>(planes2);
  g.M = M; g.K = K; g.Kp = padded_k(K); g.N = N; g.N2 = N2;
  g.NR = epi == X6_GATE ? (N + 63) / 64 * 128 : N; g.NR2 = N2;
  g.nt1 = epi == X6_GATE ? (N + 31) / 32 : (N + 63) / 64;
  g.ntiles = g.nt1 + (N2 + 63) / 64;
  g.lda = lda; g.ldc = ldc; g.ldc2 = ldc2; g.ldg = ldg;
  const dim3 grid((unsigned)((M + SK_BM - 1) / SK_BM)), blk(SK_THR);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool full = g.Kp == SK_MAXK;
  if (epi == X6_GATE && C) {
    if (full) hipLaunchKernelGGL((gemm_x6_short_k_kernel<X6_GATE, true, true>), grid, blk, 0, st, g);
    else hipLaunchKernelGGL((gemm_x6_short_k_kernel<X6_GATE, false, true>), grid, blk, 0, st, g);
  } else if (epi == X6_GATE) {
    if (full) hipLaunchKernelGGL((gemm_x6_short_k_kernel<X6_GATE, true, false>), grid, blk, 0, st, g);
    else hipLaunchKernelGGL((gemm_x6_short_k_kernel<X6_GATE, false, false>), grid, blk, 0, st, g);
  } else {
    if (full) hipLaunchKernelGGL((gemm_x6_short_k_kernel<X6_PLAIN, true, false>), grid, blk, 0, st, g);
    else hipLaunchKernelGGL((gemm_x6_short_k_kernel<X6_PLAIN, false, false>), grid, blk, 0, st, g);
  }
  AMK_CHECK_LAUNCH(who);
  return AMK_OK;
}

// One driver for every form: checks as amk_gemm_x6_nt always made them (sizes, 16-byte rows, operands < 2 GiB).
static int x6_launch(const char* who, int epi, const float* A, int64_t lda, const void* planes, int K, const float* A2,
                     int64_t lda2, const void* planes2, int K2, const float* bias, const float* AB, int64_t ldab, float* C,
                     int64_t ldc, float* G, int64_t ldg, int M, int N, void* stream) {
  const bool two = A2 != nullptr;
  AMK_CHECK_ARG(A && planes, "%s: null pointer", who);
  AMK_CHECK_ARG(M > 0 && N > 0 && K > 0 && (!two || (K2 > 0 && planes2)), "%s: non-positive size M=%d N=%d K=%d", who, M, N, K);
  AMK_CHECK_SUPPORTED(K % 4 == 0 && lda % 4 == 0 && ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(planes)) & 15) == 0,
                      "%s: K, lda must be multiples of 4 and A, the planes 16-byte aligned", who);
  const int NR = epi == X6_GATE ? (N + 63) / 64 * 128 : N;
  AMK_CHECK_SUPPORTED(((int64_t)(M - 1) * lda + K) * 4 < 0x7ffffff0ll && (int64_t)3 * NR * padded_k(K) * 2 < 0x7ffffff0ll,
                      "%s: an operand must span < 2 GiB", who);
  if (two) {
    AMK_CHECK_SUPPORTED(K2 % 4 == 0 && lda2 % 4 == 0 && ((reinterpret_cast<uintptr_t>(A2) | reinterpret_cast<uintptr_t>(planes2)) & 15) == 0,
                        "%s: K2, lda2 must be multiples of 4 and A2, its planes 16-byte aligned", who);
    AMK_CHECK_SUPPORTED(((int64_t)(M - 1) * lda2 + K2) * 4 < 0x7ffffff0ll && (int64_t)3 * NR * padded_k(K2) * 2 < 0x7ffffff0ll,
                        "%s: an operand must span < 2 GiB", who);
  }
  if (g_short_k.load(std::memory_order_relaxed) && !two && K <= SK_MAXK && (epi == X6_PLAIN || epi == X6_GATE) &&
      sk_out_ok(C, ldc, M, epi == X6_GATE ? 2 * N : N) && sk_out_ok(G, ldg, M, N))
    return sk_launch(who, epi, A, lda, planes, nullptr, K, bias, C, ldc, nullptr, 0, G, ldg, M, N, 0, stream);
  Args g;
  g.A = A; g.A2 = A2; g.bias = bias; g.AB = AB; g.C = C; g.G = G;
  g.Bp = static_cast<const __bf16*>(planes); g.Bp2 = static_cast<const __bf16*>(planes2);
  g.M = M; g.N = N; g.K = K; g.Kp = padded_k(K); g.K2 = two ? K2 : 0; g.Kp2 = two ? padded_k(K2) : 0; g.NR = NR;
  g.lda = lda; g.lda2 = lda2; g.ldc = ldc; g.ldg = ldg; g.ldab = ldab;
  const int tn = epi == X6_GATE ? 64 : BN;
  const int64_t nwg = (int64_t)((M + BM - 1) / BM) * ((N + tn - 1) / tn);
  AMK_CHECK_SUPPORTED(nwg < (1ll << 31), "%s: grid too large", who);
  const dim3 grid((unsigned)nwg), blk(NTHR);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (epi == X6_GATE) hipLaunchKernelGGL((gemm_x6_nt_kernel<X6_GATE, false>), grid, blk, 0, st, g);
  else if (epi == X6_GATE_BWD) hipLaunchKernelGGL((gemm_x6_nt_kernel<X6_GATE_BWD, false>), grid, blk, 0, st, g);
  else if (two) hipLaunchKernelGGL((gemm_x6_nt_kernel<X6_PLAIN, true>), grid, blk, 0, st, g);
  else hipLaunchKernelGGL((gemm_x6_nt_kernel<X6_PLAIN, false>), grid, blk, 0, st, g);
  AMK_CHECK_LAUNCH(who);
  return AMK_OK;
}

extern "C" int amk_gemm_x6_nt(const float* A, int64_t lda, const void* b_planes, const float* bias,
                              float* C, int64_t ldc, int M, int N, int K, void* stream) {
  AMK_CHECK_ARG(C, "amk_gemm_x6_nt: null pointer");
  return x6_launch("amk_gemm_x6_nt", X6_PLAIN, A, lda, b_planes, K, nullptr, 0, nullptr, 0, bias, nullptr, 0, C, ldc, nullptr, 0, M, N, stream);
}

// C1 = A W1^T and C2 = A W2^T in one launch of the short-K kernel (the q and kv projections of one x): A is read and
// split once, the column walk runs over both weights.  With the switch off: two launches of gemm_x6_nt_kernel.
extern "C" int amk_gemm_x6_nt_cols2(const float* A, int64_t lda, const void* planes1, const void* planes2, float* C1,
                                    int64_t ldc1, float* C2, int64_t ldc2, int M, int N1, int N2, int K, void* stream) {
  const char* who = "amk_gemm_x6_nt_cols2";
  AMK_CHECK_ARG(A && planes1 && planes2 && C1 && C2, "%s: null pointer", who);
  AMK_CHECK_ARG(M > 0 && N1 > 0 && N2 > 0 && K > 0, "%s: non-positive size M=%d N1=%d N2=%d K=%d", who, M, N1, N2, K);
  AMK_CHECK_SUPPORTED(K <= SK_MAXK, "%s: K must be <= %d", who, SK_MAXK);
  AMK_CHECK_SUPPORTED(K % 4 == 0 && lda % 4 == 0 &&
                          ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(planes1) | reinterpret_cast<uintptr_t>(planes2)) & 15) == 0,
                      "%s: K, lda must be multiples of 4 and A, the planes 16-byte aligned", who);
  AMK_CHECK_SUPPORTED(((int64_t)(M - 1) * lda + K) * 4 < 0x7ffffff0ll && (int64_t)3 * N1 * padded_k(K) * 2 < 0x7ffffff0ll &&
                          (int64_t)3 * N2 * padded_k(K) * 2 < 0x7ffffff0ll,
                      "%s: an operand must span < 2 GiB", who);
  if (!g_short_k.load(std::memory_order_relaxed) || !sk_out_ok(C1, ldc1, M, N1) || !sk_out_ok(C2, ldc2, M, N2)) {
    const int rc = amk_gemm_x6_nt(A, lda, planes1, nullptr, C1, ldc1, M, N1, K, stream);
    return rc != AMK_OK ? rc : amk_gemm_x6_nt(A, lda, planes2, nullptr, C2, ldc2, M, N2, K, stream);
  }
  return sk_launch(who, X6_PLAIN, A, lda, planes1, planes2, K, nullptr, C1, ldc1, C2, ldc2, nullptr, 0, M, N1, N2, stream);
}

extern "C" int amk_gemm_x6_nt2(const float* A, int64_t lda, const void* planes, int K, const float* A2, int64_t lda2,
                               const void* planes2, int K2, float* C, int64_t ldc, int M, int N, void* stream) {
  AMK_CHECK_ARG(C && A2 && planes2, "amk_gemm_x6_nt2: null pointer");
  return x6_launch("amk_gemm_x6_nt2", X6_PLAIN, A, lda, planes, K, A2, lda2, planes2, K2, nullptr, nullptr, 0, C, ldc, nullptr, 0, M, N, stream);
}

extern "C" int amk_gemm_x6_gate_rows(int H) { return H > 0 ? (H + 63) / 64 * 128 : 0; }

extern "C" int amk_gemm_x6_nt_swiglu(const float* A, int64_t lda, const void* gate_planes, const float* bias, float* gate,
                                     int64_t ldg, float* ab, int64_t ldab, int M, int H, int K, void* stream) {
  AMK_CHECK_ARG(gate, "amk_gemm_x6_nt_swiglu: null pointer");
  return x6_launch("amk_gemm_x6_nt_swiglu", X6_GATE, A, lda, gate_planes, K, nullptr, 0, nullptr, 0, bias, nullptr, 0, ab, ldab, gate, ldg, M, H, stream);
}

extern "C" int amk_gemm_x6_nt_swiglu_bwd(const float* dY, int64_t ldy, const void* w3t_planes, const float* ab, int64_t ldab,
                                         float* d_ab, int64_t ldd, int M, int H, int K, void* stream) {
  AMK_CHECK_ARG(ab && d_ab, "amk_gemm_x6_nt_swiglu_bwd: null pointer");
  return x6_launch("amk_gemm_x6_nt_swiglu_bwd", X6_GATE_BWD, dY, ldy, w3t_planes, K, nullptr, 0, nullptr, 0, nullptr, ab, ldab, d_ab, ldd, nullptr, 0, M, H, stream);
}

extern "C" int amk_gemm_x6_split_table(const float* flat, int64_t flat_elems, const void* table, int n_entries, int64_t n_blocks,
                                       void* planes, int64_t planes_elems, void* stream) {
  AMK_CHECK_ARG(flat && table && planes, "amk_gemm_x6_split_table: null pointer");
  AMK_CHECK_ARG(n_entries > 0 && n_blocks > 0 && flat_elems > 0 && planes_elems > 0, "amk_gemm_x6_split_table: non-positive size");
  AMK_CHECK_SUPPORTED(((reinterpret_cast<uintptr_t>(flat) | reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(table)) & 15) == 0,
                      "amk_gemm_x6_split_table: 16-byte aligned pointers");
  AMK_CHECK_SUPPORTED(n_blocks < (1ll << 31), "amk_gemm_x6_split_table: grid too large");
  hipLaunchKernelGGL(split_table_kernel, dim3((unsigned)n_blocks), dim3(256), 0, static_cast<hipStream_t>(stream), flat, flat_elems,
                     static_cast<const int64_t*>(table), n_entries, static_cast<__bf16*>(planes), planes_elems);
  AMK_CHECK_LAUNCH("amk_gemm_x6_split_table");
  return AMK_OK;
}
