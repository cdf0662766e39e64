// Weight (and bias) gradient of nn.Linear for f32 operands with SPLIT-BF16 products ("bf16x6"):
//   C[n, k] = sum_m Y[m, n] X[m, k],  Y (M, N) and X (M, K) f32 row-major, the contraction index is the ROW.
//
// The exact-f32 kernel for this product (gemm_tn_kernel, csrc/gemm_f32.hip) sits at 0.65 of the f32 MFMA peak and is the
// last Linear product of the train step on the f32 matrix pipe.  Here every operand element is split into three bf16 parts
// x = h + m + l and a product is six v_mfma_f32_32x32x16_bf16 accumulated in f32, smallest first (the split-bf16 contract of
// amk_bf16.h, Y the A operand) -- f32-level error for 6 / 16 of the f32 MFMA's matrix-pipe time.
//
// Both operands are activations, so both are split ON THE FLY between the global load and the LDS store.  The three
// planes of each operand are staged AS STORED -- [rows of the step][columns] bf16, the padded row stride of
// gemm_tn_bf16_kernel (tile width + 32: conflict-free transposing reads) -- and both MFMA operands come from
// ds_read_b64_tr_b16 (every address a multiple of 8 bytes: row strides, plane sizes and column offsets all are).
//   tile 128 (n) x 256 (k), eight waves as 2 x 4 of 64 x 64, 16 rows per step   (gradients with many tiles), or
//   tile 128 x 128, four waves as 2 x 2, 32 rows per step;
//   two LDS stages, one LDS-only barrier per step, two steps of the operand stream in flight in registers;
//   per 16-deep block a wave issues 24 MFMAs against 24 transposing reads (one per MFMA gap).
// The M rows are cut into chunks so that tiles x chunks is one workgroup per CU; partial tiles (f32) go through a workspace
// (chunks, N, K) and are summed in chunk order, eight loads in flight (x6_tn_reduce_kernel, a sibling of tn_reduce_kernel:
// the same layout, but that kernel takes the f32 file's parameter block): bitwise reproducible.
// Output row segments as in the f32 kernel: rows [0, split) come from y and go to c, rows [split, N) from y2 to c2 (dWq |
// dWkv in one launch).  db = column sums of the f32 Y pieces, taken BEFORE the split by the workgroups of the first k tile.
#include "amk_bf16.h"
#include <stdlib.h>

namespace amk_x6tn {

constexpr unsigned COL_PAST = 0x40000000u;   // an offset past every descriptor (chunk panels are < 1 GiB): reads zeros

struct Params {
  const float *y, *y2, *x;
  float *c, *c2, *dbias, *ws, *dbias_ws;
  int64_t M, ldy, ldy2, ldx, ldc, ldc2;
  int N, K, split, ntk, total, nchunk, steps_per_chunk;
};

// split4 of amk_bf16.h (the same values in the same planes) with the statements in another order: h and m are stored
// before l is computed.  The compiler's schedule of the staging code follows the statement order, and this is the order
// the kernel was measured with, so the variant stays here.
__device__ __forceinline__ void split4_hm_first(const float4& x, bf16x4 (&pl)[3]) {
  const float v[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const __bf16 h = (__bf16)v[j];
    const float r1 = v[j] - (float)h;
    const __bf16 m = (__bf16)r1;
    pl[0][j] = h; pl[1][j] = m; pl[2][j] = (__bf16)(r1 - (float)m);
  }
}

// NWN x NWK waves of 64 x 64: tile 64 NWN (n) x 64 NWK (k); BKM rows of the contraction per step
template <int NWN, int NWK, int BKM>
__global__ __launch_bounds__(64 * NWN * NWK) void gemm_x6_tn_kernel(Params p) {
  constexpr int NTH = 64 * NWN * NWK, TN = 64 * NWN, TK = 64 * NWK;
  constexpr int YSTR = TN + 32, XSTR = TK + 32;               // bf16 per LDS row (TN / 2 + 16 dwords = 16 mod 64)
  constexpr int YPL = BKM * YSTR, XPL = BKM * XSTR;           // one plane of the Y / X tile
  constexpr int XT = 3 * YPL, STAGE = 3 * YPL + 3 * XPL;      // start of the X planes / elements of one stage
  constexpr int YCG = TN / 4, YRP = NTH / YCG, YNP = BKM / YRP;   // Y: 16-byte (4 float) column groups, rows per pass, pieces per thread
  constexpr int XCG = TK / 4, XRP = NTH / XCG, XNP = BKM / XRP;
  static_assert(TN == 128 && TK % 128 == 0 && BKM % 16 == 0 && YNP >= 1 && XNP >= 1 && YNP * YRP == BKM && XNP * XRP == BKM, "tile shape");
  static_assert(YRP * TN * 4 <= STAGE * 2, "the bias fold fits the first stage");
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];   // 2 stages
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 31, hf = lane >> 5;
  const int wn = wave / NWK, wk = wave % NWK;
  const int u = xcd_remap(blockIdx.x, p.total);
  // unit order (n tile, chunk, k tile): the k tiles that read the same dY panel are neighbours (one XCD, one L2)
  const int tk = u % p.ntk, rest = u / p.ntk;
  const int tn = rest / p.nchunk, chunk = rest - tn * p.nchunk;
  int n0 = tn * TN;
  const int k0 = tk * TK;
  const bool seg = p.split > 0 && n0 >= p.split;
  const float* Yb = seg ? p.y2 : p.y;
  const int64_t ldy = seg ? p.ldy2 : p.ldy;
  const int nrows = p.split > 0 ? (seg ? p.N - p.split : p.split) : p.N;   // rows of this segment's output
  if (seg) n0 -= p.split;
  const int64_t mbeg = (int64_t)chunk * p.steps_per_chunk * BKM;
  int64_t mend = mbeg + (int64_t)p.steps_per_chunk * BKM;
  if (mend > p.M) mend = p.M;
  const int mrows = (int)(mend - mbeg);
  // an even number of steps (a step of zeros at the end if need be): the two register sets alternate without a branch
  const int nk = ((mrows + BKM - 1) / BKM + 1) & ~1;

  // staging: thread -> column group (4 floats) of each operand tile, rows sr + RP i
  const int ycg = tid % YCG, ysr = tid / YCG, xcg = tid % XCG, xsr = tid / XCG;
  const __amdgpu_buffer_rsrc_t y_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(Yb + mbeg * ldy), 0, (int)(((int64_t)(mrows - 1) * ldy + nrows) * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + mbeg * p.ldx), 0, (int)(((int64_t)(mrows - 1) * p.ldx + p.K) * 4), 0x00020000);
  const bool yok = n0 + 4 * ycg < nrows, xok = k0 + 4 * xcg < p.K;   // (N and K multiples of 4: a piece is in or out)
  unsigned yoff[YNP], xoff[XNP];
#pragma unroll
  for (int i = 0; i < YNP; ++i) yoff[i] = yok ? (unsigned)(((int64_t)(ysr + YRP * i) * ldy + n0 + 4 * ycg) * 4) : COL_PAST;
#pragma unroll
  for (int i = 0; i < XNP; ++i) xoff[i] = xok ? (unsigned)(((int64_t)(xsr + XRP * i) * p.ldx + k0 + 4 * xcg) * 4) : COL_PAST;
  const unsigned ystep = (unsigned)(BKM * ldy * 4), xstep = (unsigned)(BKM * p.ldx * 4);
  struct Stg { float4 y[YNP], x[XNP]; };
  auto gload = [&](Stg& g, int t) {   // (steps past the chunk: rows past the descriptor's range, zeros)
#pragma unroll
    for (int i = 0; i < YNP; ++i)
      g.y[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(y_rsrc, (int)(yoff[i] == COL_PAST ? COL_PAST : yoff[i] + (unsigned)t * ystep), 0, 0));
#pragma unroll
    for (int i = 0; i < XNP; ++i)
      g.x[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, (int)(xoff[i] == COL_PAST ? COL_PAST : xoff[i] + (unsigned)t * xstep), 0, 0));
  };
  const bool do_bias = p.dbias != nullptr && tk == 0;
  float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
  auto lstore = [&](__bf16* stage, const Stg& g) {
#pragma unroll
    for (int i = 0; i < YNP; ++i) {
      const float4 v = g.y[i];
      if (do_bias) { bsum.x += v.x; bsum.y += v.y; bsum.z += v.z; bsum.w += v.w; }   // (steps past the chunk carry zeros)
      bf16x4 pl[3];
      split4_hm_first(v, pl);
#pragma unroll
      for (int q = 0; q < 3; ++q) *reinterpret_cast<bf16x4*>(&stage[q * YPL + (ysr + YRP * i) * YSTR + 4 * ycg]) = pl[q];
    }
#pragma unroll
    for (int i = 0; i < XNP; ++i) {
      bf16x4 pl[3];
      split4_hm_first(g.x[i], pl);
#pragma unroll
      for (int q = 0; q < 3; ++q) *reinterpret_cast<bf16x4*>(&stage[XT + q * XPL + (xsr + XRP * i) * XSTR + 4 * xcg]) = pl[q];
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = zero16();
  // two steps in flight in registers (sets ga, gb) beside the one being staged
  Stg ga, gb;
  gload(ga, 0);
  gload(gb, 1);
  lstore(smem, ga);
  gload(ga, 2);
  lds_barrier();
  auto step = [&](int t, Stg& g) {
    const __bf16* cur = smem + (t & 1) * STAGE;
    lstore(smem + ((t + 1) & 1) * STAGE, g);   // step t+1 (loaded two steps ago) -> the other stage; then fetch step t+3
    gload(g, t + 3);
#pragma unroll
    for (int s = 0; s < BKM / 16; ++s) {
      bf16x8 a[2][3], b[2][3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i][q] = tr_frag<YSTR>(cur + q * YPL, 16 * s, 64 * wn + 32 * i, lane);
          b[i][q] = tr_frag<XSTR>(cur + XT + q * XPL, 16 * s, 64 * wk + 32 * i, lane);
        }
      }
      // six partial products per output tile, smallest first; the four tiles' chains interleave
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = mfmab(a[i][x6_pa(q)], b[j][x6_pb(q)], acc[i][j]);
    }
    lds_barrier();
  };
  for (int t = 0; t < nk; t += 2) {
    step(t, gb);
    step(t + 1, ga);
  }
  // ---- the partial tile: rows n0 + 64 wn + 32 i + (r & 3) + 8 (r >> 2) + 4 hf, column k0 + 64 wk + 32 j + ln
  float* Cb;
  int64_t ldc;
  if (p.nchunk > 1) { Cb = p.ws + ((int64_t)chunk * p.N + (seg ? p.split : 0)) * p.K; ldc = p.K; }
  else { Cb = seg ? p.c2 : p.c; ldc = seg ? p.ldc2 : p.ldc; }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kc = k0 + 64 * wk + 32 * j + ln;
      if (kc < p.K) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = n0 + 64 * wn + 32 * i + acc_row(r, hf);
          if (n < nrows) Cb[(int64_t)n * ldc + kc] = acc[i][j][r];
        }
      }
    }
  }
  if (do_bias) {   // fold the YRP row groups of each column group, in order
    float* red = reinterpret_cast<float*>(smem);   // (the loop ended with a barrier)
    *reinterpret_cast<float4*>(&red[ysr * TN + 4 * ycg]) = bsum;
    lds_barrier();
    if (tid < TN) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < YRP; ++r) s += red[r * TN + tid];
      const int n = n0 + tid;
      if (n < nrows) (p.nchunk > 1 ? p.dbias_ws + (int64_t)chunk * p.N : p.dbias)[(seg ? p.split : 0) + n] = s;
    }
  }
}

// C = sum over chunks of ws (in chunk order).  Rows [0, split) go to c, the rest to c2.  One thread per 16-byte piece; the
// chunks are read eight at a time (independent loads in flight) and added in order.  The last workgroup folds the bias partials.
__global__ __launch_bounds__(256) void x6_tn_reduce_kernel(Params p) {
  const int64_t total4 = (int64_t)p.N * p.K / 4, slab = (int64_t)p.N * p.K;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total4) {
    const float* src = p.ws + 4 * i;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int c = 0;
    for (; c + 8 <= p.nchunk; c += 8) {
      float4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const float4*>(src + (c + j) * slab);
#pragma unroll
      for (int j = 0; j < 8; ++j) { s.x += v[j].x; s.y += v[j].y; s.z += v[j].z; s.w += v[j].w; }
    }
    for (; c < p.nchunk; ++c) {
      const float4 v = *reinterpret_cast<const float4*>(src + c * slab);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const int64_t e = 4 * i, row = e / p.K;
    const int col = (int)(e - row * p.K);
    if (p.split > 0 && row >= p.split) *reinterpret_cast<float4*>(p.c2 + (row - p.split) * p.ldc2 + col) = s;
    else *reinterpret_cast<float4*>(p.c + row * p.ldc + col) = s;
  }
  if (p.dbias && blockIdx.x == gridDim.x - 1) {
    for (int n = threadIdx.x; n < p.N; n += 256) {
      float s = 0.f;
      for (int c = 0; c < p.nchunk; ++c) s += p.dbias_ws[(int64_t)c * p.N + n];
      p.dbias[n] = s;
    }
  }
}

}  // namespace amk_x6tn

using namespace amk_x6tn;

// Tile width along K: 256 (eight waves, 16 rows per step: Y is staged and split once for 256 columns of X) for the
// gradients with many tiles, else 128 (four waves, 32 rows per step) -- the rule of gemm_tn_bf16_kernel, whose staging this
// kernel shares.  AMK_X6_TN_TK overrides (tools/kbench_x6_linear.py).
static int x6tn_tile_k(int N, int K) {
  static int forced = -1;
  if (forced < 0) {
    const char* e = getenv("AMK_X6_TN_TK");
    forced = e ? atoi(e) : 0;
  }
  if (forced == 128 || forced == 256) return forced;
  return (K >= 256 && ((N + 127) / 128) * ((K + 255) / 256) >= 12) ? 256 : 128;
}

static int x6tn_step_rows(int TK) { return TK == 256 ? 16 : 32; }

// chunks of the M rows: tiles x chunks = one workgroup per CU, at least 256 rows per chunk
static int x6tn_chunks(int64_t M, int N, int K, int* spc) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  }
  const int TK = x6tn_tile_k(N, K), BKM = x6tn_step_rows(TK);
  const int tiles = ((N + 127) / 128) * ((K + TK - 1) / TK);
  const int64_t steps = (M + BKM - 1) / BKM, min_steps = 256 / BKM;
  int64_t chunks = cus / tiles;
  if (chunks < 1) chunks = 1;
  if (chunks > steps / min_steps) chunks = steps / min_steps > 0 ? steps / min_steps : 1;
  const int64_t s = (steps + chunks - 1) / chunks;
  chunks = (steps + s - 1) / s;
  *spc = (int)s;
  return (int)chunks;
}

extern "C" int64_t amk_gemm_x6_tn_ws_bytes(int64_t M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  int spc;
  const int chunks = x6tn_chunks(M, N, K, &spc);
  return chunks > 1 ? ((int64_t)chunks * N * K + (int64_t)chunks * N) * 4 : 0;
}

extern "C" int amk_gemm_x6_tn(const float* y, int64_t ldy, const float* y2, int64_t ldy2, int split, const float* x, int64_t ldx,
                              float* c, int64_t ldc, float* c2, int64_t ldc2, float* dbias, int64_t M, int N, int K,
                              void* workspace, int64_t ws_bytes, void* stream) {
  AMK_CHECK_ARG(y && x && c, "amk_gemm_x6_tn: null operand");
  AMK_CHECK_ARG(M > 0 && N > 0 && K > 0, "amk_gemm_x6_tn: non-positive size");
  const bool two = split > 0;
  if (two) {
    AMK_CHECK_ARG(y2 && c2 && split < N, "amk_gemm_x6_tn: second row segment incomplete");
    AMK_CHECK_SUPPORTED(split % 128 == 0 && ldy2 % 4 == 0 && ldc2 % 4 == 0 && (((uintptr_t)y2 | (uintptr_t)c2) & 15) == 0,
                        "amk_gemm_x6_tn: split must be a multiple of 128, ldy2 and ldc2 of 4, y2 and c2 16-byte aligned");
  }
  AMK_CHECK_SUPPORTED(N % 4 == 0 && K % 4 == 0 && ldy % 4 == 0 && ldx % 4 == 0 && ldc % 4 == 0,
                      "amk_gemm_x6_tn: N, K and the leading dimensions must be multiples of 4");
  AMK_CHECK_SUPPORTED((((uintptr_t)y | (uintptr_t)x | (uintptr_t)c) & 15) == 0, "amk_gemm_x6_tn: pointers must be 16-byte aligned");
  const int64_t lim2 = 0x7ffffff0ll, lim1 = 1ll << 30;
  AMK_CHECK_SUPPORTED(((M - 1) * ldy + (two ? split : N)) * 4 < lim2 && ((M - 1) * ldx + K) * 4 < lim2 &&
                      (!two || ((M - 1) * ldy2 + (N - split)) * 4 < lim2) && (int64_t)N * K * 4 < lim1,
                      "amk_gemm_x6_tn: an operand must span < 2 GiB, the output < 1 GiB");
  Params p = {};
  p.y = y; p.y2 = y2; p.x = x; p.c = c; p.c2 = c2; p.dbias = dbias;
  p.M = M; p.N = N; p.K = K; p.split = two ? split : 0;
  p.ldy = ldy; p.ldy2 = ldy2; p.ldx = ldx; p.ldc = ldc; p.ldc2 = ldc2;
  int spc;
  p.nchunk = x6tn_chunks(M, N, K, &spc);
  p.steps_per_chunk = spc;
  const int TK = x6tn_tile_k(N, K), BKM = x6tn_step_rows(TK);
  // (+ 3 steps: the prefetch runs that far past a chunk, and its offsets must stay below COL_PAST)
  AMK_CHECK_SUPPORTED((int64_t)(spc + 3) * BKM * ldy * 4 < lim1 && (int64_t)(spc + 3) * BKM * ldx * 4 < lim1 &&
                      (!two || (int64_t)(spc + 3) * BKM * ldy2 * 4 < lim1), "amk_gemm_x6_tn: chunk panel beyond 1 GiB");
  if (p.nchunk > 1) {
    AMK_CHECK_ARG(workspace && ws_bytes >= amk_gemm_x6_tn_ws_bytes(M, N, K) && ((uintptr_t)workspace & 15) == 0,
                  "amk_gemm_x6_tn: workspace of amk_gemm_x6_tn_ws_bytes() bytes (16-byte aligned) required");
    p.ws = static_cast<float*>(workspace);
    p.dbias_ws = p.ws + (int64_t)p.nchunk * N * K;
  }
  p.ntk = (K + TK - 1) / TK;
  const int64_t total = (int64_t)((N + 127) / 128) * p.ntk * p.nchunk;
  AMK_CHECK_SUPPORTED(total < (1ll << 31), "amk_gemm_x6_tn: grid too large");
  p.total = (int)total;
  hipStream_t st = static_cast<hipStream_t>(stream);
  constexpr size_t lds4 = (size_t)2 * 3 * 32 * ((128 + 32) + (128 + 32)) * 2, lds8 = (size_t)2 * 3 * 16 * ((128 + 32) + (256 + 32)) * 2;
  // the opt-in to > 64 KiB of dynamic LDS is per device: a refusal is an error here, not an opaque launch failure later
  int dev_id = 0;
  AMK_CHECK_ARG(hipGetDevice(&dev_id) == hipSuccess && dev_id >= 0 && dev_id < 64, "amk_gemm_x6_tn: no current device");
  AMK_CHECK_SUPPORTED((amk_lds_optin<gemm_x6_tn_kernel<2, 2, 32>>((int)lds4) && amk_lds_optin<gemm_x6_tn_kernel<2, 4, 16>>((int)lds8)),
                      "amk_gemm_x6_tn: the device refused %zu bytes of dynamic LDS", lds4);
  if (TK == 256) hipLaunchKernelGGL((gemm_x6_tn_kernel<2, 4, 16>), dim3((unsigned)total), dim3(512), lds8, st, p);
  else hipLaunchKernelGGL((gemm_x6_tn_kernel<2, 2, 32>), dim3((unsigned)total), dim3(256), lds4, st, p);
  AMK_CHECK_LAUNCH("amk_gemm_x6_tn");
  if (p.nchunk > 1) {
    const int64_t blocks = ((int64_t)N * K / 4 + 255) / 256;
    hipLaunchKernelGGL(x6_tn_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p);
    AMK_CHECK_LAUNCH("amk_gemm_x6_tn(reduce)");
  }
  return AMK_OK;
}
