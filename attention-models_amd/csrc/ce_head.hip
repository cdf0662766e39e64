// Masked-token loss head for gfx950: logits + cross-entropy on the valid rows only (exact-f32 MFMA).
//
// Replaces decoder.linear(...) followed by F.cross_entropy(logits.transpose(1, 2), tgt, ignore_index=-1) at the end
// of the Muse / MaskGit train step (reference models/muse.py:176, models/maskgit.py:187), which writes the
// (rows, vocabulary) logits to HBM, keeps their log-softmax for the backward and materialises their gradient.
// Here the logits never leave the register file in the forward, and rows whose target is ignore_index cost nothing
// beyond rounding the number of valid rows up to a row tile:
//
//   ce_compact   : rows[0 .. count) = the indices m with target[m] != ignore_index, ascending (one workgroup, a
//                  ballot / prefix scan per 1024 targets: deterministic); rows[count .. M) = -1; count.
//   ce_fwd       : ROW ON THE LANE, as vq_argmin_kernel.  A workgroup owns 128 compacted rows (32 per wave) and a
//                  contiguous slice of the vocabulary.  Per 128-word tile: z^T (128 words x 32 rows per wave) =
//                  w_tile (A operand) x x[rows]^T (B operand), both staged k-major in LDS, BK = 16 per step; then the
//                  running (max, sum of exp) of the lane's row over the lane's 64 words, and the target logit when
//                  the target falls in the tile.  The two half-waves of a row are merged at the end (half 0 first);
//                  one (max, sum, target logit) partial per (row, slice).
//   ce_finalize  : one workgroup.  Per row: the slices merged in slice order, lse = m + log(s), loss_r = lse - z_t;
//                  thread t sums rows t, t + 1024, ... in ascending order, the 1024 sums fold as a binary tree in LDS,
//                  loss = sum / count (count == 0: 0 / 0 = NaN, as torch).  No atomics anywhere.
//   ce_bwd_g     : the same logits tile again; g = (exp(z - lse) - [v == t]) * (d_loss / count) into the caller's
//                  workspace G (compacted row i at stride ldg = V rounded up to 128; columns V .. ldg are zeros).
//   ce_bwd_dx    : dx[rows[i], :] = sum_v G[i, v] w[v, :]   (contraction in ascending v);
//   ce_zero_rows : dx rows whose target is ignore_index or outside [0, V) are written as zeros.
//   ce_bwd_dw    : dw[v, :] = sum_i G[i, v] x[rows[i], :]    (contraction in ascending i, up to count rounded to 16).
// Every grid is sized from M; a row tile that starts at or past count exits before any load.
//
// With a bias (amk_ce_head_bias_fwd / _bwd: the HAS_BIAS instantiations of ce_fwd and ce_bwd_g; the biasless ones are the
// code they were): the accumulator of the logits tile is PRELOADED with b[v0 + 32 b + acc_row(r, hf)] instead of being
// cleared, so z = b[v] + sum_k x w is one MFMA chain whose first term is the bias -- no VALU instruction per MFMA.  A word
// at or past the end of the slice is not loaded, preloads 0 and becomes -inf / a zero of G as before: nothing at or past
// b[V] is read.
//   ce_bwd_db    : db[v] = sum_i G[i, v] over the compacted rows, the f32 G that dw reads.  A workgroup of 1024 threads
//                  owns 32 columns: thread (column c = tid & 31, group q = tid >> 5) adds rows q, q + 32, q + 64, ... in
//                  ascending order (ceil(count / 32) terms, f32), the 32 group sums of a column fold as a binary tree in
//                  LDS (q += q + 16, then 8, 4, 2, 1).  No atomics; count == 0 writes zeros.  No workspace beyond G.
//
// A target that is neither ignore_index nor in [0, V) is never used as an index: its row is counted (count includes
// it), its loss is NaN -- so the mean is NaN -- and it receives and gives no gradient (its G row is zero, its dx row is
// zero); d_loss / count still divides by the count that includes it.
#include "ce_head_common.h"

namespace amk_ce {

using namespace amk_ce_common;   // TR, TA, SCAN, the limits, slices, the host drivers

constexpr int BK = 16;       // contraction depth per LDS stage
constexpr int LD = 132;      // LDS row stride (floats): 16-byte aligned rows

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

struct Stage { float4 v[2]; };

// Operand whose contraction index is contiguous in memory (a tile of 128 rows x BK): thread f covers row f >> 2,
// elements k0 + 4 (f & 3) .. + 3; written k-major.
template <class RowPtr>
__device__ __forceinline__ void load_t(RowPtr rowptr, int k0, int klim, Stage& s) {
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int f = threadIdx.x + 256 * ps;
    const float* p = rowptr(f >> 2);
    const int k = k0 + 4 * (f & 3);
    s.v[ps] = (p && k < klim) ? ld4(p + k) : zero4();
  }
}
__device__ __forceinline__ void store_t(float* T, const Stage& s) {
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int f = threadIdx.x + 256 * ps;
    float* d = T + 4 * (f & 3) * LD + (f >> 2);
    d[0] = s.v[ps].x; d[LD] = s.v[ps].y; d[2 * LD] = s.v[ps].z; d[3 * LD] = s.v[ps].w;
  }
}
// Operand whose contraction index is the memory row (BK rows x 128 columns): thread f covers row f >> 5, columns
// c0 + 4 (f & 31) .. + 3.
template <class RowPtr>
__device__ __forceinline__ void load_d(RowPtr rowptr, int c0, int clim, Stage& s) {
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int f = threadIdx.x + 256 * ps;
    const float* p = rowptr(f >> 5);
    const int c = c0 + 4 * (f & 31);
    s.v[ps] = (p && c < clim) ? ld4(p + c) : zero4();
  }
}
__device__ __forceinline__ void store_d(float* T, const Stage& s) {
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int f = threadIdx.x + 256 * ps;
    st4(T + (f >> 5) * LD + 4 * (f & 31), s.v[ps]);
  }
}

// acc[b][r] += sum_kk As[kk][32 b + acc_row(r, hf)] * Bs[kk][32 wave + ln], kk ascending in pairs (hf picks the
// element of the pair the lane supplies).
__device__ __forceinline__ void mma_stage(const float* As, const float* Bs, f32x16 (&acc)[4], int wave, int ln, int hf) {
#pragma unroll
  for (int kk = 0; kk < BK / 2; ++kk) {
    const float b = Bs[(2 * kk + hf) * LD + 32 * wave + ln];
    const float* ar = As + (2 * kk + hf) * LD + ln;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) acc[blk] = mfma32(ar[32 * blk], b, acc[blk]);
  }
}

// The staged product over a contraction of length L (a multiple of BK is not required: the loaders zero-fill):
// loads of stage s + 1 are in flight while stage s is multiplied.
template <class LoadA, class StoreA, class LoadB, class StoreB>
__device__ __forceinline__ void product(int L, float* As, float* Bs, f32x16 (&acc)[4], LoadA loadA, StoreA storeA,
                                        LoadB loadB, StoreB storeB) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  Stage sa, sb;
  loadA(0, sa);
  loadB(0, sb);
  for (int k0 = 0; k0 < L; k0 += BK) {
    __syncthreads();
    storeA(As, sa);
    storeB(Bs, sb);
    __syncthreads();
    if (k0 + BK < L) {
      loadA(k0 + BK, sa);
      loadB(k0 + BK, sb);
    }
    mma_stage(As, Bs, acc, wave, ln, hf);
  }
}

__device__ __forceinline__ void clear(f32x16 (&acc)[4]) {
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCAN) void ce_compact_kernel(const int64_t* __restrict__ target, int64_t ignore_index, int M,
                                                          int32_t* __restrict__ rows, int32_t* __restrict__ count) {
  __shared__ int wsum[SCAN / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int c0 = 0; c0 < M; c0 += SCAN) {
    const int m = c0 + tid;
    const bool on = m < M && target[m] != ignore_index;
    const unsigned long long bal = __ballot(on);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SCAN / 64; ++w) {
      const int c = wsum[w];
      off += w < wave ? c : 0;
      total += c;
    }
    if (on) rows[base + off + before] = m;
    base += total;
    __syncthreads();
  }
  for (int i = base + tid; i < M; i += SCAN) rows[i] = -1;
  if (tid == 0) count[0] = base;
}

// acc[b][r] = bias[v0 + 32 b + acc_row(r, hf)]: the bias is the first term of the logits' MFMA chain.  A whole tile inside
// the slice (a workgroup-uniform test) takes sixteen 16-byte loads (registers 4 g .. 4 g + 3 of a block are four
// consecutive words; bias is 16-byte aligned and v0 a multiple of 128); the slice's last, partial tile loads word by word
// under a predicate (a word at or past vend is not loaded and keeps 0): nothing at or past bias[vend] is read.
__device__ __forceinline__ void preload_bias(const float* __restrict__ bias, int v0, int vend, int hf, f32x16 (&acc)[4]) {
  if (v0 + TA <= vend) {
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 q = *reinterpret_cast<const float4*>(bias + v0 + 32 * b + 8 * g + 4 * hf);
        acc[b][4 * g] = q.x; acc[b][4 * g + 1] = q.y; acc[b][4 * g + 2] = q.z; acc[b][4 * g + 3] = q.w;
      }
  } else {
    const float* bp = bias + v0 + 4 * hf;   // one base, constant offsets: the loads are predicated, not clamped
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = 32 * b + 8 * (r >> 2) + (r & 3);   // acc_row(r, hf) - 4 hf
        float bv = 0.f;
        if (v0 + 4 * hf + o < vend) bv = bp[o];
        acc[b][r] = bv;
      }
  }
}

// ---------------------------------------------------------------------------------------
// The logits tile shared by ce_fwd and ce_bwd_g: z^T for words [v0, v0 + 128) x the workgroup's 128 compacted rows.
template <bool HAS_BIAS>
__device__ __forceinline__ void logits_tile(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w, int64_t ldw,
                                            int K, int v0, int vend, const int* srow, float* As, float* Bs, f32x16 (&acc)[4],
                                            const float* __restrict__ bias) {
  auto wrow = [&](int c) -> const float* { return v0 + c < vend ? w + (int64_t)(v0 + c) * ldw : nullptr; };
  auto xrow = [&](int c) -> const float* { const int r = srow[c]; return r >= 0 ? x + (int64_t)r * ldx : nullptr; };
  if constexpr (HAS_BIAS) {
    const int hf = (threadIdx.x & 63) >> 5;
    preload_bias(bias, v0, vend, hf, acc);
  } else {
    clear(acc);
  }
  product(K, As, Bs, acc,
          [&](int k0, Stage& s) { load_t(wrow, k0, K, s); }, [&](float* T, const Stage& s) { store_t(T, s); },
          [&](int k0, Stage& s) { load_t(xrow, k0, K, s); }, [&](float* T, const Stage& s) { store_t(T, s); });
}

template <bool HAS_BIAS>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                     int64_t ldw, const int64_t* __restrict__ target, int V, int K,
                                                     int nsplit, int vper, const int32_t* __restrict__ rows,
                                                     const int32_t* __restrict__ count, float* __restrict__ pm,
                                                     float* __restrict__ ps, float* __restrict__ pz,
                                                     const float* __restrict__ bias) {
  __shared__ __attribute__((aligned(16))) float As[BK * LD];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LD];
  __shared__ int srow[TR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  const int split = blockIdx.x % nsplit;
  const int r0 = (blockIdx.x / nsplit) * TR;
  const int cnt = count[0];
  if (r0 >= cnt) return;
  if (tid < TR) srow[tid] = r0 + tid < cnt ? rows[r0 + tid] : -1;
  __syncthreads();
  const int i = r0 + 32 * wave + ln;
  const int src = srow[32 * wave + ln];
  const int64_t t = src >= 0 ? target[src] : -1;

  const int vbeg = split * vper, vend = min(V, vbeg + vper);
  float m = -INFINITY, s = 0.f, zt = 0.f;
  bool found = false;
  f32x16 acc[4];
  for (int v0 = vbeg; v0 < vend; v0 += TA) {
    logits_tile<HAS_BIAS>(x, ldx, w, ldw, K, v0, vend, srow, As, Bs, acc, bias);
    float tmax = -INFINITY;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int v = v0 + 32 * b + acc_row(r, hf);
        const float z = v < vend ? acc[b][r] : -INFINITY;
        acc[b][r] = z;
        tmax = fmaxf(tmax, z);
        if (v == t) { zt = z; found = true; }
      }
    const float mn = fmaxf(m, tmax);
    if (mn > -INFINITY) {   // (a lane half none of whose words is in the tile keeps (-inf, 0))
      float add = 0.f;
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) add += __expf(acc[b][r] - mn);
      s = s * __expf(m - mn) + add;
      m = mn;
    }
  }
  // the two half-waves of a row hold interleaved words: half 0's sum first
  const float om = __shfl_xor(m, 32, 64), os = __shfl_xor(s, 32, 64), oz = __shfl_xor(zt, 32, 64);
  const bool of = __shfl_xor((int)found, 32, 64) != 0;
  if (hf == 0 && src >= 0) {
    const float mm = fmaxf(m, om);
    const float s0 = m > -INFINITY ? s * __expf(m - mm) : 0.f;
    const float s1 = om > -INFINITY ? os * __expf(om - mm) : 0.f;
    const int64_t o = (int64_t)i * nsplit + split;
    pm[o] = mm;
    ps[o] = s0 + s1;
    pz[o] = found ? zt : (of ? oz : 0.f);
  }
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCAN) void ce_finalize_kernel(const float* __restrict__ pm, const float* __restrict__ ps,
                                                           const float* __restrict__ pz, const int64_t* __restrict__ target,
                                                           const int32_t* __restrict__ rows, const int32_t* __restrict__ count,
                                                           int V, int nsplit, int vper, float* __restrict__ lse,
                                                           float* __restrict__ loss) {
  __shared__ float red[SCAN];
  const int tid = threadIdx.x;
  const int cnt = count[0];
  float part = 0.f;
  for (int i = tid; i < cnt; i += SCAN) {
    const int64_t o = (int64_t)i * nsplit;
    float m = pm[o], s = ps[o];
    for (int sl = 1; sl < nsplit; ++sl) {
      const float om = pm[o + sl], os = ps[o + sl];
      const float mm = fmaxf(m, om);
      s = s * __expf(m - mm) + os * __expf(om - mm);
      m = mm;
    }
    const float l = m + logf(s);
    lse[i] = l;
    const int64_t t = target[rows[i]];
    part += (t >= 0 && t < V) ? l - pz[o + (int)(t / vper)] : __builtin_nanf("");
  }
  red[tid] = part;
  __syncthreads();
  for (int o = SCAN / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) loss[0] = red[0] / (float)cnt;
}

// ---------------------------------------------------------------------------------------
template <bool HAS_BIAS>
__global__ __launch_bounds__(256) void ce_bwd_g_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                       int64_t ldw, const int64_t* __restrict__ target, int V, int K, int nvt,
                                                       const float* __restrict__ d_loss, const float* __restrict__ lse,
                                                       const int32_t* __restrict__ rows, const int32_t* __restrict__ count,
                                                       float* __restrict__ G, int64_t ldg, const float* __restrict__ bias) {
  __shared__ __attribute__((aligned(16))) float As[BK * LD];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LD];
  __shared__ int srow[TR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  const int v0 = (blockIdx.x % nvt) * TA;
  const int r0 = (blockIdx.x / nvt) * TR;
  const int cnt = count[0];
  if (r0 >= cnt) return;
  if (tid < TR) srow[tid] = r0 + tid < cnt ? rows[r0 + tid] : -1;
  __syncthreads();
  f32x16 acc[4];
  logits_tile<HAS_BIAS>(x, ldx, w, ldw, K, v0, V, srow, As, Bs, acc, bias);
  const int i = r0 + 32 * wave + ln;
  const int src = srow[32 * wave + ln];
  if (src < 0) return;
  const int64_t t = target[src];
  const bool oor = t < 0 || t >= V;
  const float l = lse[i];
  const float sc = d_loss[0] / (float)cnt;
  float* gp = G + (int64_t)i * ldg;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int v = v0 + 32 * b + 8 * g + 4 * hf;
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = __expf(acc[b][4 * g + e] - l);
        const float gv = (p - (v + e == t ? 1.f : 0.f)) * sc;
        o[e] = (v + e < V && !oor) ? gv : 0.f;
      }
      st4(gp + v, make_float4(o[0], o[1], o[2], o[3]));
    }
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ce_bwd_dx_kernel(const float* __restrict__ G, int64_t ldg, const float* __restrict__ w,
                                                        int64_t ldw, const int64_t* __restrict__ target, int V, int K, int nkt,
                                                        const int32_t* __restrict__ rows, const int32_t* __restrict__ count,
                                                        float* __restrict__ dx, int64_t lddx) {
  __shared__ __attribute__((aligned(16))) float As[BK * LD];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  const int kt0 = (blockIdx.x % nkt) * TA;
  const int r0 = (blockIdx.x / nkt) * TR;
  const int cnt = count[0];
  if (r0 >= cnt) return;
  const int vpad = (int)ldg;
  f32x16 acc[4];
  clear(acc);
  auto grow = [&](int c) -> const float* { return r0 + c < cnt ? G + (int64_t)(r0 + c) * ldg : nullptr; };
  product(V, As, Bs, acc,
          [&](int v0, Stage& s) {
            load_d([&](int kk) -> const float* { return v0 + kk < V ? w + (int64_t)(v0 + kk) * ldw : nullptr; }, kt0, K, s);
          },
          [&](float* T, const Stage& s) { store_d(T, s); },
          [&](int v0, Stage& s) { load_t(grow, v0, vpad, s); }, [&](float* T, const Stage& s) { store_t(T, s); });
  const int i = r0 + 32 * wave + ln;
  if (i >= cnt) return;
  const int src = rows[i];
  const int64_t t = target[src];
  if (t < 0 || t >= V) return;   // ce_zero_rows writes that row
  float* dp = dx + (int64_t)src * lddx;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int k = kt0 + 32 * b + 8 * g + 4 * hf;
      if (k < K) st4(dp + k, make_float4(acc[b][4 * g], acc[b][4 * g + 1], acc[b][4 * g + 2], acc[b][4 * g + 3]));
    }
}

__global__ __launch_bounds__(256) void ce_zero_rows_kernel(const int64_t* __restrict__ target, int64_t ignore_index, int64_t M,
                                                           int V, int K, float* __restrict__ dx, int64_t lddx) {
  const int k4 = K / 4;
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t m = f / k4;
  if (m >= M) return;
  const int64_t t = target[m];
  if (t == ignore_index || t < 0 || t >= V) st4(dx + m * lddx + 4 * (f % k4), zero4());
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ce_bwd_dw_kernel(const float* __restrict__ G, int64_t ldg, const float* __restrict__ x,
                                                        int64_t ldx, int V, int K, int nkt, const int32_t* __restrict__ rows,
                                                        const int32_t* __restrict__ count, float* __restrict__ dw, int64_t lddw) {
  __shared__ __attribute__((aligned(16))) float As[BK * LD];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  const int kt0 = (blockIdx.x % nkt) * TR;
  const int vt0 = (blockIdx.x / nkt) * TA;
  const int cnt = count[0];
  const int vpad = (int)ldg;
  f32x16 acc[4];
  clear(acc);
  product(cnt, As, Bs, acc,
          [&](int i0, Stage& s) {
            load_d([&](int kk) -> const float* { return i0 + kk < cnt ? G + (int64_t)(i0 + kk) * ldg : nullptr; }, vt0, vpad, s);
          },
          [&](float* T, const Stage& s) { store_d(T, s); },
          [&](int i0, Stage& s) {
            load_d([&](int kk) -> const float* { return i0 + kk < cnt ? x + (int64_t)rows[i0 + kk] * ldx : nullptr; }, kt0, K, s);
          },
          [&](float* T, const Stage& s) { store_d(T, s); });
  const int k = kt0 + 32 * wave + ln;
  if (k >= K) return;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int v = vt0 + 32 * b + acc_row(r, hf);
      if (v < V) dw[(int64_t)v * lddw + k] = acc[b][r];
    }
}

// ---------------------------------------------------------------------------------------
// db[v] = sum_i G[i, v], i < count: see the file header for the order.
constexpr int DBC = 32;   // columns per workgroup
constexpr int DBQ = 32;   // row groups per column
__global__ __launch_bounds__(DBC * DBQ) void ce_bwd_db_kernel(const float* __restrict__ G, int64_t ldg, int V,
                                                              const int32_t* __restrict__ count, float* __restrict__ db) {
  __shared__ float red[DBQ][DBC + 1];
  const int c = threadIdx.x & (DBC - 1), q = threadIdx.x / DBC;
  const int v = blockIdx.x * DBC + c;   // (< ldg: the grid covers ldg / DBC workgroups)
  const int cnt = count[0];
  float sum = 0.f;
  for (int i = q; i < cnt; i += DBQ) sum += G[(int64_t)i * ldg + v];
  red[q][c] = sum;
  __syncthreads();
  for (int o = DBQ / 2; o >= 1; o >>= 1) {
    if (q < o) red[q][c] += red[q + o][c];
    __syncthreads();
  }
  if (q == 0 && v < V) db[v] = red[0][c];
}

// this file, as the drivers of ce_head_common.h see it
struct Head {
  using T = float;
  static constexpr int MULT = 4;
  static constexpr decltype(&ce_fwd_kernel<false>) fwd[2] = {ce_fwd_kernel<false>, ce_fwd_kernel<true>};
  static constexpr decltype(&ce_bwd_g_kernel<false>) bwd_g[2] = {ce_bwd_g_kernel<false>, ce_bwd_g_kernel<true>};
  static constexpr auto zero_rows = &ce_zero_rows_kernel;
  static constexpr auto bwd_dx = &ce_bwd_dx_kernel;
  static constexpr auto bwd_dw = &ce_bwd_dw_kernel;
  static constexpr auto bwd_db = &ce_bwd_db_kernel;
  static constexpr int DB_COLS = DBC, DB_THREADS = DBC * DBQ;
};

}  // namespace amk_ce

// the one copy of the two kernels both heads launch
void amk_ce_common::ce_compact(hipStream_t st, const int64_t* target, int64_t ignore_index, int M, int32_t* rows, int32_t* count) {
  hipLaunchKernelGGL(amk_ce::ce_compact_kernel, dim3(1), dim3(SCAN), 0, st, target, ignore_index, M, rows, count);
}

void amk_ce_common::ce_finalize(hipStream_t st, const float* pm, const float* ps, const float* pz, const int64_t* target,
                                const int32_t* rows, const int32_t* count, int V, int nsplit, int vper, float* lse, float* loss) {
  hipLaunchKernelGGL(amk_ce::ce_finalize_kernel, dim3(1), dim3(SCAN), 0, st, pm, ps, pz, target, rows, count, V, nsplit, vper, lse,
                     loss);
}

using namespace amk_ce;

extern "C" int64_t amk_ce_head_fwd_ws_bytes(int64_t M, int V, int K) { return ce_fwd_ws_bytes(M, V, K); }

extern "C" int64_t amk_ce_head_bwd_ws_bytes(int64_t M, int V, int K) { return ce_bwd_ws_bytes(M, V, K, sizeof(Head::T)); }

extern "C" int amk_ce_head_fwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const int64_t* target,
                               int64_t ignore_index, int64_t M, int V, int K, float* loss, float* lse, int32_t* rows,
                               int32_t* count, void* ws, int64_t ws_bytes, void* stream) {
  return fwd_impl<Head>("amk_ce_head_fwd", x, ldx, w, ldw, target, ignore_index, M, V, K, loss, lse, rows, count, ws, ws_bytes,
                        stream, nullptr);
}

extern "C" int amk_ce_head_bias_fwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias,
                                    const int64_t* target, int64_t ignore_index, int64_t M, int V, int K, float* loss, float* lse,
                                    int32_t* rows, int32_t* count, void* ws, int64_t ws_bytes, void* stream) {
  AMK_CHECK_ARG(bias, "amk_ce_head_bias_fwd: null pointer (bias)");
  AMK_CHECK_ARG(a16(bias), "amk_ce_head_bias_fwd: misaligned pointer (bias: 16 bytes)");
  return fwd_impl<Head>("amk_ce_head_bias_fwd", x, ldx, w, ldw, target, ignore_index, M, V, K, loss, lse, rows, count, ws, ws_bytes,
                        stream, bias);
}

extern "C" int amk_ce_head_bwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const int64_t* target,
                               int64_t ignore_index, int64_t M, int V, int K, const float* d_loss, const float* lse,
                               const int32_t* rows, const int32_t* count, float* dx, int64_t lddx, float* dw, int64_t lddw,
                               void* ws, int64_t ws_bytes, void* stream) {
  return bwd_impl<Head>("amk_ce_head_bwd", x, ldx, w, ldw, target, ignore_index, M, V, K, d_loss, lse, rows, count, dx, lddx, dw,
                        lddw, ws, ws_bytes, stream, nullptr, nullptr);
}

extern "C" int amk_ce_head_bias_bwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias,
                                    const int64_t* target, int64_t ignore_index, int64_t M, int V, int K, const float* d_loss,
                                    const float* lse, const int32_t* rows, const int32_t* count, float* dx, int64_t lddx, float* dw,
                                    int64_t lddw, float* dbias, void* ws, int64_t ws_bytes, void* stream) {
  AMK_CHECK_ARG(bias && dbias, "amk_ce_head_bias_bwd: null pointer (bias or dbias)");
  AMK_CHECK_ARG(a16(bias) && a16(dbias), "amk_ce_head_bias_bwd: misaligned pointer (bias, dbias: 16 bytes)");
  return bwd_impl<Head>("amk_ce_head_bias_bwd", x, ldx, w, ldw, target, ignore_index, M, V, K, d_loss, lse, rows, count, dx, lddx,
                        dw, lddw, ws, ws_bytes, stream, bias, dbias);
}

