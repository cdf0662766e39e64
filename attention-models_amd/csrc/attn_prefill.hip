// Many-row attention for KV-cached decoding: n new query rows per (batch, head) against a cache of keys and values, with
// the append of the n new rows fused in (include/amk.h: amk_attn_prefill, amk_attn_prefill_bf16).  Replaces, for the n rows
// of a prompt, the score / softmax / PV core of models/softmax_attention.py:62-76 as the sampling loop of
// models/parti.py:135-152 would call it on a cache that already holds p0 rows.  The many-row form of csrc/attn_decode.hip:
// the same lane layout and the same chain of sums per row, so tests/attn_decode_ref.py's bound holds for row i with
// J = p0 + i + 1 keys.  Never captured: the position is still read on the device, but the grid depends on n.
//
//   * a workgroup owns (batch, head, chunk of KEYS = 64 keys, block of ROWS = 16 query rows), 256 threads.  A group of 8
//     lanes owns a key, as in the decode kernel: the 32 key groups take keys j0 + kg + 32 p, p < 2.  K and V of the
//     workgroup's (at most two) keys per group go from global memory to VGPRs ONCE, as f32, and serve all 16 rows.
//   * the rows go RB at a time (4, 2 or 1 by the registers a row needs).  Per row, exactly the decode kernel's chain:
//     a lane's dot product by FMA in the order of its dims, 3 shuffle additions, the chunk's maximum M, p = exp2(s - M),
//     l += p, o += p v per lane, the 32 key groups' partial rows added in key-group order through LDS.
//   * the causal predicate is computed from indices: row i attends keys j < p0 + i + 1.  A row with one active chunk is
//     written directly; otherwise each chunk leaves (M, l, o[D]) in the workspace and attn_prefill_combine_kernel, next
//     on the stream, adds the partials in chunk order.  No f32 atomics on data, no hand-off between workgroups: a row's
//     result does not depend on the batch size, on the row blocks or on the run.
//   * append mode: keys j >= p0 are rows j - p0 of k_new / v_new, never the cache.  Cache row p0 + i is written by ONE
//     workgroup, the one whose row block holds i and whose chunk holds p0 + i, as 16-byte pieces of the new row, bitwise.
//     Cache rows below p0 are only read, rows from p0 on only written: no workgroup reads a row that another writes.
//   * read mode (k_new null): every row attends rows 0 .. p0 - 1 (all `capacity` rows with n_dev null), with the key mask.
//   * the bf16 entry point runs the same body: a 16-byte piece holds 8 elements, lane g of a key's group holds dims
//     [8 (g + 8 i), +8) and, at D % 64 == 32, lanes 4-7 hold nothing of the last step.  bf16 -> f32 is exact; everything
//     between the loads and the store is f32 and o is rounded once, to nearest even, where it is stored.
#include "amk_bf16.h"
#include "attn_common.h"

namespace amk_prefill {

constexpr int GROUP = 8;               // lanes per key
constexpr int KGROUPS = 256 / GROUP;   // keys in flight per workgroup and pass
constexpr int KEYS = 64;               // keys per chunk: the decode kernel's default
constexpr int PASSES = KEYS / KGROUPS;
constexpr int ROWS = 16;               // query rows per workgroup

template <typename T>
struct Args {
  const T *q, *k_new, *v_new;
  T *k_cache, *v_cache, *o;
  float *ws_ml, *ws_o;
  const int32_t* n_dev;
  const uint8_t* key_mask;
  int H, capacity, n, nsplit;
  int64_t q_sb, q_st, q_sh, n_sb, n_st, n_sh, c_sb, c_st, c_sh, o_sb, o_st, o_sh;
  float qscale;
};

// one 16-byte piece as f32
__device__ __forceinline__ void load_piece(const float* p, float* r) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
}
__device__ __forceinline__ void load_piece(const __bf16* p, float* r) {
  const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (float)t[e];
}

// the dims of one row this lane owns: piece i holds dims [VEC (g + 8 i), +VEC); zeros where the lane owns nothing
template <typename T, int D, int NS>
__device__ __forceinline__ void load_row(const T* p, int g, float* r) {
  constexpr int VEC = 16 / sizeof(T);
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    if (VEC * (g + GROUP * i) < D) {
      load_piece(p + VEC * (g + GROUP * i), r + VEC * i);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) r[VEC * i + e] = 0.f;
    }
  }
}

// valid rows of the call, or -1 where nothing may be read or written
template <typename T>
__device__ __forceinline__ int valid_rows(const Args<T>& a, bool append) {
  const int p0 = a.n_dev ? *a.n_dev : a.capacity;
  if (append) return (p0 < 0 || p0 > a.capacity - a.n) ? -1 : p0;
  return (p0 < 1 || p0 > a.capacity) ? -1 : p0;
}

template <typename T, int D32>
__global__ __launch_bounds__(256) void attn_prefill_kernel(Args<T> a) {
  constexpr int D = D32 * 32;
  constexpr int VEC = 16 / sizeof(T);                      // elements of a 16-byte piece
  constexpr int NS = (D + GROUP * VEC - 1) / (GROUP * VEC);   // pieces per lane and row
  constexpr int NE = NS * VEC;                             // f32 registers per lane and row
  constexpr int RB = NE <= 8 ? 4 : (NE <= 16 ? 2 : 1);     // rows in flight
  constexpr int RSTRIDE = KGROUPS * D + KGROUPS + 4;       // per row in flight: partial rows, denominators, wave maxima
  __shared__ __attribute__((aligned(16))) float red[RB * RSTRIDE];
  const int s = blockIdx.x % a.nsplit, rblk = blockIdx.x / a.nsplit, h = blockIdx.y, b = blockIdx.z;
  const bool append = a.k_new != nullptr;
  const int p0 = valid_rows(a, append);
  if (p0 < 0) return;   // out of range: nothing is read or written
  const int i0 = rblk * ROWS, i1 = min(i0 + ROWS, a.n);
  const int j0 = s * KEYS;
  const int nk_last = append ? p0 + i1 : p0;   // keys the block's last row attends
  if (j0 >= nk_last) return;
  const int j1 = min(j0 + KEYS, nk_last);
  const int tid = threadIdx.x, g = tid & (GROUP - 1), kg = tid / GROUP;
  const int64_t cbase = b * a.c_sb + h * a.c_sh;
  const int64_t nbase = b * a.n_sb + h * a.n_sh;
  const uint8_t* km = a.key_mask ? a.key_mask + (int64_t)b * a.capacity : nullptr;

  // ---- the append: rows i of this block whose position p0 + i lies in this chunk -- one writer per cache row
  if (append) {
    constexpr int PIECES = D / VEC;
    const int ia = max(i0, j0 - p0), ib = min(i1, j0 + KEYS - p0);
    for (int it = tid; it < (ib - ia) * 2 * PIECES; it += 256) {
      const int i = ia + it / (2 * PIECES), rem = it % (2 * PIECES), pc = rem % PIECES;
      const T* src = (rem < PIECES ? a.k_new : a.v_new) + nbase + i * a.n_st + pc * VEC;
      T* dst = (rem < PIECES ? a.k_cache : a.v_cache) + cbase + (p0 + i) * a.c_st + pc * VEC;
      *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    }
  }

  // ---- K and V of this lane's keys, once for all rows of the block
  float kf[PASSES][NE], vf[PASSES][NE];
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int j = j0 + kg + KGROUPS * p;
    if (j < j1) {
      const bool fresh = append && j >= p0;
      const int64_t off = fresh ? nbase + (j - p0) * a.n_st : cbase + j * a.c_st;
      load_row<T, D, NS>((fresh ? a.k_new : a.k_cache) + off, g, kf[p]);
      load_row<T, D, NS>((fresh ? a.v_new : a.v_cache) + off, g, vf[p]);
    } else {
#pragma unroll
      for (int e = 0; e < NE; ++e) kf[p][e] = vf[p][e] = 0.f;
    }
  }

  for (int ig = i0; ig < i1; ig += RB) {
    int nk[RB];   // keys row ig + r attends in this chunk's range: j < nk[r]; j0 where the row has none here
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int i = ig + r;
      nk[r] = i < i1 ? min(j1, append ? p0 + i + 1 : p0) : j0;
    }
    bool any = false;
#pragma unroll
    for (int r = 0; r < RB; ++r) any = any || nk[r] > j0;
    if (!any) continue;   // none of these rows reaches this chunk (uniform over the workgroup)

    float qf[RB][NE];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (nk[r] > j0) {
        load_row<T, D, NS>(a.q + b * a.q_sb + (ig + r) * a.q_st + h * a.q_sh, g, qf[r]);
#pragma unroll
        for (int e = 0; e < NE; ++e) qf[r][e] *= a.qscale;
      } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) qf[r][e] = 0.f;
      }
    }

    // ---- pass 1: scores and the chunk's maximum per row
    float sc[RB][PASSES], mx[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) mx[r] = -INFINITY;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int j = j0 + kg + KGROUPS * p;
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) dot = fmaf(qf[r][e], kf[p][e], dot);
        dot += __shfl_xor(dot, 1, 64);
        dot += __shfl_xor(dot, 2, 64);
        dot += __shfl_xor(dot, 4, 64);
        if (j < nk[r]) {
          if (km && km[j] == 0) dot = AMK_FILL_MASKED;   // masked_fill(~context_mask, -1e9)
          sc[r][p] = dot;
          mx[r] = fmaxf(mx[r], dot);
        } else {
          sc[r][p] = -INFINITY;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      float m = mx[r];
      m = fmaxf(m, __shfl_xor(m, 8, 64));
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      if ((tid & 63) == 0) red[r * RSTRIDE + KGROUPS * D + KGROUPS + (tid >> 6)] = m;
    }
    __syncthreads();

    // ---- pass 2: p = exp2(s - M), l and o per key group.  Every thread keeps each row's M in a register: the words the
    // maxima went through are rewritten by the next row group before its first barrier, so nothing reads them after this pass
    float Mr[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const float* rx = red + r * RSTRIDE + KGROUPS * D + KGROUPS;
      const float M = fmaxf(fmaxf(rx[0], rx[1]), fmaxf(rx[2], rx[3]));   // finite where the row has a key here
      Mr[r] = M;
      float l = 0.f, of[NE];
#pragma unroll
      for (int e = 0; e < NE; ++e) of[e] = 0.f;
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int j = j0 + kg + KGROUPS * p;
        if (j < nk[r]) {
          const float pj = __builtin_amdgcn_exp2f(sc[r][p] - M);
          l += pj;
#pragma unroll
          for (int e = 0; e < NE; ++e) of[e] = fmaf(pj, vf[p][e], of[e]);
        }
      }
      float* rp = red + r * RSTRIDE + kg * D;
#pragma unroll
      for (int i = 0; i < NS; ++i)
        if (VEC * (g + GROUP * i) < D) {
#pragma unroll
          for (int e = 0; e < VEC; e += 4)
            *reinterpret_cast<float4*>(rp + VEC * (g + GROUP * i) + e) =
                make_float4(of[VEC * i + e], of[VEC * i + e + 1], of[VEC * i + e + 2], of[VEC * i + e + 3]);
        }
      if (g == 0) red[r * RSTRIDE + KGROUPS * D + kg] = l;
    }
    __syncthreads();

    // ---- each row's (l, o[d]) of the chunk: the 32 key groups in order; one thread per (row, dim)
    for (int it = tid; it < RB * D; it += 256) {
      const int r = it / D, d = it - r * D, i = ig + r;
      if (i >= i1) continue;
      const int nki = append ? p0 + i + 1 : p0;   // all the keys row i attends
      if (nki <= j0) continue;
      const float* rp = red + r * RSTRIDE;
      float od = 0.f, L = 0.f;
#pragma unroll 8
      for (int k = 0; k < KGROUPS; ++k) {
        od += rp[k * D + d];
        L += rp[KGROUPS * D + k];
      }
      if (nki <= KEYS) {   // one chunk: the row is done
        a.o[b * a.o_sb + i * a.o_st + h * a.o_sh + d] = (T)(od / L);
        continue;
      }
      // more chunks: leave the partial; attn_prefill_combine_kernel, next on the stream, adds them in chunk order
      const int64_t slot = (((int64_t)b * a.H + h) * a.n + i) * a.nsplit + s;
      a.ws_o[slot * D + d] = od;
      if (d == 0) {
        float M = Mr[0];   // row r's maximum, from this thread's registers
#pragma unroll
        for (int r2 = 1; r2 < RB; ++r2) M = r == r2 ? Mr[r2] : M;
        a.ws_ml[slot * 2] = M;
        a.ws_ml[slot * 2 + 1] = L;
      }
    }
    // No third barrier.  This phase reads the partial rows and denominators only, and the next row group writes those after
    // its first barrier, which no thread passes before it has left this phase.  The four maxima words ARE rewritten before
    // that barrier -- they were last read in pass 2, before the second barrier above.
  }
}

// The second launch: one thread per (row, dim) adds the row's chunks in chunk order.
template <typename T>
__global__ __launch_bounds__(256) void attn_prefill_combine_kernel(Args<T> a, int D) {
  const int h = blockIdx.y, b = blockIdx.z;
  const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= (int64_t)a.n * D) return;
  const int i = (int)(it / D), d = (int)(it - (int64_t)i * D);
  const bool append = a.k_new != nullptr;
  const int p0 = valid_rows(a, append);
  if (p0 < 0) return;
  const int nki = append ? p0 + i + 1 : p0;
  if (nki <= KEYS) return;   // written by the chunk's own workgroup
  const int active = (nki + KEYS - 1) / KEYS;
  const int64_t slot = (((int64_t)b * a.H + h) * a.n + i) * a.nsplit;
  const float* wml = a.ws_ml + slot * 2;
  const float* wo = a.ws_o + slot * D;
  // o[d] = (sum_c f_c o_c[d]) / (sum_c f_c l_c), f_c = exp2(M_c - max M), chunks in order
  float Mt = -INFINITY;
  for (int t = 0; t < active; ++t) Mt = fmaxf(Mt, wml[2 * t]);
  float acc = 0.f, den = 0.f;
  for (int t = 0; t < active; ++t) {
    const float f = __builtin_amdgcn_exp2f(wml[2 * t] - Mt);
    acc = fmaf(f, wo[(int64_t)t * D + d], acc);
    den = fmaf(f, wml[2 * t + 1], den);
  }
  a.o[b * a.o_sb + i * a.o_st + h * a.o_sh + d] = (T)(acc / den);   // bf16: the one rounding, to nearest even
}

static inline int64_t round4(int64_t x) { return (x + 3) & ~(int64_t)3; }
static inline int64_t nsplit_of(int capacity) { return (capacity + KEYS - 1) / KEYS; }
static inline int64_t nblocks_of(int n) { return (n + ROWS - 1) / ROWS; }

template <typename T>
static void launch_chunks(int d32, dim3 grid, hipStream_t st, const Args<T>& a) {
  switch (d32) {
    case 1: hipLaunchKernelGGL((attn_prefill_kernel<T, 1>), grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((attn_prefill_kernel<T, 2>), grid, dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL((attn_prefill_kernel<T, 3>), grid, dim3(256), 0, st, a); break;
    case 4: hipLaunchKernelGGL((attn_prefill_kernel<T, 4>), grid, dim3(256), 0, st, a); break;
    case 5: hipLaunchKernelGGL((attn_prefill_kernel<T, 5>), grid, dim3(256), 0, st, a); break;
    case 6: hipLaunchKernelGGL((attn_prefill_kernel<T, 6>), grid, dim3(256), 0, st, a); break;
    case 7: hipLaunchKernelGGL((attn_prefill_kernel<T, 7>), grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((attn_prefill_kernel<T, 8>), grid, dim3(256), 0, st, a); break;
  }
}

template <typename T>
static int run(const char* name, const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o,
               float* ws, const int32_t* n_dev, const uint8_t* key_mask, int B, int H, int D, int capacity, int n,
               int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t new_sb, int64_t new_st, int64_t new_sh,
               int64_t c_sb, int64_t c_st, int64_t c_sh, int64_t o_sb, int64_t o_st, int64_t o_sh, float scale, void* stream) {
  constexpr int VEC = 16 / sizeof(T);
  AMK_CHECK_ARG(q && k_cache && v_cache && o && ws, "%s: null pointer", name);
  AMK_CHECK_ARG((k_new != nullptr) == (v_new != nullptr), "%s: k_new and v_new go together", name);
  AMK_CHECK_ARG(!k_new || n_dev, "%s: append mode needs the device-resident length n_dev", name);
  AMK_CHECK_ARG(B > 0 && H > 0 && D > 0 && capacity > 0 && n > 0, "%s: bad sizes B=%d H=%d D=%d capacity=%d n=%d", name, B, H, D,
                capacity, n);
  AMK_CHECK_SUPPORTED(D % 32 == 0 && D <= 256, "%s: head dim %d (a multiple of 32 from 32 to 256)", name, D);
  AMK_CHECK_SUPPORTED(H <= 65535 && B <= 65535, "%s: B=%d, H=%d beyond the grid", name, B, H);
  const int64_t nsplit = nsplit_of(capacity), gx = nsplit * nblocks_of(n), cx = ((int64_t)n * D + 255) / 256;
  AMK_CHECK_SUPPORTED(gx <= 2147483647LL && cx <= 2147483647LL, "%s: capacity=%d, n=%d beyond the grid", name, capacity, n);
  AMK_CHECK_ARG(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_new) | reinterpret_cast<uintptr_t>(v_new) |
                  reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache) | reinterpret_cast<uintptr_t>(o) |
                  reinterpret_cast<uintptr_t>(ws)) & 15) == 0 && (reinterpret_cast<uintptr_t>(n_dev) & 3) == 0,
                "%s: pointers must be 16-byte aligned (n_dev: 4)", name);
  AMK_CHECK_ARG(((q_sb | q_st | q_sh | new_sb | new_st | new_sh | c_sb | c_st | c_sh | o_sb | o_st | o_sh) & (VEC - 1)) == 0,
                "%s: strides must be multiples of %d elements", name, VEC);
  hipStream_t st = static_cast<hipStream_t>(stream);
  Args<T> a;
  a.q = static_cast<const T*>(q); a.k_new = static_cast<const T*>(k_new); a.v_new = static_cast<const T*>(v_new);
  a.k_cache = static_cast<T*>(k_cache); a.v_cache = static_cast<T*>(v_cache); a.o = static_cast<T*>(o);
  a.ws_ml = ws;
  a.ws_o = ws + round4((int64_t)B * H * n * nsplit * 2);
  a.n_dev = n_dev; a.key_mask = key_mask;
  a.H = H; a.capacity = capacity; a.n = n; a.nsplit = (int)nsplit;
  a.q_sb = q_sb; a.q_st = q_st; a.q_sh = q_sh; a.n_sb = new_sb; a.n_st = new_st; a.n_sh = new_sh;
  a.c_sb = c_sb; a.c_st = c_st; a.c_sh = c_sh; a.o_sb = o_sb; a.o_st = o_st; a.o_sh = o_sh;
  a.qscale = scale * AMK_LOG2E;
  launch_chunks<T>(D / 32, dim3((unsigned)gx, (unsigned)H, (unsigned)B), st, a);
  if (nsplit > 1)
    hipLaunchKernelGGL(attn_prefill_combine_kernel<T>, dim3((unsigned)cx, (unsigned)H, (unsigned)B), dim3(256), 0, st, a, D);
  AMK_CHECK_LAUNCH(name);
  return AMK_OK;
}

}  // namespace amk_prefill

extern "C" int64_t amk_attn_prefill_ws_floats(int B, int H, int D, int capacity, int n) {
  if (B <= 0 || H <= 0 || D <= 0 || capacity <= 0 || n <= 0) return 0;
  const int64_t slots = (int64_t)B * H * n * amk_prefill::nsplit_of(capacity);
  return amk_prefill::round4(slots * 2) + slots * D;
}

extern "C" int amk_attn_prefill(const float* q, const float* k_new, const float* v_new, float* k_cache, float* v_cache,
                                float* o, float* ws, const int32_t* n_dev, const uint8_t* key_mask,
                                int B, int H, int D, int capacity, int n,
                                int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t new_sb, int64_t new_st, int64_t new_sh,
                                int64_t c_sb, int64_t c_st, int64_t c_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                                float scale, void* stream) {
  return amk_prefill::run<float>("amk_attn_prefill", q, k_new, v_new, k_cache, v_cache, o, ws, n_dev, key_mask, B, H, D, capacity,
                                 n, q_sb, q_st, q_sh, new_sb, new_st, new_sh, c_sb, c_st, c_sh, o_sb, o_st, o_sh, scale, stream);
}

extern "C" int amk_attn_prefill_bf16(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                                     void* o, float* ws, const int32_t* n_dev, const uint8_t* key_mask,
                                     int B, int H, int D, int capacity, int n,
                                     int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t new_sb, int64_t new_st, int64_t new_sh,
                                     int64_t c_sb, int64_t c_st, int64_t c_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                                     float scale, void* stream) {
  return amk_prefill::run<__bf16>("amk_attn_prefill_bf16", q, k_new, v_new, k_cache, v_cache, o, ws, n_dev, key_mask, B, H, D,
                                  capacity, n, q_sb, q_st, q_sh, new_sb, new_st, new_sh, c_sb, c_st, c_sh, o_sb, o_st, o_sh, scale,
                                  stream);
}
