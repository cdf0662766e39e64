// Fused softmax-attention forward with SPLIT-BF16 products ("bf16x6") for gfx950.
//
// Same algorithm, masks, statistics and memory layout as attn_fwd.hip; only the two contractions
// are fed differently.  Every f32 operand x is split into three bf16 parts x = h + m + l
// (h = bf16(x), m = bf16(x - h), l = bf16(x - h - m): 24 mantissa bits) and a product a*b is
// formed as the six partial products  a_m b_m, a_l b_h, a_h b_l, a_m b_h, a_h b_m, a_h b_h,
// each exact in f32, accumulated in f32 by v_mfma_f32_32x32x16_bf16.  Measured
// (tools/ubench_bf16x6.hip): the error of a K = 64 dot product against double precision is
// 1.5e-6, the exact-f32 v_mfma_f32_32x32x2_f32 gives 2.6e-6 -- it is not a reduced-precision
// path -- and six of these MFMAs do a 32x32x16 block in 192 matrix cycles where the f32 MFMA
// needs 512 (399 against 155 algorithmic TFLOP/s).  The price is VALU work to split the operands
// (about 5.5 instructions per element, and the bf16 MFMA hides only about two VALU instructions
// per MFMA): so K and V are split ONCE per call by a pre-pass (attn_split_kv_kernel, three bf16
// planes per tile; V transposed and in accumulator key order, so that its A-operand fragments are
// single 16-byte reads) instead of once per query block, Q once per wave, and only P -- which
// exists nowhere else -- inside the tile loop, out of the S accumulators.
//
//   S^T (keys x queries) = K Q^T : A = K rows (LDS, 8 consecutive d per lane), B = Q^T (registers)
//   O^T (dims x queries) += V^T P^T : A = V^T rows (LDS, 8 keys per lane in accumulator order),
//                                     B = P^T out of the S^T accumulators (registers 8t..8t+7 of a
//                                     32-key block are the 8 keys of one k-slot)
// The 32x32x16 bf16 MFMA has the accumulator layout of the 32x32x2 f32 one, so fills, the online
// softmax, the rescale and the epilogue are those of attn_fwd.hip -- and so is the score-keeping store
// (KEEP: the raw S^T accumulators leave in the ScoreTiles layout for amk_attn_bwd_kept).
//
// Two kernels: attn_fwd_x6_kernel<CAUSAL, KEEP> takes the masks; attn_fwd_x6_plain_kernel<KEEP> is the
// unmasked specialisation with attn_fwd_plain_kernel's softmax (lazy reference, no fill path, peeled ragged tile,
// v_max3_f32 row maxima: this file is built with -fno-honor-nans -mno-amdgpu-ieee as attn_fwd.hip is).
#include "attn_common.h"
#include "amk_bf16.h"
#include <type_traits>

namespace amk_attn {

constexpr int PSTR = 72;                 // bf16 per LDS row (64 + 8): 144 B, conflict-free 16-byte row reads
constexpr int PLANE = TILE * PSTR;       // one plane of a 64-row tile

// Q^T operand: lane (query, half) holds, for each of the four 16-deep k-blocks c, the three planes of
// (q * scale * log2 e)[query][16c + 8*half + j], j = 0..7
__device__ __forceinline__ void load_q_planes(const FwdParams& p, int b, int h, int qi, int hf, bool qvalid, bf16x8 (&qpl)[4][3]) {
  const float qscale = p.scale * AMK_LOG2E;
  const float* qp = p.q + (int64_t)b * p.qs.sb + (int64_t)qi * p.qs.st + (int64_t)h * p.qs.sh + 8 * hf;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float4 t0 = qvalid ? ld4(qp + 16 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 t1 = qvalid ? ld4(qp + 16 * c + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float x[8] = {t0.x * qscale, t0.y * qscale, t0.z * qscale, t0.w * qscale,
                        t1.x * qscale, t1.y * qscale, t1.z * qscale, t1.w * qscale};
    split8(x, 0, qpl[c]);
  }
}
// S^T += K Q^T for the two 32-key halves of the tile: 2 x 4 k-blocks x 6 MFMAs
__device__ __forceinline__ void st_x6(const __bf16* Kp, const bf16x8 (&qpl)[4][3], int ln, int hf, f32x16& s0, f32x16& s1) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    bf16x8 ka[3], kb2[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      ka[q] = *reinterpret_cast<const bf16x8*>(&Kp[q * PLANE + ln * PSTR + 16 * c + 8 * hf]);
      kb2[q] = *reinterpret_cast<const bf16x8*>(&Kp[q * PLANE + (32 + ln) * PSTR + 16 * c + 8 * hf]);
    }
    mfma6x2(ka, qpl[c], s0, kb2, qpl[c], s1);
  }
}
// O^T += V^T P^T: 4 groups of 16 keys x 2 dim blocks x 6 MFMAs
// group g = 2*blk + t: registers 8t..8t+7 of S^T block blk are keys 32*blk + 16*t + 4*half + (j&3) + 8*(j>>2)
__device__ __forceinline__ void pv_x6(const __bf16* Vt, const f32x16& s0, const f32x16& s1, int ln, int hf, f32x16& o0, f32x16& o1) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = (g < 2) ? s0[8 * (g & 1) + j] : s1[8 * (g & 1) + j];
    bf16x8 pp[3];
    split8(x, 0, pp);
    bf16x8 va[3], vb[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      va[q] = *reinterpret_cast<const bf16x8*>(&Vt[q * PLANE + ln * PSTR + 16 * g + 8 * hf]);
      vb[q] = *reinterpret_cast<const bf16x8*>(&Vt[q * PLANE + (32 + ln) * PSTR + 16 * g + 8 * hf]);
    }
    mfma6x2(va, pp, o0, vb, pp, o1);
  }
}
// KEEP: the raw scores of one 64-key tile (log2 domain, before any fill), addressed as in attn_fwd.hip
__device__ __forceinline__ void keep_x6(float* sc_ptr, int64_t sc_kstep, int t, const f32x16& s0, const f32x16& s1) {
  float* t0 = sc_ptr + (int64_t)(2 * t) * sc_kstep;
  float* t1 = t0 + sc_kstep;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    __builtin_nontemporal_store(s0[r], t0 + acc_row(r, 0) * 32);
    __builtin_nontemporal_store(s1[r], t1 + acc_row(r, 0) * 32);
  }
}
// epilogue: normalise, store O rows and the softmax statistics (reference or maximum, sum relative to it)
__device__ __forceinline__ void epilogue_x6(const FwdParams& p, int b, int h, int qi, int hf, bool qvalid, const f32x16& o0,
                                            const f32x16& o1, float m_ref, float l_run) {
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.f / l_tot;
  if (qvalid) {
    float* op = p.o + (int64_t)b * p.os.sb + (int64_t)qi * p.os.st + (int64_t)h * p.os.sh + 4 * hf;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      st4(op + 8 * g, make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv));
      st4(op + 32 + 8 * g, make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv));
    }
    if (hf == 0) {
      float* sp = p.stats + (((int64_t)b * p.H + h) * p.I + qi) * 2;
      sp[0] = m_ref;
      sp[1] = l_tot;
    }
  }
}

template <bool CAUSAL, bool KEEP>
__global__ __launch_bounds__(WG, 2) void attn_fwd_x6_kernel(FwdParams p) {
  __shared__ __attribute__((aligned(16))) __bf16 Kp[3 * PLANE];   // [plane][key][d]
  __shared__ __attribute__((aligned(16))) __bf16 Vt[3 * PLANE];   // [plane][d][key position]
  __shared__ __attribute__((aligned(16))) float Kfill[TILE];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;

  // (wave-uniform by construction, said explicitly: see attn_fwd_plain_kernel)
  const int wg = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));
  const int qb = __builtin_amdgcn_readfirstlane(wg % p.nblk);
  const int bh = __builtin_amdgcn_readfirstlane(wg / p.nblk);
  const int h = __builtin_amdgcn_readfirstlane(bh % p.H), b = __builtin_amdgcn_readfirstlane(bh / p.H);

  const int qi = qb * BLK + wave * 32 + ln;  // this lane's query row
  const bool qvalid = qi < p.I;

  bf16x8 qpl[4][3];
  load_q_planes(p, b, h, qi, hf, qvalid, qpl);

  const uint8_t* kmask = p.key_mask ? p.key_mask + (int64_t)b * p.J : nullptr;
  const uint8_t* cmrow = CAUSAL ? p.causal_mask + (int64_t)qi * p.J : nullptr;

  // staging: the pre-pass left, per (batch, head, 64-key tile), 24 KB of K planes [key][plane][64 d] and
  // 24 KB of V^T planes [dim][plane][64 key positions], contiguous: 1536 16-byte chunks each, six per thread.
  const int ntile = (p.J + TILE - 1) / TILE;
  // one buffer descriptor over this (batch, head)'s tiles; chunk c of tile t is at byte (t*3072 + c)*16
  const __amdgpu_buffer_rsrc_t wsrc = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<char*>(p.x6_ws) + (int64_t)bh * ntile * 2 * 24576, 0, ntile * 2 * 24576, 0x00020000);
  float4 kch[6], vch[6];
  int lds_off[6];   // bf16 index inside a 3-plane LDS tile for chunk tid + 256*n
#pragma unroll
  for (int n = 0; n < 6; ++n) {
    const int c = tid + 256 * n;
    const int row = c / 24, plane = (c % 24) >> 3, k8 = c & 7;
    lds_off[n] = plane * PLANE + row * PSTR + 8 * k8;
  }
  float fillst = 0.f;
  auto prefetch = [&](int t) {
    const int base = t * 2 * 24576 + tid * 16;
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      kch[n] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wsrc, base + 4096 * n, 0, 0));
      vch[n] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wsrc, base + 24576 + 4096 * n, 0, 0));
    }
    if (tid < TILE) {
      const int j = t * TILE + tid;
      float f = 0.f;
      if (j >= p.J) f = -INFINITY;                       // beyond the sequence: weight 0
      else if (kmask && kmask[j] == 0) f = AMK_FILL_MASKED;  // masked_fill(~context_mask, -1e9)
      fillst = f;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      *reinterpret_cast<float4*>(&Kp[lds_off[n]]) = kch[n];
      *reinterpret_cast<float4*>(&Vt[lds_off[n]]) = vch[n];
    }
    if (tid < TILE) Kfill[tid] = fillst;
  };

  f32x16 o0 = zero16(), o1 = zero16();
  float m_run = -INFINITY, l_run = 0.f;

  const ScoreTiles stl(p.I, p.J);
  const int64_t sc_kstep = (int64_t)stl.nqt * 1024;  // floats between consecutive 32-key blocks
  float* sc_ptr = nullptr;
  if (KEEP) sc_ptr = p.scores + ((int64_t)bh * stl.nkb * stl.nqt + (qb * NWAVE + wave)) * 1024 + 4 * hf * 32 + ln;

  prefetch(0);
  for (int t = 0; t < ntile; ++t) {
    const int j0 = t * TILE;
    __syncthreads();  // every wave is done reading the previous tile
    commit();
    __syncthreads();
    if (t + 1 < ntile) prefetch(t + 1);

    unsigned cbits0 = 0, cbits1 = 0;
    if (CAUSAL) {
      if (qvalid) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ja = j0 + acc_row(r, hf), jb = ja + 32;
          if (ja < p.J && cmrow[ja]) cbits0 |= 1u << r;
          if (jb < p.J && cmrow[jb]) cbits1 |= 1u << r;
        }
      }
    }

    // ---- S^T = K Q^T for the two 32-key halves of the tile ----
    f32x16 s0 = zero16(), s1 = zero16();
    st_x6(Kp, qpl, ln, hf, s0, s1);
    if (KEEP) keep_x6(sc_ptr, sc_kstep, t, s0, s1);

    // ---- fills and online softmax: as attn_fwd.hip ----
    const bool plain = !CAUSAL && kmask == nullptr && (j0 + TILE <= p.J);  // wave-uniform
    float mx;
    if (plain) {
      mx = vmax(s0[0], s1[0], p.pinf);
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = vmax(mx, vmax(s0[r], s1[r], p.pinf), p.pinf);
    } else {
      mx = -INFINITY;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 f0 = ld4(&Kfill[8 * g + 4 * hf]);
        const float4 f1 = ld4(&Kfill[32 + 8 * g + 4 * hf]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          float t0 = s0[r], t1 = s1[r];
          const float fa = f4(f0, e), fb = f4(f1, e);
          t0 = (fa == 0.f) ? t0 : fa;
          t1 = (fb == 0.f) ? t1 : fb;
          if (CAUSAL) {
            t0 = ((cbits0 >> r) & 1u) ? AMK_FILL_MASKED : t0;
            t1 = ((cbits1 >> r) & 1u) ? AMK_FILL_MASKED : t1;
          }
          s0[r] = t0;
          s1[r] = t1;
          mx = vmax(mx, vmax(t0, t1, p.pinf), p.pinf);
        }
      }
    }
    mx = vmax(mx, __shfl_xor(mx, 32, 64), p.pinf);
    const float m_new = vmax(m_run, mx, p.pinf);
    f32x2 lsum2 = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p0 = __builtin_amdgcn_exp2f(s0[r] - m_new);
      const float p1 = __builtin_amdgcn_exp2f(s1[r] - m_new);
      s0[r] = p0;
      s1[r] = p1;
      lsum2 += (f32x2){p0, p1};
    }
    const float lsum = lsum2.x + lsum2.y;
    if (__any(m_new != m_run)) {
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o0[r] *= alpha;
        o1[r] *= alpha;
      }
      m_run = m_new;
    }
    l_run += lsum;

    pv_x6(Vt, s0, s1, ln, hf, o0, o1);
  }
  epilogue_x6(p, b, h, qi, hf, qvalid, o0, o1, m_run, l_run);
}

// ------------------------------------------------------------------------------------------------------------------
// The split-bf16 forward WITHOUT masks: attn_fwd_plain_kernel's softmax (see the comment there) on the x6 products.
// Here a VALU instruction costs more than it does next to the f32 MFMA (the bf16 MFMA hides about two per MFMA, and
// splitting P already takes ~5.5 per score), so the eager maximum's rescale, the fill path and the two-operand maxima
// weigh more than they did in the f32 kernel.
// Every S^T chain opens with a zero accumulator and the reference is subtracted afterwards (one v_sub per score), with
// or without KEEP.  The f32 kernel's form -- -mref as the chain's C operand -- was built and measured here too: 1 % faster
// (0.396 against 0.400 ms at the ViT-VQGAN layer shape, profiles/kbench_attn_fwd_x6.log) and not kept: the partial
// products are added smallest first, so an accumulator that starts at |mref| rounds every one of them at ulp(mref), and
// a score whose own sum |q||k| is far below |mref| (a row with one outlier key) leaves the per-element bound the kept
// scores are held to (tests/test_attention_x6_bounds.py shows it on the emulation).  As it stands the scores are bit
// for bit those of the KEEP variant and of attn_fwd_x6_kernel.
constexpr float LAZY_TAU = 8.f;   // as attn_fwd.hip

__device__ __forceinline__ float max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }

template <bool KEEP>
__global__ __launch_bounds__(WG, 2) void attn_fwd_x6_plain_kernel(FwdParams p) {
  __shared__ __attribute__((aligned(16))) __bf16 Kp[3 * PLANE];   // [plane][key][d]
  __shared__ __attribute__((aligned(16))) __bf16 Vt[3 * PLANE];   // [plane][d][key position]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;

  const int wg = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));
  const int qb = __builtin_amdgcn_readfirstlane(wg % p.nblk);
  const int bh = __builtin_amdgcn_readfirstlane(wg / p.nblk);
  const int h = __builtin_amdgcn_readfirstlane(bh % p.H), b = __builtin_amdgcn_readfirstlane(bh / p.H);

  const int qi = qb * BLK + wave * 32 + ln;  // this lane's query row
  const bool qvalid = qi < p.I;

  bf16x8 qpl[4][3];
  load_q_planes(p, b, h, qi, hf, qvalid, qpl);

  // staging as in attn_fwd_x6_kernel (the pre-pass wrote zeros for rows beyond the sequence)
  const int ntile = (p.J + TILE - 1) / TILE;
  const int nfull = p.J / TILE;
  const __amdgpu_buffer_rsrc_t wsrc = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<char*>(p.x6_ws) + (int64_t)bh * ntile * 2 * 24576, 0, ntile * 2 * 24576, 0x00020000);
  float4 kch[6], vch[6];
  int lds_off[6];
#pragma unroll
  for (int n = 0; n < 6; ++n) {
    const int c = tid + 256 * n;
    const int row = c / 24, plane = (c % 24) >> 3, k8 = c & 7;
    lds_off[n] = plane * PLANE + row * PSTR + 8 * k8;
  }
  auto prefetch = [&](int t) {
    const int base = t * 2 * 24576 + tid * 16;
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      kch[n] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wsrc, base + 4096 * n, 0, 0));
      vch[n] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wsrc, base + 24576 + 4096 * n, 0, 0));
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      *reinterpret_cast<float4*>(&Kp[lds_off[n]]) = kch[n];
      *reinterpret_cast<float4*>(&Vt[lds_off[n]]) = vch[n];
    }
  };

  f32x16 o0 = zero16(), o1 = zero16();
  float mref = 0.f, l_run = 0.f;

  const ScoreTiles stl(p.I, p.J);
  const int64_t sc_kstep = (int64_t)stl.nqt * 1024;
  float* sc_ptr = nullptr;
  if (KEEP) sc_ptr = p.scores + ((int64_t)bh * stl.nkb * stl.nqt + (qb * NWAVE + wave)) * 1024 + 4 * hf * 32 + ln;

  auto tile = [&](const int t, auto ragged_c) {
    constexpr bool RAGGED = decltype(ragged_c)::value;
    __syncthreads();  // every wave is done reading the previous tile
    commit();
    __syncthreads();
    if (t + 1 < ntile) prefetch(t + 1);

    f32x16 s0 = zero16(), s1 = zero16();
    st_x6(Kp, qpl, ln, hf, s0, s1);
    if (KEEP) keep_x6(sc_ptr, sc_kstep, t, s0, s1);
    if (RAGGED) {  // keys beyond the sequence: weight 0
      const int j0 = t * TILE;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s0[r] = (j0 + acc_row(r, hf) < p.J) ? s0[r] : -INFINITY;
        s1[r] = (j0 + 32 + acc_row(r, hf) < p.J) ? s1[r] : -INFINITY;
      }
    }
    // ---- the tile's row maximum, relative to the reference
    float mx = max3(s0[0], s1[0], s0[1]);
    mx = max3(mx, s1[1], s0[2]);
#pragma unroll
    for (int r = 2; r < 15; ++r) mx = max3(mx, s1[r], s0[r + 1]);
    mx = __builtin_fmaxf(mx, s1[15]);
    mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32, 64));
    mx -= mref;
    if (t == 0 || __any(mx > LAZY_TAU)) {  // rare after the first tile: move the reference of the rows that need it
      const float d = t == 0 ? mx : __builtin_fmaxf(mx, 0.f);
      if (t != 0) {
        const float alpha = __builtin_amdgcn_exp2f(-d);
        l_run *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          o0[r] *= alpha;
          o1[r] *= alpha;
        }
      }
      mref += d;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s0[r] = __builtin_amdgcn_exp2f(s0[r] - mref);
      s1[r] = __builtin_amdgcn_exp2f(s1[r] - mref);
    }
    f32x2 lsa = {0.f, 0.f}, lsb = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      lsa += (f32x2){s0[r], s0[r + 1]};
      lsb += (f32x2){s1[r], s1[r + 1]};
    }
    lsa += lsb;
    l_run += lsa.x + lsa.y;

    pv_x6(Vt, s0, s1, ln, hf, o0, o1);
  };

  prefetch(0);
  for (int t = 0; t < nfull; ++t) tile(t, std::false_type{});
  if (nfull < ntile) tile(nfull, std::true_type{});

  epilogue_x6(p, b, h, qi, hf, qvalid, o0, o1, mref, l_run);
}

// Pre-pass: one workgroup per (batch, head, 64-key tile) splits the K and V rows of the tile into bf16 planes.
//   K tile  -> [key 0..63][plane 0..2][64 d]
//   V tile  -> [dim 0..63][plane 0..2][64 key positions]; inside each group of 16 keys the positions are in
//              accumulator order [0..3, 8..11, 4..7, 12..15] (the k-slots of a P^T fragment)
// Rows beyond the sequence are written as zeros.
__global__ __launch_bounds__(WG) void attn_split_kv_kernel(FwdParams p) {
  const int tid = threadIdx.x;
  const int ntile = (p.J + TILE - 1) / TILE;
  // (wave-uniform, said explicitly: see attn_fwd_plain_kernel)
  const int t = __builtin_amdgcn_readfirstlane(blockIdx.x % ntile);
  const int bh = __builtin_amdgcn_readfirstlane(blockIdx.x / ntile);
  const int h = __builtin_amdgcn_readfirstlane(bh % p.H), b = __builtin_amdgcn_readfirstlane(bh / p.H);
  const float* kbase = p.k + (int64_t)b * p.ks.sb + (int64_t)h * p.ks.sh;
  const float* vbase = p.v + (int64_t)b * p.vs.sb + (int64_t)h * p.vs.sh;
  __bf16* out = reinterpret_cast<__bf16*>(p.x6_ws) + ((int64_t)bh * ntile + t) * 2 * 1536 * 8;
  const int srow = tid >> 4, scol = (tid & 15) * 4;
  RowStager kload, vload;
  kload.init(kbase, p.ks.st, p.J, tid);
  vload.init(vbase, p.vs.st, p.J, tid);
  kload.seek(t, p.ks.st, tid);
  vload.seek(t, p.vs.st, tid);
#pragma unroll
  for (int i = 0; i < 4; ++i) vload.voff[i] = (int)(((int64_t)(4 * srow + i) * p.vs.st + scol) * 4) + t * vload.step;
  float4 kst[4], vst[4];
  kload.load(kst);
  vload.load(vst);
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {   // K: row srow + 16*ps, dims scol..scol+3
    bf16x4 pl[3];
    split4(kst[ps], pl);
    const int r = srow + 16 * ps;
#pragma unroll
    for (int q = 0; q < 3; ++q) *reinterpret_cast<bf16x4*>(out + (r * 3 + q) * 64 + scol) = pl[q];
  }
  // V: this thread holds keys 4*srow .. 4*srow+3 x dims scol..scol+3; position of the key quad in its 16-group
  const int vpos = 16 * (srow >> 2) + 4 * (((srow & 1) << 1) | ((srow >> 1) & 1));
  __bf16* vout = out + 1536 * 8;
#pragma unroll
  for (int dd = 0; dd < 4; ++dd) {
    bf16x4 pl[3];
    split4(make_float4(f4(vst[0], dd), f4(vst[1], dd), f4(vst[2], dd), f4(vst[3], dd)), pl);
#pragma unroll
    for (int q = 0; q < 3; ++q) *reinterpret_cast<bf16x4*>(vout + ((scol + dd) * 3 + q) * 64 + vpos) = pl[q];
  }
}

void launch_attn_fwd_x6(const FwdParams& p, int64_t nwg, hipStream_t st, bool plain) {
  const int ntile = (p.J + TILE - 1) / TILE;
  const dim3 grid((unsigned)nwg), block(WG);
  hipLaunchKernelGGL(attn_split_kv_kernel, dim3((unsigned)((int64_t)p.B * p.H * ntile)), block, 0, st, p);
  const bool keep = p.scores != nullptr;
  if (p.causal_mask) {
    if (keep) hipLaunchKernelGGL((attn_fwd_x6_kernel<true, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((attn_fwd_x6_kernel<true, false>), grid, block, 0, st, p);
  } else if (p.key_mask || !plain) {
    if (keep) hipLaunchKernelGGL((attn_fwd_x6_kernel<false, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((attn_fwd_x6_kernel<false, false>), grid, block, 0, st, p);
  } else if (keep) {
    hipLaunchKernelGGL((attn_fwd_x6_plain_kernel<true>), grid, block, 0, st, p);
  } else {
    hipLaunchKernelGGL((attn_fwd_x6_plain_kernel<false>), grid, block, 0, st, p);
  }
}

}  // namespace amk_attn
