// Fused softmax-attention forward for gfx950 (exact-f32 MFMA, flash-style online softmax).
//
// Replaces models/softmax_attention.py:62-76 of the reference: einsum QK^T -> two
// masked_fill(-1e9) -> softmax -> einsum PV, which materialise the (B,h,I,J) scores
// several times in HBM.  Here a workgroup (4 waves, one per SIMD) owns 128 query rows
// of one (batch, head); each wave owns 32 of them with the QUERY ON THE LANE:
//
//   S^T tile (32 keys x 32 queries) = K_tile (A operand, rows from LDS, ds_read_b128)
//                                     x Q^T (B operand, 32 registers, loaded once)
//   -> lane (query = l&31, half = l>>5) holds 16 keys of its query per 32-key tile, so
//      the row max / row sum are in-register plus ONE cross-half exchange per 64 keys;
//   O^T tile (32 dims x 32 queries) += V_tile^T (A operand, ds_read_b32 column reads)
//                                      x P^T (B operand = the S^T accumulator registers
//                                      as they stand: no LDS round trip, no shuffles)
//   -> O stays query-on-lane too, so the online-softmax rescale is a per-lane scalar.
//
// K/V tiles of 64 keys are staged global -> registers -> LDS (loads for tile t+1 are
// issued before the MFMAs of tile t and written after them).
#include "attn_common.h"
#include <stdlib.h>
#include <type_traits>

// diagnostic builds only (tools/ablate_attn_fwd.sh): AMK_FWD_ABL bits switch parts of the tile loop off -- WRONG results,
// timing only: 1 no s - m, 2 no row max, 4 no row sum, 8 no exp, 16 no V reads from LDS, 32 no K reads from LDS,
// 64 tiles staged once (no global loads / LDS stores after the first), 128 no accumulator zeroing
#ifndef AMK_FWD_ABL
#define AMK_FWD_ABL 0
#endif

namespace amk_attn {

template <bool CAUSAL, bool SCHED, bool KEEP>
__global__ __launch_bounds__(WG, 2) void attn_fwd_kernel(FwdParams p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * TILE * LDS_STRIDE + TILE];
  float* Ks = smem;
  float* Vs = smem + TILE * LDS_STRIDE;
  float* Kfill = smem + 2 * TILE * LDS_STRIDE;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;

  const int wg = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));  // (wave-uniform; see attn_fwd_plain_kernel)
  const int qb = __builtin_amdgcn_readfirstlane(wg % p.nblk);
  const int bh = __builtin_amdgcn_readfirstlane(wg / p.nblk);
  const int h = __builtin_amdgcn_readfirstlane(bh % p.H), b = __builtin_amdgcn_readfirstlane(bh / p.H);

  const int qi = qb * BLK + wave * 32 + ln;  // this lane's query row
  const bool qvalid = qi < p.I;

  // Q^T operand: lane (query, half) holds (q * scale * log2 e)[query][32*half + s], s = 0..31,
  // so S^T comes out of the MFMAs already in the log2 domain of the exp2-based softmax.
  const float qscale = p.scale * AMK_LOG2E;
  float qreg[32];
  {
    const float* qp = p.q + (int64_t)b * p.qs.sb + (int64_t)qi * p.qs.st + (int64_t)h * p.qs.sh + 32 * hf;
#pragma unroll
    for (int s4 = 0; s4 < 8; ++s4) {
      float4 t = qvalid ? ld4(qp + 4 * s4) : make_float4(0.f, 0.f, 0.f, 0.f);
      qreg[4 * s4 + 0] = t.x * qscale;
      qreg[4 * s4 + 1] = t.y * qscale;
      qreg[4 * s4 + 2] = t.z * qscale;
      qreg[4 * s4 + 3] = t.w * qscale;
    }
  }

  const float* kbase = p.k + (int64_t)b * p.ks.sb + (int64_t)h * p.ks.sh;
  const float* vbase = p.v + (int64_t)b * p.vs.sb + (int64_t)h * p.vs.sh;
  const uint8_t* kmask = p.key_mask ? p.key_mask + (int64_t)b * p.J : nullptr;
  const uint8_t* cmrow = CAUSAL ? p.causal_mask + (int64_t)qi * p.J : nullptr;

  // staging registers: thread -> (row = tid/16 + 16*pass, 4 floats at column 4*(tid%16))
  const int srow = tid >> 4, scol = (tid & 15) * 4;
  float4 kst[4], vst[4];
  float fillst = 0.f;

  RowStager kload, vload;
  kload.init(kbase, p.ks.st, p.J, tid);
  vload.init(vbase, p.vs.st, p.J, tid);
  auto prefetch = [&](int j0) {
    kload.load(kst);
    vload.load(vst);
    if (tid < TILE) {
      const int j = j0 + tid;
      float f = 0.f;
      if (j >= p.J) f = -INFINITY;                       // beyond the sequence: weight 0
      else if (kmask && kmask[j] == 0) f = AMK_FILL_MASKED;  // masked_fill(~context_mask, -1e9)
      fillst = f;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int r = srow + 16 * ps;
      st4(&Ks[r * LDS_STRIDE + scol], kst[ps]);
      st4(&Vs[r * LDS_STRIDE + scol], vst[ps]);
    }
    if (tid < TILE) Kfill[tid] = fillst;
  };

  f32x16 o0 = zero16(), o1 = zero16();
  float m_run = -INFINITY, l_run = 0.f;

  // KEEP: S^T leaves for the backward as 32x32 tiles [key][query] (ScoreTiles): register r of this
  // lane is key acc_row(r, hf) of query ln, so a half-wave stores 128 contiguous bytes per register.
  const ScoreTiles stl(p.I, p.J);
  const int64_t sc_kstep = (int64_t)stl.nqt * 1024;  // floats between consecutive 32-key blocks
  float* sc_ptr = nullptr;
  if (KEEP) sc_ptr = p.scores + ((int64_t)bh * stl.nkb * stl.nqt + (qb * NWAVE + wave)) * 1024 + 4 * hf * 32 + ln;

  const int ntile = (p.J + TILE - 1) / TILE;
  prefetch(0);
  for (int t = 0; t < ntile; ++t) {
    const int j0 = t * TILE;
    if (!(AMK_FWD_ABL & 64) || t == 0) {
    __syncthreads();  // every wave is done reading the previous tile
    commit();
    __syncthreads();
    if (t + 1 < ntile) prefetch(j0 + TILE);
    }

    // causal bytes of this lane's query row for the 2 x 16 keys it will own in this tile
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

    // ---- S^T = K Q^T for the two 32-key halves of the tile (2 x 32 MFMAs) ----
    // K fragments are read one 4-deep k-block AHEAD of the MFMAs that consume them, so an
    // LDS round trip never sits between two MFMAs of this wave.
    f32x16 s0, s1;
    if (!(AMK_FWD_ABL & 128) || t == 0) { s0 = zero16(); s1 = zero16(); } else { s0 = o0; s1 = o1; }
    {
      const float* k0 = &Ks[ln * LDS_STRIDE + 32 * hf];
      const float* k1 = &Ks[(32 + ln) * LDS_STRIDE + 32 * hf];
      float4 a0 = ld4(k0), a1 = ld4(k1);
      if (SCHED) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // the prologue reads
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4) {
        float4 n0 = a0, n1 = a1;
        if (s4 + 1 < 8 && !(AMK_FWD_ABL & 32)) {
          n0 = ld4(k0 + 4 * (s4 + 1));
          n1 = ld4(k1 + 4 * (s4 + 1));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s0 = mfma32(f4(a0, e), qreg[4 * s4 + e], s0);
          s1 = mfma32(f4(a1, e), qreg[4 * s4 + e], s1);
        }
        if (SCHED) {
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // the 2 reads of the next k-block
          __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);  // then this block's 8 MFMAs
        }
        a0 = n0;
        a1 = n1;
      }
    }
    if (KEEP) {  // the raw scores (log2 domain, before any fill): what the backward would recompute
      float* t0 = sc_ptr + (int64_t)(2 * t) * sc_kstep;
      float* t1 = t0 + sc_kstep;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        __builtin_nontemporal_store(s0[r], t0 + acc_row(r, 0) * 32);
        __builtin_nontemporal_store(s1[r], t1 + acc_row(r, 0) * 32);
      }
    }
    // ---- fills and online softmax (lane-local + one cross-half exchange) ----
    // "plain" tiles (no key mask, no causal mask, all 64 keys inside the sequence) skip the fills.
    const bool plain = !CAUSAL && kmask == nullptr && (j0 + TILE <= p.J);  // wave-uniform
    float mx;
    if (plain && (AMK_FWD_ABL & 2)) {
      mx = s0[0];
    } else if (plain) {
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
      float x0 = s0[r], x1 = s1[r];
      if (!(AMK_FWD_ABL & 1)) { x0 -= m_new; x1 -= m_new; }
      const float p0 = (AMK_FWD_ABL & 8) ? x0 : __builtin_amdgcn_exp2f(x0);
      const float p1 = (AMK_FWD_ABL & 8) ? x1 : __builtin_amdgcn_exp2f(x1);
      s0[r] = p0;
      s1[r] = p1;
      if (!(AMK_FWD_ABL & 4)) lsum2 += (f32x2){p0, p1};  // one v_pk_add_f32 per pair
    }
    const float lsum = lsum2.x + lsum2.y;
    if (__any(m_new != m_run)) {  // the running max moved for some row of this wave: rescale
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

    // ---- O^T += V^T P^T (2 x 32 MFMAs); P^T is the S^T accumulator as it stands ----
    // V fragments are read one step (4 MFMAs) ahead.
    {
      const float* vcol = &Vs[(4 * hf) * LDS_STRIDE + ln];
      // step r uses rows acc_row(r, hf) and 32 + acc_row(r, hf), columns ln and ln + 32
      float c0 = vcol[0], c1 = vcol[32], c2 = vcol[32 * LDS_STRIDE], c3 = vcol[32 * LDS_STRIDE + 32];
      if (SCHED) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // the prologue reads
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float n0 = c0, n1 = c1, n2 = c2, n3 = c3;
        if (r + 1 < 16 && !(AMK_FWD_ABL & 16)) {
          const int row = ((r + 1) & 3) + 8 * ((r + 1) >> 2);
          n0 = vcol[row * LDS_STRIDE];
          n1 = vcol[row * LDS_STRIDE + 32];
          n2 = vcol[(32 + row) * LDS_STRIDE];
          n3 = vcol[(32 + row) * LDS_STRIDE + 32];
        }
        o0 = mfma32(c0, s0[r], o0);
        o1 = mfma32(c1, s0[r], o1);
        o0 = mfma32(c2, s1[r], o0);
        o1 = mfma32(c3, s1[r], o1);
        if (SCHED) {
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        }
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
      }
    }
  }

  // ---- epilogue: normalise, store O rows and the softmax statistics ----
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
      sp[0] = m_run;
      sp[1] = l_tot;
    }
  }
}


// ------------------------------------------------------------------------------------------------------------------
// The forward WITHOUT masks (no key-padding mask, no causal mask: every layer of ViT-VQGAN / ViT, the self-attention of
// the Muse decoder): same tiling and MFMA schedule as attn_fwd_kernel, with the softmax's VALU work cut from ~210 to
// ~100 instructions per 64-key tile and wave (every f32 VALU instruction costs ~4 cycles of the f32 MFMA pipe,
// tools/ubench_mfma_valu.hip; ablation: tools/ablate_attn_fwd.sh):
//   * LAZY REFERENCE.  softmax is invariant to the constant subtracted from the scores, so the running "max" only has
//     to stay within 2^LAZY_TAU of the true one: p = exp2(s - mref) is at most 2^8, l and O accumulate in f32 exactly
//     as before, and (mref, l) leave as the row statistics (the backward forms exp2(S - mref) / l: the same P).  The
//     reference moves only when a row's tile maximum exceeds it by more than LAZY_TAU (first tile: always) -- with 32
//     independent rows per wave the true maximum moves in almost every tile of SOME lane, so the eager form paid its
//     32 accumulator rescales nearly always; the lazy one almost never.
//   * -mref IS THE INITIAL ACCUMULATOR of the S^T chain (the MFMA's C operand, sixteen registers kept equal to -mref):
//     scores leave the matrix pipe already relative to the reference -- no v_sub per score, no zeroing.  (KEEP: the raw
//     scores go to HBM for the backward, so that variant keeps the subtraction.)
//   * no fill path at all in the loop (the mask variants modify scores element-wise in a branch, which costs 32 v_mov per
//     tile to break the accumulator tuples up); the ragged last tile (J % 64 != 0) is a peeled copy of the tile body;
//   * row maxima by v_max3_f32 (16 instead of 33 instructions; this file is built with -fno-honor-nans
//     -mno-amdgpu-ieee, as csrc/vq.hip is: no NaN can arise -- see the Makefile).
constexpr float LAZY_TAU = 8.f;

__device__ __forceinline__ float max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }

template <bool KEEP>
__global__ __launch_bounds__(WG, 2) void attn_fwd_plain_kernel(FwdParams p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * TILE * LDS_STRIDE];
  float* Ks = smem;
  float* Vs = smem + TILE * LDS_STRIDE;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;

  // (wave-uniform by construction; said explicitly: built without IEEE mode the compiler otherwise treats the quotients as
  // divergent and wraps every load through the K / V descriptors in a waterfall loop)
  const int wg = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));
  const int qb = __builtin_amdgcn_readfirstlane(wg % p.nblk);
  const int bh = __builtin_amdgcn_readfirstlane(wg / p.nblk);
  const int h = __builtin_amdgcn_readfirstlane(bh % p.H), b = __builtin_amdgcn_readfirstlane(bh / p.H);

  const int qi = qb * BLK + wave * 32 + ln;  // this lane's query row
  const bool qvalid = qi < p.I;

  const float qscale = p.scale * AMK_LOG2E;
  float qreg[32];
  {
    const float* qp = p.q + (int64_t)b * p.qs.sb + (int64_t)qi * p.qs.st + (int64_t)h * p.qs.sh + 32 * hf;
#pragma unroll
    for (int s4 = 0; s4 < 8; ++s4) {
      float4 t = qvalid ? ld4(qp + 4 * s4) : make_float4(0.f, 0.f, 0.f, 0.f);
      qreg[4 * s4 + 0] = t.x * qscale;
      qreg[4 * s4 + 1] = t.y * qscale;
      qreg[4 * s4 + 2] = t.z * qscale;
      qreg[4 * s4 + 3] = t.w * qscale;
    }
  }

  const float* kbase = p.k + (int64_t)b * p.ks.sb + (int64_t)h * p.ks.sh;
  const float* vbase = p.v + (int64_t)b * p.vs.sb + (int64_t)h * p.vs.sh;

  const int srow = tid >> 4, scol = (tid & 15) * 4;
  float4 kst[4], vst[4];
  RowStager kload, vload;
  kload.init(kbase, p.ks.st, p.J, tid);
  vload.init(vbase, p.vs.st, p.J, tid);
  auto prefetch = [&]() {
    kload.load(kst);
    vload.load(vst);
  };
  auto commit = [&]() {
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int r = srow + 16 * ps;
      st4(&Ks[r * LDS_STRIDE + scol], kst[ps]);
      st4(&Vs[r * LDS_STRIDE + scol], vst[ps]);
    }
  };

  f32x16 o0 = zero16(), o1 = zero16();
  f32x16 negm = zero16();            // sixteen copies of -mref: the C operand that opens every S^T chain
  float mref = 0.f, l_run = 0.f;

  const ScoreTiles stl(p.I, p.J);
  const int64_t sc_kstep = (int64_t)stl.nqt * 1024;
  float* sc_ptr = nullptr;
  if (KEEP) sc_ptr = p.scores + ((int64_t)bh * stl.nkb * stl.nqt + (qb * NWAVE + wave)) * 1024 + 4 * hf * 32 + ln;

  const int ntile = (p.J + TILE - 1) / TILE;
  const int nfull = p.J / TILE;

  auto tile = [&](const int t, auto ragged_c) {
    constexpr bool RAGGED = decltype(ragged_c)::value;
    __syncthreads();  // every wave is done reading the previous tile
    commit();
    __syncthreads();
    if (t + 1 < ntile) prefetch();

    // ---- S^T = K Q^T (- mref) for the two 32-key halves of the tile (2 x 32 MFMAs), K fragments one k-block ahead
    f32x16 s0, s1;
    if (KEEP) {
      s0 = zero16();
      s1 = zero16();
    } else {
      s0 = negm;
      s1 = negm;
    }
    {
      const float* k0 = &Ks[ln * LDS_STRIDE + 32 * hf];
      const float* k1 = &Ks[(32 + ln) * LDS_STRIDE + 32 * hf];
      float4 a0 = ld4(k0), a1 = ld4(k1);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4) {
        float4 n0 = a0, n1 = a1;
        if (s4 + 1 < 8) {
          n0 = ld4(k0 + 4 * (s4 + 1));
          n1 = ld4(k1 + 4 * (s4 + 1));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s0 = mfma32(f4(a0, e), qreg[4 * s4 + e], s0);
          s1 = mfma32(f4(a1, e), qreg[4 * s4 + e], s1);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
        a0 = n0;
        a1 = n1;
      }
    }
    if (KEEP) {  // the raw scores (log2 domain): what the backward would recompute
      float* t0 = sc_ptr + (int64_t)(2 * t) * sc_kstep;
      float* t1 = t0 + sc_kstep;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        __builtin_nontemporal_store(s0[r], t0 + acc_row(r, 0) * 32);
        __builtin_nontemporal_store(s1[r], t1 + acc_row(r, 0) * 32);
      }
    }
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
    if (KEEP) mx -= mref;
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
      if (!KEEP) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s0[r] -= d;
          s1[r] -= d;
          negm[r] = -mref;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s0[r] = __builtin_amdgcn_exp2f(KEEP ? s0[r] - mref : s0[r]);
      s1[r] = __builtin_amdgcn_exp2f(KEEP ? s1[r] - mref : s1[r]);
    }
    // row sums over register PAIRS of each accumulator (adjacent registers: one v_pk_add_f32 per pair)
    f32x2 lsa = {0.f, 0.f}, lsb = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      lsa += (f32x2){s0[r], s0[r + 1]};
      lsb += (f32x2){s1[r], s1[r + 1]};
    }
    lsa += lsb;
    l_run += lsa.x + lsa.y;

    // ---- O^T += V^T P^T (2 x 32 MFMAs); P^T is the S^T accumulator as it stands; V fragments one step ahead
    {
      const float* vcol = &Vs[(4 * hf) * LDS_STRIDE + ln];
      float c0 = vcol[0], c1 = vcol[32], c2 = vcol[32 * LDS_STRIDE], c3 = vcol[32 * LDS_STRIDE + 32];
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float n0 = c0, n1 = c1, n2 = c2, n3 = c3;
        if (r + 1 < 16) {
          const int row = ((r + 1) & 3) + 8 * ((r + 1) >> 2);
          n0 = vcol[row * LDS_STRIDE];
          n1 = vcol[row * LDS_STRIDE + 32];
          n2 = vcol[(32 + row) * LDS_STRIDE];
          n3 = vcol[(32 + row) * LDS_STRIDE + 32];
        }
        o0 = mfma32(c0, s0[r], o0);
        o1 = mfma32(c1, s0[r], o1);
        o0 = mfma32(c2, s1[r], o0);
        o1 = mfma32(c3, s1[r], o1);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
      }
    }
  };

  prefetch();
  for (int t = 0; t < nfull; ++t) tile(t, std::false_type{});
  if (nfull < ntile) tile(nfull, std::true_type{});

  // ---- epilogue: normalise, store O rows and the softmax statistics (reference, sum relative to it)
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
      sp[0] = mref;
      sp[1] = l_tot;
    }
  }
}

}  // namespace amk_attn

using namespace amk_attn;

// AMK_ATTN_FWD_PLAIN=0: unmasked calls go through the mask-capable kernels as well, f32 and split-bf16 (A/B measurements)
static bool getenv_plain() {   // (read per call: tools/ab_attn_fwd.py flips it inside one process)
  const char* e = getenv("AMK_ATTN_FWD_PLAIN");
  return !(e && e[0] == '0');
}

static int attn_fwd_impl(void* x6_ws, bool x6, float* scores, const float* q, const float* k, const float* v, float* o, float* stats,
                         const uint8_t* key_mask, const uint8_t* causal_mask,
                         int B, int H, int I, int J, int Dh,
                         int64_t q_sb, int64_t q_st, int64_t q_sh,
                         int64_t k_sb, int64_t k_st, int64_t k_sh,
                         int64_t v_sb, int64_t v_st, int64_t v_sh,
                         int64_t o_sb, int64_t o_st, int64_t o_sh,
                         float scale, void* stream) {
  AMK_CHECK_ARG(q && k && v && o && stats, "amk_attn_fwd: null tensor pointer");
  AMK_CHECK_ARG(B > 0 && H > 0 && I > 0 && J > 0, "amk_attn_fwd: non-positive size B=%d H=%d I=%d J=%d", B, H, I, J);
  AMK_CHECK_SUPPORTED(Dh == D || attn_gen_supported(Dh), "amk_attn_fwd: head dim %d not supported (a multiple of 32 from 32 to 256)", Dh);
  AMK_CHECK_SUPPORTED(Dh == D || !x6, "amk_attn_fwd_x6: the split-bf16 forward is built for head dim %d", D);
  AMK_CHECK_SUPPORTED(Dh == D || !scores || Dh == 32 || Dh == 128,
                      "amk_attn_fwd_keep: kept scores exist for head dims 32, 64 and 128 only (head dim %d)", Dh);
  AMK_CHECK_SUPPORTED(Dh == D || !scores || (!key_mask && !causal_mask),
                      "amk_attn_fwd_keep: for head dims 32 / 128 the score-keeping forward exists without masks only");
  FwdParams p;
  p.q = q; p.k = k; p.v = v; p.o = o; p.stats = stats;
  p.key_mask = key_mask; p.causal_mask = causal_mask;
  p.B = B; p.H = H; p.I = I; p.J = J;
  p.qs = {q_sb, q_st, q_sh}; p.ks = {k_sb, k_st, k_sh}; p.vs = {v_sb, v_st, v_sh}; p.os = {o_sb, o_st, o_sh};
  p.scale = scale;
  p.pinf = INFINITY;
  p.nblk = (I + BLK - 1) / BLK;
  p.x6_ws = x6_ws;
  p.scores = scores;
  AMK_CHECK_ARG(!scores || aligned16(scores), "amk_attn_fwd_keep: the scores buffer must be 16-byte aligned");
  AMK_CHECK_ARG(!x6 || (x6_ws && aligned16(x6_ws)), "amk_attn_fwd_x6: workspace missing or not 16-byte aligned");
  AMK_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(o) && strides_ok(p.qs) &&
                    strides_ok(p.ks) && strides_ok(p.vs) && strides_ok(p.os),
                "amk_attn_fwd: pointers must be 16-byte aligned and strides multiples of 4 elements");
  const int64_t nwg = (int64_t)B * H * p.nblk;
  AMK_CHECK_SUPPORTED(nwg < (1ll << 31), "amk_attn_fwd: grid too large");
  AMK_CHECK_SUPPORTED(((int64_t)J + TILE) * k_st * 4 < (1ll << 31) && ((int64_t)J + TILE) * v_st * 4 < (1ll << 31),
                      "amk_attn_fwd: one (batch, head) K/V slab must span < 2 GiB");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (Dh != D)
    launch_attn_fwd_gen(p, Dh, nwg, st);
  else if (x6)
    launch_attn_fwd_x6(p, nwg, st, getenv_plain());
  else if (!causal_mask && !key_mask && getenv_plain() && scores)
    hipLaunchKernelGGL((attn_fwd_plain_kernel<true>), dim3((unsigned)nwg), dim3(WG), 0, st, p);
  else if (!causal_mask && !key_mask && getenv_plain())
    hipLaunchKernelGGL((attn_fwd_plain_kernel<false>), dim3((unsigned)nwg), dim3(WG), 0, st, p);
  else if (causal_mask && scores)
    hipLaunchKernelGGL((attn_fwd_kernel<true, false, true>), dim3((unsigned)nwg), dim3(WG), 0, st, p);
  else if (causal_mask)
    hipLaunchKernelGGL((attn_fwd_kernel<true, false, false>), dim3((unsigned)nwg), dim3(WG), 0, st, p);
  else if (scores)
    hipLaunchKernelGGL((attn_fwd_kernel<false, true, true>), dim3((unsigned)nwg), dim3(WG), 0, st, p);
  else
    hipLaunchKernelGGL((attn_fwd_kernel<false, true, false>), dim3((unsigned)nwg), dim3(WG), 0, st, p);
  AMK_CHECK_LAUNCH("amk_attn_fwd");
  return AMK_OK;
}

extern "C" int amk_attn_fwd(const float* q, const float* k, const float* v, float* o, float* stats,
                            const uint8_t* key_mask, const uint8_t* causal_mask,
                            int B, int H, int I, int J, int Dh,
                            int64_t q_sb, int64_t q_st, int64_t q_sh,
                            int64_t k_sb, int64_t k_st, int64_t k_sh,
                            int64_t v_sb, int64_t v_st, int64_t v_sh,
                            int64_t o_sb, int64_t o_st, int64_t o_sh,
                            float scale, void* stream) {
  return attn_fwd_impl(nullptr, false, nullptr, q, k, v, o, stats, key_mask, causal_mask, B, H, I, J, Dh, q_sb, q_st, q_sh, k_sb, k_st, k_sh,
                       v_sb, v_st, v_sh, o_sb, o_st, o_sh, scale, stream);
}

extern "C" int64_t amk_attn_scores_bytes(int B, int H, int I, int J) {
  if (B <= 0 || H <= 0 || I <= 0 || J <= 0) return 0;
  return ScoreTiles(I, J).floats(B, H) * (int64_t)sizeof(float);
}

extern "C" int amk_attn_fwd_keep(const float* q, const float* k, const float* v, float* o, float* stats, float* scores,
                                 const uint8_t* key_mask, const uint8_t* causal_mask,
                                 int B, int H, int I, int J, int Dh,
                                 int64_t q_sb, int64_t q_st, int64_t q_sh,
                                 int64_t k_sb, int64_t k_st, int64_t k_sh,
                                 int64_t v_sb, int64_t v_st, int64_t v_sh,
                                 int64_t o_sb, int64_t o_st, int64_t o_sh,
                                 float scale, void* stream) {
  AMK_CHECK_ARG(scores, "amk_attn_fwd_keep: null scores buffer");
  return attn_fwd_impl(nullptr, false, scores, q, k, v, o, stats, key_mask, causal_mask, B, H, I, J, Dh, q_sb, q_st, q_sh, k_sb,
                       k_st, k_sh, v_sb, v_st, v_sh, o_sb, o_st, o_sh, scale, stream);
}

extern "C" int64_t amk_attn_fwd_x6_ws_bytes(int B, int H, int J) {
  if (B <= 0 || H <= 0 || J <= 0) return 0;
  return (int64_t)B * H * ((J + TILE - 1) / TILE) * 2 * 24576;
}

extern "C" int amk_attn_fwd_x6(const float* q, const float* k, const float* v, float* o, float* stats, void* ws,
                               const uint8_t* key_mask, const uint8_t* causal_mask,
                               int B, int H, int I, int J, int Dh,
                               int64_t q_sb, int64_t q_st, int64_t q_sh,
                               int64_t k_sb, int64_t k_st, int64_t k_sh,
                               int64_t v_sb, int64_t v_st, int64_t v_sh,
                               int64_t o_sb, int64_t o_st, int64_t o_sh,
                               float scale, void* stream) {
  return attn_fwd_impl(ws, true, nullptr, q, k, v, o, stats, key_mask, causal_mask, B, H, I, J, Dh, q_sb, q_st, q_sh, k_sb, k_st, k_sh,
                       v_sb, v_st, v_sh, o_sb, o_st, o_sh, scale, stream);
}

extern "C" int amk_attn_fwd_x6_keep(const float* q, const float* k, const float* v, float* o, float* stats, void* ws, float* scores,
                                    const uint8_t* key_mask, const uint8_t* causal_mask,
                                    int B, int H, int I, int J, int Dh,
                                    int64_t q_sb, int64_t q_st, int64_t q_sh,
                                    int64_t k_sb, int64_t k_st, int64_t k_sh,
                                    int64_t v_sb, int64_t v_st, int64_t v_sh,
                                    int64_t o_sb, int64_t o_st, int64_t o_sh,
                                    float scale, void* stream) {
  AMK_CHECK_ARG(scores, "amk_attn_fwd_x6_keep: null scores buffer");
  return attn_fwd_impl(ws, true, scores, q, k, v, o, stats, key_mask, causal_mask, B, H, I, J, Dh, q_sb, q_st, q_sh, k_sb, k_st,
                       k_sh, v_sb, v_st, v_sh, o_sb, o_st, o_sh, scale, stream);
}
