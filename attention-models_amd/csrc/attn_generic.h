// Softmax attention with the head dim as a template parameter, any multiple of 32 up to 256 (the reference takes
// any dim_head, models/softmax_attention.py:23): the plain form of the forward, and the backward's three reproducible
// recompute kernels (delta, dK/dV, dQ; no atomics).  Exact-f32 v_mfma_f32_32x32x2_f32, the reduction axis on the
// lane, accumulators reused as the next product's B operand.
// The backward kernels serve every head dim, 64 included (instantiated by attn_bwd.hip, next to the dispatch).  The
// forward here serves the head dims other than 64: the D = 64 forward is the tuned one of attn_fwd.hip
// (software-pipelined operand reads, kept scores), and the one-pass backward of head dims 32, 64 and 128
// is attn_bwd_fused.hip.
// attn_generic.hip instantiates D = 32 and 128 and dispatches; attn_generic_dNNN.hip one further head dim each
// (separate translation units, so the build compiles them in parallel).
#pragma once
#include "attn_common.h"
#include <type_traits>

namespace amk_attn {

template <int DH>
struct GenGeom {
  static_assert(DH % 32 == 0 && DH >= 32 && DH <= 256, "head dims: multiples of 32 up to 256");
  static constexpr int HD = DH / 2;                 // k-extent owned by one half-wave
  // LDS row stride.  A ds_read_b128 row read puts lane l on row l: its 16-lane groups cover 16 distinct rows mod 16,
  // and LS / 4 = DH / 4 + 1 is odd (DH / 4 is a multiple of 8) for every head dim here, so those rows start on 16
  // distinct 16-byte slots of the 64 banks: conflict-free.  Column reads (ds_read_b32, one row per half-wave) and the
  // staging stores (ds_write_b128, 8 contiguous lanes = 32 consecutive floats of one row) are conflict-free at any LS.
  static constexpr int LS = DH + 4;
  static constexpr int NT = DH / 32;                // 32-wide output tiles
  static constexpr int TL = DH <= 64 ? 64 : 32;     // rows of the streamed operand per LDS tile
  static constexpr int NS = TL / 32;                // 32-row sub-tiles per LDS tile
  static constexpr int F4R = DH / 4;                // float4 per row
  // Staging: the TL x F4R float4 of a tile numbered row-major, thread tid takes numbers tid + 256 * ps.  TL * F4R =
  // 8 * DH (TL = 32) or 16 * DH (TL = 64) is a multiple of 256 for every head dim here, so every pass is whole; for
  // the powers of two (F4R | 256) this is the old "RP = 256 / F4R rows per pass" mapping.
  static constexpr int NP = TL * F4R / 256;         // passes per tile
  static_assert(TL * F4R % 256 == 0, "whole staging passes");
  // Register budget at one wave per SIMD (512 VGPR + AGPR).  The next tile is normally prefetched into registers
  // (2 * NP float4 per lane) while the current one is consumed; where that would spill, the tile is loaded at the
  // top of its own iteration instead (PF_* = false), its global latency exposed once per tile.
  static constexpr bool PF_FWD = DH <= 224;         // forward, dQ: q (and dO) rows DH / 2 + accumulators DH / 2 (+ DH / 2)
  static constexpr bool PF_DQ = DH <= 224;
  // dK / dV: k, v rows and both accumulators are 2 * DH registers per lane, 512 at DH = 256.  From DH = 160 on they
  // run as two passes over the queries: dV (k rows + dV accumulators) and dK (k, v rows + dK accumulators).
  static constexpr bool SPLIT_DKDV = DH >= 160;
  static constexpr bool PF_DK = DH <= 192;          // the dK pass (the dV pass and the fused form always prefetch)
  // Where even that leaves the arch-VGPR half of the file short (the MFMA B operands are the register rows), the
  // last PK_* float4 of one register row are parked in LDS (RowPark): the masked forward's q row, the dQ kernel's
  // dO row, the dK pass's v row.
  static constexpr int PK_FWD = DH == 256 ? 8 : 0;
  static constexpr int PK_DQ = DH == 256 ? 16 : 0;
  static constexpr int PK_DK = DH == 256 ? 20 : (DH == 224 ? 12 : (DH == 192 ? 8 : 0));
  // Head dim 64 has registers to spare in the recompute backward and runs it at two waves per SIMD (the causal
  // dK / dV, which carries the mask bits on top of both accumulators, at one).  Three refinements keep it inside that
  // budget and off the VALU; the other head dims sit at the limits above and stay without them:
  static constexpr int WAVES_DQ = DH <= 64 ? 2 : 1;
  static constexpr int waves_dkdv(bool causal) { return DH <= 32 || (DH == 64 && !causal) ? 2 : 1; }
  // a wave-uniform branch around the fill handling where no key of the tile (dQ) or of the wave (dK / dV) is filled
  // (without it the unmasked dK / dV spills at two waves)
  static constexpr bool SKIP_FILLS = DH == 64;
  // the causal-mask bytes of a tile gathered once into one bit word per 32-row sub-tile, tested per element
  static constexpr bool MASK_BITS = DH == 64;
  // dK / dV: the products of one P / dS column issue as all of dV's tiles, then dK's, not tile by tile (0.3 % of the
  // kernel at the ViT-VQGAN layer shape, measured)
  static constexpr bool DV_FIRST = DH == 64;
};

// LDS slots for the last PK float4 of one lane's register row: private to the lane (written and read by the same
// lane, so no barrier), 64 consecutive 16-byte slots per wave and float4, so a ds_read_b128 is conflict-free.
template <int PK>
struct RowPark {
  float4* slot;
  __device__ __forceinline__ RowPark(float4* buf, int wave, int lane) : slot(buf + wave * PK * 64 + lane) {}
  __device__ __forceinline__ void put(int k, float4 v) const { slot[k * 64] = v; }
  __device__ __forceinline__ float4 get(int k) const { return slot[k * 64]; }
};

// dK / dV kernel: both (the fused form), or one of the two passes of SPLIT_DKDV
enum DkdvPart { DKDV_BOTH = 0, DKDV_DV = 1, DKDV_DK = 2 };

// Streams TL rows x DH floats global -> registers through a range-checked buffer descriptor.
template <int DH>
struct GenStager {
  using G = GenGeom<DH>;
  __amdgpu_buffer_rsrc_t rsrc;
  int voff[G::NP];
  int step;
  // (for F4R | 256 the same numbers as tid / F4R + (256 / F4R) * ps, tid % F4R: written that way there)
  static __device__ __forceinline__ int srow(int tid, int ps) {
    return 256 % G::F4R == 0 ? tid / G::F4R + 256 / G::F4R * ps : (tid + 256 * ps) / G::F4R;
  }
  static __device__ __forceinline__ int scol(int tid, int ps) {
    return 256 % G::F4R == 0 ? tid % G::F4R * 4 : (tid + 256 * ps) % G::F4R * 4;
  }
  __device__ __forceinline__ void init(const float* base, int64_t row_stride, int nrows, int tid) {
    rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)(((int64_t)(nrows - 1) * row_stride + DH) * 4), 0x00020000);
#pragma unroll
    for (int ps = 0; ps < G::NP; ++ps) voff[ps] = (int)(((int64_t)srow(tid, ps) * row_stride + scol(tid, ps)) * 4);
    step = (int)(G::TL * row_stride * 4);
  }
  __device__ __forceinline__ void load(float4 (&dst)[G::NP]) {
#pragma unroll
    for (int ps = 0; ps < G::NP; ++ps) {
      dst[ps] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff[ps], 0, 0));
      voff[ps] += step;
    }
  }
  // LDS float offset of pass ps of this thread inside a [TL][LS] tile
  static __device__ __forceinline__ int lds_off(int tid, int ps) { return srow(tid, ps) * G::LS + scol(tid, ps); }
};

// The delta kernel: LPR lanes per (b, h, i) row, DH / 4 rounded up to a power of two (the xor-shuffle sum needs
// power-of-two lane groups); lanes past the row's DH / 4 float4 add zero.
template <int DH>
struct DeltaGeom {
  static constexpr int F4R = DH / 4;
  static constexpr int LPR = F4R <= 8 ? 8 : (F4R <= 16 ? 16 : (F4R <= 32 ? 32 : 64));
};

// ------------------------------------------------------------------------------------------------
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(WG, (DH <= 32 ? 2 : 1)) void attn_fwd_gen_kernel(FwdParams p) {
  using G = GenGeom<DH>;
  constexpr int HD = G::HD, LS = G::LS, NT = G::NT, TL = G::TL, NS = G::NS;
  __shared__ __attribute__((aligned(16))) float smem[2 * TL * LS + TL];
  float* Ks = smem;
  float* Vs = smem + TL * LS;
  float* Kfill = smem + 2 * TL * LS;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  const int wg = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));
  const int qb = __builtin_amdgcn_readfirstlane(wg % p.nblk);
  const int bh = __builtin_amdgcn_readfirstlane(wg / p.nblk);
  const int h = __builtin_amdgcn_readfirstlane(bh % p.H), b = __builtin_amdgcn_readfirstlane(bh / p.H);
  const int qi = qb * BLK + wave * 32 + ln;
  const bool qvalid = qi < p.I;

  const float qscale = p.scale * AMK_LOG2E;
  constexpr int PK = G::PK_FWD, CUT = HD / 4 - PK;   // q row: float4 [0, CUT) in registers, the rest parked
  __shared__ __attribute__((aligned(16))) float4 qpark[PK > 0 ? NWAVE * PK * 64 : 1];
  const RowPark<PK> qpk(qpark, wave, lane);
  float qreg[HD];
  {
    const float* qp = p.q + (int64_t)b * p.qs.sb + (int64_t)qi * p.qs.st + (int64_t)h * p.qs.sh + HD * hf;
#pragma unroll
    for (int s4 = 0; s4 < HD / 4; ++s4) {
      const float4 t = qvalid ? ld4(qp + 4 * s4) : make_float4(0.f, 0.f, 0.f, 0.f);
      if (s4 >= CUT) {
        qpk.put(s4 - CUT, make_float4(t.x * qscale, t.y * qscale, t.z * qscale, t.w * qscale));
        continue;
      }
      qreg[4 * s4 + 0] = t.x * qscale; qreg[4 * s4 + 1] = t.y * qscale;
      qreg[4 * s4 + 2] = t.z * qscale; qreg[4 * s4 + 3] = t.w * qscale;
    }
  }
  const float* kbase = p.k + (int64_t)b * p.ks.sb + (int64_t)h * p.ks.sh;
  const float* vbase = p.v + (int64_t)b * p.vs.sb + (int64_t)h * p.vs.sh;
  const uint8_t* kmask = p.key_mask ? p.key_mask + (int64_t)b * p.J : nullptr;
  const uint8_t* cmrow = CAUSAL ? p.causal_mask + (int64_t)qi * p.J : nullptr;

  float4 kst[G::NP], vst[G::NP];
  float fillst = 0.f;
  GenStager<DH> kload, vload;
  kload.init(kbase, p.ks.st, p.J, tid);
  vload.init(vbase, p.vs.st, p.J, tid);
  auto prefetch = [&](int j0) {
    kload.load(kst);
    vload.load(vst);
    if (tid < TL) {
      const int j = j0 + tid;
      float f = 0.f;
      if (j >= p.J) f = -INFINITY;
      else if (kmask && kmask[j] == 0) f = AMK_FILL_MASKED;
      fillst = f;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int ps = 0; ps < G::NP; ++ps) {
      st4(&Ks[GenStager<DH>::lds_off(tid, ps)], kst[ps]);
      st4(&Vs[GenStager<DH>::lds_off(tid, ps)], vst[ps]);
    }
    if (tid < TL) Kfill[tid] = fillst;
  };

  f32x16 o[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) o[n] = zero16();
  float m_run = -INFINITY, l_run = 0.f;

  const int ntile = (p.J + TL - 1) / TL;
  constexpr bool PF = G::PF_FWD;
  if (PF) prefetch(0);
  for (int t = 0; t < ntile; ++t) {
    const int j0 = t * TL;
    if (!PF) prefetch(j0);
    __syncthreads();
    commit();
    __syncthreads();
    if (PF && t + 1 < ntile) prefetch(j0 + TL);

    // S^T for the NS sub-tiles of 32 keys, fills, tile maximum
    f32x16 s[NS];
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      s[u] = zero16();
      const float* kr = &Ks[(32 * u + ln) * LS + HD * hf];
#pragma unroll
      for (int s4 = 0; s4 < HD / 4; ++s4) {
        const float4 a = ld4(kr + 4 * s4);
        const float4 qk = s4 < CUT ? a : qpk.get(s4 - CUT);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[u] = mfma32(f4(a, e), s4 < CUT ? qreg[4 * s4 + e] : f4(qk, e), s[u]);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 f = ld4(&Kfill[32 * u + 8 * g + 4 * hf]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const float fe = f4(f, e);
          float tt = (fe == 0.f) ? s[u][r] : fe;
          if (CAUSAL) {
            const int j = j0 + 32 * u + acc_row(r, hf);
            if (qvalid && j < p.J && cmrow[j]) tt = AMK_FILL_MASKED;
          }
          s[u][r] = tt;
          mx = vmax(mx, tt, p.pinf);
        }
      }
    }
    mx = vmax(mx, __shfl_xor(mx, 32, 64), p.pinf);
    const float m_new = vmax(m_run, mx, p.pinf);
    float lsum = 0.f;
#pragma unroll
    for (int u = 0; u < NS; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pr = __builtin_amdgcn_exp2f(s[u][r] - m_new);
        s[u][r] = pr;
        lsum += pr;
      }
    if (__any(m_new != m_run)) {
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= alpha;
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[n][r] *= alpha;
      m_run = m_new;
    }
    l_run += lsum;
    // O^T += V^T P^T
#pragma unroll
    for (int u = 0; u < NS; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* vc = &Vs[(32 * u + acc_row(r, hf)) * LS + ln];
#pragma unroll
        for (int n = 0; n < NT; ++n) o[n] = mfma32(vc[32 * n], s[u][r], o[n]);
      }
  }

  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.f / l_tot;
  if (qvalid) {
    float* op = p.o + (int64_t)b * p.os.sb + (int64_t)qi * p.os.st + (int64_t)h * p.os.sh + 4 * hf;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        st4(op + 32 * n + 8 * g, make_float4(o[n][4 * g] * inv, o[n][4 * g + 1] * inv, o[n][4 * g + 2] * inv, o[n][4 * g + 3] * inv));
    if (hf == 0) {
      float* sp = p.stats + (((int64_t)b * p.H + h) * p.I + qi) * 2;
      sp[0] = m_run;
      sp[1] = l_tot;
    }
  }
}


// ------------------------------------------------------------------------------------------------
// The forward WITHOUT masks for head dims 32 / 128 (round 4): attn_fwd_plain_kernel of attn_fwd.hip with the head dim as a
// template parameter -- lazy softmax reference held in the MFMA accumulators (-m_ref is the C operand that opens every
// S^T chain; the reference moves only when a row's tile maximum passes it by 2^8), v_max3 row maxima, packed row sums,
// no fill path (the ragged last tile is a peeled copy of the tile body), operand fragments read a step ahead.  (m_ref, l)
// leave as the statistics; the recompute backward forms exp2(S - m_ref) / l, the same P.
__device__ __forceinline__ float gmax3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }

// KEEP: the raw scores also leave for the one-pass backward (ScoreTiles, as amk_attn_fwd_keep for head dim 64); that form
// forms its S^T chains from zero and subtracts the reference afterwards (the backward needs the raw numbers).
template <int DH, bool KEEP>
__global__ __launch_bounds__(WG, (DH <= 32 ? 2 : 1)) void attn_fwd_gen_plain_kernel(FwdParams p) {
  using G = GenGeom<DH>;
  constexpr int HD = G::HD, LS = G::LS, NT = G::NT, TL = G::TL, NS = G::NS;
  constexpr float TAU = 8.f;
  __shared__ __attribute__((aligned(16))) float smem[2 * TL * LS];
  float* Ks = smem;
  float* Vs = smem + TL * LS;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  // (wave-uniform; said explicitly because this file is built without IEEE mode: see attn_fwd_plain_kernel)
  const int wg = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));
  const int qb = __builtin_amdgcn_readfirstlane(wg % p.nblk);
  const int bh = __builtin_amdgcn_readfirstlane(wg / p.nblk);
  const int h = __builtin_amdgcn_readfirstlane(bh % p.H), b = __builtin_amdgcn_readfirstlane(bh / p.H);
  const int qi = qb * BLK + wave * 32 + ln;
  const bool qvalid = qi < p.I;

  const float qscale = p.scale * AMK_LOG2E;
  float qreg[HD];
  {
    const float* qp = p.q + (int64_t)b * p.qs.sb + (int64_t)qi * p.qs.st + (int64_t)h * p.qs.sh + HD * hf;
#pragma unroll
    for (int s4 = 0; s4 < HD / 4; ++s4) {
      const float4 t = qvalid ? ld4(qp + 4 * s4) : make_float4(0.f, 0.f, 0.f, 0.f);
      qreg[4 * s4 + 0] = t.x * qscale; qreg[4 * s4 + 1] = t.y * qscale;
      qreg[4 * s4 + 2] = t.z * qscale; qreg[4 * s4 + 3] = t.w * qscale;
    }
  }
  const float* kbase = p.k + (int64_t)b * p.ks.sb + (int64_t)h * p.ks.sh;
  const float* vbase = p.v + (int64_t)b * p.vs.sb + (int64_t)h * p.vs.sh;
  float4 kst[G::NP], vst[G::NP];
  GenStager<DH> kload, vload;
  kload.init(kbase, p.ks.st, p.J, tid);
  vload.init(vbase, p.vs.st, p.J, tid);
  auto prefetch = [&]() {
    kload.load(kst);
    vload.load(vst);
  };
  auto commit = [&]() {
#pragma unroll
    for (int ps = 0; ps < G::NP; ++ps) {
      st4(&Ks[GenStager<DH>::lds_off(tid, ps)], kst[ps]);
      st4(&Vs[GenStager<DH>::lds_off(tid, ps)], vst[ps]);
    }
  };

  f32x16 o[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) o[n] = zero16();
  f32x16 negm = zero16();
  float mref = 0.f, l_run = 0.f;
  const int ntile = (p.J + TL - 1) / TL;
  const int nfull = p.J / TL;
  const ScoreTiles stl(p.I, p.J);
  const int64_t sc_kstep = (int64_t)stl.nqt * 1024;  // floats between consecutive 32-key blocks
  float* sc_ptr = nullptr;
  if (KEEP) sc_ptr = p.scores + ((int64_t)bh * stl.nkb * stl.nqt + (qb * NWAVE + wave)) * 1024 + 4 * hf * 32 + ln;

  auto tile = [&](const int t, auto ragged_c) {
    constexpr bool RAGGED = decltype(ragged_c)::value;
    constexpr bool PF = G::PF_FWD;
    if (!PF) prefetch();
    __syncthreads();
    commit();
    __syncthreads();
    if (PF && t + 1 < ntile) prefetch();

    f32x16 s[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      s[u] = KEEP ? zero16() : negm;
      const float* kr = &Ks[(32 * u + ln) * LS + HD * hf];
      float4 a = ld4(kr);
#pragma unroll
      for (int s4 = 0; s4 < HD / 4; ++s4) {
        float4 nx = a;
        if (s4 + 1 < HD / 4) nx = ld4(kr + 4 * (s4 + 1));   // the next k-block's fragment, one step ahead of its MFMAs
#pragma unroll
        for (int e = 0; e < 4; ++e) s[u] = mfma32(f4(a, e), qreg[4 * s4 + e], s[u]);
        a = nx;
      }
    }
    if (KEEP) {
#pragma unroll
      for (int u = 0; u < NS; ++u) {
        float* t0 = sc_ptr + (int64_t)(NS * t + u) * sc_kstep;
#pragma unroll
        for (int r = 0; r < 16; ++r) __builtin_nontemporal_store(s[u][r], t0 + acc_row(r, 0) * 32);
      }
    }
    if (RAGGED) {
#pragma unroll
      for (int u = 0; u < NS; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[u][r] = (t * TL + 32 * u + acc_row(r, hf) < p.J) ? s[u][r] : -INFINITY;
    }
    float mx = gmax3(s[0][0], s[0][1], s[0][2]);
#pragma unroll
    for (int r = 3; r + 1 < 16; r += 2) mx = gmax3(mx, s[0][r], s[0][r + 1]);
    mx = __builtin_fmaxf(mx, s[0][15]);
#pragma unroll
    for (int u = 1; u < NS; ++u)
#pragma unroll
      for (int r = 0; r < 16; r += 2) mx = gmax3(mx, s[u][r], s[u][r + 1]);
    mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (KEEP) mx -= mref;
    if (t == 0 || __any(mx > TAU)) {   // rare after the first tile
      const float d = t == 0 ? mx : __builtin_fmaxf(mx, 0.f);
      if (t != 0) {
        const float alpha = __builtin_amdgcn_exp2f(-d);
        l_run *= alpha;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[n][r] *= alpha;
      }
      mref += d;
      if (!KEEP) {
#pragma unroll
        for (int u = 0; u < NS; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) s[u][r] -= d;
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[r] = -mref;
      }
    }
    f32x2 ls = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NS; ++u) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[u][r] = __builtin_amdgcn_exp2f(KEEP ? s[u][r] - mref : s[u][r]);
#pragma unroll
      for (int r = 0; r < 16; r += 2) ls += (f32x2){s[u][r], s[u][r + 1]};
    }
    l_run += ls.x + ls.y;
    // O^T += V^T P^T, the V column fragments of step r + 1 read under the MFMAs of step r
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      float c[NT], nx[NT];
      {
        const float* vc = &Vs[(32 * u + acc_row(0, hf)) * LS + ln];
#pragma unroll
        for (int n = 0; n < NT; ++n) c[n] = vc[32 * n];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (r + 1 < 16) {
          const float* vc = &Vs[(32 * u + acc_row(r + 1, hf)) * LS + ln];
#pragma unroll
          for (int n = 0; n < NT; ++n) nx[n] = vc[32 * n];
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) o[n] = mfma32(c[n], s[u][r], o[n]);
#pragma unroll
        for (int n = 0; n < NT; ++n) c[n] = nx[n];
      }
    }
  };

  if (G::PF_FWD) prefetch();
  for (int t = 0; t < nfull; ++t) tile(t, std::false_type{});
  if (nfull < ntile) tile(nfull, std::true_type{});

  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.f / l_tot;
  if (qvalid) {
    float* op = p.o + (int64_t)b * p.os.sb + (int64_t)qi * p.os.st + (int64_t)h * p.os.sh + 4 * hf;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        st4(op + 32 * n + 8 * g, make_float4(o[n][4 * g] * inv, o[n][4 * g + 1] * inv, o[n][4 * g + 2] * inv, o[n][4 * g + 3] * inv));
    if (hf == 0) {
      float* sp = p.stats + (((int64_t)b * p.H + h) * p.I + qi) * 2;
      sp[0] = mref;
      sp[1] = l_tot;
    }
  }
}

// ------------------------------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(256) void attn_bwd_delta_gen_kernel(BwdParams p) {
  constexpr int LPR = DeltaGeom<DH>::LPR;
  const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  const int64_t nrow = (int64_t)p.B * p.H * p.I;
  const int c = (threadIdx.x % LPR) * 4;
  float acc = 0.f;
  if (row < nrow && (LPR * 4 == DH || c < DH)) {
    const int i = (int)(row % p.I);
    const int64_t bh = row / p.I;
    const int h = (int)(bh % p.H), b = (int)(bh / p.H);
    const float4 a = ld4(p.o + (int64_t)b * p.os.sb + (int64_t)i * p.os.st + (int64_t)h * p.os.sh + c);
    const float4 g = ld4(p.d_o + (int64_t)b * p.dos.sb + (int64_t)i * p.dos.st + (int64_t)h * p.dos.sh + c);
    acc = a.x * g.x + a.y * g.y + a.z * g.z + a.w * g.w;
  }
#pragma unroll
  for (int o = LPR / 2; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (row < nrow && (threadIdx.x % LPR) == 0) p.delta[row] = acc;
}

// ------------------------------------------------------------------------------------------------
// dQ: query on the lane (the forward's skeleton)
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(WG, GenGeom<DH>::WAVES_DQ) void attn_bwd_dq_gen_kernel(BwdParams p) {
  using G = GenGeom<DH>;
  constexpr int HD = G::HD, LS = G::LS, NT = G::NT, TL = G::TL, NS = G::NS;
  __shared__ __attribute__((aligned(16))) float smem[2 * TL * LS + TL];
  float* Ks = smem;
  float* Vs = smem + TL * LS;
  float* Kfill = smem + 2 * TL * LS;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  const int wg = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));
  const int qb = __builtin_amdgcn_readfirstlane(wg % p.nqblk);
  const int bh = __builtin_amdgcn_readfirstlane(wg / p.nqblk);
  const int h = __builtin_amdgcn_readfirstlane(bh % p.H), b = __builtin_amdgcn_readfirstlane(bh / p.H);
  const int qi = qb * BLK + wave * 32 + ln;
  const bool qvalid = qi < p.I;

  const float qscale = p.scale * AMK_LOG2E;
  constexpr int PK = G::PK_DQ, CUT = HD / 4 - PK;    // dO row: float4 [0, CUT) in registers, the rest parked
  __shared__ __attribute__((aligned(16))) float4 gpark[PK > 0 ? NWAVE * PK * 64 : 1];
  const RowPark<PK> gpk(gpark, wave, lane);
  float qreg[HD], greg[HD];
  float m_q = INFINITY, linv_q = 0.f, delta_q = 0.f;
  {
    const float* qp = p.q + (int64_t)b * p.qs.sb + (int64_t)qi * p.qs.st + (int64_t)h * p.qs.sh + HD * hf;
    const float* gp = p.d_o + (int64_t)b * p.dos.sb + (int64_t)qi * p.dos.st + (int64_t)h * p.dos.sh + HD * hf;
#pragma unroll
    for (int s4 = 0; s4 < HD / 4; ++s4) {
      const float4 t = qvalid ? ld4(qp + 4 * s4) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 g = qvalid ? ld4(gp + 4 * s4) : make_float4(0.f, 0.f, 0.f, 0.f);
      qreg[4 * s4 + 0] = t.x * qscale; qreg[4 * s4 + 1] = t.y * qscale;
      qreg[4 * s4 + 2] = t.z * qscale; qreg[4 * s4 + 3] = t.w * qscale;
      if (s4 >= CUT) gpk.put(s4 - CUT, g);
      else { greg[4 * s4 + 0] = g.x; greg[4 * s4 + 1] = g.y; greg[4 * s4 + 2] = g.z; greg[4 * s4 + 3] = g.w; }
    }
    if (qvalid) {
      const int64_t row = ((int64_t)b * p.H + h) * p.I + qi;
      m_q = p.stats[2 * row];
      linv_q = 1.f / p.stats[2 * row + 1];
      delta_q = p.delta[row];
    }
  }
  const float* kbase = p.k + (int64_t)b * p.ks.sb + (int64_t)h * p.ks.sh;
  const float* vbase = p.v + (int64_t)b * p.vs.sb + (int64_t)h * p.vs.sh;
  const uint8_t* kmask = p.key_mask ? p.key_mask + (int64_t)b * p.J : nullptr;
  const uint8_t* cmrow = CAUSAL ? p.causal_mask + (int64_t)qi * p.J : nullptr;

  float4 kst[G::NP], vst[G::NP];
  float fillst = 0.f;
  GenStager<DH> kload, vload;
  kload.init(kbase, p.ks.st, p.J, tid);
  vload.init(vbase, p.vs.st, p.J, tid);
  auto prefetch = [&](int j0) {
    kload.load(kst);
    vload.load(vst);
    if (tid < TL) {
      const int j = j0 + tid;
      float f = 0.f;
      if (j >= p.J) f = -INFINITY;
      else if (kmask && kmask[j] == 0) f = AMK_FILL_MASKED;
      fillst = f;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int ps = 0; ps < G::NP; ++ps) {
      st4(&Ks[GenStager<DH>::lds_off(tid, ps)], kst[ps]);
      st4(&Vs[GenStager<DH>::lds_off(tid, ps)], vst[ps]);
    }
    if (tid < TL) Kfill[tid] = fillst;
  };

  f32x16 dq[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) dq[n] = zero16();
  const int ntile = (p.J + TL - 1) / TL;
  constexpr bool PF = G::PF_DQ;
  if (PF) prefetch(0);
  for (int t = 0; t < ntile; ++t) {
    const int j0 = t * TL;
    if (!PF) prefetch(j0);
    __syncthreads();
    commit();
    __syncthreads();
    if (PF && t + 1 < ntile) prefetch(j0 + TL);
    unsigned cbits[NS] = {};
    if constexpr (CAUSAL && G::MASK_BITS) {
      if (qvalid) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
          for (int u = 0; u < NS; ++u) {
            const int j = j0 + 32 * u + acc_row(r, hf);
            if (j < p.J && cmrow[j]) cbits[u] |= 1u << r;
          }
      }
    }
    bool plain = false;   // wave-uniform: nothing in this tile is filled
    if constexpr (G::SKIP_FILLS && !CAUSAL) plain = kmask == nullptr && j0 + TL <= p.J;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      f32x16 s = zero16(), dp = zero16();
      const float* kr = &Ks[(32 * u + ln) * LS + HD * hf];
      const float* vr = &Vs[(32 * u + ln) * LS + HD * hf];
#pragma unroll
      for (int s4 = 0; s4 < HD / 4; ++s4) {
        const float4 a = ld4(kr + 4 * s4);
        const float4 c = ld4(vr + 4 * s4);
        const float4 gk = s4 < CUT ? c : gpk.get(s4 - CUT);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s = mfma32(f4(a, e), qreg[4 * s4 + e], s);
          dp = mfma32(f4(c, e), s4 < CUT ? greg[4 * s4 + e] : f4(gk, e), dp);
        }
      }
      if (plain) {  // dS^T = P^T o (dP^T - delta)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pr = __builtin_amdgcn_exp2f(s[r] - m_q) * linv_q;
          s[r] = pr * (dp[r] - delta_q);
        }
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 f = ld4(&Kfill[32 * u + 8 * g + 4 * hf]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * g + e;
            const float fe = f4(f, e);
            bool filled = fe != 0.f;
            float tt = filled ? fe : s[r];
            if constexpr (CAUSAL && G::MASK_BITS) {
              if ((cbits[u] >> r) & 1u) { tt = AMK_FILL_MASKED; filled = true; }
            } else if (CAUSAL) {
              const int j = j0 + 32 * u + acc_row(r, hf);
              if (qvalid && j < p.J && cmrow[j]) { tt = AMK_FILL_MASKED; filled = true; }
            }
            const float pr = __builtin_amdgcn_exp2f(tt - m_q) * linv_q;
            s[r] = filled ? 0.f : pr * (dp[r] - delta_q);  // dS^T (no gradient through fills)
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* kc = &Ks[(32 * u + acc_row(r, hf)) * LS + ln];
#pragma unroll
        for (int n = 0; n < NT; ++n) dq[n] = mfma32(kc[32 * n], s[r], dq[n]);
      }
    }
  }
  if (qvalid) {
    float* dp_ = p.dq + (int64_t)b * p.dqs.sb + (int64_t)qi * p.dqs.st + (int64_t)h * p.dqs.sh + 4 * hf;
    const float sc = p.scale;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        st4(dp_ + 32 * n + 8 * g, make_float4(dq[n][4 * g] * sc, dq[n][4 * g + 1] * sc, dq[n][4 * g + 2] * sc, dq[n][4 * g + 3] * sc));
  }
}

// ------------------------------------------------------------------------------------------------
// dK, dV: key on the lane (a wave owns 32 keys; k, v in registers).  PART = DKDV_DV / DKDV_DK computes one of the two
// (what the other needs alone -- v rows, dP, the deltas -- is dead code there and drops out).
template <int DH, bool CAUSAL, int PART = DKDV_BOTH>
__global__ __launch_bounds__(WG, GenGeom<DH>::waves_dkdv(CAUSAL)) void attn_bwd_dkdv_gen_kernel(BwdParams p) {
  using G = GenGeom<DH>;
  constexpr int HD = G::HD, LS = G::LS, NT = G::NT, TL = G::TL, NS = G::NS;
  __shared__ __attribute__((aligned(16))) float smem[2 * TL * LS + 3 * TL];
  float* Qs = smem;
  float* Gs = smem + TL * LS;
  float* Ms = smem + 2 * TL * LS;
  float* Ls = Ms + TL;
  float* Ds = Ls + TL;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  const int wg = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));
  const int kb = __builtin_amdgcn_readfirstlane(wg % p.nkblk);
  const int bh = __builtin_amdgcn_readfirstlane(wg / p.nkblk);
  const int h = __builtin_amdgcn_readfirstlane(bh % p.H), b = __builtin_amdgcn_readfirstlane(bh / p.H);
  const int kj = kb * BLK + wave * 32 + ln;
  const bool kvalid = kj < p.J;

  constexpr int PK = PART == DKDV_DK ? G::PK_DK : 0, CUT = HD / 4 - PK;   // v row: float4 [0, CUT) in registers
  __shared__ __attribute__((aligned(16))) float4 vpark[PK > 0 ? NWAVE * PK * 64 : 1];
  const RowPark<PK> vpk(vpark, wave, lane);
  float kreg[HD], vreg[HD];
  {
    const float* kp = p.k + (int64_t)b * p.ks.sb + (int64_t)kj * p.ks.st + (int64_t)h * p.ks.sh + HD * hf;
    const float* vp = p.v + (int64_t)b * p.vs.sb + (int64_t)kj * p.vs.st + (int64_t)h * p.vs.sh + HD * hf;
#pragma unroll
    for (int s4 = 0; s4 < HD / 4; ++s4) {
      const float4 a = kvalid ? ld4(kp + 4 * s4) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 c = kvalid ? ld4(vp + 4 * s4) : make_float4(0.f, 0.f, 0.f, 0.f);
      kreg[4 * s4 + 0] = a.x; kreg[4 * s4 + 1] = a.y; kreg[4 * s4 + 2] = a.z; kreg[4 * s4 + 3] = a.w;
      if (s4 >= CUT) vpk.put(s4 - CUT, c);
      else { vreg[4 * s4 + 0] = c.x; vreg[4 * s4 + 1] = c.y; vreg[4 * s4 + 2] = c.z; vreg[4 * s4 + 3] = c.w; }
    }
  }
  float kfill = 0.f;
  if (!kvalid) kfill = -INFINITY;
  else if (p.key_mask && p.key_mask[(int64_t)b * p.J + kj] == 0) kfill = AMK_FILL_MASKED;
  bool plain = false;   // wave-uniform: none of this wave's keys is filled
  if constexpr (G::SKIP_FILLS && !CAUSAL) plain = __all(kfill == 0.f);

  const float* qbase = p.q + (int64_t)b * p.qs.sb + (int64_t)h * p.qs.sh;
  const float* gbase = p.d_o + (int64_t)b * p.dos.sb + (int64_t)h * p.dos.sh;
  const float* stbase = p.stats + ((int64_t)b * p.H + h) * p.I * 2;
  const float* dlbase = p.delta + ((int64_t)b * p.H + h) * p.I;

  float4 qst[G::NP], gst[G::NP];
  float mst = 0.f, lst = 0.f, dst = 0.f;
  GenStager<DH> qload, gload;
  qload.init(qbase, p.qs.st, p.I, tid);
  gload.init(gbase, p.dos.st, p.I, tid);
  auto prefetch = [&](int i0) {
    qload.load(qst);
    gload.load(gst);
    if (tid < TL) {
      const int i = i0 + tid;
      if (i < p.I) {
        mst = stbase[2 * i];
        lst = 1.f / stbase[2 * i + 1];
        dst = dlbase[i];
      } else {
        mst = INFINITY; lst = 0.f; dst = 0.f;
      }
    }
  };
  auto commit = [&]() {
    const float sc = p.scale * AMK_LOG2E;
#pragma unroll
    for (int ps = 0; ps < G::NP; ++ps) {
      st4(&Qs[GenStager<DH>::lds_off(tid, ps)], make_float4(qst[ps].x * sc, qst[ps].y * sc, qst[ps].z * sc, qst[ps].w * sc));
      st4(&Gs[GenStager<DH>::lds_off(tid, ps)], gst[ps]);
    }
    if (tid < TL) { Ms[tid] = mst; Ls[tid] = lst; Ds[tid] = dst; }
  };

  f32x16 dk[NT], dv[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) { dk[n] = zero16(); dv[n] = zero16(); }
  const uint8_t* cmcol = CAUSAL ? p.causal_mask + kj : nullptr;

  const int ntile = (p.I + TL - 1) / TL;
  constexpr bool PF = PART != DKDV_DK || G::PF_DK;
  if (PF) prefetch(0);
  for (int t = 0; t < ntile; ++t) {
    const int i0 = t * TL;
    if (!PF) prefetch(i0);
    __syncthreads();
    commit();
    __syncthreads();
    if (PF && t + 1 < ntile) prefetch(i0 + TL);
    unsigned cbits[NS] = {};
    if constexpr (CAUSAL && G::MASK_BITS) {
      if (kvalid) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
          for (int u = 0; u < NS; ++u) {
            const int i = i0 + 32 * u + acc_row(r, hf);
            if (i < p.I && cmcol[(int64_t)i * p.J]) cbits[u] |= 1u << r;
          }
      }
    }
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      f32x16 s = zero16(), dp = zero16();
      const float* qr = &Qs[(32 * u + ln) * LS + HD * hf];
      const float* gr = &Gs[(32 * u + ln) * LS + HD * hf];
#pragma unroll
      for (int s4 = 0; s4 < HD / 4; ++s4) {
        const float4 a = ld4(qr + 4 * s4);
        const float4 c = ld4(gr + 4 * s4);
        const float4 vk = s4 < CUT ? c : vpk.get(s4 - CUT);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s = mfma32(f4(a, e), kreg[4 * s4 + e], s);
          dp = mfma32(f4(c, e), s4 < CUT ? vreg[4 * s4 + e] : f4(vk, e), dp);
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 m4 = ld4(&Ms[32 * u + 8 * g + 4 * hf]);
        const float4 l4 = ld4(&Ls[32 * u + 8 * g + 4 * hf]);
        const float4 d4 = ld4(&Ds[32 * u + 8 * g + 4 * hf]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          if (plain) {
            const float pr = __builtin_amdgcn_exp2f(s[r] - f4(m4, e)) * f4(l4, e);
            s[r] = pr;                                    // P
            dp[r] = pr * (dp[r] - f4(d4, e));             // dS
            continue;
          }
          bool filled = kfill != 0.f;
          float tt = filled ? kfill : s[r];
          if constexpr (CAUSAL && G::MASK_BITS) {
            if ((cbits[u] >> r) & 1u) { tt = AMK_FILL_MASKED; filled = true; }
          } else if (CAUSAL) {
            const int i = i0 + 32 * u + acc_row(r, hf);
            if (kvalid && i < p.I && cmcol[(int64_t)i * p.J]) { tt = AMK_FILL_MASKED; filled = true; }
          }
          const float pr = __builtin_amdgcn_exp2f(tt - f4(m4, e)) * f4(l4, e);
          s[r] = pr;                                      // P
          dp[r] = filled ? 0.f : pr * (dp[r] - f4(d4, e));  // dS (no gradient through fills)
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* gc = &Gs[(32 * u + acc_row(r, hf)) * LS + ln];
        const float* qc = &Qs[(32 * u + acc_row(r, hf)) * LS + ln];
        if constexpr (G::DV_FIRST) {
#pragma unroll
          for (int n = 0; n < NT; ++n)
            if (PART != DKDV_DK) dv[n] = mfma32(gc[32 * n], s[r], dv[n]);
#pragma unroll
          for (int n = 0; n < NT; ++n)
            if (PART != DKDV_DV) dk[n] = mfma32(qc[32 * n], dp[r], dk[n]);
        } else {
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            if (PART != DKDV_DK) dv[n] = mfma32(gc[32 * n], s[r], dv[n]);
            if (PART != DKDV_DV) dk[n] = mfma32(qc[32 * n], dp[r], dk[n]);
          }
        }
      }
    }
  }
  if (kvalid) {
    float* dkp = p.dk + (int64_t)b * p.dks.sb + (int64_t)kj * p.dks.st + (int64_t)h * p.dks.sh + 4 * hf;
    float* dvp = p.dv + (int64_t)b * p.dvs.sb + (int64_t)kj * p.dvs.st + (int64_t)h * p.dvs.sh + 4 * hf;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (PART != DKDV_DV)
          st4(dkp + 32 * n + 8 * g, make_float4(dk[n][4 * g] * AMK_LN2, dk[n][4 * g + 1] * AMK_LN2, dk[n][4 * g + 2] * AMK_LN2, dk[n][4 * g + 3] * AMK_LN2));
        if (PART != DKDV_DK)
          st4(dvp + 32 * n + 8 * g, make_float4(dv[n][4 * g], dv[n][4 * g + 1], dv[n][4 * g + 2], dv[n][4 * g + 3]));
      }
  }
}

// ------------------------------------------------------------------------------------------------
// Launchers of one head dim: defined here, instantiated explicitly by the translation unit that owns the head dim.
template <int DH>
void launch_fwd_gen_dh(const FwdParams& p, int64_t nwg, hipStream_t st) {
  if (p.causal_mask) hipLaunchKernelGGL((attn_fwd_gen_kernel<DH, true>), dim3((unsigned)nwg), dim3(WG), 0, st, p);
  else if (!p.key_mask && p.scores) hipLaunchKernelGGL((attn_fwd_gen_plain_kernel<DH, true>), dim3((unsigned)nwg), dim3(WG), 0, st, p);
  else if (!p.key_mask) hipLaunchKernelGGL((attn_fwd_gen_plain_kernel<DH, false>), dim3((unsigned)nwg), dim3(WG), 0, st, p);
  else hipLaunchKernelGGL((attn_fwd_gen_kernel<DH, false>), dim3((unsigned)nwg), dim3(WG), 0, st, p);
}

template <int DH>
void launch_bwd_gen_dh(const BwdParams& p, int stages, hipStream_t st) {
  const int64_t nrow = (int64_t)p.B * p.H * p.I;
  const int64_t nq = (int64_t)p.B * p.H * p.nqblk, nk = (int64_t)p.B * p.H * p.nkblk;
  constexpr int RPB = 256 / DeltaGeom<DH>::LPR;
  if (stages & AMK_ATTN_BWD_DELTA)
    hipLaunchKernelGGL(attn_bwd_delta_gen_kernel<DH>, dim3((unsigned)((nrow + RPB - 1) / RPB)), dim3(256), 0, st, p);
  if (stages & AMK_ATTN_BWD_DKDV) {
    if constexpr (GenGeom<DH>::SPLIT_DKDV) {   // two passes: dV, then dK
      if (p.causal_mask) {
        hipLaunchKernelGGL((attn_bwd_dkdv_gen_kernel<DH, true, DKDV_DV>), dim3((unsigned)nk), dim3(WG), 0, st, p);
        hipLaunchKernelGGL((attn_bwd_dkdv_gen_kernel<DH, true, DKDV_DK>), dim3((unsigned)nk), dim3(WG), 0, st, p);
      } else {
        hipLaunchKernelGGL((attn_bwd_dkdv_gen_kernel<DH, false, DKDV_DV>), dim3((unsigned)nk), dim3(WG), 0, st, p);
        hipLaunchKernelGGL((attn_bwd_dkdv_gen_kernel<DH, false, DKDV_DK>), dim3((unsigned)nk), dim3(WG), 0, st, p);
      }
    } else {
      if (p.causal_mask) hipLaunchKernelGGL((attn_bwd_dkdv_gen_kernel<DH, true>), dim3((unsigned)nk), dim3(WG), 0, st, p);
      else hipLaunchKernelGGL((attn_bwd_dkdv_gen_kernel<DH, false>), dim3((unsigned)nk), dim3(WG), 0, st, p);
    }
  }
  if (stages & AMK_ATTN_BWD_DQ) {
    if (p.causal_mask) hipLaunchKernelGGL((attn_bwd_dq_gen_kernel<DH, true>), dim3((unsigned)nq), dim3(WG), 0, st, p);
    else hipLaunchKernelGGL((attn_bwd_dq_gen_kernel<DH, false>), dim3((unsigned)nq), dim3(WG), 0, st, p);
  }
}

// (head dim 64 has the backward launcher only: its forward is attn_fwd.hip's)
#define AMK_ATTN_GEN_BWD_INSTANTIATE(DH) template void launch_bwd_gen_dh<DH>(const BwdParams& p, int stages, hipStream_t st);
#define AMK_ATTN_GEN_BWD_EXTERN(DH) extern AMK_ATTN_GEN_BWD_INSTANTIATE(DH)
#define AMK_ATTN_GEN_INSTANTIATE(DH)                                                            \
  template void launch_fwd_gen_dh<DH>(const FwdParams& p, int64_t nwg, hipStream_t st);        \
  AMK_ATTN_GEN_BWD_INSTANTIATE(DH)
#define AMK_ATTN_GEN_EXTERN(DH)                                                                 \
  extern template void launch_fwd_gen_dh<DH>(const FwdParams& p, int64_t nwg, hipStream_t st); \
  AMK_ATTN_GEN_BWD_EXTERN(DH)

}  // namespace amk_attn
