// The kept-scores one-pass attention backward of attn_bwd_fused.hip (head dim 64, 256 keys per workgroup) with its
// dV^T += dO^T P and dK^T += Q^T dS products on SPLIT-BF16 MFMA ("bf16x6", attn_fwd_x6.hip): AMK_ATTN_BWD_X6.
//
// Everything else is attn_bwd_fused_kernel<64, 8, 1, true, DQ, CAUSAL>, statement for statement: the kept scores come
// back from HBM, dP = dO V^T - delta runs on v_mfma_f32_32x32x2_f32 (A = f32 dO rows from LDS, B = v registers), P and
// dS are formed by the same arithmetic on the same fills, dS crosses LDS in f32 and dQ = dS K runs on
// v_mfma_f32_16x16x4_f32 -- so dq is bit for bit the f32 kernel's (under DQ = 1; with atomics up to arrival order).
//
// What changes is the half of the matrix time that sums over the tile's 32 queries:
//   q * scale * log2 e and dO are split into three bf16 planes (x = h + m + l, split4) between their global load and
//     the LDS store, once per tile per workgroup (8 elements per thread), and stored as transposed-read images
//     [32 queries][TSTR] as they arrive (attn_bf16.hip); the f32 Qs image is not needed with kept scores and is gone;
//   P and dS are split in registers: registers 8t .. 8t+7 of the 32x32 accumulator are the 8 queries of k-slot t
//     of this lane's key -- the packed-accumulator B operand of attn_bf16.hip, three planes each;
//   A fragments (8 queries of one head dim, in that order) come by ds_read_b64_tr_b16 from the plane images;
//   six partial products per block, smallest first, the two 32-wide dim tiles of a product alternating (mfma6x2 of
//     attn_fwd_x6.hip: no MFMA waits on its predecessor): 48 v_mfma_f32_32x32x16_bf16 of 32 cycles for 64 32x32x2
//     f32 ones of 64 cycles and 64 scalar ds_read_b32.
// LDS: Gs 8.5 + K 68 + dS 32.5 + row constants 0.5 + six plane images 36 = 145.5 KiB: one workgroup per CU, as the
// f32 kernel in fact runs (118 KiB), so the launch bounds give the wave its 256 registers.
#include "attn_common.h"
#include "amk_bf16.h"

namespace amk_attn {

namespace {

constexpr int DH = 64, NW = 8, TQ = 32, NT = 64 * NW, KB = 32 * NW, HD = DH / 2, LS = DH + 4, NTILE = DH / 32;
constexpr int DS_STRIDE = KB + 4, KPG = KB / 4;
constexpr int TSTR = 96;                 // bf16 per row of a transposed-read image (64 + 32): 192 B
constexpr int PIMG = TQ * TSTR;          // one plane image
constexpr int F32_FLOATS = TQ * LS + KB * LS + TQ * DS_STRIDE + 4 * TQ;
constexpr int LDS_BYTES = F32_FLOATS * 4 + 6 * PIMG * 2;
static_assert(F32_FLOATS % 4 == 0 && LDS_BYTES <= 160 * 1024, "16-byte aligned plane images inside the CU's LDS");

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// c0 / c1 (dims 0..31 / 32..63 x this lane's key) += X^T acc over the 16 queries of k-slot ks: X the plane images of
// dO or q, acc the P or dS accumulator
__device__ __forceinline__ void x6_pair(const __bf16* img, const f32x16& acc, int ks, int lane, f32x16& c0, f32x16& c1) {
  bf16x8 b[3], a0[3], a1[3];
  split8(acc, 8 * ks, b);   // registers 8 ks .. of the accumulator: the B operand's k-slot
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    a0[q] = tr_frag_packed<TSTR>(img + q * PIMG, ks, 0, lane);
    a1[q] = tr_frag_packed<TSTR>(img + q * PIMG, ks, 32, lane);
  }
  mfma6x2(a0, b, c0, a1, b, c1);
}

// DQ and CAUSAL as in attn_bwd_fused_kernel
template <int DQ, bool CAUSAL>
__global__ __launch_bounds__(NT, 1) void attn_bwd_fused_x6_kernel(BwdParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Gs = smem;                           // [TQ][LS]  dO, f32 rows: the A operand of dP
  float* Kc = Gs + TQ * LS;                   // [KB][LS]  this workgroup's K rows
  float* dSl = Kc + KB * LS;                  // [TQ][DS_STRIDE]   dS of the current tile
  float* Ms = dSl + TQ * DS_STRIDE;
  float* Ls = Ms + TQ;
  float* Ds = Ls + TQ;    // MINUS delta: the initial accumulator of the dP chain
  float* MLs = Ds + TQ;   // m + log2 l
  __bf16* Qp = reinterpret_cast<__bf16*>(MLs + TQ);   // 3 x [TQ][TSTR]  planes of q * scale * log2 e
  __bf16* Gp = Qp + 3 * PIMG;                         // 3 x [TQ][TSTR]  planes of dO

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ln = lane & 31, hf = lane >> 5;

  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int kb = wg % p.nkblk;
  const int bh = wg / p.nkblk;
  const int h = bh % p.H, b = bh / p.H;
  const int kj = kb * KB + wave * 32 + ln;  // this lane's key row
  const bool kvalid = kj < p.J;

  const float* kbase = p.k + (int64_t)b * p.ks.sb + (int64_t)h * p.ks.sh;
  const float* vbase = p.v + (int64_t)b * p.vs.sb + (int64_t)h * p.vs.sh;

  float vreg[HD];   // B operand of dP held for the whole kernel: v of this lane's key
  {
    const float* vp = vbase + (int64_t)kj * p.vs.st + HD * hf;
#pragma unroll
    for (int s4 = 0; s4 < HD / 4; ++s4) {
      const float4 c = kvalid ? ld4(vp + 4 * s4) : make_float4(0.f, 0.f, 0.f, 0.f);
      vreg[4 * s4 + 0] = c.x; vreg[4 * s4 + 1] = c.y; vreg[4 * s4 + 2] = c.z; vreg[4 * s4 + 3] = c.w;
    }
  }
  float kfill = 0.f;  // 0 keep, -1e9*log2e masked key, -inf beyond the sequence
  if (!kvalid) kfill = -INFINITY;
  else if (p.key_mask && p.key_mask[(int64_t)b * p.J + kj] == 0) kfill = AMK_FILL_MASKED;
  const bool plain = !CAUSAL && __all(kfill == 0.f);  // wave-uniform: none of this wave's scores is filled
  // CAUSAL: this lane's key column of the mask, requested a tile ahead (unconditional loads at clamped rows)
  const uint8_t* cm_col = CAUSAL ? p.causal_mask + min(kj, p.J - 1) : nullptr;
  unsigned cm_raw[16];
  unsigned cbits = 0xffffu;   // bit r: the score of register r (query acc_row(r, hf)) is kept
  auto load_cmask = [&](int i0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) cm_raw[r] = cm_col[(int64_t)min(i0 + acc_row(r, hf), p.I - 1) * p.J];
  };
  auto fold_cmask = [&]() {
    cbits = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) cbits |= (cm_raw[r] == 0 ? 1u : 0u) << r;   // (a non-zero byte masks)
  };

  // K rows of the whole workgroup -> LDS once (B operand of the dQ product)
  using KStager = RowStagerT<KB / 2, NT, DH>;
  using QStager = RowStagerT<TQ, NT, DH>;
  static_assert(QStager::NP == 1, "one 16-byte piece of q and of dO per thread and tile");
  const int srow = (unsigned)tid / QStager::F4R, scol = ((unsigned)tid % QStager::F4R) * 4;
  {
    KStager kl;
    const float* kblk = kbase + (int64_t)kb * KB * p.ks.st;
    kl.init(kblk, p.ks.st, min(KB, p.J - kb * KB), tid);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      float4 t[KStager::NP];
      kl.load(t);
#pragma unroll
      for (int ps = 0; ps < KStager::NP; ++ps) st4(&Kc[((KB / 2) * half + srow + KStager::RP * ps) * LS + scol], t[ps]);
    }
  }

  const float* qbase = p.q + (int64_t)b * p.qs.sb + (int64_t)h * p.qs.sh;
  const float* gbase = p.d_o + (int64_t)b * p.dos.sb + (int64_t)h * p.dos.sh;
  const float* stbase = p.stats + ((int64_t)b * p.H + h) * p.I * 2;
  const float* dlbase = p.delta + ((int64_t)b * p.H + h) * p.I;
  float* dqbase = (DQ == 1 && p.nkblk > 1 ? p.dq_part + (int64_t)kb * p.B * p.I * p.H * DH : p.dq) +
                  (int64_t)b * p.dqs.sb + (int64_t)h * p.dqs.sh;
  // dq rows through a buffer descriptor: rows beyond the sequence are dropped by the hardware range check
  const __amdgpu_buffer_rsrc_t dq_rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)dqbase, 0, (int)(((int64_t)(p.I - 1) * p.dqs.st + DH) * 4), 0x00020000);

  // kept scores: this wave's 32 keys x all query tiles are nqt consecutive 4-KiB tiles; a descriptor of zero records
  // (key block beyond the forward's tiles) reads zeros
  __amdgpu_buffer_rsrc_t sc_rsrc;
  int sc_voff;
  {
    const ScoreTiles stl(p.I, p.J);
    const int kb32 = kb * NW + wave;
    const float* tiles = p.scores + ((int64_t)bh * stl.nkb + min(kb32, stl.nkb - 1)) * stl.nqt * 1024;
    sc_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)tiles, 0, kb32 < stl.nkb ? stl.nqt * 4096 : 0, 0x00020000);
    sc_voff = ln * 128 + hf * 16;  // row = this lane's key, 4 queries of register group g at +32 g bytes
  }
  float4 sk[4];  // the score registers of the coming tile (16 queries of this lane's key)
  auto load_scores = [&](int qt) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
      sk[g] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(sc_rsrc, sc_voff + qt * 4096 + 32 * g, 0, 2));
  };

  float4 qst[1], gst[1];
  QStager qload, gload;
  qload.init(qbase, p.qs.st, p.I, tid);
  gload.init(gbase, p.dos.st, p.I, tid);
  // No branch around any vector-memory instruction of the tile loop (see attn_bwd_fused.hip)
  float2 ml_raw = make_float2(0.f, 1.f);
  float dl_raw = 0.f;
  bool row_ok = false;
  auto prefetch = [&](int qt) {  // loads only: whatever consumes them waits in commit(), a tile later
    qload.seek(qt, p.qs.st, tid);
    gload.seek(qt, p.dos.st, tid);
    qload.load(qst);
    gload.load(gst);
    const int i = qt * TQ + (tid & (TQ - 1));
    const int ic = min(i, p.I - 1);
    ml_raw = *reinterpret_cast<const float2*>(stbase + 2 * ic);
    dl_raw = dlbase[ic];
    row_ok = i < p.I;
  };
  auto commit = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    const float sc = p.scale * AMK_LOG2E;  // the kept scores are in the log2 domain; dK is scaled back by ln 2
    bf16x4 qpl[3], gpl[3];
    split4(make_float4(qst[0].x * sc, qst[0].y * sc, qst[0].z * sc, qst[0].w * sc), qpl);
    split4(gst[0], gpl);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      *reinterpret_cast<bf16x4*>(&Qp[q * PIMG + srow * TSTR + scol]) = qpl[q];
      *reinterpret_cast<bf16x4*>(&Gp[q * PIMG + srow * TSTR + scol]) = gpl[q];
    }
    st4(&Gs[srow * LS + scol], gst[0]);
    if (tid < TQ) {  // LDS stores only.  Rows beyond the sequence: P = exp2(x - inf) * 0 = 0
      Ms[tid] = row_ok ? ml_raw.x : INFINITY;
      Ls[tid] = row_ok ? 1.f / ml_raw.y : 0.f;
      Ds[tid] = row_ok ? -dl_raw : 0.f;
      MLs[tid] = row_ok ? ml_raw.x + __builtin_amdgcn_logf(ml_raw.y) : INFINITY;   // (v_log_f32 is log2)
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  f32x16 dk[NTILE], dv[NTILE];
#pragma unroll
  for (int n = 0; n < NTILE; ++n) { dk[n] = zero16(); dv[n] = zero16(); }

  // dQ product geometry: 16x16x4 MFMA, lane = (column c = l & 15, k-group kg = l >> 4); wave = (16 queries, 16 dims)
  const int c16 = lane & 15, kg = lane >> 4;
  const int qhalf = (unsigned)wave % 2;
  const int dcol0 = 16 * ((unsigned)wave / 2);
  const float* ds_row = &dSl[(16 * qhalf + c16) * DS_STRIDE + KPG * kg];  // A: dS[query][KPG*kg + s]
  const float* kc_col = &Kc[(KPG * kg) * LS + dcol0 + c16];               // B: K[KPG*kg + s][dcol]

  const int ntile = (p.I + TQ - 1) / TQ;
  // Two barriers per query tile, rotated start tiles per (batch, head): as attn_bwd_fused_kernel
  const int rot = (int)(((unsigned)bh * 5u) % (unsigned)ntile);
  auto tile_of = [&](int t) { const int x = t + rot; return x >= ntile ? x - ntile : x; };
  prefetch(rot);
  load_scores(rot);
  if (CAUSAL) { load_cmask(rot * TQ); fold_cmask(); }
  __syncthreads();  // the K block is in LDS
  commit();
  __syncthreads();
  prefetch(tile_of(min(1, ntile - 1)));
  __builtin_amdgcn_s_waitcnt(0x0F70);   // enter the loop with nothing in flight: vmcnt(0)
  for (int t = 0; t < ntile; ++t) {
    const int i0 = tile_of(t) * TQ;

    // ---- dP = dO V^T - delta for the tile's queries x this wave's 32 keys (f32 MFMA), S from the kept scores
    f32x16 s, dp;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 d4 = ld4(&Ds[8 * g + 4 * hf]);
      dp[4 * g + 0] = d4.x; dp[4 * g + 1] = d4.y; dp[4 * g + 2] = d4.z; dp[4 * g + 3] = d4.w;
    }
    {
      const float* gr = &Gs[ln * LS + HD * hf];
#pragma unroll
      for (int s4 = 0; s4 < HD / 4; ++s4) {
        const float4 c = ld4(gr + 4 * s4);
#pragma unroll
        for (int e = 0; e < 4; ++e) dp = mfma32(f4(c, e), vreg[4 * s4 + e], dp);
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      s[4 * g + 0] = sk[g].x; s[4 * g + 1] = sk[g].y; s[4 * g + 2] = sk[g].z; s[4 * g + 3] = sk[g].w;
    }
    // ---- P and dS (register r of this lane is query acc_row(r, hf))
    if (plain) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 ml4 = ld4(&MLs[8 * g + 4 * hf]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const float pr = __builtin_amdgcn_exp2f(s[r] - f4(ml4, e));
          s[r] = pr;
          dp[r] = pr * dp[r];
        }
      }
    } else {
      const float fillv = kfill != 0.f ? kfill : AMK_FILL_MASKED;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 m4 = ld4(&Ms[8 * g + 4 * hf]);
        const float4 l4 = ld4(&Ls[8 * g + 4 * hf]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const bool filled = kfill != 0.f || !((cbits >> r) & 1u);
          const float tt = filled ? fillv : s[r];
          const float pr = __builtin_amdgcn_exp2f(tt - f4(m4, e)) * f4(l4, e);
          s[r] = pr;
          dp[r] = filled ? 0.f : pr * dp[r];
        }
      }
    }
    // ---- dS -> LDS as [query][key], in f32, for the workgroup-wide dQ product
#pragma unroll
    for (int r = 0; r < 16; ++r) dSl[acc_row(r, hf) * DS_STRIDE + 32 * wave + ln] = dp[r];

    // the next tile's scores, ahead of the dV / dK products
    load_scores(tile_of(min(t + 1, ntile - 1)));
    __builtin_amdgcn_sched_barrier(0);  // issued HERE: the compiler otherwise sinks them below the MFMAs

    // ---- dV^T += dO^T P ; dK^T += (q*scale*log2e)^T dS on split-bf16: two 16-query k-slots x 2 products x (2 dim
    //      tiles x 6 partial products, smallest first, the two dim tiles alternating: mfma6x2 of attn_fwd_x6.hip)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      x6_pair(Gp, s, ks, lane, dv[0], dv[1]);
      x6_pair(Qp, dp, ks, lane, dk[0], dk[1]);
    }
    // the next tile's mask bytes: in flight under the dQ product only, folded into bits behind it (sixteen registers
    // that the products above have no room for)
    if (CAUSAL) load_cmask(tile_of(min(t + 1, ntile - 1)) * TQ);
    __syncthreads();  // every wave's dS columns are in LDS; the dO / plane / stats tiles are dead
    commit();         // (the last iteration commits a tile nobody reads)
    prefetch(tile_of(min(t + 2, ntile - 1)));

    // ---- dQ (16 queries x 16 columns per wave) = dS (16 x KB) K (KB x 16): 16x16x4 f32 MFMAs, even / odd k-steps in
    //      two accumulator chains
    f32x4 qacc[2];
    qacc[0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    qacc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s4 = 0; s4 < KPG / 4; ++s4) {
      const float4 a = ld4(ds_row + 4 * s4);
#pragma unroll
      for (int e = 0; e < 4; ++e) qacc[e % 2] = mfma16(f4(a, e), kc_col[(4 * s4 + e) * LS], qacc[e % 2]);
    }
    {
      const float sc = p.scale;
      const int qi0 = i0 + 16 * qhalf + 4 * kg;
      const int off = (int)(((int64_t)qi0 * p.dqs.st + dcol0 + c16) * 4);
      const int rstep = (int)(p.dqs.st * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = qacc[0][r];
        x += qacc[1][r];
        x *= sc;
        if (DQ == 0) __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(x, dq_rsrc, off + r * rstep, 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x), dq_rsrc, off + r * rstep, 0, 0);
      }
    }
    if (CAUSAL) fold_cmask();
    __syncthreads();  // dS consumed, the next dO / plane tiles visible
  }

  if (kvalid) {
    // (the lane id afresh: the two addresses are formed here, nothing of them is held in registers across the tile loop)
    const int le = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int kje = kb * KB + wave * 32 + (le & 31), hfe = le >> 5;
    float* dkp = p.dk + (int64_t)b * p.dks.sb + (int64_t)kje * p.dks.st + (int64_t)h * p.dks.sh + 4 * hfe;
    float* dvp = p.dv + (int64_t)b * p.dvs.sb + (int64_t)kje * p.dvs.st + (int64_t)h * p.dvs.sh + 4 * hfe;
#pragma unroll
    for (int n = 0; n < NTILE; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        st4(dkp + 32 * n + 8 * g, make_float4(dk[n][4 * g] * AMK_LN2, dk[n][4 * g + 1] * AMK_LN2, dk[n][4 * g + 2] * AMK_LN2, dk[n][4 * g + 3] * AMK_LN2));
        st4(dvp + 32 * n + 8 * g, make_float4(dv[n][4 * g], dv[n][4 * g + 1], dv[n][4 * g + 2], dv[n][4 * g + 3]));
      }
  }
}

template <int DQ, bool CAUSAL>
bool launch_one(BwdParams p, hipStream_t st) {
  if (!amk_lds_optin<attn_bwd_fused_x6_kernel<DQ, CAUSAL>>(LDS_BYTES)) return false;
  p.nkblk = (p.J + KB - 1) / KB;
  const int64_t ndq = (int64_t)p.B * p.I * p.H * DH;
  if (DQ == 0 && hipMemsetAsync(p.dq, 0, (size_t)ndq * sizeof(float), st) != hipSuccess) return false;
  const int64_t nk = (int64_t)p.B * p.H * p.nkblk;
  hipLaunchKernelGGL((attn_bwd_fused_x6_kernel<DQ, CAUSAL>), dim3((unsigned)nk), dim3(NT), LDS_BYTES, st, p);
  if (DQ == 1 && p.nkblk > 1) launch_attn_bwd_dq_reduce(p.dq_part, p.nkblk, ndq / 4, p.dq, st);
  return true;
}

}  // namespace

// Head dim 64, 256 keys per workgroup, kept scores, dense (B, I, H, 64) dq: the caller (attn_bwd.hip) has checked all
// four.  p.dq_part != null: reproducible dq.  false: nothing launched.
bool launch_attn_bwd_fused_x6(const BwdParams& p, hipStream_t st) {
  if (!p.scores || !(p.dqs.sh == DH && p.dqs.st == (int64_t)p.H * DH && p.dqs.sb == (int64_t)p.I * p.H * DH)) return false;
  if (p.dq_part) return p.causal_mask ? launch_one<1, true>(p, st) : launch_one<1, false>(p, st);
  return p.causal_mask ? launch_one<0, true>(p, st) : launch_one<0, false>(p, st);
}

}  // namespace amk_attn
