// Softmax attention on bf16 operands (models/softmax_attention.py:62-76 under the reference's bf16 autocast,
// cfg/vitvqgan.yaml:73) for head dims 32 and 128: the two designs of csrc/attn_bf16.hip -- see its header comment for the
// arithmetic, the fill rule and the statistics, which are the same here -- with the head dim D as a template argument,
// written on the counts D / 16 (16-deep steps of a contraction over the head dim) and D / 32 (32-wide blocks of an
// output's head dim).  What follows from D:
//
//   row-read images      stride D + 8 bf16: a 16-byte row read starts each row 4 (D / 8 + 1) banks after the previous
//                        one, D / 8 + 1 odd, so the 16 lanes of a ds_read_b128 group cover the 64 banks (D = 32: 20
//                        banks, D = 128: 68)
//   transposed-read      the 32 lanes of a ds_read_b64_tr_b16 half read 4 consecutive rows x 64 B; the four rows must
//   images               start 16 banks apart (mod 64).  D + 32 does that where D is a multiple of 64 (D = 128: 80 = 16
//                        mod 64); at D = 32 it would be 32 banks (rows 0 / 2 and 1 / 3 on the same banks, 2-way), and
//                        the unpadded row, 16 banks, is the conflict-free one: tstr()
//   forward LDS          2 stages x 64 keys x (KSTR + TSTR) bf16 (+ 512 B of fills when masked): 18 944 B at D = 32,
//                        76 288 B at D = 128 -- dynamic, opted in per device; two workgroups per CU at both
//   backward key block   D = 128: 4 waves x 32 keys = 128 keys per workgroup (8 waves would need 207 872 B of LDS), LDS
//                        142 336 B.  D = 32: 8 waves x 32 keys = 256 keys, as at D = 64, LDS 84 992 B: half the dQ
//                        partials and half the Q / dO traffic of 128-key blocks
//   backward registers   D = 128: dK^T + dV^T 128, K / V fragments 64, S + dP 32, the dQ product's K operands 64
//                        (unmasked), staged Q / dO pieces 32: one wave per SIMD (launch bound 256 x 1, up to 512
//                        registers per lane).  D = 32: two waves per SIMD (512 x 1)
//   dQ tiles             2 query halves x D / 16 dim blocks of 16 x 16 per 32-query tile.  D = 128: sixteen, dealt
//                        round-robin to the four waves -- wave w owns query half w & 1 and dim blocks (w >> 1) + 2 i,
//                        four tiles that share the dS operand.  D = 32: four tiles on waves 0..3; waves 4..7 repeat
//                        them with their stores dropped by a zero-byte descriptor (no branch in the tile loop)
// dQ leaves as per-key-block f32 partials (nkblk, B, I, H, D) that a second launch sums in key-block order: no atomics,
// bitwise reproducible, batch- and head-invariant.
#include "attn_common.h"
#include "amk_bf16.h"

namespace amk_attn_bf16 {

using amk_attn::Strides;
using amk_attn::vmax;
using amk_attn::f32x2;

constexpr int kstr(int D) { return D + 8; }                        // bf16 per row of a row-read image
constexpr int tstr(int D) { return D % 64 == 0 ? D + 32 : D; }     // bf16 per row of a transposed-read image
constexpr int hd_bw(int D) { return D <= 32 ? 8 : 4; }   // waves per backward workgroup
constexpr int hd_bkeys(int D) { return 32 * hd_bw(D); }  // keys per backward workgroup
constexpr int HD_DSTR = 48;              // bf16 per row of the dS^T image [key][32 queries]

constexpr size_t hd_fwd_lds(int D, bool masked) { return (size_t)2 * 64 * (kstr(D) + tstr(D)) * 2 + (masked ? 2 * 64 * 4 : 0); }
constexpr size_t hd_bwd_lds(int D) {
  return (size_t)(hd_bkeys(D) * tstr(D) + 2 * hd_bkeys(D) * HD_DSTR + 4 * (32 * kstr(D) + 32 * tstr(D))) * 2 + 2 * 128 * 4;
}

// ---------------------------------------------------------------------------------------------------------------
template <int D, bool MASKED>
__global__ __launch_bounds__(256, 2) void attn_bf16_hd_fwd_kernel(Params p) {
  constexpr int NC = D / 16, NB = D / 32, KSTR = kstr(D), TSTR = tstr(D);
  // staging: a 64-row tile of 2 D-byte rows = 8 D pieces of 16 B: D / 32 per thread for K, as many for V
  constexpr int PPR = D / 8, RP = 256 / PPR, NP = 64 / RP;
  static_assert(D % 32 == 0 && 256 % PPR == 0 && NP * RP == 64, "the workgroup's passes cover a 64-key tile exactly");
  // two LDS stages: tile t + 1 is committed while tile t is being read, one barrier per tile
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __bf16* const Ks2 = reinterpret_cast<__bf16*>(smem_raw);      // 2 x [64 keys][KSTR]
  __bf16* const Vs2 = Ks2 + 2 * 64 * KSTR;                      // 2 x [64 keys][TSTR]
  float* const Kfill2 = reinterpret_cast<float*>(Vs2 + 2 * 64 * TSTR);   // MASKED: 2 x 64: per key of the tile 0 keep / fill / -inf past J
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 31, hf = lane >> 5;
  const int wg = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));
  const int qb = __builtin_amdgcn_readfirstlane(wg % p.nqblk), bh = __builtin_amdgcn_readfirstlane(wg / p.nqblk);
  const int h = __builtin_amdgcn_readfirstlane(bh % p.H), b = __builtin_amdgcn_readfirstlane(bh / p.H);
  const int qi = qb * 128 + wave * 32 + ln;
  const bool qvalid = qi < p.I;

  // Q^T operand: lane (query, half) holds q[query][16 c + 8 half + j], j = 0..7, for the D / 16 k-blocks c
  bf16x8 qf[NC];
  {
    const __bf16* qp = p.q + (int64_t)b * p.qs.sb + (int64_t)qi * p.qs.st + (int64_t)h * p.qs.sh + 8 * hf;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (qvalid) qf[c] = *reinterpret_cast<const bf16x8*>(qp + 16 * c);
      else {
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[c][j] = (__bf16)0.f;
      }
    }
  }
  const __bf16* kbase = p.k + (int64_t)b * p.ks.sb + (int64_t)h * p.ks.sh;
  const __bf16* vbase = p.v + (int64_t)b * p.vs.sb + (int64_t)h * p.vs.sh;
  const __amdgpu_buffer_rsrc_t k_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, (int)(((int64_t)(p.J - 1) * p.ks.st + D) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t v_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)vbase, 0, (int)(((int64_t)(p.J - 1) * p.vs.st + D) * 2), 0x00020000);
  const int srow = tid / PPR, sch = (tid % PPR) * 8;   // rows srow + RP i, 8 bf16 at column sch
  int koff[NP], voff[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    koff[i] = (int)(((int64_t)(srow + RP * i) * p.ks.st + sch) * 2);
    voff[i] = (int)(((int64_t)(srow + RP * i) * p.vs.st + sch) * 2);
  }
  const int kstep = (int)(64 * p.ks.st * 2), vstep = (int)(64 * p.vs.st * 2);
  float4 kst[NP], vst[NP];
  const float fill_raw = -1.0e9f / p.scale;   // masked_fill(-1e9) acts on the SCALED scores; s here is the raw q . k
  const uint8_t* kmrow = MASKED && p.key_mask ? p.key_mask + (int64_t)b * p.J : nullptr;
  const uint8_t* cmrow = MASKED && p.causal_mask ? p.causal_mask + (int64_t)min(qi, p.I - 1) * p.J : nullptr;
  float fillst = 0.f;
  auto prefetch = [&](int t) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      kst[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, koff[i] + t * kstep, 0, 0));
      vst[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(v_rsrc, voff[i] + t * vstep, 0, 0));
    }
    if (MASKED) {   // (all threads, clamped address: no branch around the load)
      const int j = t * 64 + (tid & 63);
      const uint8_t keep = kmrow ? kmrow[min(j, p.J - 1)] : (uint8_t)1;
      fillst = j >= p.J ? -INFINITY : (keep ? 0.f : fill_raw);
    }
  };
  auto commit = [&](int stage) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      *reinterpret_cast<float4*>(&Ks2[stage * 64 * KSTR + (srow + RP * i) * KSTR + sch]) = kst[i];
      *reinterpret_cast<float4*>(&Vs2[stage * 64 * TSTR + (srow + RP * i) * TSTR + sch]) = vst[i];
    }
    if (MASKED) Kfill2[stage * 64 + (tid & 63)] = fillst;   // (four waves write the same 64 values)
  };
  const float c2 = p.scale * AMK_LOG2E;
  f32x16 o[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) o[nb] = zero16();
  float m_run = -INFINITY, l_run = 0.f;   // m_run: running max of the RAW scores (unmasked: a lazy reference, see below)
  float mc_run = 0.f;                     // m_run * c2
  const float lazy_tau = 8.f / c2;        // the reference moves when a row's maximum passes it by 2^8 in the exponent
  const int ntile = (p.J + 63) / 64;
  prefetch(0);
  commit(0);
  prefetch(1);         // (unconditional throughout: a tile past the sequence is outside the descriptors and reads zeros)
  lds_barrier();
  for (int t = 0; t < ntile; ++t) {
    const int j0 = t * 64;
    const __bf16* Ks = Ks2 + (t & 1) * 64 * KSTR;
    const __bf16* Vs = Vs2 + (t & 1) * 64 * TSTR;
    const float* Kfill = Kfill2 + (t & 1) * 64;
    // ---- S^T = K Q^T: two 32-key blocks x D / 16 16-deep steps
    f32x16 s0 = zero16(), s1 = zero16();
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const bf16x8 ka = *reinterpret_cast<const bf16x8*>(&Ks[ln * KSTR + 16 * c + 8 * hf]);
      const bf16x8 kb = *reinterpret_cast<const bf16x8*>(&Ks[(32 + ln) * KSTR + 16 * c + 8 * hf]);
      s0 = mfmab(ka, qf[c], s0);
      s1 = mfmab(kb, qf[c], s1);
    }
    if (MASKED) {
      // fills: per key of the tile from LDS; the causal bytes of this lane's query row for its 2 x 16 keys
      unsigned cb0 = 0, cb1 = 0;
      if (cmrow) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ja = j0 + acc_row(r, hf);
          cb0 |= (cmrow[min(ja, p.J - 1)] ? 1u : 0u) << r;
          cb1 |= (cmrow[min(ja + 32, p.J - 1)] ? 1u : 0u) << r;
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 f0 = *reinterpret_cast<const float4*>(&Kfill[8 * g + 4 * hf]);
        const float4 f1 = *reinterpret_cast<const float4*>(&Kfill[32 + 8 * g + 4 * hf]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const float fa = f4(f0, e), fb = f4(f1, e);
          float t0 = ((cb0 >> r) & 1u) ? fill_raw : s0[r], t1 = ((cb1 >> r) & 1u) ? fill_raw : s1[r];
          s0[r] = fa == 0.f ? t0 : fa;     // (key-padding fill and the -inf past the sequence win over the causal fill: same value or -inf)
          s1[r] = fb == 0.f ? t1 : fb;
        }
      }
    } else if (j0 + 64 > p.J) {   // keys beyond the sequence (the last tile only): weight 0
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ja = j0 + acc_row(r, hf);
        if (ja >= p.J) s0[r] = -INFINITY;
        if (ja + 32 >= p.J) s1[r] = -INFINITY;
      }
    }
    if (!MASKED) {
      // Unmasked: the lazy reference of csrc/attn_bf16.hip: m_run only has to stay within 2^8 of the true maximum, so
      // the accumulator rescales become rare; (m_run, l) leave as the statistics and the backward forms the same P
      float mx = max3(s0[0], s1[0], s0[1]);
      mx = max3(mx, s1[1], s0[2]);
#pragma unroll
      for (int r = 2; r < 15; ++r) mx = max3(mx, s1[r], s0[r + 1]);
      mx = __builtin_fmaxf(mx, s1[15]);
      mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32, 64));
      if (t == 0 || __any(mx > m_run + lazy_tau)) {
        const float m_new = t == 0 ? mx : __builtin_fmaxf(m_run, mx);
        if (t != 0) {
          const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c2);
          l_run *= alpha;
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[nb][r] *= alpha;
          }
        }
        m_run = m_new;
        mc_run = m_new * c2;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s0[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[r], c2, -mc_run));
        s1[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[r], c2, -mc_run));
      }
      f32x2 la = {0.f, 0.f}, lb = {0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        la += (f32x2){s0[r], s0[r + 1]};
        lb += (f32x2){s1[r], s1[r + 1]};
      }
      la += lb;
      l_run += la.x + la.y;
    } else {
      float mx = vmax(s0[0], s1[0], p.pinf);
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = vmax(mx, vmax(s0[r], s1[r], p.pinf), p.pinf);
      mx = vmax(mx, __shfl_xor(mx, 32, 64), p.pinf);
      const float m_new = vmax(m_run, mx, p.pinf);
      const float mc = __fmul_rn(m_new, c2);
      float lsum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        // two rounded operations, so that s == m gives exactly 0 at any magnitude (a fused multiply-add leaves the
        // rounding error of m * c2, +-64 at the fill value's 1.4e9)
        const float p0 = __builtin_amdgcn_exp2f(mul_sub_rn(s0[r], c2, mc));
        const float p1 = __builtin_amdgcn_exp2f(mul_sub_rn(s1[r], c2, mc));
        s0[r] = p0;
        s1[r] = p1;
        lsum += p0 + p1;
      }
      if (__any(m_new != m_run)) {
        const float alpha = __builtin_amdgcn_exp2f(mul_sub_rn(m_run, c2, mc));
        l_run *= alpha;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
          for (int r = 0; r < 16; ++r) o[nb][r] *= alpha;
        }
        m_run = m_new;
      }
      l_run += lsum;
    }
    // ---- O^T += V^T P^T: four 16-key slots x D / 32 32-dim blocks
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const bf16x8 pp = (g < 2) ? pack8(s0, g & 1) : pack8(s1, g & 1);
      const __bf16* vt = Vs + (32 * (g >> 1)) * TSTR;     // the 32-key block of this slot
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) o[nb] = mfmab(tr_frag_packed<TSTR>(vt, g & 1, 32 * nb, lane), pp, o[nb]);
    }
    commit((t + 1) & 1);   // tile t + 1 (requested a tile ago) into the other stage; past the last tile: zeros nobody reads
    prefetch(t + 2);
    lds_barrier();   // every wave is done with stage t & 1 and has written its part of stage (t + 1) & 1
  }
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.f / l_tot;
  if (qvalid) {
    __bf16* op = p.out + (int64_t)b * p.os.sb + (int64_t)qi * p.os.st + (int64_t)h * p.os.sh + 4 * hf;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4 a;
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = (__bf16)(o[nb][4 * g + e] * inv);
        *reinterpret_cast<bf16x4*>(op + 32 * nb + 8 * g) = a;
      }
    }
    if (hf == 0) {
      float* sp = p.stats + (((int64_t)b * p.H + h) * p.I + qi) * 2;
      sp[0] = __fmul_rn(m_run, c2);   // log2 domain, as the f32 kernels store it
      sp[1] = l_tot;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// delta[b, h, i] = sum_d dO[b, i, h, d] * O[b, i, h, d]   (16 lanes per row, 16-byte pieces dealt round-robin)
template <int D>
__global__ __launch_bounds__(256) void attn_bf16_hd_delta_kernel(Params p) {
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);   // over B * H * I
  const int part = threadIdx.x & 15;
  const int64_t nrow = (int64_t)p.B * p.H * p.I;
  const int64_t rc = row < nrow ? row : nrow - 1;   // (clamped: every lane of a wave takes part in the shuffles)
  const int i = (int)(rc % p.I);
  const int64_t bh = rc / p.I;
  const int h = (int)(bh % p.H), b = (int)(bh / p.H);
  const __bf16* dop = p.d_o + (int64_t)b * p.dos.sb + (int64_t)i * p.dos.st + (int64_t)h * p.dos.sh;
  const __bf16* op = p.o + (int64_t)b * p.os.sb + (int64_t)i * p.os.st + (int64_t)h * p.os.sh;
  float s = 0.f;
  for (int c = part; c < D / 8; c += 16) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(dop + 8 * c);
    const bf16x8 w = *reinterpret_cast<const bf16x8*>(op + 8 * c);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += (float)a[e] * (float)w[e];
  }
#pragma unroll
  for (int x = 8; x >= 1; x >>= 1) s += __shfl_xor(s, x, 64);
  if (part == 0 && row < nrow) {
    // the row constants as the backward's MFMA chains start from them: S' = q.k - (m + log2 l) / c2 (so that
    // P = exp2(c2 S') comes out normalised) and dP' = dO.v - delta
    const float m = p.stats[2 * row], l = p.stats[2 * row + 1];
    const float c2 = p.scale * AMK_LOG2E;
    reinterpret_cast<float4*>(p.delta)[row] = make_float4(-(m + __builtin_log2f(l)) / c2, -s, m, 1.f / l);
  }
}

template <int D, bool MASKED, bool CAUSAL>
__global__ __launch_bounds__(64 * hd_bw(D), 1) void attn_bf16_hd_bwd_kernel(Params p) {
  constexpr int NC = D / 16, NB = D / 32, KSTR = kstr(D), TSTR = tstr(D), BW = hd_bw(D), BKEYS = hd_bkeys(D), DSTR = HD_DSTR, NT = 64 * BW;
  constexpr int KS = BKEYS / 32;                 // 32-deep steps of the dQ product
  constexpr int NQT = 2 * (D / 16);              // 16 x 16 dQ tiles per 32-query tile
  constexpr int QW = NQT < BW ? NQT : BW;        // waves the tiles are dealt to (D = 32: four of the eight)
  constexpr int TPW = NQT / QW;                  // tiles per such wave
  static_assert(TPW * QW == NQT && QW % 2 == 0 && BW % QW == 0, "the dQ tiles are dealt evenly to the waves");
  // query-tile staging: 32 rows of 2 D bytes = 4 D pieces of 16 B per tensor, piece tid + NT i (D = 32: 128 pieces on 256
  // threads -- the upper half requests and writes the lower half's pieces again, no branch around a memory instruction)
  constexpr int PT = 4 * D, NPQ = PT > NT ? PT / NT : 1, PPR = D / 8;
  static_assert(PT % NT == 0 || NT % PT == 0, "pieces and threads divide one another");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __bf16* Kt = reinterpret_cast<__bf16*>(smem_raw);                 // [BKEYS keys][TSTR]
  __bf16* dSs = Kt + BKEYS * TSTR;                                  // 2 x [BKEYS keys][DSTR]
  __bf16* tiles = dSs + 2 * BKEYS * DSTR;                           // 2 stages x {Qrow, Qtr, dOrow, dOtr}
  constexpr int STG = 2 * (32 * KSTR + 32 * TSTR);
  float* stat = reinterpret_cast<float*>(tiles + 2 * STG);          // 2 stages x {-(m + log2 l) / c2, -delta, m, 1 / l} x 32

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 31, hf = lane >> 5;
  const int wg = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x));
  const int kb = __builtin_amdgcn_readfirstlane(wg % p.nkblk), bh = __builtin_amdgcn_readfirstlane(wg / p.nkblk);
  const int h = __builtin_amdgcn_readfirstlane(bh % p.H), b = __builtin_amdgcn_readfirstlane(bh / p.H);
  const int key0 = kb * BKEYS;
  const int key = key0 + 32 * wave + ln;
  const bool kvalid = key < p.J;
  const __bf16* kbase = p.k + (int64_t)b * p.ks.sb + (int64_t)h * p.ks.sh;
  const __bf16* vbase = p.v + (int64_t)b * p.vs.sb + (int64_t)h * p.vs.sh;
  // this lane's key: K and V fragments for S = Q K^T and dP = dO V^T (B operands: k = head dim, column = key)
  bf16x8 kf[NC], vf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (kvalid) {
      kf[c] = *reinterpret_cast<const bf16x8*>(kbase + (int64_t)key * p.ks.st + 16 * c + 8 * hf);
      vf[c] = *reinterpret_cast<const bf16x8*>(vbase + (int64_t)key * p.vs.st + 16 * c + 8 * hf);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) { kf[c][j] = (__bf16)0.f; vf[c][j] = (__bf16)0.f; }
    }
  }
  // the workgroup's K rows as an LDS image for dQ = dS K (rows past the sequence: zeros)
  {
    const __amdgpu_buffer_rsrc_t k_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, (int)(((int64_t)(p.J - 1) * p.ks.st + D) * 2), 0x00020000);
    constexpr int KROWS = NT / PPR;   // rows one pass of the workgroup covers
    static_assert(BKEYS % KROWS == 0, "the passes cover the key block exactly");
#pragma unroll
    for (int i = 0; i < BKEYS / KROWS; ++i) {
      const int row = tid / PPR + KROWS * i, ch = (tid % PPR) * 8;
      const float4 v = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, (int)(((int64_t)(key0 + row) * p.ks.st + ch) * 2), 0, 0));
      *reinterpret_cast<float4*>(&Kt[row * TSTR + ch]) = v;
    }
  }
  const __bf16* qbase = p.q + (int64_t)b * p.qs.sb + (int64_t)h * p.qs.sh;
  const __bf16* dobase = p.d_o + (int64_t)b * p.dos.sb + (int64_t)h * p.dos.sh;
  const __amdgpu_buffer_rsrc_t q_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)qbase, 0, (int)(((int64_t)(p.I - 1) * p.qs.st + D) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t do_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)dobase, 0, (int)(((int64_t)(p.I - 1) * p.dos.st + D) * 2), 0x00020000);
  int prow[NPQ], pch[NPQ], qoff[NPQ], dooff[NPQ];
#pragma unroll
  for (int i = 0; i < NPQ; ++i) {
    const int pc = (tid + NT * i) % PT;
    prow[i] = pc / PPR; pch[i] = (pc % PPR) * 8;
    qoff[i] = (int)(((int64_t)prow[i] * p.qs.st + pch[i]) * 2);
    dooff[i] = (int)(((int64_t)prow[i] * p.dos.st + pch[i]) * 2);
  }
  const int qstep = (int)(32 * p.qs.st * 2), dostep = (int)(32 * p.dos.st * 2);
  const float4* rcp = reinterpret_cast<const float4*>(p.delta) + (int64_t)bh * p.I;
  float4 qpiece[2][NPQ], dopiece[2][NPQ];   // two tiles in flight
  float4 st_rc[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  const int ntile = (p.I + 31) / 32;
  const __amdgpu_buffer_rsrc_t rc_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)rcp, 0, p.I * 16, 0x00020000);
  // MASKED: this lane's key is filled for every query (key-padding mask); the causal bytes of its column come per tile
  const float fill_raw = -1.0e9f / p.scale;
  const bool kfilled = MASKED && p.key_mask && p.key_mask[(int64_t)b * p.J + min(key, p.J - 1)] == 0;
  // (through a buffer descriptor: 32-bit offsets, rows past I clamped -- the causal mask is (I, J) bytes, I * J < 2^31)
  const __amdgpu_buffer_rsrc_t cm_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(CAUSAL ? p.causal_mask : (const uint8_t*)p.delta), 0,
                                                                           CAUSAL ? p.I * p.J : 0, 0x00020000);
  const int cm_key = min(key, p.J - 1);
  // No branch around a memory instruction anywhere in the tile loop (see csrc/attn_bf16.hip)
  auto prefetch = [&](int t, int slot) {
#pragma unroll
    for (int i = 0; i < NPQ; ++i) {
      qpiece[slot][i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(q_rsrc, qoff[i] + t * qstep, 0, 0));
      dopiece[slot][i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(do_rsrc, dooff[i] + t * dostep, 0, 0));
    }
    const int i = t * 32 + (tid & 31);
    // rows past the sequence read zeros: P = exp2(0) = 1 there, next to dO = 0 and q = 0 rows: dV, dK get nothing, dS = 0
    if (MASKED) st_rc[slot] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rc_rsrc, i * 16, 0, 0));
    else {
      const float2 two = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rc_rsrc, i * 16, 0, 0));
      st_rc[slot].x = two.x; st_rc[slot].y = two.y;
    }
  };
  auto commit = [&](int stage, int slot) {
    __bf16* qimg = tiles + stage * STG;
    __bf16* doimg = qimg + 32 * KSTR + 32 * TSTR;
#pragma unroll
    for (int i = 0; i < NPQ; ++i) {
      *reinterpret_cast<float4*>(&qimg[prow[i] * KSTR + pch[i]]) = qpiece[slot][i];                  // row-read image
      *reinterpret_cast<float4*>(&qimg[32 * KSTR + prow[i] * TSTR + pch[i]]) = qpiece[slot][i];      // transposed-read image
      *reinterpret_cast<float4*>(&doimg[prow[i] * KSTR + pch[i]]) = dopiece[slot][i];
      *reinterpret_cast<float4*>(&doimg[32 * KSTR + prow[i] * TSTR + pch[i]]) = dopiece[slot][i];
    }
    {   // every thread writes the constants of row tid & 31 (copies of the same value): no branch around the request
      float* sb = stat + stage * 128;
      sb[tid & 31] = st_rc[slot].x; sb[32 + (tid & 31)] = st_rc[slot].y;
      if (MASKED) { sb[64 + (tid & 31)] = st_rc[slot].z; sb[96 + (tid & 31)] = st_rc[slot].w; }
    }
  };
  const float c2 = p.scale * AMK_LOG2E;
  f32x16 dk[NB], dv[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) { dk[nb] = zero16(); dv[nb] = zero16(); }
  const bool tail_keys = key0 + BKEYS > p.J;   // some of the workgroup's keys are past the sequence
  prefetch(0, 0);
  commit(0, 0);
  prefetch(1, 1);   // (tiles past the end: the descriptor returns zeros)
  prefetch(2, 0);
  __syncthreads();
  float* dqp = p.dq_part + (((int64_t)kb * p.B + b) * p.I * p.H + h) * D;   // [kb][b][i][h][d]
  // dQ: wave w < QW owns the 16 x 16 blocks (queries 16 (w & 1), dims 16 ((w >> 1) + (QW / 2) i)) of every tile, so its K
  // operands -- the same for every tile -- stay in registers (MASKED: re-read from LDS per tile, as in csrc/attn_bf16.hip).
  // Waves past QW (D = 32) repeat the work of wave w - QW into a descriptor of zero bytes, which drops their stores: a
  // wave-uniform branch around the product would put its LDS reads and stores behind a condition (see below)
  const int wq = wave % QW;
  const int qblk = wq & 1, dblk0 = wq >> 1;
  bf16x8 kq[MASKED ? 1 : TPW][MASKED ? 1 : KS];
  if (!MASKED) {
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) kq[i][ks] = tr_frag16(Kt, TSTR, 32 * ks, 16 * (dblk0 + (QW / 2) * i), lane);
    }
  }
  const __amdgpu_buffer_rsrc_t dq_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)dqp, 0, wave < QW ? (int)(((int64_t)(p.I - 1) * p.H * D + D) * 4) : 0, 0x00020000);
  auto dq_tile = [&](int tt) {
    const __bf16* img = dSs + (tt & 1) * BKEYS * DSTR;
    // the dQ^T blocks (dims x queries), so that a lane ends with four consecutive dims of ONE query: a 16-byte store
    f32x4v acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) acc[i] = (f32x4v){0.f, 0.f, 0.f, 0.f};
    int kofs = 0;
    if (MASKED) asm volatile("" : "+v"(kofs));   // (opaque: keeps the compiler from hoisting the K reads out of the tile loop)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 dsf = tr_frag16(img, DSTR, 32 * ks, 16 * qblk, lane);
#pragma unroll
      for (int i = 0; i < TPW; ++i)
        acc[i] = mfma16(MASKED ? tr_frag16(Kt + kofs, TSTR, 32 * ks, 16 * (dblk0 + (QW / 2) * i), lane) : kq[MASKED ? 0 : i][MASKED ? 0 : ks], dsf, acc[i]);
    }
    const int i = tt * 32 + 16 * qblk + (lane & 15);   // (tile -1 and rows past the sequence: outside the descriptor, dropped)
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      const float4 w = make_float4(acc[u][0] * p.scale, acc[u][1] * p.scale, acc[u][2] * p.scale, acc[u][3] * p.scale);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, w), dq_rsrc,
                                             (i * p.H * D + 16 * (dblk0 + (QW / 2) * u) + 4 * (lane >> 4)) * 4, 0, 0);
    }
  };
  auto tile_step = [&](int t, int slot) {   // slot: where tile t + 1 waits in registers
    const int sg = t & 1;
    const __bf16* Qrow = tiles + sg * STG;
    const __bf16* Qtr = Qrow + 32 * KSTR;
    const __bf16* dOrow = Qtr + 32 * TSTR;
    const __bf16* dOtr = dOrow + 32 * KSTR;
    const float* sb = stat + sg * 128;
    // ---- S' = Q K^T - lse / c2, dP' = dO V^T - delta: rows = queries (registers r <-> rows 8 g + 4 half + e of the
    //      tile), columns = keys (this lane's key); the row constants are the chains' initial accumulators
    f32x16 s, dp;
    unsigned cbits = 0;   // CAUSAL: bit r = the causal mask fills (query of register r, this lane's key)
    if (CAUSAL) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        cbits |= (__builtin_amdgcn_raw_buffer_load_b8(cm_rsrc, min(32 * t + acc_row(r, hf), p.I - 1) * p.J + cm_key, 0, 0) ? 1u : 0u) << r;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 d4 = *reinterpret_cast<const float4*>(&sb[32 + 8 * g + 4 * hf]);
      dp[4 * g] = d4.x; dp[4 * g + 1] = d4.y; dp[4 * g + 2] = d4.z; dp[4 * g + 3] = d4.w;
      if (MASKED) {   // raw scores: the fill replaces them below
        s[4 * g] = 0.f; s[4 * g + 1] = 0.f; s[4 * g + 2] = 0.f; s[4 * g + 3] = 0.f;
      } else {
        const float4 a4 = *reinterpret_cast<const float4*>(&sb[8 * g + 4 * hf]);
        s[4 * g] = a4.x; s[4 * g + 1] = a4.y; s[4 * g + 2] = a4.z; s[4 * g + 3] = a4.w;
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const bf16x8 qa = *reinterpret_cast<const bf16x8*>(&Qrow[ln * KSTR + 16 * c + 8 * hf]);
      const bf16x8 da = *reinterpret_cast<const bf16x8*>(&dOrow[ln * KSTR + 16 * c + 8 * hf]);
      s = mfmab(qa, kf[c], s);
      dp = mfmab(da, vf[c], dp);
    }
    // ---- dQ of the previous tile (32 queries x D dims) = dS (32 x BKEYS keys) K (BKEYS x D): issued here, behind the
    //      S / dP chains in the matrix pipe, so that it runs under the exp work below
    dq_tile(t - 1);   // (t = 0: an image nobody wrote, rows -32..-1: every store is dropped)
    // ---- P = exp2(c2 S'), dS / scale = P dP' (the scale goes onto dK and dQ where they are stored)
    if (MASKED) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 m4 = *reinterpret_cast<const float4*>(&sb[64 + 8 * g + 4 * hf]);
        const float4 l4 = *reinterpret_cast<const float4*>(&sb[96 + 8 * g + 4 * hf]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const bool filled = kfilled || ((cbits >> r) & 1u);
          const float tt = filled ? fill_raw : s[r];
          // (s * c2) - m with two rounded operations, as the forward formed it: exactly 0 where the fill is the row maximum
          float pr = __builtin_amdgcn_exp2f(mul_sub_rn(tt, c2, f4(m4, e))) * f4(l4, e);
          pr = kvalid ? pr : 0.f;
          s[r] = pr;                                 // a filled position still has its weight in P (dV), but passes no gradient
          dp[r] = filled ? 0.f : dp[r] * pr;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float pr = __builtin_amdgcn_exp2f(s[r] * c2);
        if (tail_keys) pr = kvalid ? pr : 0.f;
        s[r] = pr;
        dp[r] *= pr;
      }
    }
    // ---- dS^T image for dQ: this lane's key row, its 16 queries as four 8-byte pieces (image t & 1: the dQ product
    //      of tile t runs in the NEXT iteration, beside that tile's S / dP work, so one barrier per tile is enough)
    {
      __bf16* row = dSs + (t & 1) * BKEYS * DSTR + (32 * wave + ln) * DSTR + 4 * hf;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = (__bf16)dp[4 * g + e];
        *reinterpret_cast<bf16x4*>(row + 8 * g) = w;
      }
    }
    // ---- dV^T += dO^T P, dK^T += Q^T dS (sums over the tile's 32 queries: two 16-deep slots)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bf16x8 pb = pack8(s, u), db = pack8(dp, u);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        dv[nb] = mfmab(tr_frag_packed<TSTR>(dOtr, u, 32 * nb, lane), pb, dv[nb]);
        dk[nb] = mfmab(tr_frag_packed<TSTR>(Qtr, u, 32 * nb, lane), db, dk[nb]);
      }
    }
    commit((t + 1) & 1, slot);   // (past the last tile: zeros nobody reads)
    prefetch(t + 3, slot);
    __syncthreads();   // this tile's dS rows are in LDS, the next tile's images and statistics in place
  };
  const int ntile2 = (ntile + 1) & ~1;   // an even count: a tile past the sequence has q = 0, dO = 0 (dS = 0, nothing added)
  for (int t = 0; t < ntile2; t += 2) {
    tile_step(t, 1);
    tile_step(t + 1, 0);
  }
  dq_tile(ntile2 - 1);
  if (kvalid) {
    __bf16* kp = p.dk + (int64_t)b * p.dks.sb + (int64_t)key * p.dks.st + (int64_t)h * p.dks.sh + 4 * hf;
    __bf16* vp = p.dv + (int64_t)b * p.dvs.sb + (int64_t)key * p.dvs.st + (int64_t)h * p.dvs.sh + 4 * hf;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4 a, d;
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = (__bf16)(dk[nb][4 * g + e] * p.scale); d[e] = (__bf16)dv[nb][4 * g + e]; }
        *reinterpret_cast<bf16x4*>(kp + 32 * nb + 8 * g) = a;
        *reinterpret_cast<bf16x4*>(vp + 32 * nb + 8 * g) = d;
      }
    }
  }
}

// dq[b, i, h, :] = sum over key blocks (in order) of the f32 partials, rounded to bf16 once
template <int D>
__global__ __launch_bounds__(256) void attn_bf16_hd_dq_reduce_kernel(Params p) {
  const int64_t n4 = (int64_t)p.B * p.I * p.H * (D / 4);   // float4 pieces of one partial
  const int64_t i4 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i4 >= n4) return;
  const float4* src = reinterpret_cast<const float4*>(p.dq_part) + i4;
  float4 s = src[0];
  for (int kb = 1; kb < p.nkblk; ++kb) {
    const float4 v = src[kb * n4];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const int d4 = (int)(i4 % (D / 4));
  const int64_t r = i4 / (D / 4);       // (b, i, h)
  const int h = (int)(r % p.H);
  const int64_t bi = r / p.H;
  const int i = (int)(bi % p.I), b = (int)(bi / p.I);
  bf16x4 w;
  w[0] = (__bf16)s.x; w[1] = (__bf16)s.y; w[2] = (__bf16)s.z; w[3] = (__bf16)s.w;
  *reinterpret_cast<bf16x4*>(p.dq + (int64_t)b * p.dqs.sb + (int64_t)i * p.dqs.st + (int64_t)h * p.dqs.sh + 4 * d4) = w;
}

}  // namespace amk_attn_bf16

using namespace amk_attn_bf16;
using amk_attn::strides_ok8;

static bool hd_supported(int Dh) { return Dh == 32 || Dh == 128; }
#define AMK_HD_REFUSAL(who) who ": head dim %d not supported (32, 128; head dim 64 runs on amk_attn_bf16_fwd / amk_attn_bf16_bwd)"

template <int D>
static int hd_fwd_launch(const Params& p, int64_t nwg, hipStream_t st) {
  const bool masked = p.key_mask || p.causal_mask;
  const size_t lds = hd_fwd_lds(D, masked);
  AMK_CHECK_SUPPORTED((amk_lds_optin<attn_bf16_hd_fwd_kernel<D, false>>((int)hd_fwd_lds(D, false)) &&
                       amk_lds_optin<attn_bf16_hd_fwd_kernel<D, true>>((int)hd_fwd_lds(D, true))),
                      "amk_attn_bf16_hd_fwd: the device refused %zu bytes of dynamic LDS", lds);
  if (masked) hipLaunchKernelGGL((attn_bf16_hd_fwd_kernel<D, true>), dim3((unsigned)nwg), dim3(256), lds, st, p);
  else hipLaunchKernelGGL((attn_bf16_hd_fwd_kernel<D, false>), dim3((unsigned)nwg), dim3(256), lds, st, p);
  return AMK_OK;
}

extern "C" int amk_attn_bf16_hd_fwd(const void* q, const void* k, const void* v, void* o, float* stats,
                                    const uint8_t* key_mask, const uint8_t* causal_mask,
                                    int B, int H, int I, int J, int Dh,
                                    int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                                    int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                                    float scale, void* stream) {
  AMK_CHECK_ARG(q && k && v && o && stats, "amk_attn_bf16_hd_fwd: null tensor pointer");
  AMK_CHECK_ARG(B > 0 && H > 0 && I > 0 && J > 0, "amk_attn_bf16_hd_fwd: non-positive size B=%d H=%d I=%d J=%d", B, H, I, J);
  AMK_CHECK_SUPPORTED(hd_supported(Dh), AMK_HD_REFUSAL("amk_attn_bf16_hd_fwd"), Dh);
  Params p = {};
  p.q = (const __bf16*)q; p.k = (const __bf16*)k; p.v = (const __bf16*)v; p.out = (__bf16*)o; p.stats = stats;
  p.key_mask = key_mask; p.causal_mask = causal_mask;
  p.B = B; p.H = H; p.I = I; p.J = J;
  p.qs = {q_sb, q_st, q_sh}; p.ks = {k_sb, k_st, k_sh}; p.vs = {v_sb, v_st, v_sh}; p.os = {o_sb, o_st, o_sh};
  p.scale = scale; p.pinf = INFINITY;
  p.nqblk = (I + 127) / 128;
  AMK_CHECK_ARG(a16(q) && a16(k) && a16(v) && a16(o) && strides_ok8(p.qs) && strides_ok8(p.ks) && strides_ok8(p.vs) && strides_ok8(p.os),
                "amk_attn_bf16_hd_fwd: pointers must be 16-byte aligned and strides multiples of 8 elements");
  const int64_t nwg = (int64_t)B * H * p.nqblk;
  AMK_CHECK_SUPPORTED(nwg < (1ll << 31), "amk_attn_bf16_hd_fwd: grid too large");
  AMK_CHECK_SUPPORTED(((int64_t)J + 64) * k_st * 2 < (1ll << 31) && ((int64_t)J + 64) * v_st * 2 < (1ll << 31),
                      "amk_attn_bf16_hd_fwd: one (batch, head) K/V slab must span < 2 GiB");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = Dh == 32 ? hd_fwd_launch<32>(p, nwg, st) : hd_fwd_launch<128>(p, nwg, st);
  if (rc != AMK_OK) return rc;
  AMK_CHECK_LAUNCH("amk_attn_bf16_hd_fwd");
  return AMK_OK;
}

extern "C" int64_t amk_attn_bf16_hd_bwd_ws_floats(int B, int H, int I, int J, int Dh) {
  if (B <= 0 || H <= 0 || I <= 0 || J <= 0 || !hd_supported(Dh)) return 0;
  const int64_t nkblk = (J + hd_bkeys(Dh) - 1) / hd_bkeys(Dh);
  return 4 * (int64_t)B * H * I + nkblk * B * I * H * Dh;   // four row constants per query + dQ partials
}

template <int D>
static int hd_bwd_launch(const Params& p, hipStream_t st) {
  constexpr size_t lds = hd_bwd_lds(D);
  AMK_CHECK_SUPPORTED((amk_lds_optin<attn_bf16_hd_bwd_kernel<D, false, false>>((int)lds) && amk_lds_optin<attn_bf16_hd_bwd_kernel<D, true, false>>((int)lds) &&
                       amk_lds_optin<attn_bf16_hd_bwd_kernel<D, true, true>>((int)lds)),
                      "amk_attn_bf16_hd_bwd: the device refused %zu bytes of dynamic LDS", lds);
  const int64_t rows = (int64_t)p.B * p.H * p.I;
  hipLaunchKernelGGL(attn_bf16_hd_delta_kernel<D>, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, p);
  const int64_t nwg = (int64_t)p.B * p.H * p.nkblk;
  if (p.causal_mask) hipLaunchKernelGGL((attn_bf16_hd_bwd_kernel<D, true, true>), dim3((unsigned)nwg), dim3(64 * hd_bw(D)), lds, st, p);
  else if (p.key_mask) hipLaunchKernelGGL((attn_bf16_hd_bwd_kernel<D, true, false>), dim3((unsigned)nwg), dim3(64 * hd_bw(D)), lds, st, p);
  else hipLaunchKernelGGL((attn_bf16_hd_bwd_kernel<D, false, false>), dim3((unsigned)nwg), dim3(64 * hd_bw(D)), lds, st, p);
  const int64_t n4 = (int64_t)p.B * p.I * p.H * (D / 4);
  hipLaunchKernelGGL(attn_bf16_hd_dq_reduce_kernel<D>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, p);
  return AMK_OK;
}

extern "C" int amk_attn_bf16_hd_bwd(const void* q, const void* k, const void* v, const void* o, const float* stats, const void* d_o,
                                    void* dq, void* dk, void* dv, float* ws,
                                    const uint8_t* key_mask, const uint8_t* causal_mask,
                                    int B, int H, int I, int J, int Dh,
                                    int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                                    int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                                    int64_t do_sb, int64_t do_st, int64_t do_sh, int64_t dq_sb, int64_t dq_st, int64_t dq_sh,
                                    int64_t dk_sb, int64_t dk_st, int64_t dk_sh, int64_t dv_sb, int64_t dv_st, int64_t dv_sh,
                                    float scale, void* stream) {
  AMK_CHECK_ARG(q && k && v && o && stats && d_o && dq && dk && dv && ws, "amk_attn_bf16_hd_bwd: null tensor pointer");
  AMK_CHECK_ARG(B > 0 && H > 0 && I > 0 && J > 0, "amk_attn_bf16_hd_bwd: non-positive size B=%d H=%d I=%d J=%d", B, H, I, J);
  AMK_CHECK_SUPPORTED(hd_supported(Dh), AMK_HD_REFUSAL("amk_attn_bf16_hd_bwd"), Dh);
  Params p = {};
  p.q = (const __bf16*)q; p.k = (const __bf16*)k; p.v = (const __bf16*)v; p.o = (const __bf16*)o; p.d_o = (const __bf16*)d_o;
  p.dq = (__bf16*)dq; p.dk = (__bf16*)dk; p.dv = (__bf16*)dv;
  p.stats = const_cast<float*>(stats);
  p.key_mask = key_mask; p.causal_mask = causal_mask;
  p.B = B; p.H = H; p.I = I; p.J = J;
  p.qs = {q_sb, q_st, q_sh}; p.ks = {k_sb, k_st, k_sh}; p.vs = {v_sb, v_st, v_sh}; p.os = {o_sb, o_st, o_sh};
  p.dos = {do_sb, do_st, do_sh}; p.dqs = {dq_sb, dq_st, dq_sh}; p.dks = {dk_sb, dk_st, dk_sh}; p.dvs = {dv_sb, dv_st, dv_sh};
  p.scale = scale; p.pinf = INFINITY;
  const int bkeys = hd_bkeys(Dh);
  p.nkblk = (J + bkeys - 1) / bkeys;
  p.delta = ws;
  p.dq_part = ws + 4 * (int64_t)B * H * I;
  AMK_CHECK_ARG(a16(q) && a16(k) && a16(v) && a16(o) && a16(d_o) && a16(dq) && a16(dk) && a16(dv) && a16(p.dq_part) &&
                    strides_ok8(p.qs) && strides_ok8(p.ks) && strides_ok8(p.vs) && strides_ok8(p.os) && strides_ok8(p.dos) &&
                    strides_ok8(p.dqs) && strides_ok8(p.dks) && strides_ok8(p.dvs),
                "amk_attn_bf16_hd_bwd: pointers must be 16-byte aligned and strides multiples of 8 elements");
  AMK_CHECK_SUPPORTED(((int64_t)J + bkeys) * k_st * 2 < (1ll << 31) && ((int64_t)J + bkeys) * v_st * 2 < (1ll << 31) &&
                          ((int64_t)I + 32) * q_st * 2 < (1ll << 31) && ((int64_t)I + 32) * do_st * 2 < (1ll << 31),
                      "amk_attn_bf16_hd_bwd: one (batch, head) slab must span < 2 GiB");
  // the kernels address one key block's dQ partial, the row constants and the causal mask with 32-bit byte offsets
  AMK_CHECK_SUPPORTED(((int64_t)I + 32) * H * Dh * 4 < (1ll << 31) && (int64_t)I * 16 < (1ll << 31) && (!causal_mask || (int64_t)I * J < (1ll << 31)),
                      "amk_attn_bf16_hd_bwd: one key block's dq partial (I x H x D f32) and the causal mask must span < 2 GiB");
  AMK_CHECK_SUPPORTED((int64_t)B * H * p.nkblk < (1ll << 31), "amk_attn_bf16_hd_bwd: grid too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = Dh == 32 ? hd_bwd_launch<32>(p, st) : hd_bwd_launch<128>(p, st);
  if (rc != AMK_OK) return rc;
  AMK_CHECK_LAUNCH("amk_attn_bf16_hd_bwd");
  return AMK_OK;
}
