// Softmax-attention backward for gfx950: the host entry points and the dispatch over head dims and `stages`.
//
// Autograd of models/softmax_attention.py:62-76 of the reference, where PyTorch keeps the
// (B,h,I,J) score and probability tensors for the backward.  Here P is recomputed from
// q, k and the saved row statistics {m, l}.  Two forms:
//
//   the recompute kernels of attn_generic.h (every head dim; three launches, no atomics, bitwise reproducible)
//     attn_bwd_delta : delta[b,h,i] = sum_d dO*O                     (HBM-bound, tiny)
//     attn_bwd_dq    : QUERY ON THE LANE (same skeleton as the forward)
//          S^T  = K Q^T, dP^T = V dO^T      (A = K / V rows from LDS, B = q / dO registers)
//          dS^T = P^T o (dP^T - delta)      (per-lane scalars m, 1/l, delta)
//          dQ^T += K^T dS^T                 (A = K columns from LDS, B = the dS^T accumulator)
//     attn_bwd_dkdv  : KEY ON THE LANE (a wave owns 32 keys, k / v live in registers)
//          S  = Q K^T,  dP = dO V^T         (A = q / dO rows from LDS, B = k / v registers)
//          dV^T += dO^T P,  dK^T += Q^T dS  (A = dO / q columns from LDS, B = accumulators)
//   the one-pass kernel of attn_bwd_fused.hip (head dims 32, 64, 128), after delta
//
// Gradients do not flow through positions the forward filled with -1e9 (masked_fill).
#include "attn_generic.h"

namespace amk_attn {
// the head dim 64 recompute kernels live here (the other head dims: attn_generic.hip, attn_generic_dNNN.hip)
AMK_ATTN_GEN_BWD_INSTANTIATE(64)
}  // namespace amk_attn

using namespace amk_attn;

static int attn_bwd_impl(const float* scores, const float* q, const float* k, const float* v, const float* o,
                            const float* stats, const float* d_o,
                            float* dq, float* dk, float* dv, float* delta_ws,
                            const uint8_t* key_mask, const uint8_t* causal_mask,
                            int B, int H, int I, int J, int Dh,
                            int64_t q_sb, int64_t q_st, int64_t q_sh,
                            int64_t k_sb, int64_t k_st, int64_t k_sh,
                            int64_t v_sb, int64_t v_st, int64_t v_sh,
                            int64_t o_sb, int64_t o_st, int64_t o_sh,
                            int64_t do_sb, int64_t do_st, int64_t do_sh,
                            int64_t dq_sb, int64_t dq_st, int64_t dq_sh,
                            int64_t dk_sb, int64_t dk_st, int64_t dk_sh,
                            int64_t dv_sb, int64_t dv_st, int64_t dv_sh,
                            float scale, int stages, void* stream) {
  AMK_CHECK_ARG(q && k && v && o && stats && d_o && dq && dk && dv && delta_ws, "amk_attn_bwd: null tensor pointer");
  AMK_CHECK_ARG(B > 0 && H > 0 && I > 0 && J > 0, "amk_attn_bwd: non-positive size B=%d H=%d I=%d J=%d", B, H, I, J);
  AMK_CHECK_SUPPORTED(Dh == D || attn_gen_supported(Dh), "amk_attn_bwd: head dim %d not supported (a multiple of 32 from 32 to 256)", Dh);
  AMK_CHECK_SUPPORTED(Dh == D || !scores || Dh == 32 || Dh == 128,
                      "amk_attn_bwd_kept: kept scores exist for head dims 32, 64 and 128 only (head dim %d)", Dh);
  AMK_CHECK_SUPPORTED(Dh == D || !scores || !(stages & AMK_ATTN_BWD_DQ_REPRO),
                      "amk_attn_bwd_kept: kept scores with the reproducible dq exist for head dim %d only", D);
  BwdParams p;
  p.q = q; p.k = k; p.v = v; p.o = o; p.stats = stats; p.d_o = d_o;
  p.dq = dq; p.dk = dk; p.dv = dv; p.delta = delta_ws;
  p.key_mask = key_mask; p.causal_mask = causal_mask;
  p.B = B; p.H = H; p.I = I; p.J = J;
  p.qs = {q_sb, q_st, q_sh}; p.ks = {k_sb, k_st, k_sh}; p.vs = {v_sb, v_st, v_sh}; p.os = {o_sb, o_st, o_sh};
  p.dos = {do_sb, do_st, do_sh}; p.dqs = {dq_sb, dq_st, dq_sh}; p.dks = {dk_sb, dk_st, dk_sh}; p.dvs = {dv_sb, dv_st, dv_sh};
  p.scale = scale;
  p.pinf = INFINITY;
  p.nqblk = (I + BLK - 1) / BLK;
  p.nkblk = (J + BLK - 1) / BLK;
  p.scores = scores;
  // reproducible dq from the one-pass kernel: the partials live behind the deltas in the workspace
  p.dq_part = (stages & AMK_ATTN_BWD_DQ_REPRO) ? delta_ws + (((int64_t)B * H * I + 3) & ~(int64_t)3) : nullptr;
  AMK_CHECK_ARG(!scores || aligned16(scores), "amk_attn_bwd_kept: the scores buffer must be 16-byte aligned");
  AMK_CHECK_ARG(!scores || (stages & AMK_ATTN_BWD_FUSED), "amk_attn_bwd_kept: kept scores are read by the fused pass only");
  AMK_CHECK_ARG(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(o) && aligned16(d_o) && aligned16(dq) &&
                    aligned16(dk) && aligned16(dv) && strides_ok(p.qs) && strides_ok(p.ks) && strides_ok(p.vs) &&
                    strides_ok(p.os) && strides_ok(p.dos) && strides_ok(p.dqs) && strides_ok(p.dks) && strides_ok(p.dvs),
                "amk_attn_bwd: pointers must be 16-byte aligned and strides multiples of 4 elements");
  const int64_t nrow = (int64_t)B * H * I;
  const int64_t nq = (int64_t)B * H * p.nqblk, nk = (int64_t)B * H * p.nkblk;
  AMK_CHECK_SUPPORTED(nq < (1ll << 31) && nk < (1ll << 31) && (nrow + 15) / 16 < (1ll << 31), "amk_attn_bwd: grid too large");
  AMK_CHECK_SUPPORTED(((int64_t)J + TILE) * k_st * 4 < (1ll << 31) && ((int64_t)J + TILE) * v_st * 4 < (1ll << 31) &&
                          ((int64_t)I + TILE) * q_st * 4 < (1ll << 31) && ((int64_t)I + TILE) * do_st * 4 < (1ll << 31),
                      "amk_attn_bwd: one (batch, head) slab must span < 2 GiB");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool x6 = (stages & AMK_ATTN_BWD_X6) != 0;
  if (x6) {   // the split-bf16 variant of the kept-scores kernel has one geometry and no fallback
    const int keys = fused_keys_per_wg(J, (stages & AMK_ATTN_BWD_KEYS256) ? 256 : ((stages & AMK_ATTN_BWD_KEYS128) ? 128 : 0));
    AMK_CHECK_SUPPORTED(scores && (stages & AMK_ATTN_BWD_FUSED), "amk_attn_bwd: AMK_ATTN_BWD_X6 is for amk_attn_bwd_kept with AMK_ATTN_BWD_FUSED");
    AMK_CHECK_SUPPORTED(Dh == D, "amk_attn_bwd_kept: AMK_ATTN_BWD_X6 exists for head dim %d only (head dim %d)", D, Dh);
    AMK_CHECK_SUPPORTED(keys == 256, "amk_attn_bwd_kept: AMK_ATTN_BWD_X6 runs at 256 keys per workgroup only (J = %d: %d)", J, keys);
    AMK_CHECK_SUPPORTED(dq_sh == D && dq_st == (int64_t)H * D && dq_sb == (int64_t)I * H * D,
                        "amk_attn_bwd_kept: AMK_ATTN_BWD_X6 needs the dense (B, I, H, %d) dq layout", D);
  }
  if (stages & AMK_ATTN_BWD_DELTA) launch_attn_bwd_gen(p, Dh, AMK_ATTN_BWD_DELTA, st);
  if (x6) {
    AMK_CHECK_SUPPORTED(launch_attn_bwd_fused_x6(p, st), "amk_attn_bwd_kept: the split-bf16 one-pass kernel could not be launched");
    AMK_CHECK_LAUNCH("amk_attn_bwd");
    return AMK_OK;
  }
  if (stages & AMK_ATTN_BWD_FUSED) {
    // the one-pass kernel of this head dim (attn_bwd_fused.hip: 32, 64, 128; the others have none) when the layout
    // allows it, else the two recompute kernels
    const int keys = (stages & AMK_ATTN_BWD_KEYS256) ? 256 : ((stages & AMK_ATTN_BWD_KEYS128) ? 128 : 0);
    const bool ran = launch_attn_bwd_fused(p, Dh, keys, st);
    AMK_CHECK_SUPPORTED(ran || Dh == D || !scores,
                        "amk_attn_bwd_kept: the one-pass kernel could not run (dq layout) and the recompute kernels do not read kept scores");
    stages = ran ? 0 : (AMK_ATTN_BWD_DKDV | AMK_ATTN_BWD_DQ);
  }
  launch_attn_bwd_gen(p, Dh, stages & (AMK_ATTN_BWD_DKDV | AMK_ATTN_BWD_DQ), st);
  AMK_CHECK_LAUNCH("amk_attn_bwd");
  return AMK_OK;
}

extern "C" int64_t amk_attn_bwd_ws_floats(int B, int H, int I, int J, int stages) {
  if (B <= 0 || H <= 0 || I <= 0 || J <= 0) return 0;
  int64_t n = ((int64_t)B * H * I + 3) & ~(int64_t)3;
  if ((stages & AMK_ATTN_BWD_FUSED) && (stages & AMK_ATTN_BWD_DQ_REPRO)) {
    const int keys = fused_keys_per_wg(J, (stages & AMK_ATTN_BWD_KEYS256) ? 256 : ((stages & AMK_ATTN_BWD_KEYS128) ? 128 : 0));
    const int nk = (J + keys - 1) / keys;
    if (nk > 1) n += (int64_t)nk * B * I * H * D;
  }
  return n;
}

extern "C" int amk_attn_bwd(const float* q, const float* k, const float* v, const float* o,
                            const float* stats, const float* d_o,
                            float* dq, float* dk, float* dv, float* delta_ws,
                            const uint8_t* key_mask, const uint8_t* causal_mask,
                            int B, int H, int I, int J, int Dh,
                            int64_t q_sb, int64_t q_st, int64_t q_sh,
                            int64_t k_sb, int64_t k_st, int64_t k_sh,
                            int64_t v_sb, int64_t v_st, int64_t v_sh,
                            int64_t o_sb, int64_t o_st, int64_t o_sh,
                            int64_t do_sb, int64_t do_st, int64_t do_sh,
                            int64_t dq_sb, int64_t dq_st, int64_t dq_sh,
                            int64_t dk_sb, int64_t dk_st, int64_t dk_sh,
                            int64_t dv_sb, int64_t dv_st, int64_t dv_sh,
                            float scale, int stages, void* stream) {
  return attn_bwd_impl(nullptr, q, k, v, o, stats, d_o, dq, dk, dv, delta_ws, key_mask, causal_mask, B, H, I, J, Dh,
                       q_sb, q_st, q_sh, k_sb, k_st, k_sh, v_sb, v_st, v_sh, o_sb, o_st, o_sh, do_sb, do_st, do_sh,
                       dq_sb, dq_st, dq_sh, dk_sb, dk_st, dk_sh, dv_sb, dv_st, dv_sh, scale, stages, stream);
}

extern "C" int amk_attn_bwd_kept(const float* scores, const float* q, const float* k, const float* v, const float* o,
                                 const float* stats, const float* d_o,
                                 float* dq, float* dk, float* dv, float* delta_ws,
                                 const uint8_t* key_mask, const uint8_t* causal_mask,
                                 int B, int H, int I, int J, int Dh,
                                 int64_t q_sb, int64_t q_st, int64_t q_sh,
                                 int64_t k_sb, int64_t k_st, int64_t k_sh,
                                 int64_t v_sb, int64_t v_st, int64_t v_sh,
                                 int64_t o_sb, int64_t o_st, int64_t o_sh,
                                 int64_t do_sb, int64_t do_st, int64_t do_sh,
                                 int64_t dq_sb, int64_t dq_st, int64_t dq_sh,
                                 int64_t dk_sb, int64_t dk_st, int64_t dk_sh,
                                 int64_t dv_sb, int64_t dv_st, int64_t dv_sh,
                                 float scale, int stages, void* stream) {
  AMK_CHECK_ARG(scores, "amk_attn_bwd_kept: null scores buffer");
  return attn_bwd_impl(scores, q, k, v, o, stats, d_o, dq, dk, dv, delta_ws, key_mask, causal_mask, B, H, I, J, Dh,
                       q_sb, q_st, q_sh, k_sb, k_st, k_sh, v_sb, v_st, v_sh, o_sb, o_st, o_sh, do_sb, do_st, do_sh,
                       dq_sb, dq_st, dq_sh, dk_sb, dk_st, dk_sh, dv_sb, dv_st, dv_sh, scale, stages, stream);
}
