/*
 * amk.h -- C ABI of libamk.so: the MI355X (gfx950 / CDNA4) kernels behind the
 * attention / MoE / VQ hot path of pranoyr/attention-models.
 *
 * The reference has no FFI: its hot path is five Python nn.Modules (SURVEY.md
 * section 8b).  This header is the boundary a maintainer binds instead of the
 * eager-PyTorch op sequences inside those modules; every entry point cites the
 * reference lines it replaces.  The Python binding that ships with this repo is
 * attention-models_amd/amk/lib.py (ctypes); INTEGRATION.md shows the stub.
 *
 * Contract (all entry points)
 *   - extern "C", plain pointers and sizes; no C++ / torch types cross the ABI.
 *   - every pointer is a DEVICE pointer (hipMalloc'ed, fp32 unless stated),
 *     allocated and owned by the caller; the library never allocates, frees or
 *     synchronises.  Workspaces are caller-allocated, sizes stated per function.
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the default stream).
 *   - return value: AMK_OK (0) or a negative AMK_E* code; amk_last_error()
 *     returns a thread-local message for the last failure on this thread.
 *   - tensors are row-major; "stride" arguments are in ELEMENTS, the innermost
 *     (head-dim / feature) axis is always contiguous.
 *   - indices are int64 where the reference returns torch.int64.
 */
#ifndef AMK_H_
#define AMK_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMK_VERSION 140 /* 0.4.0: amk_attn_bf16_fwd / _bwd take key_mask / causal_mask (signatures changed), the optimizer step takes a per-parameter table (decoupled weight decay, device-resident learning rate), one-pass backward for head dims 32 / 128 behind amk_attn_bwd; 0.3.5: amk_agent_conv_grad_reduce; 0.3.4: amk_moe_route_distinct, _rows forms of combine / gate_grad; 0.3.3: amk_moe_expert_sums; 0.3.2: bf16 forward / input-gradient GEMM; 0.3.1: bf16 weight-gradient GEMM; 0.3.0: dense f32 GEMMs with LayerNorm / SwiGLU / residual / bias-gradient fusions (amk_gemm_f32) */

enum {
  AMK_OK = 0,
  AMK_EINVAL = -1,       /* bad argument (null pointer, non-positive size, ...) */
  AMK_EUNSUPPORTED = -2, /* shape outside what the kernels are built for        */
  AMK_ELAUNCH = -3       /* hipLaunchKernel / hipMemsetAsync reported an error  */
};

int amk_version(void);
/* Offload architecture the code objects were built for ("gfx950"). */
const char* amk_arch(void);
const char* amk_last_error(void);

/* --------------------------------------------------------------------------
 * Fused softmax attention core.
 * Replaces models/softmax_attention.py:62-76 (and the identical core of
 * models/switchhead_attention.py:98-111): scaled QK^T, key-padding fill,
 * causal fill, row softmax, PV -- without materialising the (B,h,I,J) scores.
 *
 *   S[b,h,i,j] = sum_d (q[b,h,i,d]*scale) * k[b,h,j,d]
 *   S = -1e9 where key_mask[b,j] == 0          (reference: masked_fill(~context_mask))
 *   S = -1e9 where causal_mask[i,j] != 0       (reference: masked_fill(causal_mask))
 *   P = softmax_j(S);  o[b,h,i,:] = sum_j P[b,h,i,j] v[b,h,j,:]
 *   stats[b,h,i] = { m, l }: a row reference m in the log2 domain and l = sum_j exp2(S*log2(e) - m)
 *                 (saved for the backward, which forms P = exp2(S*log2(e) - m) / l; two floats per row so
 *                  that a fully masked row, S = -1e9 everywhere, keeps its exact 1/J weights).
 *                 With a mask m = max_j S*log2(e); without masks (D = 64) m is a reference within 8 of
 *                 that maximum -- it moves only when a tile's maximum passes it by more than 8 -- and l
 *                 is the sum relative to it: the same P.
 *
 * q/o are addressed as  base + b*sb + t*st + h*sh + d   (d < D contiguous), so
 * the (B,T,h*D) projection outputs are consumed in place (st = h*D, sh = D) as
 * well as (B,h,T,D) tensors (sh = T*D, st = D).  k and v likewise with J rows.
 * key_mask: uint8 (B,J) contiguous or NULL; causal_mask: uint8 (I,J) contiguous
 * or NULL.  stats: (B,H,I,2) contiguous.  D is a multiple of 32 from 32 to 256; any other head dim is
 * AMK_EUNSUPPORTED before any device work.  64: the tuned kernels and the split-bf16 forward; 32 / 128:
 * csrc/attn_generic.h -- forward, with kept scores when there is no mask -- and the head dim 64 one-pass backward
 * of csrc/attn_bwd_fused.hip at their own geometry, dq by atomics; their reproducible backward is the two recompute
 * kernels of csrc/attn_generic.h.  96, 160, 192, 224, 256 (same library version, 0.4.0): the forward and the
 * recompute backward of csrc/attn_generic.h only -- amk_attn_fwd_keep / amk_attn_bwd_kept return
 * AMK_EUNSUPPORTED for them, and a FUSED request to amk_attn_bwd runs the recompute kernels.
 * -------------------------------------------------------------------------- */
int amk_attn_fwd(const float* q, const float* k, const float* v, float* o, float* stats,
                 const uint8_t* key_mask, const uint8_t* causal_mask,
                 int B, int H, int I, int J, int D,
                 int64_t q_sb, int64_t q_st, int64_t q_sh,
                 int64_t k_sb, int64_t k_st, int64_t k_sh,
                 int64_t v_sb, int64_t v_st, int64_t v_sh,
                 int64_t o_sb, int64_t o_st, int64_t o_sh,
                 float scale, void* stream);

/* The same forward, which also leaves the raw scores for the backward (training): scores must hold
 * amk_attn_scores_bytes(B, H, I, J) bytes (4 bytes per (b, h, i, j), both sequence lengths padded to the
 * kernels' tiles; 32x32 tiles, [b][h][key block][query block][key][query]).  The reference keeps the same
 * tensor alive for autograd (models/softmax_attention.py:62, the einsum output); here it is written
 * once and read once, by amk_attn_bwd_kept, which then runs four matrix products instead of five. */
int64_t amk_attn_scores_bytes(int B, int H, int I, int J);
int amk_attn_fwd_keep(const float* q, const float* k, const float* v, float* o, float* stats, float* scores,
                      const uint8_t* key_mask, const uint8_t* causal_mask,
                      int B, int H, int I, int J, int D,
                      int64_t q_sb, int64_t q_st, int64_t q_sh,
                      int64_t k_sb, int64_t k_st, int64_t k_sh,
                      int64_t v_sb, int64_t v_st, int64_t v_sh,
                      int64_t o_sb, int64_t o_st, int64_t o_sh,
                      float scale, void* stream);

/* The same forward with split-bf16 products: every f32 operand is split into three bf16 parts
 * (24 mantissa bits) and each product is the sum of six exact partial products accumulated in f32
 * (v_mfma_f32_32x32x16_bf16).  Same arguments, outputs, statistics and masks; the error against a
 * double-precision result is that of the f32 MFMA path (1.5e-6 vs 2.6e-6 on K = 64 dot products,
 * tools/ubench_bf16x6.hip), not that of a bf16 computation.  The backward is amk_attn_bwd, or amk_attn_bwd_kept
 * after amk_attn_fwd_x6_keep.
 * ws: amk_attn_fwd_x6_ws_bytes(B, H, J) bytes (48 KiB per (batch, head, 64-key tile): K and V split into
 * bf16 planes once per call by a pre-pass); contents undefined on return. */
int64_t amk_attn_fwd_x6_ws_bytes(int B, int H, int J);
int amk_attn_fwd_x6(const float* q, const float* k, const float* v, float* o, float* stats, void* ws,
                    const uint8_t* key_mask, const uint8_t* causal_mask,
                    int B, int H, int I, int J, int D,
                    int64_t q_sb, int64_t q_st, int64_t q_sh,
                    int64_t k_sb, int64_t k_st, int64_t k_sh,
                    int64_t v_sb, int64_t v_st, int64_t v_sh,
                    int64_t o_sb, int64_t o_st, int64_t o_sh,
                    float scale, void* stream);
/* amk_attn_fwd_x6 that also leaves its raw scores (the split-bf16 products, before any fill) for amk_attn_bwd_kept:
 * `scores` as for amk_attn_fwd_keep (non-null, 16-byte aligned, amk_attn_scores_bytes(B, H, I, J) bytes, same layout),
 * head dim 64 only.  The backward then forms P from the very scores the forward's statistics were taken from.
 * (Added within 0.4.0: an addition only, no signature changed.) */
int amk_attn_fwd_x6_keep(const float* q, const float* k, const float* v, float* o, float* stats, void* ws, float* scores,
                         const uint8_t* key_mask, const uint8_t* causal_mask,
                         int B, int H, int I, int J, int D,
                         int64_t q_sb, int64_t q_st, int64_t q_sh,
                         int64_t k_sb, int64_t k_st, int64_t k_sh,
                         int64_t v_sb, int64_t v_st, int64_t v_sh,
                         int64_t o_sb, int64_t o_st, int64_t o_sh,
                         float scale, void* stream);

/* --------------------------------------------------------------------------
 * Single-token attention against a key / value cache (KV-cached decoding), f32, with the cache append fused in
 * (csrc/attn_decode.hip).  Replaces, for ONE new query row per (batch, head), the core of
 * models/softmax_attention.py:62-76 as the sampling loop of models/parti.py:135-152 needs it once the keys and
 * values of the earlier rows are kept instead of recomputed.  (Added within 0.4.0, same library version: an
 * addition only, no signature changed.)
 *
 *   q, k_new, v_new  one row per (b, h), addressed  base + b*sb + h*sh + d: the (B, 1, h*D) and (B, 1, 2*h*D)
 *                    projection outputs in place; k_new and v_new are two pointers into one '(kv h d)' row and
 *                    share their strides (new_sb, new_sh).
 *   k_cache, v_cache `capacity` rows per batch, addressed  b*c_sb + t*c_st + h*c_sh + d  (shared strides): one
 *                    (B, capacity, 2*h*D) buffer per layer in the projection's own column layout.
 *   n_dev            DEVICE int32: the number of rows already valid.  It lives in device memory so that one
 *                    captured launch serves every position; the grid is sized from `capacity` on the host and
 *                    workgroups whose key range is empty leave at once.  Never written by the kernel.
 *   key_mask         uint8 (B, capacity) contiguous or NULL, 0 = fill -1e9 as in amk_attn_fwd; a row whose keys are
 *                    all masked gets the uniform 1/J weights of that contract.
 *
 * Append mode (k_new, v_new non-null; self-attention): with n = *n_dev < capacity, row n of both caches becomes the
 * new row and the query attends rows 0 .. n.  The workgroup that owns position n takes the row from k_new / v_new,
 * never from the cache, and is the only writer of cache row n.  n_dev must not be NULL.
 * Read mode (k_new, v_new NULL; cross-attention): the query attends rows 0 .. n - 1; n_dev NULL means
 * n = capacity, with no device read.  The caches are not written.
 * n out of range (append: n < 0 or n >= capacity; read: n < 1 or n > capacity): no byte outside the buffers is
 * touched and o and the caches are left as they are.
 *
 * Scores are (q * scale) . k, the softmax runs in the exp2 domain, f32 throughout.  The keys are split over
 * workgroups (64 per chunk); with more than one chunk each leaves (m, l, o[D]) in ws and a second launch on `stream`,
 * one workgroup per (b, h), adds the partials in chunk order.  No f32 atomics on data, no counters and no memset:
 * bitwise reproducible run to run and independent of B, and the workspace carries no state between calls (nothing
 * in it needs zeroing).  An in-launch reduction on a ticket counter was measured against this form and lost
 * (DESIGN.md section 4i); it is not in the library.
 * ws: amk_attn_decode_ws_floats(B, H, D, capacity) floats, 16-byte aligned, contents undefined on entry and on
 * return.
 * D: a multiple of 32 from 32 to 256, else AMK_EUNSUPPORTED before any device work (as B or H above 65535).
 * AMK_EINVAL: a null q, cache, o or ws, only one of k_new / v_new, append mode without n_dev, a non-positive size,
 * a pointer not 16-byte aligned (n_dev: 4) or a stride that is not a multiple of 4 elements.
 * -------------------------------------------------------------------------- */
int64_t amk_attn_decode_ws_floats(int B, int H, int D, int capacity);
int amk_attn_decode(const float* q, const float* k_new, const float* v_new, float* k_cache, float* v_cache,
                    float* o, float* ws, const int32_t* n_dev, const uint8_t* key_mask,
                    int B, int H, int D, int capacity,
                    int64_t q_sb, int64_t q_sh, int64_t new_sb, int64_t new_sh,
                    int64_t c_sb, int64_t c_st, int64_t c_sh, int64_t o_sb, int64_t o_sh,
                    float scale, void* stream);

/* amk_attn_decode on a bf16 cache, for the decode under bf16 autocast (csrc/attn_decode.hip; replaces the same lines,
 * models/softmax_attention.py:62-76 for one new row inside the loop of models/parti.py:135-152, under torch.autocast).
 * The contract above holds word for word -- append and read mode, n_dev on the device, key_mask, out-of-range n, the
 * two launches, no atomics, bitwise reproducible and independent of B -- with these differences:
 *   q, k_new, v_new, k_cache, v_cache and o are bf16.  Every stride is in elements and a multiple of 8; the pointers
 *   are 16-byte aligned.  ws is the same f32 workspace, amk_attn_decode_ws_floats(B, H, D, capacity) floats.
 *   bf16 -> f32 is exact; q is scaled in f32 after the conversion; scores, maxima, exp2, l and o stay f32 and p is never
 *   rounded to bf16.  o is rounded ONCE, to nearest even, on its final store.  Append mode writes cache row n as the bits
 *   of k_new / v_new.
 * (Added within 0.4.0, same library version: an addition only.) */
int amk_attn_decode_bf16(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                         void* o, float* ws, const int32_t* n_dev, const uint8_t* key_mask,
                         int B, int H, int D, int capacity,
                         int64_t q_sb, int64_t q_sh, int64_t new_sb, int64_t new_sh,
                         int64_t c_sb, int64_t c_st, int64_t c_sh, int64_t o_sb, int64_t o_sh,
                         float scale, void* stream);

/* --------------------------------------------------------------------------
 * The many-row form of amk_attn_decode: n new query rows per (batch, head) in one pass, for a decode that starts from
 * tokens the caller already has (csrc/attn_prefill.hip).  Replaces, for the n rows of a prompt, the core of
 * models/softmax_attention.py:62-76 as the sampling loop of models/parti.py:135-152 needs it on a cache that holds
 * p0 rows.  Inference only.  (Added within 0.4.0, same library version: an addition only.)
 *
 *   q, k_new, v_new  n rows per (b, h), addressed  base + b*sb + i*st + h*sh + d: the (B, n, h*D) and (B, n, 2*h*D)
 *                    projection outputs in place, or column slices of one; k_new and v_new share their strides.
 *   k_cache, v_cache, key_mask, scale, stream: as for amk_attn_decode.
 *   n_dev            DEVICE int32 holding p0, the number of rows already valid.  Never written.
 *   o                (B, n, h*D) under (o_sb, o_st, o_sh).
 *
 * Append mode (k_new, v_new non-null; causal self-attention): with p0 = *n_dev and p0 + n <= capacity, cache row
 * p0 + i becomes row i of k_new / v_new, bitwise, for every i < n, and row i of o is the softmax attention of q_i over
 * rows 0 .. p0 + i.  The causal predicate is computed from the indices; there is no mask tensor.  Keys j >= p0 are
 * taken from k_new / v_new, never from the cache, and every new cache row has exactly one writer in the launch, so no
 * workgroup reads a row that another writes.
 * Read mode (k_new, v_new NULL; the cross-attention of a prefill pass): all n rows attend rows 0 .. p0 - 1, all
 * `capacity` rows with n_dev NULL; masked keys are filled with -1e9.  The caches are not written.
 * Out of range (append: p0 < 0 or p0 + n > capacity; read: p0 < 1 or p0 > capacity): nothing is read or written.
 *
 * Row i runs the chain of amk_attn_decode at J = p0 + i + 1 keys (read mode: J = p0) with 64 keys per chunk: f32
 * scores in the exp2 domain, one maximum and one exp2 per key and chunk, the key groups added in order, and for a row
 * with more than one chunk (m, l, o[D]) per chunk in ws and a second launch on `stream` that adds them in chunk order.
 * A workgroup loads its chunk's K and V once for a block of 16 rows.  No f32 atomics on data and no hand-off between
 * workgroups: bitwise reproducible, and a row's result depends neither on B nor on how the rows are blocked.
 * amk_attn_prefill_bf16: q, k_new, v_new, the caches and o are bf16, the strides multiples of 8 elements; scores,
 * softmax and sums stay f32 and o is rounded ONCE, to nearest even, as amk_attn_decode_bf16 does.
 * ws: amk_attn_prefill_ws_floats(B, H, D, capacity, n) floats, 16-byte aligned, contents undefined on entry and return.
 * AMK_EUNSUPPORTED before any device work: D not a multiple of 32 from 32 to 256, B or H above 65535, a grid beyond
 * 2^31 - 1 workgroups.  AMK_EINVAL: a null q, cache, o or ws, only one of k_new / v_new, append mode without n_dev, a
 * non-positive size (n = 0 included), a pointer not 16-byte aligned (n_dev: 4), a stride off its multiple (f32: 4).
 * -------------------------------------------------------------------------- */
int64_t amk_attn_prefill_ws_floats(int B, int H, int D, int capacity, int n);
int amk_attn_prefill(const float* q, const float* k_new, const float* v_new, float* k_cache, float* v_cache,
                     float* o, float* ws, const int32_t* n_dev, const uint8_t* key_mask,
                     int B, int H, int D, int capacity, int n,
                     int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t new_sb, int64_t new_st, int64_t new_sh,
                     int64_t c_sb, int64_t c_st, int64_t c_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                     float scale, void* stream);
int amk_attn_prefill_bf16(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                          void* o, float* ws, const int32_t* n_dev, const uint8_t* key_mask,
                          int B, int H, int D, int capacity, int n,
                          int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t new_sb, int64_t new_st, int64_t new_sh,
                          int64_t c_sb, int64_t c_st, int64_t c_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                          float scale, void* stream);

/* A few rows times a weight matrix on bf16 MFMA (csrc/gemm_rows_bf16.hip):  y (M, N) = x (M, K) . w (N, K)^T + bias.
 * Replaces nn.Linear under torch.autocast where M is the batch of a decode step: the projections of
 * models/softmax_attention.py:30-44 and :78-81, the two Linear layers of models/transformer.py:22-43 and the logits of
 * models/parti.py:146, each for ONE new row per sequence.
 *   x (M, K) and w (N, K) bf16, row strides ldx / ldw in elements (multiples of 8, at least K), 16-byte aligned;
 *   bias (N) f32 or NULL, added in f32; accumulation f32; y f32 (out_bf16 = 0) or bf16 rounded once to nearest even
 *   (out_bf16 != 0), row stride ldy (a multiple of 4, at least N).
 * Any M, N, K >= 1.  Tails are predicates: no byte past a row's K elements is read, whatever the padding up to ldx / ldw
 * holds.  Rows go in blocks of 16 on v_mfma_f32_16x16x32_bf16; one workgroup per (16 columns, 16 rows) whose four waves
 * split K and add their partial tiles in wave order.  No atomics, nothing split across workgroups: bitwise reproducible,
 * and row m of y is bitwise independent of M and of the other rows.
 * AMK_EINVAL: a null x, w or y, a non-positive size, a leading dimension below its row length or off its multiple, a
 * misaligned pointer.  (Added within 0.4.0, same library version: an addition only.) */
int amk_gemm_rows_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias,
                       void* y, int64_t ldy, int M, int N, int K, int out_bf16, void* stream);

/* Backward of amk_attn_fwd (autograd of the same reference lines).
 * Inputs: q,k,v,o,stats as in the forward, d_o (gradient of o, same addressing
 * as o with its own strides).  Outputs: dq (q-like), dk (k-like), dv (v-like),
 * each fully overwritten.  delta_ws: workspace of amk_attn_bwd_ws_floats(B, H, I, J, stages) floats
 * (B*H*I rounded up to 4, unless AMK_ATTN_BWD_DQ_REPRO asks for more).
 * Gradients do not flow through filled (-1e9) positions, as in masked_fill.
 * `stages` selects the launches.  bit 0: delta = rowsum(dO*O) into delta_ws (must have run
 * before any other bit).  Then EITHER bit 3 (AMK_ATTN_BWD_FUSED): one pass, each of the five
 * products computed once, dq accumulated with f32 atomics (dq must be the dense (B,I,H,D) layout;
 * it is zeroed here; dq differs in the last bits from run to run; key and causal masks are taken;
 * falls back to the two-kernel path when dq is strided, and at the head dims that have no one-pass
 * kernel: it exists for 32, 64 and 128) -- OR bits 1 and 2: two recompute kernels, dK/dV and dQ,
 * no atomics, bitwise reproducible, one template family for every head dim.  Profilers time one
 * stage by passing its bit. */
#define AMK_ATTN_BWD_DELTA 1
#define AMK_ATTN_BWD_DKDV 2
#define AMK_ATTN_BWD_DQ 4
#define AMK_ATTN_BWD_FUSED 8
#define AMK_ATTN_BWD_ALL 7          /* delta + dK/dV + dQ: reproducible */
#define AMK_ATTN_BWD_FAST 9         /* delta + fused */
/* fused pass only: keys per workgroup (neither bit: 256 when J >= 256, else 128).  256 halves the
 * number of atomic adds per dq element (J / 256 instead of J / 128). */
#define AMK_ATTN_BWD_KEYS128 16
#define AMK_ATTN_BWD_KEYS256 32
/* fused pass only: bitwise reproducible dq.  No atomics: a workgroup that holds every key of its (batch, head)
 * (J <= keys per workgroup) stores dq directly; otherwise every key block stores its partial and a second
 * launch sums the partials in key-block order.  delta_ws must then hold amk_attn_bwd_ws_floats(...) floats
 * (the deltas followed by the partials). */
#define AMK_ATTN_BWD_DQ_REPRO 64
#define AMK_ATTN_BWD_FAST_REPRO 73  /* delta + fused + reproducible dq */
/* amk_attn_bwd_kept only, with AMK_ATTN_BWD_FUSED: the dV and dK products of the one-pass kernel on split-bf16 MFMA
 * (six partial products of three bf16 planes per operand, f32 accumulation: f32-grade results, see amk_attn_fwd_x6;
 * csrc/attn_bwd_fused_x6.hip).  dq is that of the call without the bit, bit for bit under AMK_ATTN_BWD_DQ_REPRO.
 * Head dim 64 at 256 keys per workgroup (J >= 256, or AMK_ATTN_BWD_KEYS256) with the dense dq layout; every other
 * call with the bit set -- amk_attn_bwd included -- is refused with AMK_EUNSUPPORTED, nothing launched. */
#define AMK_ATTN_BWD_X6 128
int64_t amk_attn_bwd_ws_floats(int B, int H, int I, int J, int stages);
int amk_attn_bwd(const float* q, const float* k, const float* v, const float* o,
                 const float* stats, const float* d_o,
                 float* dq, float* dk, float* dv, float* delta_ws,
                 const uint8_t* key_mask, const uint8_t* causal_mask,
                 int B, int H, int I, int J, int D,
                 int64_t q_sb, int64_t q_st, int64_t q_sh,
                 int64_t k_sb, int64_t k_st, int64_t k_sh,
                 int64_t v_sb, int64_t v_st, int64_t v_sh,
                 int64_t o_sb, int64_t o_st, int64_t o_sh,
                 int64_t do_sb, int64_t do_st, int64_t do_sh,
                 int64_t dq_sb, int64_t dq_st, int64_t dq_sh,
                 int64_t dk_sb, int64_t dk_st, int64_t dk_sh,
                 int64_t dv_sb, int64_t dv_st, int64_t dv_sh,
                 float scale, int stages, void* stream);
/* amk_attn_bwd reading the scores amk_attn_fwd_keep left (same q, k, masks, scale): the fused pass skips
 * its S = QK^T product; the results are those of amk_attn_bwd bit for bit (dq up to the atomics' order).
 * `stages` must contain AMK_ATTN_BWD_FUSED; when the fused pass cannot run (strided dq) the two recompute
 * kernels run and the scores are not read at head dim 64; head dims 32 / 128 refuse that call
 * (AMK_EUNSUPPORTED). */
int amk_attn_bwd_kept(const float* scores, const float* q, const float* k, const float* v, const float* o,
                      const float* stats, const float* d_o,
                      float* dq, float* dk, float* dv, float* delta_ws,
                      const uint8_t* key_mask, const uint8_t* causal_mask,
                      int B, int H, int I, int J, int D,
                      int64_t q_sb, int64_t q_st, int64_t q_sh,
                      int64_t k_sb, int64_t k_st, int64_t k_sh,
                      int64_t v_sb, int64_t v_st, int64_t v_sh,
                      int64_t o_sb, int64_t o_st, int64_t o_sh,
                      int64_t do_sb, int64_t do_st, int64_t do_sh,
                      int64_t dq_sb, int64_t dq_st, int64_t dq_sh,
                      int64_t dk_sb, int64_t dk_st, int64_t dk_sh,
                      int64_t dv_sb, int64_t dv_st, int64_t dv_sh,
                      float scale, int stages, void* stream);

/* --------------------------------------------------------------------------
 * VQ codebook nearest-neighbour lookup.
 * Replaces models/vitvqgan.py:151-171 (Codebook.forward) and :16-17 (l2_norm).
 *
 *   zn = z / max(||z||, 1e-12)                   (N,C)
 *   en = E / max(||E||, 1e-12)                   (K,C)
 *   dist[n,k] = (sum zn[n]^2 + sum en[k]^2) - 2 * <zn[n], en[k]>
 *   idx[n] = argmin_k dist[n,k]                  (first minimum on ties)
 *   zq[n]  = E[idx[n]] / max(||E[idx[n]]||, 1e-12)
 *   out[n] = zn[n] + (zq[n] - zn[n])             (straight-through value)
 *   sqerr_partial[w] = partial sums of (zq - zn)^2 ; the caller forms
 *        loss = (1 + beta) * sum(sqerr_partial) / (N*C)
 *
 * C must be 32, 64, 128 or 256; K is any positive size (the reference takes any codebook_size,
 * models/vitvqgan.py:141).  nsplit >= 1 splits the codebook over workgroups; internally the
 * normalised codebook is padded to Kp = amk_vq_padded_codes(K, nsplit) rows (whole 32-code tiles
 * per slice; the padding scores -inf and is never chosen).  Workspaces: en_ws Kp*C floats,
 * ee_ws Kp floats, pmin_ws N*nsplit floats, pidx_ws N*nsplit int32.  sqerr_partial holds
 * amk_vq_num_partials(N) floats.  The distance matrix is never written to HBM.
 * -------------------------------------------------------------------------- */
int64_t amk_vq_num_partials(int64_t N);
int amk_vq_padded_codes(int K, int nsplit);
int amk_vq_lookup_fwd(const float* z, const float* codebook, int64_t N, int K, int C, int nsplit,
                      float* en_ws, float* ee_ws, float* pmin_ws, int32_t* pidx_ws,
                      int64_t* idx, float* out, float* zq, float* zn, float* sqerr_partial,
                      void* stream);

/* Backward of Codebook.forward (autograd of models/vitvqgan.py:151-171).
 *   g_out (N,C): gradient of `out`; g_loss: DEVICE pointer to the scalar
 *   gradient of the loss.  dz (N,C) is overwritten; dcodebook (K,C) is zeroed
 *   here and then scatter-added by idx.
 *   dzn = g_out + g_loss*2*beta*(zn - zq)/(N*C);   dz = J_norm(z)^T dzn
 *   dzq = g_loss*2*(zq - zn)/(N*C);  dE[idx[n]] += J_norm(E[idx[n]])^T dzq */
int amk_vq_lookup_bwd(const float* z, const float* codebook, const float* zn, const float* zq,
                      const int64_t* idx, const float* g_out, const float* g_loss, float beta,
                      int64_t N, int K, int C, float* dz, float* dcodebook, void* stream);

/* The same backward without atomics: instead of scatter-adding into dcodebook, every row's contribution
 * J_norm(E[idx[n]])^T dzq[n] is written to ge_rows (N,C); the caller adds the rows into dcodebook[idx[n]] in an
 * order of its choosing (the Python binding uses a deterministic index_add_ when reproducible gradients are asked
 * for: AMK_DETERMINISTIC=1 / torch.use_deterministic_algorithms). */
int amk_vq_lookup_bwd_rows(const float* z, const float* codebook, const float* zn, const float* zq,
                           const int64_t* idx, const float* g_out, const float* g_loss, float beta,
                           int64_t N, int K, int C, float* dz, float* ge_rows, void* stream);

/* Codebook.indices_to_embeddings (models/vitvqgan.py:173-176): out[n] = l2norm(E[idx[n]]).
 * The indices are the caller's: one outside [0, K) is never dereferenced (it reads row 0 or K-1) and
 * is counted in *bad_count (device int32, zeroed by the caller; NULL = do not count) -- the reference
 * raises IndexError there (nn.Embedding), and so does the Python binding from the count.
 * amk_vq_lookup_bwd clamps its (forward-produced) indices the same way. */
int amk_vq_gather(const int64_t* idx, const float* codebook, int64_t N, int K, int C,
                  float* out, int32_t* bad_count, void* stream);

/* --------------------------------------------------------------------------
 * Top-k expert routing and grouped expert GEMMs.
 * Replace the per-expert Python loops (torch.where + gather + Linear + index_put) of
 * MoELayer.forward (models/moe.py:23-38) and SwitchHeadAttention.moe_v / moe_out
 * (models/switchhead_attention.py:58-88).  A routed "unit" u is a token (MoELayer) or a
 * (token, head) (SwitchHead); a "pair" is p = u*k + slot.
 * -------------------------------------------------------------------------- */

/* torch.topk(logits, k) + sigmoid of the selected logits, and the expert-major ordering.
 *   logits (U,E) -> ids int64 (U,k) descending by logit (lowest index on equal logits),
 *   gate (U,k) = sigmoid(selected logit); offsets int32 (E+1), perm int32 (U*k): pairs grouped
 *   by expert, ascending pair index inside an expert (deterministic).
 *   Workspaces: counts int32 (E), rank int32 (U*k), blockhist int32 (amk_moe_route_ws_ints(U,E,k)).
 *   k <= 8, E <= 1024. */
int64_t amk_moe_route_ws_ints(int64_t U, int E, int k);
int amk_moe_route(const float* logits, int64_t U, int E, int k,
                  int64_t* ids, float* gate, int32_t* counts, int32_t* rank, int32_t* blockhist,
                  int32_t* offsets, int32_t* perm, void* stream);

/* Y[p,:] = A[p / a_div, :] * W[e(p)]^T (+ bias[e(p)]) for every pair: the expert Linear layers
 * (models/moe.py:34-36, switchhead_attention.py:69-71,86).  A rows have Kd floats at stride lda;
 * W is (E,N,Kd) contiguous, bias (E,N) or NULL, Y is (P,N).  N, Kd, lda multiples of 4. */
int amk_grouped_gemm_nt(const float* A, int64_t lda, int a_div, const float* W, const float* bias,
                        const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                        float* Y, void* stream);

/* Y[p,:] = scale[p] * (A[p / a_div, :] * W[e(p)]): input gradient of the expert Linear.
 * A rows have N floats, Y is (P,Kd); scale (P) or NULL. */
int amk_grouped_gemm_nn(const float* A, int64_t lda, int a_div, const float* W, const float* scale,
                        const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                        float* Y, void* stream);

/* The same two products with the sum over the pairs of an output row folded in: pair p ADDS its row into
 * Y[p / y_div, :] (f32 atomics; Y is ((P-1)/y_div + 1, N) resp. (.., Kd) and must be ZEROED by the caller).
 * Replaces amk_grouped_gemm_* followed by amk_moe_combine where the combine is un-weighted -- the head / slot sum
 * of SwitchHead's output experts (switchhead_attention.py:86-87,115: 16 pairs per token, a 272 MB per-pair
 * intermediate at the ViTMoE layer size) and the sum of the input gradients of its V experts -- at the price of
 * the reference's fixed accumulation order (ascending expert id): sums differ in the last bits from run to run.
 * Needs the wide kernels: N >= 128 and Kd % 32 == 0 (nt), Kd >= 128 and N % 32 == 0 (nn), buffers below 2 GB;
 * AMK_EUNSUPPORTED otherwise. */
int amk_grouped_gemm_nt_acc(const float* A, int64_t lda, int a_div, const float* W, const float* bias,
                            const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                            float* Y, int y_div, void* stream);
int amk_grouped_gemm_nn_acc(const float* A, int64_t lda, int a_div, const float* W, const float* scale,
                            const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                            float* Y, int y_div, void* stream);

/* dW[e] = sum_{p in e} scale[p] * G[p / g_div, :]^T (x) X[p / x_div, :]   (E,N,Kd), fully
 * overwritten; dbias[e] = sum_{p in e} scale[p] * G[p / g_div, :] (E,N) or NULL.  (With few output tiles and long
 * experts the entry zeroes dW and two workgroups per tile add their halves of the pairs: 0 + a + b, the same bits in
 * either order.) */
int amk_grouped_gemm_wgrad(const float* G, int64_t ldg, int g_div, const float* X, int64_t ldx, int x_div,
                           const float* scale, const int32_t* offsets, const int32_t* perm,
                           int64_t P, int E, int N, int Kd, float* dW, float* dbias, void* stream);

/* out[g,:] = sum_{o<outer} ( sum over the k slots of unit g*outer+o, in ASCENDING EXPERT ID,
 * of scale[p]*Y[p,:] ): the accumulation order of the reference loops (moe.py:32-36) and the
 * head sum of switchhead_attention.py:115.  scale (G*outer*k) or NULL (moe_out is un-weighted). */
int amk_moe_combine(const float* Y, const int64_t* ids, const float* scale, int64_t G, int outer, int k,
                    int N, float* out, void* stream);

/* The selection alone: ids (U,k) = top-k expert indices of every logits row (descending value, lowest index on ties, as
 * torch.topk), gate (U,k) = sigmoid of the selected logits -- the first stage of amk_moe_route, for callers that build
 * their own lists (amk_moe_route_distinct). */
int amk_moe_topk(const float* logits, int64_t U, int E, int k, int64_t* ids, float* gate, void* stream);

/* Lists of the DISTINCT (row group, expert) combinations of a routing: group g = pairs g*fan .. g*fan+fan-1 (in
 * SwitchHead one token's heads x slots).  Where all pairs of a group read the same input row (moe_v,
 * switchhead_attention.py:58-73: the token's row for every head) or their products are summed over the group anyway
 * (moe_out, :75-88,115), an expert's product is needed once per distinct (group, expert) -- 12.9 instead of 16 per
 * token at E 32, h 8, top-2.  offsets (E+1) / perm (up to G*min(fan,E) entries) list "virtual pairs" g*E + e by expert,
 * groups ascending; the amk_grouped_gemm_* entry points run on them unchanged with P = G*E, a_div = E (input row g,
 * output row g*E + e).  mask (G) is a workspace.  E <= 64, fan <= 4096. */
int amk_moe_route_distinct(const int64_t* ids, int64_t G, int fan, int E, uint64_t* mask,
                           int32_t* offsets, int32_t* perm, void* stream);

/* amk_moe_combine / amk_moe_gate_grad reading such per-(group, expert) rows: pair p reads Y row
 * (p / v_div) * E + ids[p]  (v_div = pairs per group; v_div == 0: row p, the plain entry points). */
int amk_moe_combine_rows(const float* Y, const int64_t* ids, const float* scale, int64_t G, int outer, int k,
                         int N, int v_div, int E, float* out, void* stream);
int amk_moe_gate_grad_rows(const float* d_out, const float* Y, const int64_t* ids, const float* gate,
                           int64_t P, int k, int E, int N, int g_div, int v_div, float* dlogits, void* stream);

/* Z[g, e, :] = sum over the fan pairs of row g (pairs g*fan .. g*fan+fan-1) that chose expert e = ids[p] of
 * scale[p] * A[p / a_div, :]  (d floats at stride lda; scale (G*fan) or NULL).  Z (G, E*d) is fully overwritten, in a
 * fixed order.  With it the head / slot sum of SwitchHead's output experts (switchhead_attention.py:86-87,115) is one
 * dense product Z x (E*d, N) instead of amk_grouped_gemm_nt + amk_moe_combine and their (pairs, N) intermediate, and
 * likewise the input gradient of its V experts (switchhead_attention.py:69-71) -- worth it where a row has at least
 * E/2 pairs (the dense product does E/fan times the routed FLOPs).  d, lda multiples of 4; fan <= 4096. */
int amk_moe_expert_sums(const float* A, int64_t lda, int a_div, const int64_t* ids, const float* scale,
                        int64_t G, int fan, int E, int d, float* Z, void* stream);

/* Gradient of the gate logits through sigmoid(topk): dlogits (P/k, E) fully overwritten,
 * dlogits[p/k, ids[p]] = gate[p]*(1-gate[p]) * <d_out[p / g_div, :], Y[p, :]>, zero elsewhere. */
int amk_moe_gate_grad(const float* d_out, const float* Y, const int64_t* ids, const float* gate,
                      int64_t P, int k, int E, int N, int g_div, float* dlogits, void* stream);

/* --------------------------------------------------------------------------
 * AgentAttention core.
 * Replaces models/agent_attention.py:55-73: agent tokens A = adaptive average pool of q over
 * the sequence into P bins per head (AdaptiveAvgPool2d over the (t, h) plane with
 * h == P, the only configuration in which the reference runs -- SURVEY.md section 0.5),
 *   V_a = softmax((A*scale) K^T) V,   O = softmax((q*scale) A^T) V_a + dwc(v)
 * where dwc is the depthwise 3x3 convolution (weights (D,1,3,3), bias (D)) over the
 * (head, token) plane.  The reference's scalar bias1 / bias2 are added to whole softmax rows,
 * so they change nothing and receive zero gradient; they do not cross the ABI.
 * q,k,v,o addressed like amk_attn_fwd (T rows).  Saved for the backward: agents (B,H,P,D),
 * vagent (B,H,P,D), stats1 (B,H,P,2) = {row max, row sum} of the aggregation softmax.
 * D is 32, 64 or 128 (any other head dim: AMK_EUNSUPPORTED before any device work), P <= 16, P <= T.
 * The sequence is processed in chunks of 128 tokens (64 at D = 128), one workgroup per
 * (batch, head, chunk); sums over tokens go through per-chunk partials in the caller's workspace
 * `ws` (amk_agent_ws_floats_dh(B,H,T,P,D,backward) floats, contents undefined on return) and are
 * folded in chunk order, so results are bitwise reproducible.
 *   head dim | chunk | backward chunk kernels
 *   32       | 128   | LDS-staged (AMK_AGENT_STREAM does not apply)
 *   64       | 128   | streaming for P <= 8 (AMK_AGENT_STREAM=0: LDS-staged), LDS-staged for P > 8
 *   128      |  64   | LDS-staged (AMK_AGENT_STREAM does not apply)
 * AMK_AGENT_STREAM is read on every call of amk_agent_attn_bwd.
 * amk_agent_num_chunks / amk_agent_ws_floats are the D = 64 sizes; the _dh forms take the head
 * dim and return 0 for an unsupported one.
 * -------------------------------------------------------------------------- */
int amk_agent_num_chunks(int T);                                  /* ceil(T / 128); 0 for T <= 0 */
int64_t amk_agent_ws_floats(int B, int H, int T, int P, int backward); /* workspace size in floats */
int amk_agent_num_chunks_dh(int T, int D);                        /* ceil(T / chunk(D)) */
int64_t amk_agent_ws_floats_dh(int B, int H, int T, int P, int D, int backward);

int amk_agent_attn_fwd(const float* q, const float* k, const float* v, const float* conv_w, const float* conv_b,
                       float* o, float* agents, float* vagent, float* stats1, float* ws,
                       int B, int H, int T, int D, int P,
                       int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                       int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                       float scale, void* stream);

/* Backward of amk_agent_attn_fwd: dq, dk, dv fully overwritten (q/k/v-like addressing);
 * dconvw_part (B*H*NC, 9, D) and dconvb_part (B*H*NC, D), NC = amk_agent_num_chunks_dh(T, D), are
 * per-(batch, head, chunk) partial sums of the convolution weight / bias gradients (the caller
 * sums over the first axis; weight element [c][0][a][b] is partial [.., a*3+b, c]);
 * ws: amk_agent_ws_floats_dh(B,H,T,P,D,1) floats. */
int amk_agent_attn_bwd(const float* q, const float* k, const float* v, const float* conv_w, const float* d_o,
                       const float* agents, const float* vagent, const float* stats1,
                       float* dq, float* dk, float* dv, float* ws, float* dconvw_part, float* dconvb_part,
                       int B, int H, int T, int D, int P,
                       int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                       int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t do_sb, int64_t do_st, int64_t do_sh,
                       int64_t dq_sb, int64_t dq_st, int64_t dq_sh, int64_t dk_sb, int64_t dk_st, int64_t dk_sh,
                       int64_t dv_sb, int64_t dv_st, int64_t dv_sh, float scale, void* stream);

/* The sums over the first axis of amk_agent_attn_bwd's partials, in a fixed order, in one launch: dconvw (D, 1, 3, 3)
 * = the depthwise convolution's weight gradient in the parameter's layout (agent_attention.py:41-45), dconvb (D). */
int amk_agent_conv_grad_reduce(const float* dconvw_part, const float* dconvb_part, int64_t rows, int D,
                               float* dconvw, float* dconvb, void* stream);

/* The AgentAttention core (models/agent_attention.py:55-73) on bf16 elements, for torch.autocast(bfloat16): q, k, v, o
 * (and d_o, dq, dk, dv in the backward) are bf16 views, strides in elements; agents, vagent, stats1, the workspaces,
 * the convolution's parameters and its gradient partials stay f32 and amk_agent_conv_grad_reduce is shared.  The same
 * kernels as the f32 entry points above, instantiated on another element type: a lane's 4 channels are one 8-byte
 * access, widened exactly on the load; all arithmetic is the f32 arithmetic of amk_agent_attn_fwd / _bwd in the same
 * order; o, dq, dk, dv are rounded to nearest even once, on the store.  So the f32 outputs equal bit for bit those of
 * the f32 entry points on the upcast tensors, and the bf16 outputs are their f32 outputs rounded once.  dq is the sum
 * of a stage-2 part and a pooled part written by two kernels: the first part crosses in f32 through the workspace,
 * which is why the backward's workspace is (B,H,T,D) floats larger:
 *   amk_agent_bf16_ws_floats(.., 0) = amk_agent_ws_floats_dh(.., 0),  (.., 1) = amk_agent_ws_floats_dh(.., 1) + B*H*T*D.
 * Refused before any device work: null pointers, non-positive sizes, a bf16 tensor (or the backward's ws) that is not
 * 16-byte aligned, a stride that is no multiple of 8 elements (AMK_EINVAL); D outside {32, 64, 128}, P > 16 or P > T,
 * a batch entry of 2 GiB or more (2-byte elements) or negative strides, a grid beyond 2^31 (AMK_EUNSUPPORTED).
 * AMK_AGENT_STREAM is read on every call of amk_agent_attn_bf16_bwd, as in amk_agent_attn_bwd. */
int64_t amk_agent_bf16_ws_floats(int B, int H, int T, int P, int D, int backward);

int amk_agent_attn_bf16_fwd(const void* q, const void* k, const void* v, const float* conv_w, const float* conv_b,
                            void* o, float* agents, float* vagent, float* stats1, float* ws,
                            int B, int H, int T, int D, int P,
                            int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                            int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                            float scale, void* stream);

int amk_agent_attn_bf16_bwd(const void* q, const void* k, const void* v, const float* conv_w, const void* d_o,
                            const float* agents, const float* vagent, const float* stats1,
                            void* dq, void* dk, void* dv, float* ws, float* dconvw_part, float* dconvb_part,
                            int B, int H, int T, int D, int P,
                            int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                            int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t do_sb, int64_t do_st, int64_t do_sh,
                            int64_t dq_sb, int64_t dq_st, int64_t dq_sh, int64_t dk_sb, int64_t dk_st, int64_t dk_sh,
                            int64_t dv_sb, int64_t dv_st, int64_t dv_sh, float scale, void* stream);

/* --------------------------------------------------------------------------
 * Residual-add + LayerNorm and the bias-gradient column sum (the
 * pre-LN / residual epilogues around the attention and FFN of models/vitvqgan.py:44-61 and
 * models/transformer.py:11-19,58-76).
 *   forward : h = x + res (written only when res != NULL; then h != NULL too);  y = LN(h)*gamma + beta
 *             mean, rstd (M) are saved for the backward.  eps as torch.nn.LayerNorm (1e-5 default).
 *   backward: dh = LN'(dy) + dh_in (dh_in may be NULL); dgb_part (amk_rowsum_num_partials(M), 2, D)
 *             holds per-workgroup partial sums of dgamma (row 0) and dbeta (row 1): the caller sums axis 0.
 *             `h` is the forward's h (or x when there was no residual).
 *   colsum  : part (amk_rowsum_num_partials(M), N) partial column sums of x (M, N); caller sums axis 0.
 * Widths: multiples of 4 up to 4096; all matrices row-major contiguous; HBM-bound, one pass each.
 * -------------------------------------------------------------------------- */
int amk_rowsum_num_partials(int64_t M);
int amk_add_layernorm_fwd(const float* x, const float* res, const float* gamma, const float* beta,
                          int64_t M, int D, float eps, float* h, float* y, float* mean, float* rstd, void* stream);
int amk_add_layernorm_bwd(const float* dy, const float* h, const float* dh_in, const float* gamma,
                          const float* mean, const float* rstd, int64_t M, int D, float* dh, float* dgb_part,
                          void* stream);
int amk_colsum(const float* x, int64_t M, int N, float* part, void* stream);

/* --------------------------------------------------------------------------
 * Fused SwiGLU gate (epilogue of the ViT-VQGAN FFN):
 *   out[m, j] = silu(ab[m, j]) * ab[m, H + j]      ab: (M, 2H) = w12(x), out: (M, H)
 * replaces chunk -> silu -> mul of the SwiGLU the reference's FeedForward keywords describe
 * (models/vitvqgan.py:20-34).  Backward writes d_ab (M, 2H) = (d_a | d_b) in one pass
 * (no chunk-backward concatenation).  H must be a multiple of 4.
 * -------------------------------------------------------------------------- */
int amk_swiglu_fwd(const float* ab, int64_t M, int H, float* out, void* stream);
int amk_swiglu_bwd(const float* ab, const float* d_out, int64_t M, int H, float* d_ab, void* stream);

/* GEGLU gate of the transformer FFN (models/transformer.py:22-27): out[m, j] = gelu(ab[m, j]) * ab[m, H + j]
 * with the exact (erf) GELU of F.gelu; same layout and rules as the SwiGLU pair above. */
int amk_geglu_fwd(const float* ab, int64_t M, int H, float* out, void* stream);
int amk_geglu_bwd(const float* ab, const float* d_out, int64_t M, int H, float* d_ab, void* stream);

/* --------------------------------------------------------------------------
 * Optimizer step over flat gradient buckets.
 * Replaces, per phase of the train step, accelerator.clip_grad_norm_ + Adam.step + zero_grad
 * (trainers/vitgqgan.py:67-68,159-163,185-189; trainers/vit.py:29-31,74-76 for AdamW):
 *
 *   amk_sumsq_partials   partials[w] (w < amk_opt_num_partials()) = sum of x^2 over the w-th fixed range
 *   amk_adam_flat_step   norm = sqrt(sum of all `partials`), coef = min(1, max_norm / (norm + 1e-6))
 *                        (max_norm <= 0: no clipping), then for every element of an ACTIVE parameter
 *                          g *= coef; [Adam: g += wd * p | AdamW: p -= lr * wd * p]
 *                          m += (1 - beta1) (g - m); v = beta2 v + (1 - beta2) g^2
 *                          p -= tab.step_size * m / (sqrt(v) / tab.bc2_sqrt + eps)
 *                        and grad is left zeroed (all parameters).  torch.optim.Adam / AdamW arithmetic.
 * Buffers are flat fp32 arrays of n elements, n a multiple of 256; the i-th segment of 256 elements
 * belongs to parameter seg_param[i]; param_tab is (P, 4) floats per step: {active (0 / 1),
 * lr / (1 - beta1^t), sqrt(1 - beta2^t), weight-decay factor} with t the parameter's own step count.
 * `decoupled`: bit 0 selects AdamW (1) or Adam-with-L2 (0); bit 1 set = the decay factor is read per parameter from
 * param_tab[.][3] (wd for Adam, lr * wd for AdamW: per-group weight decay as trainers/muse.py:48-58 sets it up, and a
 * learning rate that lives on the device for a graph-captured step) instead of the `lr` / `weight_decay` arguments.
 * Inactive parameters (no gradient this step) are left untouched, as optimizers skip .grad None.
 * -------------------------------------------------------------------------- */
int amk_opt_num_partials(void);
int amk_sumsq_partials(const float* x, int64_t n, float* partials, void* stream);
int amk_adam_flat_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       const int32_t* seg_param, const float* param_tab,
                       const float* partials, int n_partials,
                       float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int decoupled, float* norm_out, void* stream);
/* The same step, also refreshing param_bf16 (n bf16 values, 8-byte aligned; NULL: none): the copy of the parameters the
 * mixed-precision GEMMs read, so that torch.autocast's per-call weight casts (accelerator.autocast, trainers/
 * vitgqgan.py:139-190) have nothing left to do. */
int amk_adam_flat_step_shadow(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                              const int32_t* seg_param, const float* param_tab,
                              const float* partials, int n_partials,
                              float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                              int decoupled, float* norm_out, void* param_bf16, void* stream);

/* --------------------------------------------------------------------------
 * One step of the masked-token parallel decode.
 * Replaces, per step of MUSE.generate / MaskGitTransformer.generate (models/muse.py:211-236,
 * models/maskgit.py:255-272), the chain CFG combine -> softmax -> filter_logits (top-k, scatter) ->
 * gumbel_softmax(tau).argmax -> probs.gather -> masked writes over the (R, V) logits:
 *   s      = null + cfg_scale * (logits - null)       (null_logits NULL: s = logits)
 *   pred   = argmax over the `keep` largest s of (s + g)    (tau > 0; tau == 0 gives 0, as the reference's
 *            division by zero does -- every Gumbel-softmax entry is NaN and argmax returns 0)
 *   ids[r] = pred where mask[r] != 0 (mask NULL: every row)
 *   scores[r] = softmax(s)[pred]; rows with mask[r] == 0 get `unmasked_score` when it is >= 0
 * g: `gumbel` (R, V) when given, else -log(-log u) with u from Philox4x32-10 keyed by (seed, offset, row, j/4)
 * -- torch's distribution, not its stream.  R rows of V logits (V % 4 == 0, V <= 36864), contiguous.
 * -------------------------------------------------------------------------- */
int amk_sample_step(const float* logits, const float* null_logits, float cfg_scale,
                    const float* gumbel, uint64_t seed, uint64_t offset, float tau,
                    int64_t R, int V, int keep, const uint8_t* mask, float unmasked_score,
                    int64_t* ids, float* scores, void* stream);

/* --------------------------------------------------------------------------
 * Dense GEMM with split-bf16 products (the projections around the attention
 * core and the FFN -- nn.Linear in models/softmax_attention.py:30-42,80 and models/vitvqgan.py:20-61):
 *   C[m, n] = sum_k A[m, k] * W[n, k] (+ bias[n])        A (M, K), W (N, K), C (M, N), all f32, row-major
 * i.e. F.linear(A, W, bias); the input gradient dX = dY W is the same call with W^T in W's place.
 * Every operand is split into three bf16 parts (24 mantissa bits) and every product is the sum of six
 * exact partial products accumulated in f32 (v_mfma_f32_32x32x16_bf16): f32-level error (tests compare
 * with float64), 6/16 of the matrix-pipe time of the exact-f32 MFMA.  Its bound is the bf16 MFMA peak / 6.
 * The weight is split once per call by amk_gemm_x6_split into `planes` (amk_gemm_x6_planes_bytes(N, K)
 * bytes: three bf16 planes, K padded to 32); the activations are split inside the GEMM.
 * lda / ldw / ldc: row strides in elements (multiples of 4); K a multiple of 4; pointers 16-byte aligned.
 * -------------------------------------------------------------------------- */
int64_t amk_gemm_x6_planes_bytes(int N, int K);
int amk_gemm_x6_split(const float* W, int64_t ldw, int N, int K, void* planes, void* stream);
int amk_gemm_x6_nt(const float* A, int64_t lda, const void* w_planes, const float* bias,
                   float* C, int64_t ldc, int M, int N, int K, void* stream);
/* The same product on planes that are already there (the plane shadow of amk.optim.FlatAdam), with what the exact-f32
 * path fuses on the train step's shapes:
 *   amk_gemm_x6_nt2            C = A W^T + A2 W2^T, one contraction in two segments (dX = dq Wq + dkv Wkv against the planes
 *                              of Wq^T and Wkv^T, each [3][N][K* padded to 32]).
 *   amk_gemm_x6_nt_swiglu      (a | b) = A w12^T + bias (w12 (2H, K)); gate = silu(a) * b (M, H); (a | b) (M, 2H) is written
 *                              only when `ab` is given.  `gate_planes` hold w12 in the GATE ORDER: amk_gemm_x6_gate_rows(H)
 *                              = 128 ceil(H / 64) rows per plane, plane row 128 t + j = row 64 t + j of w12 for j < 64, row
 *                              H + 64 t + j - 64 for j >= 64, zero rows where that column is past H.
 *   amk_gemm_x6_nt_swiglu_bwd  dGate = dY W3 against the planes of W3^T ([3][H][K padded]); reads (a | b), writes (dA | dB).
 *   amk_gemm_x6_split_table    the split of every weight of one flat parameter buffer in one launch.  `table` (device,
 *                              n_entries x 8 int64): {src, R, K, H, blk0, dst_w, dst_wt, NR} -- W = flat + src is (R, K)
 *                              row-major (R, K multiples of 4), its planes go to planes + dst_w (bf16 elements) as
 *                              [3][NR][K padded] in row order (H = 0, NR >= R) or in the gate order (H > 0, R = 2H), the
 *                              planes of W^T to planes + dst_wt as [3][K][R padded] (dst_wt < 0: none); the entry owns
 *                              workgroups blk0 .. blk0 + ceil(R / 32) ceil(K / 32) - 1 of the n_blocks.  `planes` must have
 *                              been zeroed once (gate-order rows past H are never written); an entry that does not fit
 *                              flat_elems / planes_elems writes nothing. */
int amk_gemm_x6_nt2(const float* A, int64_t lda, const void* planes, int K, const float* A2, int64_t lda2,
                    const void* planes2, int K2, float* C, int64_t ldc, int M, int N, void* stream);
/* C1 = A W1^T (M, N1) and C2 = A W2^T (M, N2) in one launch that reads and splits A once (the q and kv projections of
 * one x); preconditions and error codes of amk_gemm_x6_nt, and AMK_EUNSUPPORTED for K > 256.  Bit for bit the two
 * amk_gemm_x6_nt calls. */
int amk_gemm_x6_nt_cols2(const float* A, int64_t lda, const void* planes1, const void* planes2, float* C1,
                         int64_t ldc1, float* C2, int64_t ldc2, int M, int N1, int N2, int K, void* stream);
/* Process-wide A/B switch of the kernel for K <= 256 (one contraction segment, the plain and the gate form): on != 0
 * (the default) they run the row-block-stationary kernel, 0 the tile kernel of every other form; bit-identical results.
 * Returns the previous value; a negative argument only queries. */
int amk_gemm_x6_short_k(int on);
int amk_gemm_x6_gate_rows(int H);
int amk_gemm_x6_nt_swiglu(const float* A, int64_t lda, const void* gate_planes, const float* bias, float* gate,
                          int64_t ldg, float* ab, int64_t ldab, int M, int H, int K, void* stream);
int amk_gemm_x6_nt_swiglu_bwd(const float* dY, int64_t ldy, const void* w3t_planes, const float* ab, int64_t ldab,
                              float* d_ab, int64_t ldd, int M, int H, int K, void* stream);
int amk_gemm_x6_split_table(const float* flat, int64_t flat_elems, const void* table, int n_entries, int64_t n_blocks,
                            void* planes, int64_t planes_elems, void* stream);
/* The weight (and bias) gradient of the same layers on split-bf16 products (csrc/gemm_x6_tn.hip):
 * c[n, k] = sum_m y[m, n] x[m, k] with y (M, N) and x (M, K) f32 row-major (the contraction index is the row), both split
 * into three bf16 parts inside the kernel, six products per 16 rows accumulated in f32; dbias (N, optional) = the column
 * sums of y in f32.  split > 0 (a multiple of 128, < N): rows [0, split) of the result come from y and go to c, rows
 * [split, N) come from y2 (M, N - split) and go to c2, against the same x (dWq | dWkv in one launch); split = 0: y2, c2
 * unused.  The M rows are summed in chunks, in a fixed order (bitwise reproducible); workspace: the _ws_bytes() call
 * below (0 when one chunk suffices), 16-byte aligned.  AMK_EUNSUPPORTED: N, K or a leading dimension not a multiple of 4, a
 * pointer off 16-byte alignment, an operand of 2 GiB or more, an output or one chunk's operand rows of 1 GiB or more. */
int64_t amk_gemm_x6_tn_ws_bytes(int64_t M, int N, int K);
int amk_gemm_x6_tn(const float* y, int64_t ldy, const float* y2, int64_t ldy2, int split, const float* x, int64_t ldx,
                   float* c, int64_t ldc, float* c2, int64_t ldc2, float* dbias, int64_t M, int N, int K,
                   void* workspace, int64_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Dense exact-f32 GEMMs with the surrounding element-wise passes folded in.
 * Replaces, around the attention core and in the FFN of the ViT-VQGAN blocks, nn.Linear forward / backward
 * (models/softmax_attention.py:30-42,80; models/vitvqgan.py:20-34) together with nn.LayerNorm applied to its
 * input (models/vitvqgan.py:44-48), the residual add behind it (:50-61), the SwiGLU gate between w12 and w3 and
 * the bias gradients.  All operands f32 row-major; products on v_mfma_f32_32x32x2_f32 (exact f32).
 *
 *   op AMK_GEMM_NT   C[m, n] = sum_k A'[m, k] W[n, k] (+ bias[n]) (+ resid[m, n])        F.linear(A', W, bias)
 *        A (m x k, lda), W (n x k, ldw), C (m x n, ldc).  A' = ((A - ln_mean[m]) * ln_rstd[m]) * ln_gamma[k] +
 *        ln_beta[k] when ln_mean != NULL (LayerNorm applied while the tile is staged), else A.
 *        split > 0: output columns [split, n) use (w2, ldw2, bias2, c2, ldc2) instead -- two projections of the
 *        same input in one launch; split a multiple of 128.
 *        epilogue AMK_EPI_BIAS, AMK_EPI_RESID (adds resid (m x n, ldr); resid may be c itself), or
 *        AMK_EPI_SWIGLU: W is w12 (2n x k), bias (2n) or NULL; gate[m, j] = silu(a) * b with a = column j,
 *        b = column n + j of A' W^T + bias; gate (m x n, ldg) is written, and c (m x 2n, ldc) = (a | b) too
 *        unless c == NULL.
 *   op AMK_GEMM_NN   C[m, n] = sum_k A[m, k] W[k, n]                                     dX = dY W
 *        A (m x k, lda), W (k x n, ldw).  split > 0: contraction indices [split, k) read (a2, lda2) column
 *        k - split and (w2, ldw2) row k - split.
 *        epilogue AMK_EPI_BIAS (bias must be NULL: plain store), or AMK_EPI_SWIGLU_BWD: the product is dGate
 *        (m x n); ab (m x 2n, ldab) is the forward's (a | b); c (m x 2n, ldc) = (dA | dB) =
 *        (dGate * b * silu'(a) | dGate * silu(a)).
 *   op AMK_GEMM_TN   C[n, k] = sum_m Y[m, n] X'[m, k]                                    dW = dY^T X', db = colsum(dY)
 *        a = Y (m x n, lda), w = X (m x k, ldw), c (n x k, ldc); X' = LayerNorm(X) as above when ln_mean != NULL
 *        (ln_gamma / ln_beta indexed by k).  split > 0: output rows [split, n) read Y = (a2, lda2) column
 *        n - split and are written to (c2, ldc2); split a multiple of 128.  dbias (n) != NULL: column sums of Y.
 *        The m rows are cut into chunks; partial tiles go through `workspace` (amk_gemm_f32_ws_bytes(d) bytes,
 *        16-byte aligned) and are summed in chunk order: bitwise reproducible.
 * k and every leading dimension multiples of 4, pointers 16-byte aligned, operand panels below 1 GiB.
 * amk_row_stats: mean and rstd = 1 / sqrt(var + eps) (biased variance, two-pass) of every row of x (M x D),
 * the statistics nn.LayerNorm uses; D a multiple of 4, at most 4096.
 * -------------------------------------------------------------------------- */
enum { AMK_GEMM_NT = 0, AMK_GEMM_NN = 1, AMK_GEMM_TN = 2 };
enum { AMK_EPI_BIAS = 0, AMK_EPI_RESID = 1, AMK_EPI_SWIGLU = 2, AMK_EPI_SWIGLU_BWD = 3 };
typedef struct amk_gemm_desc {
  int32_t op, epilogue;
  int64_t m;
  int32_t n, k, split, reserved;
  const float *a, *a2, *w, *w2;
  float *c, *c2;
  int64_t lda, lda2, ldw, ldw2, ldc, ldc2;
  const float *bias, *bias2, *resid;
  int64_t ldr;
  const float *ln_mean, *ln_rstd, *ln_gamma, *ln_beta;
  const float* ab;
  int64_t ldab;
  float* gate;
  int64_t ldg;
  float* dbias;
} amk_gemm_desc;
int64_t amk_gemm_f32_ws_bytes(const amk_gemm_desc* d);
int amk_gemm_f32(const amk_gemm_desc* d, void* workspace, int64_t ws_bytes, void* stream);
int amk_row_stats(const float* x, int64_t M, int D, float eps, float* mean, float* rstd, void* stream);

/* --------------------------------------------------------------------------
 * Softmax attention on bf16 tensors (the reference's shipped training precision: cfg/vitvqgan.yaml:73 runs
 * models/softmax_attention.py:62-76 under bf16 autocast -- projections and both einsums in bf16, softmax in f32).
 * q, k, v, o, d_o, dq, dk, dv are bf16 (2-byte elements, strides in ELEMENTS, multiples of 8, 16-byte aligned);
 * contractions on v_mfma_f32_32x32x16_bf16 with f32 accumulation; scores, softmax and stats (B,H,I,2) are f32 as in
 * amk_attn_fwd.  Head dim 64.  key_mask (B, J) 1 = keep and causal_mask (I, J) 1 = masked, bytes, either may be NULL:
 * the masked_fill(-1e9) semantics of amk_attn_fwd (models/softmax_attention.py:65-71; a fully masked row keeps uniform
 * weights), as template variants of the same kernels -- what Muse's padded text prompts (models/muse.py:88-96) and every
 * masked call under the reference's autocast need.
 * Backward: ws = amk_attn_bf16_bwd_ws_floats(B,H,I,J) floats (four row constants per query and per-key-block dq
 * partials, summed in key-block order by a second launch: no atomics, bitwise reproducible).
 * -------------------------------------------------------------------------- */
int amk_attn_bf16_fwd(const void* q, const void* k, const void* v, void* o, float* stats,
                      const uint8_t* key_mask, const uint8_t* causal_mask,
                      int B, int H, int I, int J, int D,
                      int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                      int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                      float scale, void* stream);
int64_t amk_attn_bf16_bwd_ws_floats(int B, int H, int I, int J);
int amk_attn_bf16_bwd(const void* q, const void* k, const void* v, const void* o, const float* stats, const void* d_o,
                      void* dq, void* dk, void* dv, float* ws,
                      const uint8_t* key_mask, const uint8_t* causal_mask,
                      int B, int H, int I, int J, int D,
                      int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                      int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                      int64_t do_sb, int64_t do_st, int64_t do_sh, int64_t dq_sb, int64_t dq_st, int64_t dq_sh,
                      int64_t dk_sb, int64_t dk_st, int64_t dk_sh, int64_t dv_sb, int64_t dv_st, int64_t dv_sh,
                      float scale, void* stream);

/* The same two kernels for head dims 32 and 128 (models/softmax_attention.py:62-76 under bf16 autocast at the head dims
 * a user who changes d_head picks first; csrc/attn_bf16_hd.hip: the head dim is a template argument; 256 keys per
 * backward workgroup at head dim 32, 128 at head dim 128).  Arguments, masks, alignment rules, statistics and error codes as amk_attn_bf16_fwd / _bwd; the
 * workspace size takes the head dim.  D must be 32 or 128: anything else is AMK_EUNSUPPORTED (0 floats from
 * amk_attn_bf16_hd_bwd_ws_floats) -- head dim 64 runs on amk_attn_bf16_fwd / _bwd.  Argument errors are AMK_EINVAL
 * with nothing launched. */
int amk_attn_bf16_hd_fwd(const void* q, const void* k, const void* v, void* o, float* stats,
                         const uint8_t* key_mask, const uint8_t* causal_mask,
                         int B, int H, int I, int J, int D,
                         int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                         int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                         float scale, void* stream);
int64_t amk_attn_bf16_hd_bwd_ws_floats(int B, int H, int I, int J, int D);
int amk_attn_bf16_hd_bwd(const void* q, const void* k, const void* v, const void* o, const float* stats, const void* d_o,
                         void* dq, void* dk, void* dv, float* ws,
                         const uint8_t* key_mask, const uint8_t* causal_mask,
                         int B, int H, int I, int J, int D,
                         int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                         int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                         int64_t do_sb, int64_t do_st, int64_t do_sh, int64_t dq_sb, int64_t dq_st, int64_t dq_sh,
                         int64_t dk_sb, int64_t dk_st, int64_t dk_sh, int64_t dv_sb, int64_t dv_st, int64_t dv_sh,
                         float scale, void* stream);

/* --------------------------------------------------------------------------
 * Element-wise passes of the mixed-precision (bf16 autocast) mode: the ops of amk_swiglu_* / amk_add_layernorm_*
 * (models/vitvqgan.py:20-61) reading and writing bf16 where the neighbouring GEMM is a bf16 GEMM, so that no separate
 * cast pass runs (cfg/vitvqgan.yaml:73: nn.Linear in bf16, LayerNorm in f32).  Arithmetic in f32.
 *   swiglu_bf16   : ab (M, 2H) bf16 -> out (M, H) bf16;  backward: ab, d_out bf16 -> d_ab (M, 2H) bf16
 *   mixed LN fwd  : h = x (+ res): x f32 or bf16 (x_is_bf16), res f32 or NULL; h f32 (may be NULL without res and with
 *                   f32 x), y = LN(h) * gamma + beta written as bf16, mean / rstd f32
 *   mixed LN bwd  : dy bf16 or f32 (dy_is_bf16), h f32 -> dh f32 (+ dh_in), dh_bf16 = the same rounded to bf16 (or NULL);
 *                   dgb_part as amk_add_layernorm_bwd
 * -------------------------------------------------------------------------- */
int amk_swiglu_bf16_fwd(const void* ab, int64_t M, int H, void* out, void* stream);
int amk_swiglu_bf16_bwd(const void* ab, const void* d_out, int64_t M, int H, void* d_ab, void* stream);
int amk_add_layernorm_mixed_fwd(const void* x, int x_is_bf16, const float* res, const float* gamma, const float* beta,
                                int64_t M, int D, float eps, float* h, void* y_bf16, float* mean, float* rstd, void* stream);
int amk_add_layernorm_mixed_bwd(const void* dy, int dy_is_bf16, const float* h, const float* dh_in, const float* gamma,
                                const float* mean, const float* rstd, int64_t M, int D, float* dh, void* dh_bf16,
                                float* dgb_part, void* stream);

/* ----------------------------------------------------------------------------
 * The gate and the LayerNorm of the transformer FFN under bf16 autocast as one row-wise pass each way
 * (models/transformer.py:22-43: Linear(dim, 2 inner) -> gate * gelu(val) -> LayerNorm(inner) -> Linear(inner, dim)).
 *   forward : ab (M, 2H) bf16 = (val | gate) as chunk(2, -1) gives them, row stride ab_stride elements;
 *             g = gelu(val) * gate (exact erf, f32, never rounded to bf16 and never written), two-pass mean / variance
 *             of g, y (M, H) = (g - mean) rstd gamma + beta rounded to bf16 once; mean, rstd (M) f32; gamma, beta (H) f32.
 *   backward: recomputes g and xhat from ab, mean, rstd; dy (M, H) bf16;
 *             dg = rstd (dy gamma - mean_j(dy gamma) - xhat mean_j(dy gamma xhat)),
 *             d_ab (M, 2H) contiguous = (dg gate gelu'(val) | dg gelu(val)) rounded to bf16 once;
 *             dgb_part (amk_geglu_ln_bf16_num_partials(M, H), 2, H) f32: per-workgroup partial sums of dgamma (row 0)
 *             and dbeta (row 1), at most 512 of them; the caller sums axis 0.  No atomics: bitwise reproducible.
 * H a multiple of 8 with 8 <= H <= 4096, else AMK_EUNSUPPORTED.  AMK_EINVAL: a null pointer, M <= 0 or H <= 0,
 * ab_stride not a multiple of 8 or below 2H, ab / dy / y / d_ab / gamma / beta / dgb_part off 16-byte alignment.
 * A refused call launches nothing and writes nothing.
 * -------------------------------------------------------------------------- */
int amk_geglu_ln_bf16_num_partials(int64_t M, int H);
int amk_geglu_ln_bf16_fwd(const void* ab, int64_t ab_stride, int64_t M, int H, const float* gamma, const float* beta,
                          float eps, void* y, float* mean, float* rstd, void* stream);
int amk_geglu_ln_bf16_bwd(const void* ab, int64_t ab_stride, const void* dy, const float* gamma, const float* mean,
                          const float* rstd, int64_t M, int H, void* d_ab, float* dgb_part, void* stream);

/* Weight and bias gradient of nn.Linear in the mixed-precision mode (csrc/gemm_bf16.hip): c[n, k] = sum_m y[m, n] x[m, k]
 * with y (M, N) and x (M, K) in bf16 as the autocast GEMMs leave them, c (N, K) and dbias (N, optional: column sums of y)
 * in f32 as the parameters' gradients are kept.  Replaces the autograd backward of nn.Linear under torch.autocast
 * (reference: models/softmax_attention.py:30-42,80, models/vitvqgan.py:20-34 under cfg/vitvqgan.yaml:73).  N, K, ldy, ldx
 * multiples of 8, ldc of 4; sums in a fixed order (bitwise reproducible).  workspace: amk_gemm_tn_bf16_ws_bytes(). */
int64_t amk_gemm_tn_bf16_ws_bytes(int64_t M, int N, int K);
int amk_gemm_tn_bf16(const void* y, int64_t ldy, const void* x, int64_t ldx, float* c, int64_t ldc, float* dbias,
                     int64_t M, int N, int K, void* workspace, int64_t ws_bytes, void* stream);

/* Forward and input gradient of nn.Linear in the mixed-precision mode (csrc/gemm_bf16.hip), bf16 in and out, f32
 * accumulation, the f32 bias added before the one rounding:
 *   op 0: c (M, N) = a (M, K) w^T + bias, w (N, K) as nn.Linear stores it;   op 1: c (M, N) = a (M, K) w, w (K, N) (dX = dY W)
 *   epi 1 (op 0): the SwiGLU gate of models/vitvqgan.py:20-34 folded in: w = w12 (2 H, K), g (M, H) = silu(a-half) * b-half,
 *   c (M, 2 H) optional (NULL: the pre-activations are not written).
 * N, K and the leading dimensions multiples of 8 (N of 16 with epi 1); pointers 16-byte aligned; bias may be NULL. */
int amk_gemm_bf16(int op, int epi, const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias,
                  void* c, int64_t ldc, void* g, int64_t ldg, int64_t M, int N, int K, void* stream);

/* dab (M, 2 H) = (dA | dB): the backward of the SwiGLU gate applied to dG = dy (M, K) w3 (K, H), with the forward's
 * ab (M, 2 H) = (a | b) -- the input gradient of the FFN's second projection and the gate's backward in one launch
 * (models/vitvqgan.py:20-34, backward).  dG is rounded to bf16 before the gate's arithmetic (f32), exactly as
 * amk_gemm_bf16(op 1) followed by amk_swiglu_bf16_bwd would; H, K and the leading dimensions multiples of 8. */
int amk_gemm_bf16_swiglu_bwd(const void* dy, int64_t lddy, const void* w3, int64_t ldw, const void* ab, int64_t ldab,
                             void* dab, int64_t lddab, int64_t M, int H, int K, void* stream);

/* ----------------------------------------------------------------------------
 * The logits head of the masked-token decode under bf16 autocast (models/muse.py:211-217: two decoder passes, each ending
 * in final_norm + a bias-free Linear, combined as null + s (logits - null); models/maskgit.py:248: the same head, one pass,
 * no guidance).  The Linear has no bias and the guidance is linear, so the combination is taken on the normalised
 * activations and ONE product gives the guided logits:  null + s (cond - null) = W (LN(h_null) + s (LN(h_cond) - LN(h_null))).
 *
 * amk_cfg_layernorm_bf16 (csrc/mixed_bf16.hip): row m of hc and of hn (M, D), each f32 or bf16 (hc_is_bf16 / hn_is_bf16),
 *   is normalised with its own f32 two-pass mean and rstd, y = xhat gamma + beta; the rows are combined in f32 as
 *   u = yn + cfg_scale (yc - yn) and u is rounded to bf16 once (nearest even) into y (M, D).  hn NULL: u = yc, a plain
 *   LayerNorm to bf16; cfg_scale == 1 takes that path too (u = yc exactly).  No atomics, no workspace; row m is bitwise
 *   independent of M.  D a multiple of 4 up to 4096, else AMK_EUNSUPPORTED; AMK_EINVAL: a null hc / gamma / beta / y,
 *   M <= 0 or D <= 0, a pointer off 16-byte alignment.  A refused call launches nothing and writes nothing.
 *
 * amk_gemm_bf16_f32out (csrc/gemm_bf16.hip): c (M, N) f32 = a (M, K) w (N, K)^T (+ f32 bias), bf16 operands, accumulation on
 *   v_mfma_f32_32x32x16_bf16 exactly as amk_gemm_bf16 op 0, the accumulator stored as it is: the logits are never rounded
 *   to bf16.  N, K, lda, ldw multiples of 8, ldc of 4, operand panels below 1 GiB (AMK_EUNSUPPORTED); pointers 16-byte
 *   aligned, leading dimensions no shorter than their rows (AMK_EINVAL); bias may be NULL.
 * -------------------------------------------------------------------------- */
int amk_cfg_layernorm_bf16(const void* hc, int hc_is_bf16, const void* hn, int hn_is_bf16, const float* gamma,
                           const float* beta, float cfg_scale, int64_t M, int D, float eps, void* y_bf16, void* stream);
int amk_gemm_bf16_f32out(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, float* c, int64_t ldc,
                         int64_t M, int N, int K, void* stream);

/* --------------------------------------------------------------------------
 * Training-mode BatchNorm2d + LeakyReLU(slope) of the PatchGAN discriminator (csrc/discr_norm.hip), f32, contiguous
 * NCHW x (N, C, HW); reference: models/utils/discriminator.py:34-35,42-43 (BatchNorm2d followed by LeakyReLU(0.2)).
 * (The bf16 form for the autocast step, amk_bnact_bf16_*, follows below.)
 * Per channel, n = N HW: mu and var are the biased batch statistics, r = (var + eps)^-1/2, xh = (x - mu) r,
 * y = gamma xh + beta, z = y > 0 ? y : slope y, s = dz/dy (1 or slope).  y is recomputed from x, never stored.
 *   fwd     : z; mean, rstd (C) for the backward; running_mean / running_var (C, may be NULL) updated as torch does
 *             (momentum m; the variance term unbiased, var n / (n - 1)).
 *   bwd     : gy = s gz, Sgy = sum gy, Sgyx = sum gy xh;  gx = gamma r (gy - Sgy/n - xh Sgyx/n);
 *             sums (2, C) = (Sgy, Sgyx) for bwd_bwd; dbeta = Sgy and dgamma = Sgyx (C, each may be NULL).
 *   bwd_bwd : the derivative of bwd given ggx and the optional gg_gamma, gg_beta (C, NULL = 0): with A = Sgy/n,
 *             B = Sgyx/n, C = sum ggx/n, D = sum ggx xh/n, E = sum ggx gy/n
 *               g_gz = s [gamma r (ggx - C - xh D) + gg_gamma xh + gg_beta]
 *               g_x  = -gamma r^2 [xh (E - AC - 3BD) + B (ggx - C) + D (gy - A)] + gg_gamma r (gy - A - xh B)
 *               g_gamma = n r (E - AC - BD) (may be NULL); the beta gradient is zero.
 * Any HW; the (N, C, HW) tensors 16-byte aligned; reductions through ordered per-workgroup partials in ws
 * (amk_bnact_ws_floats(N, C, HW) floats), no atomics: bitwise reproducible.  Two launches per entry point.
 * -------------------------------------------------------------------------- */
int64_t amk_bnact_ws_floats(int N, int C, int64_t HW);
int amk_bnact_fwd(const float* x, const float* gamma, const float* beta, int N, int C, int64_t HW, float eps,
                  float momentum, float slope, float* z, float* mean, float* rstd, float* running_mean,
                  float* running_var, float* ws, void* stream);
int amk_bnact_bwd(const float* gz, const float* x, const float* gamma, const float* beta, const float* mean,
                  const float* rstd, int N, int C, int64_t HW, float slope, float* gx, float* sums, float* dgamma,
                  float* dbeta, float* ws, void* stream);
int amk_bnact_bwd_bwd(const float* ggx, const float* gg_gamma, const float* gg_beta, const float* gz, const float* x,
                      const float* gamma, const float* beta, const float* mean, const float* rstd, const float* sums,
                      int N, int C, int64_t HW, float slope, float* g_gz, float* g_x, float* g_gamma, float* ws,
                      void* stream);

/* The same three entry points under bf16 autocast (csrc/discr_norm.hip, the same kernels on bf16 elements): x, z, gz, gx,
 * ggx, g_gz and g_x are bf16 (const void* / void*); gamma, beta, mean, rstd, the running statistics, dgamma, dbeta, sums,
 * gg_gamma, gg_beta, g_gamma and ws f32.  Replaces what models/utils/discriminator.py:34-35 and :42-43 (BatchNorm2d
 * followed by LeakyReLU(0.2, True)) run as under torch.autocast(dtype=bfloat16), the precision cfg/vitvqgan.yaml:73
 * trains in: MIOpen's batch norm on the convolution's bf16 output, ATen's leaky_relu_ and leaky_relu_backward, and for
 * the gradient penalty (trainers/vitgqgan.py:115-131) ATen's composite double backward.  The bf16 values are widened to f32
 * on the load; the statistics (two passes, Chan's merge), y = fmaf(x, scale, shift) recomputed from x in every pass, s
 * taken from that f32 y and every sum are the f32 arithmetic of amk_bnact_*; each bf16 output is rounded once, to nearest
 * even, on the store.  16-byte accesses hold 8 elements: a plane is walked as a scalar head of (8 - base % 8) % 8 elements,
 * an aligned body and a scalar tail of up to 7.  The same refusals and return codes, launches, workspace
 * (amk_bnact_ws_floats) and reproducibility as amk_bnact_*. */
int amk_bnact_bf16_fwd(const void* x, const float* gamma, const float* beta, int N, int C, int64_t HW, float eps,
                       float momentum, float slope, void* z, float* mean, float* rstd, float* running_mean,
                       float* running_var, float* ws, void* stream);
int amk_bnact_bf16_bwd(const void* gz, const void* x, const float* gamma, const float* beta, const float* mean,
                       const float* rstd, int N, int C, int64_t HW, float slope, void* gx, float* sums, float* dgamma,
                       float* dbeta, float* ws, void* stream);
int amk_bnact_bf16_bwd_bwd(const void* ggx, const float* gg_gamma, const float* gg_beta, const void* gz, const void* x,
                           const float* gamma, const float* beta, const float* mean, const float* rstd,
                           const float* sums, int N, int C, int64_t HW, float slope, void* g_gz, void* g_x,
                           float* g_gamma, float* ws, void* stream);

/* --------------------------------------------------------------------------
 * GroupNorm(G, C, eps) + optional Swish of the conv VQGAN (csrc/gn_act.hip), f32, contiguous NCHW x (N, C, HW);
 * replaces the GroupNorm and Swish modules of the reference, models/vqgan.py:11-22.
 * Per sample n and group g (cpg = C / G consecutive channels, one contiguous run of m = cpg HW floats): mu and var are
 * the biased statistics of the run, r = (var + eps)^-1/2, xh = (x - mu) r, y = gamma_c xh + beta_c, z = act(y);
 * act 0 = identity, act 1 = swish y sigma(y).  y and sigma are recomputed from x, never stored.
 *   fwd : z; mean, rstd (N, G) for the backward.
 *   bwd : gy = gz act'(y), swish' = sigma (1 + y (1 - sigma));  dbeta_c = sum_{n,hw} gy, dgamma_c = sum_{n,hw} gy xh (C);
 *         S1 = sum_run gamma_c gy, S2 = sum_run gamma_c gy xh;  gx = r (gamma_c gy - S1/m - xh S2/m).
 * Any HW; x, z, gz and gx 16-byte aligned; G must divide C (else AMK_EUNSUPPORTED, as is a grid beyond 2^31
 * workgroups); act outside {0, 1} is AMK_EINVAL.  Reductions go through ordered per-workgroup partials in ws
 * (amk_gnact_ws_floats(N, C, HW, G) floats), no atomics: bitwise reproducible, and a sample's outputs do not depend
 * on the rest of the batch.  Two launches forward, three backward.
 * -------------------------------------------------------------------------- */
int64_t amk_gnact_ws_floats(int N, int C, int64_t HW, int G);
int amk_gnact_fwd(const float* x, const float* gamma, const float* beta, int N, int C, int64_t HW, int G, float eps,
                  int act, float* z, float* mean, float* rstd, float* ws, void* stream);
int amk_gnact_bwd(const float* gz, const float* x, const float* gamma, const float* beta, const float* mean,
                  const float* rstd, int N, int C, int64_t HW, int G, int act, float* gx, float* dgamma, float* dbeta,
                  float* ws, void* stream);

/* The same pair under bf16 autocast (csrc/gn_act.hip, the same kernels on bf16 elements): x, z, gz and gx are bf16
 * (const void* / void*), gamma, beta, mean, rstd, dgamma and dbeta f32.  Replaces what models/vqgan.py:11-22 runs as under
 * torch.autocast(dtype=bfloat16): the cast of the convolution's bf16 output to f32, the f32 GroupNorm, sigmoid and mul,
 * and the cast back to bf16 at the next convolution's input.  The bf16 values of x and gz are widened to f32 on the load;
 * statistics, y, sigma, swish' and every sum are the f32 arithmetic of amk_gnact_*; z and gx are rounded to bf16 once,
 * to nearest even, on the store.  16-byte accesses hold 8 elements: a plane is walked as a scalar head of up to 7
 * elements, an aligned body and a scalar tail.  The same refusals and return codes, launches and reproducibility as
 * amk_gnact_*; ws holds amk_gnact_bf16_ws_floats(N, C, HW, G) floats. */
int64_t amk_gnact_bf16_ws_floats(int N, int C, int64_t HW, int G);
int amk_gnact_bf16_fwd(const void* x, const float* gamma, const float* beta, int N, int C, int64_t HW, int G, float eps,
                       int act, void* z, float* mean, float* rstd, float* ws, void* stream);
int amk_gnact_bf16_bwd(const void* gz, const void* x, const float* gamma, const float* beta, const float* mean,
                       const float* rstd, int N, int C, int64_t HW, int G, int act, void* gx, float* dgamma, float* dbeta,
                       float* ws, void* stream);

/* --------------------------------------------------------------------------
 * LPIPS distance head on one feature level (csrc/lpips.hip), f32, contiguous NCHW a, b (N, C, HW), w (C); replaces,
 * per level, normalize_tensor on both features, (feats0 - feats1) ** 2, the level's 1x1 NetLinLayer convolution and
 * spatial_average of lpips 0.1.4 (LPIPS(net='vgg', lpips=True, spatial=False)), which the reference's generator loss
 * calls at trainers/vitgqgan.py:173-181.
 * Per sample n and pixel p: na = sqrt(sum_c a_c^2), ah_c = a_c / (na + eps), likewise nb and bh_c; e_c = ah_c - bh_c,
 * d = sum_c w_c e_c^2, t = sum_c w_c e_c ah_c.
 *   fwd : out_n = (1 / HW) sum_p d (N); rows (3, N, HW) for the backward: 1 / (na + eps) -- stored as 0 where
 *         na == 0 --, 1 / (nb + eps), and t (na + eps) / na (0 where na == 0).
 *   bwd : with g (N) the cotangent of out and k = 2 g_n / HW:  ga_c = k (w_c e_c - ah_c t (na + eps) / na) / (na + eps).
 *         A pixel with na == 0 gets ga_c = 0 for every c, where autograd gives NaN (sqrt'(0) * 0): the one deliberate
 *         difference; the in-place ReLU in front of every level discards what arrives at such a pixel.  No gradient
 *         for b or w.  eps is read through the rows.
 * Any C and HW; a, b, ga and rows 16-byte aligned, null pointers and sizes < 1 are AMK_EINVAL; a grid beyond 2^31
 * workgroups is AMK_EUNSUPPORTED; all before any launch.  The per-workgroup sums of d go through ws
 * (amk_lpips_ws_floats(N, C, HW) floats) and are folded per sample in a fixed order, no atomics: out and ga are bitwise
 * reproducible, and a sample's outputs do not depend on the rest of the batch.  Two launches forward, one backward.
 * -------------------------------------------------------------------------- */
int64_t amk_lpips_ws_floats(int N, int C, int64_t HW);
int amk_lpips_fwd(const float* a, const float* b, const float* w, int N, int C, int64_t HW, float eps, float* out,
                  float* rows, float* ws, void* stream);
int amk_lpips_bwd(const float* g, const float* a, const float* b, const float* w, const float* rows, int N, int C,
                  int64_t HW, float eps, float* ga, void* stream);

/* The same head under bf16 autocast (the same kernels on bf16 elements): a, b and ga are bf16 (const void* / void*), w, g,
 * out, rows and ws f32.  Replaces what the chain above runs as on the convolutions' bf16 features.  a and b are widened to
 * f32 on the load, everything between is the f32 arithmetic of amk_lpips_*, ga is rounded to bf16 once, to nearest even,
 * on the store.  The same refusals, launches and reproducibility; ws holds amk_lpips_bf16_ws_floats(N, C, HW) floats. */
int64_t amk_lpips_bf16_ws_floats(int N, int C, int64_t HW);
int amk_lpips_bf16_fwd(const void* a, const void* b, const float* w, int N, int C, int64_t HW, float eps, float* out,
                       float* rows, float* ws, void* stream);
int amk_lpips_bf16_bwd(const float* g, const void* a, const void* b, const float* w, const float* rows, int N, int C,
                       int64_t HW, float eps, void* ga, void* stream);

/* --------------------------------------------------------------------------
 * Masked-token loss head (csrc/ce_head.hip): logits + cross-entropy on the rows that count, f32 on
 * v_mfma_f32_32x32x2_f32.  Replaces decoder.linear(...) followed by F.cross_entropy(logits.transpose(1, 2), tgt,
 * ignore_index=-1) of the reference's train steps (models/muse.py:176, models/maskgit.py:187):
 *   z[m, v] = sum_k x[m, k] w[v, k]                     x (M, K) at row stride ldx, w (V, K) at ldw, no bias
 *   loss    = mean over the rows with target[m] != ignore_index of  logsumexp_v z[m, v] - z[m, target[m]]
 * The logits are never written in the forward and rows with target == ignore_index cost no matrix work: `rows`
 * (int32, M) receives the valid row indices in ascending order (entries past count: -1) and `count` (int32, 1) their
 * number, both on the device and never read on the host, so the call is safe under graph capture.  lse[i], i < count,
 * is the log-sum-exp of row rows[i] (entries past count are not written).  The forward is free of atomics: bitwise
 * reproducible.
 * count == 0: loss is NaN (0 / 0, as torch), dx and dw are zeros, nothing faults.
 * A target that is neither ignore_index nor in [0, V) is never used as an index.  Its row counts as valid (count
 * includes it), makes the loss NaN, and neither receives nor gives a gradient: its dx row is zero and it adds nothing
 * to dw, while d_loss / count still divides by the count that includes it.
 * Backward: d_loss is a DEVICE scalar.  g[i, v] = (exp(z - lse[i]) - [v == target]) d_loss / count is recomputed into
 * ws (compacted rows at stride V rounded up to 128, transient); dx[rows] = g w at row stride lddx, rows that are
 * ignored or out of range written as exact zeros; dw = g^T x[rows] (V, K) at lddw, fully overwritten.  Fixed
 * accumulation orders: bitwise reproducible.  Only the K floats of a row are written in dx / dw (padding untouched).
 * ws: amk_ce_head_fwd_ws_bytes / _bwd_ws_bytes bytes (0 for sizes outside the limits), contents undefined on return.
 * AMK_EINVAL: null pointer, non-positive size, a leading dimension below K, misaligned pointer (x, w, dx, dw, ws: 16
 * bytes; target: 8; the others: 4), workspace too small.  AMK_EUNSUPPORTED: K or a leading dimension not a multiple
 * of 4; M > 2^24, V > 2^22, K > 2^16, or a grid of 2^31 workgroups.  All refusals precede any device work.
 * -------------------------------------------------------------------------- */
int64_t amk_ce_head_fwd_ws_bytes(int64_t M, int V, int K);
int64_t amk_ce_head_bwd_ws_bytes(int64_t M, int V, int K);
int amk_ce_head_fwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const int64_t* target,
                    int64_t ignore_index, int64_t M, int V, int K, float* loss, float* lse, int32_t* rows,
                    int32_t* count, void* ws, int64_t ws_bytes, void* stream);
int amk_ce_head_bwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const int64_t* target,
                    int64_t ignore_index, int64_t M, int V, int K, const float* d_loss, const float* lse,
                    const int32_t* rows, const int32_t* count, float* dx, int64_t lddx, float* dw, int64_t lddw,
                    void* ws, int64_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------
 * The loss head with a bias (csrc/ce_head.hip): z[m, v] = sum_k x[m, k] w[v, k] + bias[v], everything else as
 * amk_ce_head_fwd / _bwd above.  bias (V,) f32 is the first term of each logit's MFMA chain (the accumulator is preloaded
 * with it); nothing at or past bias[V] is read, for any V.  The backward also writes dbias[v] = sum over the compacted
 * rows of g[i, v] for every v < V, f32, in a fixed order without atomics (bitwise reproducible; zeros when no row is
 * valid; a row whose target is out of range gives nothing).  dbias sums the g that dw reads and needs no workspace of
 * its own: the biasless sizes amk_ce_head_fwd_ws_bytes / _bwd_ws_bytes apply.
 * Refusals as above, and AMK_EINVAL for a null bias or dbias or one that is not 16-byte aligned.
 * -------------------------------------------------------------------------- */
int amk_ce_head_bias_fwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias,
                         const int64_t* target, int64_t ignore_index, int64_t M, int V, int K, float* loss, float* lse,
                         int32_t* rows, int32_t* count, void* ws, int64_t ws_bytes, void* stream);
int amk_ce_head_bias_bwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias,
                         const int64_t* target, int64_t ignore_index, int64_t M, int V, int K, const float* d_loss,
                         const float* lse, const int32_t* rows, const int32_t* count, float* dx, int64_t lddx, float* dw,
                         int64_t lddw, float* dbias, void* ws, int64_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------
 * The masked-token loss head under bf16 autocast (csrc/ce_head_bf16.hip): the head above with bf16 operands on
 * v_mfma_f32_32x32x16_bf16.  x (M, K) and w (V, K) are bf16, row-major with unit column stride; products accumulate in
 * f32 and every softmax quantity stays in f32 (running maximum, sum of exp, lse, the target logit, the loss,
 * d_loss / count): the logits are never rounded to bf16 and never written in the forward.  loss and lse are f32.
 * Semantics as above, restated:
 *   - a row is valid when target[m] != ignore_index; `rows` (int32, M: the valid indices ascending, then -1) and
 *     `count` (int32, 1) are built on the device and never read on the host; every grid is sized from M and a row tile
 *     that starts at or past count exits before any load (rows with an ignored target are never read);
 *   - count == 0: loss is NaN, dx and dw are zeros;
 *   - a target outside [0, V) that is not ignore_index makes the loss NaN, takes and gives no gradient, and is still
 *     counted in the divisor of the mean and of d_loss / count;
 *   - the dx rows of ignored and out-of-range targets are written as exact zeros;
 *   - no atomics: forward and backward are bitwise reproducible from run to run.
 * Backward: d_loss is a DEVICE scalar (f32).  g = (exp(z - lse) - [v == target]) d_loss / count is recomputed in f32 and
 * rounded once to bf16 into ws (compacted rows at stride V rounded up to 128, transient: M x that stride bf16);
 * dx[rows] = g w (bf16 at row stride lddx, f32 accumulation over ascending v, one rounding); dw = g^T x[rows] (V, K) F32
 * at lddw (f32 accumulation over ascending compacted row), fully overwritten.  Only the K elements of a row are written
 * in dx / dw (padding untouched).
 * ws: amk_ce_head_bf16_fwd_ws_bytes / _bwd_ws_bytes bytes (0 for sizes outside the limits), contents undefined on return.
 * AMK_EINVAL: null pointer, non-positive size, a leading dimension below K, misaligned pointer (x, w, dx, dw, ws: 16
 * bytes; target: 8; the others: 4), workspace too small.  AMK_EUNSUPPORTED: K or a leading dimension not a multiple
 * of 8; M > 2^24, V > 2^22, K > 2^16, or a grid of 2^31 workgroups.  All refusals precede any device work.
 * -------------------------------------------------------------------------- */
int64_t amk_ce_head_bf16_fwd_ws_bytes(int64_t M, int V, int K);
int64_t amk_ce_head_bf16_bwd_ws_bytes(int64_t M, int V, int K);
int amk_ce_head_bf16_fwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const int64_t* target,
                         int64_t ignore_index, int64_t M, int V, int K, float* loss, float* lse, int32_t* rows,
                         int32_t* count, void* ws, int64_t ws_bytes, void* stream);
int amk_ce_head_bf16_bwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const int64_t* target,
                         int64_t ignore_index, int64_t M, int V, int K, const float* d_loss, const float* lse,
                         const int32_t* rows, const int32_t* count, void* dx, int64_t lddx, float* dw, int64_t lddw,
                         void* ws, int64_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------
 * The bf16 loss head with a bias (csrc/ce_head_bf16.hip): amk_ce_head_bf16_fwd / _bwd with
 * z[m, v] = sum_k x[m, k] w[v, k] + bias[v].  bias (V,) stays F32 -- the master bias is never rounded to bf16 -- and is
 * the first term of each logit's f32 MFMA chain; nothing at or past bias[V] is read.  dbias[v] (f32, v < V) = the sum
 * over the compacted rows of the once-rounded bf16 g that dw reads, accumulated in f32 in a fixed order without atomics;
 * zeros when no row is valid.  No workspace of its own: amk_ce_head_bf16_fwd_ws_bytes / _bwd_ws_bytes apply.
 * Refusals as above, and AMK_EINVAL for a null bias or dbias or one that is not 16-byte aligned.
 * -------------------------------------------------------------------------- */
int amk_ce_head_bias_bf16_fwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias,
                              const int64_t* target, int64_t ignore_index, int64_t M, int V, int K, float* loss, float* lse,
                              int32_t* rows, int32_t* count, void* ws, int64_t ws_bytes, void* stream);
int amk_ce_head_bias_bf16_bwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias,
                              const int64_t* target, int64_t ignore_index, int64_t M, int V, int K, const float* d_loss,
                              const float* lse, const int32_t* rows, const int32_t* count, void* dx, int64_t lddx, float* dw,
                              int64_t lddw, float* dbias, void* ws, int64_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------
 * The routed expert products of MoELayer under bf16 autocast (csrc/moe_bf16.hip): the per-expert nn.Linear layers of
 * models/moe.py:23-38 inside accelerator.autocast() (trainers/vit.py:67), forward, input gradient and weight / bias
 * gradient, on v_mfma_f32_32x32x16_bf16.  They take the offsets (E+1) / perm lists of amk_moe_route and the a_div /
 * g_div / x_div addressing of amk_grouped_gemm_nt / _nn / _wgrad; rows the lists do not name are left untouched, an
 * expert without pairs gets exactly zero dW and dbias.  Operands are bf16, accumulation is f32 and every OUTPUT IS
 * F32 (Y feeds amk_moe_combine / amk_moe_gate_grad unchanged; dW and dbias are parameter gradients).  No atomics, no
 * workspace, nothing allocated or synchronised: bitwise reproducible from run to run and capturable.
 *   nt:    Y[p,:] = A[p / a_div,:] W[e(p)]^T + bias[e(p)]; A bf16 rows of Kd at stride lda, W bf16 (E,N,Kd), bias f32
 *          (E,N) or NULL, Y f32 (P,N).
 *   nn:    Y[p,:] = scale[p] (G[p / a_div,:] W[e(p)]); G bf16 rows of N at stride ldg, scale f32 (P) or NULL (applied
 *          in f32 after the chain), Y f32 (P,Kd).
 *   wgrad: dW[e] = sum_{p in e} scale[p] G[p / g_div,:]^T (x) X[p / x_div,:], dbias[e] = sum scale[p] G[..]; G, X bf16,
 *          scale[p] G rounded once to bf16 where it is staged; dW f32 (E,N,Kd) and dbias f32 (E,N) or NULL, both fully
 *          overwritten.
 * AMK_EINVAL: null pointer, non-positive size, a pointer not 16-byte aligned, a row stride that is not a multiple of 8
 * or is shorter than the row.  AMK_EUNSUPPORTED: N or Kd not a multiple of 8, E > 1024, a buffer of 2 GiB or more, a
 * grid of 2^31 workgroups.  All refusals precede any device work.
 * -------------------------------------------------------------------------- */
int amk_grouped_gemm_nt_bf16(const void* A, int64_t lda, int a_div, const void* W, const float* bias,
                             const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                             float* Y, void* stream);
int amk_grouped_gemm_nn_bf16(const void* G, int64_t ldg, int a_div, const void* W, const float* scale,
                             const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                             float* Y, void* stream);
int amk_grouped_gemm_wgrad_bf16(const void* G, int64_t ldg, int g_div, const void* X, int64_t ldx, int x_div,
                                const float* scale, const int32_t* offsets, const int32_t* perm,
                                int64_t P, int E, int N, int Kd, float* dW, float* dbias, void* stream);

/* --------------------------------------------------------------------------
 * SwitchHeadAttention's experts under bf16 autocast (csrc/moe_bf16.hip): the nn.Linear experts of
 * models/switchhead_attention.py:46,53 inside accelerator.autocast() (trainers/vit.py:67) -- V experts (E, d, dim),
 * output experts (E, dim, d), d <= 64 -- as ops._SharedRowExpertsBF16 / _SummedExpertsBF16 form them (:58-88,115): the
 * three grouped products above in a tile form for a side of at most 64, and the per-expert sums with a bf16 result.
 * The contract is that of the block above: bf16 operands, f32 accumulation, f32 Y / dW, the same offsets / perm lists
 * (amk_moe_route's, or amk_moe_route_distinct's virtual pairs with P = G E and a_div = E) and a_div / g_div / x_div
 * addressing, rows the lists do not name untouched, exactly zero dW for an expert without pairs; no atomics, no
 * workspace, nothing allocated or synchronised, bitwise reproducible and capturable.
 *   nt64:    amk_grouped_gemm_nt_bf16 for N <= 64 (unit: 256 pairs x all outputs, the waves over the pairs).
 *   nn64:    amk_grouped_gemm_nn_bf16 for Kd <= 64.
 *   wgrad64: amk_grouped_gemm_wgrad_bf16 for min(N, Kd) <= 64, without dbias (the experts have none).
 *   amk_moe_expert_sums_bf16: amk_moe_expert_sums with Z (G, E d) in bf16, fully overwritten:
 *            Z[g,e,:] = bf16(sum over the fan pairs p = g fan + j of row g with ids[p] == e of scale[p] A[p / a_div,:]),
 *            the sum in f32 in ascending j exactly as the f32 kernel forms it, rounded once.  A: f32 rows
 *            (a_is_bf16 == 0) or bf16 rows (!= 0) of d at stride lda ELEMENTS; scale f32 (G fan) or NULL.
 * AMK_EINVAL: null pointer, non-positive size, a pointer not 16-byte aligned, a row stride that is not a multiple of 8
 * or is shorter than the row.  AMK_EUNSUPPORTED: the narrow side above 64 (nt64: N, nn64: Kd, wgrad64: both N and
 * Kd), N, Kd or d not a multiple of 8, E > 1024, fan > 4096, a buffer of 2 GiB or more, a grid of 2^31 workgroups.
 * All refusals precede any device work.
 * -------------------------------------------------------------------------- */
int amk_grouped_gemm_nt64_bf16(const void* A, int64_t lda, int a_div, const void* W, const float* bias,
                               const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                               float* Y, void* stream);
int amk_grouped_gemm_nn64_bf16(const void* G, int64_t ldg, int a_div, const void* W, const float* scale,
                               const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                               float* Y, void* stream);
int amk_grouped_gemm_wgrad64_bf16(const void* G, int64_t ldg, int g_div, const void* X, int64_t ldx, int x_div,
                                  const float* scale, const int32_t* offsets, const int32_t* perm,
                                  int64_t P, int E, int N, int Kd, float* dW, void* stream);
int amk_moe_expert_sums_bf16(const void* A, int a_is_bf16, int64_t lda, int a_div, const int64_t* ids, const float* scale,
                             int64_t G, int fan, int E, int d, void* Z, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMK_H_ */
