// What the two loss heads (csrc/ce_head.hip: exact f32; csrc/ce_head_bf16.hip: bf16 operands) share: the tile sizes and
// limits, the vocabulary slices, ce_compact and ce_finalize, the argument checks and the two host drivers.  A head file
// keeps its tile kernels and describes itself to the drivers with a struct H of static members:
//
//   H::T           element type of x, w, dx and the backward workspace G
//   H::MULT        what K and the leading dimensions must be a multiple of: the elements of one 16-byte piece of T
//   H::fwd[b], H::bwd_g[b]                      ce_fwd_kernel<b> / ce_bwd_g_kernel<b>, b = with a bias
//   H::zero_rows, H::bwd_dx, H::bwd_dw, H::bwd_db   the file's other four kernels
//   H::DB_COLS, H::DB_THREADS                   columns and threads of one workgroup of ce_bwd_db
//
// The file header of csrc/ce_head.hip says what each kernel computes.
#pragma once
#include "amk_common.h"

namespace amk_ce_common {

constexpr int TR = 128;      // B-side tile: 32 per wave, the lane's index
constexpr int TA = 128;      // A-side tile: every wave sees all of it (4 MFMA blocks of 32)
constexpr int SCAN = 1024;   // threads of ce_compact / ce_finalize

constexpr int64_t CE_MAX_M = 1ll << 24;   // count stays exact in f32; rows are int32
constexpr int CE_MAX_V = 1 << 22;
constexpr int CE_MAX_K = 1 << 16;

// vocabulary slices of the forward: enough workgroups for the machine when there are few row tiles; whole 128-word
// tiles per slice, no empty slice
static void slices(int64_t M, int V, int* nsplit, int* vper) {
  const int64_t nrt = (M + TR - 1) / TR;
  const int nvt = (V + TA - 1) / TA;
  int64_t want = (512 + nrt - 1) / nrt;
  if (want > 16) want = 16;
  if (want > nvt) want = nvt;
  if (want < 1) want = 1;
  const int per = (int)((nvt + want - 1) / want);
  *vper = per * TA;
  *nsplit = (nvt + per - 1) / per;
}

static int64_t ldg_of(int V) { return ((int64_t)V + TA - 1) / TA * TA; }

static bool ce_a4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
static bool ce_a8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// ce_compact_kernel and ce_finalize_kernel never touch x or w: one copy, in csrc/ce_head.hip, launched through these
// (one workgroup of SCAN threads each)
void ce_compact(hipStream_t st, const int64_t* target, int64_t ignore_index, int M, int32_t* rows, int32_t* count);
void ce_finalize(hipStream_t st, const float* pm, const float* ps, const float* pz, const int64_t* target, const int32_t* rows,
                 const int32_t* count, int V, int nsplit, int vper, float* lse, float* loss);

// the forward workspace is f32 partials in both heads; the backward one is G, elem_bytes per element
static int64_t ce_fwd_ws_bytes(int64_t M, int V, int K) {
  if (M <= 0 || V <= 0 || K <= 0 || M > CE_MAX_M || V > CE_MAX_V) return 0;
  int ns, vper;
  slices(M, V, &ns, &vper);
  return 3 * M * ns * (int64_t)sizeof(float);
}

static int64_t ce_bwd_ws_bytes(int64_t M, int V, int K, int64_t elem_bytes) {
  if (M <= 0 || V <= 0 || K <= 0 || M > CE_MAX_M || V > CE_MAX_V) return 0;
  return M * ldg_of(V) * elem_bytes;
}

static int check_common(const char* who, int mult, int64_t ldx, int64_t ldw, int64_t M, int V, int K) {
  AMK_CHECK_ARG(M > 0 && V > 0 && K > 0, "%s: non-positive size M=%lld V=%d K=%d", who, (long long)M, V, K);
  AMK_CHECK_SUPPORTED(K % mult == 0, "%s: K=%d must be a multiple of %d", who, K, mult);
  AMK_CHECK_SUPPORTED(ldx % mult == 0 && ldw % mult == 0, "%s: ldx=%lld and ldw=%lld must be multiples of %d", who,
                      (long long)ldx, (long long)ldw, mult);
  AMK_CHECK_ARG(ldx >= K && ldw >= K, "%s: a leading dimension is below K", who);
  AMK_CHECK_SUPPORTED(M <= CE_MAX_M && V <= CE_MAX_V && K <= CE_MAX_K,
                      "%s: operand above the limits (M <= 2^24, V <= 2^22, K <= 2^16): M=%lld V=%d K=%d", who, (long long)M, V, K);
  const int64_t nrt = (M + TR - 1) / TR, widest = ldg_of(V) / TA > (K + TA - 1) / TA ? ldg_of(V) / TA : (K + TA - 1) / TA;
  AMK_CHECK_SUPPORTED(nrt * widest < (1ll << 31), "%s: grid too large (M=%lld V=%d K=%d)", who, (long long)M, V, K);
  return AMK_OK;
}

// bias == nullptr: the biasless head (who names the entry point in the messages)
template <class H>
static int fwd_impl(const char* who, const void* x, int64_t ldx, const void* w, int64_t ldw, const int64_t* target,
                    int64_t ignore_index, int64_t M, int V, int K, float* loss, float* lse, int32_t* rows, int32_t* count, void* ws,
                    int64_t ws_bytes, void* stream, const float* bias) {
  using T = typename H::T;
  AMK_CHECK_ARG(x && w && target && loss && lse && rows && count && ws, "%s: null pointer", who);
  const int rc = check_common(who, H::MULT, ldx, ldw, M, V, K);
  if (rc != AMK_OK) return rc;
  AMK_CHECK_ARG(a16(x) && a16(w) && a16(ws) && ce_a8(target) && ce_a4(loss) && ce_a4(lse) && ce_a4(rows) && ce_a4(count),
                "%s: misaligned pointer (x, w, ws: 16 bytes; target: 8; loss, lse, rows, count: 4)", who);
  AMK_CHECK_ARG(ws_bytes >= ce_fwd_ws_bytes(M, V, K), "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes,
                (long long)ce_fwd_ws_bytes(M, V, K));
  int ns, vper;
  slices(M, V, &ns, &vper);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* pm = static_cast<float*>(ws);
  float* ps = pm + M * ns;
  float* pz = ps + M * ns;
  const int64_t nrt = (M + TR - 1) / TR;
  ce_compact(st, target, ignore_index, (int)M, rows, count);
  hipLaunchKernelGGL(H::fwd[bias != nullptr], dim3((unsigned)(nrt * ns)), dim3(256), 0, st, static_cast<const T*>(x), ldx,
                     static_cast<const T*>(w), ldw, target, V, K, ns, vper, rows, count, pm, ps, pz, bias);
  ce_finalize(st, pm, ps, pz, target, rows, count, V, ns, vper, lse, loss);
  AMK_CHECK_LAUNCH(who);
  return AMK_OK;
}

// bias == nullptr: the biasless head, dbias not used
template <class H>
static int bwd_impl(const char* who, const void* x, int64_t ldx, const void* w, int64_t ldw, const int64_t* target,
                    int64_t ignore_index, int64_t M, int V, int K, const float* d_loss, const float* lse, const int32_t* rows,
                    const int32_t* count, void* dx, int64_t lddx, float* dw, int64_t lddw, void* ws, int64_t ws_bytes, void* stream,
                    const float* bias, float* dbias) {
  using T = typename H::T;
  AMK_CHECK_ARG(x && w && target && d_loss && lse && rows && count && dx && dw && ws, "%s: null pointer", who);
  const int rc = check_common(who, H::MULT, ldx, ldw, M, V, K);
  if (rc != AMK_OK) return rc;
  AMK_CHECK_SUPPORTED(lddx % H::MULT == 0 && lddw % H::MULT == 0, "%s: lddx=%lld and lddw=%lld must be multiples of %d", who,
                      (long long)lddx, (long long)lddw, H::MULT);
  AMK_CHECK_ARG(lddx >= K && lddw >= K, "%s: a leading dimension is below K", who);
  AMK_CHECK_ARG(a16(x) && a16(w) && a16(dx) && a16(dw) && a16(ws) && ce_a8(target) && ce_a4(d_loss) && ce_a4(lse) &&
                    ce_a4(rows) && ce_a4(count),
                "%s: misaligned pointer (x, w, dx, dw, ws: 16 bytes; target: 8; d_loss, lse, rows, count: 4)", who);
  const int64_t need = ce_bwd_ws_bytes(M, V, K, sizeof(T));
  AMK_CHECK_ARG(ws_bytes >= need, "%s: workspace of %lld bytes, %lld needed", who, (long long)ws_bytes, (long long)need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const T* xt = static_cast<const T*>(x);
  const T* wt = static_cast<const T*>(w);
  T* dxt = static_cast<T*>(dx);
  T* G = static_cast<T*>(ws);
  const int64_t ldg = ldg_of(V);
  const int64_t nrt = (M + TR - 1) / TR;
  const int nvt = (int)(ldg / TA), nkt = (K + TA - 1) / TA;
  hipLaunchKernelGGL(H::bwd_g[bias != nullptr], dim3((unsigned)(nrt * nvt)), dim3(256), 0, st, xt, ldx, wt, ldw, target, V, K, nvt,
                     d_loss, lse, rows, count, G, ldg, bias);
  hipLaunchKernelGGL(H::zero_rows, dim3((unsigned)((M * (K / H::MULT) + 255) / 256)), dim3(256), 0, st, target, ignore_index, M, V, K,
                     dxt, lddx);
  hipLaunchKernelGGL(H::bwd_dx, dim3((unsigned)(nrt * nkt)), dim3(256), 0, st, G, ldg, wt, ldw, target, V, K, nkt, rows, count, dxt,
                     lddx);
  hipLaunchKernelGGL(H::bwd_dw, dim3((unsigned)(nvt * nkt)), dim3(256), 0, st, G, ldg, xt, ldx, V, K, nkt, rows, count, dw, lddw);
  if (bias)
    hipLaunchKernelGGL(H::bwd_db, dim3((unsigned)(ldg / H::DB_COLS)), dim3(H::DB_THREADS), 0, st, G, ldg, V, count, dbias);
  AMK_CHECK_LAUNCH(who);
  return AMK_OK;
}

}  // namespace amk_ce_common
