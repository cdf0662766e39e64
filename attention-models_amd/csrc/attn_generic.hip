// Softmax attention by head dim: the dispatch, and the D = 32 / 128 instantiations of the kernels in
// attn_generic.h.  Head dims 96, 160, 192, 224, 256 are instantiated one per translation unit in
// attn_generic_dNNN.hip; head dim 64 has the backward only, instantiated in attn_bwd.hip.
#include "attn_generic.h"

namespace amk_attn {

AMK_ATTN_GEN_INSTANTIATE(32)
AMK_ATTN_GEN_INSTANTIATE(128)
AMK_ATTN_GEN_BWD_EXTERN(64)
AMK_ATTN_GEN_EXTERN(96)
AMK_ATTN_GEN_EXTERN(160)
AMK_ATTN_GEN_EXTERN(192)
AMK_ATTN_GEN_EXTERN(224)
AMK_ATTN_GEN_EXTERN(256)

// every multiple of 32 up to 256 except 64, which has the tuned forward of attn_fwd.hip and its own one-pass backward
bool attn_gen_supported(int Dh) { return Dh % 32 == 0 && Dh >= 32 && Dh <= 256 && Dh != D; }

void launch_attn_fwd_gen(const FwdParams& p, int Dh, int64_t nwg, hipStream_t st) {
  switch (Dh) {
    case 32: launch_fwd_gen_dh<32>(p, nwg, st); break;
    case 96: launch_fwd_gen_dh<96>(p, nwg, st); break;
    case 128: launch_fwd_gen_dh<128>(p, nwg, st); break;
    case 160: launch_fwd_gen_dh<160>(p, nwg, st); break;
    case 192: launch_fwd_gen_dh<192>(p, nwg, st); break;
    case 224: launch_fwd_gen_dh<224>(p, nwg, st); break;
    default: launch_fwd_gen_dh<256>(p, nwg, st); break;
  }
}

// the DELTA, DKDV and DQ bits of amk_attn_bwd's stages
void launch_attn_bwd_gen(const BwdParams& p, int Dh, int stages, hipStream_t st) {
  switch (Dh) {
    case 32: launch_bwd_gen_dh<32>(p, stages, st); break;
    case 64: launch_bwd_gen_dh<64>(p, stages, st); break;
    case 96: launch_bwd_gen_dh<96>(p, stages, st); break;
    case 128: launch_bwd_gen_dh<128>(p, stages, st); break;
    case 160: launch_bwd_gen_dh<160>(p, stages, st); break;
    case 192: launch_bwd_gen_dh<192>(p, stages, st); break;
    case 224: launch_bwd_gen_dh<224>(p, stages, st); break;
    default: launch_bwd_gen_dh<256>(p, stages, st); break;
  }
}

}  // namespace amk_attn
