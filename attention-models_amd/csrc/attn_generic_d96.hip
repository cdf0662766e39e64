// Softmax attention, head dim 96: the kernels of attn_generic.h (dispatch in attn_generic.hip).
#include "attn_generic.h"

namespace amk_attn {
AMK_ATTN_GEN_INSTANTIATE(96)
}  // namespace amk_attn
