// f16 instantiations of the long-sequence backward (hstu_attn_bwd_long.cuh: dK / dV kernel + dQ kernel).
#include "capi_internal.h"
#include "hstu_attn_bwd_long.cuh"
namespace hstu {
template int launch_bwd_long<f16_t>(const AttnPlan&, const HstuAttnBwdParams&, hipStream_t);
}  // namespace hstu
