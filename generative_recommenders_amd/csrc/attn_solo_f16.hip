// f16 instantiations of the short-sequence kernels.
#include "attn_solo.cuh"
namespace hstu {
template int launch_fwd_solo<f16_t>(const AttnPlan&, const HstuAttnParams&, hipStream_t);
template int launch_bwd_solo<f16_t>(const AttnPlan&, const HstuAttnBwdParams&, hipStream_t);
template int launch_fwd_solo_bias<f16_t>(const AttnPlan&, const HstuAttnParams&, hipStream_t);
template int launch_bwd_solo_bias<f16_t>(const AttnPlan&, const HstuAttnBwdParams&, hipStream_t);
}  // namespace hstu
