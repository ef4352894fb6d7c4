// bf16 instantiations of the research-path (relative position / time bias) attention kernels.
#include "attn_launch.cuh"
namespace hstu {
template int launch_fwd_bias<bf16_t>(const AttnPlan&, const HstuAttnParams&, hipStream_t);
template int launch_bwd_bias<bf16_t>(const AttnPlan&, const HstuAttnBwdParams&, hipStream_t);
}  // namespace hstu
