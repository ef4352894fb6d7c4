// f32 instantiations of the research-path (relative position / time bias) attention kernels.
#include "attn_launch.cuh"
namespace hstu {
template int launch_fwd_bias<float>(const AttnPlan&, const HstuAttnParams&, hipStream_t);
template int launch_bwd_bias<float>(const AttnPlan&, const HstuAttnBwdParams&, hipStream_t);
}  // namespace hstu
