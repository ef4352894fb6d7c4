// f32 instantiations of the HSTU attention kernels (one TU per dtype: parallel builds), and the f32 switch on the schedule.
#include "attn_launch.cuh"
namespace hstu {
template int launch_attn_fwd<float>(const AttnPlan&, const HstuAttnParams&, hipStream_t);
template int launch_attn_bwd<float>(const AttnPlan&, const HstuAttnBwdParams&, hipStream_t);
}  // namespace hstu
