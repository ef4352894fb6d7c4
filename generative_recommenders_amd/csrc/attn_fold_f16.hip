// f16 instantiations of the folded backward schedule.
#include "attn_fold.cuh"
namespace hstu {
template int launch_bwd_fold<f16_t>(const AttnPlan&, const HstuAttnBwdParams&, hipStream_t);
}  // namespace hstu
