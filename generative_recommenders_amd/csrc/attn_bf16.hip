// bf16 instantiations of the HSTU attention kernels (one TU per dtype: parallel builds), and the bf16 switch on the schedule.
#include "attn_launch.cuh"
namespace hstu {
template int launch_attn_fwd<bf16_t>(const AttnPlan&, const HstuAttnParams&, hipStream_t);
template int launch_attn_bwd<bf16_t>(const AttnPlan&, const HstuAttnBwdParams&, hipStream_t);
}  // namespace hstu
#ifdef HSTU_TRACE
// trace builds only (tools/trace_build.sh): the trace pointer lives in this TU, next to the kernels it instruments
extern "C" int hstu_trace_set_fwd(unsigned long long* ptr) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(hstu::g_hstu_trace_fwd), &ptr, sizeof(ptr));
}
#endif
