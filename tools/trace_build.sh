#!/bin/bash
# Debug build of the attention kernels with the s_memtime trace enabled -> tests/probe/libhstu_trace.so
set -e
cd "$(dirname "$0")/../generative_recommenders_amd/csrc"
mkdir -p build_trace
for f in capi attn_misc attn_bf16 attn_bias_bf16 attn_fold_bf16 attn_solo_bf16 jagged_ops norm_ops ln_linear aux_ops position_ops embedding_grad loss_ops; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -DHSTU_TRACE $HSTU_EXTRA -I. -I../../include -c $f.hip -o build_trace/$f.o &
done
wait
cat > build_trace/stubs.cpp <<'EOS'
#include "../capi_internal.h"
namespace hstu {
// the launchers of the units this build leaves out
#define FWD(NAME) template <typename T> int NAME(const AttnPlan&, const HstuAttnParams&, hipStream_t) { return -2; }
#define BWD(NAME) template <typename T> int NAME(const AttnPlan&, const HstuAttnBwdParams&, hipStream_t) { return -2; }
FWD(launch_attn_fwd) BWD(launch_attn_bwd) FWD(launch_fwd_bias) BWD(launch_bwd_bias) FWD(launch_fwd_solo) BWD(launch_bwd_solo)
FWD(launch_fwd_solo_bias) BWD(launch_bwd_solo_bias) BWD(launch_bwd_fold) BWD(launch_bwd_long)
#define FWD_INST(NAME, T) template int NAME<T>(const AttnPlan&, const HstuAttnParams&, hipStream_t);
#define BWD_INST(NAME, T) template int NAME<T>(const AttnPlan&, const HstuAttnBwdParams&, hipStream_t);
FWD_INST(launch_attn_fwd, f16_t) FWD_INST(launch_attn_fwd, float) BWD_INST(launch_attn_bwd, f16_t) BWD_INST(launch_attn_bwd, float)
FWD_INST(launch_fwd_bias, f16_t) FWD_INST(launch_fwd_bias, float) BWD_INST(launch_bwd_bias, f16_t) BWD_INST(launch_bwd_bias, float)
FWD_INST(launch_fwd_solo, f16_t) BWD_INST(launch_bwd_solo, f16_t) FWD_INST(launch_fwd_solo_bias, f16_t) BWD_INST(launch_bwd_solo_bias, f16_t)
BWD_INST(launch_bwd_fold, f16_t) BWD_INST(launch_bwd_long, f16_t) BWD_INST(launch_bwd_long, bf16_t)
}
EOS
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I. -I../../include -c build_trace/stubs.cpp -o build_trace/stubs.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC build_trace/*.o -o ../../tests/probe/libhstu_trace.so
echo built tests/probe/libhstu_trace.so
