// The token step's attention kernels in bf16 storage: the ONE unit that instantiates dec_self_attn_qkv_kernel, dec_slot_self_attn_kernel
// and dec_cross_attn_q_kernel for T = bf16_t (decode_attn_launch.hpp says why the three share a unit).  The other units reach them
// through launch_self_attn / launch_cross_attn (decode_step.hpp).
#include "decode_attn_launch.hpp"

namespace mh {
int launch_self_attn_bf16(const dec::SelfAttnP& sa, const dec::HeadProjP& hp, int inner, const dec::SelfKv8P* f8, const uint8_t* origin,
                        const int32_t* slot_pos, hipStream_t s) {
  return self_attn_of<bf16_t>(sa, hp, inner, f8, origin, slot_pos, s);
}
int launch_cross_attn_bf16(const dec::CrossAttnP& ca, const dec::HeadProjP& hp, hipStream_t s) { return cross_attn_of<bf16_t>(ca, hp, s); }
#ifdef MH_PHASE_STAMPS
int attn_bf16_phase_stamps(unsigned long long* acc, int reset) { return dec::take_phase_stamps(acc, reset); }
#endif
}  // namespace mh
