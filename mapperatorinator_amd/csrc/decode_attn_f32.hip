// The token step's attention kernels in fp32 storage: the ONE unit that instantiates dec_self_attn_qkv_kernel, dec_slot_self_attn_kernel
// and dec_cross_attn_q_kernel for T = float (decode_attn_launch.hpp says why the three share a unit).  The other units reach them
// through launch_self_attn / launch_cross_attn (decode_step.hpp).
#include "decode_attn_launch.hpp"

namespace mh {
int launch_self_attn_f32(const dec::SelfAttnP& sa, const dec::HeadProjP& hp, int inner, const dec::SelfKv8P* f8, const uint8_t* origin,
                        const int32_t* slot_pos, hipStream_t s) {
  return self_attn_of<float>(sa, hp, inner, f8, origin, slot_pos, s);
}
int launch_cross_attn_f32(const dec::CrossAttnP& ca, const dec::HeadProjP& hp, hipStream_t s) { return cross_attn_of<float>(ca, hp, s); }
#ifdef MH_PHASE_STAMPS
int attn_f32_phase_stamps(unsigned long long* acc, int reset) { return dec::take_phase_stamps(acc, reset); }
#endif
}  // namespace mh
