// The decode self-attention with its own q / k / v projections and cache append: two entry kernels over one textual body
// (decode_self_attn_body.hpp), instantiated in decode_attn_bf16.hip / decode_attn_f32.hip (one storage type each) and nowhere else.
#pragma once
#include "decode_device.hpp"

namespace mh {
namespace dec {

// self-attention of one (b, h) with its own q / k / v projections: appends the new key / value row to the caches and
// attends over keys 0 .. pos-1 from the cache plus the new key straight from LDS (merged last)
// F8 (bf16 storage only; mh_t5_generate_skv8): keys 0 .. pos-1 come from the e4m3 shadow cache `f8` with their per-row scales (64-byte
// rows, 8 bytes per lane); the new key / value are attended at storage precision from LDS as ever, written to the bf16 cache as ever
// (256 bytes per workgroup: the bf16 cache stays valid for everything that reads it) and appended to the shadow by waves 1 / 2
// IDX (mh_t5_step_indexed: beam search without cache copies): cached key / value j < pos of decode row b is read from cache row
// origin[b][j]; the new row is still written to cache row b at pos.  The row's table entries are requested with the first round trip
// and staged in LDS, so that the key loop has no dependent global load in front of its K / V loads.  Everything else -- bias, masks,
// window, the order of every sum -- is per decode row b as in the plain form: same bits as a cache whose rows were copied.
// F8 with IDX (mh_t5_step_indexed_skv8): cached key / value j < pos is the e4m3 row of shadow row origin[b][j] with THAT row's scale
// pair; the new row goes to bf16 cache row b and, quantised, to shadow row b at pos -- never to an origin row, so the shadow keeps
// the table's invariant (every (row, position) written once, no entry goes stale).
// SLOT (mh_t5_slots_*: in-flight decode, every row a slot with a window of its own): the position of row b is slot_pos[b], the row's
// own, instead of the chain's *pos; a negative entry is an idle slot, whose workgroups return before they store anything -- so no step
// can write a cache row that an admission is filling (the admission makes the entry non-negative last, and the chain waits for the
// admission's event before the step that first sees it).  Everything else is the plain form of that row at that position: bias row,
// RoPE row, j_first, the key-loop split, the new key merged last, the order of every sum -- the bits of a batch-1 call at *pos =
// slot_pos[b].  The prompt mask is [rows][P] with P the stride of the slot's mask buffer (ones behind the row's own prompt).  No IDX.
// F8 with SLOT (mh_t5_slots_open_kv8): the F8 row of the uniform call at the row's own position -- keys < slot_pos[b] from shadow row b
// with their scales, the new key / value at storage precision, appended by waves 1 / 2 to shadow row b at slot_pos[b]; an idle slot
// returns before the append too.  Every key below the position was written by this window's admission or by its own earlier steps,
// so what an earlier window (or nobody) left in the row is never read.
// The flag is on the kernel's BODY; the two kernels below are its entry points.  dec_self_attn_qkv_kernel keeps its six template
// arguments -- its instantiations are a pinned list (tests/test_beam_self_kv_fp8_cpu.py) with pinned instruction bytes
// (tools/device_code_diff.py) -- and the slot form is dec_slot_self_attn_kernel<T, KC, WH, LN[, F8]>.
template <typename T, int KC, bool WH = false, bool LN = false, bool F8 = false, bool IDX = false>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4, 4)))   // 16 waves = 4 per SIMD: the whole 128-register budget
void dec_self_attn_qkv_kernel(const float* h_, const float* lnw_, const void* W_, const int* pos_,
                                                                 const void* kc_, const void* vc_, int H_, int d_, SelfAttnP p,
                                                                 HeadProjP hp,   // leading scalars: preloaded kernel arguments
                                                                 typename std::conditional<F8, typename std::conditional<IDX, SelfKv8IdxP, SelfKv8P>::type,
                                                                                           typename std::conditional<IDX, SelfIdxP, NoSelfKv8P>::type>::type f8) {
  constexpr bool SLOT = false;
#include "decode_self_attn_body.hpp"
}
// the slot form (SLOT above): the same arguments, the positions of the chain's rows behind them
// (IDX / SLOT are template parameters only so that the body's `if constexpr` branches stay dependent: never given)
template <typename T, int KC, bool WH = false, bool LN = false, bool F8 = false, bool IDX = false, bool SLOT = true>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4, 4)))
void dec_slot_self_attn_kernel(const float* h_, const float* lnw_, const void* W_, const int* pos_, const void* kc_, const void* vc_,
                               int H_, int d_, SelfAttnP p, HeadProjP hp, typename std::conditional<F8, SelfKv8SlotP, SelfSlotP>::type f8) {
  static_assert(SLOT && !IDX, "the slot form");
#include "decode_self_attn_body.hpp"
}

}  // namespace dec
}  // namespace mh
