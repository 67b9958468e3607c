// The launchers of the token step's attention kernels, templates over the storage type T: included by decode_attn_bf16.hip and
// decode_attn_f32.hip, each of which instantiates them -- and with them the kernels of decode_self_attn.hpp and decode_cross_attn.hpp
// -- for its one T.  The three attention kernels stay in ONE unit per storage type: compiled apart, the slot form of the
// self-attention (all 72 instantiations) and the d_model = 128 cross-attention kernels (9) come out with other instruction bytes;
// cut by storage type, all 288 keep theirs (profiles/decode_units.txt).
#pragma once
#include "decode_cross_attn.hpp"
#include "decode_self_attn.hpp"
#include "decode_step.hpp"

namespace mh {
namespace {

// attention kernels that project their own q (/ k / v): see decode_device.hpp.  d_model = 128 KC, KC in 1..8
// (check_decode_shape).
#define MH_SELF_LEAD_ARGS hp.h, hp.ln_w, hp.W, sa.pos, sa.kc, sa.vc, sa.H, hp.d
// f8 != NULL: the F8 instantiation over this layer's rows of the e4m3 shadow cache (bf16 storage only)
// origin != NULL: the IDX instantiation, cached rows read through the beam search's index table (mh_t5_step_indexed); with f8 as well,
// the F8 + IDX one: the shadow rows and their scales through the same table (mh_t5_step_indexed_skv8)
template <typename T, int KC>
int launch_self_qkv(const dec::SelfAttnP& sa, const dec::HeadProjP& hp, int inner, hipStream_t s, const dec::SelfKv8P* f8,
                    const uint8_t* origin = nullptr, const int32_t* slot_pos = nullptr) {
  MH_REQUIRE(hp.ldh == hp.d && hp.ldw == hp.d && inner == sa.H * 64, "decode: dense residual rows / projection weights expected");
  // dec_self_attn_qkv_kernel<.., F8, IDX> over its cache block, in the model's form (dispatch_attn_form)
  auto qkv = [&](auto f8c, auto idx, const auto& cache) {
    dispatch_attn_form(sa.rope, hp.ln_b, [&](auto wh, auto ln) {
      hipLaunchKernelGGL((dec::dec_self_attn_qkv_kernel<T, KC, decltype(wh)::value, decltype(ln)::value, decltype(f8c)::value, decltype(idx)::value>),
                         dim3(sa.B * sa.H), dim3(1024), 0, s, MH_SELF_LEAD_ARGS, sa, hp, cache);
    });
  };
  if (slot_pos) {   // slot_pos != NULL: the SLOT instantiation, every row at its own position (mh_t5_slots_*); with f8 as well, the
                    // F8 + SLOT one: every row over its own shadow row (mh_t5_slots_open_kv8)
    MH_REQUIRE(!origin, "decode: the slot form of the self-attention has no indexed cache");
    auto slot = [&](auto f8c, const auto& cache) {
      dispatch_attn_form(sa.rope, hp.ln_b, [&](auto wh, auto ln) {
        hipLaunchKernelGGL((dec::dec_slot_self_attn_kernel<T, KC, decltype(wh)::value, decltype(ln)::value, decltype(f8c)::value>),
                           dim3(sa.B * sa.H), dim3(1024), 0, s, MH_SELF_LEAD_ARGS, sa, hp, cache);
      });
    };
    if (!f8) {
      slot(std::false_type{}, dec::SelfSlotP{slot_pos});
    } else if constexpr (sizeof(T) == 2) {
      dec::SelfKv8SlotP sl8{};
      sl8.k8 = f8->k8; sl8.v8 = f8->v8; sl8.ks = f8->ks; sl8.vs = f8->vs; sl8.slot_pos = slot_pos;
      slot(std::true_type{}, sl8);
    } else { set_error("decode: the e4m3 self-attention cache needs bf16 storage"); return MH_ERR_ARG; }
  } else if (origin) {   // with f8 as well: the shadow rows and their scales through the table (mh_t5_step_indexed_skv8)
    MH_REQUIRE(sa.tgt_len <= dec::kSelfIdxMaxTgt, "decode: the indexed self-attention stages at most %d table entries (tgt_len %d)",
               dec::kSelfIdxMaxTgt, sa.tgt_len);
    if (!f8) {
      qkv(std::false_type{}, std::true_type{}, dec::SelfIdxP{origin});
    } else if constexpr (sizeof(T) == 2) {
      dec::SelfKv8IdxP ix8{};
      ix8.k8 = f8->k8; ix8.v8 = f8->v8; ix8.ks = f8->ks; ix8.vs = f8->vs; ix8.origin = origin;
      qkv(std::true_type{}, std::true_type{}, ix8);
    } else { set_error("decode: the e4m3 self-attention cache needs bf16 storage"); return MH_ERR_ARG; }
  } else if (f8) {
    if constexpr (sizeof(T) == 2) qkv(std::true_type{}, std::false_type{}, *f8);
    else { set_error("decode: the e4m3 self-attention cache needs bf16 storage"); return MH_ERR_ARG; }
  } else {
    qkv(std::false_type{}, std::false_type{}, dec::NoSelfKv8P{});
  }
  return check_launch("dec_self_attn_qkv_kernel");
}

#define MH_CROSS_LEAD_ARGS hp.h, hp.ln_w, hp.W, ca.k, ca.v, ca.H, ca.L, hp.d, ca.kv_B
template <typename T, int KC>
int launch_cross_q(const dec::CrossAttnP& ca, const dec::HeadProjP& hp, hipStream_t s) {
  MH_REQUIRE(hp.ldh == hp.d && hp.ldw == hp.d, "decode: dense residual rows / projection weights expected");
  // one key in flight per 8-lane group: 64 VGPRs without spills (two 16-wave workgroups per CU); U = 2 measured the
  // same bandwidth.  The Whisper family: biased Wq, scaled scores (over the e4m3 copy the scale folds into the key scale)
  auto cross = [&](auto f8c) {
    dispatch_attn_form(ca.scale != 0.f, hp.ln_b, [&](auto wh, auto ln) {
      hipLaunchKernelGGL((dec::dec_cross_attn_q_kernel<T, KC, 1, decltype(f8c)::value, decltype(wh)::value, decltype(ln)::value>),
                         dim3(ca.B * ca.H), dim3(1024), 0, s, MH_CROSS_LEAD_ARGS, ca, hp);
    });
  };
  if (ca.kscale != nullptr) {   // the e4m3 copy of the cross K/V
    if constexpr (sizeof(T) == 2) cross(std::true_type{});
    else { set_error("decode: the fp8 cross K/V copy needs bf16 storage"); return MH_ERR_ARG; }
  } else {
    cross(std::false_type{});
  }
  return check_launch("dec_cross_attn_q_kernel");
}


// the plain launch functions of a unit (decode_step.hpp: launch_self_attn_* / launch_cross_attn_*) are these at its T
template <typename T>
int self_attn_of(const dec::SelfAttnP& sa, const dec::HeadProjP& hp, int inner, const dec::SelfKv8P* f8, const uint8_t* origin,
                 const int32_t* slot_pos, hipStream_t s) {
  return dispatch_kc(hp.d, [&](auto kc) { return launch_self_qkv<T, decltype(kc)::value>(sa, hp, inner, s, f8, origin, slot_pos); });
}
template <typename T>
int cross_attn_of(const dec::CrossAttnP& ca, const dec::HeadProjP& hp, hipStream_t s) {
  return dispatch_kc(hp.d, [&](auto kc) { return launch_cross_q<T, decltype(kc)::value>(ca, hp, s); });
}

}  // namespace
}  // namespace mh
