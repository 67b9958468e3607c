"""The decode mode switches of `generate_kwargs`, read, refused and spelled for their callees in ONE place (a leaf module: it imports
nothing else from the package, so server / modeling / scheduler / t5_engine / beam all import it at top level).

    generate_kwargs       T5Engine.generate, decode    T5Engine.generate_beam        beam.beam_search
    cross_kv_fp8          (the caller's argument)      (the caller's argument)       kv_fp8 = True | None
    self_kv_fp8           self_kv_fp8                  beam_self_kv_fp8              self_kv_fp8
    beam_cache            -                            beam_cache                    cache
    beam_prefill          -                            beam_prefill                  prefill
    beam_sample_kernel    -                            device_draw                   device_draw

A switch at its default is not passed at all (engines written against an earlier signature keep working), except the two cross K/V
columns above.  Adding a switch: a field, its line in `of`, its refusal if it has one, its keyword in the three `*_kwargs` methods."""
from __future__ import annotations

import dataclasses

import torch


def require_bf16_for_cross_kv_fp8(dtype) -> None:
    """`cross_kv_fp8` on a model that does not store bf16: refused on the host, before anything is encoded (the copy is made of
    bf16 rows, and the fp32 cross-attention kernel has no e4m3 form)."""
    if dtype != torch.bfloat16:
        raise ValueError(f"cross_kv_fp8 needs bf16 storage (this model stores {dtype}): the e4m3 copy of the cross-attention K / V "
                         "is made of bf16 rows")


def require_bf16_for_self_kv_fp8(dtype, num_beams: int = 1, beam_cache: str = "copy") -> None:
    """`self_kv_fp8` where it is not built: refused on the host, before anything is encoded.  The shadow cache is made of bf16 rows
    (fp32 storage has no e4m3 self-attention kernel), and the step-wise entries of beam search over the copied cache (`mh_t5_step`,
    `mh_t5_step_fp8`, `mh_t5_reorder_cache`) have no shadow-cache form.  Beams over the indexed cache have one
    (`mh_t5_step_indexed_skv8`) and pass."""
    if dtype != torch.bfloat16:
        raise ValueError(f"self_kv_fp8 needs bf16 storage (this model stores {dtype}): the e4m3 self-attention cache is made of "
                         "bf16 rows")
    if num_beams > 1 and beam_cache != "indexed":
        raise ValueError(f"self_kv_fp8 is not built for beam search over the copied cache (num_beams={num_beams}): mh_t5_step and the "
                         "cache reorder have no e4m3 shadow-cache form; pass beam_cache='indexed', use num_beams=1 or drop the flag")


def check_cache_mode(cache, prefill):
    """`cache` / `prefill` of `beam_search`, else ValueError: the hosts above it refuse with it before they encode anything"""
    if cache not in ("copy", "indexed"):
        raise ValueError(f"beam cache {cache!r}: expected 'copy' or 'indexed'")
    if prefill and cache != "indexed":
        raise ValueError("the batched prompt prefill of the beam search (prefill / beam_prefill) needs cache='indexed'")


@dataclasses.dataclass(frozen=True)
class DecodeModes:
    cross_kv_fp8: bool = False          # the token steps stream an e4m3 copy of the cross-attention K / V
    self_kv_fp8: bool = False           # ... and attend an e4m3 shadow of the self-attention cache
    beam_cache: str = "copy"            # beam search: "indexed" follows the self-attention cache by index instead of copying it
    beam_prefill: bool = False          # ... and prefills the prompt once per chunk
    beam_sample_kernel: bool = False    # beam-sample draws inside the step kernel

    @classmethod
    def of(cls, gk: dict, dtype, num_beams: int = 1, *, beam_switches: bool = True, order=("cross", "cache", "self")):
        """The switches among the generate kwargs `gk` of one call, refused where they are not built (ValueError; `order`: which refusal
        speaks first when several apply).  `dtype`: what the model stores; None where the caller cannot tell (a duck-typed model or engine
        without `.dtype`) -- the two storage refusals are then left to the engine entries, which make them too.  `beam_switches=False`: a call
        that never reaches the beam search does not read `beam_cache` / `beam_prefill`."""
        m = cls(bool(gk.get("cross_kv_fp8", False)), bool(gk.get("self_kv_fp8", False)),
                gk.get("beam_cache", "copy") if beam_switches else "copy", bool(gk.get("beam_prefill", False)) and beam_switches,
                bool(gk.get("beam_sample_kernel", False)))
        for what in order:
            if what == "cross" and m.cross_kv_fp8 and dtype is not None:
                require_bf16_for_cross_kv_fp8(dtype)
            if what == "cache":
                check_cache_mode(m.beam_cache, m.beam_prefill)
            if what == "self" and m.self_kv_fp8 and dtype is not None:
                require_bf16_for_self_kv_fp8(dtype, num_beams, m.beam_cache)
        return m

    def decode_kwargs(self) -> dict:
        """keywords of `T5Engine.generate` / `decode` (beside the cross K/V argument, which each caller makes its own way)"""
        return dict(self_kv_fp8=True) if self.self_kv_fp8 else {}

    def _beam_kwargs(self, cache: str, prefill: str, self_kv_fp8: str) -> dict:
        kw = dict(device_draw=True) if self.beam_sample_kernel else {}
        if self.beam_cache != "copy":
            kw.update({cache: self.beam_cache, prefill: self.beam_prefill})
        return dict(kw, **{self_kv_fp8: True}) if self.self_kv_fp8 else kw

    def generate_beam_kwargs(self) -> dict:
        """keywords of `T5Engine.generate_beam` (beside `cross_kv_fp8`)"""
        return self._beam_kwargs("beam_cache", "beam_prefill", "beam_self_kv_fp8")

    def beam_search_kwargs(self) -> dict:
        """keywords of `beam.beam_search`; `kv_fp8=True` has the search make the e4m3 copy itself (of the doubled rows under guidance)"""
        return dict(self._beam_kwargs("cache", "prefill", "self_kv_fp8"), kv_fp8=True if self.cross_kv_fp8 else None)
