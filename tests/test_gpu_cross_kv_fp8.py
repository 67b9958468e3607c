"""-m gpu: the e4m3 copy of the cross-attention K / V (`cross_kv_fp8`) on the Whisper-family decoders (library arch 1 / 2) and under
beam search (mh_t5_step_fp8).

Contract: not a parity mode.  The device must compute what the bf16-contract oracle computes when ITS cross K / V went through the
same quantisation (absmax / 448 per (layer, k|v, row, head), torch.float8_e4m3fn), to the family's bf16 bound plus a margin for
e4m3 rounding ties; every way of sharing K/V rows between decode rows (guidance pairs, beam groups) must read the same bytes and
scales, i.e. be bit-equal to the same rows decoded over repeated K/V."""
import ctypes as C
import functools

import pytest
import torch

from conftest import ts_range

pytestmark = pytest.mark.gpu
GAP_BF16 = 0.25
# e4m3 rounding ties: the device multiplies by 1 / scale where torch divides by the scale, so an element that sits on a rounding
# boundary may land one e4m3 step away from the oracle's.  The T5 test of the mode (tests/test_gpu_t5.py) found +0.1 on the worst
# |dlogit| over its bf16 floor; the same allowance is added to each family's existing bf16 bound (0.2, 0.3 for the LayerNorm family).
E4M3_TIE_MARGIN = 0.1


def gen_kwargs(tgt, **over):
    kw = dict(precision="fp32", do_sample=False, num_beams=1, top_p=1.0, top_k=0, max_length=tgt, cfg_scale=1.0, timeshift_bias=0,
              types_first=False, temperature=1.0, lookback_time=0, lookahead_time=0, context_type="map", pad_token_id=0)
    kw.update(over)
    return kw


def qdq(x):
    """(B, H, L, 64) -> the values the e4m3 copy stands for: one scale per (row, head), absmax / 448"""
    scale = x.abs().amax(dim=(2, 3), keepdim=True) / 448.0
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    return (x / scale).to(torch.float8_e4m3fn).float() * scale


@functools.lru_cache(maxsize=None)
def family(kind, size, frames, tgt):
    """(dims, tokenizer, state dict, bf16 model, plain oracle class + constructor arguments) of one family at one shape"""
    from mapperatorinator_amd import Tokenizer
    from mapperatorinator_amd.modeling import MapperatorinatorHIP
    from mapperatorinator_amd.whisper_engine import VARWHISPER_PRESETS
    from mh_testing import random_varwhisper_state_dict, random_whisper_family_state_dict
    from oracle import varwhisper as ovw
    from oracle import whisper_family as wf
    d = VARWHISPER_PRESETS[size]
    tok = Tokenizer.benchmark_vocab(src_seq_len=frames)
    n_mels = dict(var=128, rope=80, hf=388)[kind]
    if kind == "var":
        sd = random_varwhisper_state_dict(d.d_model, d.n_heads, d.n_enc_layers, d.n_dec_layers, d.d_ff, tok.vocab_size_in,
                                          tok.vocab_size_out, seed=77, head_gain=5.0, gains={"decoder_embedder": 0.5})
        make = lambda cls=ovw.VarWhisperOracle: cls(sd, d.d_model, d.n_heads, d.n_enc_layers, d.n_dec_layers, rounding="bf16")
        base = ovw.VarWhisperOracle
    else:
        sd = random_whisper_family_state_dict(kind, d.d_model, d.n_heads, d.n_enc_layers, d.n_dec_layers, d.d_ff, tok.vocab_size_in,
                                              tok.vocab_size_out, n_mels, src_positions=frames // 2, tgt_positions=tgt, seed=77,
                                              head_gain=5.0, gains={"decoder_embedder": 0.5})
        base = wf.RoPEWhisperOracle if kind == "rope" else wf.HFWhisperOracle
        make = lambda cls=base: cls(sd, d.d_model, d.n_heads, d.n_enc_layers, d.n_dec_layers, rounding="bf16", n_mels=n_mels)
    model = MapperatorinatorHIP(sd, d, vocab_size_in=tok.vocab_size_in, vocab_size_out=tok.vocab_size_out, n_mels=n_mels,
                                src_seq_len=frames, tgt_seq_len=tgt, dtype=torch.bfloat16, device="cuda", f_min=0 if kind == "hf" else 20)

    class Quantised(base):                     # the family's oracle over cross K / V quantised and dequantised as the device does it
        def cross_kv(self, enc):
            return [(qdq(k), qdq(v)) for k, v in super().cross_kv(enc)]
    return d, tok, model, make, Quantised


def oracle_encode(kind, o, audio):
    return o.encoder(o.frontend(o.log_mel(audio))) if kind == "hf" else o.encode_audio(audio)


@pytest.mark.parametrize("size,B,frames,tgt", [("test", 5, 514, 40), ("small", 2, 512, 32)])
@pytest.mark.parametrize("kind", ["var", "rope", "hf"])
def test_teacher_forced_vs_the_oracle_with_quantised_kv(kind, size, B, frames, tgt):
    """1-token prompt (every position is a token step), teacher-forced on the quantised-K/V oracle's own free run.  test: 514 frames =
    257 keys, two full 128-key passes of the 16 waves plus a one-key tail; small: d = 768, the KC = 6 instantiation of the releases.
    Gate as for the family's bf16 test: no real mismatch above the 0.25 gap, near-tie flips <= 5 % of the steps, worst |dlogit| below
    the family's bf16 bound + E4M3_TIE_MARGIN.  The plain bf16 run against the plain oracle on the same ids is measured beside it
    (what the margin is a margin over), and the mode must be on: logits differ from the bf16-K/V run of the same kernels."""
    from mapperatorinator_amd.server import build_sampling
    from mh_testing import synthetic_audio_varied
    d, tok, model, make, Quantised = family(kind, size, frames, tgt)
    audio = synthetic_audio_varied(B, (frames - 1) * 128, seed=3)
    prompt = torch.tensor([[1]] * B)
    ts0, ts1 = ts_range(tok)
    o, oq = make(), make(Quantised)
    enc_o = oracle_encode(kind, o, audio)
    args = (enc_o, prompt, None, [tok.eos_id], tgt, ts0, ts1, [tok.sos_id])
    free = oq.generate(*args)
    forced = torch.zeros((B, tgt), dtype=torch.long)
    forced[:, :free.shape[1]] = free
    want, scores_q = oq.generate(*args, forced=forced, return_logits=True)
    _, scores_p = o.generate(*args, forced=forced, return_logits=True)
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    out8 = model.engine.generate(audio, prompt, None, [tok.eos_id], sp, forced=forced, dump_logits=True, cross_kv_fp8=True)
    sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
    out16 = model.engine.generate(audio, prompt, None, [tok.eos_id], sp, forced=forced, dump_logits=True)
    got, lg8, lg16 = out8["tokens"], out8["logits"].cpu(), out16["logits"].cpu()
    n_cmp = n_bad = n_tie = n_close = 0
    worst8 = worst16 = cost_worst = 0.0
    cost_sum, cost_n, same_top1 = 0.0, 0, 0
    for i, (sq, s16) in enumerate(zip(scores_q, scores_p)):
        col = 1 + i
        top2 = sq.topk(2, dim=-1).values
        gap = top2[:, 0] - top2[:, 1]
        fin = torch.isfinite(sq)
        assert torch.equal(fin, torch.isfinite(lg8[col]))
        worst8 = max(worst8, (lg8[col][fin] - sq[fin]).abs().max().item())
        worst16 = max(worst16, (lg16[col][fin] - s16[fin]).abs().max().item())
        dm = (lg8[col][fin] - lg16[col][fin]).abs()
        cost_worst, cost_sum, cost_n = max(cost_worst, dm.max().item()), cost_sum + dm.sum().item(), cost_n + dm.numel()
        same_top1 += int((lg8[col].argmax(-1) == lg16[col].argmax(-1)).sum())
        for b in range(B):
            n_cmp += 1
            n_close += int(gap[b] <= GAP_BF16)
            if got[b, col] != want[b, col]:
                if gap[b] > GAP_BF16:
                    n_bad += 1
                else:
                    n_tie += 1
    base = 0.3 if kind == "hf" else 0.2
    print(f"{kind}whisper-{size} e4m3 cross K/V teacher-forced: {n_cmp} steps ({n_close} inside the {GAP_BF16} gap), {n_tie} near-tie flips, "
          f"{n_bad} real mismatches, worst |dlogit| {worst8:.3f} vs the quantised-K/V oracle; plain bf16 run vs the plain oracle on the same "
          f"ids {worst16:.3f} (difference {worst8 - worst16:+.3f}, allowance {E4M3_TIE_MARGIN} over the family's {base}); cost of the mode vs the bf16-K/V run: mean "
          f"{cost_sum / cost_n:.4f} worst {cost_worst:.3f}, same top-1 on {same_top1 / n_cmp:.3f} of the steps")
    # measured (MI355X), worst |dlogit| of the e4m3 run vs the quantised-K/V oracle / of the bf16 run vs the plain oracle on the same ids
    # (difference = the margin used), near-tie flips:
    #   var  test 0.105 / 0.075 (+0.030), 0 of 195      var  small 0.083 / 0.061 (+0.022), 1 of 62
    #   rope test 0.114 / 0.084 (+0.030), 0 of 195      rope small 0.083 / 0.071 (+0.012), 0 of 62
    #   hf   test 0.315 / 0.259 (+0.056), 5 of 195      hf   small 0.387 / 0.193 (+0.194), 0 of 62
    # The rotary families stay inside T5's +0.1.  hf small goes beyond it relative to its own bf16 run -- not by ties alone: the device's
    # and the oracle's K / V differ by bf16 roundings of the encoder, and an element whose two values straddle an e4m3 boundary lands a
    # whole e4m3 step apart (the LayerNorm family's logits are the most sensitive: the mode itself moves them by up to 0.8) -- and is
    # still below the bound, which stays the family's bf16 bound + T5's margin and is not fitted to these figures.
    assert cost_worst > 0, "the mode is not on: the logits equal the bf16-K/V run's"
    assert n_bad == 0 and n_tie <= 0.05 * n_cmp
    assert worst8 < base + E4M3_TIE_MARGIN


def _device_kv(eng, audio):
    eng._enter()
    with eng.on_stream():
        kv = eng.cross_kv(eng.encode_mel(eng.mel(audio.to(eng.device, torch.float32))))
    eng._leave()
    eng.synchronize()
    return kv


def test_guidance_pairs_read_the_bytes_and_scales_of_their_kv_row():
    """kv_B > 0: under guidance decode rows b and b + G share K/V row b.  rope `test` shape, cfg_scale = 2, teacher-forced: the guided
    scores must equal, bit for bit, uncond + (cond - uncond) * scale formed (in the kernel's operation order, no fused multiply-add)
    from the raw logits of the same [negative | prompt] rows decoded WITHOUT guidance over the K/V rows repeated and then quantised:
    same bytes, same scales, and decode is batch-invariant."""
    from mapperatorinator_amd.server import build_sampling
    from mh_testing import synthetic_audio_varied
    B, frames, tgt = 5, 514, 40
    d, tok, model, _, _ = family("rope", "test", frames, tgt)
    eng = model.engine
    ts0, ts1 = ts_range(tok)
    neg_id = ts1 + 3                                        # not a TIME_SHIFT id: both halves keep the same monotonic mask
    assert not (ts0 <= neg_id < ts1) and neg_id < tok.vocab_size_out and neg_id != tok.sos_id
    audio = synthetic_audio_varied(B, (frames - 1) * 128, seed=3)
    g = torch.Generator().manual_seed(9)
    forced = torch.randint(ts1, tok.vocab_size_out, (B, tgt), generator=g)
    forced[:, 1::3] = torch.randint(ts0, ts1, forced[:, 1::3].shape, generator=g)     # time shifts too: the mask moves
    forced[:, 0] = tok.sos_id
    prompt2 = torch.cat([torch.full((B, 1), neg_id), forced[:, :1]], 0).to(eng.device, torch.int32).contiguous()
    forced2 = torch.cat([forced, forced], 0).to(eng.device, torch.int32).contiguous()
    eos_table = torch.zeros(tok.vocab_size_out, dtype=torch.uint8, device=eng.device)
    kv = _device_kv(eng, audio)
    eng._enter()
    with eng.on_stream():
        kv2 = torch.cat([kv, kv], 2).contiguous()
        sp, _ = build_sampling(tok, gen_kwargs(tgt, cfg_scale=2.0), tgt)
        kv8, kv8_2 = eng.cross_kv_fp8(kv), eng.cross_kv_fp8(kv2)
        _, _, guided = eng.decode(kv, prompt2, None, eos_table, sp, forced2, True, kv_fp8=kv8)
        sp, _ = build_sampling(tok, gen_kwargs(tgt), tgt)
        _, _, plain = eng.decode(kv2, prompt2, None, eos_table, sp, forced2, True, kv_fp8=kv8_2)
        sp, _ = build_sampling(tok, gen_kwargs(tgt, cfg_scale=2.0), tgt)
        _, _, guided16 = eng.decode(kv, prompt2, None, eos_table, sp, forced2, True)
    eng._leave()
    eng.synchronize()
    guided, plain, guided16 = guided[1:].cpu(), plain[1:].cpu(), guided16[1:].cpu()
    assert guided.shape == (tgt - 1, B, tok.vocab_size_out) and plain.shape == (tgt - 1, 2 * B, tok.vocab_size_out)
    uncond, cond = plain[:, B:], plain[:, :B]               # HF's processor on the reference's row order: first half = "cond"
    fin = torch.isfinite(guided)
    assert torch.equal(fin, torch.isfinite(uncond)) and torch.equal(fin, torch.isfinite(cond)) and fin.any() and not fin.all()
    want = uncond + (cond - uncond) * 2.0
    assert torch.equal(guided[fin], want[fin]), (guided[fin] - want[fin]).abs().max()
    assert not torch.equal(guided[fin], guided16[fin])      # ... and the copy was what the guided run read


def test_beam_groups_read_the_bytes_and_scales_of_their_kv_row():
    """kv_B < 0 at the step level: G = 2 chunks x 3 beams on the var `test` shape, 6 positions, every beam of a chunk fed the same
    ids.  mh_t5_step_fp8 with kv_group = 3 must be bit-equal to kv_group = 1 over the copy of the repeat_interleave(3)-ed K/V, the
    rows of a chunk bit-equal to each other, and the logits must differ from mh_t5_step's (the copy was read)."""
    from mapperatorinator_amd import _lib
    from mh_testing import synthetic_audio_varied
    G, nb, n_pos, frames, tgt = 2, 3, 6, 514, 40
    d, tok, model, _, _ = family("var", "test", frames, tgt)
    eng, lib = model.engine, _lib.load()
    p, R, V = eng.packed, G * nb, tok.vocab_size_out
    kv = _device_kv(eng, synthetic_audio_varied(G, (frames - 1) * 128, seed=3))
    ids = torch.randint(3, V, (n_pos, G), generator=torch.Generator().manual_seed(4)).repeat_interleave(nb, 1)
    ids = ids.to(eng.device, torch.int32).contiguous()
    ws_bytes = int(lib.mh_t5_decode_workspace_bytes(C.byref(p.cfg), R))

    def run(kv_rows, group, fp8):
        eng._enter()
        with eng.on_stream():
            ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=eng.device)
            kv8 = eng.cross_kv_fp8(kv_rows) if fp8 else None
            out = torch.empty((n_pos, R, V), dtype=torch.float32, device=eng.device)
            for pos in range(n_pos):
                if fp8:
                    rc = lib.mh_t5_step_fp8(C.byref(p.cfg), C.byref(p.w), kv_rows.data_ptr(), kv8.data_ptr(), R, group, ids[pos].data_ptr(),
                                            pos, None, 1, out[pos].data_ptr(), ws.data_ptr(), ws.numel(), eng._s())
                else:
                    rc = lib.mh_t5_step(C.byref(p.cfg), C.byref(p.w), kv_rows.data_ptr(), R, group, ids[pos].data_ptr(), pos, None, 1,
                                        out[pos].data_ptr(), ws.data_ptr(), ws.numel(), eng._s())
                _lib.check(rc, "mh_t5_step_fp8" if fp8 else "mh_t5_step")
        eng._leave()
        eng.synchronize()
        return out.cpu()
    grouped = run(kv, nb, True)
    repeated = run(kv.repeat_interleave(nb, dim=2).contiguous(), 1, True)
    bf16 = run(kv, nb, False)
    assert torch.isfinite(grouped).all()
    assert torch.equal(grouped, repeated)
    per_chunk = grouped.view(n_pos, G, nb, V)
    assert torch.equal(per_chunk, per_chunk[:, :, :1].expand_as(per_chunk))
    assert not torch.equal(per_chunk[:, 0, 0], per_chunk[:, 1, 0])          # (the chunks do differ)
    diff = (grouped - bf16).abs().max().item()
    print(f"mh_t5_step_fp8 vs mh_t5_step, {G} x {nb} rows, {n_pos} positions: max |dlogit| {diff:.4f}")
    assert diff > 0


@pytest.mark.parametrize("kind,guided", [("hf", False), ("rope", True)])
def test_beam_search_end_to_end_kernel_and_torch_bookkeeping_agree(monkeypatch, kind, guided):
    """`model_generate(num_beams=2, cross_kv_fp8=True)`: the LayerNorm instantiation (hf) and kv_B < 0 together, then guidance under
    beams (rope: the copy is made of the doubled rows).  The one-kernel beam step and the torch-op bookkeeping consume the same step
    logits and must return the same ids; the search must have read the copy (one call of mh_t5_step_fp8 per step, none of mh_t5_step)."""
    from mapperatorinator_amd import _lib
    from mapperatorinator_amd.server import model_generate
    from mh_testing import synthetic_audio_varied
    B, frames, tgt = 2, 514, 40
    d, tok, model, _, _ = family(kind, "test", frames, tgt)
    audio = synthetic_audio_varied(B, (frames - 1) * 128, seed=3)
    prompt = torch.tensor([[1, 40], [0, 1]])
    mk = dict(inputs=audio, decoder_input_ids=prompt, decoder_attention_mask=prompt.ne(0))
    gk = gen_kwargs(tgt, num_beams=2, cross_kv_fp8=True)
    if guided:
        neg = torch.tensor([[1, 9], [0, 1]])
        mk.update(negative_prompt=neg, negative_prompt_attention_mask=neg.ne(0))
        gk["cfg_scale"] = 2.0
    lib = _lib.load()
    calls = dict(fp8=0, bf16=0)
    real8, real16 = lib.mh_t5_step_fp8, lib.mh_t5_step

    def counted(name, fn):
        def f(*a):
            calls[name] += 1
            return fn(*a)
        return f
    monkeypatch.setattr(lib, "mh_t5_step_fp8", counted("fp8", real8))
    monkeypatch.setattr(lib, "mh_t5_step", counted("bf16", real16))
    ids_k, _ = model_generate(model, tok, mk, dict(gk, beam_use_kernel=True))
    n_kernel = dict(calls)
    ids_t, _ = model_generate(model, tok, mk, dict(gk, beam_use_kernel=False))
    ids_16, _ = model_generate(model, tok, mk, dict(gk, cross_kv_fp8=False))
    assert n_kernel["fp8"] >= ids_k.shape[1] - 1 and n_kernel["bf16"] == 0
    assert calls["fp8"] == 2 * n_kernel["fp8"] and calls["bf16"] > 0
    assert ids_k.shape[0] == B and ids_k.shape[1] > prompt.shape[1]
    assert torch.equal(ids_k, ids_t), (ids_k.tolist(), ids_t.tolist())
    print(f"{kind} beams{' + guidance' if guided else ''} over the e4m3 copy: {ids_k.shape[1] - prompt.shape[1]} new columns, "
          f"{int((ids_k[:, :ids_16.shape[1]] != ids_16[:, :ids_k.shape[1]]).sum())} ids differ from the bf16-K/V search")


@pytest.mark.parametrize("nb", [1, 2])
def test_scheduler_equals_the_windows_decoded_one_by_one(nb):
    """One three-window song at `test` dims through SequentialWindowScheduler with cross_kv_fp8: every window must come out as
    engine.generate / generate_beam return it for that window alone (each prompt carries ids of the window before)."""
    from mapperatorinator_amd.scheduler import SequentialWindowScheduler, SongJob
    from mapperatorinator_amd.server import build_sampling
    from mh_testing import synthetic_audio_varied
    frames, tgt, n = 514, 40, 3
    d, tok, model, _, _ = family("var", "test", frames, tgt)
    eng = model.engine
    song = synthetic_audio_varied(n, (frames - 1) * 128, seed=8)
    gk = gen_kwargs(tgt, num_beams=nb, cross_kv_fp8=True)

    def prompt_from(prev):
        carry = [] if prev is None else [t for t in prev.tolist() if t > 2][-3:]
        return torch.tensor([[tok.sos_id] + carry])

    def cut(row, P, eos):
        hit = torch.isin(row[P:], torch.tensor(sorted(eos))).nonzero()
        return row[:P + int(hit[0]) + 1] if hit.numel() else row
    want, prev = [], None
    for w in range(n):
        prompt = prompt_from(prev)
        sp, eos = build_sampling(tok, dict(gk, conditional_temperature_per_row=True), tgt)
        if nb == 1:
            out = eng.generate(song[w:w + 1], prompt, None, eos, sp, cross_kv_fp8=True)
        else:
            out = eng.generate_beam(song[w:w + 1], prompt, None, eos, sp, nb, cross_kv_fp8=True)
        row = cut(out["tokens"][0], prompt.shape[1], eos)
        prev = row[prompt.shape[1]:]
        want.append(row)
    got, state = [None] * n, [None]

    def on_result(w, row, st):
        got[w] = row
        state[0] = row[prompt_from(state[0]).shape[1]:]
    job = SongJob(frames=song, prompt_fn=lambda w: dict(decoder_input_ids=prompt_from(state[0])), on_result=on_result, generate_kwargs=gk)
    stats = SequentialWindowScheduler(model, tok, encode_batch=4, decode_batch=8).run([job])
    assert stats["windows"] == n
    for w in range(n):
        assert got[w].shape == want[w].shape and torch.equal(got[w], want[w]), (w, got[w].tolist(), want[w].tolist())
    assert len(want[0]) > 2


@pytest.mark.parametrize("L", [257, 2048])
def test_quantiser_at_a_ragged_and_at_the_longest_released_key_count(L):
    """mh_t5_quantize_cross_kv takes any src_len: L = 257 (no multiple of 8 keys x 16 waves, nor of its own 256-thread stride) and
    L = 2048 (RoPEWhisper's 4096 frames).  Scales are absmax / 448 bit for bit; a byte may differ from torch's x / scale rounding only
    where the device's x * (1 / scale) crosses a rounding boundary: by one e4m3 step, on a tiny fraction of the elements."""
    from mapperatorinator_amd import _lib
    d, tok, model, _, _ = family("var", "test", 514, 40)
    eng, lib = model.engine, _lib.load()
    cfg = type(eng.packed.cfg).from_buffer_copy(eng.packed.cfg)
    cfg.src_len, cfg.in_frames = L, 2 * L                    # (the Whisper family's config check: src_len = the conv-strided frames)
    nl, H, B = cfg.n_dec_layers, cfg.n_heads, 3
    g = torch.Generator().manual_seed(L)
    kv = (torch.randn(nl, 2, B, H, L, 64, generator=g) * torch.rand(nl, 2, B, H, 1, 1, generator=g) * 4).to(torch.bfloat16)
    kv[0, 1, 1, 0] = 0                                       # an all-zero slab: scale 1, bytes 0
    n = int(lib.mh_t5_cross_kv_fp8_bytes(C.byref(cfg), B))
    data = kv.numel()
    assert n == (data + 255) // 256 * 256 + (nl * 2 * B * H * 4 + 255) // 256 * 256
    out = torch.full((n,), 0xAA, dtype=torch.uint8, device=eng.device)
    _lib.check(lib.mh_t5_quantize_cross_kv(C.byref(cfg), kv.to(eng.device).data_ptr(), B, out.data_ptr(), None), "mh_t5_quantize_cross_kv")
    torch.cuda.synchronize()
    out = out.cpu()
    got = out[:data].view(torch.float8_e4m3fn).float().view(kv.shape)
    scales = out[(data + 255) // 256 * 256:][:nl * 2 * B * H * 4].view(torch.float32).view(nl, 2, B, H, 1, 1)
    x = kv.float()
    want_scale = x.abs().amax(dim=(4, 5), keepdim=True) / 448.0
    want_scale = torch.where(want_scale > 0, want_scale, torch.ones_like(want_scale))
    assert torch.equal(scales, want_scale)
    want = (x / want_scale).to(torch.float8_e4m3fn).float()
    assert torch.isfinite(got).all() and got.abs().max() <= 448 and (got[0, 1, 1, 0] == 0).all()
    off = got != want
    # one e4m3 step is at most 1/8 of the value (2^-3 relative at the bottom of a binade; subnormals: 2^-9 absolute)
    assert off.float().mean().item() < 1e-3 and ((got - want).abs()[off] <= want.abs()[off] / 8 + 2.0 ** -9).all()
    print(f"quantiser L = {L}: {int(off.sum())} of {off.numel()} bytes one step from torch's rounding")
