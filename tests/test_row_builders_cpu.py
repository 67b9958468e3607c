"""not gpu: the three row builders the generation hosts share -- `t5_engine.guided_rows`, `t5_engine.eos_id_table`,
`ConditioningEmbedders.encoder_bias` -- each against a restatement written out here."""
import pytest
import torch

from mapperatorinator_amd.conditioning import ConditioningEmbedders
from mapperatorinator_amd.t5_engine import eos_id_table, guided_rows


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("with_forced", [False, True])
def test_guided_rows_are_negative_rows_over_prompt_rows(with_mask, with_forced):
    prompt = torch.tensor([[1, 7, 9], [0, 1, 8]])                              # 2 prompts x 3 columns
    neg = torch.tensor([[1, 5], [0, 1]], dtype=torch.int32)                    # 2 columns, another integer type
    mask = prompt.ne(0) if with_mask else None
    forced = torch.arange(12).reshape(2, 6) if with_forced else None
    kept = prompt.clone()
    p, m, f = guided_rows(prompt, mask, neg, forced)
    assert torch.equal(prompt, kept)                                           # the caller's prompt is not written to
    assert p.dtype == prompt.dtype and p.tolist() == [[1, 5, 9], [0, 1, 8], [1, 7, 9], [0, 1, 8]]
    assert (m is None) if mask is None else m.tolist() == [[True, True, True], [False, True, True]] * 2
    assert (f is None) if forced is None else f.tolist() == forced.tolist() * 2
    assert guided_rows(prompt, mask, neg)[2] is None
    with pytest.raises(ValueError, match="^negative prompt longer than the prompt$"):
        guided_rows(prompt, mask, torch.tensor([[1, 5, 6, 2], [0, 1, 3, 2]]), forced)   # one column too long


def test_eos_id_table_marks_the_ids_inside_the_vocabulary():
    vocab = 11
    table = eos_id_table([2, 7, 2, vocab, -1, 10], vocab)                     # a duplicate, one id == vocab_out, a negative id
    assert table.dtype == torch.uint8 and table.shape == (vocab,) and table.device.type == "cpu"
    assert table.tolist() == [0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1]
    assert eos_id_table(torch.tensor([3]), 4).tolist() == [0, 0, 0, 1]
    for none in ([], None, [vocab], [-3]):
        assert eos_id_table(none, vocab).tolist() == [0] * vocab


def test_encoder_bias_is_row_bias_with_an_encoder_embedder_and_channels_without():
    from mapperatorinator_amd.t5_engine import T5_PRESETS
    from mh_testing import add_random_conditioning, random_t5_state_dict
    sd = random_t5_state_dict(T5_PRESETS["tiny"], 64, 64, seed=3)
    add_random_conditioning(sd, 128, 388, 16, 11, seed=1)
    kw = dict(difficulty=torch.tensor([3.0, 6.5]), mapper_idx=torch.tensor([-1, 4]), song_position=torch.tensor([[0.0, 0.3], [0.3, 0.6]]))
    projected = ConditioningEmbedders(sd, 388)
    bare = {k: v for k, v in sd.items() if not k.startswith("encoder_embedder.")}
    vec = projected.vectors(2, **kw)
    bare["transformer.model.encoder.conv1.weight"] = torch.zeros(8, 388 + vec.shape[1], 3)
    as_channels = ConditioningEmbedders(bare, 388)
    assert not projected.as_channels and as_channels.as_channels and as_channels.active and vec.shape[0] == 2
    for dtype in (torch.bfloat16, torch.float32):
        assert torch.equal(projected.encoder_bias(vec, dtype), projected.row_bias(vec, dtype))
        assert projected.encoder_bias(vec, dtype).shape == (2, 128)
        assert torch.equal(as_channels.encoder_bias(vec, dtype), as_channels.channels(vec, dtype))
        assert as_channels.encoder_bias(vec, dtype).shape == vec.shape
    assert not torch.equal(projected.encoder_bias(vec, torch.bfloat16), projected.encoder_bias(vec, torch.float32))
