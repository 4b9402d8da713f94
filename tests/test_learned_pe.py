"""``pos_emb_type: learned`` (PositionEmbeddingLearned, position_embedding.py:52-71) builds,
and its state_dict is the reference's: keys, order and shapes of the fixtures' own lists (the
reference model's state_dict), for the regressor head and for the CorrespondenceDecoder, which
holds the same module (the MLP then appears under both prefixes). CPU only."""
import ast

import pytest
import torch

from conftest import forward_fixture


def _sd_keys(d):
    raw = d['sd_keys'].item()
    return ast.literal_eval(raw.decode() if isinstance(raw, bytes) else str(raw))


@pytest.mark.parametrize('name', ['forward_modelnet_learned_pe',
                                  'forward_modelnet_learned_pe_decoder'])
def test_learned_pe_state_dict_is_the_references(name):
    import fgreg
    from fgreg.transformer import PositionEmbeddingLearned
    cfg, sd, _, _, _, d = forward_fixture(name)
    assert cfg.pos_emb_type == 'learned'
    model = fgreg.RegTR(cfg)
    assert isinstance(model.pos_embed, PositionEmbeddingLearned)
    mine = [(k, list(v.shape)) for k, v in model.state_dict().items()
            if not k.startswith('feature_criterion')]
    ref = [(k, list(s)) for k, s in _sd_keys(d)]
    assert mine == ref
    pe = [k for k, _ in ref if k.startswith('pos_embed.')]
    assert pe == [f'pos_embed.mlp.{i}.{t}' for i in (0, 2, 4, 6, 8) for t in ('weight', 'bias')]
    decoder = 'decoder' in name
    assert decoder == any(k.startswith('correspondence_decoder.pos_embed.') for k, _ in ref)
    # a reference checkpoint loads without unexpected keys; where the MLP is stored under both
    # prefixes the parameter ends with the value the reference ends with (load_state_dict
    # visits pos_embed first, then correspondence_decoder.pos_embed: the later copy stays)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith('feature_criterion') for k in missing)
    last = 'correspondence_decoder.pos_embed.' if decoder else 'pos_embed.'
    for i in (0, 2, 4, 6, 8):
        assert torch.equal(model.pos_embed.mlp[i].weight, sd[f'{last}mlp.{i}.weight'])
        assert torch.equal(model.pos_embed.mlp[i].bias, sd[f'{last}mlp.{i}.bias'])
    if decoder:
        assert model.correspondence_decoder.pos_embed is model.pos_embed
        assert not torch.equal(sd['pos_embed.mlp.8.weight'],
                               sd['correspondence_decoder.pos_embed.mlp.8.weight'])


def test_learned_pe_widths():
    from fgreg.transformer import PositionEmbeddingLearned
    m = PositionEmbeddingLearned(3, 512)
    assert [tuple(m.mlp[i].weight.shape) for i in (0, 2, 4, 6, 8)] == \
        [(32, 3), (64, 32), (128, 64), (256, 128), (512, 256)]
    assert all(isinstance(m.mlp[i], torch.nn.ReLU) for i in (1, 3, 5, 7))


def test_unknown_pos_emb_type_still_raises():
    import fgreg
    with pytest.raises(NotImplementedError):
        fgreg.RegTR(fgreg.config.get('modelnet', pos_emb_type='bogus'))
