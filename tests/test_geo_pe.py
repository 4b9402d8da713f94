"""``pos_emb_type: geometric`` (GeometricStructureEmbedding, position_embedding.py:129-196)
builds, its state_dict is the reference's (keys, order and shapes of the fixture's own list),
the optional geo_* keys reach the module, and the refusals are raised at construction. CPU only
(the embedding itself has no CPU path: tests/test_gpu_geo_embed.py, tests/test_gpu_geo_pe.py)."""
import ast

import numpy as np
import pytest
import torch

import _geo_ref as gr
from conftest import forward_fixture, golden


def _sd_keys(d):
    raw = d['sd_keys'].item()
    return ast.literal_eval(raw.decode() if isinstance(raw, bytes) else str(raw))


def test_geo_pe_state_dict_is_the_references():
    import fgreg
    from fgreg.transformer import GeometricStructureEmbedding
    cfg, sd, _, _, _, d = forward_fixture('forward_modelnet_geo_pe')
    assert cfg.pos_emb_type == 'geometric' and cfg.geo_sigma_d == 0.05
    model = fgreg.RegTR(cfg)
    assert isinstance(model.pos_embed, GeometricStructureEmbedding)
    mine = [(k, list(v.shape)) for k, v in model.state_dict().items()
            if not k.startswith('feature_criterion')]
    ref = [(k, list(s)) for k, s in _sd_keys(d)]
    assert mine == ref
    assert [k for k, _ in ref if k.startswith('pos_embed.')] == \
        ['pos_embed.embedding.div_term'] + [f'pos_embed.proj_{p}.{t}' for p in 'da'
                                            for t in ('weight', 'bias')]
    # div_term is a buffer of constants from torch.exp on the host (its last bit differs between
    # CPUs' vector libraries): ours is the reference's own
    assert torch.allclose(model.pos_embed.embedding.div_term, sd['pos_embed.embedding.div_term'],
                          rtol=1e-6, atol=0)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith('feature_criterion') for k in missing)


def test_class_fixture_keys_and_defaults():
    from fgreg.transformer import GeometricStructureEmbedding
    f = golden('pos_embed_geo')
    m = GeometricStructureEmbedding(256)
    assert (m.sigma_d, m.sigma_a, m.angle_k, m.reduction_a) == (0.2, 15, 3, 'max')
    assert [(k, list(v.shape)) for k, v in m.state_dict().items()] == \
        [(k, list(s)) for k, s in _sd_keys(f)]
    assert torch.allclose(m.embedding.div_term, torch.from_numpy(f['div_term']), rtol=1e-6, atol=0)
    assert torch.equal(m.embedding.div_term, gr.div_term(256, torch.float32))
    with pytest.raises(ValueError, match='Unsupported reduction mode'):
        GeometricStructureEmbedding(256, reduction_a='sum')
    with pytest.raises(ValueError, match='odd d_model'):
        GeometricStructureEmbedding(255)


def test_short_cloud_is_refused_before_any_launch():
    """n <= k: ValueError from the host lengths (no GPU needed to see it)."""
    from fgreg.transformer import GeometricStructureEmbedding
    m = GeometricStructureEmbedding(256)
    xyz = torch.zeros(43, 3)
    off = torch.tensor([0, 3, 43])
    for fn in (m, m.forward_composed, m.train_forward):
        with pytest.raises(ValueError, match='3 points'):
            fn(xyz, off, [3, 40])


def test_regtr_options_and_refusals():
    import fgreg
    import fgreg.config as fc
    geo = dict(pos_emb_type='geometric')
    pe = fgreg.RegTR(fc.get('modelnet', **geo)).pos_embed
    assert (pe.sigma_d, pe.sigma_a, pe.angle_k, pe.reduction_a) == (0.2, 15, 3, 'max')
    pe = fgreg.RegTR(fc.get('modelnet', geo_sigma_d=0.05, geo_sigma_a=10, geo_angle_k=4,
                            geo_reduction_a='mean', **geo)).pos_embed
    assert (pe.sigma_d, pe.sigma_a, pe.angle_k, pe.reduction_a) == (0.05, 10, 4, 'mean')
    with pytest.raises(NotImplementedError, match='corr_decoder_has_pos_emb'):
        fgreg.RegTR(fc.get('modelnet', direct_regress_coor=False, **geo))
    dec = fgreg.RegTR(fc.get('modelnet', direct_regress_coor=False,
                             corr_decoder_has_pos_emb=False, **geo))
    assert not dec.correspondence_decoder.use_pos_emb
    with pytest.raises(ValueError, match='Unsupported reduction mode'):
        fgreg.RegTR(fc.get('modelnet', geo_reduction_a='median', **geo))
    with pytest.raises(NotImplementedError):
        fgreg.RegTR(fc.get('modelnet', pos_emb_type='bogus'))


def test_host_restatement_tie_rule():
    """tests/_geo_ref.knn: the point itself is excluded by index (a duplicate of it is not), and
    ties go to the lower index."""
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 1]], np.float32)
    nn = gr.knn(x, [5], 3, dtype=np.float32)
    assert nn[0].tolist() == [3, 1, 2] and nn[3].tolist() == [0, 1, 2]
    assert gr.knn(np.concatenate([x, x]), [5, 5], 3, dtype=np.float32)[5].tolist() == [8, 6, 7]
