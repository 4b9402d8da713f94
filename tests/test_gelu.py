"""``transformer_act: gelu`` (transformers.py:265-273, F.gelu) builds, the activation adds no
parameters (the state_dict is the reference's GELU model's, which is the ReLU model's list), and
the option's other values behave as the reference's _get_activation_fn: 'glu' cannot work there
either (refused with the reason), anything else is a RuntimeError. CPU only."""
import ast

import pytest

from conftest import forward_fixture


def _sd_keys(d):
    raw = d['sd_keys'].item()
    return ast.literal_eval(raw.decode() if isinstance(raw, bytes) else str(raw))


def test_gelu_model_builds():
    import fgreg
    from fgreg import ops
    model = fgreg.RegTR(fgreg.config.get('modelnet', transformer_act='gelu'))
    layers = model.transformer_encoder.layers
    assert len(layers) > 0 and all(l.act == ops.ACT_GELU == 4 for l in layers)
    relu = fgreg.RegTR(fgreg.config.get('modelnet'))
    assert all(l.act == ops.ACT_RELU for l in relu.transformer_encoder.layers)
    assert [(k, v.shape) for k, v in model.state_dict().items()] == \
        [(k, v.shape) for k, v in relu.state_dict().items()]


@pytest.mark.parametrize('name', ['forward_modelnet_gelu', 'forward_modelnet_gelu_postnorm'])
def test_gelu_state_dict_is_the_references(name):
    import fgreg
    cfg, sd, _, _, _, d = forward_fixture(name)
    assert cfg.transformer_act == 'gelu' and cfg.pre_norm == ('postnorm' not in name)
    model = fgreg.RegTR(cfg)
    mine = [(k, list(v.shape)) for k, v in model.state_dict().items()
            if not k.startswith('feature_criterion')]
    ref = [(k, list(s)) for k, s in _sd_keys(d)]
    assert mine == ref
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith('feature_criterion') for k in missing)
    if 'postnorm' not in name:
        # the activation has no parameters: the same list as the ReLU model's fixture
        assert ref == [(k, list(s)) for k, s in _sd_keys(forward_fixture('forward_modelnet_small')[5])]


def test_glu_is_refused_with_the_reason():
    import fgreg
    with pytest.raises(NotImplementedError, match='halves the hidden width'):
        fgreg.RegTR(fgreg.config.get('modelnet', transformer_act='glu'))


def test_unknown_activation_is_a_runtime_error():
    import fgreg
    with pytest.raises(RuntimeError) as e:
        fgreg.RegTR(fgreg.config.get('modelnet', transformer_act='swish'))
    assert not isinstance(e.value, NotImplementedError)      # a subclass of RuntimeError


def test_relu_still_builds():
    import fgreg
    from fgreg.transformer import TransformerCrossEncoderLayer
    fgreg.RegTR(fgreg.config.get('modelnet', transformer_act='relu'))
    assert TransformerCrossEncoderLayer(32, 4, 64).act == fgreg.ops.ACT_RELU
