"""CPU: the KPConv influence functions (KP_influence: linear | gaussian | constant) and
aggregation modes (aggregation_mode: sum | closest) of finegrained_kpconv_blocks.py:347-372
build through every layer that carries them, unknown values are refused with the reference's
messages, and the C ABI refuses an unknown mode code without a GPU."""
import ctypes
import itertools

import pytest
import torch

import _kpconv_modes as km
from conftest import golden, rel_err

COMBOS = list(itertools.product(('linear', 'gaussian', 'constant'), ('sum', 'closest')))


@pytest.mark.parametrize('influence,aggregation', COMBOS)
def test_kpconv_and_model_build(influence, aggregation):
    import fgreg
    import fgreg.config as fc
    from fgreg.backbone import KPConv
    conv = KPConv(15, 3, 16, 24, KP_extent=0.06, radius=0.0825, KP_influence=influence,
                  aggregation_mode=aggregation)
    assert (conv.KP_influence, conv.aggregation_mode) == (influence, aggregation)
    assert tuple(conv.weights.shape) == (15, 16, 24) and tuple(conv.kernel_points.shape) == (15, 3)
    model = fgreg.RegTR(fc.get('modelnet', first_feats_dim=32, d_embed=32, d_feedforward=64,
                               KP_influence=influence, aggregation_mode=aggregation))
    convs = [m for m in model.modules() if isinstance(m, KPConv)]
    assert len(convs) >= 5
    assert all((c.KP_influence, c.aggregation_mode) == (influence, aggregation) for c in convs)


def test_unknown_values_raise_the_reference_messages():
    from fgreg import ops
    from fgreg.backbone import KPConv
    kw = dict(KP_extent=0.06, radius=0.0825)
    with pytest.raises(ValueError, match=r'Unknown influence function type \(config.KP_influence\)'):
        KPConv(15, 3, 16, 24, KP_influence='cubic', **kw)
    with pytest.raises(ValueError, match="Unknown convolution mode. Should be 'closest' or 'sum'"):
        KPConv(15, 3, 16, 24, aggregation_mode='mean', **kw)
    with pytest.raises(ValueError):
        ops.kp_modes('linear', 'max')
    assert ops.kp_modes('gaussian', 'closest') == (1, 1) and ops.kp_modes('constant', 'sum') == (2, 0)
    # what stays out of scope stays NotImplementedError
    with pytest.raises(NotImplementedError):
        KPConv(15, 3, 16, 24, deformable=True, **kw)
    with pytest.raises(NotImplementedError):
        KPConv(15, 2, 16, 24, **kw)


def test_abi_refuses_unknown_modes_without_gpu():
    """fgr_kpconv_gather_mode / fgr_kpconv_scatter_mode with a mode code outside FGR_KP_* /
    FGR_AGG_* return FGR_E_ARG, name themselves and the value in fgr_last_error, and launch
    nothing (no GPU here); with nq = 0 the six valid pairs are accepted."""
    import fgreg
    L = fgreg.load()
    f1 = ctypes.c_float(1.0)
    gather = lambda nq, inf, agg: L.fgr_kpconv_gather_mode(None, None, nq, 10, None, 4, None, 16, None,
                                                           15, f1, inf, agg, None, None, None, 0, None)
    for nq in (0, 10):
        assert gather(nq, 7, 0) == -1
        msg = L.fgr_last_error().decode()
        assert 'fgr_kpconv_gather_mode' in msg and 'influence 7' in msg, msg
        assert gather(nq, 0, 2) == -1
        assert 'aggregation 2' in L.fgr_last_error().decode()
        assert gather(nq, -1, 0) == -1
    for inf, agg in itertools.product(range(3), range(2)):
        assert gather(0, inf, agg) == 0
    # the width refusal of fgr_kpconv_gather holds for the new entry point
    assert L.fgr_kpconv_gather_mode(None, None, 0, 10, None, 4, None, 96, None, 15, f1, 1, 1, None,
                                    None, None, 0, None) == -1
    assert b'cin 96 unsupported (need 1..64, 128 or 256)' in L.fgr_last_error()
    rc = L.fgr_kpconv_scatter_mode(None, None, 10, 10, None, 4, None, 16, None, 15, f1, 3, 0, None,
                                   None, None, None, 0, None)
    assert rc == -1
    msg = L.fgr_last_error().decode()
    assert 'fgr_kpconv_scatter_mode' in msg and 'influence 3' in msg, msg


@pytest.mark.parametrize('influence,aggregation', km.NEW_COMBOS)
def test_restatement_matches_the_reference_module(influence, aggregation):
    """tests/_kpconv_modes.py's fp64 restatement (the checker of the GPU tests) against the
    reference's own KPConv module run in fp32 (kpconv_modes.npz, whose table follows the tie
    rule): within 1e-5, ten times under the forward tests' tolerance."""
    d = golden('kpconv_modes')
    T = lambda k: torch.from_numpy(d[k])
    out = km.kpconv_ref(T('q').double(), T('s').double(), T('idx').long(), T('x').double(),
                        T(f'W.{influence}.{aggregation}').double(), T('kp').double(),
                        float(d['extent']), influence, aggregation)
    assert rel_err(out, d[f'out.{influence}.{aggregation}']) < 1e-5


@pytest.mark.parametrize('cin,H,n_kp', [(1, 7, 15), (16, 70, 15), (64, 70, 15), (128, 7, 17),
                                        (256, 70, 32), (12, 70, 15)])
def test_table_rules_hold(cin, H, n_kp):
    """The builder's own assertions (tie rule <= 1 %, both rules <= 15 %, fp32 argmin = fp64
    argmin on the edited table) and that no near-tie is left."""
    q, s, idx, x, kp, cnt = km.table(cin, H, n_kp)
    d2 = km.sq_distances(q.double(), s.double(), idx, kp.double())
    assert float(km.tie_gap(d2)[idx < s.shape[0]].min()) >= km.TIE * km.EXT ** 2
    assert bool((idx[3] == s.shape[0]).all()) and float(cnt[3]) == 1.0
