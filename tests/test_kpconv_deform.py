"""CPU: deformable / modulated KPConv blocks (finegrained_kpconv_blocks.py:215-234, :270-345,
:384-385) build through every layer with the reference's state_dict keys, what stays out of
scope is still refused, tests/_kpconv_deform.py's restatement agrees with the reference's own
module, its table rules hold, and the four new C entry points check their arguments without a
GPU."""
import ast
import ctypes
import itertools

import pytest
import torch

import _kpconv_deform as kd
from conftest import forward_fixture, golden, rel_err

ARCH = ['simple', 'resnetb', 'resnetb_deformable', 'resnetb_deformable_strided',
        'resnetb_deformable', 'resnetb']


@pytest.mark.parametrize('name,modulated', [('forward_modelnet_deform', False),
                                            ('forward_modelnet_deform_mod', True)])
def test_model_has_the_reference_state_dict(name, modulated):
    """A model of the fixture's config has exactly the reference's state_dict keys and shapes, in
    the reference's order, and loads the rebuilt weights strictly."""
    import fgreg
    from fgreg.backbone import DeformableKPConv
    cfg, sd, _, _, _, d = forward_fixture(name)
    assert list(cfg.architecture) == ARCH and bool(cfg.modulated) == modulated
    model = fgreg.RegTR(cfg)
    raw = d['sd_keys'].item()
    keys = ast.literal_eval(raw.decode() if isinstance(raw, bytes) else str(raw))
    mine = [(k, list(v.shape)) for k, v in model.state_dict().items()
            if not k.startswith('feature_criterion')]
    assert mine == [(k, list(s)) for k, s in keys]
    own = {k: v for k, v in model.state_dict().items() if k.startswith('feature_criterion')}
    model.load_state_dict(dict(sd, **own), strict=True)
    convs = [m for m in model.modules() if isinstance(m, DeformableKPConv)]
    assert len(convs) == 3 and all(c.modulated == modulated for c in convs)
    K = cfg.num_kernel_points
    assert all(tuple(c.offset_bias.shape) == ((4 if modulated else 3) * K,) for c in convs)
    assert sum('.offset_' in k for k in model.state_dict()) == 9


def test_deformable_kpconv_parameters():
    from fgreg.backbone import DeformableKPConv, KPConv
    conv = DeformableKPConv(15, 3, 16, 24, KP_extent=0.06, radius=0.0825, modulated=True)
    assert [k for k, _ in conv.named_parameters()] == [
        'weights', 'offset_bias', 'kernel_points', 'offset_conv.weights', 'offset_conv.kernel_points']
    assert tuple(conv.offset_conv.weights.shape) == (15, 16, 60) and isinstance(conv.offset_conv, KPConv)
    assert bool((conv.offset_bias == 0).all()) and not conv.kernel_points.requires_grad
    assert conv.deformed_KP is None and conv.offset_features is None
    assert tuple(DeformableKPConv(15, 3, 16, 24, 0.06, 0.0825).offset_bias.shape) == (45,)


def test_out_of_scope_is_still_refused():
    import fgreg.config as fc
    from fgreg.backbone import KPConv, block_decider
    with pytest.raises(NotImplementedError, match='DeformableKPConv'):
        KPConv(15, 3, 16, 24, KP_extent=0.06, radius=0.0825, deformable=True)
    cfg = fc.get('modelnet')
    for name in ('resnetb_invariant', 'simple_equivariant', 'resnetb_invariant_strided', 'unary',
                 'max_pool', 'nearest_upsample'):
        with pytest.raises(NotImplementedError):
            block_decider(name, 0.08, 64, 128, 0, cfg)
    for name in ('simple_deformable', 'simple_deformable_strided', 'resnetb_deformable',
                 'resnetb_deformable_strided'):
        block_decider(name, 0.08, 64, 128, 0, cfg)


@pytest.mark.parametrize('modulated', [False, True])
@pytest.mark.parametrize('influence,aggregation', kd.COMBOS)
def test_restatement_matches_the_reference_module(influence, aggregation, modulated):
    """The fp64 restatement (the checker of the GPU tests) against the reference's own
    KPConv(deformable=True) run in fp32 (kpconv_deform.npz): output and deformed_KP within 1e-5."""
    d = golden('kpconv_deform')
    name = f'{influence}.{aggregation}.{int(modulated)}'
    T = lambda k: torch.from_numpy(d[k]).double()
    out, kp_q = kd.deform_kpconv_ref(T('q'), T('s'), torch.from_numpy(d['idx']).long(), T('x'),
                                     T(f'W.{name}'), T('kp'), T(f'offset_W.{name}'), T('offset_kp'),
                                     T(f'offset_bias.{name}'), float(d['extent']), influence,
                                     aggregation, modulated)
    assert rel_err(kp_q, d[f'deformed_KP.{name}']) < 1e-5
    assert rel_err(out, d[f'out.{name}']) < 1e-5


@pytest.mark.parametrize('cin,H,n_kp', [(1, 7, 15), (16, 70, 15), (64, 70, 17), (128, 7, 15),
                                        (256, 70, 32), (12, 70, 15)])
def test_table_rules_hold(cin, H, n_kp):
    """The builder's own assertions (module docstring of _kpconv_deform.py) and that no unsafe
    entry is left on the edited table."""
    q, s, idx, x, kp, kp_q, mod, cnt, st = kd.table(cin, H, n_kp)
    live = idx < s.shape[0]
    d2 = kd.sq_distances(q.double(), s.double(), idx, kp_q.double())
    assert not bool(kd.unsafe_entries(d2, kd.EXT, live)[1].any())
    assert st['share_tie'] <= 0.02 and st['share_all'] <= 0.20 and st['n_in'] >= 20 and st['n_out'] >= 20
    assert bool((idx[3] == s.shape[0]).all()) and float(cnt[3]) == 1.0
    assert float(mod.min()) > 0.2 and float(mod.max()) < 1.8


def _entry_points(L):
    """name -> call(nq, cin, n_kp, extent, inf, agg) with NULL operands."""
    f = ctypes.c_float
    return {
        'fgr_kpconv_gather_deform': lambda nq, cin, K, e, i, a: L.fgr_kpconv_gather_deform(
            None, None, nq, 0, None, 4, None, cin, None, None, K, f(e), i, a, None, None, None, 0, None),
        'fgr_kpconv_scatter_deform': lambda nq, cin, K, e, i, a: L.fgr_kpconv_scatter_deform(
            None, None, nq, 0, None, 4, None, cin, None, None, K, f(e), i, a, None, None, None, None,
            0, None),
        'fgr_kpconv_deform_grad': lambda nq, cin, K, e, i, a: L.fgr_kpconv_deform_grad(
            None, None, nq, 0, None, 4, None, cin, None, None, None, K, f(e), i, a, None, None, None),
    }


def test_abi_checks_arguments_without_gpu():
    """Each new entry point returns FGR_E_ARG and names itself and the bad value for a bad mode
    code, cin 96, n_kp 33 or extent 0, launching nothing (no GPU here), and accepts nq = 0 for
    the six mode pairs."""
    import fgreg
    L = fgreg.load()
    for name, call in _entry_points(L).items():
        for nq in (0, 10):
            for args, what in (((16, 15, 0.5, 7, 0), 'influence 7'), ((16, 15, 0.5, 0, 2), 'aggregation 2'),
                               ((16, 15, 0.5, -1, 1), 'influence -1'), ((96, 15, 0.5, 0, 0), 'cin 96'),
                               ((16, 33, 0.5, 0, 0), 'n_kp 33'), ((16, 15, 0.0, 0, 0), 'extent 0')):
                assert call(nq, *args) == -1, (name, nq, args)
                msg = L.fgr_last_error().decode()
                assert name + ':' in msg and what in msg, (name, msg)
        for inf, agg in itertools.product(range(3), range(2)):
            assert call(0, 16, 15, 0.5, inf, agg) == 0, (name, inf, agg)
    points = lambda nq, K, e: L.fgr_kpconv_deform_points(None, None, None, None, nq, K,
                                                         ctypes.c_float(e), None, None, None)
    for nq in (0, 10):
        for (K, e), what in (((33, 0.5), 'n_kp 33'), ((15, 0.0), 'extent 0')):
            assert points(nq, K, e) == -1
            msg = L.fgr_last_error().decode()
            assert 'fgr_kpconv_deform_points:' in msg and what in msg, msg
    assert points(0, 15, 0.5) == 0
    assert points(10, 15, 0.5) == -1 and b'null pointer' in L.fgr_last_error()
    nb = ctypes.c_size_t(7)
    assert L.fgr_kpconv_gather_deform_workspace(90, 16, nb) == 0 and nb.value == 0
    assert L.fgr_kpconv_scatter_deform_workspace(70, 7, 16, nb) == 0 and nb.value == 70 * 7 * 16 * 4
