#!/usr/bin/env python3
"""Golden vectors for ``KP_influence: gaussian | constant`` and ``aggregation_mode: closest``
(models/backbone_kpconv/finegrained_kpconv_blocks.py:347-372), computed by running the
REFERENCE itself.

TEST INFRASTRUCTURE ONLY, beside make_golden.py (whose helpers it imports and which it leaves
untouched): it needs the reference checkout and oracle/_ref/libkpconv_ref.so, and runs on the
CPU. Only the .npz files it writes travel.

  kpconv_modes.npz                  the reference's KPConv module (15 kernel points, 16 -> 24
                                    channels) on one small table for the five new (influence,
                                    aggregation) pairs: inputs, kernel points, and per pair the
                                    weights and the output. Pins tests/_kpconv_modes.py's
                                    restatement to the reference.
  forward_modelnet_kp_gaussian.npz  forward_modelnet_small's config, pairs and seed plus
                                    KP_influence='gaussian'
  forward_modelnet_kp_closest.npz   the same plus aggregation_mode='closest', on tie-edited
                                    neighbour tables (below)
  train_modelnet_kp_gaussian.npz    make_golden.make_train's recipe on the gaussian model, in
                                    fp32 and with the reference's modules in fp64, at the
                                    first weight seed whose step fp32 resolves (make_train)

Near-ties. ``closest`` sends a neighbour to the weight matrix of its nearest kernel point; two
fp32 evaluations of d2 that round differently may pick different ones where two kernel points
are nearly equidistant, and no tolerance covers that. So the tables of the fixtures are edited:
an entry becomes the shadow index when, in fp64, the gap between its two smallest d2 is below
a stated fraction of extent^2 under the kernel points of ANY KPConv that reads the table
(kpconv_modes: TIE_UNIT = 1e-3, the rule of tests/_kpconv_modes.py; the forward fixture:
TIE_MODEL = 1e-5, at most 0.1 % of a table's valid entries, asserted). The forward fixture's
reference run wraps the reference model's own preprocessor to apply the edit, the edited tables
are what the fixture stores, and the generator asserts that on them the fp32 argmin equals the
fp64 argmin for every valid entry of every KPConv.

Each forward fixture must be able to tell its option from linear / sum: the generator asserts
that src_feat differs from forward_modelnet_small's by rel_err > 1e-2 (MIN_DIFF, 100 x the
forward tests' tolerance).

Usage:  python tests/golden/make_golden_kpconv_modes.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_golden as mg  # noqa: E402

NEW_COMBOS = [('linear', 'closest'), ('gaussian', 'sum'), ('gaussian', 'closest'),
              ('constant', 'sum'), ('constant', 'closest')]
GAUSSIAN = dict(mg.SMALL_MODELNET, KP_influence='gaussian')
CLOSEST = dict(mg.SMALL_MODELNET, aggregation_mode='closest')
MIN_DIFF = 1e-2
TIE_UNIT, TIE_MODEL, MAX_SHARE = 1e-3, 1e-5, 1e-3
OWN_TOL = 2.5e-3       # the reference's fp32 training step against its own fp64 run (make_train)


def _rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))


def _d2(q, s, idx, kp, dtype):
    q, s, kp = q.to(dtype), s.to(dtype), kp.to(dtype)
    sp = torch.cat((s, torch.zeros_like(s[:1]) + 1e6), 0)
    nb = sp[idx] - q.unsqueeze(1)
    return ((nb.unsqueeze(2) - kp) ** 2).sum(3)


def _near_ties(q, s, idx, kp, extent, frac):
    """Valid entries whose two smallest fp64 d2 are closer than frac * extent^2."""
    two = torch.topk(_d2(q, s, idx, kp, torch.float64), 2, dim=2, largest=False).values
    return ((two[..., 1] - two[..., 0]) < frac * extent ** 2) & (idx < s.shape[0])


def _assert_argmin_agrees(q, s, idx, kp, what):
    valid = idx < s.shape[0]
    a64 = torch.argmin(_d2(q, s, idx, kp, torch.float64), dim=2)
    a32 = torch.argmin(_d2(q, s, idx, kp, torch.float32), dim=2)
    assert bool((a64 == a32)[valid].all()), ('fp32 and fp64 argmin disagree', what)


def make_module():
    import backbone_kpconv.finegrained_kpconv_blocks as fb
    g = np.load(os.path.join(HERE, 'geom_modelnet.npz'))
    pts = torch.from_numpy(g['points'])
    limit = int(g['limit'])
    NQ, extent, radius = 300, 0.06, 0.0825
    q = pts[:NQ]
    idx = torch.from_numpy(g['conv'][:NQ, :limit].astype(np.int64))
    torch.manual_seed(2)
    np.random.seed(2)
    x = torch.randn(len(pts), 16)
    x[::7] = -x[::7].abs()           # rows whose feature sum is <= 0 do not count (blocks:395-399)
    arrays, kp0 = {}, None
    for influence, aggregation in NEW_COMBOS:
        cwd = os.getcwd()
        os.chdir(mg.REF)
        try:
            conv = fb.KPConv(15, 3, 16, 24, KP_extent=extent, radius=radius,
                             fixed_kernel_points='center', KP_influence=influence,
                             aggregation_mode=aggregation)
        finally:
            os.chdir(cwd)
        conv.eval()
        if kp0 is None:              # one set of kernel points for the five modules
            kp0 = conv.kernel_points.detach().clone()
            tie = _near_ties(q, pts, idx, kp0, extent, TIE_UNIT)
            share = int(tie.sum()) / int((idx < len(pts)).sum())
            print(f'kpconv_modes: tie rule replaces {share:.3%} of the valid entries')
            assert share <= 0.01, share
            idx[tie] = len(pts)
            _assert_argmin_agrees(q, pts, idx, kp0, 'kpconv_modes')
        conv.kernel_points.data.copy_(kp0)
        with torch.no_grad():
            out = conv(q, pts, idx, x)
        arrays[f'W.{influence}.{aggregation}'] = conv.weights.detach().numpy()
        arrays[f'out.{influence}.{aggregation}'] = out.numpy()
    mg.save('kpconv_modes', q=q.numpy(), s=pts.numpy(), idx=mg._idx(idx.numpy()), x=x.numpy(),
            kp=kp0.numpy(), extent=np.float64(extent), radius=np.float64(radius), **arrays)


def _pairs():
    pairs = [mg.modelnet_like_pair(i, n_raw=512) for i in range(2)]     # forward_modelnet_small's
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _assert_differs(out, what):
    base = np.load(os.path.join(HERE, 'forward_modelnet_small.npz'))
    for b in range(2):
        diff = _rel_err(out['src_feat'][b].numpy(), base[f'out.src_feat.{b}'])
        print(f'{what}: src_feat.{b} vs linear / sum: rel_err {diff:.3g}')
        assert diff > MIN_DIFF, ('the fixture cannot tell the option from linear / sum', what, b, diff)


def _tables(model, meta):
    """(name, level, q, s, [KPConv modules reading it]) of every neighbour table a KPConv reads."""
    blocks = [m for m in model.modules() if hasattr(m, 'KPConv') and hasattr(m, 'layer_ind')]
    out = []
    for key in ('neighbors', 'pools'):
        for l in range(len(meta[key])):
            strided = key == 'pools'
            convs = [b.KPConv for b in blocks
                     if b.layer_ind == l and ('strided' in b.block_name) == strided]
            if convs:
                q = meta['points'][l + 1] if strided else meta['points'][l]
                out.append((key, l, q, meta['points'][l], convs))
    return out


def _tie_edit(model, meta):
    """Replaces near-tied entries by the shadow index, in place."""
    for key, l, q, s, convs in _tables(model, meta):
        idx = meta[key][l]
        tie = torch.zeros_like(idx, dtype=torch.bool)
        for c in convs:
            tie |= _near_ties(q, s, idx, c.kernel_points.detach(), float(c.KP_extent), TIE_MODEL)
        share = int(tie.sum()) / max(int((idx < s.shape[0]).sum()), 1)
        print(f'closest: {key}[{l}] ({len(convs)} convs): {int(tie.sum())} near-ties, {share:.4%}')
        assert share <= MAX_SHARE, (key, l, share)
        idx[tie] = s.shape[0]
        for c in convs:
            _assert_argmin_agrees(q, s, idx, c.kernel_points.detach(), (key, l))
    return meta


class _TieEdited(torch.nn.Module):
    """The reference model's own preprocessor, its tables tie-edited for the model's KPConvs."""

    def __init__(self, inner, model):
        super().__init__()
        self.inner = inner
        self.__dict__['model'] = model          # not a child module: no cycle

    def forward(self, *a, **k):
        return _tie_edit(self.__dict__['model'], self.inner(*a, **k))


def make_forward(fr, fk):
    src, tgt = _pairs()
    model, meta, out = mg.run_forward(fr, fk, mg.load_cfg('modelnet.yaml', **GAUSSIAN), src, tgt)
    assert model.kpf_encoder.encoder_blocks[0].KPConv.KP_influence == 'gaussian'
    _assert_differs(out, 'gaussian')
    mg.save('forward_modelnet_kp_gaussian', **mg.pack_forward(model, meta, out, GAUSSIAN, src, tgt, 4.0))

    model, _, _ = mg.run_forward(fr, fk, mg.load_cfg('modelnet.yaml', **CLOSEST), src, tgt)
    assert model.kpf_encoder.encoder_blocks[0].KPConv.aggregation_mode == 'closest'
    model.preprocessor = _TieEdited(model.preprocessor, model)
    batch = {'src_xyz': [torch.from_numpy(c) for c in src],
             'tgt_xyz': [torch.from_numpy(c) for c in tgt]}
    with torch.no_grad(), mg.cuda_to_cpu():
        out = model(batch)
    meta = batch['kpconv_meta']
    _assert_differs(out, 'closest')
    mg.save('forward_modelnet_kp_closest', **mg.pack_forward(model, meta, out, CLOSEST, src, tgt, 4.0))


def _cast(v, dtype):
    """Every floating tensor of a nested dict / list structure in ``dtype``."""
    if torch.is_tensor(v):
        return v.to(dtype) if v.is_floating_point() and v.dtype != dtype else v
    if isinstance(v, dict):
        return {k: _cast(x, dtype) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_cast(x, dtype) for x in v)
    return v


def _train_step(fr, fk, dtype, seed):
    """make_golden.make_train's step on the gaussian model (same pairs, loss inputs; weights of
    ``seed``) with the reference's modules in ``dtype`` -> (losses, {parameter: gradient}, model)."""
    src, tgt = _pairs()
    model, meta, out = mg.run_forward(fr, fk, mg.load_cfg('modelnet.yaml', **GAUSSIAN), src, tgt,
                                      seed=seed)
    lf = np.load(os.path.join(HERE, 'loss_modelnet_small.npz'))
    model.feature_criterion.W.data.copy_(torch.from_numpy(lf['W']))
    model.feature_criterion_un.W.data.copy_(torch.from_numpy(lf['W_un']))
    model.train()
    model.to(dtype)
    batch = _cast({'src_xyz': [torch.from_numpy(c) for c in src],
                   'tgt_xyz': [torch.from_numpy(c) for c in tgt],
                   'pose': torch.from_numpy(lf['pose']),
                   'src_overlap': [torch.from_numpy(lf[f'src_overlap.{b}']) for b in range(2)],
                   'tgt_overlap': [torch.from_numpy(lf[f'tgt_overlap.{b}']) for b in range(2)]}, dtype)
    model.zero_grad()
    with mg.cuda_to_cpu():
        pred = model(batch)
        # the preprocessor's tables and key points stay fp32 whatever the modules are
        pred, batch = _cast(pred, dtype), _cast(batch, dtype)
        losses = model.compute_loss(pred, batch)
        losses['total'].backward()
    return losses, {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, model


def _own_error(grads, grads64):
    """The reference's fp32 gradients against its own fp64 run: the worst relative error of a
    gradient norm and the worst relative Frobenius error of a TRAIN_FULL_GRADS gradient."""
    worst = (0.0, None)
    for k, g in grads.items():
        n, n64 = float(g.double().norm()), float(grads64[k].norm())
        worst = max(worst, (abs(n - n64) / max(n64, 1e-12), 'gnorm.' + k))
        if k in mg.TRAIN_FULL_GRADS:
            worst = max(worst, (float((g.double() - grads64[k]).norm()) / max(n64, 1e-12), 'grad.' + k))
    return worst


def make_train(fr, fk):
    """The recipe of make_golden.make_train on the gaussian model in fp32 (loss.*, gnorm.*,
    gsum.*, grad.*), and the same step with the reference's modules in fp64 (f64.loss.*,
    f64.gnorm.*, f64.grad.*, the full gradients stored as fp32).

    The weight seed is chosen by a rule on the reference alone. The gradient of this network is
    discontinuous where an activation input sits at its kink (tests/test_gpu_train.py's module
    docstring), as ``closest`` is where two kernel points tie, and a fixture on such a point is
    met by chance only. With seed 0 (make_train's) the gaussian model has one: an input of
    kpf_encoder.encoder_blocks.4's last ReLU / LeakyReLU lies 9.4e-7 from zero, the reference's
    fp32 forward takes the other branch than its own fp64 forward there, and its fp32 gradients
    of the whole encoder are up to 1.2e-2 from its fp64 ones -- above the 1e-2 that the tests
    allow an implementation. So, like the tie rule of the tables: the fixture takes the smallest
    seed for which the reference's fp32 step agrees with its own fp64 step within OWN_TOL =
    GRAD_TOL / 4 = 2.5e-3 in every gradient norm and every stored full gradient (a yardstick
    four times finer than the bound it is used for). The figures of every seed tried are
    printed. The weights of that seed are rebuilt by the test from (key, shape, seed) as every
    fixture's are (named_weights.py); the kernel points of that seed are stored (sd.*)."""
    for seed in range(8):
        losses, grads, model = _train_step(fr, fk, torch.float32, seed)
        losses64, grads64, _ = _train_step(fr, fk, torch.float64, seed)
        err, where = _own_error(grads, grads64)
        print(f'seed {seed}: the reference in fp32 against its own fp64 run: worst {err:.3e} ({where})')
        if err <= OWN_TOL:
            break
    else:
        raise AssertionError('no seed below 8 gives a reference step that fp32 resolves')
    fwd = np.load(os.path.join(HERE, 'forward_modelnet_kp_gaussian.npz'))
    assert repr([(k, list(sh)) for k, sh in model.sd_keys_shapes]) == _keys_repr(fwd)
    arrays = {'sd_seed': np.int64(seed)}
    for k, v in model.state_dict().items():
        if 'kernel_points' in k:
            arrays[f'sd.{k}'] = v.float().numpy()
    for k, v in losses.items():
        arrays[f'loss.{k}'] = np.float32(v.item())
        arrays[f'f64.loss.{k}'] = np.float64(losses64[k].item())
    for k, g in grads.items():
        g, g64 = g.double(), grads64[k]
        arrays[f'gnorm.{k}'] = np.float64(g.norm().item())
        arrays[f'gsum.{k}'] = np.float64(g.sum().item())
        arrays[f'f64.gnorm.{k}'] = np.float64(g64.norm().item())
        if k in mg.TRAIN_FULL_GRADS:
            arrays[f'grad.{k}'] = grads[k].numpy()
            arrays[f'f64.grad.{k}'] = g64.float().numpy()
    mg.save('train_modelnet_kp_gaussian', **arrays)


def _keys_repr(npz):
    raw = npz['sd_keys'].item()
    return raw.decode() if isinstance(raw, bytes) else str(raw)


if __name__ == '__main__':
    fr, fk = mg.import_reference()
    make_module()
    make_forward(fr, fk)
    make_train(fr, fk)
