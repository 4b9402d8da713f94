"""Cross-encoder transformer on packed, unpadded clouds.

Parameter names follow models/transformer/transformers.py (``layers.{i}.self_attn``,
``multihead_attn`` as nn.MultiheadAttention, ``linear1/2``, ``norm1-3``, final
``norm``), so reference checkpoints load unchanged. The compute differs in layout:
the reference pads src and tgt to (N_max, B, d) and runs every op twice (src, tgt)
with key padding masks (finegrained_regtr.py:164-179); here all 2B clouds stay
packed in one (N_tot, d) tensor in the encoder's cloud order
(src_0..src_{B-1}, tgt_0..tgt_{B-1}) and

* self-attention = one QKV GEMM over all rows + fgr_attention with every cloud
  attending to itself;
* cross-attention = one QKV GEMM over all rows + fgr_attention with cloud c
  attending to its partner (c + B) mod 2B -- both directions in one launch, reading
  the same pre-update activations exactly like the reference's simultaneous update
  (transformers.py:213-229);
* LayerNorm (+ positional embedding add) = fgr_layernorm.
Masked keys never exist, so no -inf masking is needed; padded query rows never exist,
so no work is wasted on them.
"""
import copy
import math

import torch
import torch.nn as nn

from . import linear as lin
from . import ops
from .linear import linear, linear_ln, ln_fusable

class Segments:
    """Device-side segment tables of one packed batch of 2B clouds (built before any graph
    capture: they are host -> device copies)."""

    def __init__(self, lengths, device, n_layers=0, phantoms=None):
        """``phantoms``: optional per-cloud counts of query-only rows appended after the 2B
        clouds' rows, grouped by cloud (the reference's padded positions, which it computes as
        queries of every attention and never as keys: CorrespondenceDecoder top-k masking on
        padded batches, finegrained_regtr.py:353-357). Each non-empty group is one more
        segment whose key segment is its cloud (self-attention) or the partner (cross);
        ``cloud_off`` = ``off[:2B + 1]`` is the clouds' own table."""
        self.lengths = [int(n) for n in lengths]
        n = len(self.lengths)
        assert n % 2 == 0
        self.B = n // 2
        self.phantoms = [int(p) for p in phantoms] if phantoms is not None else [0] * n
        assert len(self.phantoms) == n and min(self.phantoms, default=0) >= 0
        # segment -> the cloud it belongs to (the clouds first, then the phantom groups)
        self.seg_cloud = list(range(n)) + [c for c in range(n) if self.phantoms[c] > 0]
        self.seg_lengths = self.lengths + [p for p in self.phantoms if p > 0]
        self.n_phantom = sum(self.phantoms)
        self.off = ops.offsets(self.seg_lengths, device)
        self.cloud_off = self.off[:n + 1]
        self.self_seg = ops.to_device(self.seg_cloud, torch.int32, device)
        self.cross_seg = ops.to_device([(c + self.B) % n for c in self.seg_cloud], torch.int32,
                                       device)
        self.max_len = max(self.seg_lengths) if n else 0
        self.layer_tables = None
        if n_layers:
            # (layer, segment) segments of the L stacked layer outputs (L * N rows): segment
            # l * S + s attends to l * S + partner(cloud of s); value rows = the partner's xyz
            # rows, built from the host lengths (reading self.off back would sync the stream)
            N = sum(self.seg_lengths)
            S = len(self.seg_lengths)
            host_off = [0]
            for ln in self.seg_lengths[:-1]:
                host_off.append(host_off[-1] + ln)
            q_off = [l * N + o for l in range(n_layers) for o in host_off]
            q_off.append(n_layers * N)
            kv_seg = [l * S + (c + self.B) % n for l in range(n_layers) for c in self.seg_cloud]
            v_off = host_off * n_layers
            self.layer_tables = (ops.to_device(q_off, torch.int64, device),
                                 ops.to_device(kv_seg, torch.int32, device),
                                 ops.to_device(v_off, torch.int64, device))


class _QKTap(nn.Module):
    """Identity on (q, k), called only on the recording route with the fp32 in_proj outputs
    that both ops.attention and ops.attention_weights read: a forward hook on a layer's
    ``in_proj_tap`` sees exactly what a recorded map was computed from. No parameters."""

    def forward(self, q, k):
        return q, k


class TransformerCrossEncoderLayer(nn.Module):
    """transformers.py:84-258: forward_pre (pre_norm: True, the shipped configs) and
    forward_post (pre_norm: False); dropout must be 0 at inference."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation='relu',
                 normalize_before=False, sa_val_has_pos_emb=False, ca_val_has_pos_emb=False,
                 attention_type='dot_prod'):
        super().__init__()
        if attention_type != 'dot_prod':
            raise NotImplementedError(attention_type)
        # _get_activation_fn (transformers.py:265-273): relu | gelu | glu, else RuntimeError
        if activation == 'glu':
            raise NotImplementedError(
                "transformer_act 'glu': the reference's own F.glu halves the hidden width "
                '(dim_feedforward -> dim_feedforward / 2), so the reference itself fails in '
                'linear2; there is nothing to reproduce')
        if activation not in ('relu', 'gelu'):
            raise RuntimeError(f'transformer_act must be relu or gelu, not {activation!r}')
        self.activation = activation
        self.act = ops.ACT_GELU if activation == 'gelu' else ops.ACT_RELU
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.multihead_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.norm3 = nn.LayerNorm(d_model)
        self.nhead = nhead
        self.normalize_before = normalize_before
        self.sa_val_has_pos_emb = sa_val_has_pos_emb
        self.ca_val_has_pos_emb = ca_val_has_pos_emb
        # the attention maps of the last recording forward (transformers.py:116, 177-179,
        # 240-242): (src, tgt) pairs of padded (B, Nq_max, Nk_max) head-mean weights
        self.satt_weights, self.xatt_weights = None, None
        self.in_proj_tap = _QKTap()

    def _attention(self, q, k, v, seg, kv_seg, record):
        """ops.attention on fp32 q / k / v; ``record`` (a list) also receives the packed
        (N, seg.max_len) head-mean attention map of the same q / k."""
        if record is not None:
            q, k = self.in_proj_tap(q, k)
            record.append(ops.attention_weights(q, k, seg.off, seg.off, kv_seg, seg.max_len,
                                                self.nhead))
        return ops.attention(q, k, v, seg.off, seg.off, kv_seg, seg.max_len, self.nhead)

    def _attend(self, mha, h_pos, h_nopos, val_has_pos, seg, kv_seg, ln=None, side=None,
                record=None):
        """``ln`` = (x, norm, pos): h_pos = norm(x) + pos is formed inside the in_proj GEMM
        (linear_ln; val_has_pos only); ``side`` = (norm2, out2): out2 = norm2(x) as well.
        ``record`` (a list): the recording route. The launches that keep q / k / v out of fp32
        memory (ln_qkv_attention, qkv_attention) are not taken, and the attention map of the
        q / k that ops.attention reads is appended to the list."""
        W, b = mha.in_proj_weight, mha.in_proj_bias
        if ln is not None:
            x, norm, pos = ln
            d = x.shape[1]
            # the image path forms norm(x) + pos in its prologue: it needs the pos rows
            # (transformer_encoder_has_pos_emb False -> pos None -> linear_ln below)
            if (record is None and lin.MODE == 'f16x3' and ops.ATTN_MODE == 'f16x3'
                    and pos is not None and ops.ln_qkv_supported(x.shape[0], d, self.nhead)
                    and (side is None or side[0].eps == norm.eps)):
                # k / v straight into the attention's images (no fp32 k / v, no image launch)
                return ops.ln_qkv_attention(x, norm, lin.weight_image(W, mode='f16x3'), b, pos,
                                            seg.off, kv_seg, seg.max_len, self.nhead, side=side)
            qkv = linear_ln(x, norm, W, b, add=pos, side=side)        # (N, 3d): [q | k | v]
            q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
            return self._attention(q, k, v, seg, kv_seg, record)
        d = h_pos.shape[1]
        if (record is None and val_has_pos and lin.MODE == 'f16x3' and ops.ATTN_MODE == 'f16x3'
                and ops.qkv_supported(h_pos.shape[0], d, self.nhead)):
            # head dim 64: the in_proj writes the attention's K / V images itself
            return ops.qkv_attention(h_pos, lin.weight_image(W, mode='f16x3'), b, seg.off, kv_seg,
                                     seg.max_len, self.nhead)
        if (record is None and val_has_pos and lin.MODE == 'bf16' and ops.ATTN_MODE == 'bf16'
                and ops.qkv_bf16_supported(h_pos.shape[0], d, self.nhead)):
            return ops.qkv_attention(h_pos, lin.weight_image(W, mode='bf16'), b, seg.off, kv_seg,
                                     seg.max_len, self.nhead, mode='bf16')
        if val_has_pos:
            qkv = linear(h_pos, W, b)                                 # (N, 3d): [q | k | v]
            q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        else:
            qk = linear(h_pos, W, b[:2 * d], rows=(0, 2 * d))         # [q | k]
            q, k = qk[:, :d], qk[:, d:]
            v = linear(h_nopos, W, b[2 * d:], rows=(2 * d, 3 * d))
        return self._attention(q, k, v, seg, kv_seg, record)

    def _store_maps(self, packed, seg):
        """The packed self / cross maps of one recording forward -> satt_weights, xatt_weights
        in the reference's padded layout: per side (B, Nq_max, Nk_max) with a pair's valid block
        at [b, :n_q, :n_k] and zeros elsewhere. Padded query rows are zero here (the reference
        holds a padded query's softmax there; nothing can use those rows). Only the 2B clouds
        are read: the decoder's query-only phantom segments never appear."""
        B, lens = seg.B, seg.lengths
        start = [0]
        for n in lens:
            start.append(start[-1] + n)

        def padded(w, cross):
            sides = []
            for s in (0, 1):
                clouds = range(s * B, (s + 1) * B)
                keys = [(c + B) % (2 * B) if cross else c for c in clouds]
                t = w.new_zeros((B, max(lens[c] for c in clouds), max(lens[c] for c in keys)))
                for b, (c, kc) in enumerate(zip(clouds, keys)):
                    t[b, :lens[c], :lens[kc]] = w[start[c]:start[c + 1], :lens[kc]]
                sides.append(t)
            return tuple(sides)

        self.satt_weights = padded(packed[0], False)
        self.xatt_weights = padded(packed[1], True)

    def takes_side(self, x, pos):
        """True if forward_packed can also write another LayerNorm of its input x (``side``)
        from its fused norm1 -> in_proj launch."""
        n, d = x.shape
        return (self.normalize_before and self.sa_val_has_pos_emb and pos is not None
                and ln_fusable(n, 3 * d, d))

    def wants_h1(self, x):
        """True if forward_packed takes a precomputed norm1(x) + pos (``h1``): pre-norm, values
        with pos, and norm1 not folded into the in_proj GEMM."""
        n, d = x.shape
        return (self.normalize_before and self.sa_val_has_pos_emb
                and not ln_fusable(n, 3 * d, d))

    def forward_packed(self, x, pos, seg: Segments, pending_bias=None, h1=None, side=None,
                       record=False):
        """x (N_tot, d) packed clouds -> (x, pending bias) (forward_pre, transformers.py:183-244).
        ``record``: also store this layer's attention maps (satt_weights, xatt_weights).

        Every residual GEMM adds its Linear's bias and the residual in its epilogue, so each
        LayerNorm only reads x (no in-place bias pass writing x back); ``pending_bias`` (a
        bias still to be added to x by the first LayerNorm) is accepted for callers that
        defer one, and the returned pending bias is None."""
        if not self.normalize_before:
            return self._forward_post(x, pos, seg, pending_bias, record), None
        rec = [] if record else None
        n, d = x.shape
        # LayerNorm (+ pos) folded into the next GEMM where that GEMM supports it
        # (linear_ln): the norm output is never written
        fuse_in = ln_fusable(n, 3 * d, d)
        # self-attention, shared weights for src and tgt (:193-210)
        if fuse_in and self.sa_val_has_pos_emb and pending_bias is None:
            o = self._attend(self.self_attn, None, None, True, seg, seg.self_seg,
                             ln=(x, self.norm1, pos), side=side, record=rec)
            side = None
        elif h1 is not None:              # norm1(x) + pos from the previous layer's output norm
            assert pending_bias is None and self.sa_val_has_pos_emb
            o = self._attend(self.self_attn, h1, None, True, seg, seg.self_seg, record=rec)
        else:
            if side is not None:
                ops.layernorm(x, side[0].weight, side[0].bias, side[0].eps, out=side[1])
                side = None
            h = ops.layernorm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps, add=pos,
                              pre_bias=pending_bias)
            h0 = None if self.sa_val_has_pos_emb else ops.layernorm(
                x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
            o = self._attend(self.self_attn, h, h0, self.sa_val_has_pos_emb, seg, seg.self_seg,
                             record=rec)
        x = linear(o, self.self_attn.out_proj.weight, self.self_attn.out_proj.bias, residual=x)
        # cross-attention, both directions at once (:212-229)
        if fuse_in and self.ca_val_has_pos_emb:
            o = self._attend(self.multihead_attn, None, None, True, seg, seg.cross_seg,
                             ln=(x, self.norm2, pos), record=rec)
        else:
            h = ops.layernorm(x, self.norm2.weight, self.norm2.bias, self.norm2.eps, add=pos)
            h0 = None if self.ca_val_has_pos_emb else ops.layernorm(
                x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
            o = self._attend(self.multihead_attn, h, h0, self.ca_val_has_pos_emb, seg,
                             seg.cross_seg, record=rec)
        if rec is not None:
            self._store_maps(rec, seg)
        x = linear(o, self.multihead_attn.out_proj.weight, self.multihead_attn.out_proj.bias,
                   residual=x)
        # position-wise feed-forward (:231-238): one launch where supported (ops.ffn: the
        # hidden activations stay on chip), else linear_ln (or layernorm + linear) then linear
        if lin.MODE == 'f16x3' and ops.ffn_supported(n, d, self.linear1.out_features, self.act):
            return ops.ffn(x, self.norm3, lin.weight_image(self.linear1.weight, mode='f16x3'),
                           self.linear1.bias, lin.weight_image(self.linear2.weight, mode='ffn2'),
                           self.linear2.bias, self._ffn_bound(), act=self.act), None
        if self.act == ops.ACT_GELU:      # no GEMM epilogue has GELU: fp32, in place, between
            h = ops.gelu_(linear_ln(x, self.norm3, self.linear1.weight, self.linear1.bias))
        else:
            h = linear_ln(x, self.norm3, self.linear1.weight, self.linear1.bias, act=ops.ACT_RELU)
        return linear(h, self.linear2.weight, self.linear2.bias, residual=x), None

    def _ffn_bound(self):
        """{max_j ||linear1.weight[j]||_2, max_j |linear1.bias[j]|} on the device (the fused
        feed-forward kernel's hidden-value scale, ops.ffn), rebuilt when either tensor changes."""
        w, b = self.linear1.weight, self.linear1.bias
        key = (w.data_ptr(), w._version, b.data_ptr(), b._version)
        st = self.__dict__.get('_ffn_bound_cache')
        if st is None or st[0] != key:
            with torch.no_grad():
                bound = torch.stack([w.detach().norm(dim=1).max(),
                                     b.detach().abs().max()]).float().contiguous()
            st = (key, bound)
            self.__dict__['_ffn_bound_cache'] = st          # not a parameter / buffer
            ops.note_state(bound)
        return st[1]

    def _forward_post(self, x, pos, seg: Segments, pending_bias=None, record=False):
        """forward_post (transformers.py:109-181): each sub-block's residual sum is formed in
        its output GEMM's epilogue, then LayerNorm'd; the norm1 output is also written with the
        positional embedding added (the cross-attention's q / k input, :139-147). Both
        directions of each attention run in one launch, reading the same pre-update rows
        like the reference's simultaneous src / tgt update."""
        assert pending_bias is None          # only the pre-norm path defers a bias
        rec = [] if record else None
        h = ops.add(x, pos)                                       # with_pos_embed (:121-124)
        o = self._attend(self.self_attn, h, x, self.sa_val_has_pos_emb, seg, seg.self_seg,
                         record=rec)
        t = linear(o, self.self_attn.out_proj.weight, self.self_attn.out_proj.bias, residual=x)
        x = ops.layernorm(t, self.norm1.weight, self.norm1.bias, self.norm1.eps)       # :127
        h = ops.layernorm(t, self.norm1.weight, self.norm1.bias, self.norm1.eps, add=pos)
        o = self._attend(self.multihead_attn, h, x, self.ca_val_has_pos_emb, seg, seg.cross_seg,
                         record=rec)
        if rec is not None:
            self._store_maps(rec, seg)
        t = linear(o, self.multihead_attn.out_proj.weight, self.multihead_attn.out_proj.bias,
                   residual=x)
        x = ops.layernorm(t, self.norm2.weight, self.norm2.bias, self.norm2.eps)       # :163
        if self.act == ops.ACT_GELU:                                                   # :167-169
            h = ops.gelu_(linear(x, self.linear1.weight, self.linear1.bias))
        else:
            h = linear(x, self.linear1.weight, self.linear1.bias, act=ops.ACT_RELU)
        t = linear(h, self.linear2.weight, self.linear2.bias, residual=x)
        return ops.layernorm(t, self.norm3.weight, self.norm3.bias, self.norm3.eps)


class TransformerCrossEncoder(nn.Module):
    """transformers.py:18-81 with return_intermediate=True semantics.

    ``record_attention`` (default False): a forward made while it is True also stores every
    layer's head-averaged attention maps (layer.satt_weights / xatt_weights) for
    ``get_attentions``. Unlike the reference, which keeps them on every forward, recording is
    opt-in: the fast forward never forms an attention matrix, so a recording forward takes the
    route that writes fp32 q / k / v (linear / linear_ln, then ops.attention) and computes the
    maps from those q / k with a kernel of their own (ops.attention_weights, exact fp32 in
    either precision mode). Its outputs equal a plain forward's up to rounding. The maps of a
    padded query row are zero (the reference holds that padded query's softmax there)."""

    record_attention = False

    def __init__(self, cross_encoder_layer, num_layers, norm=None, return_intermediate=False):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(cross_encoder_layer) for _ in range(num_layers)])
        self.num_layers = num_layers
        self.norm = norm
        self.return_intermediate = return_intermediate

    def forward_packed(self, x, pos, seg: Segments):
        """-> (L, N_tot, d) normalised intermediates (or (1, N_tot, d))."""
        L = len(self.layers)
        n, d = x.shape
        inter = torch.empty((L if self.return_intermediate else 1, n, d), dtype=x.dtype,
                            device=x.device)
        x = x.clone()                      # the residual stream is updated in place
        pending = None
        h1 = side = None
        for l, layer in enumerate(self.layers):
            x, pending = layer.forward_packed(x, pos, seg, pending, h1=h1, side=side,
                                              record=self.record_attention)
            h1 = side = None
            if self.return_intermediate or l == L - 1:
                nxt = self.layers[l + 1] if l + 1 < L else None
                if (nxt is not None and self.norm is not None and pending is None
                        and nxt.takes_side(x, pos) and self.norm.eps == nxt.norm1.eps):
                    # this layer's output norm is written by the next layer's fused
                    # norm1 -> in_proj launch (same rows, same statistics)
                    side = (self.norm, inter[l if self.return_intermediate else 0])
                elif (nxt is not None and self.norm is not None and pending is None
                        and nxt.wants_h1(x) and self.norm.eps == nxt.norm1.eps):
                    # this layer's output norm and the next layer's norm1 (+ pos): one pass
                    _, h1 = ops.layernorm_dual(x, self.norm, nxt.norm1, add_b=pos,
                                               out_a=inter[l if self.return_intermediate else 0])
                else:
                    self._norm(x, pending, inter[l if self.return_intermediate else 0])
                pending = None
        return inter

    def get_attentions(self):
        """transformers.py:61-81: the maps of the last recording forward, stacked over the
        layers: ((src_satt, tgt_satt), (src_xatt, tgt_xatt)) of shapes (L, B, Ns, Ns),
        (L, B, Nt, Nt), (L, B, Ns, Nt), (L, B, Nt, Ns) with Ns / Nt the longest src / tgt
        cloud. Cross-attention maps are those of the rows before either side's update."""
        if any(l.satt_weights is None or l.xatt_weights is None for l in self.layers):
            raise RuntimeError('no attention maps recorded: set record_attention = True and '
                               'run a forward')
        satt = tuple(torch.stack([l.satt_weights[s] for l in self.layers]) for s in (0, 1))
        xatt = tuple(torch.stack([l.xatt_weights[s] for l in self.layers]) for s in (0, 1))
        return satt, xatt

    def _norm(self, x, pending, out):
        if self.norm is None:
            if pending is not None:
                x.add_(pending)
            out.copy_(x)
            return out
        return ops.layernorm(x, self.norm.weight, self.norm.bias, self.norm.eps,
                             pre_bias=pending, out=out)


class PositionEmbeddingCoordsSine(nn.Module):
    """position_embedding.py:8-49 on fgr_sine_pos_embed."""

    def __init__(self, n_dim=1, d_model=256, temperature=10000, scale=None):
        super().__init__()
        if n_dim != 3:
            raise NotImplementedError('coordinates are 3-D in this path')
        self.n_dim, self.d_model, self.temperature = n_dim, d_model, temperature
        self.scale = 1.0 if scale is None else scale

    def forward(self, xyz):
        return ops.sine_pos_embed(xyz, self.d_model, self.temperature, self.scale)


class PositionEmbeddingLearned(nn.Module):
    """position_embedding.py:52-71: the per-point MLP 3 -> 32 -> 64 -> 128 -> 256 -> d_model with
    ReLU between the layers (``pos_emb_type: learned``). ``self.mlp`` has the reference's layout
    (Linear at indices 0, 2, 4, 6, 8), so its state_dict keys are ``mlp.{0,2,4,6,8}.{weight,
    bias}``.

    Inference: one launch (ops.pos_mlp, fgr_pos_mlp_f16x3) where ops.pos_mlp_supported, else
    five linear() calls. The MLP always runs in f16x3, in both precision modes -- like the sine
    embedding, which is fp32 under lin.MODE == 'bf16' too: the embedding is added to every
    attention input, and at 0.1 % of the forward's products it buys nothing in bf16. Training
    (train_forward) goes through autograd.linear_t, so the ten parameters get gradients from
    the existing backward kernels. Weight images come from the linear.weight_image cache: an
    in-place update or load_state_dict invalidates them like every other layer's."""

    def __init__(self, n_dim=3, d_model=256):
        super().__init__()
        if n_dim != 3:
            raise NotImplementedError('coordinates are 3-D in this path')
        self.n_dim, self.d_model = n_dim, d_model
        self.mlp = nn.Sequential(
            nn.Linear(n_dim, 32), nn.ReLU(),
            nn.Linear(32, 64), nn.ReLU(),
            nn.Linear(64, 128), nn.ReLU(),
            nn.Linear(128, 256), nn.ReLU(),
            nn.Linear(256, d_model))

    def _linears(self):
        return [self.mlp[i] for i in (0, 2, 4, 6, 8)]

    def forward(self, xyz):
        ls = self._linears()
        with lin.mode_scope('f16x3'):
            if ops.pos_mlp_supported(xyz.shape[0], self.d_model):
                imgs = [lin.weight_image(m.weight, mode='f16x3') for m in ls[1:]]
                return ops.pos_mlp(xyz, ls[0].weight, ls[0].bias, imgs, [m.bias for m in ls[1:]])
            return self.forward_chain(xyz)

    def forward_chain(self, xyz):
        """The same MLP as five linear() launches (the path for widths the fused kernel refuses,
        and its A/B baseline)."""
        ls = self._linears()
        h = xyz.contiguous()
        with lin.mode_scope('f16x3'):
            for i, m in enumerate(ls):
                h = lin.linear(h, m.weight, m.bias, act=ops.ACT_RELU if i < 4 else ops.ACT_NONE)
        return h

    def train_forward(self, xyz):
        """Differentiable forward: five autograd.linear_t calls (f16x3)."""
        from .autograd import linear_t
        ls = self._linears()
        h = xyz.contiguous()
        with lin.mode_scope('f16x3'):
            for i, m in enumerate(ls):
                h = linear_t(h, m.weight, m.bias, act=ops.ACT_RELU if i < 4 else ops.ACT_NONE)
        return h


class SinusoidalPositionalEmbedding(nn.Module):
    """position_embedding.py:102-126: E(t) = [sin(t w_0), cos(t w_0), sin(t w_1), ...] with
    w_m = exp(-2 m ln(10000) / d_model) kept as the buffer ``div_term`` (so it is in the
    state_dict, as the reference's)."""

    def __init__(self, d_model):
        super().__init__()
        if d_model % 2 != 0:
            raise ValueError(f'Sinusoidal positional encoding with odd d_model: {d_model}')
        self.d_model = d_model
        div_indices = torch.arange(0, d_model, 2).float()
        self.register_buffer('div_term', torch.exp(div_indices * (-math.log(10000.0) / d_model)))

    def forward(self, emb_indices):
        """(*) -> (*, d_model), detached, in torch ops (the composed and training paths; the
        fused kernel builds the same rows on chip)."""
        omegas = emb_indices.reshape(-1, 1) * self.div_term.view(1, -1)
        emb = torch.stack([torch.sin(omegas), torch.cos(omegas)], dim=2)
        return emb.view(*emb_indices.shape, self.d_model).detach()


class GeometricStructureEmbedding(nn.Module):
    """position_embedding.py:129-196 (``pos_emb_type: geometric``): per point, the
    rotation-invariant embedding of its distances and angles to its ``angle_k`` nearest
    neighbours of the same cloud. With k = angle_k, D = hidden_dim and nn(i) the k nearest
    OTHER points of point i's cloud,

        d_ij  = |p_j - p_i| / sigma_d                                         j in nn(i)
        a_ijr = atan2(|(p_r - p_i) x (p_j - p_i)|, (p_r - p_i) . (p_j - p_i))
                * 180 / (sigma_a pi)                                          j, r in nn(i)
        out_i = max_j [ proj_d(E(d_ij)) + red_r proj_a(E(a_ijr)) ]

    with E the interleaved sinusoidal embedding (SinusoidalPositionalEmbedding), red = max or
    mean (``reduction_a``) and both maxima per channel; r = j stays in (angle 0), as in the
    reference. State_dict layout of the reference: ``embedding.div_term`` (buffer),
    ``proj_d.{weight,bias}``, ``proj_a.{weight,bias}``.

    The reference embeds every pair and triplet of a cloud ((1, N, N, k, D) tensors) and then
    gathers the k nearest columns; only the k (1 + k) rows per point that survive the gather are
    computed here. Two deliberate differences, which agree with the reference wherever a cloud
    has no duplicate points (grid subsampling guarantees that):

    * distances come from coordinate differences, not from x^2 - 2 x.y + y^2 in fp32 (clamped at
      0), whose cancellation error reaches the distance itself at 3DMatch scale (x^2 ~ 16,
      d^2 ~ 0.01); ours is the more accurate form;
    * the point itself is excluded by index, not by dropping the first of the k + 1 smallest;
      ties in squared distance go to the lower index.

    A cloud with n <= k points makes the reference's topk raise; forward raises ValueError from
    the host lengths before anything is launched.

    forward(xyz, cloud_off, lengths): xyz (N, 3) the packed clouds, cloud_off their device
    offsets (Segments.cloud_off), lengths the host lengths. Two launches where
    ops.geo_embed_supported (fgr_geo_embed_indices, fgr_geo_embed_f16x3), else forward_composed.
    Always f16x3, in both precision modes, like the other two embeddings. No host sync, so it
    runs inside the captured core graph. train_forward is differentiable in proj_d / proj_a."""

    def __init__(self, hidden_dim, sigma_d=0.2, sigma_a=15, angle_k=3, reduction_a='max'):
        super().__init__()
        self.sigma_d = sigma_d
        self.sigma_a = sigma_a
        self.factor_a = 180.0 / (self.sigma_a * math.pi)
        self.angle_k = angle_k
        self.hidden_dim = hidden_dim
        self.embedding = SinusoidalPositionalEmbedding(hidden_dim)
        self.proj_d = nn.Linear(hidden_dim, hidden_dim)
        self.proj_a = nn.Linear(hidden_dim, hidden_dim)
        self.reduction_a = reduction_a
        if self.reduction_a not in ['max', 'mean']:
            raise ValueError(f'Unsupported reduction mode: {self.reduction_a}.')

    def _indices(self, xyz, cloud_off, lengths):
        k = self.angle_k
        short = [int(n) for n in lengths if int(n) <= k]
        if short:
            raise ValueError(f'GeometricStructureEmbedding: a cloud of {short[0]} points has no '
                             f'{k} nearest neighbours (angle_k {k} needs more than {k} points)')
        if sum(int(n) for n in lengths) != xyz.shape[0]:
            raise ValueError('GeometricStructureEmbedding: lengths do not sum to the rows of xyz')
        with torch.no_grad():
            return ops.geo_embed_indices(xyz, cloud_off, k, self.sigma_d, self.sigma_a)

    def forward(self, xyz, cloud_off, lengths):
        k, D = self.angle_k, self.hidden_dim
        if not ops.geo_embed_supported(max(xyz.shape[0], 1), D, k):
            return self.forward_composed(xyz, cloud_off, lengths)
        _, d, a = self._indices(xyz, cloud_off, lengths)
        return ops.geo_embed(d, a, self.embedding.div_term,
                             lin.weight_image(self.proj_d.weight, mode='f16x3'), self.proj_d.bias,
                             lin.weight_image(self.proj_a.weight, mode='f16x3'), self.proj_a.bias,
                             ops.GEO_MEAN if self.reduction_a == 'mean' else ops.GEO_MAX)

    def _reduce(self, pd, pa, n):
        k, D = self.angle_k, self.hidden_dim
        pa = pa.view(n, k, k, D)
        pa = pa.max(dim=2)[0] if self.reduction_a == 'max' else pa.mean(dim=2)
        return (pd.view(n, k, D) + pa).max(dim=1)[0]

    def forward_composed(self, xyz, cloud_off, lengths):
        """The same embedding from the indices kernel, torch sin / cos, two linear() launches and
        torch reductions (the path for shapes the fused kernel refuses, and its A/B baseline)."""
        _, d, a = self._indices(xyz, cloud_off, lengths)
        with lin.mode_scope('f16x3'):
            pd = linear(self.embedding(d.reshape(-1)), self.proj_d.weight, self.proj_d.bias)
            pa = linear(self.embedding(a.reshape(-1)), self.proj_a.weight, self.proj_a.bias)
        return self._reduce(pd, pa, xyz.shape[0])

    def train_forward(self, xyz, cloud_off, lengths):
        """Differentiable forward: the indices without gradients and E detached, as in the
        reference; two autograd.linear_t calls (f16x3) and torch reductions."""
        from .autograd import linear_t
        _, d, a = self._indices(xyz, cloud_off, lengths)
        with lin.mode_scope('f16x3'):
            pd = linear_t(self.embedding(d.reshape(-1)), self.proj_d.weight, self.proj_d.bias)
            pa = linear_t(self.embedding(a.reshape(-1)), self.proj_a.weight, self.proj_a.bias)
        return self._reduce(pd, pa, xyz.shape[0])
