"""MI355X-native mirror of ``finetune_src/reverie/vlnbert_navref.py``: `ObjectEmbeddings` (:12-42) and `NavRefCMT` (:45-158).

NavRefCMT is NavCMT with a third vision segment -- the candidate objects of the current viewpoint -- and a second head that grounds
the target object.  It differs from ``models.vilmodel_cmt.NavCMT`` where the reference does:

* `language` returns ONE tensor, also under `no_lang_ca` (the x-layers then pass the text through unchanged, and every layer's
  cross attention reads that same tensor);
* `visual` encodes ``hist ⊕ ob ⊕ obj`` and returns ``(act_logits, obj_logits, txt, hist, ob, obj)`` with
  ``act_logits = next_action(ob * hist[:, :1])`` always and ``obj_logits = ref_object(obj * txt[:, :1])``, -inf where the
  object mask is False.

The object embedder is one HIP launch behind its dense layer (ops.obj_embed; csrc/obj_embed.hip).
"""
from __future__ import annotations

import torch
from torch import nn

from .. import ops, streams
from ..models.vilmodel_cmt import (BertEmbeddings, BertLayerNorm, BertPreTrainedModel, HistoryEmbeddings, ImageEmbeddings,
                                   LxmertEncoder, NextActionPrediction)
from ..modeling import precision_of

OBJ_TOKEN_TYPE = 1      # token_type_embeddings row of every object (vlnbert_navref.py:129)
OBJ_NAV_TYPE = 2        # nav_type_embedding row of every object: the STOP type (:131)


class ObjectEmbeddings(nn.Module):
    """vlnbert_navref.py:12-42: LN(LN_img(W obj) + LN_ang(W ang) + LN_pos(W pos) + nav + type) -> dropout."""

    def __init__(self, config):
        super().__init__()
        self.img_linear = nn.Linear(config.obj_feat_size, config.hidden_size)
        self.img_layer_norm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.ang_linear = nn.Linear(config.angle_feat_size, config.hidden_size)
        self.ang_layer_norm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.pos_linear = nn.Linear(5, config.hidden_size)
        self.pos_layer_norm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.layer_norm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self.prec = precision_of(config)

    def forward(self, obj_feat, obj_ang, obj_pos, type_table, nav_type_table):
        """obj_feat [B, n, obj_feat_size], obj_ang [B, n, 4] (row-strided views allowed), obj_pos [B, n, 5]; `type_table` /
        `nav_type_table` are the token-type and navigation-type embedding TABLES -- their rows 1 and 2 are added to every object
        (the reference passes those rows gathered per object)."""
        p = float(self.dropout.p) if self.training else 0.0
        if ops.obj_embed_ok(obj_feat, obj_ang, obj_pos, self, type_table, nav_type_table):
            return ops.obj_embed(obj_feat, obj_ang, obj_pos, self, type_table, nav_type_table, p, self.prec)
        B, n = obj_feat.shape[:2]
        H = self.img_linear.weight.shape[0]
        M = B * n
        a = ops.layer_norm(ops.linear(obj_feat, self.img_linear.weight, self.img_linear.bias, ops.ACT_NONE, self.prec), None, self.img_layer_norm)
        # K = 4 / 5: exact fp32 contractions
        b = ops.layer_norm(ops.linear(obj_ang, self.ang_linear.weight, self.ang_linear.bias, ops.ACT_NONE, "fp32"), None, self.ang_layer_norm)
        c = ops.layer_norm(ops.linear(obj_pos, self.pos_linear.weight, self.pos_linear.bias, ops.ACT_NONE, "fp32"), None, self.pos_layer_norm)
        e = ops.add3(a, b, c).view(M, H)
        zeros = ops.const_index("zeros", M, device=obj_feat.device)
        e = ops.gather_rows(nav_type_table[OBJ_NAV_TYPE:OBJ_NAV_TYPE + 1], zeros, base=e)
        e = ops.gather_rows(type_table[OBJ_TOKEN_TYPE:OBJ_TOKEN_TYPE + 1], zeros, base=e)
        return ops.layer_norm(e.view(B, n, H), None, self.layer_norm, p_post=p)


class NavRefCMT(BertPreTrainedModel):
    """vlnbert_navref.py:45-158: `language` (once per episode), `history` (one step), `visual` (one decision)."""
    _hamt_container = True      # (optim.AdamW.attach) direct parameter reads below are behind streams.gate

    def __init__(self, config):
        super().__init__(config)
        self.embeddings = BertEmbeddings(config)
        self.img_embeddings = ImageEmbeddings(config)
        self.obj_embeddings = ObjectEmbeddings(config)
        self.hist_embeddings = HistoryEmbeddings(config)
        self.encoder = LxmertEncoder(config)
        self.next_action = NextActionPrediction(config.hidden_size, config.pred_head_dropout_prob, precision_of(config))
        self.ref_object = NextActionPrediction(config.hidden_size, config.pred_head_dropout_prob, precision_of(config))
        self.init_weights()

    def forward(self, mode, txt_ids=None, txt_embeds=None, txt_masks=None, hist_img_feats=None, hist_ang_feats=None,
                hist_pano_img_feats=None, hist_pano_ang_feats=None, hist_embeds=None, ob_step_ids=None, hist_masks=None,
                ob_img_feats=None, ob_ang_feats=None, ob_nav_types=None, ob_masks=None,
                obj_feats=None, obj_angles=None, obj_poses=None, obj_masks=None):
        cfg = self.config
        if mode == 'language':
            txt_m = ops.extend_mask(txt_masks)
            txt = self.embeddings(txt_ids)
            for layer in self.encoder.layer:
                txt = layer(txt, txt_m)[0]
            return txt.detach() if cfg.fix_lang_embedding else txt

        if mode == 'history':
            h = self.hist_embeddings(hist_img_feats, hist_ang_feats, ob_step_ids,
                                     pano_img_feats=hist_pano_img_feats, pano_ang_feats=hist_pano_ang_feats)
            return h.detach() if cfg.fix_hist_embedding else h

        if mode == 'visual':
            hist_m = ops.extend_mask(hist_masks)
            if self.encoder.h_layers is not None:
                for layer in self.encoder.h_layers:
                    hist_embeds = layer(hist_embeds, hist_m)[0]
            ob_m = ops.extend_mask(ob_masks)
            B = ob_img_feats.size(0)
            tt_table = self.embeddings.token_type_embeddings.weight
            nav_table = self.img_embeddings.nav_type_embedding.weight
            streams.gate(tt_table, nav_table)      # (read directly here and by the object embedder)
            ones = torch.ones(B, dtype=torch.long, device=ob_img_feats.device)
            tt = ops.gather_rows(tt_table, ones).view(B, 1, -1)
            ob = self.img_embeddings(ob_img_feats, ob_ang_feats, tt, nav_types=ob_nav_types)
            if self.encoder.r_layers is not None:
                for layer in self.encoder.r_layers:
                    ob = layer(ob, ob_m)[0]
            if getattr(cfg, "fix_obs_embedding", False):
                ob = ob.detach()
            obj_m = ops.extend_mask(obj_masks)
            obj = self.obj_embeddings(obj_feats, obj_angles, obj_poses, tt_table, nav_table)
            n_hist, n_ob = hist_embeds.size(1), ob.size(1)
            vis = torch.cat([hist_embeds, ob, obj], 1)
            vis_m = torch.cat([hist_m, ob_m, obj_m], -1)
            txt_m = ops.extend_mask(txt_masks)
            for layer in self.encoder.x_layers:
                txt_embeds, vis = layer(txt_embeds, txt_m, vis, vis_m)
            hist_out = vis[:, :n_hist]
            ob_out = vis[:, n_hist:n_hist + n_ob].contiguous()
            obj_out = vis[:, n_hist + n_ob:].contiguous()
            act_logits = ops.fill_where_zero(self.next_action(ops.mul_bcast(ob_out, hist_out[:, 0])).squeeze(-1), ob_nav_types, -float('inf'))
            obj_logits = ops.fill_where_zero(self.ref_object(ops.mul_bcast(obj_out, txt_embeds[:, 0])).squeeze(-1),
                                             obj_masks.to(torch.long), -float('inf'))
            return act_logits, obj_logits, txt_embeds, hist_out, ob_out, obj_out
        raise ValueError(mode)
