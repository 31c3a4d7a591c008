"""The comparison baselines of the paper's results table on the HIP path: mRoBERTa, TomRoBERTa (TomBERT) and
EF-CapTrRoBERTa.

Constructor and `forward` signatures, attribute names and state-dict keys are the reference training scripts'
(mROBERTa/train_mroberta_vimacsa_full.py:191-288, tomROBERTa/train_tomroberta_vimacsa_full.py:187-257,
EF-CapTrRoBERTa/train_ef_captr_roberta.py:121-134), with `self.roberta` this project's RobertaModel and the torch modules of
the reference replaced by fcmf_framework.torch_layers.

`forward_aspects` is the entry the driver uses, as FCMF.forward_aspects is: the A aspect prompts of a review in one pass,
inputs [B, A, S].  What does not depend on the aspect runs once per review -- the two 2048 -> H projections of the visual
tokens and the cross-attention's key / value projections -- and the cross-attention reads them with kv_share = A (the A
prompts of a review are consecutive rows).  It equals stacking `forward` over the aspect axis.
"""
import torch
import torch.nn as nn

from . import ops
from .layers import to_compute
from .roberta import RobertaModel
from .torch_layers import MultiheadAttention, TransformerEncoder, TransformerEncoderLayer


def _per_aspect(out, B, A):
    """logits [B*A, C], or (logits, weights [B*A, Tq, Tk]), of an aspect-batched _fuse -> the same with [B, A] in front"""
    if isinstance(out, tuple):
        return tuple(t.view(B, A, *t.shape[1:]) for t in out)
    return out.view(B, A, -1)


class _Baseline(nn.Module):
    def _init_weights(self, module):
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(mean=0.0, std=0.02)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(mean=0.0, std=0.02)
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)

    def apply_custom_init(self, module):
        module.apply(self._init_weights)

    def _encode(self, ids, mask):
        """last_hidden_state of [..., S] token ids as [rows, S, H]"""
        S = ids.shape[-1]
        return self.roberta.encode(ids.reshape(-1, S), attention_mask=mask.reshape(-1, S))

    def _visual_tokens(self, visual_embeds_att, roi_embeds_att):
        """[B, N_img, 49, 2048] patches and [B, N_img, N_roi, 2048] ROIs -> [B, N_img * (49 + N_roi), H]: all patches, then all ROIs"""
        B, NI, PT, D = visual_embeds_att.shape
        NR = roi_embeds_att.shape[2]
        vis = ops.linear(to_compute(visual_embeds_att.reshape(B, NI * PT, D)), self.vis_projection.weight, self.vis_projection.bias)
        roi = ops.linear(to_compute(roi_embeds_att.reshape(B, NI * NR, D)), self.roi_projection.weight, self.roi_projection.bias)
        return torch.cat([vis, roi], dim=1)

    def _classify(self, pooled):
        pooled = ops.dropout(pooled.contiguous(), self.dropout.p, self.training)
        return ops.linear(pooled, self.classifier.weight, self.classifier.bias).float()

    def loss_aspects(self, logits, labels, weight=None, label_smoothing=0.0, focal_gamma=0.0, rdrop_alpha=0.0):
        """sum over aspects of the batch-mean cross entropy, as FCMF.loss_aspects (the same options: the aspects are the segments;
        rdrop_alpha > 0: logits [2B, A, C] of two passes, labels [B, A], + the symmetric-KL term)"""
        kl = None
        if rdrop_alpha != 0.0:
            labels, kl = ops.rdrop_pairs(logits, labels, rdrop_alpha)      # the labels repeated, the symmetric-KL term
        B, A, C = logits.shape
        if weight is None and label_smoothing == 0.0 and focal_gamma == 0.0:
            ce = ops.cross_entropy(logits.reshape(B * A, C), labels.reshape(B * A), mult=float(A))
        else:
            ce = ops.cross_entropy(logits.reshape(B * A, C), labels.reshape(B * A), weight=weight, label_smoothing=label_smoothing,
                                   focal_gamma=focal_gamma, segments=A)
        return ce if kl is None else ce + kl


class mRoBERTa(_Baseline):
    """text encoder -> the sentence tokens attend to every visual token of the review -> +residual, LayerNorm -> three
    transformer layers over the sentence -> [CLS] -> classifier"""

    def __init__(self, pretrained_path, num_labels=4):
        super().__init__()
        self.roberta = RobertaModel.from_pretrained(pretrained_path)
        config = self.roberta.config
        self.hidden_size = config.hidden_size
        self.vis_projection = nn.Linear(2048, self.hidden_size)
        self.roi_projection = nn.Linear(2048, self.hidden_size)
        self.cross_attention = MultiheadAttention(embed_dim=self.hidden_size, num_heads=config.num_attention_heads,
                                                  dropout=config.attention_probs_dropout_prob, batch_first=True)
        self.norm_cross = nn.LayerNorm(self.hidden_size)
        mm_layer = TransformerEncoderLayer(d_model=self.hidden_size, nhead=config.num_attention_heads,
                                           dim_feedforward=config.intermediate_size, dropout=config.hidden_dropout_prob,
                                           activation="gelu", batch_first=True)
        self.mm_encoder = TransformerEncoder(mm_layer, num_layers=3)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self.classifier = nn.Linear(self.hidden_size, num_labels)
        self.apply_custom_init(self.classifier)
        self.apply_custom_init(self.vis_projection)
        self.apply_custom_init(self.roi_projection)

    def _fuse(self, text_feats, visual_feats, attention_mask, kv_share, output_attentions=False):
        """-> logits; with output_attentions (logits, the cross-attention weights [rows, S, visual tokens], head mean)"""
        attn_output, weights = self.cross_attention(query=text_feats, key=visual_feats, value=visual_feats, kv_share=kv_share,
                                                    need_weights=output_attentions)
        fused_feats = ops.add_layer_norm(attn_output, text_feats, self.norm_cross.weight, self.norm_cross.bias, self.norm_cross.eps)
        mm_output = self.mm_encoder(fused_feats, src_key_padding_mask=(attention_mask == 0))
        logits = self._classify(mm_output[:, 0, :])
        return (logits, weights) if output_attentions else logits

    def forward(self, input_ids, attention_mask, visual_embeds_att, roi_embeds_att, output_attentions=False):
        """-> logits; with output_attentions (logits, cross-attention weights [B, S, visual tokens], head mean)"""
        text_feats = self._encode(input_ids, attention_mask)
        return self._fuse(text_feats, self._visual_tokens(visual_embeds_att, roi_embeds_att), attention_mask, 1, output_attentions)

    def forward_aspects(self, input_ids, attention_mask, visual_embeds_att, roi_embeds_att, output_attentions=False):
        """input_ids / attention_mask [B, A, S] -> logits [B, A, num_labels]; with output_attentions also the cross-attention
        weights [B, A, S, visual tokens] (head mean, float32): one row block per aspect prompt"""
        B, A, S = input_ids.shape
        text_feats = self._encode(input_ids, attention_mask)
        out = self._fuse(text_feats, self._visual_tokens(visual_embeds_att, roi_embeds_att), attention_mask.reshape(B * A, S), A,
                         output_attentions)
        return _per_aspect(out, B, A)


class TargetImageMatching(nn.Module):
    """the target tokens attend to the visual tokens; +residual, LayerNorm, feed-forward, +residual, LayerNorm: the tail is
    one fused autograd node (fused.PostAttentionFn)"""

    def __init__(self, hidden_size, num_heads, dropout=0.1):
        super().__init__()
        self.mha = MultiheadAttention(embed_dim=hidden_size, num_heads=num_heads, dropout=dropout, batch_first=True)
        self.norm1 = nn.LayerNorm(hidden_size)
        self.norm2 = nn.LayerNorm(hidden_size)
        self.feed_forward = nn.Sequential(nn.Linear(hidden_size, hidden_size * 4), nn.GELU(), nn.Linear(hidden_size * 4, hidden_size),
                                          nn.Dropout(dropout))
        self.dropout = nn.Dropout(dropout)

    def forward(self, target_feats, image_feats, kv_share=1, need_weights=False):
        """-> the layer's output; with need_weights (output, the target -> visual-token weights [rows, T, tokens], head mean)"""
        from .fused import PostAttentionFn
        q, k, v, mask, share = self.mha._project(target_feats, image_feats, image_feats, None, kv_share)
        c = self.mha._attend(q, k, v, mask, share)
        weights = (ops.shared_kv_attention_probs(q, k, heads=self.mha.num_heads, kv_share=share, average_heads=True)
                   if need_weights else None)
        p = float(self.dropout.p) if self.training else 0.0
        s0, s1 = (ops.next_seed(), ops.next_seed()) if p > 0 else (0, 0)
        ff = self.feed_forward
        out = PostAttentionFn.apply(c, target_feats, self.mha.out_proj.weight, self.mha.out_proj.bias, self.norm1.weight,
                                    self.norm1.bias, ff[0].weight, ff[0].bias, ff[2].weight, ff[2].bias, self.norm2.weight,
                                    self.norm2.bias, float(self.norm1.eps), p, s0, s1)
        return (out, weights) if need_weights else out


class TomBERT(_Baseline):
    """target encoder + sentence encoder (one RoBERTa) -> target-image matching -> its [CLS] in front of the sentence ->
    one transformer layer -> [visual CLS | first sentence token] -> classifier"""

    def __init__(self, pretrained_path, num_labels=4):
        super().__init__()
        self.roberta = RobertaModel.from_pretrained(pretrained_path)
        config = self.roberta.config
        self.hidden_size = config.hidden_size
        self.vis_projection = nn.Linear(2048, self.hidden_size)
        self.roi_projection = nn.Linear(2048, self.hidden_size)
        self.ti_matching = nn.ModuleList([TargetImageMatching(self.hidden_size, config.num_attention_heads,
                                                              config.attention_probs_dropout_prob) for _ in range(1)])
        encoder_layer = TransformerEncoderLayer(d_model=self.hidden_size, nhead=config.num_attention_heads,
                                                dim_feedforward=config.intermediate_size, dropout=config.hidden_dropout_prob,
                                                activation="gelu", batch_first=True)
        self.mm_encoder = TransformerEncoder(encoder_layer, num_layers=1)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self.classifier = nn.Linear(self.hidden_size * 2, num_labels)
        self.apply_custom_init(self.classifier)
        self.apply_custom_init(self.vis_projection)
        self.apply_custom_init(self.roi_projection)

    def _fuse(self, h_t, h_s, sentence_mask, g_visual, kv_share, output_attentions=False):
        """-> logits; with output_attentions (logits, the matching layer's target -> visual-token weights [rows, T, tokens])"""
        h_v, weights = h_t, None
        for layer in self.ti_matching:
            h_v = layer(target_feats=h_v, image_feats=g_visual, kv_share=kv_share, need_weights=output_attentions)
            if output_attentions:
                h_v, weights = h_v
        mm_input = torch.cat([h_v[:, 0:1, :], h_s], dim=1)
        valid_cls = torch.ones(sentence_mask.size(0), 1, dtype=sentence_mask.dtype, device=sentence_mask.device)
        mm_mask = torch.cat([valid_cls, sentence_mask], dim=1)
        h_mm = self.mm_encoder(mm_input, src_key_padding_mask=(mm_mask == 0))
        logits = self._classify(h_mm[:, 0:2, :].reshape(h_mm.shape[0], -1))      # [visual CLS | first sentence token]
        return (logits, weights) if output_attentions else logits

    def forward(self, target_ids, target_mask, sentence_ids, sentence_mask, visual_embeds_att, roi_embeds_att,
                output_attentions=False):
        """-> logits; with output_attentions (logits, target -> visual-token weights [B, T, visual tokens], head mean)"""
        h_t = self._encode(target_ids, target_mask)
        h_s = self._encode(sentence_ids, sentence_mask)
        return self._fuse(h_t, h_s, sentence_mask, self._visual_tokens(visual_embeds_att, roi_embeds_att), 1, output_attentions)

    def forward_aspects(self, target_ids, target_mask, sentence_ids, sentence_mask, visual_embeds_att, roi_embeds_att,
                        output_attentions=False):
        """target_* [B, A, T], sentence_* [B, A, S] -> logits [B, A, num_labels]; with output_attentions also the target ->
        visual-token weights [B, A, T, visual tokens] (head mean, float32)"""
        B, A, S = sentence_ids.shape
        h_t = self._encode(target_ids, target_mask)
        h_s = self._encode(sentence_ids, sentence_mask)
        out = self._fuse(h_t, h_s, sentence_mask.reshape(B * A, S), self._visual_tokens(visual_embeds_att, roi_embeds_att), A,
                         output_attentions)
        return _per_aspect(out, B, A)


class EFCapTrRoBERTa(_Baseline):
    """early fusion through captions: RoBERTa over the (review, "aspect . captions") pair -> [CLS] -> classifier"""

    def __init__(self, pretrained_path, num_labels=4):
        super().__init__()
        self.roberta = RobertaModel.from_pretrained(pretrained_path)
        config = self.roberta.config
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self.classifier = nn.Linear(config.hidden_size, num_labels)

    def forward(self, input_ids, attention_mask):
        return self._classify(self._encode(input_ids, attention_mask)[:, 0, :])

    def forward_aspects(self, input_ids, attention_mask):
        """input_ids / attention_mask [B, A, S] -> logits [B, A, num_labels]"""
        B, A, _ = input_ids.shape
        return self.forward(input_ids, attention_mask).view(B, A, -1)
