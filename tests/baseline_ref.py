"""The comparison baselines after their text encoder, written with torch's own nn.MultiheadAttention / nn.TransformerEncoder as
the published training scripts write them: the CPU restatement that tests/test_baselines_*.py compare the product with."""
import torch
import torch.nn as nn

CFG = dict(vocab_size=512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
           max_position_embeddings=64, type_vocab_size=1, pad_token_id=1, layer_norm_eps=1e-5, hidden_dropout_prob=0.1,
           attention_probs_dropout_prob=0.1)


def _torch_encoder(layers):
    layer = nn.TransformerEncoderLayer(d_model=CFG["hidden_size"], nhead=CFG["num_attention_heads"],
                                       dim_feedforward=CFG["intermediate_size"], dropout=0.1, activation="gelu", batch_first=True)
    return nn.TransformerEncoder(layer, num_layers=layers, enable_nested_tensor=False)


class RefM(nn.Module):
    """mRoBERTa after the text encoder, with torch's modules"""

    def __init__(self):
        super().__init__()
        H = CFG["hidden_size"]
        self.vis_projection, self.roi_projection = nn.Linear(2048, H), nn.Linear(2048, H)
        self.cross_attention = nn.MultiheadAttention(H, CFG["num_attention_heads"], dropout=0.1, batch_first=True)
        self.norm_cross = nn.LayerNorm(H)
        self.mm_encoder = _torch_encoder(3)
        self.classifier = nn.Linear(H, 4)

    def visual(self, vis, roi):
        b = vis.shape[0]
        return torch.cat([self.vis_projection(vis.reshape(b, -1, 2048)), self.roi_projection(roi.reshape(b, -1, 2048))], 1)

    def forward(self, text, mask, vis, roi):
        v = self.visual(vis, roi)
        a, _ = self.cross_attention(query=text, key=v, value=v)
        h = self.mm_encoder(self.norm_cross(text + a), src_key_padding_mask=(mask == 0))
        return self.classifier(h[:, 0, :])


class RefTIM(nn.Module):
    def __init__(self):
        super().__init__()
        H = CFG["hidden_size"]
        self.mha = nn.MultiheadAttention(H, CFG["num_attention_heads"], dropout=0.1, batch_first=True)
        self.norm1, self.norm2 = nn.LayerNorm(H), nn.LayerNorm(H)
        self.feed_forward = nn.Sequential(nn.Linear(H, 4 * H), nn.GELU(), nn.Linear(4 * H, H), nn.Dropout(0.1))

    def forward(self, t, v):
        a, _ = self.mha(query=t, key=v, value=v)
        h = self.norm1(t + a)
        return self.norm2(h + self.feed_forward(h))


class RefT(RefM):
    """TomBERT after the two text encodings"""

    def __init__(self):
        nn.Module.__init__(self)
        H = CFG["hidden_size"]
        self.vis_projection, self.roi_projection = nn.Linear(2048, H), nn.Linear(2048, H)
        self.ti_matching = nn.ModuleList([RefTIM()])
        self.mm_encoder = _torch_encoder(1)
        self.classifier = nn.Linear(2 * H, 4)

    def forward(self, h_t, h_s, smask, vis, roi):
        h_v = self.ti_matching[0](h_t, self.visual(vis, roi))
        x = torch.cat([h_v[:, 0:1], h_s], 1)
        m = torch.cat([torch.ones(smask.shape[0], 1, dtype=smask.dtype), smask], 1)
        h = self.mm_encoder(x, src_key_padding_mask=(m == 0))
        return self.classifier(torch.cat([h[:, 0], h[:, 1]], 1))


# ---- what tools/make_baseline_golden.py and tests/test_baselines_golden_gpu.py must agree on: seeded inputs and weights -------
FIX_B, FIX_A, FIX_S, FIX_T = 3, 3, 40, 16


def fixture_batch(NI, NR, seed=1):
    """-> sentence ids / mask [B, A, S] with different pad lengths, target ids / mask [B, A, 16], patches [B, NI, 49, 2048],
    ROIs [B, NI, NR, 2048], labels [B, A]"""
    g = torch.Generator().manual_seed(seed)
    B, A, S, T = FIX_B, FIX_A, FIX_S, FIX_T
    ids = torch.randint(3, CFG["vocab_size"], (B, A, S), generator=g)
    lens = torch.tensor([[40, 33, 21], [17, 40, 9], [28, 12, 40]])
    mask = (torch.arange(S)[None, None, :] < lens[..., None]).long()
    ids = torch.where(mask.bool(), ids, torch.full_like(ids, CFG["pad_token_id"]))
    tids = torch.randint(3, CFG["vocab_size"], (B, A, T), generator=g)
    tmask = (torch.arange(T)[None, None, :] < torch.randint(2, T + 1, (B, A, 1), generator=g)).long()
    tids = torch.where(tmask.bool(), tids, torch.full_like(tids, CFG["pad_token_id"]))
    vis = torch.randn(B, NI, 49, 2048, generator=g) * 0.5
    roi = torch.randn(B, NI, NR, 2048, generator=g) * 0.5
    labels = torch.randint(0, 4, (B, A), generator=g)
    return ids, mask, tids, tmask, vis, roi, labels


def seeded_state(shapes, seed=0):
    """name -> shape (floating parameters) -> name -> float32 tensor: N(0, 0.05), LayerNorm scales 1 + N(0, 0.1); one generator
    per name, so the values do not depend on the order or on which other names are present"""
    import zlib
    out = {}
    for n, shape in shapes.items():
        g = torch.Generator().manual_seed(seed * 1000003 + zlib.crc32(n.encode()))
        x = torch.randn(tuple(shape), generator=g)
        scale_of_norm = n.endswith("weight") and ("LayerNorm" in n or "norm" in n.split(".")[-2])
        out[n] = 1 + 0.1 * x if scale_of_norm else 0.05 * x
    return out
