"""Write tests/golden/iaog_attention_weights.npz: what the REFERENCE IAOG `Attention` (fcmf_framework/mm_modeling.py of
sonbui25/Multimodal-Aspect-Category-Sentiment-Analysis) returns as (output, score) for seeded weights and inputs.

    python tools/make_attn_probs_golden.py --reference /path/to/reference/checkout

The class is imported from the reference checkout (by file path: the product's own fcmf_framework package never shadows it);
nothing of it is copied here.  The fixture holds arrays only:
  w_kx, w_qx [4, 32, 8], proj_w [32, 32], proj_b [32]               n_head = 4, embed = 32, hidden = 8
  <case>_k, <case>_q, <case>_score, <case>_output  (float32)        case = B{1,2,3}_{self,cross,cross_tril}
    self       k = q [B, 5, 32], 2-D memory_len (the tril rule)
    cross      k [B, 7, 32], q [B, 5, 32], memory_len = None
    cross_tril the same shapes with a 2-D memory_len
B = 2 shares a factor with the 4 heads (several output slots read one head), B = 3 is coprime to it.
tests/test_attn_probs_cpu.py guards the fixture against a float64 restatement of the slot -> head rule."""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NH, E, HID, QL, KL = 4, 32, 8, 5, 7


def reference_attention(ref_dir):
    path = os.path.join(ref_dir, "fcmf_framework", "mm_modeling.py")
    spec = importlib.util.spec_from_file_location("reference_mm_modeling", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Attention


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "iaog_attention_weights.npz"))
    args = ap.parse_args()
    Attention = reference_attention(args.reference)
    g = torch.Generator().manual_seed(20261017)
    att = Attention(E, HID, NH, "scaled_dot_product", 0.1).eval()
    with torch.no_grad():
        att.w_kx.copy_(torch.randn(NH, E, HID, generator=g) * 0.3)
        att.w_qx.copy_(torch.randn(NH, E, HID, generator=g) * 0.3)
        att.proj.weight.copy_(torch.randn(E, NH * HID, generator=g) * 0.2)
        att.proj.bias.copy_(torch.randn(E, generator=g) * 0.1)
    out = dict(w_kx=att.w_kx, w_qx=att.w_qx, proj_w=att.proj.weight, proj_b=att.proj.bias)
    for B in (1, 2, 3):
        x = torch.randn(B, QL, E, generator=g)
        k = torch.randn(B, KL, E, generator=g)
        q = torch.randn(B, QL, E, generator=g)
        tril_self = torch.arange(1, QL + 1).repeat(B, 1)       # any 2-D memory_len selects the tril rule
        tril_cross = torch.ones(B, KL, dtype=torch.int64)
        for name, kk, qq, ml in (("self", x, x, tril_self), ("cross", k, q, None), ("cross_tril", k, q, tril_cross)):
            with torch.no_grad():
                output, score = att(kk, qq, ml)
            assert score.shape == (NH * B, QL, kk.shape[1]) and output.shape == (B, QL, E)
            assert att.attention_weights is score
            for key, v in (("k", kk), ("q", qq), ("score", score), ("output", output)):
                out[f"B{B}_{name}_{key}"] = v
    np.savez(args.out, **{k: v.detach().float().numpy() for k, v in out.items()})
    print("wrote", args.out, os.path.getsize(args.out), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
