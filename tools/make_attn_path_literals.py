"""Print the DESC / PTRS literals of tests/test_attn_path_cpu.py (CPU tensors only, no GPU):
    python tools/make_attn_path_literals.py
The committed literals were printed at the commit before fcmf_framework/attn.py existed, where the builders were ops._desc and
fused._qkv_desc (both asked for the fused cases, and they agreed); from then on this prints what attn.desc and fused give."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multimodal-aspect-category-sentiment-analysis_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_attn_path_cpu as T                                    # noqa: E402
from fcmf_framework import fused, ops                             # noqa: E402

desc = ops._desc if hasattr(ops, "_desc") else T.attn.desc
got = {name: T.fields(desc(*T._case(name))) for name in T.CASES}
for name, dtype in T.FUSED_CASES.items():
    qkv, mask, G, Tn, Hd, heads, p, seed = T._fused_case(dtype)
    if hasattr(fused, "_qkv_desc"):
        got[name] = T.fields(fused._qkv_desc(qkv, G, Tn, Hd, heads, mask, 1.0 / 8, p, seed))
        x = qkv.view(G, Tn, 3 * Hd)
        assert got[name] == T.fields(desc(x[:, :, :Hd], x[:, :, Hd:2 * Hd], x[:, :, 2 * Hd:], None, None, mask, None, heads, 1,
                                          1.0 / 8, p, seed, False, 0))
    else:
        got[name] = T.fields(fused._self_desc(qkv, mask, G, Tn, Hd, heads, p, seed))
for i, title in enumerate(("DESC", "PTRS")):
    print(title + " = {")
    for name, f in got.items():
        print(f'    "{name}": {f[i]},')
    print("}")
