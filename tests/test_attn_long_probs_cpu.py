"""CPU-side checks of the long-key probability kernel's C-ABI boundary and of the Python surface that goes with it: the symbol
is declared, exported and bound with as many arguments as the header gives it, the ABI version stands, the fusion-map switch is
off by default, and MultiheadAttention.forward carries torch's need_weights / average_attn_weights arguments."""
import ctypes
import inspect
import os
import re

from conftest import PKG, ROOT

NAME = "fcmf_attn_mfma_long_probs"


def _header():
    src = open(os.path.join(ROOT, "include", "fcmf_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_symbol_declared_exported_and_bound():
    from fcmf_framework import _hip
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, _header())
    assert m, f"{NAME} is not declared in include/fcmf_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    lib = ctypes.CDLL(os.path.join(PKG, "fcmf_framework", "libfcmf_hip.so"))
    assert hasattr(lib, NAME), f"{NAME} is not exported by libfcmf_hip.so"
    assert NAME in _hip.SIGNATURES
    assert len(_hip.SIGNATURES[NAME]) == len(params) == 14
    # pointers, then the int geometry, the two int64 row strides, the float scale, the mode and the stream, as the header orders them
    kinds = {"*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
    want = [kinds["*"] if "*" in p else kinds[p.split()[0]] for p in params]
    assert _hip.SIGNATURES[NAME] == want
    assert _hip.lib().fcmf_abi_version() == 4


def test_fusion_attention_switch_is_off_by_default_and_round_trips():
    from fcmf_framework import ops
    assert ops.output_fusion_attentions() is False
    assert ops.output_attentions() is False
    try:
        ops.set_output_fusion_attentions(True)
        assert ops.output_fusion_attentions() is True
        assert ops.output_attentions() is False          # separate from the text encoder's switch
        ops.set_output_fusion_attentions(0)
        assert ops.output_fusion_attentions() is False
    finally:
        ops.set_output_fusion_attentions(False)


def test_multihead_attention_forward_signature():
    from fcmf_framework.torch_layers import MultiheadAttention
    p = inspect.signature(MultiheadAttention.forward).parameters
    assert p["need_weights"].default is False and p["average_attn_weights"].default is True
    assert p["attn_mask"].default is None and p["kv_share"].default is None and p["key_padding_mask"].default is None
    assert callable(getattr(__import__("fcmf_framework.ops", fromlist=["ops"]), "shared_kv_attention_probs"))


def test_baselines_take_output_attentions():
    from fcmf_framework import baselines
    for cls in (baselines.mRoBERTa, baselines.TomBERT):
        for fn in (cls.forward, cls.forward_aspects):
            assert inspect.signature(fn).parameters["output_attentions"].default is False


def test_driver_parses_dump_attention_maps_and_every_reference_flag():
    import run_multimodal_fcmf as drv
    base = ["--output_dir", "o", "--pretrained_hf_model", "m"]
    assert drv.build_parser().parse_args(base).dump_attention_maps is False
    args = drv.build_parser().parse_args(base + ["--dump_attention_maps", "--do_eval", "--num_imgs", "7", "--num_rois", "4", "--fp16",
                                                 "--ddp", "--local_rank", "0", "--fine_tune_cnn", "--alpha", "0.7"])
    assert args.dump_attention_maps is True and args.do_eval and args.num_rois == 4
