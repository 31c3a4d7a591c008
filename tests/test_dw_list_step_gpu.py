"""One training step of a small FCMF with the weight gradients flushed as ONE list (ops.deferred_dw -> fcmf_gemm_dw_list) against
the same step with the queue switched off (FCMF_DEFER_DW=0): every parameter's gradient, the mm layer's weights with their several
uses included, with and without a flush of an arena range in the middle of the backward pass."""
import pytest
import torch

from helpers import batch_to, build_fcmf
import synthetic_data as synth

pytestmark = pytest.mark.gpu

# the batch geometry of tests/golden/fcmf_tiny.npz (B 3, S 16, 2 images, 5 ROIs); hidden sizes from 256 up, so that the weight
# gradients are matrices the 256 x 256 tile kernel takes (the tiny fixture's 64 x 64 ones would all run as separate GEMMs)
CFG = dict(synth.TINY_CFG, hidden_size=256, intermediate_size=512)
B, S, NI, NR = 3, 16, 2, 5


def test_list_gradients_equal_immediate_ones(dev):
    from fcmf_framework import ops
    from fcmf_framework.dp import GradArena
    model, _ = build_fcmf(CFG, NI, NR, dev)
    model.eval()
    b = batch_to(synth.synth_batch(B, CFG, S=S, num_imgs=NI, num_roi=NR, seed=42), dev)
    old_arena, old_dtype = ops.grad_arena(), ops.compute_dtype()
    try:
        ops.set_compute_dtype(torch.bfloat16)
        ops.shadows.clear()
        arena = GradArena.for_model(model)
        grads, queued = {}, {}
        for mode in ("off", "list", "list+range-flush"):
            ops.DEFER_DW = mode != "off"
            arena.zero()
            before = (ops.deferred_dw.batched_launches, ops.deferred_dw.batched_matrices)
            seen = []
            push = ops.deferred_dw.push
            ops.deferred_dw.push = lambda *a, **k: (seen.append(a[2].data_ptr()), push(*a, **k))[1]
            try:
                out = model.forward_aspects(b["input_ids"], b["visual_embeds_att"], b["roi_embeds_att"], b["roi_coors"], b["token_type_ids"],
                                            b["attention_mask"], b["added_attention_mask"])
                loss = model.loss_aspects(out, b["labels"])
                hooks = []
                if mode == "list+range-flush":
                    # what a data-parallel bucket group does before it is sent: flush the gradients of ITS range of the arena
                    lo = arena.flat.data_ptr()
                    hi = lo + arena.flat.numel() * 2        # (the first half of the float32 arena)
                    hooks = [p.register_post_accumulate_grad_hook(lambda p: ops.flush_deferred_dw(lo, hi)) for p in list(model.parameters())[-30::5]]
                loss.backward()
                for h in hooks:
                    h.remove()
            finally:
                ops.deferred_dw.push = push
            assert not ops.deferred_dw.q and not ops.deferred_dw.armed
            queued[mode] = seen
            launches = ops.deferred_dw.batched_launches - before[0]
            if mode == "off":
                assert launches == 0
            elif mode == "list":
                assert launches == 1, launches            # the whole queue: one list
                assert ops.deferred_dw.batched_matrices - before[1] == len(seen)
            else:
                assert launches >= 2, launches
            grads[mode] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        # the mm layer's weights are applied to the text rows, the ROIs and the fusion layer: several producers of one destination wait
        # in the queue together
        assert len(queued["list"]) > len(set(queued["list"])), "no destination had several queued producers"
        ref = grads["off"]
        assert ref and all(torch.isfinite(g).all() for g in ref.values())
        for mode in ("list", "list+range-flush"):
            assert grads[mode].keys() == ref.keys()
            for n, r in ref.items():
                d = (grads[mode][n] - r).norm().item()
                assert d <= 1e-5 * r.norm().item() + 1e-12, (mode, n, d, r.norm().item())
    finally:
        ops.DEFER_DW = True
        if "arena" in locals():
            arena.deactivate()
        ops.set_grad_arena(old_arena)
        ops.set_compute_dtype(old_dtype)
        ops.shadows.clear()
        model.zero_grad(set_to_none=True)
