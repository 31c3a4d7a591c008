"""fcmf_crop_resize_normalize (fcmf_framework.image_ops.crop_batch) against review_batches.to_crop on the CPU: torch's
antialiased bilinear resize of the float values, round half to even, clamp, / 255, ImageNet mean / std.

Bounds: every element within one uint8 level of the normalised output (1 / (255 * 0.224) + 1e-5: a float-rounding difference
of the filter sum that lands on the other side of a .5 moves the rounded value by one level), and >= 99.5 % of the elements
within 1e-5.  bf16 output is compared with the float32 reference rounded to bf16."""
import numpy as np
import pytest
import torch

import review_batches as RB

pytestmark = pytest.mark.gpu

LEVEL = 1.0 / (255 * 0.224) + 1e-5


def _photo(h, w, seed):
    """a smooth uint8 photo with texture: [3, h, w]"""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0, 1, h).view(1, h, 1)
    xx = torch.linspace(0, 1, w).view(1, 1, w)
    base = 127 + 90 * torch.sin(6 * yy + 4 * xx + torch.tensor([0.0, 1.0, 2.0]).view(3, 1, 1))
    return (base + 40 * torch.rand(3, h, w, generator=g)).clamp(0, 255).to(torch.uint8)


def _ref(photo, box, size, flip):
    x1, x2, y1, y2 = box if box is not None else (0, photo.shape[1], 0, photo.shape[2])
    out = RB.to_crop(photo[:, x1:x2, y1:y2], size)
    return out.flip(-1) if flip else out


def _check(got, ref, dtype):
    got = got.float().cpu()
    if dtype == torch.bfloat16:
        ref = ref.to(torch.bfloat16).float()
        tol_all, tol_most = LEVEL + 2e-2, 1e-5 + 2 ** -8 * ref.abs().max().item()
    else:
        tol_all, tol_most = LEVEL, 1e-5
    err = (got - ref).abs()
    assert torch.isfinite(got).all()
    assert err.max().item() <= tol_all, err.max().item()
    frac = (err <= tol_most).float().mean().item()
    assert frac >= 0.995, frac
    return err.max().item(), frac


CASES = [      # name, photo sizes, boxes per photo (None = whole), size
    ("downscale_non_integer", [(517, 389)], None, 224),
    ("downscale_big", [(1200, 901)], None, 224),
    ("upscale", [(97, 150)], None, 224),
    ("one_pixel_wide", [(300, 40)], [[(10, 250, 7, 8)]], 224),
    ("one_pixel_tall", [(40, 300)], [[(5, 6, 0, 300)]], 224),
    ("extreme_aspect", [(1000, 23)], None, 224),
    ("roi_clipped_ends", [(360, 480)], [[(100, 900, 50, 700), (0, 30, 470, 5000), (350, 361, 0, 480)]], 224),
    ("mixed_batch", [(517, 389), (97, 150), (1200, 300), (224, 224)], [None, [(3, 50, 4, 97)], None, [(0, 224, 0, 224)]], 224),
    ("other_size", [(300, 200)], None, 64),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_crop_batch_matches_to_crop(dev, case, layout, dtype):
    from fcmf_framework.image_ops import crop_batch
    name, sizes, boxes, S = case
    photos = [_photo(h, w, 10 + i) for i, (h, w) in enumerate(sizes)]
    crops = [(p, b) for i, p in enumerate(photos) for b in ((boxes[i] if boxes else None) or [None])]
    flips = [k % 2 == 1 for k in range(len(crops))]
    src = photos if layout == "chw" else [p.permute(1, 2, 0).contiguous().numpy() for p in photos]
    out = crop_batch(src, boxes, size=S, flip=flips, dtype=dtype)
    torch.cuda.synchronize()
    assert out.shape == (len(crops), 3, S, S) and out.dtype == dtype and out.is_contiguous()
    ref = torch.stack([_ref(p, b, S, f) for (p, b), f in zip(crops, flips)])
    e, frac = _check(out, ref, dtype)
    print(f"MEASURED crop {name} {layout} {dtype}: max {e:.3e}, within 1e-5 {frac:.5f}")


def test_flip_off_and_on_are_mirror_images(dev):
    from fcmf_framework.image_ops import crop_batch
    p = _photo(333, 257, 3)
    a = crop_batch([p, p], [[(10, 300, 20, 250)], [(10, 300, 20, 250)]], flip=[False, True])
    assert torch.equal(a[0].flip(-1), a[1])
    b = crop_batch([p], flip=torch.Generator().manual_seed(0))
    assert b.shape == (1, 3, 224, 224)


def test_two_runs_are_bitwise_identical(dev):
    from fcmf_framework.image_ops import crop_batch
    photos = [_photo(517, 389, 1), _photo(97, 150, 2).permute(1, 2, 0).contiguous().numpy()]
    a = crop_batch(photos[:1], dtype=torch.float32)
    b = crop_batch(photos[:1], dtype=torch.float32)
    assert torch.equal(a, b)
    c = crop_batch([photos[1]], [[(1, 90, 2, 140)]], dtype=torch.bfloat16)
    d = crop_batch([photos[1]], [[(1, 90, 2, 140)]], dtype=torch.bfloat16)
    assert torch.equal(c, d)


@pytest.mark.parametrize("box", [(-1, 10, 0, 10), (0, 10, -3, 10), (5, 5, 0, 10), (0, 10, 40, 50), (50, 60, 0, 10)])
def test_bad_crops_raise_before_any_launch(dev, box, monkeypatch):
    from fcmf_framework import _hip as H
    from fcmf_framework.image_ops import crop_batch
    calls = []
    lib = H.lib()
    real = lib.fcmf_crop_resize_normalize

    class Spy:
        def __getattr__(self, k):
            return getattr(lib, k)

        def fcmf_crop_resize_normalize(self, *a):
            calls.append(a)
            return real(*a)
    monkeypatch.setattr(H, "lib", lambda: Spy())
    with pytest.raises(H.HipLibraryError):
        crop_batch([_photo(40, 30, 5)], [[box]])
    assert calls == []
    crop_batch([_photo(40, 30, 5)], [[(0, 10, 0, 10)]])
    assert len(calls) == 1
