"""Photo / ROI crops -> normalised trunk input on the MI355X (`fcmf_crop_resize_normalize`, csrc/image.hip).

The category classifiers (image_processing/run_image_categories.py, run_roi_categories.py) turn every photo or ROI crop into a
224 x 224 normalised tensor: v2.Resize((224, 224), antialias=True) -> RandomHorizontalFlip -> ConvertImageDtype -> Normalize
(reference image_processing/run_image_categories.py:35-41, run_roi_categories.py:34-45).  `crop_batch` computes what
`review_batches.to_crop` computes on the host, for a whole batch in one launch:
  * the decoded uint8 photos are copied once into a pinned staging buffer (a ring of reusable buffers, as device_prefetch.py
    keeps them) together with the crop descriptors, and uploaded in ONE copy on a dedicated stream;
  * the crops are described, not copied: six ROIs of one photo read the same uploaded bytes;
  * HWC photos (PIL / numpy) and CHW photos (torchvision tensors) are both read in place through their strides.
"""
import ctypes

import numpy as np
import torch

from . import _hip as H

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
_DESC = ctypes.sizeof(H.CropDesc)


class _Staging:
    """pinned upload buffers, reused round-robin once the copy that last read a buffer has finished"""

    def __init__(self, depth=3):
        self.depth, self.bufs, self.events, self.pos = depth, [], [], 0
        self.streams = {}

    def copy_stream(self, device):
        s = self.streams.get(device)
        if s is None:
            s = self.streams[device] = torch.cuda.Stream(device=device)
        return s

    def take(self, nbytes):
        i = self.pos % self.depth
        self.pos += 1
        while len(self.bufs) <= i:
            self.bufs.append(None)
            self.events.append(None)
        if self.events[i] is not None:
            self.events[i].synchronize()
        if self.bufs[i] is None or self.bufs[i].numel() < nbytes:
            self.bufs[i] = torch.empty(max(nbytes, 1 << 20) * 5 // 4, dtype=torch.uint8).pin_memory()
        return i, self.bufs[i]


_staging = _Staging()


def _as_u8(photo, hwc):
    """-> (contiguous uint8 numpy array, (sC, sH, sW), H, W)"""
    if torch.is_tensor(photo):
        if photo.is_cuda:
            raise H.HipLibraryError("crop_batch takes decoded photos in host memory")
        hwc = False if hwc is None else hwc
        a = photo.contiguous().numpy()
    else:
        hwc = True if hwc is None else hwc
        a = np.ascontiguousarray(photo)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2 if hwc else 0] != 3:
        raise H.HipLibraryError(f"crop_batch: expected uint8 {'[H, W, 3]' if hwc else '[3, H, W]'} photos, got {a.dtype} {a.shape}")
    if hwc:
        Hh, Ww = a.shape[0], a.shape[1]
        return a, (1, 3 * Ww, 3), Hh, Ww
    Hh, Ww = a.shape[1], a.shape[2]
    return a, (Hh * Ww, Ww, 1), Hh, Ww


def crop_batch(photos, boxes=None, size=224, flip=None, dtype=torch.float32, hwc=None, device=None):
    """photos: uint8 photos of any size -- torch tensors [3, H, W] (torchvision.io), numpy arrays [H, W, 3] (PIL); `hwc`
    overrides that guess.  boxes: None (each photo whole) or one entry per photo: None (whole) or a list of
    (x1, x2, y1, y2) crop boxes, meaning photo[:, x1:x2, y1:y2] (x = rows, ends clipped as a slice).
    flip: None / False (no flip), True (all), one bool per output crop, or a torch.Generator (a fair coin per crop).
    -> [n_crops, 3, size, size] contiguous `dtype` (float32 / bfloat16) on `device` (default: the current GPU), photo-major."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dtype not in (torch.float32, torch.bfloat16):
        raise H.HipLibraryError(f"crop_batch: float32 or bfloat16 output, not {dtype}")
    if boxes is not None and len(boxes) != len(photos):
        raise H.HipLibraryError("crop_batch: one boxes entry per photo")
    arrs, descs, offset, max_rows, seen = [], [], 0, 1, {}
    for i, ph in enumerate(photos):
        if id(ph) in seen:                       # the same photo object again (one entry per ROI): uploaded once
            base, (sC, sH, sW), Hh, Ww = seen[id(ph)]
        else:
            a, (sC, sH, sW), Hh, Ww = _as_u8(ph, hwc)
            base = offset
            arrs.append((base, a))
            seen[id(ph)] = (base, (sC, sH, sW), Hh, Ww)
            offset += (a.nbytes + 255) // 256 * 256
        bl = None if boxes is None else boxes[i]
        for (x1, x2, y1, y2) in ([(0, Hh, 0, Ww)] if bl is None else bl):
            x1, x2, y1, y2 = int(x1), int(x2), int(y1), int(y2)
            if min(x1, x2, y1, y2) < 0:
                raise H.HipLibraryError(f"crop_batch: negative crop bound ({x1}, {x2}, {y1}, {y2}) of photo {i}")
            hc, wc = min(x2, Hh) - x1, min(y2, Ww) - y1
            if hc <= 0 or wc <= 0:
                raise H.HipLibraryError(f"crop_batch: empty crop ({x1}, {x2}, {y1}, {y2}) of photo {i} ({Hh} x {Ww})")
            max_rows = max(max_rows, hc)
            descs.append(H.CropDesc(base, Hh, Ww, sC, sH, sW, x1, x2, y1, y2, 0, 0))
    n = len(descs)
    if n == 0:
        return torch.empty((0, 3, size, size), dtype=dtype, device=device)
    if isinstance(flip, torch.Generator):
        flips = (torch.rand(n, generator=flip) < 0.5).tolist()
    elif flip is None or isinstance(flip, bool):
        flips = [bool(flip)] * n
    else:
        flips = [bool(f) for f in flip]
        if len(flips) != n:
            raise H.HipLibraryError(f"crop_batch: {len(flips)} flip flags for {n} crops")
    for d, f in zip(descs, flips):
        d.flip = int(f)
    src_bytes = offset
    total = src_bytes + n * _DESC
    # host: photos and descriptors into one pinned buffer
    slot, buf = _staging.take(total)
    host = buf.numpy()
    for off, a in arrs:
        host[off:off + a.nbytes] = a.reshape(-1)
    host[src_bytes:total] = np.frombuffer(bytes((H.CropDesc * n)(*descs)), dtype=np.uint8)
    # one upload on the copy stream; the compute stream waits for it
    cs = _staging.copy_stream(device)
    with torch.cuda.stream(cs):
        dbuf = torch.empty(total, dtype=torch.uint8, device=device)
        dbuf.copy_(buf[:total], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(cs)
    _staging.events[slot] = ev
    cur = torch.cuda.current_stream(device)
    cur.wait_event(ev)
    dbuf.record_stream(cur)
    with torch.cuda.device(device):
        scratch = torch.empty(n * 3 * max_rows * size, dtype=torch.float32, device=device)
        out = torch.empty((n, 3, size, size), dtype=dtype, device=device)
        mean = (ctypes.c_float * 3)(*IMAGENET_MEAN)
        std = (ctypes.c_float * 3)(*IMAGENET_STD)
        H.check(H.lib().fcmf_crop_resize_normalize(H.ptr(dbuf), src_bytes, dbuf.data_ptr() + src_bytes, n, max_rows, size, mean, std,
                                                   H.ptr(scratch), scratch.numel() * 4, H.ptr(out), H.dt(out), H.stream()),
                "fcmf_crop_resize_normalize")
    return out
