"""Pillow's antialiased resize on the device (csrc/resample.hip): raw RGB images of differing sizes -> one
batch, bit-identical to `Image.fromarray(im).resize(size, Image.BILINEAR)` (+ ToTensor + Normalize), in three launches for
any number of images and without a host read.

    batch = pil_resize([im0, im1], (448, 448))                                   # uint8 [2, 448, 448, 3] on the device
    x = pil_resize([im0, im1], 448, normalize=(blob.MEAN, blob.STD))             # fp32  [2, 3, 448, 448]

Images are NumPy arrays (host: uploaded as ONE pinned, non-blocking copy) or device tensors; a CPU torch tensor is an error, and
so is a machine without a GPU (no CPU fallback).  A source with h > 100 w is refused: Pillow resizes those in another pass order."""
import ctypes

import numpy as np
import torch

from . import _lib

def _size(size):
    """Pillow's `size`: (width, height); one integer means a square."""
    if isinstance(size, (int, np.integer)):
        return int(size), int(size)
    if len(size) != 2:
        raise ValueError("cim_amd.resample: size must be (width, height) or one integer, got %r" % (size,))
    return int(size[0]), int(size[1])


def ksize(n_in, n_out):
    """Entries of one row of the coefficient table of an axis n_in -> n_out (include/cim_hip.h)."""
    return int(np.ceil(max(float(n_in) / float(n_out), 1.0))) * 2 + 1


class _Batch(object):
    """The descriptor, workspace and (from `gather`) source bytes of one call, owned by name until its results exist (the kernels
    run asynchronously and the uploads do not block)."""

    def __init__(self, sizes, out_w, out_h, device, what):
        if not torch.cuda.is_available():
            raise _lib.CimHipError("%s: no GPU (there is no CPU fallback)" % what)
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if device.type != "cuda":
            raise _lib.CimHipError("%s: device %s (no CPU fallback)" % (what, device))
        desc, total = [], 0
        for h, w in sizes:
            desc += [total, int(h), int(w)]
            total += int(h) * int(w) * 3
        self.b, self.device, self.nbytes = len(desc) // 3, device, total
        self.sizes = [(desc[3 * i + 1], desc[3 * i + 2]) for i in range(self.b)]
        self.offsets = desc[0::3]
        self.desc_host = np.ascontiguousarray(np.array(desc, dtype=np.int64))
        self.desc_ptr = self.desc_host.ctypes.data_as(ctypes.c_void_p)
        nbytes = _lib.call("cim_resample_ws_bytes", self.b, self.desc_ptr, out_w, out_h)      # (validates the whole batch)
        if nbytes < 0:
            raise _lib.CimHipError("cim_resample_ws_bytes: " + _lib.load().cim_last_error().decode())
        # (pinned + non_blocking: a pageable copy would make the host wait for everything already on the stream)
        self.desc_pinned = torch.from_numpy(self.desc_host).pin_memory()
        self.desc_dev = self.desc_pinned.to(device, non_blocking=True)
        self.ws = torch.empty((int(nbytes) + 7) // 8, dtype=torch.int64, device=device)
        self.src = None


def _gather(images, out_w, out_h, device, what):
    """-> _Batch with `src`: the images' bytes in one device buffer (host arrays: one pinned buffer, one non-blocking upload)."""
    whole = images if torch.is_tensor(images) and images.ndim == 4 else None      # one [B, h, w, 3] tensor: no gathering copy
    if torch.is_tensor(images) or isinstance(images, np.ndarray):
        images = [images] if images.ndim == 3 else list(images)
    images = list(images)
    if not images:
        raise ValueError("%s: no image" % what)
    on_device = [torch.is_tensor(im) for im in images]
    if any(on_device) and not all(on_device):
        raise ValueError("%s: NumPy arrays and tensors mixed in one batch" % what)
    if all(on_device):
        if not all(im.is_cuda for im in images):
            raise _lib.CimHipError("%s: CUDA/HIP tensor expected (no CPU fallback); host images are NumPy arrays" % what)
        device = images[0].device
    else:
        images = [np.ascontiguousarray(im) for im in images]
    for i, im in enumerate(images):
        if im.ndim != 3 or im.shape[2] != 3 or im.dtype not in (torch.uint8, np.uint8):
            raise ValueError("%s: image %d must be uint8 [h, w, 3] (RGB), got %s %s" % (what, i, tuple(im.shape), im.dtype))
    run = _Batch([im.shape[:2] for im in images], out_w, out_h, device, what)
    if all(on_device):
        flat = [whole.contiguous().reshape(-1)] if whole is not None else [im.contiguous().reshape(-1) for im in images]
        run.src = flat[0] if len(flat) == 1 else torch.cat(flat)
    else:
        run.src_pinned = torch.empty(run.nbytes, dtype=torch.uint8, pin_memory=True)
        host = run.src_pinned.numpy()
        for off, im in zip(run.offsets, images):
            host[off:off + im.size] = im.reshape(-1)
        run.src = run.src_pinned.to(run.device, non_blocking=True)
    return run


def pil_resize(images, size, *, normalize=None, device=None):
    """images: one uint8 [h, w, 3] array or a list of them (sizes may differ; or one [B, h, w, 3]), host NumPy or device tensors;
    size: Pillow's (width, height), or one integer.  Returns the device uint8 [B, H, W, 3] tensor Pillow's
    resize(size, Image.BILINEAR) gives image by image, or with normalize = (mean, std) (three floats each) the fp32
    [B, 3, H, W] tensor ((x / 255 - mean) / std in fp32: ToTensor + Normalize).  Three launches for the batch, no host read."""
    what = "cim_amd.resample.pil_resize"
    out_w, out_h = _size(size)
    run = _gather(images, out_w, out_h, device, what)
    if normalize is None:
        out = torch.empty((run.b, out_h, out_w, 3), dtype=torch.uint8, device=run.device)
        dst_u8, dst_f32, ms = out.data_ptr(), None, None
    else:
        mean, std = normalize
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("%s: normalize = (mean, std) with three values each" % what)
        ms = (ctypes.c_float * 6)(*[float(v) for v in mean], *[float(v) for v in std])
        out = torch.empty((run.b, 3, out_h, out_w), dtype=torch.float32, device=run.device)
        dst_u8, dst_f32 = None, out.data_ptr()
    with torch.cuda.device(run.device):
        _lib.call("cim_resample_rgb", run.src.data_ptr(), run.desc_ptr, run.desc_dev.data_ptr(), run.b, out_w, out_h, dst_u8, dst_f32,
                  ctypes.cast(ms, ctypes.c_void_p) if ms is not None else None, run.ws.data_ptr(), _lib.stream_ptr())
    return out


def tables(sizes, size, device=None):
    """The table launch alone (cim_resample_tables) for sources of `sizes` = [(h, w), ...]: per image
    (bounds_x [W, 2], coef_x [W, ksize], bounds_y [H, 2], coef_y [H, ksize]) as host int32 arrays (tests)."""
    out_w, out_h = _size(size)
    run = _Batch(sizes, out_w, out_h, device, "cim_amd.resample.tables")
    with torch.cuda.device(run.device):
        _lib.call("cim_resample_tables", run.desc_ptr, run.desc_dev.data_ptr(), run.b, out_w, out_h, run.ws.data_ptr(), _lib.stream_ptr())
    b = run.b
    kx = max(ksize(w, out_w) for _, w in run.sizes)
    ky = max(ksize(h, out_h) for h, _ in run.sizes)
    words = run.ws.cpu().numpy().view(np.int32)
    o_bx = 2 * b
    o_by = o_bx + b * out_w * 2
    o_cx = o_by + b * out_h * 2
    o_cy = o_cx + b * out_w * kx
    bx = words[o_bx:o_by].reshape(b, out_w, 2)
    by = words[o_by:o_cx].reshape(b, out_h, 2)
    cx = words[o_cx:o_cy].reshape(b, out_w, kx)
    cy = words[o_cy:o_cy + b * out_h * ky].reshape(b, out_h, ky)
    return [(bx[i].copy(), cx[i, :, :ksize(run.sizes[i][1], out_w)].copy(), by[i].copy(), cy[i, :, :ksize(run.sizes[i][0], out_h)].copy())
            for i in range(b)]
