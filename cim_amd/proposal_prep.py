"""Per-proposal training inputs from raw proposal masks, on the device (csrc/proposal_prep.hip).

One read of the byte masks [N,H,W] yields everything `Generalized_RCNN.forward` takes per proposal: the tight boxes and the
S x S masks of tools/pre/generate_7_7_{voc,coco}.py:35-42, the PRM / point cluster matrix of tools/pre/AGPL_label_assign.py:
154-180 and point_level_label_assign.py:66-93, and - through the existing cim_mask_iou_pair - the two N x N maps.  Every
result is bit-identical to the reference's NumPy / PIL arithmetic.  Takes DEVICE tensors and launches on the current
stream; a CPU tensor is an error (no CPU fallback).
"""
import ctypes

import numpy as np
import torch

from . import _lib, mask_iou

MAX_POINTS = _lib.CONSTANTS["CIM_PROP_MAX_POINTS"]
MAX_S = _lib.CONSTANTS["CIM_PROP_MAX_S"]
MAX_HW = _lib.CONSTANTS["CIM_SEGM_MAX_HW"]
MAX_SIDE = 65535                # the reference stores boxes as uint16


class Prepared(object):
    """What `prepare` returns; every attribute is a device tensor.
    boxes [N,4] int32 (xmin, ymin, xmax+1, ymax+1), masks [N,S,S] bool, area [N] int32, packed [words,N] int64 (the
    word-major layout of cim_mask_pack), height / width of the image."""

    def __init__(self, boxes, masks, area, packed, height, width):
        self.boxes, self.masks, self.area, self.packed = boxes, masks, area, packed
        self.height, self.width = height, width

    def maps(self):
        """(iou_f16 [N,N], asy_f16 [N,N]) from the packed words: what cim_amd.mask_iou.mask_iou_maps gives for the masks."""
        iou, asy, _ = mask_iou.maps_from_packed(self.packed)
        return iou, asy

    def roidb_fields(self, mat=None):
        """Host arrays with the dtypes of the reference's pickles - boxes uint16, masks bool, mat float32 - as a dict that
        updates a roidb entry of cim_amd.roi_data.get_minibatch."""
        out = {"boxes": self.boxes.cpu().numpy().astype(np.uint16), "masks": self.masks.cpu().numpy().astype(bool)}
        if mat is not None:
            out["mat"] = mat.cpu().numpy().astype(np.float32) if torch.is_tensor(mat) else np.asarray(mat, dtype=np.float32)
        return out


def _check_shape(n, h, w):
    if n < 1:
        raise ValueError("cim_amd.proposal_prep: N = %d proposals, at least one is needed" % n)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError("cim_amd.proposal_prep: image %d x %d, sides must be 1..%d (boxes are uint16 in the reference)" % (h, w, MAX_SIDE))
    if h * w > MAX_HW:
        raise ValueError("cim_amd.proposal_prep: %d x %d = %d pixels per mask, the kernels take at most %d" % (h, w, h * w, MAX_HW))


def _workspace(n, hw, p, device):
    nbytes = _lib.call("cim_prop_ws_bytes", n, hw, p)
    if nbytes < 0:
        raise ValueError(_lib.load().cim_last_error().decode())
    return torch.empty((int(nbytes) + 7) // 8, dtype=torch.int64, device=device)


def prepare(masks, mask_size=7):
    """masks [N,H,W] bool / uint8 on the device -> Prepared.  Raises ValueError for an empty mask (the reference's
    ind_xy[1].min() raises there), naming the first such proposal: the one host read of this call."""
    if not torch.is_tensor(masks) or not masks.is_cuda:
        raise _lib.CimHipError("cim_amd.proposal_prep.prepare: CUDA/HIP tensor expected (no CPU fallback)")
    if masks.dim() != 3:
        raise ValueError("cim_amd.proposal_prep.prepare: masks must be [N, H, W], got %s" % (tuple(masks.shape),))
    n, h, w = (int(s) for s in masks.shape)
    _check_shape(n, h, w)
    s = int(mask_size)
    if not 1 <= s <= MAX_S:
        raise ValueError("cim_amd.proposal_prep.prepare: mask_size = %d, the kernels take 1..%d" % (s, MAX_S))
    hw = h * w
    m = masks.reshape(n, hw)
    if m.dtype == torch.bool:
        m = m.contiguous().view(torch.uint8)                 # same bytes (as mask_iou.pack_masks): no conversion pass
    elif m.dtype != torch.uint8:
        m = (m != 0).to(torch.uint8).contiguous()
    else:
        m = m.contiguous()
    dev = masks.device
    packed = torch.empty(((hw + 63) // 64, n), dtype=torch.int64, device=dev)
    head = torch.empty(1 + 5 * n, dtype=torch.int32, device=dev)          # empty flag | boxes [N,4] | area [N]
    small = torch.empty((n, s, s), dtype=torch.uint8, device=dev)
    ws = _workspace(n, hw, 0, dev)
    base = head.data_ptr()
    _lib.call("cim_prop_prepare", m.data_ptr(), n, h, w, s, packed.data_ptr(), base + 4, base + 4 * (1 + 4 * n), small.data_ptr(),
              base, ws.data_ptr(), _lib.stream_ptr())
    flag = int(head[0])
    if flag != 0:
        raise ValueError("cim_amd.proposal_prep.prepare: proposal %d has no pixel (the reference's ind_xy[1].min() raises)" % (n - flag))
    return Prepared(head[1:1 + 4 * n].view(n, 4), small.view(torch.bool), head[1 + 4 * n:], packed, h, w)


def _host_i32(a, name):
    a = np.asarray(a.cpu() if torch.is_tensor(a) else a)
    if a.size and not np.all(a == np.floor(a)):
        raise ValueError("cim_amd.proposal_prep.assign_clusters: %s must be integers" % name)
    return np.ascontiguousarray(a.reshape(-1), dtype=np.int64)


def assign_clusters(prep, rows, cols, classes, num_classes):
    """The cluster matrix mat [N, num_classes + 1] float32 (device) for P points given as pixel (row, col) and class, in the
    order the reference visits them (AGPL: ascending peak score).  Per point: the proposals covering it, their average mask
    (> 0.7), every proposal's IoU with it; IoU > 0.5 assigns cluster j + 1 in column class + 1 (the last point wins),
    0 < IoU <= 0.5 without any assignment gives P + 1 in column 0.  No host synchronisation."""
    if not isinstance(prep, Prepared):
        raise TypeError("cim_amd.proposal_prep.assign_clusters: the result of prepare() is expected")
    rows, cols, classes = _host_i32(rows, "rows"), _host_i32(cols, "cols"), _host_i32(classes, "classes")
    p, c = rows.size, int(num_classes)
    if not (cols.size == p and classes.size == p):
        raise ValueError("cim_amd.proposal_prep.assign_clusters: rows, cols and classes differ in length")
    if p > MAX_POINTS:
        raise ValueError("cim_amd.proposal_prep.assign_clusters: %d points, at most %d" % (p, MAX_POINTS))
    if c < 1:
        raise ValueError("cim_amd.proposal_prep.assign_clusters: num_classes = %d" % c)
    h, w = prep.height, prep.width
    for j in range(p):
        if not (0 <= rows[j] < h and 0 <= cols[j] < w):
            raise ValueError("cim_amd.proposal_prep.assign_clusters: point %d at (row %d, col %d) lies outside the %d x %d image"
                             % (j, rows[j], cols[j], h, w))
        if not 0 <= classes[j] < c:
            raise ValueError("cim_amd.proposal_prep.assign_clusters: point %d has class %d, outside 0..%d" % (j, classes[j], c - 1))
    words, n = prep.packed.shape
    dev = prep.packed.device
    mat = torch.empty((n, c + 1), dtype=torch.float32, device=dev)
    ws = _workspace(n, h * w, p, dev)
    host = [np.ascontiguousarray(a, dtype=np.int32) for a in (rows, cols, classes)]
    ptrs = [a.ctypes.data_as(ctypes.c_void_p) for a in host]
    _lib.call("cim_prop_assign", prep.packed.data_ptr(), prep.area.data_ptr(), n, h, w, ptrs[0], ptrs[1], ptrs[2], p, c,
              mat.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
    return mat


def label_assign(model, images_u8, labels, masks_list, mask_size=7, resize="device"):
    """tools/pre/AGPL_label_assign.py `assign_voc2012` / `assign_coco2017` for a batch of images, without the reference:
    model = a cim_amd.prm.PeakResponseMapping on the device, images_u8 = B RGB uint8 arrays [h, w, 3] (host; what
    Image.open(...).convert('RGB') holds), labels = B lists of image-level classes (ascending, as torch.unique leaves them),
    masks_list = B device tensors [N_i, h, w] of the image's proposal masks.  Returns B cluster matrices `mat`
    [N_i, num_classes + 1] float32 on the device (21 or 81 columns by the model's classifier).
    resize = "device" (default): the antialiased transforms.Resize([448, 448]), ToTensor and Normalize are three launches for the
    batch (cim_amd.prm.network_input_from_images, bit-identical to Pillow: DESIGN.md 4.20); "pillow": Pillow's own call on the
    host, once per image, and an upload of the resized copy (kept for comparison; Pillow is imported on this path only).  The
    results are the same bit for bit.  Everything runs on the device with ONE host read per batch (cim_amd.prm.peaks) plus
    `prepare`'s empty-mask flag per image.  An image without classes gets the reference's `visual_cues == None` matrix
    (column 0 = 1)."""
    from . import prm
    b = len(images_u8)
    if not (len(labels) == b and len(masks_list) == b):
        raise ValueError("cim_amd.proposal_prep.label_assign: %d images, %d class lists, %d mask tensors" % (b, len(labels), len(masks_list)))
    if resize not in ("device", "pillow"):
        raise ValueError("cim_amd.proposal_prep.label_assign: resize = %r, 'device' or 'pillow' expected" % (resize,))
    size = prm.INPUT_SIZE
    sizes = [(int(m.shape[1]), int(m.shape[2])) for m in masks_list]
    if not any(len(ls) for ls in labels):
        points = [((), (), (), ())] * b
    else:
        if resize == "pillow":
            from PIL import Image
            resized = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(im, dtype=np.uint8)).resize((size, size), Image.BILINEAR))
                                for im in images_u8])
            inputs = prm.network_input(torch.from_numpy(resized).to(masks_list[0].device))
        else:
            images = [im if torch.is_tensor(im) else np.ascontiguousarray(im, dtype=np.uint8) for im in images_u8]
            inputs = prm.network_input_from_images(images, size, device=masks_list[0].device)
        points = prm.peaks(model, inputs, labels, image_sizes=sizes)
    num_classes = model[0].classifier[0].out_channels
    mats = []
    for masks, (rows, cols, classes, _) in zip(masks_list, points):
        prep = prepare(masks, mask_size)
        mats.append(assign_clusters(prep, rows, cols, classes, num_classes))
    return mats


def peaks_to_pixels(peak_list, height, width):
    """AGPL_label_assign.py:156-161: peak_list [P, 4] = (batch, class, a, b) on the PRM's 112 x 112 grid, already in ascending
    peak_score order -> (rows, cols, classes) with row = int(a * H / 112), col = int(b * W / 112) (the reference names them
    x and y and indexes mask_proposals[:, x, y])."""
    peaks = np.asarray(peak_list).reshape(-1, 4)
    rows = [int(pk[2] * height / 112) for pk in peaks]
    cols = [int(pk[3] * width / 112) for pk in peaks]
    classes = [int(pk[1]) for pk in peaks]
    return rows, cols, classes


def points_to_pixels(points):
    """point_level_label_assign.py:56, 68-75: points = (x, y, class, conf) per line of the Center_points file ->
    (rows, cols, classes) with col = int(x), row = int(y)."""
    rows = [int(pt[1]) for pt in points]
    cols = [int(pt[0]) for pt in points]
    classes = [int(pt[2]) for pt in points]
    return rows, cols, classes
