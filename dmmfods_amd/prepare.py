"""Raw frames to training tensors on the device (upstream this is host code: avgpool_tensor, lidar_array_to_image_like_tensor,
pool_lidar_tensor, create_ground_truth_maps and maxpool_tensor of utils/Dense_U_Net_lidar_helper.py, whose seven fp32 planes per frame
the loader then copies to the device).

What travels to the device is what the planes are made from - the uint8 camera image, the projected LiDAR points, the labelled
boxes.  ``dmm_prep_image``, ``dmm_prep_lidar`` and ``dmm_prep_heat_maps`` (csrc/prepare.hip) turn them into the (B, 7, Ho, Wo) batch
the model and the loss read: exact, bit-reproducible, without synchronisation.  The rules are stated in include/dmmfods_hip.h and
restated in numpy in tools/prepare_ref.py."""
import ctypes as C

import numpy as np
import torch

from . import _lib


class RawBatch:
    """B frames as compact arrays: image uint8 (B, H, W, C); points float32 (n, 3) of (x, y, d) and boxes int32 (m, 5) of
    (type, x, y, width, height), both concatenated over the frames, frame b owning [offsets[b], offsets[b + 1]) (int32, B + 1)."""

    def __init__(self, image, points, point_offsets, boxes, box_offsets):
        self.image, self.points, self.point_offsets, self.boxes, self.box_offsets = image, points, point_offsets, boxes, box_offsets

    def __len__(self):
        return self.image.shape[0]

    def pin_memory(self):
        """The same batch in pinned host memory (what a DataLoader with pin_memory=True calls)."""
        return RawBatch(*(t.pin_memory() for t in (self.image, self.points, self.point_offsets, self.boxes, self.box_offsets)))


def labels_to_boxes(label_dict):
    """Upstream's saved label dict ({name: {"type", "x", "y", "width", "height"}}, x and y the top-left corner) -> int32 (M, 5) of
    (type, x, y, width, height) in dict order, the order upstream draws them in."""
    rows = [[int(v[k]) for k in ("type", "x", "y", "width", "height")] for v in label_dict.values()]
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 5)


def collate_raw(frames, pin_memory=False):
    """frames: dicts {"image": uint8 (H, W, C), "points": float32 (N, 3), "boxes": int32 (M, 5)} of one image size -> RawBatch.
    pin_memory: the arrays are handed out in pinned host memory, for asynchronous copies."""
    frames = list(frames)
    if not frames:
        raise ValueError("collate_raw: no frames")
    images = [torch.as_tensor(f["image"]) for f in frames]
    if any(i.dtype != torch.uint8 or i.dim() != 3 or i.shape != images[0].shape for i in images):
        raise ValueError("collate_raw: every image must be uint8 (H, W, C) of one size")
    points = [torch.as_tensor(f["points"], dtype=torch.float32).reshape(-1, 3) for f in frames]
    boxes = [torch.as_tensor(f["boxes"], dtype=torch.int32).reshape(-1, 5) for f in frames]

    def offsets(parts):
        return torch.tensor(np.concatenate([[0], np.cumsum([len(p) for p in parts])]), dtype=torch.int32)

    raw = RawBatch(torch.stack(images), torch.cat(points), offsets(points), torch.cat(boxes), offsets(boxes))
    return raw.pin_memory() if pin_memory else raw


class BatchPrepare:
    """RawBatch -> (image (B, C, Ho, Wo), lidar (B, 1, Ho, Wo), heat_maps (B, 3, Ho, Wo)): fp32 views of ONE (B, C + 4, Ho, Wo) device
    tensor, Ho = H / pool, Wo = W / pool.  The compact arrays are copied to the device without blocking, the three preparations are
    enqueued on the current stream, nothing is synchronised.  The LiDAR workspace and the output are cached per shape: the views a call
    returns are overwritten by the next call of the same shape (as a loader's batch is by the next)."""

    def __init__(self, pool=10, kernel_size=5):
        for name, v in (("pool", pool), ("kernel_size", kernel_size)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} must be an integer")
        if pool < 1:
            raise ValueError("pool must be >= 1")
        if kernel_size % 2 == 0 or not 1 <= kernel_size <= 15:
            raise ValueError("kernel_size must be odd and in [1, 15]")
        self.pool, self.kernel_size = int(pool), int(kernel_size)
        self._cache = {}

    def output_size(self, H, W):
        return H // self.pool, W // self.pool

    def __call__(self, raw, device=None):
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise RuntimeError("dmmfods_amd computes on the GPU only (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        img = raw.image
        if img.dim() != 4 or img.dtype != torch.uint8:
            raise ValueError("image must be uint8 (B, H, W, C)")
        B, H, W, Cc = img.shape
        p = self.pool
        if H % p or W % p:
            raise ValueError(f"H and W must be multiples of pool ({p})")
        po, bo = (np.ascontiguousarray(torch.as_tensor(o).cpu().numpy(), dtype=np.int32) for o in (raw.point_offsets, raw.box_offsets))
        if len(po) != B + 1 or len(bo) != B + 1:
            raise ValueError("point_offsets and box_offsets must have B + 1 entries")
        L = _lib.lib()
        with torch.cuda.device(device):
            image = img.contiguous().to(device, non_blocking=True)
            points = raw.points.to(device=device, dtype=torch.float32, non_blocking=True).contiguous()
            boxes = raw.boxes.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()
            if points.shape[0] != po[-1] or boxes.shape[0] != bo[-1]:
                raise ValueError("the last offset must be the number of points / boxes")
            key = (device.index, B, H, W, Cc)
            if key not in self._cache:
                need = L.dmm_prep_lidar_workspace(B, H, W)
                if need == 0:
                    raise ValueError("dmm_prep_lidar_workspace refuses these sizes (B, H, W >= 1 and H * W < 2^31)")
                self._cache[key] = (torch.empty(need, dtype=torch.uint8, device=device),
                                    torch.empty((B, Cc + 4, H // p, W // p), dtype=torch.float32, device=device))
            ws, out = self._cache[key]
            Ho, Wo = out.shape[2:]
            stride, plane = out.stride(0), Ho * Wo
            st = _lib.stream_ptr()
            _lib.check(L.dmm_prep_image(image.data_ptr(), H * W * Cc, out.data_ptr(), stride, B, H, W, Cc, p, st))
            _lib.check(L.dmm_prep_lidar(points.data_ptr(), po.ctypes.data_as(C.POINTER(C.c_int32)), out.data_ptr() + 4 * Cc * plane, stride,
                                        B, H, W, p, self.kernel_size, ws.data_ptr(), ws.numel(), st))
            _lib.check(L.dmm_prep_heat_maps(boxes.data_ptr(), bo.ctypes.data_as(C.POINTER(C.c_int32)), out.data_ptr() + 4 * (Cc + 1) * plane,
                                            stride, B, H, W, p, st))
            # the device copies are read by launches that are only enqueued: the caching allocator hands their memory out again to this
            # stream alone, behind those launches
        return out[:, :Cc], out[:, Cc:Cc + 1], out[:, Cc + 1:]
