"""Frames as compact arrays (nothing upstream: the reference stores the seven prepared fp32 planes of a frame, datasets/WaymoData.py).
One ``.pt`` dict per frame under ``<root>/<mode>/``:
    {"image": uint8 (H, W, 3), "points": float32 (N, 3) of (x, y, d), "boxes": int32 (M, 5) of (type, x, y, width, height)}
- the decoded camera image, upstream's ``lidar_array`` and its label dict (dmmfods_amd.prepare.labels_to_boxes).  The loader has the
surface of WaymoDataset_Loader and hands out ``RawBatch``es (dmmfods_amd.prepare.collate_raw), which ``BatchPrepare`` turns into the
model's tensors on the device."""
from os import listdir
from os.path import join

import torch
from torch.utils.data import DataLoader, Dataset

from ..prepare import collate_raw

MODES = ("train", "val", "test")


class RawFramesDataset(Dataset):
    def __init__(self, mode, config):
        super().__init__()
        if mode not in MODES:
            raise ValueError("Please choose a one of the following modes: train, val, test")
        self.dir = join(config.dir.data.root, mode)
        self.files = sorted(f for f in listdir(self.dir) if f.endswith(".pt"))

    def __len__(self):
        return len(self.files)

    def __getitem__(self, idx):
        if torch.is_tensor(idx):
            idx = idx.tolist()
        return torch.load(join(self.dir, self.files[idx]))


class RawFrames_Loader:
    """train_loader / valid_loader (+ *_iterations) like WaymoDataset_Loader; in 'test' mode valid_loader serves the test split."""

    def __init__(self, config):
        self.mode = config.loader.mode
        bs = config.loader.batch_size
        # (pin_memory: the DataLoader pins a RawBatch through its pin_memory method, in this process)
        kw = dict(batch_size=bs, num_workers=config.loader.num_workers, pin_memory=config.loader.pin_memory,
                  drop_last=config.loader.drop_last, collate_fn=collate_raw)

        def iters(ds):
            return len(ds) // bs if config.loader.drop_last else -(-len(ds) // bs)

        if self.mode == "train":
            train_set, valid_set = RawFramesDataset("train", config), RawFramesDataset("val", config)
            self.train_loader, self.valid_loader = DataLoader(train_set, **kw), DataLoader(valid_set, **kw)
            self.train_iterations, self.valid_iterations = iters(train_set), iters(valid_set)
        elif self.mode == "test":
            test_set = RawFramesDataset("test", config)
            self.valid_loader = DataLoader(test_set, **kw)
            self.valid_iterations = iters(test_set)
        else:
            raise ValueError("Please choose a one of the following modes: train, val, test")
