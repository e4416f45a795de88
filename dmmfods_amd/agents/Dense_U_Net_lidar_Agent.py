"""Training / validation driver with the reference agent's surface (reference: dmmfods/agents/Dense_U_Net_lidar_Agent.py:21-450):
``run / train / train_one_epoch / validate / save_checkpoint / load_checkpoint / finalize``, the checkpoint dict keyed by
``config.agent.checkpoint.*``, optional StepLR, best-checkpoint selection by mean validation IoU.

Differences, all on purpose: the step body uses the fused HIP tail (``model.loss_backward``), so loss sums, IoU and accuracy
come back as device tensors without the per-iteration host syncs of A:252-260 / H:359-363; TensorBoard is optional (not
installed here); ``compute_dtype`` / data parallelism are new, and so is the guarded optimiser step (``max_grad_norm``, ``loss_scaler``:
clipping by global norm, a dynamic loss scale and a skipped step on overflow, dmmfods_amd/optim.py) and gradient accumulation
(``config.optimizer.accumulate_steps``: one optimiser step per N batches, on the sum of their gradients) and a frozen-encoder
phase (``config.optimizer.freeze_encoder_epochs``: decoder and head train alone for the first N epochs) and parameter groups for
fine-tuning (``config.optimizer.encoder_lr_scale``, ``no_decay_norm_bias``, ``decoupled_weight_decay``: dmmfods_amd.optim.fine_tune_groups)
and a parameter average (``config.optimizer.ema_decay``, ``ema_warmup``: validation, and with it ``best_val_iou`` and the choice of the
best checkpoint, runs on the exponential moving average of the parameters that the Adam launch keeps; it travels inside the
checkpoint's optimiser entry) and a validation threshold sweep (``config.agent.threshold_sweep``: one more launch per validation batch
takes per-class logit histograms, and the epoch's ``val_history`` row carries IoU, precision, recall, F1, accuracy and average precision
at every threshold; ``best_val_iou`` and the checkpoints do not depend on it) and on-device augmentation of the training batches
(``config.loader.augment``: a dict of ``dmmfods_amd.augment.BatchAugment``'s arguments - crop, flip, shift, image gain and bias, modality
dropout in one launch per batch; its batch counter travels in the checkpoint's ``"augment"`` entry; validation is never augmented)
and object-level validation metrics (``config.agent.object_metrics``: the logits and the target of every validation batch are cut into
connected components on the device, ``dmmfods_amd.detect``, and the epoch's ``val_history`` row carries precision, recall, F1 and AP
over objects; one synchronisation per validation batch, or with ``match: "device"`` one per epoch; ``best_val_iou`` and the
checkpoints do not depend on it) and batch preparation on the device (``config.loader.raw_frames``: a dict of ``dmmfods_amd.prepare.BatchPrepare``'s arguments; the loader yields the uint8
image, the LiDAR points and the boxes of each frame, ``dmmfods_amd.datasets.RawFrames``, and three launches build the tensors the
reference's host preparation would, in training and in validation; the augmentation, where configured, follows it)."""
import logging
import os
import warnings
from collections.abc import Mapping
from datetime import datetime
from pathlib import Path

import numpy as np
import torch

from ..augment import BatchAugment
from ..datasets.RawFrames import RawFrames_Loader
from ..datasets.WaymoData import WaymoDataset_Loader
from ..prepare import BatchPrepare
from .._lib import MATCH_MAX_PER_PLANE
from ..detect import DeviceObjectMetrics, HeatMapDetector, ObjectMetrics
from ..graphs.models.Dense_U_Net_lidar import densenet121_u_lidar
from ..metrics import ThresholdSweep, logit_thresholds
from ..optim import DynamicLossScaler, FusedAdam, fine_tune_groups
from ..utils import Dense_U_Net_lidar_helper as utils

try:  # pragma: no cover - tensorboard is not installed in the build image
    from torch.utils.tensorboard import SummaryWriter
except Exception:  # noqa: BLE001
    SummaryWriter = None

CLASS_NAMES = ("Vehicle", "Pedestrian", "Cyclist")


class _NullWriter:
    def add_scalars(self, *a, **k):
        pass

    add_hparams = add_scalars

    def close(self):
        pass


class _StepLR:
    """lr = lr0 * gamma ** (epoch // step_size), stepped once per epoch (torch.optim.lr_scheduler.StepLR semantics)."""

    def __init__(self, optimizer, step_size, gamma):
        self.opt, self.step_size, self.gamma = optimizer, step_size, gamma
        self.base = [g["lr"] for g in optimizer.param_groups]
        self.epoch = 0

    def step(self):
        self.epoch += 1
        for g, b in zip(self.opt.param_groups, self.base):
            g["lr"] = b * self.gamma ** (self.epoch // self.step_size)


class Dense_U_Net_lidar_Agent:
    def __init__(self, config=None, torchvision_init=True, compute_dtype=None, data_loader=None, loss=None, max_grad_norm=None,
                 loss_scaler=None):
        self.logger = logging.getLogger("Agent")
        # the reference always builds DenseNet-121 (A:44); torchvision_init=True would download ImageNet weights (no network)
        self.model = densenet121_u_lidar(pretrained=False, config=config, compute_dtype=compute_dtype)
        self.config = self.model.config
        # loader.raw_frames: a dict of BatchPrepare's arguments (pool, kernel_size).  The loader then yields RawBatches - uint8 image,
        # LiDAR points, boxes - and the preparation on the device takes the place of the copy of seven fp32 planes, in training and in
        # validation.  Absent: the reference's loader and not one call more.
        self.prepare = self._make_prepare(self._optional(self.config.loader, "raw_frames"))
        if data_loader is None:
            data_loader = RawFrames_Loader(self.config) if self.prepare is not None else WaymoDataset_Loader(self.config)
        self.data_loader = data_loader
        # A:54.  The step uses the fused tail; a FocalLoss / ClassWiseFocalLoss (reference L:9-91) becomes its loss epilogue.
        self.loss = loss if loss is not None else torch.nn.BCEWithLogitsLoss(reduction="none")
        if hasattr(self.loss, "attach"):
            self.loss.attach(self.model)
        elif not isinstance(self.loss, torch.nn.BCEWithLogitsLoss):
            raise ValueError("loss must be BCEWithLogitsLoss(reduction='none') or a dmmfods_amd focal loss")
        o = self.config.optimizer
        # New here: not fields of the reference's create_config, read only if a config carries them.  dynamic_loss_scale: True
        # (GradScaler's defaults), an initial scale, or a dict of DynamicLossScaler arguments.
        if max_grad_norm is None:
            max_grad_norm = self._optional(o, "max_grad_norm")
        if loss_scaler is None:
            dyn = self._optional(o, "dynamic_loss_scale")
            if isinstance(dyn, bool):
                loss_scaler = DynamicLossScaler() if dyn else None
            elif isinstance(dyn, (int, float)):
                loss_scaler = DynamicLossScaler(init_scale=float(dyn))
            elif dyn is not None:
                loss_scaler = DynamicLossScaler(**dict(dyn))
        self.loss_scaler = loss_scaler
        # accumulate_steps = N > 1: one optimiser step per window of N batches, on the SUM of their gradients (the loss is a sum,
        # A:264: the gradient of the N-fold batch, BatchNorm statistics per batch).  Absent or 1: the reference's loop.
        acc = self._optional(o, "accumulate_steps")
        self.accumulate_steps = 1 if acc is None else int(acc)
        if self.accumulate_steps < 1:
            raise ValueError("optimizer.accumulate_steps must be an integer >= 1")
        if self.accumulate_steps > 1:
            self.model.set_grad_accumulation(True)
        # freeze_encoder_epochs = N > 0: the encoder (features, stream_2_features, concat_module) is frozen for the epochs < N and released
        # at the start of epoch N (the usual schedule on a pretrained encoder).  Absent or 0: the reference's loop.
        fe = self._optional(o, "freeze_encoder_epochs")
        self.freeze_encoder_epochs = 0 if fe is None else int(fe)
        if self.freeze_encoder_epochs < 0:
            raise ValueError("optimizer.freeze_encoder_epochs must be an integer >= 0")
        self.current_epoch = 0
        self._apply_freeze_phase()   # before the optimiser is built: a frozen parameter starts without optimiser state
        # encoder_lr_scale / no_decay_norm_bias / decoupled_weight_decay: when any is present the optimiser is built over the groups of
        # fine_tune_groups (the encoder at encoder_lr_scale x learning_rate, no decay on BatchNorm weights and biases, AdamW's
        # decay) and steps with one segmented launch.  All absent: the reference's single group.
        els, ndnb, dwd = (self._optional(o, k) for k in ("encoder_lr_scale", "no_decay_norm_bias", "decoupled_weight_decay"))
        grouped = {}
        if els is not None or ndnb is not None or dwd is not None:
            grouped = dict(param_groups=fine_tune_groups(self.model, o.learning_rate, o.weight_decay,
                                                         encoder_lr_scale=1.0 if els is None else float(els), no_decay_norm_bias=bool(ndnb)),
                           decoupled_weight_decay=bool(dwd))
        # ema_decay (and ema_warmup, default True): the optimiser keeps an exponential moving average of the parameters and
        # validate() runs on it.  Absent: the reference's loop, which validates the last iterate (A:165-213).
        ema_decay, ema_warmup = self._optional(o, "ema_decay"), self._optional(o, "ema_warmup")
        if ema_decay is not None:
            grouped.update(ema_decay=float(ema_decay), ema_warmup=True if ema_warmup is None else bool(ema_warmup))
        self.optimizer = FusedAdam(self.model, lr=o.learning_rate, betas=(o.beta1, o.beta2), eps=o.eps,
                                   weight_decay=o.weight_decay, amsgrad=o.amsgrad, max_grad_norm=max_grad_norm,
                                   loss_scaler=loss_scaler, **grouped)
        # agent.threshold_sweep: validation also takes per-class logit histograms (dmmfods_amd.metrics.ThresholdSweep) and its
        # val_history row carries every thresholded metric at every threshold.  Absent: the reference's loop, not one call more.
        self.sweep, self.sweep_column = self._make_sweep(self._optional(self.config.agent, "threshold_sweep"))
        # loader.augment: a dict of BatchAugment's arguments; every training batch is cropped / flipped / shifted / scaled on the device,
        # behind the copy to it and in front of the model, by one more launch.  Validation never is.  Absent: not one call more.
        self.augment = self._make_augment(self._optional(self.config.loader, "augment"))
        # agent.object_metrics: a dict (iou, connectivity, max_per_plane, min_area, threshold); validation also turns the logits and
        # the target of every batch into objects (dmmfods_amd.detect) and its val_history row carries object-level precision, recall,
        # F1 and AP.  Absent: not one call more.
        self.object_detector, self.object_metrics = self._make_object_metrics(self._optional(self.config.agent, "object_metrics"))
        self.lr_scheduler = None
        if o.lr_scheduler.want:
            self.lr_scheduler = _StepLR(self.optimizer, o.lr_scheduler.every_n_epochs, o.lr_scheduler.gamma)
        self.current_epoch = self.current_train_iteration = self.current_val_iteration = 0
        self.best_val_iou = 0
        # per-epoch averages as the reference logs them (A:301-307, A:392-398), kept for callers / tests: one dict per epoch
        self.train_history, self.val_history = [], []
        self.cuda = torch.cuda.is_available()
        if not self.cuda:
            raise RuntimeError("dmmfods_amd computes on the GPU only (no CPU fallback)")
        self.device = torch.device("cuda")
        torch.cuda.manual_seed_all(self.config.agent.seed)
        self.model = self.model.to(self.device)
        if not torchvision_init:
            self.load_checkpoint()
        Path(self.config.dir.current_run.summary).mkdir(exist_ok=True, parents=True)
        mk = (lambda: SummaryWriter(log_dir=self.config.dir.current_run.summary, comment="Dense_U_Net")) if SummaryWriter else _NullWriter
        self.train_summary_writer, self.val_summary_writer = mk(), mk()

    def _apply_freeze_phase(self):
        """The phase current_epoch is in (only with freeze_encoder_epochs: otherwise the model's flags are left alone)."""
        if self.freeze_encoder_epochs > 0:
            want = self.current_epoch < self.freeze_encoder_epochs
            if self.model.encoder_frozen != want:
                self.model.freeze_encoder(want)

    def _make_sweep(self, spec):
        """spec: None (no sweep), an integer K (the probabilities (k + 1) / (K + 1), k = 0 .. K - 1, as logits) or a list of logit
        thresholds.  iou_threshold is always merged in, so that the configured operating point is one of the columns; ground truth is
        cut at iou_threshold, as the loss kernel cuts it.  Returns (sweep, column of iou_threshold)."""
        if spec is None:
            return None, None
        if isinstance(spec, bool):
            raise ValueError("agent.threshold_sweep must be an integer K >= 1 or a list of logit thresholds")
        if isinstance(spec, int):
            if spec < 1:
                raise ValueError("agent.threshold_sweep must be an integer K >= 1 or a list of logit thresholds")
            thr = logit_thresholds([(k + 1) / (spec + 1) for k in range(spec)])
        else:
            thr = np.asarray([float(v) for v in spec], dtype=np.float64).astype(np.float32)
            if thr.size < 1 or not np.isfinite(thr).all() or not (np.diff(thr) > 0).all():
                raise ValueError("agent.threshold_sweep: a list of finite, strictly ascending logit thresholds")
        op = np.float32(self.config.agent.iou_threshold)
        thr = np.union1d(thr, np.asarray([op], dtype=np.float32))   # sorted, without duplicates
        sweep = ThresholdSweep(self.config.model.num_classes, thresholds=thr.tolist(), gt_threshold=float(self.config.agent.iou_threshold))
        return sweep, int(np.nonzero(sweep.thresholds == op)[0][0])

    def _make_object_metrics(self, spec):
        """spec: None (no object metrics) or a dict with any of iou (0.5), connectivity (8), max_per_plane (1024), min_area (1) and
        threshold (iou_threshold; it cuts the logits and the target alike, as the loss kernel's counts do), and match: "host" (default:
        ObjectMetrics, one synchronisation per validation batch) or "device" (DeviceObjectMetrics, one per epoch; it also takes
        capacity, the predictions kept per class for the AP).  Returns (detector, metrics)."""
        if spec is None:
            return None, None
        if not isinstance(spec, Mapping):
            raise ValueError("agent.object_metrics must be a dict (iou, connectivity, max_per_plane, min_area, threshold, match, capacity)")
        kw = dict(spec)
        unknown = set(kw) - {"iou", "connectivity", "max_per_plane", "min_area", "threshold", "match", "capacity"}
        if unknown:
            raise ValueError(f"agent.object_metrics: unknown keys {sorted(unknown)}")
        iou = kw.pop("iou", 0.5)
        threshold = kw.pop("threshold", None)
        match = kw.pop("match", "host")
        if match not in ("host", "device"):
            raise ValueError(f"agent.object_metrics: match must be 'host' or 'device', got {match!r}")
        if match == "host" and "capacity" in kw:
            raise ValueError("agent.object_metrics: capacity goes with match = 'device'")
        device_kw = {"capacity": kw.pop("capacity")} if "capacity" in kw else {}
        try:
            detector = HeatMapDetector(float(self.config.agent.iou_threshold if threshold is None else threshold), **kw)
            if match == "device":
                if detector.max_per_plane > MATCH_MAX_PER_PLANE:
                    raise ValueError(f"match = 'device' takes a max_per_plane of at most {MATCH_MAX_PER_PLANE}")
                metrics = DeviceObjectMetrics(self.config.model.num_classes, iou=iou, **device_kw)
            else:
                metrics = ObjectMetrics(self.config.model.num_classes, iou=iou)
        except (TypeError, ValueError) as e:
            raise ValueError(f"agent.object_metrics: {e}") from None
        return detector, metrics

    @staticmethod
    def _make_prepare(spec):
        """spec: None (the loader yields prepared tensors) or a dict of BatchPrepare's arguments."""
        if spec is None:
            return None
        if isinstance(spec, bool) or not hasattr(spec, "keys"):
            raise ValueError("loader.raw_frames must be a dict (pool, kernel_size)")
        unknown = set(spec.keys()) - {"pool", "kernel_size"}
        if unknown:
            raise ValueError(f"loader.raw_frames: unknown keys {sorted(unknown)}")
        try:
            return BatchPrepare(**dict(spec))
        except (TypeError, ValueError) as e:
            raise ValueError(f"loader.raw_frames: {e}") from None

    @staticmethod
    def _make_augment(spec):
        """spec: None (no augmentation) or a dict of BatchAugment's arguments.  The model takes sizes that are multiples of 32, so
        out_size has to be one; rank defaults to this process's torch.distributed rank, so that every rank draws its own parameters.
        The field takes the whole-pixel arguments only: BatchAugment's `scale` and `rotate` are not wired through the
        config yet and are refused like any unknown key - a caller who wants them sets `agent.augment` to a BatchAugment of their own."""
        if spec is None:
            return None
        kw = dict(spec)
        for name in ("scale", "rotate"):
            if name in kw:
                raise TypeError(f"loader.augment got an unexpected keyword argument '{name}' (set agent.augment = BatchAugment(...) to zoom or rotate)")
        if "rank" not in kw and torch.distributed.is_available() and torch.distributed.is_initialized():
            kw["rank"] = torch.distributed.get_rank()
        aug = BatchAugment(**kw)
        if aug.out_size is not None and (aug.out_size[0] % 32 or aug.out_size[1] % 32):
            raise ValueError("loader.augment: out_size must be a multiple of 32 in both dimensions")
        return aug

    @staticmethod
    def _optional(section, name):
        try:
            return getattr(section, name)
        except (AttributeError, KeyError):
            return None

    # ------------------------------------------------------------------ checkpoints (A:96-163)
    def save_checkpoint(self, filename="checkpoint.pth.tar", is_best=False):
        k = self.config.agent.checkpoint
        state = {k.epoch: self.current_epoch, k.train_iteration: self.current_train_iteration,
                 k.val_iteration: self.current_val_iteration, k.best_val_iou: self.best_val_iou,
                 k.state_dict: self.model.state_dict(), k.optimizer: self.optimizer.state_dict()}
        if self.augment is not None:
            state["augment"] = self.augment.state_dict()   # the number of batches drawn: a resumed run continues the sequence
        if is_best:
            filename = self.config.agent.best_checkpoint_name
        Path(self.config.dir.current_run.checkpoints).mkdir(exist_ok=True, parents=True)
        torch.save(state, os.path.join(self.config.dir.current_run.checkpoints, filename))

    def load_checkpoint(self, filename=None):
        filename = filename or self.config.agent.best_checkpoint_name
        path = os.path.join(self.config.dir.current_run.checkpoints, filename)
        k = self.config.agent.checkpoint
        try:
            ck = torch.load(path, map_location="cpu")
        except OSError:
            warnings.warn("No checkpoint exists from {}. Skipping...".format(path))
            self.logger.info("**First time to train**")
            return
        self.current_epoch = ck[k.epoch]
        self.current_train_iteration = ck[k.train_iteration]
        self.current_val_iteration = ck[k.val_iteration]
        self.best_val_iou = ck[k.best_val_iou]
        self.model.load_state_dict(ck[k.state_dict])
        self._apply_freeze_phase()   # the phase of the checkpoint's epoch, before the optimiser derives its step origins from the flags
        self.optimizer.load_state_dict(ck[k.optimizer])
        if self.augment is not None:
            # seed and batch counter from the checkpoint (one without the entry: batch 0); the rank stays this process's own - every
            # rank of a data-parallel run loads the file one of them wrote
            st = ck.get("augment") or {"seed": self.augment.seed, "batches_drawn": 0}
            self.augment.load_state_dict(dict(st, rank=self.augment.rank))

    # ------------------------------------------------------------------ driver (A:165-213)
    def run(self):
        print("starting " + self.config.loader.mode + " at " + str(datetime.now()))
        try:
            if self.config.loader.mode == "test":
                with torch.no_grad():
                    self.validate()
            else:
                self.train()
        except KeyboardInterrupt:
            self.logger.info("You have entered CTRL+C.. Wait to finalize")

    def train(self):
        self.config.loss.func = str(self.loss)
        self.config.optimizer.func = "FusedAdam(" + str(self.optimizer.defaults) + ")"
        self.save_hparams_json()
        for epoch in range(self.current_epoch, self.config.agent.max_epoch):
            self.current_epoch = epoch
            self.train_one_epoch()
            with torch.no_grad():
                avg_val_iou_per_class = self.validate()
            val_iou = sum(avg_val_iou_per_class) / len(avg_val_iou_per_class)
            is_best = val_iou > self.best_val_iou
            if is_best:
                self.best_val_iou = val_iou
            self.save_checkpoint(is_best=is_best)
        self.train_summary_writer.close()
        self.val_summary_writer.close()

    def _to_device(self, *tensors):
        nb = bool(self.config.loader.async_loading)
        return tuple(t.to(self.device, non_blocking=nb) for t in tensors)

    def _batch_tensors(self, batch):
        """What the loader yields -> (image, lidar, heat maps) on the device: the copy of the three tensors, or with loader.raw_frames
        the preparation of a RawBatch."""
        if self.prepare is not None:
            return self.prepare(batch, self.device)
        return self._to_device(*batch)

    @staticmethod
    def _batch_metrics(m):
        """Per-class IoU (NaN-mean over samples, NaN -> 0), NaN counts, accuracy: A:252-260 without leaving the device."""
        iou = m["iou_per_instance_per_class"]
        nan = torch.isnan(iou)
        cnt = (~nan).sum(dim=0).clamp_min(1)
        iou_pc = torch.where(nan, torch.zeros_like(iou), iou).sum(dim=0) / cnt
        iou_pc = torch.where((~nan).any(dim=0), iou_pc, torch.zeros_like(iou_pc))
        return iou_pc, nan.sum(dim=0), m["acc_per_class"]

    def _log(self, writer, tag, loss_pc, acc_pc, iou_pc, it):
        for name, vals in (("Loss", loss_pc), ("Accuracy", acc_pc), ("IoU", iou_pc)):
            d = {c: vals[i] for i, c in enumerate(CLASS_NAMES[: len(vals)])}
            d["Overall"] = torch.mean(vals)
            writer.add_scalars(f"{tag}/{name}", d, it)

    def train_one_epoch(self):
        self._apply_freeze_phase()
        self.model.train()
        n = self.data_loader.train_iterations
        nc = self.config.model.num_classes
        ep = {k: torch.zeros((n, nc), device=self.device) for k in ("loss", "iou", "nans", "acc")}
        guard = self.optimizer._guard   # the guarded step's state (None on the plain path); read ONCE per epoch, below
        skipped0 = guard.skipped_steps if guard is not None else 0
        window = self.accumulate_steps
        open_batches = 0   # batches whose gradients sit in the arena waiting for a step (always 0 here when window == 1)
        for b, batch in enumerate(self.data_loader.train_loader):
            image, lidar, ht_map = self._batch_tensors(batch)
            if self.augment is not None:
                image, lidar, ht_map = self.augment(image, lidar, ht_map)
            if window > 1 and open_batches == 0:
                self.optimizer.zero_grad()                    # A:263 (start of a window)
            with torch.no_grad():
                self.model(image, lidar)                      # A:244
            m = self.model.loss_backward(ht_map)              # A:247-264
            open_batches += 1
            if open_batches == window:
                self.optimizer.step()                         # A:265
                open_batches = 0
            iou_pc, nans, acc_pc = self._batch_metrics(m)
            ep["loss"][b], ep["iou"][b], ep["nans"][b], ep["acc"][b] = m["loss_per_class"], iou_pc, nans, acc_pc
            self._log(self.train_summary_writer, "Training", m["loss_per_class"], acc_pc, iou_pc, self.current_train_iteration)
            self.current_train_iteration += 1
        if open_batches:   # the epoch ended inside a window: step on what it holds - nothing is carried over or dropped
            self.optimizer.step()
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()
        self.train_history.append({"epoch": self.current_epoch, "loss": ep["loss"].mean(0).cpu(), "iou": ep["iou"].mean(0).cpu(),
                                   "nans": ep["nans"].sum(0).cpu(), "acc": ep["acc"].mean(0).cpu()})
        if guard is not None:   # one synchronisation per epoch, none per step
            gs = guard.state_dict()
            self.train_history[-1].update(loss_scale=gs["scale"], skipped_steps=gs["skipped_steps"] - skipped0)
            self.logger.info("Training at Epoch-%d | Loss scale: %g | Skipped steps: %d (of %d)", self.current_epoch, gs["scale"],
                             gs["skipped_steps"] - skipped0, n)
        self.logger.info("Training at Epoch-%d | Average Loss: %s | Average IoU: %s | Number of NaNs: %s | Average Accuracy: %s",
                         self.current_epoch, ep["loss"].mean(0).tolist(), ep["iou"].mean(0).tolist(), ep["nans"].sum(0).tolist(),
                         ep["acc"].mean(0).tolist())

    def validate(self):
        """With a parameter average (optimizer.ema_decay) the epoch's validation runs on the averaged parameters and the live
        BatchNorm statistics; its val_history row carries ema: True."""
        if self.optimizer.ema_arena is None:
            return self._validate()
        with self.optimizer.ema_weights():
            avg_iou = self._validate()
        self.val_history[-1]["ema"] = True
        return avg_iou

    def _validate(self):
        self.model.eval()
        n = self.data_loader.valid_iterations
        nc = self.config.model.num_classes
        ep = {k: torch.zeros((n, nc), device=self.device) for k in ("loss", "iou", "nans", "acc")}
        if self.sweep is not None:
            self.sweep.reset()
        if self.object_metrics is not None:
            self.object_metrics.reset()
        with torch.no_grad():
            for b, batch in enumerate(self.data_loader.valid_loader):
                image, lidar, ht_map = self._batch_tensors(batch)
                prediction = self.model(image, lidar)
                m = self.model.loss_metrics(prediction, ht_map)
                if self.sweep is not None:
                    self.sweep.update(prediction, ht_map)     # one more launch on the same stream, no synchronisation
                if self.object_metrics is not None:           # two calls on the same stream; match "host" pulls the records (one
                    # synchronisation), match "device" pairs them with three more launches and pulls nothing before compute()
                    self.object_metrics.update(self.object_detector(prediction.float()), self.object_detector(ht_map.float()))
                iou_pc, nans, acc_pc = self._batch_metrics(m)
                ep["loss"][b], ep["iou"][b], ep["nans"][b], ep["acc"][b] = m["loss_per_class"], iou_pc, nans, acc_pc
                self._log(self.val_summary_writer, "Validation", m["loss_per_class"], acc_pc, iou_pc, self.current_val_iteration)
                self.current_val_iteration += 1
        avg_iou = ep["iou"].mean(0).tolist()
        self.val_history.append({"epoch": self.current_epoch, "loss": ep["loss"].mean(0).cpu(), "iou": ep["iou"].mean(0).cpu(),
                                 "nans": ep["nans"].sum(0).cpu(), "acc": ep["acc"].mean(0).cpu()})
        self.logger.info("Validation at Epoch-%d | Average Loss: %s | Average IoU: %s | Number of NaNs: %s | Average Accuracy: %s",
                         self.current_epoch, ep["loss"].mean(0).tolist(), avg_iou, ep["nans"].sum(0).tolist(), ep["acc"].mean(0).tolist())
        if self.sweep is not None and self.sweep.counts is not None:   # one synchronisation per epoch, none per batch
            sw = {k: v.cpu() for k, v in self.sweep.compute().items()}
            self.val_history[-1]["sweep"] = sw
            self.logger.info("Validation at Epoch-%d | Threshold sweep (%d logit thresholds) | Best threshold: %s | Best IoU: %s | IoU at %g: %s",
                             self.current_epoch, self.sweep.num_thresholds, sw["best_threshold"].tolist(), sw["best_iou"].tolist(),
                             float(self.sweep.thresholds[self.sweep_column]), sw["iou"][:, self.sweep_column].tolist())
        if self.object_metrics is not None:
            ob = self.object_metrics.compute()
            self.val_history[-1]["objects"] = ob
            for c in range(nc):
                self.logger.info("Validation at Epoch-%d | Objects of class %d | Found: %d of %d | Predicted: %d | Precision: %g | Recall: %g | "
                                 "F1: %g | AP: %g | Overflowed planes: %d", self.current_epoch, c, ob["tp"][c], ob["num_gt"][c],
                                 ob["num_pred"][c], ob["precision"][c], ob["recall"][c], ob["f1"][c], ob["ap"][c], ob["overflowed_planes"])
        return avg_iou

    def save_hparams_json(self):
        hp = {"loss": dict(self.config.loss), "optimizer": {k: v for k, v in dict(self.config.optimizer).items()}}
        Path(self.config.dir.current_run.summary).mkdir(exist_ok=True, parents=True)
        utils.save_json_file(os.path.join(self.config.dir.current_run.summary, "hyperparams.json"), hp, indent=4)

    def finalize(self):
        self.logger.info("Please wait while finalizing the operation.. Thank you")
        self.train_summary_writer.close()
        self.val_summary_writer.close()
        print("ending " + self.config.loader.mode + " at " + str(datetime.now()))
