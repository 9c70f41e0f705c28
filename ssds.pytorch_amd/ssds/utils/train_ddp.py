"""Data-parallel training entry point -- the reference's ``ssds/utils/train_ddp.py`` (Solver :31-191,
main :193-220) on torch DDP over RCCL/xGMI instead of Apex DDP/AMP/SyncBN over NCCL:

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        -m ssds.utils.train_ddp -cfg experiments/cfgs/ssd_mobilenetv2_512.yml --steps 100

One process per GPU; ``nccl`` backend == RCCL on ROCm.  bf16 autocast replaces AMP O1 / static loss scale
128 (bf16 has fp32's exponent range: no loss scaling).  BatchNorm stays local (per-GPU batch 64); ``--sync-bn``
computes its batch statistics over all ranks (the reference's convert_syncbn_model) on the same BatchNorm kernels and
fusions, split at one all-gather per direction (batchnorm.use_fast_sync_batchnorm; ``SSDK_FAST_BN=0 --sync-bn``: torch's
SyncBatchNorm).  Gradients: bucketed all-reduce (mean) overlapped with backward;
16 MB buckets keep every xGMI ring message bandwidth-bound for the 44 MB of SSD-MobileNetV2 gradients.
Data: synthetic COCO-shaped batches (ssds/dataset/synthetic.py) by default; ``--data DIR`` (or ``DATASET.DATASET: 'packed'``
with ``DATASET.DATASET_DIR``) trains on packed image shards through the reference's DALI graph as one HIP pass
(ssds/dataset/augment.py, tools/pack_dataset.py).

``-e`` evaluates instead (the reference's ``Solver.eval_model``, train.py:161-209): every checkpoint of ``EXP_DIR`` whose epoch
lies in ``TEST.TEST_SCOPE``, the images dealt out over the ranks, the metric records merged at the end of each epoch; rank 0
prints one line per checkpoint and appends it to ``EXP_DIR/eval_results.jsonl``."""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel as DDP

from ssds.core import checkpoint, config, criterion, optimizer
from ssds.dataset.synthetic import SyntheticDetectionLoader
from ssds.modeling import model_builder, train_routing
from ssds.pipeline.pipeline_anchor_ddp import ModelWithLossBasic, train_anchor_based_epoch


def data_dir(cfg, flag):
    """The directory of packed shards to train on, or None for the synthetic loader: ``--data DIR`` wins, then a config with
    ``DATASET.DATASET: 'packed'`` (which must name ``DATASET.DATASET_DIR``)."""
    if flag:
        return flag
    if cfg.DATASET.DATASET == "packed":
        if not cfg.DATASET.DATASET_DIR:
            raise ValueError("DATASET.DATASET is 'packed' but DATASET.DATASET_DIR is empty (or pass --data DIR)")
        return cfg.DATASET.DATASET_DIR
    return None


def select_checkpoints(index, test_scope, resume_checkpoint):
    """Which checkpoints ``Solver.eval_model`` evaluates -> [(epoch, path)], ascending by epoch.  ``index``: what
    ``checkpoint.find_previous_checkpoint(EXP_DIR)`` returned (([epochs], [paths]) or False).  Those whose epoch lies inside
    ``test_scope`` = [first, last], both inclusive (reference train.py:171-172); if the index has none, ``resume_checkpoint`` as
    epoch 0 (:188-196); if that is empty too, a ValueError."""
    first, last = int(test_scope[0]), int(test_scope[1])
    epochs, paths = index if index else ([], [])
    picked = sorted(((int(e), p) for e, p in zip(epochs, paths) if first <= int(e) <= last), key=lambda ep: ep[0])
    if picked:
        return picked
    if resume_checkpoint:
        return [(0, resume_checkpoint)]
    raise ValueError("nothing to evaluate: the checkpoint index of EXP_DIR has {} and RESUME_CHECKPOINT is empty".format(
        "no epoch inside TEST.TEST_SCOPE [{}, {}] (it has {})".format(first, last, sorted(int(e) for e in epochs))
        if epochs else "no entries"))


class _CountImages(object):
    """A loader, counting the images it hands out."""

    def __init__(self, loader):
        self.loader, self.images = loader, 0

    def __iter__(self):
        for batch in self.loader:  # (images, targets) or (images, targets, extras)
            self.images += int(batch[0].shape[0])
            yield batch


COCO_SUMMARY_KEYS = ("APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")  # what eval_model adds from CocoSummary


def _json_number(v):
    return None if (v is None or (isinstance(v, float) and math.isnan(v))) else float(v)


class Solver(object):
    """Same life cycle as the reference Solver (train_ddp.py:31-191).  ``phase="eval"``: only ``eval_model`` is used -- no model is
    built here (it builds a fresh one per checkpoint), nothing is routed for training and there is no optimizer."""

    def __init__(self, cfg, local_rank, device, steps_per_epoch=100, sync_bn=False, render=False, data=None, phase="train"):
        self.cfg, self.local_rank, self.device = cfg, local_rank, device
        self.data = data_dir(cfg, data)
        self.steps_per_epoch = steps_per_epoch
        if phase == "eval":
            return
        if local_rank == 0:
            print("===> Building model")
        self.model = model_builder.create_model(cfg.MODEL)
        self.load_model()
        train_routing.route_for_training(self.model, sync_bn=sync_bn, local_rank=local_rank)  # the kernel families, in table order
        self.model.to(self.device)
        if render and local_rank == 0:
            print("Model architectures:\n{}\n".format(self.model))
        if local_rank == 0:
            print("Trainable scope: {}".format(cfg.TRAIN.TRAINABLE_SCOPE))
        params = optimizer.trainable_param(self.model, cfg.TRAIN.TRAINABLE_SCOPE)
        self.optimizer = optimizer.configure_optimizer(params, cfg.TRAIN.OPTIMIZER)
        self.lr_scheduler = optimizer.configure_lr_scheduler(self.optimizer, cfg.TRAIN.LR_SCHEDULER)
        self.max_epochs = cfg.TRAIN.MAX_EPOCHS
        self.cls_criterion = getattr(criterion, cfg.MATCHER.CLASSIFY_LOSS)(
            alpha=cfg.MATCHER.FOCAL_ALPHA, gamma=cfg.MATCHER.FOCAL_GAMMA, negpos_ratio=cfg.MATCHER.NEGPOS_RATIO)
        self.loc_criterion = getattr(criterion, cfg.MATCHER.LOCATE_LOSS)()

    def wrap(self):
        mwl = ModelWithLossBasic(self.model, self.cls_criterion, self.loc_criterion, self.cfg.MODEL.NUM_CLASSES,
                                 self.cfg.MATCHER.MATCH_THRESHOLD, self.cfg.MATCHER.CENTER_SAMPLING_RADIUS)
        if dist.is_initialized() and dist.get_world_size() > 1:
            ids = [self.device.index] if self.device.type == "cuda" else None
            mwl = DDP(mwl, device_ids=ids, bucket_cap_mb=16, gradient_as_bucket_view=True)
        return mwl

    def train_model(self, epochs=None):
        mwl = self.wrap()
        if self.local_rank == 0:
            print("===> Loading data ({})".format("packed shards under " + self.data if self.data else "synthetic"))
        rank = dist.get_rank() if dist.is_initialized() else 0
        if self.data:
            from ssds.dataset.augment import AugmentedLoader, PackedDetectionSource

            world = dist.get_world_size() if dist.is_initialized() else 1
            loader = AugmentedLoader(PackedDetectionSource(self.data), self.cfg.DATASET, self.cfg.TRAIN.BATCH_SIZE, self.device,
                                     training=True, seed=1234, rank=rank, world_size=world, image_size=self.cfg.MODEL.IMAGE_SIZE)
        else:
            loader = SyntheticDetectionLoader(self.cfg.TRAIN.BATCH_SIZE, self.cfg.MODEL.IMAGE_SIZE,
                                              self.cfg.MODEL.NUM_CLASSES, self.steps_per_epoch, self.device,
                                              seed=1234 + rank)
        last = self.start_epoch + (epochs if epochs is not None else self.max_epochs)
        for epoch in range(self.start_epoch + 1, min(last, self.max_epochs) + 1):
            if self.local_rank == 0:
                sys.stdout.write("\rEpoch {epoch:d}/{max_epochs:d}:\n".format(epoch=epoch, max_epochs=self.max_epochs))
            inner = mwl.module.model if hasattr(mwl, "module") else mwl.model
            anchors = model_builder.create_anchors(self.cfg.MODEL, inner, self.cfg.MODEL.IMAGE_SIZE)
            if self.data:
                loader.set_epoch(epoch)
            train_anchor_based_epoch(mwl, loader, self.optimizer, anchors, epoch, self.device, self.local_rank)
            if epoch % self.cfg.TRAIN.CHECKPOINTS_EPOCHS == 0 and self.local_rank == 0 and rank == 0:
                checkpoint.save_checkpoints(inner, self.cfg.EXP_DIR, self.cfg.CHECKPOINTS_PREFIX, epoch)
            self.lr_scheduler.step()

    def load_model(self):
        previous = checkpoint.find_previous_checkpoint(self.cfg.EXP_DIR)
        if previous:
            self.start_epoch = previous[0][-1]
            checkpoint.resume_checkpoint(self.model, previous[1][-1], self.cfg.TRAIN.RESUME_SCOPE)
        else:
            self.start_epoch = 0
            if self.cfg.RESUME_CHECKPOINT:
                checkpoint.resume_checkpoint(self.model, self.cfg.RESUME_CHECKPOINT, self.cfg.TRAIN.RESUME_SCOPE)


    def eval_loader(self, dtype):
        """The eval data of this rank at ``TEST.BATCH_SIZE``: packed shards -- every image exactly once over the ranks, in order,
        the last batch possibly short -- or, without a data directory, synthetic batches (random targets: for smoke runs)."""
        rank = dist.get_rank() if dist.is_initialized() else 0
        if self.data:
            from ssds.dataset.augment import AugmentedLoader, PackedDetectionSource

            world = dist.get_world_size() if dist.is_initialized() else 1
            return AugmentedLoader(PackedDetectionSource(self.data), self.cfg.DATASET, self.cfg.TEST.BATCH_SIZE, self.device, dtype=dtype,
                                   training=False, seed=1234, rank=rank, world_size=world, image_size=self.cfg.MODEL.IMAGE_SIZE,
                                   eval_extras=True)
        return SyntheticDetectionLoader(self.cfg.TEST.BATCH_SIZE, self.cfg.MODEL.IMAGE_SIZE, self.cfg.MODEL.NUM_CLASSES,
                                        self.steps_per_epoch, self.device, seed=1234 + rank, dtype=dtype)

    def eval_model(self, data=None, dtype=torch.bfloat16):
        """The reference's ``eval_model`` (train.py:161-209) on all ranks: every checkpoint ``select_checkpoints`` picks is
        evaluated with the reference's metric (``MeanAveragePrecision`` at the decoder's NMS threshold -- the reference's
        choice, quirk included), the COCO sweep (AP@[.50:.95]) and the COCO summary (``CocoSummary``: AP by area, AR by maxDets and
        by area, crowd regions ignored -- crowd flags and annotation areas come from the shards where they hold them).  Rank 0 prints one line per checkpoint and appends it as
        JSON to ``EXP_DIR/eval_results.jsonl``; -> the list of those records (on every rank).

        Every checkpoint gets a FRESH, unrouted model (``create_model``, load, ``.eval().to(device, dtype)`` as ``SSDDetector``
        does): the recorded plan of a model keeps the weight packs it was recorded with, so loading a second checkpoint into a
        model that has already run would evaluate the first one's weights."""
        from ssds.core.evaluation_metrics import AveragePrecisionSweep, CocoSummary, MeanAveragePrecision
        from ssds.pipeline.pipeline_anchor_ddp import eval_anchor_based_epoch

        cfg = self.cfg
        if data:
            self.data = data_dir(cfg, data)
        picked = select_checkpoints(checkpoint.find_previous_checkpoint(cfg.EXP_DIR), cfg.TEST.TEST_SCOPE, cfg.RESUME_CHECKPOINT)
        multi = dist.is_initialized() and dist.get_world_size() > 1
        first_rank = (dist.get_rank() if dist.is_initialized() else 0) == 0
        decoder = model_builder.create_decoder(cfg.POST_PROCESS)
        classes = cfg.MODEL.NUM_CLASSES
        if self.local_rank == 0:
            print("===> Evaluating {} checkpoint(s) on {}".format(
                len(picked), "packed shards under " + self.data if self.data else "synthetic batches (random targets)"))
        records = []
        for epoch, path in picked:
            model = model_builder.create_model(cfg.MODEL)
            if checkpoint.resume_checkpoint(model, path, cfg.TRAIN.RESUME_SCOPE) is False:
                raise FileNotFoundError("eval_model: checkpoint of epoch {} not found at '{}'".format(epoch, path))
            model.eval().to(self.device, dtype)
            anchors = model_builder.create_anchors(cfg.MODEL, model, cfg.MODEL.IMAGE_SIZE)
            metrics = [MeanAveragePrecision(classes, decoder.conf_threshold, decoder.nms_threshold),
                       AveragePrecisionSweep(classes, decoder.conf_threshold), CocoSummary(classes, decoder.conf_threshold)]
            loader = _CountImages(self.eval_loader(dtype))
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            start = time.time()
            (ref_map, _), (ap, detail), (_, coco) = eval_anchor_based_epoch(model, loader, decoder, anchors, classes, self.device,
                                                                            metrics=metrics)
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            seconds = time.time() - start
            images = torch.tensor([loader.images], dtype=torch.int64)
            if multi:
                images = images.to(self.device) if dist.get_backend() == "nccl" else images
                dist.all_reduce(images)
            per_iou = dict((round(float(t), 2), v) for t, v in zip(detail["iou_thresholds"], detail["mAP_per_iou"]))
            record = {"epoch": int(epoch), "checkpoint": path, "mAP_reference": _json_number(float(ref_map)),
                      "AP": _json_number(float(ap)), "AP50": _json_number(per_iou.get(0.5)), "AP75": _json_number(per_iou.get(0.75)),
                      "images": int(images), "seconds": round(seconds, 3)}
            for key in COCO_SUMMARY_KEYS:  # AP / AP50 / AP75 stay those of the sweep
                record[key] = _json_number(float(coco["summary"][key]))
            records.append(record)
            if first_rank:
                show = lambda v: "nan" if v is None else "{:.4f}".format(v)  # noqa: E731
                print("Eval: epoch {} | mAP(reference) {} | AP@[.50:.95] {} | AP50 {} | AP75 {} | {} | {} images | {:.1f}s".format(
                    epoch, show(record["mAP_reference"]), show(record["AP"]), show(record["AP50"]), show(record["AP75"]),
                    " | ".join("{} {}".format(key, show(record[key])) for key in COCO_SUMMARY_KEYS), record["images"], seconds))
                os.makedirs(cfg.EXP_DIR, exist_ok=True)
                with open(os.path.join(cfg.EXP_DIR, "eval_results.jsonl"), "a") as f:
                    f.write(json.dumps(record) + "\n")
        return records


def main(argv=None):
    parser = argparse.ArgumentParser(description="Train a ssds.pytorch network (data parallel, RCCL)")
    parser.add_argument("-cfg", "--config", dest="config_file", required=True, help="the address of config file")
    parser.add_argument("--local_rank", type=int, default=int(os.environ.get("LOCAL_RANK", 0)))
    parser.add_argument("--steps", type=int, default=100, help="synthetic steps per epoch")
    parser.add_argument("--data", default=None, metavar="DIR",
                        help="train on the packed shards under DIR (tools/pack_dataset.py) instead of synthetic batches; "
                             "an epoch is then one pass over them")
    parser.add_argument("--epochs", type=int, default=1)
    parser.add_argument("--sync-bn", action="store_true")
    parser.add_argument("-r", "--render", action="store_true")
    parser.add_argument("-e", "--eval", dest="evaluate", action="store_true",
                        help="evaluate the checkpoints of EXP_DIR inside TEST.TEST_SCOPE instead of training (--steps: synthetic "
                             "batches per checkpoint when there is no --data)")
    args = parser.parse_args(argv)
    cfg = config.cfg_from_file(args.config_file)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if torch.cuda.is_available():
        torch.cuda.set_device(args.local_rank)
        device = torch.device("cuda", args.local_rank)
        backend = "nccl"  # RCCL on ROCm
    else:
        device, backend = torch.device("cpu"), "gloo"
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=backend, init_method="env://")
    solver = Solver(cfg, args.local_rank, device, steps_per_epoch=args.steps, sync_bn=args.sync_bn,
                    render=args.render, data=args.data, phase="eval" if args.evaluate else "train")
    if args.evaluate:
        solver.eval_model()
    else:
        solver.train_model(epochs=args.epochs)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
