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
(ssds/dataset/augment.py, tools/pack_dataset.py)."""
import argparse
import os
import sys

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


class Solver(object):
    """Same life cycle as the reference Solver (train_ddp.py:31-191)."""

    def __init__(self, cfg, local_rank, device, steps_per_epoch=100, sync_bn=False, render=False, data=None):
        self.cfg, self.local_rank, self.device = cfg, local_rank, device
        self.data = data_dir(cfg, data)
        self.steps_per_epoch = steps_per_epoch
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
                    render=args.render, data=args.data)
    solver.train_model(epochs=args.epochs)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
