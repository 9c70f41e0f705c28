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
from ssds.modeling import model_builder
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
        fast_bn = os.environ.get("SSDK_FAST_BN", "1") != "0"
        if sync_bn and not fast_bn:
            self.model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(self.model)
        elif fast_bn:
            from ssds.modeling.layers.batchnorm import use_fast_batchnorm, use_fast_sync_batchnorm

            if sync_bn:
                use_fast_sync_batchnorm(self.model)  # statistics over all ranks, on the same kernels and fusions
            else:
                use_fast_batchnorm(self.model)  # training BN on the ssdk kernels (local statistics, like the default)
            if os.environ.get("SSDK_FUSE_BN_ACT", "1") != "0":
                from ssds.modeling.layers.batchnorm import fuse_bn_activations

                fuse_bn_activations(self.model)  # Conv-BN-ReLU6: the clamp and its gradient mask ride on the BN passes
                from ssds.modeling.layers.batchnorm import fuse_bn_into_depthwise

                fuse_bn_into_depthwise(self.model)  # expand BN (+ ReLU6) applied by the depthwise kernels on load: no apply pass
        from ssds.modeling.layers import shuffletrain
        from ssds.modeling.nets.shufflenet import ShuffleNetV2

        if shuffletrain.enabled() and isinstance(getattr(self.model, "backbone", None), ShuffleNetV2):
            # ShuffleNetV2 backbones: the units' slice 1x1 and join on csrc/ssdk_shuffletrain.hip, their depthwise 3x3
            # on the project's depthwise kernels, 1x1 layers of any width.  After the BatchNorm swap and before the two calls below,
            # so the new DepthwiseConv2d / FastBatchNorm2d pairs get their statistics hand-off.  SSDK_SHUFFLE_TRAIN=0: chunk / cat /
            # channel_shuffle and nn.Conv2d.  Other backbones are not touched.
            shuffletrain.use_native_shuffle(self.model)
        from ssds.modeling.layers import densetrain
        from ssds.modeling.nets.densenet import DenseNet

        if isinstance(getattr(self.model, "backbone", None), DenseNet) and densetrain.enabled():
            # DenseNet backbones: a dense block trains on one feature buffer and one gradient buffer, norm1 + relu1
            # applied by the first 1x1 on load (csrc/ssdk_densetrain.hip); swapped at block level, the layers keep their classes.
            # SSDK_DENSE_TRAIN=0: _DenseBlock.forward, i.e. torch.cat and a full BatchNorm per layer.  The block's statistics are
            # local sums, so with --sync-bn the blocks stay on the module path.  Other backbones are not touched.
            if sync_bn:
                if local_rank == 0:
                    print("SSDK_DENSE_TRAIN: --sync-bn keeps the dense blocks on the module path (the block's statistics are local)")
            else:
                densetrain.use_native_dense_block(self.model)
        if os.environ.get("SSDK_PW_GEMM", "1") != "0":
            from ssds.modeling.layers.pointwise import use_pointwise_gemm

            use_pointwise_gemm(self.model)  # 1x1 convolutions on the NCHW tensors (16 bit: csrc/ssdk_pwtrain.hip; fp32: library GEMMs)
            if fast_bn:
                from ssds.modeling.layers.pointwise import fuse_conv_bn_statistics

                fuse_conv_bn_statistics(self.model)  # the 1x1 kernels hand their BatchNorm the (local) batch statistics
        from ssds.modeling.layers import groupedconv

        if groupedconv.enabled():
            # grouped 3x3 of the RegNetX / ResNeXt bottlenecks: forward, input gradient, weight gradient on csrc/ssdk_gconvtrain.hip
            # (SSDK_GCONV_TRAIN=0: nn.Conv2d, i.e. MIOpen's grouped convolution behind autocast's weight cast)
            groupedconv.use_native_gconv(self.model)
        from ssds.modeling.layers.pointwise import use_native_stem

        use_native_stem(self.model)  # the image-side 3x3 / stride-2 convolution: forward + weight gradient on csrc/ssdk_stemtrain.hip (A/B tools/run/r06_s42.sh: 17.0 vs 17.5 ms per step)
        from ssds.modeling.layers import stemconv

        if stemconv.enabled():
            # the 7x7 / stride-2 stem of the ResNet / ResNeXt backbones (any detector on them): forward + weight gradient on
            # csrc/ssdk_stem7train.hip.  SSDK_STEM7_TRAIN=0: nn.Conv2d, i.e. the library convolution behind autocast's weight cast
            stemconv.use_native_stem7(self.model)
        from ssds.modeling.layers import mbconvtrain

        if mbconvtrain.enabled():
            # the EfficientNet MBConv blocks: 5x5 depthwise forward / gradients and SiLU + squeeze-excite on csrc/ssdk_mbconvtrain.hip,
            # swapped at block level (the convolution modules keep their classes).  SSDK_MBCONV_TRAIN=0: MBConvBlock.forward, i.e.
            # the library's depthwise kernels and the eager SiLU / pool / 1x1 / multiply passes.  Any model: others have no such block
            mbconvtrain.use_native_mbconv(self.model)
        from ssds.modeling.layers.headconv import use_head_pairs

        use_head_pairs(self.model)  # SSD heads: forward of each level's loc | conf pair on the inference kernels (SSDK_HEAD_PAIR=0: MIOpen)
        from ssds.modeling.layers import denseconv
        from ssds.modeling.ssds.bifpn import SSDBiFPN
        from ssds.modeling.ssds.fpn import SSDFPN
        from ssds.modeling.ssds.yolo import YOLOV3, YOLOV4

        yolo = isinstance(self.model, (YOLOV3, YOLOV4))
        if isinstance(self.model, (SSDFPN, SSDBiFPN)) and denseconv.enabled():
            # dense 3x3 of the FPN / BiFPN detectors (towers, smoothing, heads, ResNet bottlenecks, extras): forward, input gradient,
            # weight gradient on csrc/ssdk_conv3train.hip.  Before the im2col swap below, which then skips the extras of these
            # models (no longer plain nn.Conv2d).  SSDK_DENSE3_TRAIN=0: nn.Conv2d / the im2col extras.  SSD models are not touched.
            denseconv.use_native_dense3x3(self.model)
        from ssds.modeling.layers import neckfuse

        if isinstance(self.model, (SSDFPN, SSDBiFPN)) and neckfuse.enabled():
            # the BiFPN weighted fusions, the FPN top-down upsample-adds and the ResNet stem's max-pool: forward and backward on
            # csrc/ssdk_necktrain.hip.  SSDK_NECK_TRAIN=0: the eager expressions / nn.MaxPool2d.  SSD models are not touched.
            neckfuse.use_native_neck(self.model)
        if yolo:
            # YOLOv3 / YOLOv4, each part under its own switch.  SSDK_DENSE3_TRAIN: every 3x3 of both shipped configs
            # (transforms, ConvBNReLUx2, heads, PAN stride-2 layers, ResNet BasicBlocks) fits csrc/ssdk_conv3train.hip -- before the
            # im2col swap below, which then skips the extras; measured slower than nn.Conv2d on these models, so here an unset
            # variable means 0 (denseconv.YOLO_DEFAULT).  SSDK_NECK_TRAIN: the ResNet stem max-pool on csrc/ssdk_necktrain.hip (all
            # use_native_neck touches on these models).  SSDK_CAT_TRAIN: the concatenations and the SPP block on csrc/ssdk_cattrain.hip.
            from ssds.modeling.layers import cattrain

            if denseconv.enabled(denseconv.YOLO_DEFAULT):
                denseconv.use_native_dense3x3(self.model)
            if neckfuse.enabled():
                neckfuse.use_native_neck(self.model)
            if cattrain.enabled():
                cattrain.use_native_cat(self.model)
        from ssds.modeling.ssds.shelf import SSDShelf

        if isinstance(self.model, SSDShelf):
            # SSDShelf, each part under its own switch.  SSDK_CONVT_TRAIN: the decoders' transposed 3x3 / stride 2 +
            # bias + skip add, forward and gradients on csrc/ssdk_convttrain.hip; the step measured slower with it (50.34 against
            # 47.36 ms at batch 32), so an unset variable means 0 (convttrain.DEFAULT).  SSDK_DENSE3_TRAIN: the SharedBlock 3x3 (one weight
            # on two maps), the encoder's stride-2 layers, the heads and the ResNet blocks fit csrc/ssdk_conv3train.hip -- before the
            # im2col swap below; those kernels measured slower than nn.Conv2d on ResNet-18 models and were never timed on Shelf, so
            # here an unset variable means 0, as on YOLO (denseconv.YOLO_DEFAULT).  SSDK_NECK_TRAIN: the ResNet stem max-pool on
            # csrc/ssdk_necktrain.hip (all use_native_neck touches on this model).
            from ssds.modeling.layers import convttrain

            if convttrain.enabled():
                convttrain.use_native_convt(self.model)
            if denseconv.enabled(denseconv.YOLO_DEFAULT):
                denseconv.use_native_dense3x3(self.model)
            if neckfuse.enabled():
                neckfuse.use_native_neck(self.model)
        conv3 = os.environ.get("SSDK_CONV3_NATIVE", "2")
        from ssds.modeling.layers import headconv

        headconv.WGRAD_MIN_PIXELS = 64 if conv3 == "0" else 0
        if conv3 == "2" and hasattr(self.model, "extras"):
            # (default) NO library convolution in the step: the extras' 3x3 / stride-2 layers as im2col + ssdk_pw_* + col2im with the
            # batch folded into the GEMM's pixel dimension (64 / 16 / 4 / 1 pixels per image: pointwise.FOLD_BELOW), and the weight
            # gradients of the small head levels on ssdk_pw_wgrad the same way.  tools/run/r06_s53.sh: 16.7 vs 17.0 ms per step
            # against the library (SSDK_CONV3_NATIVE=0); before the fold the same path was 0.6 ms SLOWER than the library
            from ssds.modeling.layers.pointwise import use_native_conv3x3

            use_native_conv3x3(self.model.extras)
        if conv3 == "1":
            # EVERY 3x3 layer (the heads too) as im2col + the 1x1 kernels.  Correct (tests/test_gpu_train.py) and slow: 23.2 vs
            # 20.8 ms per step when it was measured (round 6, session 4: the streaming 1x1 kernels are the wrong shape for
            # K = 864 ... 4608 at 480 output channels; the heads run on the inference kernels instead: headconv.py)
            from ssds.modeling.layers.pointwise import use_native_conv3x3

            use_native_conv3x3(self.model)
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
