"""trainer.py -- drop-in for the reference Trainer (trainer.py:40-337) driving the MI355X-native step.

Kept: `Trainer(config)` with the reference's YAML schema (configs/basic_config.yaml), dynamic model lookup
(`models.<type>.<file>.<name>`, trainer.py:154-170), one Adam over depth+pose parameters at optimizer.depth.lr,
StepLR, checkpoint dict keys (trainer.py:129-152), `train()`, `run_epoch()`, `process_batch(samples)`.
Changed underneath: the optimiser is the fused Adam over the flat arena, `zero_grad` is one memset, and when
torch.distributed is initialised the gradient arena is all-reduced once per step (RCCL over xGMI).
wandb logging and the image dumps are out of scope.
"""
import importlib
import os
import time
from inspect import getmembers, isclass

import numpy as np
import torch
from torch.utils.data import Sampler

from losses import Losses
from geometry.pose_geometry import *  # noqa: F401,F403  (the reference star-imports it, trainer.py:27)
from mcav import dist as mdist
from mcav.optim import FusedAdam


class SequentialIndicesSampler(Sampler):
    def __init__(self, indices):
        self.indices = indices

    def __iter__(self):
        return iter(self.indices)

    def __len__(self):
        return len(self.indices)


class Trainer:
    def __init__(self, config, dataset=None):
        if not torch.cuda.is_available():
            raise RuntimeError("Trainer: the MI355X path needs a GPU (there is no CPU fallback)")
        self.rank, self.world = mdist.init_from_env()
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.save_path = './pretrained/' + config['model']['name'] + '.pth'
        act = config['action']
        self.batch_size = act['batch_size']
        self.learning_rate = act['optimizer']['depth']['lr']
        self.scheduler_step_size = act['scheduler']['step_size']
        self.gamma = act['scheduler']['gamma']
        self.shuffle_dataset = config['datasets']['augmentation']['shuffle']
        self.mode = act['mode']
        self.train_from_scratch = act['from_scratch']
        self.num_epochs = act['num_epochs']
        self.num_workers = act['num_workers']
        self.log_freq = act['log_freq']
        self.epoch = 0
        self.step = 0
        self.verbose = bool(act.get('verbose', True))
        # action.hipgraph: true / false / "auto" (default).  The replayed step (two chains of graphs, mcav/graph.py) is level with eager issue
        # at batch 12 x 192 x 640 and 15 % faster at the reference config's batch 4 (the eager step is host-bound there): "auto" replays when a
        # batch is at most half the headline's pixels, and falls back to eager issue for good if a capture ever fails.
        hg = act.get('hipgraph', 'auto')
        self.use_hipgraph = hg if isinstance(hg, str) and hg.lower() == 'auto' else bool(hg)
        if isinstance(self.use_hipgraph, str):
            self.use_hipgraph = 'auto' 
        self._graphs = None

        self.depth_model = self.load_from_config(config, model_type='depth')
        self.pose_model = self.load_from_config(config, model_type='pose')
        parameters_train = list(self.depth_model.parameters()) + list(self.pose_model.parameters())
        self.model_optimizer = FusedAdam(parameters_train, self.learning_rate)
        self.model_lr_scheduler = torch.optim.lr_scheduler.StepLR(self.model_optimizer, self.scheduler_step_size, self.gamma)
        mdist.broadcast_parameters(self.model_optimizer.arena())
        if os.environ.get("MCAV_DP_OVERLAP", "1") != "0":
            mdist.enable_overlap(self.model_optimizer.arena())      # N > 1: the all-reduce hides behind the rest of backward

        self.criterion = Losses()
        self.criterion.ssim = bool((config.get('loss') or {}).get('ssim', False))     # opt-in SSIM + L1 photometric mix (losses.py)
        self.criterion.min_reprojection = bool((config.get('loss') or {}).get('min_reprojection', False))   # opt-in per-pixel minimum
        self.criterion.automask = bool((config.get('loss') or {}).get('automask', False))                   # and identity auto-masking
        self.criterion.edge_aware_smoothness = bool((config.get('loss') or {}).get('edge_aware_smoothness', False))   # monodepth2's smoothness
        self.criterion.edge_smoothness_weight = float((config.get('loss') or {}).get('edge_smoothness_weight', 1e-3))
        self.criterion.geometry_consistency = bool((config.get('loss') or {}).get('geometry_consistency', False))   # SC-SfMLearner's depth consistency
        self.criterion.geometry_consistency_weight = float((config.get('loss') or {}).get('geometry_consistency_weight', 0.5))
        self.criterion.geometry_min_valid = int((config.get('loss') or {}).get('geometry_min_valid', 100))
        self.criterion.fused_pyramid = bool((config.get('loss') or {}).get('fused_pyramid', False))       # multi-scale nets: one launch pair
        upsample = (config.get('loss') or {}).get('multiscale_upsample', 'depth')                           # depth (reference) | disparity (monodepth2)
        if upsample not in ('depth', 'disparity'):
            raise ValueError("config loss.multiscale_upsample must be depth or disparity, got %r" % (upsample,))
        self.criterion.multiscale_upsample = upsample
        from dataloaders import stereo_from_config
        self.criterion.stereo = stereo_from_config(config)      # opt-in mono + stereo (metric depth): batches carry 'stereo' / 'stereo_baseline'
        self.validation = self.validation_config(config.get('validation'))      # opt-in KITTI protocol for validate()
        from mcav.streams import Branch
        self.pose_branch = Branch()
        self.loss = None
        self.valid_acc = 0
        if self.train_from_scratch:
            if self.rank == 0 and act.get('save_checkpoints', True):
                self.save_chkpnt()
        else:
            self.load_chkpnt()

        from dataloaders import Augmentation
        self.augmentation = Augmentation.from_config(config, self.rank)     # opt-in colour jitter + flip of the training batches
        if dataset is None:
            from dataloaders import UnSupKittiDataset
            dataset = UnSupKittiDataset(config, transforms=None)
        self.dataset = dataset
        if self.validation is not None and self.validation['scaling'] == 'ground' and not getattr(dataset, "calibration", False):
            raise ValueError("config validation.scaling: ground reads every frame's P_rect_02; set datasets.calibration: true")
        if self.augmentation is not None and not getattr(dataset, "raw", False):
            raise ValueError("config datasets.augmentation: color_jitter / flip run on the GPU loader's decoded bytes; this dataset gives "
                             "finished tensors")
        self.train_loader, self.validation_loader = self.create_loaders(act['random_seed'], act['split'][1])
        self.save_checkpoints = act.get('save_checkpoints', True)

    # ------------------------------------------------------------------ checkpoints (reference trainer.py:129-152)
    def save_chkpnt(self):
        os.makedirs(os.path.dirname(self.save_path), exist_ok=True)
        self.checkpoint = {'epoch': self.epoch, 'dpth_mdl_state_dict': self.depth_model.state_dict(),
                           'pose_mdl_state_dict': self.pose_model.state_dict(),
                           'optimizer_state_dict': self.model_optimizer.state_dict(), 'loss': self.loss, 'valid_acc': self.valid_acc}
        torch.save(self.checkpoint, self.save_path)

    def load_chkpnt(self):
        self.checkpoint = torch.load(self.save_path, map_location=self.device)
        self.depth_model.load_state_dict(self.checkpoint['dpth_mdl_state_dict'])
        self.pose_model.load_state_dict(self.checkpoint['pose_mdl_state_dict'])
        # reference trainer.py:148: Adam's moments and step count resume too (FusedAdam copies them into its flat buffers)
        self.model_optimizer.load_state_dict(self.checkpoint['optimizer_state_dict'])
        self.model_optimizer.arena().bump()          # the weights changed through load_state_dict: packed copies are stale
        self.epoch = self.checkpoint['epoch']
        self.valid_acc = self.checkpoint['valid_acc']

    def load_from_config(self, config, model_type='depth'):
        module = importlib.import_module('models.' + model_type + '.' + config['model'][model_type]['file'])
        model_name = config['model'][model_type]['name']
        model = None
        for name, obj in getmembers(module, isclass):
            if name == model_name:
                model = obj
        if model is None:
            raise ValueError("config: no class %s in models.%s.%s" % (model_name, model_type, config['model'][model_type]['file']))
        scales = config['model'][model_type].get('scales')
        if scales is None:
            model = model()
        else:                  # model.depth.scales: how many decoder scales the net returns in training (DispResNet(scales=n))
            import inspect
            if 'scales' not in inspect.signature(model.__init__).parameters:
                raise ValueError("config model.%s.scales: %s takes no `scales` argument" % (model_type, model_name))
            model = model(scales=int(scales))
        if self.train_from_scratch and model_type != 'depth':
            model.init_weights()
        return model.to(self.device)

    def create_loaders(self, random_seed, valid_split_ratio):
        indices = list(range(len(self.dataset)))
        split = int(np.floor(valid_split_ratio * len(indices)))
        if self.shuffle_dataset:
            np.random.seed(random_seed)
            np.random.shuffle(indices)
        train_indices, val_indices = indices[split:], indices[:split]
        train_indices = mdist.shard_indices(train_indices, self.rank, self.world)      # data parallel: disjoint slices
        if getattr(self.dataset, "raw", False):
            # file-backed samples decoded to uint8 on the host (worker processes); resize + normalise on the GPU, one batch ahead
            from dataloaders import PrefetchLoader, raw_collate
            native = bool(getattr(self.dataset, "native_gt", False))      # (datasets.groundtruth: native or velodyne)
            mk = lambda idx, drop, aug=None: PrefetchLoader(torch.utils.data.DataLoader(self.dataset, batch_size=self.batch_size,
                                                                                      sampler=SequentialIndicesSampler(idx),
                                                                                      num_workers=self.num_workers, drop_last=drop,
                                                                                      collate_fn=raw_collate),
                                                          self.dataset.img_height, self.dataset.img_width, self.device,
                                                          native_groundtruth=native, augment=aug)
            # the protocol scores every validation image; only the training batches are augmented
            return mk(train_indices, True, self.augmentation), mk(val_indices, self.validation is None)
        mk = lambda idx, drop: torch.utils.data.DataLoader(self.dataset, batch_size=self.batch_size, sampler=SequentialIndicesSampler(idx),
                                                           num_workers=self.num_workers, drop_last=drop, pin_memory=True)
        return mk(train_indices, True), mk(val_indices, self.validation is None)

    def set_train(self):
        self.depth_model.train()
        self.pose_model.train()

    def set_eval(self):
        self.depth_model.eval()
        self.pose_model.eval()

    # ------------------------------------------------------------------ the hot loop (reference trainer.py:242-313)
    def train(self):
        self.set_train()
        self.start_time = time.time()
        for self.epoch in range(self.num_epochs):
            self.run_epoch()

    def _graphed_step(self, samples):
        """action.hipgraph: the same step replayed as one captured hipGraph per input shape (mcav/graph.py).  On one rank the Adam update is
        inside the graph; with several ranks the bucketed all-reduce runs BESIDE the replay (each bucket behind an external event node of
        the graph) and Adam follows eagerly."""
        dev = self.device
        tgt = samples['tgt'].to(dev, non_blocking=True)
        ref_imgs = [img.to(dev, non_blocking=True) for img in samples['ref_imgs']]
        K = samples['intrinsics'].to(dev, non_blocking=True)
        aug = [samples['tgt_aug']] + list(samples['ref_imgs_aug']) if 'tgt_aug' in samples else []
        aug = [img.to(dev, non_blocking=True) for img in aug]          # augmentation: the networks' inputs, three more graph inputs
        st = [samples['stereo'], samples['stereo_baseline']] if 'stereo' in samples else []
        st = [t.to(dev, non_blocking=True) for t in st]                # mono + stereo: the frame and the baselines, two more graph inputs
        if self._graphs is None:
            from mcav.graph import StepGraphs
            naug = len(aug)

            def fwd_bwd(tgt, ref0, ref1, K, *extra):
                self.model_optimizer.zero_grad()
                aug, st = extra[:naug], extra[naug:]
                batch = {'tgt': tgt, 'ref_imgs': [ref0, ref1], 'intrinsics': K, 'groundtruth': None}
                if aug:
                    batch.update(tgt_aug=aug[0], ref_imgs_aug=[aug[1], aug[2]])
                if st:
                    batch.update(stereo=st[0], stereo_baseline=st[1])
                _, loss = self.process_batch(batch)
                sum(loss).backward()
                return tuple(loss)
            buffers = list(self.depth_model.buffers()) + list(self.pose_model.buffers())
            self._graphs = StepGraphs(fwd_bwd, self.model_optimizer, capture_adam=not mdist.parallel(), buffers=buffers)
        self.model_optimizer.grad_scale = 1.0 / self.world
        self.loss = list(self._graphs(tgt, ref_imgs[0], ref_imgs[1], K, *aug, *st))
        if mdist.parallel():      # the buckets' collectives are already in flight behind the replaying graph (mcav/graph.py); remainder, wait, Adam
            self.model_optimizer.grad_scale = mdist.allreduce_gradients(self.model_optimizer.arena())
            self.model_optimizer.step()
        self.step += 1
        return None, self.loss

    def train_step(self, samples):
        """zero_grad -> process_batch -> backward -> (all-reduce) -> Adam  (reference trainer.py:261-266)."""
        if self.use_hipgraph == 'auto':
            t = samples['tgt']
            self.use_hipgraph = bool(t.shape[0] * t.shape[-2] * t.shape[-1] <= 6 * 192 * 640)
            self._hipgraph_auto = True
        if self.use_hipgraph:
            if not getattr(self, "_hipgraph_auto", False):
                return self._graphed_step(samples)
            try:
                return self._graphed_step(samples)
            except Exception as e:       # "auto" must never cost a run: same launches, issued eagerly from now on
                import warnings
                warnings.warn("hipGraph capture failed (%s: %s); issuing the step eagerly" % (type(e).__name__, e))
                torch.cuda.synchronize()
                self.use_hipgraph, self._graphs = False, None
        self.model_optimizer.zero_grad()
        outputs, self.loss = self.process_batch(samples)
        sum(self.loss).backward()
        self.model_optimizer.grad_scale = mdist.allreduce_gradients(self.model_optimizer.arena())
        self.model_optimizer.step()
        self.step += 1
        return outputs, self.loss

    def run_epoch(self):
        if hasattr(self.train_loader, "set_epoch"):
            self.train_loader.set_epoch(self.epoch)      # the augmentation records are drawn for (seed, rank, epoch)
        for batch_indx, samples in enumerate(self.train_loader):
            self.train_step(samples)
            if self.step == 1:
                # the modules, descriptors and packed-weight tables live for the whole run: take them out of the cyclic collector's reach,
                # so that its full passes (~70 ms over this heap) do not stall the launch queue mid-epoch
                import gc
                gc.collect()
                gc.freeze()
            if self.verbose and self.rank == 0 and (batch_indx % max(1, self.log_freq) == 0):
                print("epoch %d batch %d loss %.6f" % (self.epoch, batch_indx, float(sum(self.loss).detach())))
        self.model_lr_scheduler.step()
        if self.rank == 0 and self.save_checkpoints:
            self.save_chkpnt()

    def process_batch(self, samples, warp_test=False, semi_sup_pose=False):
        dev = self.device
        tgt = samples['tgt'].to(dev, non_blocking=True)
        ref_imgs = [img.to(dev, non_blocking=True) for img in samples['ref_imgs']]
        intrinsics = samples['intrinsics'].to(dev, non_blocking=True)
        gt = samples['groundtruth']
        # augmented batches (PrefetchLoader with an Augmentation): the networks see the jittered frames, the loss the plain ones
        net_tgt = samples['tgt_aug'].to(dev, non_blocking=True) if 'tgt_aug' in samples else tgt
        net_refs = [img.to(dev, non_blocking=True) for img in samples['ref_imgs_aug']] if 'ref_imgs_aug' in samples else ref_imgs
        overlap = tgt.is_cuda and not semi_sup_pose
        if overlap:        # the pose net is independent of the depth net until the loss: second HIP stream (mcav/streams.py)
            from mcav import nn as mnn
            mnn.refresh_packed_weights(tgt.device)      # both streams read the packed filters: refresh them before the fork
            poses = self.pose_branch.fork(self.pose_model, net_tgt, net_refs)
        if hasattr(self.depth_model, "forward_pair"):
            disps = list(self.depth_model.forward_pair(net_tgt, net_refs[0]))          # == two separate passes (per-pass BN statistics)
        else:
            disps = [self.depth_model(image_t) for image_t in (net_tgt, net_refs[0])]  # two separate passes, as the reference
        if semi_sup_pose:
            poses = torch.cat((samples["oxts"][0].unsqueeze(1), samples["oxts"][1].unsqueeze(1)), 1).to(dev)
        elif overlap:
            poses = self.pose_branch.join(poses)
        else:
            poses = self.pose_model(net_tgt, net_refs)
        if warp_test:
            return [disps, poses]
        st = {}
        if 'stereo' in samples:       # mono + stereo (loss.stereo): the target's stereo frame and its baseline join the loss only
            st = dict(stereo=samples['stereo'].to(dev, non_blocking=True), stereo_baseline=samples['stereo_baseline'].to(dev, non_blocking=True))
        loss = self.criterion.forward(tgt, ref_imgs, disps, poses, intrinsics, gt, **st)
        return [disps, poses], loss

    VALIDATION_DEFAULTS = {'protocol': 'eigen', 'crop': 'garg', 'min_depth': 1e-3, 'max_depth': 80.0, 'median_scaling': True, 'scale': 1.0,
                           'scaling': None, 'camera_height': 1.65}

    @classmethod
    def validation_config(cls, cfg):
        """The top-level config key `validation` (None: validate() keeps the reference's per-batch compute_errors).  Its keys and defaults:
        protocol: eigen, crop: garg (or eigen, or null = whole image), min_depth: 1e-3, max_depth: 80, median_scaling: true, scale: 1.0,
        scaling: median | ground | none (median and none are median_scaling true and false; ground scores the prediction at the metric scale
        pseudo_lidar.ground_scale estimates from it, without median scaling, and needs datasets.calibration: true), camera_height: 1.65."""
        if cfg is None:
            return None
        unknown = set(cfg) - set(cls.VALIDATION_DEFAULTS)
        if unknown:
            raise ValueError("config validation: unknown keys %s (known: %s)" % (sorted(unknown), sorted(cls.VALIDATION_DEFAULTS)))
        v = dict(cls.VALIDATION_DEFAULTS, **cfg)
        if v['protocol'] != 'eigen':
            raise ValueError("config validation.protocol: only 'eigen' (monodepth2's KITTI protocol) is implemented, got %r" % (v['protocol'],))
        if v['crop'] not in ('garg', 'eigen', None):
            raise ValueError("config validation.crop must be garg, eigen or null, got %r" % (v['crop'],))
        v['min_depth'], v['max_depth'], v['scale'] = float(v['min_depth']), float(v['max_depth']), float(v['scale'])
        v['median_scaling'] = bool(v['median_scaling'])
        if v['scaling'] is None:
            v['scaling'] = 'median' if v['median_scaling'] else 'none'
        if v['scaling'] not in ('median', 'ground', 'none'):
            raise ValueError("config validation.scaling must be median, ground or none, got %r" % (v['scaling'],))
        if 'median_scaling' in cfg and cfg.get('scaling') is not None and v['median_scaling'] != (v['scaling'] == 'median'):
            raise ValueError("config validation: scaling: %s contradicts median_scaling: %s; give one of the two keys"
                             % (v['scaling'], str(v['median_scaling']).lower()))
        v['median_scaling'] = v['scaling'] == 'median'
        v['camera_height'] = float(v['camera_height'])
        if not v['camera_height'] > 0:
            raise ValueError("config validation.camera_height must be positive, got %r" % (v['camera_height'],))
        return v

    @torch.no_grad()
    def validate_protocol(self):
        """validate() with the `validation` key: the KITTI protocol (evaluate.evaluate_depth) over the WHOLE validation loader.  Only the
        depth network runs, in eval mode, on 'tgt'; the per-image rows stay on the device and are reduced with one read-back."""
        from evaluate import eval_depth_rows, reduce_rows
        v = self.validation
        self.depth_model.eval()
        rows, ground = [], []
        try:
            for samples in self.validation_loader:
                if 'groundtruth_size' not in samples:
                    raise ValueError("validation: the KITTI protocol needs the native ground truth (datasets.groundtruth: native or velodyne with "
                                     "a KITTI split); this loader gives ground truth resized to the network's input")
                tgt = samples['tgt'].to(self.device, non_blocking=True)
                gt = samples['groundtruth'].to(self.device, non_blocking=True)
                pred, scales = self.depth_model(tgt), None
                if v['scaling'] == 'ground':
                    from pseudo_lidar import ground_scale
                    disp = pred[0] if isinstance(pred, (list, tuple)) else pred
                    ground.append(ground_scale(disp.detach().to(torch.float32), sizes=samples['native_size'], P=samples['P_rect'],
                                               camera_height=v['camera_height']).rows)
                    scales = ground[-1][:, 0]
                rows.append(eval_depth_rows(gt, pred, samples['groundtruth_size'], v['crop'], v['min_depth'], v['max_depth'],
                                            v['median_scaling'], v['scale'], scales))
        finally:
            self.set_train()
        return reduce_rows(rows, ground if v['scaling'] == 'ground' else None)

    @torch.no_grad()
    def validate(self):
        if self.validation is not None:
            return self.validate_protocol()
        from evaluate import compute_errors
        self.set_eval()
        acc = None
        for samples in self.validation_loader:
            outputs = self.process_batch(samples, warp_test=True)
            # reference trainer.py:325-329: compute_errors(gt, outputs[0]); the ground truth goes to the GPU, pixels without one are skipped
            gt = samples['groundtruth'].to(self.device, non_blocking=True)
            acc = compute_errors(gt, outputs[0][0], min_gt=1e-3)
        self.set_train()
        return acc
