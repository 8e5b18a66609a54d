"""inference.py -- from a checkpoint and a KITTI split to pseudo-LiDAR clouds on disk (the reference's inference.py stops at a plot).

    inf = Inference(config, checkpoint="pretrained/model.pth")
    disp = inf.disparity(images)                       # [B, 1, h, w], evaluation mode, no gradients
    cb = inf.clouds(samples, beams=beam_tables())      # a pseudo_lidar.CloudBatch for one loader batch
    pb = inf.pillars(samples, max_points=32)           # a pseudo_lidar.PillarBatch: what a LiDAR 3-D detector reads
    img = inf.pseudo_images(samples, pfn)              # [B, C_out, ny, nx]: what the detector's convolutional backbone reads
    det = inf.detections(samples, pfn, head)           # a pseudo_lidar.DetectionBatch: head(img) -> (boxes, scores) -> rotated NMS
    n = inf.export("out")                              # out/<date>/<drive>/pseudo_velodyne/data/<frame>.bin for every frame of the split

    python inference.py --config C --checkpoint X --out DIR [--beams NB NA] [--scale S | --scale ground] [--max-depth D]
                        [--camera-height M] [--ground-angle DEG] [--ground-min N]
                        [--pillars [--pillar-size VX VY] [--pillar-points N] [--pillar-range X0 X1 Y0 Y1 Z0 Z1]
                         [--pfn CHECKPOINT [--pfn-prefix P]]]
                        [--gdc [--gdc-beams 5 7 9 11] [--gdc-iters 400] [--gdc-k 10] [--gdc-radius 3]]

--gdc corrects every frame's depth map against a few beams of its own Velodyne scan before the cloud is made (Pseudo-LiDAR++'s
graph-based depth correction, pseudo_lidar.gdc): disparity -> depth (times the chosen scale, `ground` included) -> gdc against the
scan thinned to --gdc-beams of its 64 -> project_batch(input="depth").  It needs datasets.groundtruth: velodyne.

--pillars also writes out/<date>/<drive>/pseudo_pillars/data/<frame>.npz (voxels [P, N, 4], coords [P, 4] = (image in its batch, 0, iy,
ix), num_points [P]) beside every .bin: the cloud voxelised on the GPU (pseudo_lidar.pillarize; default PointPillars' KITTI grid).
--pfn CHECKPOINT reads a detector's pillar feature net from it (pseudo_lidar.PillarFeatureNet.from_state_dict: `linear.weight` and the
BatchNorm `norm.*` under --pfn-prefix, 4 input columns; the state dict itself or under `model_state` / `state_dict`) and adds features
[P, C_out] to every .npz; the dense pseudo-image (55 MB a frame) is not written.

--scale ground gives every frame its own metric scale from its ground plane (pseudo_lidar.ground_scale: no ground truth, no stereo); a
frame without enough ground pixels gets an empty cloud.

Only the depth network is built (as Trainer.load_from_config builds it); no pose net, no optimiser.  The loader runs with
datasets.calibration, so every batch carries its frames' P_rect_02, velodyne -> camera transform, native size and path; the clouds are
made by PseudoLiDAR.project_batch at the native resolution (one kernel sequence and, in export, one read-back per batch)."""
import argparse
import importlib
import os
from inspect import getmembers, isclass

import numpy as np
import torch
import yaml

from pseudo_lidar import PillarFeatureNet, PillarGrid, PseudoLiDAR, beam_tables, gdc as gdc_correct, ground_scale, nms as box_nms


class Inference:
    def __init__(self, config, checkpoint=None, dataset=None):
        if not torch.cuda.is_available():
            raise RuntimeError("Inference: the MI355X path needs a GPU (there is no CPU fallback)")
        self.config = config
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.depth_model = self.load_from_config(config)
        if checkpoint is not None:
            state = torch.load(checkpoint, map_location=self.device)
            self.depth_model.load_state_dict(state['dpth_mdl_state_dict'])
        self.depth_model.eval()
        self.dataset = dataset
        self.projector = PseudoLiDAR.from_matrices(np.eye(4), np.eye(3, 4), 0)     # every call brings its frames' own calibration

    def load_from_config(self, config):
        """The depth model of Trainer.load_from_config"""
        spec = config['model']['depth']
        module = importlib.import_module('models.depth.' + spec['file'])
        model = dict(getmembers(module, isclass)).get(spec['name'])
        if model is None:
            raise ValueError("config: no class %s in models.depth.%s" % (spec['name'], spec['file']))
        scales = spec.get('scales')
        if scales is None:
            return model().to(self.device)
        import inspect
        if 'scales' not in inspect.signature(model.__init__).parameters:
            raise ValueError("config model.depth.scales: %s takes no `scales` argument" % spec['name'])
        return model(scales=int(scales)).to(self.device)

    @torch.no_grad()
    def disparity(self, images):
        """images [B, 3, h, w] (normalised, as the loader gives 'tgt') -> the sigmoid disparity [B, 1, h, w]"""
        self.depth_model.eval()
        out = self.depth_model(images.to(self.device, non_blocking=True))
        return out[0] if isinstance(out, (list, tuple)) else out

    @torch.no_grad()
    def clouds(self, samples, gdc=None, **kw):
        """One batch of a datasets.calibration loader -> CloudBatch.  kw: PseudoLiDAR.project_batch's (scale -- a number, a tensor [B] or
        "ground" with its keywords in ground={...} --, max_height, max_depth, beams, intensity, out).  gdc: None, or a dict of
        pseudo_lidar.gdc's keywords plus `beams` (the beams of the 64 to keep of every frame's scan, default (5, 7, 9, 11)): the depth map
        is corrected against the thinned scan before it is projected (corrected_depth)."""
        for key in ('P_rect', 'T_velo_cam', 'native_size'):
            if key not in samples:
                raise ValueError("Inference.clouds: the batch has no %r; build the dataset with datasets.calibration: true" % key)
        if gdc is None:
            return self.projector.project_batch(self.disparity(samples['tgt']), sizes=samples['native_size'], P=samples['P_rect'],
                                                T=samples['T_velo_cam'], **kw)
        scale, ground = kw.pop('scale', 1.0), kw.pop('ground', None)
        depth = self.corrected_depth(samples, gdc, scale=scale, ground=ground).depth
        return self.projector.project_batch(depth, sizes=samples['native_size'], P=samples['P_rect'], T=samples['T_velo_cam'],
                                            input="depth", **kw)

    @torch.no_grad()
    def corrected_depth(self, samples, gdc, scale=1.0, ground=None):
        """disparity -> depth = scale / (10 disp + 0.01) (scale: a number, a tensor [B] or "ground" with ground={...}) -> pseudo_lidar.gdc
        against each frame's scan thinned to gdc['beams'] and projected onto the network's grid -> GDCResult.  The scans are read from
        <drive>/velodyne_points/data beside each frame, so the dataset must be built with datasets.groundtruth: velodyne (which checks
        that they exist) and datasets.calibration: true."""
        from geometry import velodyne
        ds = self.dataset
        if ds is None or not getattr(ds, "velodyne_gt", False) or 'path' not in samples:
            raise ValueError("Inference: gdc needs every frame's Velodyne scan and calibration; build the dataset with "
                             "datasets.groundtruth: velodyne and datasets.calibration: true")
        opts = dict(gdc)
        beams = tuple(opts.pop('beams', (5, 7, 9, 11)))
        disp = self.disparity(samples['tgt'])[:, 0]
        B, h, w = disp.shape
        sizes = samples['native_size']
        if isinstance(scale, str):
            if scale != "ground":
                raise ValueError("Inference: scale must be a number, a tensor [B] or 'ground', got %r" % (scale,))
            scale = ground_scale(disp, sizes=sizes, P=samples['P_rect'], **dict(ground or {})).scales
        depth = 1.0 / (10.0 * disp + 0.01)
        depth = depth * (scale.to(depth.device).view(B, 1, 1) if torch.is_tensor(scale) else float(scale))
        scans, Ps = [], []
        for path in samples['path']:
            scans.append(velodyne.select_beams(velodyne.load_velodyne_points(ds.resolve(ds.velodyne_scan(path))), beams))
            Ps.append(ds.velo_calib_of(path)[0])
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
        points = torch.from_numpy(np.concatenate(scans).astype(np.float32).reshape(-1, 4))
        sparse = velodyne.sparse_maps(points, offsets, np.stack(Ps), sizes, h, w, device=self.device)
        return gdc_correct(depth.contiguous(), sparse.contiguous(), P=samples['P_rect'], sizes=sizes, **opts)

    @torch.no_grad()
    def pillars(self, samples, grid=None, max_points=32, decorate=False, **cloud_kw):
        """One batch of a datasets.calibration loader -> PillarBatch: clouds(samples, **cloud_kw), voxelised on the device
        (pseudo_lidar.pillarize).  The CloudBatch stays reachable as `.cloud`."""
        cloud = self.clouds(samples, **cloud_kw)
        pb = cloud.pillars(grid=grid, max_points=max_points, decorate=decorate)
        pb.cloud = cloud
        return pb

    @torch.no_grad()
    def occupancy(self, samples, grid=None, sigma2=0.01, **cloud_kw):
        """One batch of a datasets.calibration loader -> the soft-occupancy canvas [B, nz, ny, nx] of clouds(samples, **cloud_kw)
        (pseudo_lidar.occupancy; default PIXOR's 700 x 800 x 35 grid).  Nothing is read back, and nothing is written to disk: a canvas
        is 78 MB per frame."""
        return self.clouds(samples, **cloud_kw).occupancy(grid=grid, sigma2=sigma2)

    @torch.no_grad()
    def pseudo_images(self, samples, pfn, layout="nchw", **pillar_kw):
        """One batch of a datasets.calibration loader -> [B, C_out, ny, nx]: pillars(samples, **pillar_kw) through the PillarFeatureNet
        `pfn` into the bird's-eye-view pseudo-image (pseudo_lidar.PillarFeatureNet.pseudo_image).  Nothing is read back."""
        return pfn.pseudo_image(self.pillars(samples, **pillar_kw), layout=layout)

    @torch.no_grad()
    def detections(self, samples, net, head, pillar_kw=None, **nms_kw):
        """One batch of a datasets.calibration loader -> DetectionBatch: pseudo_images(samples, net, **pillar_kw) -> head(canvas) ->
        pseudo_lidar.nms(boxes, scores, **nms_kw).  net: the PillarFeatureNet; head: the caller's backbone and detection head, a callable
        that takes the canvas [B, C_out, ny, nx] and returns (boxes [B, A, 7], scores [B, A] or [B, A, K]) on the GPU, decoded.  Nothing
        is read back."""
        boxes, scores = head(self.pseudo_images(samples, net, **dict(pillar_kw or {})))
        return box_nms(boxes, scores, **nms_kw)

    def loader(self):
        """Every frame of the split, in order, with its calibration"""
        from dataloaders import PrefetchLoader, UnSupKittiDataset, raw_collate
        if self.dataset is None:
            cfg = dict(self.config, datasets=dict(self.config['datasets'], calibration=True))
            self.dataset = UnSupKittiDataset(cfg, transforms=None)
        if not getattr(self.dataset, "calibration", False):
            raise ValueError("Inference: the dataset must be built with datasets.calibration: true")
        act = self.config['action']
        dl = torch.utils.data.DataLoader(self.dataset, batch_size=act['batch_size'], shuffle=False, num_workers=act.get('num_workers', 0),
                                         drop_last=False, collate_fn=raw_collate)
        return PrefetchLoader(dl, self.dataset.img_height, self.dataset.img_width, self.device,
                              native_groundtruth=bool(getattr(self.dataset, "native_gt", False)))

    @staticmethod
    def _frame_path(out_dir, image_path, folder, ext):
        parts = os.path.normpath(image_path).split(os.sep)
        if len(parts) < 5 or parts[-2] != "data":
            raise ValueError("Inference.export: %r is not a KITTI raw frame (<date>/<drive>/image_02/data/<frame>.png)" % image_path)
        return os.path.join(out_dir, parts[-5], parts[-4], folder, "data", os.path.splitext(parts[-1])[0] + ext)

    @staticmethod
    def cloud_path(out_dir, image_path):
        """<out_dir>/<date>/<drive>/pseudo_velodyne/data/<frame>.bin of .../<date>/<drive>/image_02/data/<frame>.png"""
        return Inference._frame_path(out_dir, image_path, "pseudo_velodyne", ".bin")

    @staticmethod
    def pillar_path(out_dir, image_path):
        """<out_dir>/<date>/<drive>/pseudo_pillars/data/<frame>.npz of .../<date>/<drive>/image_02/data/<frame>.png"""
        return Inference._frame_path(out_dir, image_path, "pseudo_pillars", ".npz")

    def export(self, out_dir, loader=None, pillars=None, pfn=None, **kw):
        """Writes one KITTI .bin (float32 x y z i) per frame of the split and returns the number of frames.  pillars: None, or a dict of
        pillarize's keywords (grid, max_points, decorate; {} for the defaults): every frame's .npz of voxels, coords and num_points is
        written too, at the cost of one more read-back of offsets and one of the used rows per batch.  pfn: a PillarFeatureNet whose
        features [P, C_out] of every frame's pillars go into the .npz as well (needs pillars)."""
        if pfn is not None and pillars is None:
            raise ValueError("Inference.export: pfn needs pillars")
        n = 0
        for samples in (self.loader() if loader is None else loader):
            paths = [self.cloud_path(out_dir, p) for p in samples['path']]
            for p in paths:
                os.makedirs(os.path.dirname(p), exist_ok=True)
            cloud = self.clouds(samples, **kw)
            cloud.save_bin(paths)
            if pillars is not None:
                npz = [self.pillar_path(out_dir, p) for p in samples['path']]
                for p in npz:
                    os.makedirs(os.path.dirname(p), exist_ok=True)
                pb = cloud.pillars(**pillars)
                if pfn is None:
                    pb.save_npz(npz)
                else:
                    pb.save_npz(npz, features=pfn.features(pb))
            n += len(paths)
        return n


def scale_argument(text):
    """--scale: a number or the word 'ground'"""
    return "ground" if text.strip().lower() == "ground" else float(text)


def pillar_arguments(args):
    """--pillars and its options -> export's `pillars` (None without the flag); a bad grid is refused before anything is loaded"""
    if not args.pillars:
        return None
    r = args.pillar_range
    return dict(grid=PillarGrid(x=(r[0], r[1]), y=(r[2], r[3]), z=(r[4], r[5]), size=tuple(args.pillar_size)), max_points=args.pillar_points)


def pfn_arguments(args):
    """--pfn and --pfn-prefix -> (checkpoint, prefix), None without the flag; --pfn without --pillars is refused before anything is loaded"""
    if args.pfn is None:
        return None
    if not args.pillars:
        raise ValueError("--pfn needs --pillars")
    return args.pfn, args.pfn_prefix


def load_pfn(checkpoint, prefix, grid, device):
    """The PillarFeatureNet of a detector checkpoint: the state dict itself, or the one under `model_state` (OpenPCDet) / `state_dict`"""
    sd = torch.load(checkpoint, map_location="cpu")
    for key in ("model_state", "state_dict"):
        if isinstance(sd, dict) and key in sd and prefix + "linear.weight" not in sd:
            sd = sd[key]
    return PillarFeatureNet.from_state_dict(sd, prefix=prefix, grid=grid, device=device)


def gdc_arguments(args):
    """--gdc and its options -> clouds' `gdc` (None without the flag)"""
    if not args.gdc:
        return None
    return dict(beams=tuple(args.gdc_beams), iters=args.gdc_iters, k=args.gdc_k, radius=args.gdc_radius)


def build_parser():
    ap = argparse.ArgumentParser(description="checkpoint + KITTI split -> pseudo-LiDAR .bin clouds")
    ap.add_argument("--config", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--beams", nargs=2, type=int, metavar=("NB", "NA"), help="one return per cell of an NB x NA beam grid (default: dense)")
    ap.add_argument("--scale", type=scale_argument, default=1.0,
                    help="a number that multiplies the depth (pred_depth_scale_factor), or 'ground': every frame's own scale from its ground plane")
    ap.add_argument("--max-depth", type=float, default=None)
    ap.add_argument("--camera-height", type=float, default=1.65, help="--scale ground: the camera above the road in metres")
    ap.add_argument("--ground-angle", type=float, default=5.0, help="--scale ground: the cone around 'down' a ground normal lies in, degrees")
    ap.add_argument("--ground-min", type=int, default=100, help="--scale ground: fewer ground pixels than this and the frame gets no cloud")
    ap.add_argument("--pillars", action="store_true", help="also write <date>/<drive>/pseudo_pillars/data/<frame>.npz: the cloud voxelised")
    ap.add_argument("--pillar-size", nargs=2, type=float, default=(0.16, 0.16), metavar=("VX", "VY"), help="--pillars: a pillar in metres")
    ap.add_argument("--pillar-points", type=int, default=32, help="--pillars: the points kept per pillar (1..64), the first in cloud order")
    ap.add_argument("--pillar-range", nargs=6, type=float, default=(0.0, 69.12, -39.68, 39.68, -3.0, 1.0),
                    metavar=("X0", "X1", "Y0", "Y1", "Z0", "Z1"), help="--pillars: the grid's extent in the velodyne frame, metres")
    ap.add_argument("--pfn", default=None, metavar="CHECKPOINT",
                    help="--pillars: a detector checkpoint whose pillar feature net adds features [P, C_out] to every .npz")
    ap.add_argument("--pfn-prefix", default="vfe.pfn_layers.0.", metavar="P", help="--pfn: where the layer sits in the state dict")
    ap.add_argument("--gdc", action="store_true",
                    help="correct every depth map against a few beams of the frame's Velodyne scan (needs datasets.groundtruth: velodyne)")
    ap.add_argument("--gdc-beams", nargs="+", type=int, default=(5, 7, 9, 11), help="--gdc: the beams of the scan's 64 that are kept")
    ap.add_argument("--gdc-iters", type=int, default=400, help="--gdc: conjugate-gradient iterations at most")
    ap.add_argument("--gdc-k", type=int, default=10, help="--gdc: neighbours per pixel (1..16)")
    ap.add_argument("--gdc-radius", type=int, default=3, help="--gdc: the neighbours come from a (2 r + 1)^2 pixel window (1..7)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    pillars = pillar_arguments(args)
    pfn = pfn_arguments(args)
    gdc = gdc_arguments(args)
    with open(args.config) as f:
        config = yaml.full_load(f)
    if gdc is not None:
        ds = config.get('datasets', {})
        if ds.get('groundtruth') != 'velodyne' or not ds.get('calibration'):
            raise ValueError("--gdc needs every frame's Velodyne scan and calibration: set datasets.groundtruth: velodyne and "
                             "datasets.calibration: true in %s" % args.config)
    kw = dict(scale=args.scale, max_depth=args.max_depth)
    if args.scale == "ground":
        kw["ground"] = dict(camera_height=args.camera_height, max_angle_deg=args.ground_angle, min_ground=args.ground_min)
    if args.beams:
        kw["beams"] = beam_tables(args.beams[0], args.beams[1])
    if gdc is not None:
        kw["gdc"] = gdc
    inf = Inference(config, args.checkpoint)
    if pfn is not None:
        kw["pfn"] = load_pfn(pfn[0], pfn[1], pillars["grid"], inf.device)
    n = inf.export(args.out, pillars=pillars, **kw)
    print("wrote %d clouds%s under %s" % (n, " and their pillars" if pillars is not None else "", args.out))


if __name__ == "__main__":
    main()
