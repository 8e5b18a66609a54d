"""dataloaders.py -- sample source for the trainer.

The reference's KITTI loader (dataloaders.py:14-252) is PIL decode + a torchvision transform chain + calib/oxts parsing.  Built here:
the split-file driven reader (UnSupKittiFiles: paths, P_rect_02 intrinsics, ground-truth maps; tested on a generated KITTI-shaped
tree, KITTI itself is not available offline), the transform chain on the GPU (GpuImageTransform: SURVEY.md section 8f "next" row 1) and
the one-batch-ahead PrefetchLoader that joins them.  Not built: the OXTS pose packets of the semi-supervised experiment.  What the
training step consumes is kept: a dict with 'tgt' [3,H,W], 'ref_imgs' [2 x [3,H,W]], 'intrinsics' [3,3] fp64,
'groundtruth' [1,H,W] (reference dataloaders.py:226-251).  SyntheticTriplets produces such samples from a seed.
`datasets.groundtruth: native` (opt-in, for evaluate.evaluate_depth): the ground truth stays at its own size, in metres, and PrefetchLoader
zero-pads each batch to its largest map and adds 'groundtruth_size' [B,2] int32 (host).  The loss never reads the ground truth.
`datasets.groundtruth: velodyne` (opt-in): the same native layout, but each map is made on the GPU from the frame's raw Velodyne scan
(<drive>/velodyne_points/data/<frame>.bin), as monodepth2's Eigen-split ground truth (geometry.velodyne.depth_maps).
`datasets.augmentation.color_jitter` / `.flip` (opt-in, Augmentation): monodepth2's training-time colour jitter and horizontal flip, on the
GPU with the resize; the training batches then also carry 'tgt_aug', 'ref_imgs_aug' (what the networks see) and 'augment_records'.
"""
import ctypes

import numpy as np
import torch
from torch.utils.data import Dataset

from geometry import velodyne


class GpuImageTransform:
    """The reference's transform chain (trainer.py:97-103 applied by dataloaders.py:32-49 load_img) on the GPU, for batches of
    decoded uint8 RGB images: /255, ToPILImage, Resize((h, w)) -- Pillow's antialiased bilinear resample, reproduced bit for bit --,
    ToTensor, Normalize(ImageNet).  Decoding the file stays on the host (PIL); one pinned copy brings the bytes over.

        t = GpuImageTransform(192, 640)
        x = t(torch.from_numpy(np.asarray(Image.open(path))))         # [H0, W0, 3] uint8 -> [3, 192, 640] float32 on the GPU
        K = t.scale_intrinsics(K, og_h, og_w)                         # dataloaders.py:95-98, on a copy
    """
    MEAN = (0.485, 0.456, 0.406)
    STD = (0.229, 0.224, 0.225)

    def __init__(self, img_height, img_width, device="cuda"):
        self.h, self.w, self.device = int(img_height), int(img_width), torch.device(device)
        self._tables = {}

    def _axis(self, in_size, out_size):
        from mcav import lib as L
        key = (in_size, out_size)
        if key not in self._tables:
            h = L.lib()
            ks = ctypes.c_int(0)
            cap = h.mcav_resample_coeffs(in_size, out_size, ctypes.byref(ks), None, None, 0)
            if cap <= 0:
                raise L.MCAVError("mcav_resample_coeffs: cannot resample %d -> %d" % (in_size, out_size))
            bounds = np.zeros(out_size * 2, np.int32)
            kk = np.zeros(cap, np.int32)
            L.check(h.mcav_resample_coeffs(in_size, out_size, ctypes.byref(ks), bounds.ctypes.data_as(ctypes.c_void_p),
                                           kk.ctypes.data_as(ctypes.c_void_p), cap), "mcav_resample_coeffs")
            self._tables[key] = (torch.from_numpy(bounds).to(self.device), torch.from_numpy(kk).to(self.device), ks.value)
        return self._tables[key]

    def __call__(self, img_u8):
        """img_u8: uint8 [H0, W0, 3] or [B, H0, W0, 3] (host or device).  -> float32 [3, h, w] / [B, 3, h, w] on the device."""
        from mcav import lib as L
        single = img_u8.dim() == 3
        x = img_u8.unsqueeze(0) if single else img_u8
        if x.dtype != torch.uint8 or x.shape[-1] != 3:
            raise L.MCAVError("GpuImageTransform: expected uint8 [..., H, W, 3], got %s %s" % (x.dtype, tuple(x.shape)))
        if not x.is_cuda:
            x = x.contiguous().pin_memory().to(self.device, non_blocking=True)
        x = x.contiguous()
        B, H0, W0, _ = x.shape
        hb, hk, hks = self._axis(W0, self.w)
        vb, vk, vks = self._axis(H0, self.h)
        h = L.lib()
        ws = L.workspace(h.mcav_image_preprocess_workspace_bytes(B, H0, self.w), x.device, "preprocess")
        out = torch.empty((B, 3, self.h, self.w), dtype=torch.float32, device=x.device)
        mean = (ctypes.c_float * 3)(*self.MEAN)
        std = (ctypes.c_float * 3)(*self.STD)
        L.check(h.mcav_image_preprocess(L.ptr(x), B, H0, W0, self.h, self.w, L.ptr(hb), L.ptr(hk), hks, L.ptr(vb), L.ptr(vk), vks, mean, std,
                                        L.ptr(out), L.ptr(ws), ws.numel(), L.stream()), "mcav_image_preprocess")
        return out[0] if single else out

    def augmented(self, img_u8, records):
        """The same chain plus a per-frame flip and colour jitter (Augmentation; include/mcav_depth.h: mcav_image_preprocess_augment).
        img_u8: uint8 [B, H0, W0, 3]; records: B host records (AUGMENT_RECORD).  -> (plain, aug) float32 [B, 3, h, w] on the device: plain is
        __call__'s output, mirrored where the record flips; aug is what the networks see."""
        from mcav import lib as L
        x = img_u8
        if x.dim() != 4 or x.dtype != torch.uint8 or x.shape[-1] != 3:
            raise L.MCAVError("GpuImageTransform.augmented: expected uint8 [B, H, W, 3], got %s %s" % (x.dtype, tuple(x.shape)))
        records = np.ascontiguousarray(records, dtype=AUGMENT_RECORD)
        if records.shape != (x.shape[0],):
            raise L.MCAVError("GpuImageTransform.augmented: %d frames but %s records" % (x.shape[0], records.shape))
        if not x.is_cuda:
            x = x.contiguous().pin_memory().to(self.device, non_blocking=True)
        x = x.contiguous()
        rec = torch.from_numpy(records.view(np.uint8)).pin_memory().to(x.device, non_blocking=True)
        B, H0, W0, _ = x.shape
        hb, hk, hks = self._axis(W0, self.w)
        vb, vk, vks = self._axis(H0, self.h)
        h = L.lib()
        ws = L.workspace(h.mcav_image_augment_workspace_bytes(B, H0, self.h, self.w), x.device, "augment")
        plain = torch.empty((B, 3, self.h, self.w), dtype=torch.float32, device=x.device)
        aug = torch.empty_like(plain)
        mean = (ctypes.c_float * 3)(*self.MEAN)
        std = (ctypes.c_float * 3)(*self.STD)
        L.check(h.mcav_image_preprocess_augment(L.ptr(x), B, H0, W0, self.h, self.w, L.ptr(hb), L.ptr(hk), hks, L.ptr(vb), L.ptr(vk), vks,
                                                mean, std, L.ptr(rec), L.ptr(plain), L.ptr(aug), L.ptr(ws), ws.numel(), L.stream()),
                "mcav_image_preprocess_augment")
        return plain, aug

    def scale_intrinsics(self, K, og_h, og_w):
        """dataloaders.py:95-98 -- on a COPY: the reference scales the cached sample's matrix in place on every fetch."""
        K = torch.as_tensor(K, dtype=torch.float64).clone()
        K[0] *= self.w / og_w
        K[1] *= self.h / og_h
        return K


def _register():
    from mcav import lib as L
    L.register({
        "mcav_resample_coeffs": (L.c_i, [L.c_i, L.c_i, L.c_p, L.c_p, L.c_p, L.c_i]),
        "mcav_image_preprocess_workspace_bytes": (L.c_sz, [L.c_i, L.c_i, L.c_i]),
        "mcav_image_preprocess": (L.c_i, [L.c_p, L.c_i, L.c_i, L.c_i, L.c_i, L.c_i, L.c_p, L.c_p, L.c_i, L.c_p, L.c_p, L.c_i, L.c_p, L.c_p, L.c_p,
                                          L.c_p, L.c_sz, L.c_p]),
        "mcav_image_augment_workspace_bytes": (L.c_sz, [L.c_i, L.c_i, L.c_i, L.c_i]),
        "mcav_image_preprocess_augment": (L.c_i, [L.c_p, L.c_i, L.c_i, L.c_i, L.c_i, L.c_i, L.c_p, L.c_p, L.c_i, L.c_p, L.c_p, L.c_i, L.c_p,
                                                  L.c_p, L.c_p, L.c_p, L.c_p, L.c_p, L.c_sz, L.c_p]),
    })


_register()


# ------------------------------------------------------------------------------------------------ training-time augmentation (monodepth2)
AUGMENT_RECORD = np.dtype([("flags", "<i4"), ("order", "u1", (4,)), ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"),
                           ("hue_shift", "<i4")])          # include/mcav_depth.h: mcav_augment_record
AUG_FLIP, AUG_COLOUR = 1, 2
AUG_OP_NONE = 255


class Augmentation:
    """monodepth2's training-time augmentation: a horizontal flip with probability p_flip and torchvision's ColorJitter (brightness,
    contrast, saturation from U[max(0, 1 - x), 1 + x], hue from U[-x, x], in a random order) with probability p_color, one record per sample
    for all its frames.  The networks see the augmented frames, the loss the plain ones (mirrored with the flip).

    Records are drawn on the host from Generator(PCG64(SeedSequence([seed, rank, epoch]))) in batch order, ten uniforms per sample whatever
    the probabilities: the stream depends on (seed, rank, epoch) only, not on num_workers, and a resumed epoch draws it again.
    A jitter range of 0 leaves its operation out (torchvision passes None then); the flip of the intrinsics is PrefetchLoader's."""
    JITTER_DEFAULTS = {'brightness': 0.2, 'contrast': 0.2, 'saturation': 0.2, 'hue': 0.1, 'p': 0.5}
    CONFIG_KEYS = ('image_width', 'image_height', 'shuffle', 'color_jitter', 'flip')

    def __init__(self, brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1, p_color=0.5, p_flip=0.5, seed=0, rank=0):
        self.brightness, self.contrast, self.saturation, self.hue = float(brightness), float(contrast), float(saturation), float(hue)
        self.p_color, self.p_flip, self.seed, self.rank = float(p_color), float(p_flip), int(seed), int(rank)
        for name in ('brightness', 'contrast', 'saturation', 'hue'):
            v = getattr(self, name)
            if not np.isfinite(v) or v < 0:
                raise ValueError("augmentation: color_jitter.%s must be a finite number >= 0, got %r" % (name, v))
        if self.hue > 0.5:
            raise ValueError("augmentation: color_jitter.hue must be at most 0.5, got %r" % (self.hue,))
        for name in ('p_color', 'p_flip'):
            v = getattr(self, name)
            if not 0.0 <= v <= 1.0:
                raise ValueError("augmentation: probability %s must lie in [0, 1], got %r" % (name, v))

    @classmethod
    def from_config(cls, config, rank=0):
        """datasets.augmentation.color_jitter {brightness, contrast, saturation, hue, p} and datasets.augmentation.flip (a probability).
        None when neither key is there: the loader then behaves as before.  A key left out of color_jitter takes monodepth2's value; with only
        one of the two keys, the other operation is off."""
        aug = config['datasets']['augmentation']
        unknown = set(aug) - set(cls.CONFIG_KEYS)
        if unknown:
            raise ValueError("config datasets.augmentation: unknown keys %s (known: %s)" % (sorted(unknown), list(cls.CONFIG_KEYS)))
        if 'color_jitter' not in aug and 'flip' not in aug:
            return None
        if config['datasets'].get('dataset', ['KITTI']) == ['synthetic']:
            raise ValueError("config datasets.augmentation: color_jitter / flip need decoded images; the synthetic triplets are normalised "
                             "floats")
        cj = aug.get('color_jitter')
        if cj is None:
            cj = dict(cls.JITTER_DEFAULTS, p=0.0)
        if not isinstance(cj, dict):
            raise ValueError("config datasets.augmentation.color_jitter must be a mapping, got %r" % (cj,))
        unknown = set(cj) - set(cls.JITTER_DEFAULTS)
        if unknown:
            raise ValueError("config datasets.augmentation.color_jitter: unknown keys %s (known: %s)" % (sorted(unknown), list(cls.JITTER_DEFAULTS)))
        cj = dict(cls.JITTER_DEFAULTS, **cj)
        return cls(cj['brightness'], cj['contrast'], cj['saturation'], cj['hue'], p_color=cj['p'], p_flip=aug.get('flip', 0.0),
                   seed=int(config['action'].get('random_seed', 0)), rank=rank)

    def generator(self, epoch):
        return np.random.Generator(np.random.PCG64(np.random.SeedSequence([self.seed, self.rank, int(epoch)])))

    def draw(self, rng, n):
        """The next n records (AUGMENT_RECORD) of the stream."""
        u = rng.random((n, 10))
        rec = np.zeros(n, AUGMENT_RECORD)
        rec['flags'] = np.where(u[:, 0] < self.p_flip, AUG_FLIP, 0) | np.where(u[:, 1] < self.p_color, AUG_COLOUR, 0)
        for col, name in ((2, 'brightness'), (3, 'contrast'), (4, 'saturation')):
            x = getattr(self, name)
            lo, hi = max(0.0, 1.0 - x), 1.0 + x
            rec[name] = (lo + (hi - lo) * u[:, col]).astype(np.float32)
        hue = -self.hue + 2.0 * self.hue * u[:, 5]
        rec['hue_shift'] = np.trunc(hue * 255.0).astype(np.int64) % 256          # torchvision: np.int8(hue_factor * 255).view(np.uint8)
        order = np.argsort(u[:, 6:10], axis=1, kind='stable').astype(np.uint8)  # torchvision: torch.randperm(4) over (b, c, s, h)
        for op, x in enumerate((self.brightness, self.contrast, self.saturation, self.hue)):
            if x == 0:
                order[order == op] = AUG_OP_NONE
        rec['order'] = order
        return rec


class SyntheticTriplets(Dataset):
    def __init__(self, config, transforms=None, length=None):
        aug = config['datasets']['augmentation']
        self.H, self.W = aug['image_height'], aug['image_width']
        self.length = length or int(config['datasets'].get('synthetic_length', 64))
        self.seed = int(config['action'].get('random_seed', 0))

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        H, W = self.H, self.W
        imgs = []
        for _ in range(3):
            x = torch.randn(1, 3, H, W, generator=g)
            x = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="reflect"), 3, 1)[0]
            imgs.append(x.contiguous())
        K = torch.tensor([[0.58 * W, 0.0, 0.5 * W], [0.0, 1.92 * H, 0.5 * H], [0.0, 0.0, 1.0]], dtype=torch.float64)
        return {"tgt": imgs[0], "ref_imgs": [imgs[1], imgs[2]], "intrinsics": K, "groundtruth": torch.zeros(1, H, W)}


def synthetic_batch(B, H, W, seed=1234):
    """A whole seeded batch in the collated layout the trainer consumes (bench.py's input): low-passed randn images,
    KITTI-like fp64 intrinsics as the reference's loader gives them."""
    g = torch.Generator().manual_seed(seed)
    imgs = []
    for _ in range(3):
        x = torch.randn(B, 3, H, W, generator=g)
        imgs.append(torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="reflect"), 3, 1).contiguous())
    K = torch.tensor([[0.58 * W, 0.0, 0.5 * W], [0.0, 1.92 * H, 0.5 * H], [0.0, 0.0, 1.0]], dtype=torch.float64).repeat(B, 1, 1)
    return {"tgt": imgs[0], "ref_imgs": [imgs[1], imgs[2]], "intrinsics": K, "groundtruth": torch.zeros(B, 1, H, W)}


# ------------------------------------------------------------------------------------------------ KITTI files (reference dataloaders.py:18-171)
def read_calib_file(path):
    """'key: v0 v1 ...' lines -> {key: float64 array}; non-numeric values (dates) are skipped (reference geometry/calibration.py:70-89)."""
    data = {}
    with open(path, "r") as f:
        for line in f:
            line = line.rstrip()
            if not line or ":" not in line:
                continue
            key, value = line.split(":", 1)
            try:
                data[key] = np.array([float(x) for x in value.split()])
            except ValueError:
                pass
    return data


def stereo_baseline_of(calib):
    """The metric stereo baseline of a KITTI drive from its calib_cam_to_cam.txt entries (mono + stereo training, losses.Losses(stereo=True)):
    t_i = K^-1 P_rect_0i[:, 3] (the camera's translation in the rectified frame; K = P_rect_0i[:, :3]) and b = t_2.x - t_3.x, the x of camera
    3's centre (image_03) in camera 2's frame (image_02): ~0.533 m for 2011_09_26."""
    t = {}
    for i in (2, 3):
        key = "P_rect_%02d" % i
        if key not in calib:
            raise ValueError("calib_cam_to_cam.txt has no %s: mono + stereo training needs both rectified projections" % key)
        P = calib[key].reshape(3, 4)
        t[i] = np.linalg.solve(P[:, :3], P[:, 3])
    return float(t[2][0] - t[3][0])


def stereo_from_config(config):
    """loss.stereo (a bool, default off): mono + stereo training.  The dataset then also loads each target's image_03 twin and its baseline.
    Raises ValueError, at configuration time, for a value that is not a bool or for the synthetic triplets (they have no stereo frame)."""
    v = (config.get('loss') or {}).get('stereo', False)
    if not isinstance(v, bool):
        raise ValueError("config loss.stereo must be true or false, got %r" % (v,))
    if v and config['datasets'].get('dataset', ['KITTI']) == ['synthetic']:
        raise ValueError("config loss.stereo: mono + stereo training needs KITTI's image_03 frames and calibration; the synthetic triplets "
                         "have no stereo frame")
    return v


def find_calib_dir(image_path):
    """The KITTI date directory (.../2011_09_26/) above an image path.  The reference slices a fixed number of characters off the path
    (dataloaders.py:155: [:29], 'mac - 20, beauty - 29'), which only works for its two directory layouts."""
    import os
    import re
    d = os.path.dirname(os.path.abspath(image_path)) if os.path.isabs(image_path) else os.path.dirname(image_path)
    while d and d not in ("/", "."):
        if re.fullmatch(r"\d{4}_\d{2}_\d{2}", os.path.basename(d)):
            return d + os.sep
        d = os.path.dirname(d)
    raise FileNotFoundError("no KITTI date directory (YYYY_MM_DD) above %s" % image_path)


class KittiDataset(Dataset):
    """Reference dataloaders.py:18-128.  Samples hold file paths only; an image is decoded on fetch (PIL, on the host).

    Two ways to get the reference's tensors out of it:
      * `transforms` = a list of host callables applied exactly as load_img does (all but the last to every image, the last -- Normalize --
        not to the ground truth): the reference's own contract, for callers that bring torchvision;
      * `transforms=None` (what Trainer passes): fetches return the decoded uint8 image ('raw' samples) and the transform chain
        (/255, Resize, Normalize) runs on the GPU in PrefetchLoader / GpuImageTransform, bit-exact against Pillow.
    OXTS poses ('oxts', used only by the reference's semi-supervised pose experiment, trainer.py:301-304) are not loaded."""

    def __init__(self, config, transforms=None):
        super().__init__()
        ds = config['datasets']
        self.split = ds['split']
        self.kitti_filepath = ds['path']
        self.img_width = ds['augmentation']['image_width']
        self.img_height = ds['augmentation']['image_height']
        self.seq_len = ds.get('sequence_length', 3)
        gt_mode = ds.get('groundtruth', 'resized')
        if gt_mode not in ('resized', 'native', 'velodyne'):
            raise ValueError("datasets.groundtruth must be 'resized' (default), 'native' or 'velodyne', got %r" % (gt_mode,))
        # the ground truth unresized, in metres (the KITTI evaluation protocol); velodyne: projected from the raw scans on the GPU
        self.native_gt = gt_mode in ('native', 'velodyne')
        self.velodyne_gt = gt_mode == 'velodyne'
        self.transforms = transforms
        self.raw = transforms is None
        if self.velodyne_gt and not self.raw:
            raise ValueError("datasets.groundtruth: velodyne builds the maps on the GPU (PrefetchLoader); it takes no host transforms")
        self.stereo = stereo_from_config(config)     # loss.stereo: each sample also carries its target's image_03 twin and the baseline
        # opt-in: each sample also carries its date's P_rect_02 and velodyne -> camera transform, its native size and its path (inference.py)
        self.calibration = bool(ds.get('calibration', False))
        self.samples = []
        self._calib = {}
        self._baseline = {}
        self._velo = {}
        self._pl_calib = {}

    def __len__(self):
        return len(self.samples)

    def resolve(self, path):
        """Split-file paths are relative to the directory the reference is run from; also accept them relative to datasets.path."""
        import os
        if os.path.exists(path):
            return path
        tail = path.lstrip("./")
        for root in (self.kitti_filepath, os.path.dirname(os.path.normpath(self.kitti_filepath))):
            for cand in (os.path.join(root, tail), os.path.join(root, *tail.split("/")[1:]) if "/" in tail else None):
                if cand and os.path.exists(cand):
                    return cand
        return path

    def intrinsics_of(self, image_path):
        """calib.P[:, :3] of the drive's date directory (reference dataloaders.py:155-157), cached per directory; a fresh copy per call."""
        d = find_calib_dir(self.resolve(image_path))
        if d not in self._calib:
            self._calib[d] = read_calib_file(d + "calib_cam_to_cam.txt")["P_rect_02"].reshape(3, 4)[:, :3].copy()
        return self._calib[d].copy()

    def baseline_of(self, image_path):
        """stereo_baseline_of the drive's calib_cam_to_cam.txt, cached per date directory."""
        d = find_calib_dir(self.resolve(image_path))
        if d not in self._baseline:
            self._baseline[d] = stereo_baseline_of(read_calib_file(d + "calib_cam_to_cam.txt"))
        return self._baseline[d]

    def stereo_twin(self, image_path):
        """The image_03 frame taken with an image_02 target.  A missing file is a configuration error, raised when the dataset is built."""
        import os
        parts = image_path.split("/")
        if "image_02" not in parts:
            raise ValueError("loss.stereo: target %r is not an image_02 frame (the stereo source is its image_03 twin)" % image_path)
        k = len(parts) - 1 - parts[::-1].index("image_02")
        twin = "/".join(parts[:k] + ["image_03"] + parts[k + 1:])
        if not os.path.exists(self.resolve(twin)):
            raise ValueError("loss.stereo: the stereo frame %s of target %s does not exist (KITTI raw: image_03 beside image_02)" % (twin, image_path))
        return twin

    def velodyne_scan(self, image_path, override=None):
        """The raw scan of an image_02 frame: <drive>/velodyne_points/data/<frame>.bin, or `override` (a split file's 4th column ending in
        .bin).  A missing file is a configuration error, raised when the dataset is built."""
        import os
        scan = override
        if scan is None:
            parts = image_path.split("/")
            if "image_02" not in parts:
                raise ValueError("datasets.groundtruth: velodyne: target %r is not an image_02 frame (KITTI raw: velodyne_points beside "
                                 "image_02)" % image_path)
            k = len(parts) - 1 - parts[::-1].index("image_02")
            scan = os.path.splitext("/".join(parts[:k] + ["velodyne_points"] + parts[k + 1:]))[0] + ".bin"
        if not os.path.exists(self.resolve(scan)):
            raise ValueError("datasets.groundtruth: velodyne: the scan %s of target %s does not exist (KITTI raw: "
                             "velodyne_points/data/<frame>.bin beside image_02)" % (scan, image_path))
        return scan

    def velo_calib_of(self, image_path):
        """geometry.velodyne.velo_to_image of the drive's date directory -> (P [3,4] float64, (H, W)), cached per directory."""
        d = find_calib_dir(self.resolve(image_path))
        if d not in self._velo:
            self._velo[d] = velodyne.velo_to_image(d, 2)
        P, hw = self._velo[d]
        return P.copy(), hw

    def pl_calib_of(self, image_path):
        """datasets.calibration: (P_rect_02 [3,4], T velodyne -> camera [4,4] = [R | T; 0 0 0 1]) of the drive's date directory, float64, as
        pseudo_lidar.PseudoLiDAR reads them; cached per directory."""
        d = find_calib_dir(self.resolve(image_path))
        if d not in self._pl_calib:
            v2c = read_calib_file(d + "calib_velo_to_cam.txt")
            T = np.vstack([np.concatenate((v2c["R"].reshape(3, 3), v2c["T"].reshape(3, 1)), axis=1), [0.0, 0.0, 0.0, 1.0]])
            self._pl_calib[d] = (read_calib_file(d + "calib_cam_to_cam.txt")["P_rect_02"].reshape(3, 4).copy(), T)
        P, T = self._pl_calib[d]
        return P.copy(), T.copy()

    def load_img(self, path, gt=False):
        """-> (image, original height, original width).  raw mode: uint8 [H0, W0, 3] tensor (the GPU runs the chain); ground truth: the
        depth PNG as float32, resized with Pillow's bilinear filter on mode 'F' (what ToPILImage + Resize do to a float map), [1, h, w];
        with datasets.groundtruth: native, the PNG / 256 (metres) at its own size, [1, H0, W0] float32."""
        from PIL import Image
        img = Image.open(self.resolve(path))
        if gt:
            arr = np.asarray(img, dtype=np.float32)
            if self.native_gt and self.transforms is None:
                return torch.from_numpy(arr / np.float32(256.0))[None], arr.shape[0], arr.shape[1]
            if self.transforms is not None:
                for t in self.transforms[:-1]:
                    arr = t(arr)
                return arr.squeeze(), None, None
            small = Image.fromarray(arr, mode="F").resize((self.img_width, self.img_height), Image.BILINEAR)
            return torch.from_numpy(np.asarray(small, dtype=np.float32).copy())[None], None, None
        arr = np.asarray(img.convert("RGB") if img.mode != "RGB" else img)
        h, w = arr.shape[0], arr.shape[1]
        if self.transforms is not None:
            x = arr.astype(np.float32) / 255.0
            for t in self.transforms[:-1]:
                x = t(x)
            return self.transforms[-1](x).squeeze(), h, w
        return torch.from_numpy(arr.copy()), h, w

    def __getitem__(self, index):
        sample = self.samples[index]
        ret = {}
        ret['tgt'], og_h, og_w = self.load_img(sample['tgt'])
        ret['ref_imgs'] = [self.load_img(p)[0] for p in sample['ref_imgs']]
        K = sample['intrinsics'].copy()                  # the reference scales the CACHED matrix in place on every fetch (dataloaders.py:95-98)
        K[0] *= self.img_width / og_w
        K[1] *= self.img_height / og_h
        ret['intrinsics'] = torch.from_numpy(K)
        if self.stereo:
            ret['stereo'] = self.load_img(sample['stereo'])[0]
            ret['stereo_baseline'] = torch.tensor(sample['stereo_baseline'], dtype=torch.float32)
        if self.calibration:
            P, T = self.pl_calib_of(sample['tgt'])
            ret['P_rect'], ret['T_velo_cam'] = torch.from_numpy(P), torch.from_numpy(T)
            ret['native_size'] = torch.tensor((og_h, og_w), dtype=torch.int32)
            ret['path'] = sample['tgt']
        if self.velodyne_gt:
            # the raw scan, unfiltered: PrefetchLoader projects the batch's scans on the GPU
            if tuple(sample['velodyne_size']) != (og_h, og_w):
                raise ValueError("datasets.groundtruth: velodyne: S_rect_02 of %s gives %dx%d, the decoded target %s is %dx%d" %
                                 (find_calib_dir(self.resolve(sample['tgt'])), sample['velodyne_size'][0], sample['velodyne_size'][1],
                                  sample['tgt'], og_h, og_w))
            ret['velodyne'] = torch.from_numpy(velodyne.load_velodyne_points(self.resolve(sample['velodyne'])))
            ret['velodyne_P'] = torch.from_numpy(sample['velodyne_P'].copy())
            ret['velodyne_size'] = torch.tensor(sample['velodyne_size'], dtype=torch.int32)
        elif sample.get('groundtruth'):
            ret['groundtruth'] = self.load_img(sample['groundtruth'], gt=True)[0]
        elif self.native_gt and self.raw:
            ret['groundtruth'] = torch.zeros(1, og_h, og_w)      # no map: no valid pixel (evaluate_depth leaves the image out)
        else:
            ret['groundtruth'] = torch.zeros(1, self.img_height, self.img_width)
        return ret


class UnSupKittiFiles(KittiDataset):
    """Reference UnSupKittiDataset (dataloaders.py:131-171): one sample per line of the split file,
    '<tgt.png> <ref0.png> <ref1.png> <groundtruth.png>'."""

    def __init__(self, config, transforms=None):
        super().__init__(config, transforms)
        with open(self.split, "r") as f:
            lines = [ln.strip() for ln in f if ln.strip()]
        for ln in lines:
            parts = ln.split(" ")
            if len(parts) < 3:
                raise ValueError("split file %s: expected 'tgt ref0 ref1 [groundtruth]', got %r" % (self.split, ln))
            self.samples.append({'tgt': parts[0], 'ref_imgs': parts[1:3], 'intrinsics': self.intrinsics_of(parts[0]),
                                 'groundtruth': parts[3] if len(parts) > 3 else None})
            if self.stereo:
                self.samples[-1].update(stereo=self.stereo_twin(parts[0]), stereo_baseline=self.baseline_of(parts[0]))
            if self.velodyne_gt:
                override = parts[3] if len(parts) > 3 and parts[3].endswith(".bin") else None
                P, hw = self.velo_calib_of(parts[0])
                self.samples[-1].update(groundtruth=None, velodyne=self.velodyne_scan(parts[0], override), velodyne_P=P, velodyne_size=hw)


def raw_collate(samples):
    """collate_fn for raw samples: KITTI drives differ in image size (375x1242, 370x1226, ...), so the uint8 images cannot be stacked on
    the host; the list goes to PrefetchLoader, which resizes on the GPU."""
    return samples


class PrefetchLoader:
    """One batch ahead: a background thread takes the DataLoader's raw sample lists, copies the decoded uint8 frames to the GPU through pinned
    memory on its own stream, runs the fused /255 + Pillow-exact resize + Normalize kernel there (GpuImageTransform, grouped by source size)
    and hands the trainer finished batches in the reference's collated layout (tgt [B,3,h,w], ref_imgs 2 x [B,3,h,w], intrinsics [B,3,3] fp64,
    groundtruth [B,1,h,w]) together with the event the consumer's stream has to wait on.  SURVEY.md 8f row 1, second half.
    native_groundtruth (datasets.groundtruth: native): the maps differ in size, so groundtruth is [B,1,Hmax,Wmax], each map zero-padded at
    its bottom and right, and 'groundtruth_size' [B,2] int32 (host) holds every map's true (H, W).  Samples that carry raw Velodyne scans
    (datasets.groundtruth: velodyne) give the same layout: the scans are copied in one pinned buffer and projected on the loader's stream
    (geometry.velodyne.depth_maps), mirrored within the true width for flipped samples.
    augment (an Augmentation): each batch also carries 'tgt_aug', 'ref_imgs_aug' (what the networks see) and 'augment_records' (host, one
    AUGMENT_RECORD per sample); a flipped sample's frames, ground truth (within its true size) and principal point (cx' = w - 1 - cx: the
    warp samples pixel centres 0..w-1) are mirrored.  Call set_epoch(epoch) before each pass: the records are drawn for (seed, rank, epoch).
    Stereo samples (loss.stereo): the target's image_03 twin runs through the same plain transform as a fourth frame set (no network sees
    it, so never jittered) -> 'stereo' [B,3,h,w], and 'stereo_baseline' [B] float32 on the device; a flipped sample's stereo frame is
    mirrored and its baseline negated (the stereo camera is then on the other side).
    datasets.calibration: 'P_rect' [B,3,4] and 'T_velo_cam' [B,4,4] float64, 'native_size' [B,2] int32 (all host) and 'path' (B strings)."""

    def __init__(self, loader, img_height, img_width, device="cuda", depth=2, native_groundtruth=False, augment=None):
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())          # the worker thread needs an explicit index
        self.loader, self.h, self.w, self.device, self.depth = loader, int(img_height), int(img_width), dev, depth
        self.native_groundtruth = bool(native_groundtruth)
        self.transform = GpuImageTransform(img_height, img_width, dev)
        self.augment = augment
        self.epoch = 0

    def __len__(self):
        return len(self.loader)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _finish(self, samples, stream, rng=None):
        B = len(samples)
        frames = [s['tgt'] for s in samples] + [s['ref_imgs'][0] for s in samples] + [s['ref_imgs'][1] for s in samples]
        stereo = 'stereo' in samples[0]
        if stereo:
            frames += [s['stereo'] for s in samples]
        out = torch.empty((len(frames), 3, self.h, self.w), dtype=torch.float32, device=self.device)
        extra = {}
        flip = np.zeros(B, bool)
        if rng is not None:
            recs = self.augment.draw(rng, B)
            flip = (recs['flags'] & AUG_FLIP) != 0
            frame_recs = np.concatenate([recs] * 3)
            out_aug = torch.empty((3 * B, 3, self.h, self.w), dtype=torch.float32, device=self.device)
            extra['augment_records'] = recs
        with torch.cuda.stream(stream):
            groups = {}
            for i, f in enumerate(frames):
                groups.setdefault(tuple(f.shape), []).append(i)
            for shape, idx in groups.items():
                plain = [i for i in idx if rng is None or i >= 3 * B]      # (the stereo frames: plain transform only)
                jitter = [i for i in idx if rng is not None and i < 3 * B]
                if plain:
                    out[plain] = self.transform(torch.stack([frames[i] for i in plain]))
                if jitter:
                    out[jitter], out_aug[jitter] = self.transform.augmented(torch.stack([frames[i] for i in jitter]), frame_recs[jitter])
            if stereo:
                b = torch.tensor([float(s['stereo_baseline']) for s in samples], dtype=torch.float32)
                if flip.any():
                    f = torch.from_numpy(flip)
                    out[3 * B:][f.to(self.device)] = out[3 * B:][f.to(self.device)].flip(-1)
                    b[f] = -b[f]
                extra['stereo'] = out[3 * B:]
                extra['stereo_baseline'] = b.pin_memory().to(self.device, non_blocking=True)
            K = torch.stack([s['intrinsics'] for s in samples])
            if flip.any():
                f = torch.from_numpy(flip)
                K = K.clone()
                K[f, 0, 2] = (self.w - 1) - K[f, 0, 2]
                K[f, 0, 1] = -K[f, 0, 1]
            K = K.to(self.device, non_blocking=True)
            if rng is not None:
                extra['tgt_aug'], extra['ref_imgs_aug'] = out_aug[:B], [out_aug[B:2 * B], out_aug[2 * B:]]
            if 'P_rect' in samples[0]:
                # datasets.calibration: host tensors (PseudoLiDAR.project_batch builds its device table from them); they describe the
                # unflipped image
                extra['P_rect'] = torch.stack([s['P_rect'] for s in samples])
                extra['T_velo_cam'] = torch.stack([s['T_velo_cam'] for s in samples])
                extra['native_size'] = torch.stack([s['native_size'] for s in samples])
                extra['path'] = [s['path'] for s in samples]
            if 'velodyne' in samples[0]:
                # datasets.groundtruth: velodyne -- the batch's scans in one pinned buffer, one copy, the maps projected on this stream
                scans = [s['velodyne'] for s in samples]
                offsets = np.concatenate([[0], np.cumsum([len(p) for p in scans])]).astype(np.int64)
                host = torch.empty((int(offsets[-1]), 4), dtype=torch.float32, pin_memory=True)
                torch.cat(scans, out=host)
                sizes = torch.stack([s['velodyne_size'] for s in samples]).to(torch.int32)
                gt = velodyne.depth_maps(host.to(self.device, non_blocking=True), offsets, torch.stack([s['velodyne_P'] for s in samples]),
                                         sizes.numpy(), flip=flip if flip.any() else None, device=self.device)
                extra['groundtruth_size'] = sizes
            elif self.native_groundtruth:
                maps = [s['groundtruth'].flip(-1) if flip[i] else s['groundtruth'] for i, s in enumerate(samples)]
                sizes = torch.tensor([tuple(m.shape[-2:]) for m in maps], dtype=torch.int32)
                host = torch.zeros((B, 1, int(sizes[:, 0].max()), int(sizes[:, 1].max())), dtype=torch.float32).pin_memory()
                for i, m in enumerate(maps):
                    host[i, :, :m.shape[-2], :m.shape[-1]] = m
                gt = host.to(self.device, non_blocking=True)
                extra['groundtruth_size'] = sizes
            else:
                gt = torch.stack([s['groundtruth'].flip(-1) if flip[i] else s['groundtruth'] for i, s in enumerate(samples)])
                gt = gt.to(self.device, non_blocking=True)
            done = torch.cuda.Event()
            done.record(stream)
        return dict({'tgt': out[:B], 'ref_imgs': [out[B:2 * B], out[2 * B:3 * B]], 'intrinsics': K, 'groundtruth': gt}, **extra), done

    def __iter__(self):
        import queue
        import threading
        q = queue.Queue(maxsize=self.depth)
        stream = torch.cuda.Stream(device=self.device)
        dev = self.device
        rng = self.augment.generator(self.epoch) if self.augment is not None else None      # drawn in batch order, in this thread

        def work():
            try:
                torch.cuda.set_device(dev)
                for samples in self.loader:
                    q.put(self._finish(samples, stream, rng))
                q.put(None)
            except BaseException as e:          # surface loader errors in the consumer
                q.put(e)
        t = threading.Thread(target=work, daemon=True)
        t.start()
        while True:
            item = q.get()
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            batch, done = item
            torch.cuda.current_stream(self.device).wait_event(done)
            for v in [batch['tgt']] + batch['ref_imgs'] + [batch['intrinsics'], batch['groundtruth']] + \
                    ([batch['tgt_aug']] + batch['ref_imgs_aug'] if 'tgt_aug' in batch else []) + \
                    ([batch['stereo'], batch['stereo_baseline']] if 'stereo' in batch else []):
                v.record_stream(torch.cuda.current_stream(self.device))
            yield batch
        t.join()


def UnSupKittiDataset(config, transforms=None):
    """The dataset the trainer asks for (reference trainer.py:106): datasets.dataset == ['synthetic'] -> seeded synthetic triplets (no KITTI
    offline); anything else -> the split-file driven KITTI reader above.  A missing split file or data root fails HERE, at configuration
    time, with the path in the message."""
    import os
    stereo_from_config(config)                   # (loss.stereo with the synthetic triplets fails here)
    if config['datasets'].get('dataset', ['KITTI']) == ['synthetic']:
        return SyntheticTriplets(config, transforms)
    split = config['datasets']['split']
    if not os.path.exists(split):
        raise FileNotFoundError("datasets.split = %r does not exist (KITTI is not shipped with this repository; set datasets.dataset: "
                                "['synthetic'] for seeded synthetic triplets, or point datasets.split / datasets.path at a KITTI raw tree)" % split)
    return UnSupKittiFiles(config, transforms)
