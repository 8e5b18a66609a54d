"""The cases of the standalone geometry, SSIM and smoothness entry points, shared by tests/test_warp_ops_cpu.py (which pins the float64
definitions of tests/warp_ops_ref.py and checks what the cases promise) and tests/test_warp_ops_gpu.py (which runs the kernels).
CPU tensors, float32 as the kernels read them (K float64, as the loader gives it)."""
import math

import torch

# (B, H, W) of the per-pixel kernels (32 x 8 pixel tiles): the smallest shape accepted; 3 x 3; exactly one tile; one past the tile in both
# directions; 2 and 3 workgroups (the backward's finalize sums the slab in four strided parts); 9 workgroups.
SHAPES = [(1, 2, 2), (2, 3, 3), (1, 8, 32), (1, 9, 33), (1, 16, 32), (1, 24, 32), (3, 17, 70)]
SMOOTH_SHAPES = [(2, 3, 3), (1, 3, 40), (1, 40, 3), (2, 8, 32), (2, 9, 33), (1, 17, 70)]
POSE_KINDS = ["zero", "small", "roll", "away"]
ANGLES = [0.0, 1e-8, 1e-4, 0.03, 1.0, math.pi - 1e-3]
POSE_BATCHES = [1, 64, 65]                         # one past the 64-thread block
DISP_N = 4096 * 256 + 3                           # the grid-stride loop takes a second trip


def gen(seed):
    return torch.Generator().manual_seed(seed)


def intrinsics(B, H, W, dtype=torch.float64):
    """KITTI-like, different per sample."""
    K = torch.tensor([[0.58 * W, 0.0, 0.5 * W], [0.0, 1.92 * H, 0.5 * H], [0.0, 0.0, 1.0]], dtype=torch.float64).repeat(B, 1, 1)
    i = torch.arange(B, dtype=torch.float64)
    K[:, 0, 0] *= 1 + 0.05 * i
    K[:, 1, 1] *= 1 - 0.03 * i
    K[:, 0, 2] += 0.3 * i
    K[:, 1, 2] -= 0.2 * i
    return K.to(dtype)


def pose_vectors(B, angle, seed):
    """[B,6]: rotations of the given angle about random axes, translations of 0.1 .. 0.3; angle 0: the zero vector, exactly."""
    g = gen(seed)
    if angle == 0.0:
        return torch.zeros(B, 6)
    axis = torch.nn.functional.normalize(torch.randn(B, 3, generator=g, dtype=torch.float64), dim=1)
    t = 0.1 + 0.2 * torch.rand(B, 3, generator=g, dtype=torch.float64)
    return torch.cat([axis * angle, t * torch.where(torch.rand(B, 3, generator=g) < 0.5, -1.0, 1.0)], 1).float()


def warp_pose(kind, B, seed):
    """zero: the identity; small: the training regime (0.03 rad, 0.02); roll: 0.06 rad about the optical axis, which takes image corners out
    of view on all four sides; away: a sideways translation that takes every pixel of every sample out of view."""
    g = gen(seed)
    p = torch.zeros(B, 6)
    if kind == "small":
        p = torch.cat([0.03 * (torch.rand(B, 3, generator=g) - 0.5) * 2, 0.02 * (torch.rand(B, 3, generator=g) - 0.5) * 2], 1)
    elif kind == "roll":
        p[:, 2] = 0.06 * torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0)
        p[:, 3:] = 0.003 * (torch.rand(B, 3, generator=g) - 0.5)
    elif kind == "away":
        p[:, 3] = 1000.0
    return p.float().contiguous()


def warp_case(B, H, W, kind, seed=0):
    """-> dict(img [B,3,H,W] in [0, 1], depth [B,H,W] in [1, 10], pose [B,6], K [B,3,3] float64, grad_out [B,3,H,W])."""
    g = gen(1000 * H + 10 * W + B + seed)
    return dict(img=torch.rand(B, 3, H, W, generator=g), depth=1 + 9 * torch.rand(B, H, W, generator=g), pose=warp_pose(kind, B, 7 * H + W),
                K=intrinsics(B, H, W), grad_out=torch.randn(B, 3, H, W, generator=g))


def behind_camera_pose(B):
    """A half turn about the y axis less 0.2 rad: most points get z < 0, finite."""
    p = torch.zeros(B, 6)
    p[:, 1] = math.pi - 0.2
    p[:, 5] = 0.3
    return p


# delta of warp_ops_ref.inverse_warp_bound per case (shape, pose kind, pose_inv): twice the largest |d ix| + |d iy| between the float32 CPU
# oracle's sampling positions (oracle.geometry in float32) and the float64 definition's, over the pixels with a tap inside the image, in
# pixels, rounded up to two digits.  Measured on the CPU by tests/test_warp_ops_cpu.py::test_recorded_deltas, which keeps them so.
DELTAS = {
    ((1, 2, 2), 'zero', 0): 2.7e-07, ((1, 2, 2), 'zero', 1): 2.7e-07, ((1, 2, 2), 'small', 0): 4.4e-07, ((1, 2, 2), 'small', 1): 5.2e-07,
    ((1, 2, 2), 'roll', 0): 1.8e-07, ((1, 2, 2), 'roll', 1): 2e-07, ((1, 2, 2), 'away', 0): 0, ((1, 2, 2), 'away', 1): 0,
    ((2, 3, 3), 'zero', 0): 5e-07, ((2, 3, 3), 'zero', 1): 5e-07, ((2, 3, 3), 'small', 0): 7.6e-07, ((2, 3, 3), 'small', 1): 1.2e-06,
    ((2, 3, 3), 'roll', 0): 7.5e-07, ((2, 3, 3), 'roll', 1): 4.9e-07, ((2, 3, 3), 'away', 0): 0, ((2, 3, 3), 'away', 1): 0,
    ((1, 8, 32), 'zero', 0): 8.9e-06, ((1, 8, 32), 'zero', 1): 8.9e-06, ((1, 8, 32), 'small', 0): 1.3e-05, ((1, 8, 32), 'small', 1): 9.8e-06,
    ((1, 8, 32), 'roll', 0): 1.1e-05, ((1, 8, 32), 'roll', 1): 1.1e-05, ((1, 8, 32), 'away', 0): 0, ((1, 8, 32), 'away', 1): 0,
    ((1, 9, 33), 'zero', 0): 7.2e-06, ((1, 9, 33), 'zero', 1): 7.2e-06, ((1, 9, 33), 'small', 0): 1.1e-05, ((1, 9, 33), 'small', 1): 1.4e-05,
    ((1, 9, 33), 'roll', 0): 1.3e-05, ((1, 9, 33), 'roll', 1): 1.1e-05, ((1, 9, 33), 'away', 0): 0, ((1, 9, 33), 'away', 1): 0,
    ((1, 16, 32), 'zero', 0): 9e-06, ((1, 16, 32), 'zero', 1): 9e-06, ((1, 16, 32), 'small', 0): 1.3e-05, ((1, 16, 32), 'small', 1): 1.6e-05,
    ((1, 16, 32), 'roll', 0): 1.2e-05, ((1, 16, 32), 'roll', 1): 8.9e-06, ((1, 16, 32), 'away', 0): 0, ((1, 16, 32), 'away', 1): 0,
    ((1, 24, 32), 'zero', 0): 1.1e-05, ((1, 24, 32), 'zero', 1): 1.1e-05, ((1, 24, 32), 'small', 0): 1.5e-05, ((1, 24, 32), 'small', 1): 1.3e-05,
    ((1, 24, 32), 'roll', 0): 1.4e-05, ((1, 24, 32), 'roll', 1): 1.6e-05, ((1, 24, 32), 'away', 0): 0, ((1, 24, 32), 'away', 1): 0,
    ((3, 17, 70), 'zero', 0): 2.9e-05, ((3, 17, 70), 'zero', 1): 2.9e-05, ((3, 17, 70), 'small', 0): 3.6e-05, ((3, 17, 70), 'small', 1): 4.3e-05,
    ((3, 17, 70), 'roll', 0): 3.3e-05, ((3, 17, 70), 'roll', 1): 3e-05, ((3, 17, 70), 'away', 0): 0, ((3, 17, 70), 'away', 1): 0,
}


def ssim_case(N, H, W, kind, seed=0):
    """-> (x, y) [N,H,W].  random: uniform in [0, 1]; same: y is x; constant: two constant images; conditioned: a checkerboard of +-0.3 about
    0.5 plus noise of 0.1, so every 3 x 3 window has a variance of at least 0.01."""
    g = gen(100 * H + W + N + seed)
    x, y = torch.rand(N, H, W, generator=g), torch.rand(N, H, W, generator=g)
    if kind == "same":
        y = x.clone()
    elif kind == "constant":
        x, y = torch.full((N, H, W), 0.25), torch.full((N, H, W), 0.75)
    elif kind == "conditioned":
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        board = (((ys + xs) % 2).float() * 2 - 1) * 0.3
        x, y = 0.5 + board + 0.1 * (x - 0.5), 0.5 - board.roll(1, 0) * 0.9 + 0.1 * (y - 0.5)
    return x.contiguous(), y.contiguous()


def dyadic_depth(B, H, W, seed=0, constant=False):
    """[B,1,H,W] multiples of 2^-6 in [1, 64): every second difference is exact in float32, so every sign is float64's, zeros included.
    The first row and the first column are linear ramps, whose second differences are exactly zero."""
    if constant:
        return torch.full((B, 1, H, W), 17.25)
    D = torch.randint(64, 4096, (B, 1, H, W), generator=gen(10 * H + W + B + seed)).float() / 64
    D[:, :, 0, :] = 2.0 + (5.0 / 64) * torch.arange(W).float()
    D[:, :, :, 0] = 2.0 + (3.0 / 64) * torch.arange(H).float()
    return D.contiguous()
