"""Float64 definitions of the standalone geometry, SSIM and smoothness entry points of csrc/warp_loss.hip (include/mcav_depth.h:
mcav_pose_to_matrix, mcav_invert_pose, mcav_reconstruct, mcav_project, mcav_inverse_warp_fwd / _bwd, mcav_ssim_fwd,
mcav_smooth_loss_fwd_bwd, mcav_disp_to_depth / _bwd), in plain torch, and the error bounds the GPU tests hold the kernels to.

The expression trees are the reference's (csrc/warp_math.h names the lines); the two guards are the float32 values the kernels use.
tests/test_warp_ops_cpu.py pins these definitions to the committed goldens and to oracle.geometry / oracle.losses evaluated in float64, so
they are not a second opinion.  u = 2^-24 is the unit roundoff of float32: one rounded operation on a value v errs by at most u |v|."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS_AXIS = float(np.float32(1e-7))
EPS_Z = float(np.float32(1e-5))
F64 = torch.float64


# ---------------------------------------------------------------------------------------------- poses
def rodrigues(v):
    """axis-angle [B,3] -> R [B,3,3]: axis = v / (|v| + 1e-7f), Rodrigues."""
    v = v.to(F64)
    angle = torch.norm(v, 2, 1, True)                                      # (its backward is 0 at v = 0, as the kernels')
    axis = v / (angle + EPS_AXIS)
    c, s = torch.cos(angle)[:, 0], torch.sin(angle)[:, 0]
    C = 1 - c
    x, y, z = axis[:, 0], axis[:, 1], axis[:, 2]
    xs, ys, zs = x * s, y * s, z * s
    xC, yC, zC = x * C, y * C, z * C
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    return torch.stack([x * xC + c, xyC - zs, zxC + ys, xyC + zs, y * yC + c, yzC - xs, zxC - ys, yzC + xs, z * zC + c], 1).view(-1, 3, 3)


def pose_to_matrix(pose, invert=False):
    """pose [B,6] -> T [B,4,4] = Trans @ Rot, or its rigid inverse [R^T | -R^T t]."""
    pose = pose.to(F64)
    R, t = rodrigues(pose[:, :3]), pose[:, 3:]
    T = torch.eye(4, dtype=F64).repeat(len(pose), 1, 1)
    T[:, :3, :3], T[:, :3, 3] = R, t
    return invert_pose(T) if invert else T


def invert_pose(T):
    T = T.to(F64)
    Rt = T[:, :3, :3].transpose(1, 2)
    out = torch.eye(4, dtype=F64).repeat(len(T), 1, 1)
    out[:, :3, :3] = Rt
    out[:, :3, 3] = -(Rt * T[:, None, :3, 3]).sum(2)
    return out


def pose_bounds(pose, invert):
    """-> (bound on |err| of the rotation entries, [B,3] bound on the translation, [B,3] the translation's product sum alone).
    Rotation: 16 u, every intermediate is at most 1 in magnitude and a 2-ulp sinf / cosf fits.  Translation: exact when not inverted.
    Inverted, t_i = sum_j (-R_ji) p_j is formed from the ROUNDED rotation: three products and two additions, 8 u sum_j |R_ji p_j| (the third
    value), plus the rotation entries' own error times the translation, 16 u sum_j |p_j|: where a column of R is small, the second term is
    all there is."""
    pose = pose.to(F64)
    if not invert:
        return 16 * U, torch.zeros(len(pose), 3, dtype=F64), torch.zeros(len(pose), 3, dtype=F64)
    R = rodrigues(pose[:, :3]).transpose(1, 2)
    products = 8 * U * (R.abs() * pose[:, None, 3:].abs()).sum(2)
    return 16 * U, products + 16 * U * pose[:, 3:].abs().sum(1, keepdim=True).expand(-1, 3), products


# ---------------------------------------------------------------------------------------------- reconstruct / project
def pixel_grid(H, W):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    return torch.stack([xs, ys, torch.ones_like(xs)], 0)                  # [3,H,W]


def reconstruct(depth, K):
    """depth [B,H,W], K [B,3,3] -> X [B,3,H,W] = (K^-1 [x y 1]^T) D."""
    B, H, W = depth.shape
    rays = torch.einsum("bij,jhw->bihw", torch.linalg.inv(K.to(F64)), pixel_grid(H, W))
    return rays * depth.to(F64)[:, None]


def reconstruct_bound(depth, K):
    """Per element.  X_i = (sum_j Kinv_ij p_j) D with p = (x, y, 1) exact and D an exact input.  The kernel rounds K^-1 to float32 (u per
    entry, the float64 inverse itself is exact to 1e-13), then per term one product (u) and at most two additions (2 u), then the product
    with D (u): first order 5 u sum_j |Kinv_ij p_j| D.  6 u covers the second-order terms."""
    B, H, W = depth.shape
    mag = torch.einsum("bij,jhw->bihw", torch.linalg.inv(K.to(F64)).abs(), pixel_grid(H, W))
    return 6 * U * mag * depth.to(F64).abs()[:, None]


def _camera(X, K, Tcw):
    B, _, H, W = X.shape
    P = K.to(F64) @ Tcw.to(F64)[:, :3, :]                                  # [B,3,4]
    c = torch.einsum("bij,bjhw->bihw", P[:, :, :3], X.to(F64)) + P[:, :, 3, None, None]
    return P, c


def project(X, K, Tcw):
    """X [B,3,H,W], K [B,3,3], Tcw [B,4,4] -> grid [B,H,W,2]: c = K [R|t] [X;1], pix = c_xy / (c_z + 1e-5f), (pix / (size - 1) - 0.5) * 2."""
    B, _, H, W = X.shape
    _, c = _camera(X, K, Tcw)
    z = c[:, 2] + EPS_Z
    gx = (c[:, 0] / z / (W - 1) - 0.5) * 2
    gy = (c[:, 1] / z / (H - 1) - 0.5) * 2
    return torch.stack([gx, gy], -1)


def project_bound(X, K, Tcw):
    """Per element of the grid, first order, over the definition's own magnitudes.
      P_ij = sum_k K_ik M_kj (M = [R|t]): K rounded to float32 (u), a product (u), two additions (2 u): |dP_ij| <= 4 u sum_k |K_ik M_kj|.
      c_i = sum_j P_ij X_j + P_i3: per term a product and up to three additions (4 u) plus dP_ij |X_j|:
            |dc_i| <= 8 u A_i,  A_i = sum_jk |K_ik M_kj X_j| + sum_k |K_ik M_k3|   (A_i >= sum_j |P_ij X_j| + |P_i3|).
      z = c_2 + 1e-5f: |dz| <= |dc_2| + u |z|.
      pix_i = c_i / z (a division within 2 u): |dpix_i| <= |dc_i| / |z| + |c_i| |dz| / z^2 + 2 u |pix_i|     (the condition of c / (z + 1e-5))
      g_i = (pix_i / (n - 1) - 0.5) * 2: the division (2 u), the subtraction (u), the doubling exact:
            |dg_i| <= 2 (|dpix_i| / (n - 1) + 2 u |pix_i| / (n - 1) + u |pix_i / (n - 1) - 0.5|).
    Times 1.01 for the second-order terms.  Meant for z >= 0.5."""
    B, _, H, W = X.shape
    Ka, Ma, Xa = K.to(F64).abs(), Tcw.to(F64)[:, :3, :].abs(), X.to(F64).abs()
    A = torch.einsum("bik,bkj,bjhw->bihw", Ka, Ma[:, :, :3], Xa) + torch.einsum("bik,bk->bi", Ka, Ma[:, :, 3])[:, :, None, None]
    _, c = _camera(X, K, Tcw)
    dc = 8 * U * A
    z = c[:, 2] + EPS_Z
    dz = dc[:, 2] + U * z.abs()
    out = []
    for i, n in ((0, W), (1, H)):
        pix = c[:, i] / z
        dpix = dc[:, i] / z.abs() + c[:, i].abs() * dz / (z * z) + 2 * U * pix.abs()
        out.append(2 * (dpix / (n - 1) + 2 * U * pix.abs() / (n - 1) + U * (pix / (n - 1) - 0.5).abs()))
    return 1.01 * torch.stack(out, -1)


# ---------------------------------------------------------------------------------------------- inverse warp
def sampling_position(grid, H, W):
    """grid [B,H,W,2] in [-1, 1] -> (ix, iy) in source pixels (align_corners=True): ((g + 1) / 2) * (size - 1)."""
    return (grid[..., 0] + 1) / 2 * (W - 1), (grid[..., 1] + 1) / 2 * (H - 1)


def warp_position(depth, pose, K, pose_inv):
    B, H, W = depth.shape
    grid = project(reconstruct(depth, K), K, pose_to_matrix(pose, bool(pose_inv)))
    return sampling_position(grid, H, W)


def bilinear_taps(img, ix, iy):
    """img [B,C,H,W] float64, positions [B,H,W] -> (texels [B,C,4,H,W] = nw, ne, sw, se with zeros outside the image, wx1, wy1)."""
    B, C, H, W = img.shape
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    flat = img.reshape(B, C, H * W)
    tex = []
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().view(B, 1, H * W).expand(B, C, H * W)
            tex.append(torch.where(ok.view(B, 1, H * W), flat.gather(2, idx), torch.zeros((), dtype=img.dtype)).view(B, C, H, W))
    return torch.stack(tex, 2), wx1, wy1


def inverse_warp(img, depth, pose, K, pose_inv):
    """-> out [B,3,H,W]: bilinear sample (zeros outside, align_corners=True) of img at the projected positions.  Differentiable (autograd)
    w.r.t. depth and pose."""
    ix, iy = warp_position(depth, pose, K, pose_inv)
    t, wx1, wy1 = bilinear_taps(img.to(F64), ix.detach(), iy.detach())
    x0, y0 = torch.floor(ix.detach()), torch.floor(iy.detach())
    wx1, wy1 = (ix - x0)[:, None], (iy - y0)[:, None]
    wx0, wy0 = 1 - wx1, 1 - wy1
    return t[:, :, 0] * (wx0 * wy0) + t[:, :, 1] * (wx1 * wy0) + t[:, :, 2] * (wx0 * wy1) + t[:, :, 3] * (wx1 * wy1)


def inverse_warp_bound(img, depth, pose, K, pose_inv, delta):
    """Per element of the forward output: |err| <= spread * delta + 8 u max|texel|.  The output is continuous in the sampling position and
    linear in each coordinate inside a cell with slopes of at most the range (spread) of the four texels the float64 definition taps; delta
    bounds the distance |d ix| + |d iy| between the kernel's and the definition's positions: twice what the float32 CPU oracle's positions
    measure for the case on the CPU (recorded in tests/warp_ops_cases.py).  8 u max|texel|: the weights (3 roundings each) and the
    four-term sum."""
    ix, iy = warp_position(depth, pose, K, pose_inv)
    t, _, _ = bilinear_taps(img.to(F64), ix, iy)
    spread = t.max(2).values - t.min(2).values
    return spread * delta + 8 * U * t.abs().max(2).values


# ---------------------------------------------------------------------------------------------- SSIM
def _reflect_pad(x):
    """reflection padding by one pixel, spelled out: at H = 2 or W = 2 both reflections fold onto the same pixel."""
    x = torch.cat([x[..., 1:2, :], x, x[..., -2:-1, :]], -2)
    return torch.cat([x[..., 1:2], x, x[..., -2:-1]], -1)


def ssim(x, y, C1=1e-4, C2=9e-4):
    """x, y [N,H,W] -> clamp((1 - SSIM) / 2, 0, 1), 3 x 3 box over reflection padding; C1, C2 as the float32 values the entry receives."""
    x, y = x.to(F64)[None], y.to(F64)[None]
    C1, C2 = float(np.float32(C1)), float(np.float32(C2))
    box = lambda t: F.avg_pool2d(_reflect_pad(t), 3, 1)
    mx, my = box(x), box(y)
    vx, vy, vxy = box(x * x) - mx * mx, box(y * y) - my * my, box(x * y) - mx * my
    num = (2 * mx * my + C1) * (2 * vxy + C2)
    den = (mx * mx + my * my + C1) * (vx + vy + C2)
    return ((1 - num / den) / 2).clamp(0, 1)[0]


def ssim_bound(x, y, C1=1e-4, C2=9e-4):
    """Per element, first order, for the kernel's evaluation order (no fma contraction there).  With E[.] the window mean of magnitudes:
      a 9-term sum: 8 u sum |a_i|; of products: 9 u; times k = fl(1/9) (u) and the product (u):
        m = s k: 10 u |m|-like;  m_x m_y, m_x^2: (2 * 10 + 1) u = 21 u;  E[ab] k: 11 u E|ab|
      v_x = E[x^2] - m_x^2: 11 u E[x^2] + 21 u m_x^2 + u |v_x|   (the cancellation: absolute, not relative);  v_xy alike with E|xy|, |m_x m_y|
      A1 = 2 m_xy + C1: 2 * 21 u |m_xy| + u |A1|;  A2 = 2 v_xy + C2: 2 dv_xy + u |A2|
      B1 = m_x^2 + m_y^2 + C1: 21 u (m_x^2 + m_y^2) + 2 u B1;  B2 = v_x + v_y + C2: dv_x + dv_y + 2 u B2
      num = A1 A2, den = B1 B2: |A2| dA1 + |A1| dA2 + u |num| (den alike);  q = num / den (2 u): dnum / den + |num| dden / den^2 + 2 u |q|
      out = (1 - q) / 2: dq / 2 + u |1 - q| / 2; the clamp does not increase it.
    Times 1.01 for the second-order terms.  Meant for variances >= 0.01, where den is bounded away from 0."""
    x, y = x.to(F64)[None], y.to(F64)[None]
    C1, C2 = float(np.float32(C1)), float(np.float32(C2))
    box = lambda t: F.avg_pool2d(_reflect_pad(t), 3, 1)
    mx, my = box(x), box(y)
    ax, ay = box(x.abs()), box(y.abs())
    exx, eyy, exy = box(x * x), box(y * y), box((x * y).abs())
    mxy, mxx, myy = mx * my, mx * mx, my * my
    vx, vy, vxy = exx - mxx, eyy - myy, box(x * y) - mxy
    d_mxy, d_mxx, d_myy = 21 * U * ax * ay, 21 * U * ax * ax, 21 * U * ay * ay
    d_vx, d_vy = 11 * U * exx + d_mxx + U * vx.abs(), 11 * U * eyy + d_myy + U * vy.abs()
    d_vxy = 11 * U * exy + d_mxy + U * vxy.abs()
    A1, A2, B1, B2 = 2 * mxy + C1, 2 * vxy + C2, mxx + myy + C1, vx + vy + C2
    dA1, dA2 = 2 * d_mxy + U * A1.abs(), 2 * d_vxy + U * A2.abs()
    dB1, dB2 = d_mxx + d_myy + 2 * U * B1.abs(), d_vx + d_vy + 2 * U * B2.abs()
    num, den = A1 * A2, B1 * B2
    dnum = A2.abs() * dA1 + A1.abs() * dA2 + U * num.abs()
    dden = B2.abs() * dB1 + B1.abs() * dB2 + U * den.abs()
    q = num / den
    dq = dnum / den.abs() + num.abs() * dden / (den * den) + 2 * U * q.abs()
    return (1.01 * (dq / 2 + U * (1 - q).abs() / 2))[0]


# ---------------------------------------------------------------------------------------------- smoothness
def smooth_terms(D):
    """depth [B,1,H,W] -> the four second-difference fields of Losses.smooth_loss (dx2, dxdy, dydx, dy2)."""
    dy = D[:, :, 1:] - D[:, :, :-1]
    dx = D[:, :, :, 1:] - D[:, :, :, :-1]
    return dx[:, :, :, 1:] - dx[:, :, :, :-1], dx[:, :, 1:] - dx[:, :, :-1], dy[:, :, :, 1:] - dy[:, :, :, :-1], dy[:, :, 1:] - dy[:, :, :-1]


def smooth(depth, weight=1.0, upstream=1.0):
    """-> (weight * term, upstream * weight * d term / d depth) in float64, term = the four means of |second difference|; |.|' at 0 is 0.
    weight and upstream as the float32 values the entry receives."""
    D = depth.to(F64).clone().requires_grad_()
    w = float(np.float32(weight))
    loss = w * sum(t.abs().mean() for t in smooth_terms(D))
    (g,) = torch.autograd.grad(loss, D)
    return float(loss.detach()), float(np.float32(upstream)) * g


def smooth_coefficient(B, H, W, weight=1.0, upstream=1.0):
    """The largest coefficient a sign carries in the gradient: 2 cxx, 2 cyy (the centre of a second difference) or cxy = 2 / n (dxdy and dydx
    are the same field), times weight and upstream."""
    c = max(2.0 / (B * H * (W - 2)), 2.0 / (B * (H - 2) * W), 2.0 / (B * (H - 1) * (W - 1)))
    return abs(float(np.float32(weight)) * float(np.float32(upstream))) * c


def smooth_gradient_bound(B, H, W, weight=1.0, upstream=1.0):
    """A pixel's gradient is upstream times a sum of ten signed coefficients (cxx, 2 cxx, cxx, cyy, 2 cyy, cyy, four times cxy) whose signs
    are exact on a dyadic grid.  With S = 4 cxx + 4 cyy + 4 cxy: each coefficient is weight / (float)n, one rounding (u S in all); nine
    additions of partial sums of at most S (9 u S); the product with upstream (u S): 11 u S."""
    S = 4.0 / (B * H * (W - 2)) + 4.0 / (B * (H - 2) * W) + 8.0 / (B * (H - 1) * (W - 1))
    return 11 * U * abs(float(np.float32(weight)) * float(np.float32(upstream))) * S


# ---------------------------------------------------------------------------------------------- disparity -> depth
def disp_to_depth(disp):
    return 1 / (10 * disp.to(F64) + float(np.float32(0.01)))


def disp_to_depth_bwd(disp, d_depth):
    D = disp_to_depth(disp)
    return d_depth.to(F64) * (-10 * D * D)


def ulps(got, want64):
    """|got - want| in units of the spacing of float32 at want -> the largest."""
    w32 = want64.to(torch.float32)
    spacing = torch.from_numpy(np.spacing(np.abs(w32.numpy()).astype(np.float32))).to(F64)
    return float(((got.to(F64) - want64).abs() / spacing).max())
