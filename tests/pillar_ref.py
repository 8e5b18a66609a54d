"""TEST INFRASTRUCTURE: the definition of the pillar voxeliser (include/mcav_depth.h: mcav_pillarize, pseudo_lidar.pillarize) in numpy, one
operation per rounding, and a literal sequential transcription of second.pytorch's points_to_voxel loop to hold it against.

    points [n_max, 4] float32 (x, y, z, i), offsets int32 [B + 1] (offsets[0] = 0, ascending): image b owns rows offsets[b] .. offsets[b+1];
    n = min(offsets[B], n_max); rows at and beyond n are never read.
    cell     fx = floor((x - x0) / vx) in float32, fy likewise; kept iff 0 <= fx < nx, 0 <= fy < ny, z0 <= z < z1, compared as floats
             (NaN and +-inf drop out, -0.0 is 0); cell = (b, iy, ix)
    pillars  the non-empty cells in ascending (b, iy, ix) order; pillar_offsets [B + 1]
    slots    the min(count, N) points of the cell with the smallest row indices, ascending; the rest of the N slots +0.0
    coords   (b, 0, iy, ix)
    columns  C = 4: x y z i as they are.  decorate: C = 9, 4..6 = x - mx, y - my, z - mz (m: float64 sum in slot order / num_points, rounded
             once to float32), 7..8 = x - ((float)ix * vx + (vx * 0.5 + x0)), y likewise
"""
import collections

import numpy as np

F = np.float32
Grid = collections.namedtuple("Grid", "x0 y0 z0 z1 vx vy nx ny")


def make_grid(x=(0.0, 69.12), y=(-39.68, 39.68), z=(-3.0, 1.0), size=(0.16, 0.16)):
    """PointPillars' KITTI grid by default: 432 x 496.  nx = round((x1 - x0) / vx) in float64; the kernel's scalars are float32."""
    nx = int(np.round((np.float64(x[1]) - np.float64(x[0])) / np.float64(size[0])))
    ny = int(np.round((np.float64(y[1]) - np.float64(y[0])) / np.float64(size[1])))
    return Grid(F(x[0]), F(y[0]), F(z[0]), F(z[1]), F(size[0]), F(size[1]), nx, ny)


def live_rows(points, offsets):
    return max(min(int(offsets[-1]), points.shape[0]), 0)


def image_of(offsets, i):
    """the b with offsets[b] <= i < offsets[b + 1]; empty images are stepped over"""
    B = len(offsets) - 1
    return np.searchsorted(np.asarray(offsets[1:B], np.int64), i, side="right")


def axis_cells(v, origin, size, n):
    """-> (float32 floor((v - origin) / size), whether it names one of n cells)"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (v - F(origin)).astype(F)
        f = np.floor((d / F(size)).astype(F))
        ok = (f >= F(0)) & (f < F(n))
    cell = np.where(ok, f, F(0)).astype(np.int64)
    return cell, ok & (cell < n)          # float32(n) rounds up above 2^24: never past the grid


def cells_of(points, grid):
    """-> ix, iy (int64) and the keep mask, per row"""
    ix, okx = axis_cells(points[:, 0], grid.x0, grid.vx, grid.nx)
    iy, oky = axis_cells(points[:, 1], grid.y0, grid.vy, grid.ny)
    with np.errstate(invalid="ignore"):
        okz = (points[:, 2] >= grid.z0) & (points[:, 2] < grid.z1)
    return ix, iy, okx & oky & okz


def cell_counts(points, offsets, grid):
    """-> int64 [B, ny, nx]: the points of every cell"""
    points = np.asarray(points, F)
    B = len(offsets) - 1
    n = live_rows(points, offsets)
    ix, iy, keep = cells_of(points[:n], grid)
    b = image_of(offsets, np.arange(n, dtype=np.int64))
    out = np.zeros((B, grid.ny, grid.nx), np.int64)
    np.add.at(out, (b[keep], iy[keep], ix[keep]), 1)
    return out


def centre(i, origin, size):
    """(float)i * size + (size * 0.5 + origin), float32, three roundings"""
    half = F(F(F(size) * F(0.5)) + F(origin))
    return (np.asarray(i).astype(F) * F(size)).astype(F) + half


def pillarize(points, offsets, grid, max_points=32, decorate=False, capacity=None):
    """-> dict(voxels [P', N, C] float32, coords [P', 4] int32, num_points [P'] int32, offsets int32 [B + 1]) with P' = min(P, capacity)"""
    points = np.asarray(points, F)
    offsets = np.asarray(offsets, np.int32)
    B, N = len(offsets) - 1, int(max_points)
    assert 1 <= N <= 64 and offsets[0] == 0 and (np.diff(offsets) >= 0).all()
    n = live_rows(points, offsets)
    pts = points[:n]
    idx = np.arange(n, dtype=np.int64)
    b = image_of(offsets, idx)
    ix, iy, keep = cells_of(pts, grid)
    cell = ((b * grid.ny + iy) * grid.nx + ix)[keep]
    rows = idx[keep]
    order = np.argsort(cell, kind="stable")                # within a cell: ascending row index
    cell, rows = cell[order], rows[order]
    ucell, start, count = np.unique(cell, return_index=True, return_counts=True)
    P = len(ucell)
    pb = ucell // (grid.ny * grid.nx)
    poff = np.searchsorted(pb, np.arange(B + 1), side="left").astype(np.int32)
    C = 9 if decorate else 4
    num = np.minimum(count, N).astype(np.int32)
    vox = np.zeros((P, N, C), F)
    group = np.repeat(np.arange(P), count)
    slot = np.arange(len(cell)) - np.repeat(start, count)
    take = slot < N
    vox[group[take], slot[take], :4] = pts[rows[take]]
    piy, pix = (ucell // grid.nx) % grid.ny, ucell % grid.nx
    coords = np.stack([pb, np.zeros_like(pb), piy, pix], axis=1).astype(np.int32).reshape(P, 4)
    if decorate:
        used = np.arange(N)[None, :] < num[:, None]
        mean = np.zeros((P, 3), F)
        with np.errstate(invalid="ignore", over="ignore"):
            for col in range(3):
                acc = np.zeros(P, np.float64)
                for s in range(N):                         # slot order
                    acc = np.where(used[:, s], acc + vox[:, s, col].astype(np.float64), acc)
                mean[:, col] = (acc / num.astype(np.float64)).astype(F)
            cx = centre(pix, grid.x0, grid.vx)
            cy = centre(piy, grid.y0, grid.vy)
            for col in range(3):
                vox[:, :, 4 + col] = np.where(used, vox[:, :, col] - mean[:, col, None], F(0))
            vox[:, :, 7] = np.where(used, vox[:, :, 0] - cx[:, None], F(0))
            vox[:, :, 8] = np.where(used, vox[:, :, 1] - cy[:, None], F(0))
    cap = P if capacity is None else min(int(capacity), P)
    return dict(voxels=vox[:cap], coords=coords[:cap], num_points=num[:cap], offsets=poff)


def points_to_voxel_sequential(points, grid, max_points):
    """second.pytorch core/point_cloud/point_cloud_ops.py _points_to_voxel_kernel, statement for statement, for one image: float32, a
    (ny, nx) grid, no max_voxels cap; x and y go through its floor((p - lo) / size) test, z through the definition's z0 <= z < z1 (its
    single z cell).  -> voxels [V, N, 4], coors [V, 2] = (iy, ix), num_points_per_voxel [V], in order of first appearance."""
    points = np.asarray(points, F)
    lo, size, gsz = (grid.x0, grid.y0), (grid.vx, grid.vy), (grid.nx, grid.ny)
    coor_to_voxelidx = -np.ones((grid.ny, grid.nx), np.int64)
    voxels, coors, num_points_per_voxel = [], [], []
    coor = [0, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(points.shape[0]):
            failed = False
            for j in range(2):
                c = np.floor(F(F(points[i, j] - F(lo[j])) / F(size[j])))
                if not (c >= 0 and c < F(gsz[j])) or int(c) >= gsz[j]:
                    failed = True
                    break
                coor[j] = int(c)
            if failed or not (points[i, 2] >= grid.z0 and points[i, 2] < grid.z1):
                continue
            voxelidx = coor_to_voxelidx[coor[1], coor[0]]
            if voxelidx == -1:
                voxelidx = len(voxels)
                coor_to_voxelidx[coor[1], coor[0]] = voxelidx
                voxels.append(np.zeros((max_points, 4), F))
                coors.append((coor[1], coor[0]))
                num_points_per_voxel.append(0)
            num = num_points_per_voxel[voxelidx]
            if num < max_points:
                voxels[voxelidx][num] = points[i]
                num_points_per_voxel[voxelidx] += 1
    V = len(voxels)
    return (np.stack(voxels) if V else np.zeros((0, max_points, 4), F), np.asarray(coors, np.int64).reshape(V, 2),
            np.asarray(num_points_per_voxel, np.int32))


def sequential_batch(points, offsets, grid, max_points):
    """points_to_voxel_sequential per image, each image's voxels sorted by (iy, ix) -> the C = 4 result of pillarize"""
    points = np.asarray(points, F)
    n = live_rows(points, offsets)
    vox, coords, num, poff = [], [], [], [0]
    for b in range(len(offsets) - 1):
        lo, hi = min(int(offsets[b]), n), min(int(offsets[b + 1]), n)
        v, c, k = points_to_voxel_sequential(points[lo:hi], grid, max_points)
        order = np.lexsort((c[:, 1], c[:, 0]))
        vox.append(v[order]); num.append(k[order])
        coords.append(np.concatenate([np.full((len(order), 1), b), np.zeros((len(order), 1), np.int64), c[order]], axis=1))
        poff.append(poff[-1] + len(order))
    return dict(voxels=np.concatenate(vox), coords=np.concatenate(coords).astype(np.int32), num_points=np.concatenate(num),
                offsets=np.asarray(poff, np.int32))
