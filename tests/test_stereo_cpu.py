"""CPU: the mono + stereo loss (include/mcav_depth.h: mcav_warp_loss_stereo_fwd_bwd).  The test reference tests/stereo_ref.py against a literal
transcription of monodepth2's MS loss loop and against the masked reference it extends, its tie order and selection code 3 on hand-built
scenes, the Python surface's argument checks, and the stereo instantiations of the fused kernels in the compiled gfx950 ISA."""
import pytest
import torch
import torch.nn.functional as F

import minreproj_ref as M
import stereo_ref as R
from oracle.losses import ssim_distance


def _inputs(B, H, W, seed, zero_pose0=False):
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[0.58 * W, 0, 0.5 * W], [0, 1.92 * H, 0.5 * H], [0, 0, 1]], dtype=torch.float64).repeat(B, 1, 1)
    imgs = [torch.rand(B, 3, H, W, generator=g, dtype=torch.float64) for _ in range(4)]
    dt, dr = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64), torch.rand(B, 1, H, W, generator=g, dtype=torch.float64)
    poses = 0.02 * torch.randn(B, 2, 6, generator=g, dtype=torch.float64)
    if zero_pose0:
        poses[:, 0] = 0
    b = 0.3 + 0.4 * torch.rand(B, generator=g, dtype=torch.float64)
    return imgs, dt, dr, poses, K, b


# ---------------------------------------------------------------------------------------------- monodepth2, transcribed
def _md2_backproject(depth, inv_K):
    B, _, H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=depth.dtype), torch.arange(W, dtype=depth.dtype), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=depth.dtype)], 0).unsqueeze(0).repeat(B, 1, 1)
    cam = depth.view(B, 1, -1) * torch.matmul(inv_K[:, :3, :3], pix)
    return torch.cat([cam, torch.ones(B, 1, H * W, dtype=depth.dtype)], 1)


def _md2_project(points, K, T, H, W, eps):
    P = torch.matmul(K, T)[:, :3, :]
    cam = torch.matmul(P, points)
    pix = cam[:, :2, :] / (cam[:, 2, :].unsqueeze(1) + eps)
    pix = pix.view(-1, 2, H, W).permute(0, 2, 3, 1)
    pix[..., 0] /= W - 1
    pix[..., 1] /= H - 1
    return (pix - 0.5) * 2


def _md2_reprojection_loss(pred, target, ssim):
    l1 = (target - pred).abs().mean(1, True)
    if not ssim:
        return l1
    return 0.85 * ssim_distance(pred, target).mean(1, True) + 0.15 * l1


def md2_ms_loss(inputs, depth, K, T, ssim, avg_reprojection, automask, eps):
    """monodepth2's trainer.generate_images_pred + compute_losses at one scale, frame_ids [0, -1, 1, "s"].  The three points where this
    project differs from monodepth2 are stated, not hidden: the sampling uses zero padding with align_corners=True (the reference's
    F.grid_sample call, not monodepth2's "border"), the projection's z guard is a parameter (monodepth2: 1e-7, the kernels: 1e-5), and the
    identity errors get no random tie-break noise (the kernels break ties deterministically)."""
    B, _, H, W = inputs[0].shape
    K4 = torch.eye(4, dtype=K.dtype).repeat(B, 1, 1)
    K4[:, :3, :3] = K
    inv_K = torch.inverse(K4)
    cam_points = _md2_backproject(depth, inv_K)
    preds = {}
    for fid in (-1, 1, "s"):
        pix = _md2_project(cam_points, K4, T[fid], H, W, eps)
        preds[fid] = F.grid_sample(inputs[fid], pix, padding_mode="zeros", align_corners=True)
    target = inputs[0]
    reprojection_losses = torch.cat([_md2_reprojection_loss(preds[f], target, ssim) for f in (-1, 1, "s")], 1)
    if automask:
        identity_losses = torch.cat([_md2_reprojection_loss(inputs[f], target, ssim) for f in (-1, 1, "s")], 1)
    reprojection_loss = reprojection_losses.mean(1, keepdim=True) if avg_reprojection else reprojection_losses
    combined = torch.cat((identity_losses, reprojection_loss), 1) if automask else reprojection_loss
    to_optimise = combined if combined.shape[1] == 1 else torch.min(combined, dim=1)[0]
    return to_optimise.mean()


def _rt(pose):
    from oracle.geometry import pose_to_matrix
    return pose_to_matrix(pose)


@pytest.mark.parametrize("ssim", [False, True])
@pytest.mark.parametrize("mode", ["avg", "min", "min+auto"])
def test_reference_is_monodepth2_ms(ssim, mode):
    """The target-view group of the reference is monodepth2's MS loss with its warps' term weights summing to 1: (1/3, 1/3, 1/3) and warp 2
    weighted 0.  monodepth2's stereo_T for a left target is [I | (-baseline, 0, 0)]: b > 0."""
    imgs, dt, dr, poses, K, b = _inputs(2, 9, 13, 3)
    tgt, r0, r1, st = imgs
    depth = 1.0 / (10.0 * dt + 0.01)
    T = {-1: _rt(poses[:, 0]), 1: _rt(poses[:, 1]), "s": torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)}
    T["s"][:, 0, 3] = -b
    md2 = md2_ms_loss({0: tgt, -1: r0, 1: r1, "s": st}, depth, K, T, ssim, mode == "avg", mode == "min+auto", eps=1e-5)
    got, _, _ = R.stereo_losses(tgt, [r0, r1], st, b, [[dt], [dr]], poses, K, ssim=ssim, min_reprojection=mode != "avg",
                                automask=mode == "min+auto", term_weights=(1 / 3, 1 / 3, 0.0, 1 / 3))
    assert abs(float(got[0]) - float(md2)) <= 1e-12 * abs(float(md2)), (float(got[0]), float(md2))
    # monodepth2's own z guard moves sampling positions by ~1e-6 relative: the same loss to that order
    md2_eps = md2_ms_loss({0: tgt, -1: r0, 1: r1, "s": st}, depth, K, T, ssim, mode == "avg", mode == "min+auto", eps=1e-7)
    assert abs(float(got[0]) - float(md2_eps)) <= 1e-4 * abs(float(md2_eps))


@pytest.mark.parametrize("ssim", [False, True])
def test_zero_baseline_and_stereo_equal_to_ref0_is_the_masked_reference(ssim):
    """b = 0, stereo = ref0 and pose[0] = 0: warp s IS warp 0 (e_s == e_0, i_s == i_0 exactly), so every later stereo candidate ties with
    warp 0's and loses -- the masked reference with the matching weights, selection included (code 3 never appears)."""
    imgs, dt, dr, poses, K, _ = _inputs(2, 9, 13, 5, zero_pose0=True)
    tgt, r0, r1, _ = imgs
    b = torch.zeros(2, dtype=torch.float64)
    for minr, auto in ((True, False), (True, True)):
        want = M.run(tgt, [r0, r1], dt, dr, poses, K, torch.float64, ssim=ssim, min_reprojection=minr, automask=auto)
        got = R.run(tgt, [r0, r1], r0.clone(), b, dt, dr, poses, K, torch.float64, ssim=ssim, min_reprojection=minr, automask=auto)
        assert abs(got[0][0] - want[0][0]) <= 1e-13 * abs(want[0][0]) and got[0][1] == want[0][1]
        for g, w in zip(got[1], want[1]):
            assert float((g - w).abs().max()) <= 1e-12 * float(w.abs().max()) + 1e-300
        assert torch.equal(got[2][0], want[2][0])
    # without min-reprojection the stereo term is a term of its own: with weight 0 it is the masked / oracle loss
    for auto in (False, True):
        want = M.run(tgt, [r0, r1], dt, dr, poses, K, torch.float64, ssim=ssim, automask=auto)
        got = R.run(tgt, [r0, r1], r0.clone(), b, dt, dr, poses, K, torch.float64, ssim=ssim, automask=auto, term_weights=(0.25, 0.25, 0.5, 0.0))
        assert abs(got[0][0] - want[0][0]) <= 1e-13 * abs(want[0][0])
        assert torch.equal(got[2][0], want[2][0])


def shifted_scene(B, H, W, baseline, seed=0, dtype=torch.float64):
    """A smooth texture S seen by the stereo camera and its exact left view at a known fronto-parallel depth: tgt(x, y) = S(x - fx b / D, y).
    -> tgt, stereo, disparity (sigmoid form) of D, K."""
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[0.58 * W, 0, 0.5 * W], [0, 1.92 * H, 0.5 * H], [0, 0, 1]], dtype=dtype).repeat(B, 1, 1)
    D = 8.0
    shift = float(K[0, 0, 0]) * baseline / D
    ph = torch.rand(3, generator=g, dtype=dtype) * 6.28
    xs = torch.arange(W, dtype=dtype).view(1, 1, 1, W)
    ys = torch.arange(H, dtype=dtype).view(1, 1, H, 1)
    c = torch.arange(3, dtype=dtype).view(1, 3, 1, 1)
    S = lambda x: 0.5 + 0.25 * torch.sin(0.37 * x + ph.view(1, 3, 1, 1) + 0.21 * ys) + 0.1 * torch.cos(0.11 * x * (c + 1))
    disp = torch.full((B, 1, H, W), (1.0 / D - 0.01) / 10.0, dtype=dtype)
    return S(xs - shift).expand(B, 3, H, W).contiguous(), S(xs).expand(B, 3, H, W).contiguous(), disp, K


def test_stereo_wins_where_it_explains_the_target_and_gets_the_gradient():
    B, H, W, b = 1, 12, 40, 0.5
    tgt, st, disp, K = shifted_scene(B, H, W, b)
    g = torch.Generator().manual_seed(1)
    refs = [torch.rand(B, 3, H, W, generator=g, dtype=torch.float64) for _ in range(2)]
    poses = torch.zeros(B, 2, 6, dtype=torch.float64)
    loss, grads, sels, _ = R.run(tgt, refs, st, torch.full((B,), b, dtype=torch.float64), disp, disp.clone(), poses, K, torch.float64,
                                 min_reprojection=True, automask=True)
    code = sels[0][:, 0]
    shift = int(float(K[0, 0, 0]) * b / 8.0) + 2
    assert bool((code[..., shift:] == R.STEREO).all()), code           # everywhere the stereo frame saw the pixel: code 3
    # a pixel won by an identity error sends no gradient: the identities win nowhere here, but the gradient of stereo-won pixels is there
    gd = grads[0][:, 0]
    assert float(gd[..., shift:-shift].abs().sum()) > 0


def test_tie_order_identities_first_then_stereo_last():
    """A later candidate wins only if strictly smaller: with e_s == e_1 the pixel stays with warp 1; with i_s == e_s the identity wins."""
    t = lambda *v: torch.tensor(v, dtype=torch.float64).reshape(1, 2, 2)
    i0, i1, i_s = t(9, 9, 9, 9), t(9, 9, 9, 9), t(9, 9, 0.5, 9)
    e0, e1, e_s = t(3, 2, 1, 0.5), t(3, 1, 1, 0.7), t(3, 1, 0.5, 0.4)
    m, code, _ = M.select([i0, i1, i_s, e0, e1, e_s], [2, 2, 2, 0, 1, R.STEREO])
    assert code.flatten().tolist() == [0, 1, 2, 3]
    assert m.flatten().tolist() == [3, 1, 0.5, 0.4]


def test_static_scene_identity_everywhere_no_photometric_gradient():
    """tgt = ref0 = ref1 = stereo, zero poses, b != 0: every identity error is 0, the selection is all identity, loss_mam is 0, and d disp_t
    is the smoothness gradient alone (the stereo warp, which does move the pixels, sends nothing)."""
    imgs, dt, dr, _, K, b = _inputs(1, 7, 9, 8)
    tgt = imgs[0]
    poses = torch.zeros(1, 2, 6, dtype=torch.float64)
    for ssim in (False, True):
        loss, grads, sels, _ = R.run(tgt, [tgt.clone(), tgt.clone()], tgt.clone(), b[:1], dt, dr, poses, K, ssim=ssim, min_reprojection=True,
                                     automask=True)
        assert (sels[0] == R.IDENTITY).all() and loss[0] == 0.0
        _, smooth, _, _ = R.run(tgt, [tgt.clone(), tgt.clone()], tgt.clone(), b[:1], dt, dr, poses, K, upstream=(0.0, 1.0), ssim=ssim,
                                min_reprojection=True, automask=True)
        assert torch.equal(grads[0], smooth[0]) and float(grads[2].abs().max()) == 0


def test_losses_stereo_needs_its_inputs():
    from mcav import lib as L
    from losses import Losses
    crit = Losses(stereo=True)
    assert crit.stereo
    t = torch.zeros(1, 3, 8, 16)
    d = [[torch.zeros(1, 1, 8, 16)], [torch.zeros(1, 1, 8, 16)]]
    with pytest.raises(L.MCAVError):
        crit.forward(t, [t, t], d, torch.zeros(1, 2, 6), torch.eye(3).repeat(1, 1, 1), None)
    with pytest.raises(L.MCAVError):
        crit.forward(t, [t, t], d, torch.zeros(1, 2, 6), torch.eye(3).repeat(1, 1, 1), None, stereo=t)
    assert not Losses().stereo


# ---------------------------------------------------------------------------------------------- the compiled kernels
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import test_isa_handoff as T
    return T._device_functions(tmp_path_factory, "warp_loss.hip")


def _stereo(kernels):
    return {n: b for n, b in kernels.items() if "warp_loss" in n and "_stereo_kernel" in n}


def test_stereo_instantiations_exist(kernels):
    st = _stereo(kernels)
    for kern in ("warp_loss_l1_stereo_kernel", "warp_loss_ssim_stereo_kernel"):
        for mode in range(4):
            assert any(kern + "ILj%dE" % mode in n for n in st), (kern, mode, list(st))
    assert len(st) == 8, list(st)


def test_stereo_instantiations_keep_the_ticket_hand_off(kernels):
    import test_isa_handoff as T
    st = _stereo(kernels)
    assert set(T._ticket_kernels(st)) == set(st)
    T.test_stores_are_acknowledged_before_every_ticket(st)
    T.test_published_words_and_finisher_reads_are_agent_scope(st)


def test_stereo_instantiations_do_not_spill(kernels):
    for n, body in _stereo(kernels).items():
        assert sum(1 for i in body if i.startswith("scratch_")) == 0, n
