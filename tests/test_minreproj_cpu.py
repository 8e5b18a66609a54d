"""CPU: the masked loss modes (per-pixel minimum reprojection, auto-masking).  The test reference against the oracle with both modes off,
its selection and tie rules on hand-built 1x1x3x3 cases, and the masked instantiations of the fused kernels in the compiled gfx950 ISA."""
import pytest
import torch

import minreproj_ref as R

K33 = torch.tensor([[[2.0, 0.0, 1.0], [0.0, 2.0, 1.0], [0.0, 0.0, 1.0]]], dtype=torch.float64)


def _inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[0.58 * W, 0, 0.5 * W], [0, 1.92 * H, 0.5 * H], [0, 0, 1]], dtype=torch.float64).repeat(B, 1, 1)
    imgs = [torch.rand(B, 3, H, W, generator=g, dtype=torch.float64) for _ in range(3)]
    dt, dr = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64), torch.rand(B, 1, H, W, generator=g, dtype=torch.float64)
    poses = 0.02 * torch.randn(B, 2, 6, generator=g, dtype=torch.float64)
    return imgs, dt, dr, poses, K


@pytest.mark.parametrize("ssim", [False, True])
def test_reference_with_both_modes_off_is_the_oracle(ssim):
    from oracle import losses as ol
    imgs, dt, dr, poses, K = _inputs(2, 9, 13, 5)
    want = ol.losses_forward(imgs[0], imgs[1:], [[dt], [dr]], poses, K, 0.85 if ssim else 0.0)
    got, sels, _ = R.masked_losses(imgs[0], imgs[1:], [[dt], [dr]], poses, K, ssim=ssim)
    for a, b in zip(got, want):
        assert abs(float(a) - float(b)) <= 1e-12 * abs(float(b))
    assert int(sels[0].abs().sum()) == 0
    # several scales: the same per scale, coarse depths resized
    dts = [dt, torch.rand(2, 1, 4, 6, dtype=torch.float64)]
    drs = [dr, torch.rand(2, 1, 4, 6, dtype=torch.float64)]
    want = ol.losses_forward(imgs[0], imgs[1:], [dts, drs], poses, K, 0.85 if ssim else 0.0)
    got, _, _ = R.masked_losses(imgs[0], imgs[1:], [dts, drs], poses, K, ssim=ssim)
    for a, b in zip(got, want):
        assert abs(float(a) - float(b)) <= 1e-12 * abs(float(b))


def test_select_tie_order():
    """Identities first, then reprojections; a later candidate wins only if strictly smaller."""
    t = lambda *v: torch.tensor(v, dtype=torch.float64).reshape(1, 3, 3)
    i0, i1 = t(1, 1, 1, 2, 2, 2, 3, 3, 3), t(1, 0.5, 1, 2, 2, 2, 3, 3, 3)
    e0, e1 = t(1, 1, 0.9, 1, 2, 5, 4, 0.1, 3), t(1, 1, 0.9, 2, 1, 5, 4, 0.1, 0.2)
    m, code, gap = R.select([i0, i1, e0, e1], [2, 2, 0, 1])
    assert code.flatten().tolist() == [2, 2, 0, 0, 1, 2, 2, 0, 1]
    assert m.flatten().tolist() == [1, 0.5, 0.9, 1, 1, 2, 3, 0.1, 0.2]
    assert gap.flatten()[0] == 0 and gap.flatten()[2] == 0          # exact ties are gaps of zero
    _, code, _ = R.select([e0, e1], [0, 1])
    assert code.flatten().tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 1]


def _scene(tgt_v, ref_v, pose, seed=0, H=3, W=3):
    g = torch.Generator().manual_seed(seed)
    tgt = torch.full((1, 3, H, W), tgt_v, dtype=torch.float64) if tgt_v is not None else torch.rand(1, 3, H, W, generator=g, dtype=torch.float64)
    ref = torch.full((1, 3, H, W), ref_v, dtype=torch.float64) if ref_v is not None else torch.rand(1, 3, H, W, generator=g, dtype=torch.float64)
    disp = torch.full((1, 1, H, W), 0.5, dtype=torch.float64)
    poses = torch.tensor(pose, dtype=torch.float64).reshape(1, 1, 6).repeat(1, 2, 1)
    return tgt, [ref, ref.clone()], [[disp], [disp.clone()]], poses


def test_equal_reprojections_take_warp_0():
    """ref0 == ref1 and the two poses equal: e_0 == e_1 exactly at every pixel -> warp 0 (plane 0 code 0) wherever a reprojection wins."""
    tgt, refs, disp, poses = _scene(None, None, [0.01, -0.02, 0.03, 0.05, 0.0, 0.02], seed=3)
    _, sels, gaps = R.masked_losses(tgt, refs, disp, poses, K33, min_reprojection=True)
    assert (gaps[0][:, 0] == 0).all()
    assert (sels[0][:, 0] == 0).all() and (sels[0][:, 1] == 0).all()
    _, sels, _ = R.masked_losses(tgt, refs, disp, poses, K33, min_reprojection=True, automask=True)
    assert set(sels[0][:, 0].flatten().tolist()) <= {0, 2}           # never warp 1


@pytest.mark.parametrize("ssim", [False, True])
def test_identity_equal_to_reprojection_takes_the_identity(ssim):
    """Constant images, a pose that moves every sample out of view (the warped image is exactly zero): with ref = 2 tgt the L1 identity
    error |tgt - ref| equals the reprojection error |tgt - 0| at every pixel -> the identity wins, the loss is that error, no gradient."""
    tgt, refs, disp, poses = _scene(0.25, 0.5, [0.0, 0.0, 0.0, 1e3, 1e3, 0.0])
    for minr in (False, True):
        out, sels, _ = R.masked_losses(tgt, refs, disp, poses, K33, ssim=ssim, min_reprojection=minr, automask=True)
        if not ssim:
            assert (sels[0] == R.IDENTITY).all(), sels[0]
            assert abs(float(out[0]) - 0.25) < 1e-15
    # the tie broken by one ulp towards the reprojection: warp 0 kept (warp 2 compares 0.5 + ulp with 0.25 + ulp: identity)
    tgt, refs, disp, poses = _scene(0.25, 0.5 + 2 ** -50, [0.0, 0.0, 0.0, 1e3, 1e3, 0.0])
    _, sels, _ = R.masked_losses(tgt, refs, disp, poses, K33, min_reprojection=True, automask=True)
    assert (sels[0][:, 0] == 0).all() and (sels[0][:, 1] == R.IDENTITY).all()


def test_static_scene_is_all_identity_without_gradient():
    tgt, _, disp, _ = _scene(None, None, [0.0] * 6, seed=4, H=5, W=7)
    poses = torch.zeros(1, 2, 6, dtype=torch.float64)
    for ssim in (False, True):
        loss, grads, sels, _ = R.run(tgt, [tgt.clone(), tgt.clone()], disp[0][0], disp[1][0], poses, K33.clone(), ssim=ssim,
                                     min_reprojection=True, automask=True)
        assert (sels[0] == R.IDENTITY).all()
        assert loss[0] == 0.0
        _, smooth_only, _, _ = R.run(tgt, [tgt.clone(), tgt.clone()], disp[0][0], disp[1][0], poses, K33.clone(), upstream=(0.0, 1.0),
                                     ssim=ssim, min_reprojection=True, automask=True)
        assert torch.equal(grads[0], smooth_only[0]) and float(grads[1].abs().max()) == 0 and float(grads[2].abs().max()) == 0


# ---------------------------------------------------------------------------------------------- the compiled kernels
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import test_isa_handoff as T
    return T._device_functions(tmp_path_factory, "warp_loss.hip")


MODES = {"Lj1E": "min-reprojection", "Lj2E": "automask", "Lj3E": "both"}


def test_masked_instantiations_exist(kernels):
    for kern in ("warp_loss_l1_kernel", "warp_loss_ssim_kernel"):
        for tag in MODES:
            assert any(kern in n and "ILb0E" + tag in n for n in kernels), (kern, tag, [n for n in kernels if kern in n])


def test_masked_instantiations_keep_the_ticket_hand_off(kernels):
    import test_isa_handoff as T
    masked = {n: b for n, b in kernels.items() if "warp_loss" in n and any("ILb0E" + t in n for t in MODES)}
    assert len(masked) == 6, list(masked)
    assert set(T._ticket_kernels(masked)) == set(masked)
    T.test_stores_are_acknowledged_before_every_ticket(masked)
    T.test_published_words_and_finisher_reads_are_agent_scope(masked)


def test_no_instantiation_spills(kernels):
    """The masked instantiations use no scratch; the plain ones keep what they had (the plain L1 kernel one dword at 168 VGPRs, the
    per-pixel dump instantiation its dump arrays)."""
    for n, body in kernels.items():
        if "warp_loss" not in n:
            continue
        n_scratch = sum(1 for i in body if i.startswith("scratch_"))
        if any("ILb0E" + t in n for t in MODES):
            assert n_scratch == 0, (n, n_scratch)
        elif "l1_kernelILb0E" in n:
            assert n_scratch <= 2, (n, n_scratch)
        elif "ssim" in n:
            assert n_scratch == 0, (n, n_scratch)
