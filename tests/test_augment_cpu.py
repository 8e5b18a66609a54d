"""CPU: the augmentation's definition (tests/augment_ref.py) against the installed Pillow, csrc/augment_math.h compiled for the host against
the definition on every colour, the record stream of dataloaders.Augmentation, config validation and the pinned fixture."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import augment_ref as R
from conftest import PKG, REPO
from make_augment_golden import adjust_hue, pil_augment

ALL = np.arange(1 << 24, dtype=np.int64)
ALPHAS = [0.8, 1.0, 1.2, float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2))), 0.0, 2.5]


@pytest.fixture(scope="module")
def all_colours():
    c = ALL
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.fixture(scope="module")
def pil_hsv(all_colours):
    from PIL import Image
    return np.asarray(Image.fromarray(all_colours).convert("HSV")).copy()


def _image():
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (64, 256, 3)).astype(np.uint8)
    img[0, :, 0] = np.arange(256)
    img[1, :, 1] = np.arange(256)
    img[2, :, 2] = np.arange(256)
    return img


@pytest.mark.parametrize("f", ALPHAS)
def test_enhance_operations_match_pillow(f):
    from PIL import Image, ImageEnhance
    img = _image()
    im = Image.fromarray(img)
    f32 = np.float32(f)
    assert np.array_equal(np.asarray(ImageEnhance.Brightness(im).enhance(f)), R.brightness(img, f32))
    assert np.array_equal(np.asarray(ImageEnhance.Color(im).enhance(f)), R.saturation(img, f32))
    assert np.array_equal(np.asarray(ImageEnhance.Contrast(im).enhance(f)), R.contrast(img, f32))
    assert np.array_equal(np.asarray(im.convert("L")), R.luma(img))


def test_contrast_mean_at_exact_ties():
    """S / n = k + 0.5 exactly: int(k + 1.0) = k + 1, as ImageStat's float64 mean + 0.5 gives."""
    from PIL import Image, ImageEnhance
    for lo in (0, 10, 127, 200):
        img = np.zeros((2, 2, 3), np.uint8)
        img[0, :] = lo                      # grey: L = the value itself
        img[1, :] = lo + 1
        assert R.luma(img).sum() * 2 == (2 * lo + 1) * 4
        assert R.contrast_mean(img) == lo + 1
        deg = np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).degenerate)
        assert (deg == lo + 1).all()
        for f in (0.8, 1.2):
            assert np.array_equal(np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).enhance(f)), R.contrast(img, np.float32(f)))


def test_rgb_to_hsv_on_every_colour(all_colours, pil_hsv):
    assert np.array_equal(R.rgb_to_hsv(all_colours), pil_hsv)


@pytest.mark.parametrize("shift", [0, 1, 12, 25, 231, 244, 255])
def test_hsv_round_trip_on_every_colour(all_colours, pil_hsv, shift):
    from PIL import Image
    h = pil_hsv.copy()
    h[..., 0] = (h[..., 0].astype(np.int64) + shift) % 256
    want = np.asarray(Image.fromarray(h, "HSV").convert("RGB"))
    assert np.array_equal(R.hsv_to_rgb(h), want)
    if shift in (0, 25):
        assert np.array_equal(R.hue(all_colours, shift), want)


def test_hue_shift_is_torchvisions():
    for hf in (0.1, -0.1, 0.5, -0.5, 0.0, 0.0039, -0.0039, 0.333):
        assert R.hue_shift_of(hf) == int(np.int8(hf * 255).view(np.uint8))


def _record(flags, order, b, c, s, hue_factor):
    rec = np.zeros((), R_DTYPE())
    rec["flags"], rec["order"] = flags, order
    rec["brightness"], rec["contrast"], rec["saturation"] = np.float32(b), np.float32(c), np.float32(s)
    rec["hue_shift"] = R.hue_shift_of(hue_factor)
    return rec


def R_DTYPE():
    from dataloaders import AUGMENT_RECORD
    return AUGMENT_RECORD


@pytest.mark.parametrize("k", range(24))
def test_whole_chain_in_every_order_matches_pillow(k):
    import itertools
    order = list(itertools.permutations(range(4)))[k]
    rng = np.random.RandomState(k)
    src = rng.randint(0, 256, (47, 157, 3)).astype(np.uint8)
    factors = tuple(float(np.float32(x)) for x in rng.uniform(0.8, 1.2, 3))
    hue_factor = [0.1, -0.1, 0.5, -0.5][k % 4]
    flip = k % 2 == 1
    rec = _record(R.COLOUR | (R.FLIP if flip else 0), order, *factors, hue_factor)
    want_plain, want_aug = pil_augment(src, 24, 80, flip, order, factors, hue_factor)
    plain, aug = R.augment_bytes(R.pil_resize(src, 24, 80), rec)
    assert np.array_equal(plain, want_plain)
    assert np.array_equal(aug, want_aug)


def test_skipped_operations_and_identity_colour():
    rng = np.random.RandomState(5)
    src = rng.randint(0, 256, (24, 80, 3)).astype(np.uint8)
    rec = _record(R.COLOUR, (0, 1, 2, R.NONE), 1.0, 1.0, 1.0, 0.0)
    plain, aug = R.augment_bytes(src, rec)
    assert np.array_equal(plain, aug)
    rec = _record(R.COLOUR, (R.NONE, 3, R.NONE, R.NONE), 1.0, 1.0, 1.0, 0.2)
    assert np.array_equal(R.augment_bytes(src, rec)[1], np.asarray(adjust_hue(__import__("PIL.Image").Image.fromarray(src), 0.2)))


@pytest.mark.parametrize("src_hw,dst_hw", [((375, 1242), (192, 640)), ((370, 1226), (192, 640)), ((352, 1216), (192, 640)),
                                           ((375, 1242), (320, 1024)), ((47, 156), (24, 80)), ((47, 157), (24, 81))])
def test_mirror_after_resize_equals_pillow_flip_then_resize(src_hw, dst_hw):
    from PIL import Image
    rng = np.random.RandomState(src_hw[1])
    src = rng.randint(0, 256, src_hw + (3,)).astype(np.uint8)
    want = np.asarray(Image.fromarray(src).transpose(Image.FLIP_LEFT_RIGHT).resize(dst_hw[::-1], Image.BILINEAR))
    assert np.array_equal(R.pil_resize(src, *dst_hw)[:, ::-1], want)


def test_restatement_reproduces_the_pinned_fixture(golden):
    g = golden("augment.npz")
    h, w = (int(v) for v in g["size"])
    recs = g["records"].reshape(-1).view(R_DTYPE())
    for f, r, p, a in zip(g["frames"], recs, g["plain"], g["aug"]):
        plain, aug = R.augment_bytes(R.pil_resize(f, h, w), r)
        assert np.array_equal(plain, p) and np.array_equal(aug, a)


# ---------------------------------------------------------------------------------------------------- csrc/augment_math.h on the host
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("augment_hostcheck") / "libaugment_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(REPO, "tests", "augment_hostcheck", "augment_hostcheck.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    p = ctypes.c_void_p
    lib.au_luma.argtypes = [p, ctypes.c_int, p]
    lib.au_blend.argtypes = [p, p, ctypes.c_int, ctypes.c_float, p]
    lib.au_rgb_to_hsv.argtypes = [p, ctypes.c_int, p]
    lib.au_op.argtypes = [p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int]
    lib.au_contrast_mean.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.au_contrast_mean.restype = ctypes.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_host_luma_and_hsv_on_every_colour(host, all_colours):
    flat = np.ascontiguousarray(all_colours.reshape(-1, 3))
    n = flat.shape[0]
    out = np.zeros(n, np.int32)
    host.au_luma(_p(flat), n, _p(out))
    assert np.array_equal(out, R.luma(flat))
    hsv = np.zeros_like(flat)
    host.au_rgb_to_hsv(_p(flat), n, _p(hsv))
    assert np.array_equal(hsv, R.rgb_to_hsv(flat))


@pytest.mark.parametrize("shift", [0, 25, 231])
def test_host_hue_on_every_colour(host, all_colours, shift):
    flat = np.ascontiguousarray(all_colours.reshape(-1, 3))
    got = flat.copy()
    host.au_op(_p(got), got.shape[0], R.HUE, 1.0, shift, 0)
    assert np.array_equal(got, R.hue(flat, shift))


@pytest.mark.parametrize("alpha", ALPHAS)
def test_host_blend_on_every_byte_pair(host, alpha):
    a = (np.arange(65536) >> 8).astype(np.uint8)
    b = (np.arange(65536) & 255).astype(np.uint8)
    out = np.zeros(65536, np.uint8)
    host.au_blend(_p(a), _p(b), 65536, alpha, _p(out))
    assert np.array_equal(out, R.blend(a, b, np.float32(alpha)))


@pytest.mark.parametrize("op", [R.BRIGHTNESS, R.SATURATION, R.CONTRAST])
@pytest.mark.parametrize("f", [0.8, 1.2])
def test_host_enhance_on_every_colour(host, all_colours, op, f):
    flat = np.ascontiguousarray(all_colours.reshape(-1, 3))
    got = flat.copy()
    host.au_op(_p(got), got.shape[0], op, f, 0, 97)
    if op == R.CONTRAST:
        want = R.blend(np.full(flat.shape, 97), flat, np.float32(f)).astype(np.uint8)
    else:
        want = (R.brightness if op == R.BRIGHTNESS else R.saturation)(flat, np.float32(f))
    assert np.array_equal(got, want)


def test_host_contrast_mean(host):
    for S, n in ((21, 2), (0, 5), (255 * 122880, 122880), (122880 * 100 + 61440, 122880), (7, 3), (2 ** 40 + 1, 2 ** 33)):
        assert host.au_contrast_mean(S, n) == int(S / n + 0.5)


# ---------------------------------------------------------------------------------------------------- records and configuration
def test_records_are_deterministic_and_in_bounds():
    from dataloaders import AUG_COLOUR, AUG_FLIP, Augmentation
    a = Augmentation(seed=7, rank=0)
    r0 = a.draw(a.generator(0), 4000)
    assert np.array_equal(r0, a.draw(a.generator(0), 4000))
    g = a.generator(0)                                  # batch boundaries do not matter: the stream is per sample
    assert np.array_equal(np.concatenate([a.draw(g, 12), a.draw(g, 5), a.draw(g, 3983)]), r0)
    assert not np.array_equal(r0, a.draw(a.generator(1), 4000))
    assert not np.array_equal(r0, Augmentation(seed=7, rank=1).draw(Augmentation(seed=7, rank=1).generator(0), 4000))
    assert not np.array_equal(r0, Augmentation(seed=8).draw(Augmentation(seed=8).generator(0), 4000))
    for name in ("brightness", "contrast", "saturation"):
        assert r0[name].min() >= np.float32(0.8) and r0[name].max() <= np.float32(1.2)
    hs = (r0["hue_shift"].astype(np.int64) + 128) % 256 - 128
    assert hs.min() >= -25 and hs.max() <= 25 and r0["hue_shift"].min() >= 0 and r0["hue_shift"].max() <= 255
    assert all(sorted(o) == [0, 1, 2, 3] for o in r0["order"])
    assert len({tuple(o) for o in r0["order"]}) == 24
    flip, col = (r0["flags"] & AUG_FLIP) != 0, (r0["flags"] & AUG_COLOUR) != 0
    assert 0.45 < flip.mean() < 0.55 and 0.45 < col.mean() < 0.55
    assert set(np.unique(r0["flags"])) <= {0, 1, 2, 3}


def test_zero_probabilities_and_ranges():
    from dataloaders import AUG_OP_NONE, Augmentation
    a = Augmentation(p_color=0.0, p_flip=0.0)
    assert (a.draw(a.generator(3), 1000)["flags"] == 0).all()
    a = Augmentation(brightness=0.0, hue=0.0, p_color=1.0, p_flip=1.0)
    r = a.draw(a.generator(0), 100)
    assert (r["flags"] == 3).all() and (r["brightness"] == 1.0).all()
    for o in r["order"]:
        assert sorted(o) == [1, 2, AUG_OP_NONE, AUG_OP_NONE]


def _config(**aug):
    import yaml
    cfg = yaml.full_load(open(os.path.join(PKG, "configs", "basic_config.yaml")))
    cfg["datasets"]["dataset"] = ["KITTI"]
    cfg["datasets"]["augmentation"].update(aug)
    return cfg


def test_config_keys():
    from dataloaders import Augmentation
    assert Augmentation.from_config(_config()) is None
    a = Augmentation.from_config(_config(color_jitter={"brightness": 0.2, "contrast": 0.2, "saturation": 0.2, "hue": 0.1, "p": 0.5},
                                         flip=0.5), rank=3)
    assert (a.brightness, a.contrast, a.saturation, a.hue, a.p_color, a.p_flip, a.seed, a.rank) == (0.2, 0.2, 0.2, 0.1, 0.5, 0.5, 42, 3)
    a = Augmentation.from_config(_config(flip=0.25))
    assert a.p_color == 0.0 and a.p_flip == 0.25
    a = Augmentation.from_config(_config(color_jitter={"hue": 0.05}))
    assert (a.brightness, a.hue, a.p_color, a.p_flip) == (0.2, 0.05, 0.5, 0.0)


@pytest.mark.parametrize("aug,match", [({"colour_jitter": {}}, "unknown"), ({"color_jitter": {"gamma": 0.1}}, "unknown"),
                                       ({"color_jitter": {"hue": 0.6}}, "hue"), ({"color_jitter": {"p": 1.5}}, "probability"),
                                       ({"color_jitter": {"p": -0.1}}, "probability"), ({"flip": 2.0}, "probability"),
                                       ({"flip": -1}, "probability"), ({"color_jitter": {"brightness": -0.2}}, "brightness"),
                                       ({"color_jitter": 0.2}, "mapping")])
def test_bad_configs_are_rejected(aug, match):
    from dataloaders import Augmentation
    with pytest.raises(ValueError, match=match):
        Augmentation.from_config(_config(**aug))


def test_synthetic_batches_are_not_augmented():
    from dataloaders import Augmentation
    cfg = _config(flip=0.5)
    cfg["datasets"]["dataset"] = ["synthetic"]
    with pytest.raises(ValueError, match="synthetic"):
        Augmentation.from_config(cfg)


def test_record_layout_matches_header():
    from dataloaders import AUG_COLOUR, AUG_FLIP, AUG_OP_NONE, AUGMENT_RECORD
    text = open(os.path.join(REPO, "include", "mcav_depth.h")).read()
    assert AUGMENT_RECORD.itemsize == 24 and "/* 24 bytes */" in text
    assert list(AUGMENT_RECORD.names) == ["flags", "order", "brightness", "contrast", "saturation", "hue_shift"]
    for name, v in (("FLIP", AUG_FLIP), ("COLOUR", AUG_COLOUR), ("OP_BRIGHTNESS", R.BRIGHTNESS), ("OP_CONTRAST", R.CONTRAST),
                    ("OP_SATURATION", R.SATURATION), ("OP_HUE", R.HUE), ("OP_NONE", AUG_OP_NONE)):
        assert "#define MCAV_AUG_%s %d\n" % (name, v) in text
