#!/usr/bin/env python
"""Generate tests/golden/colorize_r8_write.npz by RUNNING the reference's own colorize + imwrite.

Run in the build container only (needs /root/reference; nothing here travels to the GPU machine):

    python tests/golden/make_colorize_r8.py

The fixture pins the colourise of an 8-BIT reflectance map (rf_colorize_ragged_r8_srgb_u8: a
filtered `-r.png` on the device): small photos, reflectance bytes, and the bytes the reference's
image_utils.colorize + imwrite(sRGB=True) hand to cv2.imwrite for the float32 map
bytes.astype(np.float32) / np.float32(255).  As in make_golden.py the reference's image_utils is
imported under a stub `cv2` that records what imwrite is given.  Cases:

  ramp   16x20: every byte value 0..255, the one byte 0 under a lit pixel (shading +inf); both
         results normalised
  photo  33x31: a natural-looking photo under a smooth map with noise; both results normalised
  dark   9x11:  a grey 0/1 photo under bytes 255 (and any byte under black): max <= 1 for both
         results, written as they are
  nan    7x13:  bytes 1 under map bytes 240..255 and one byte 0 under a black pixel: 0/0 = NaN in both
         results, which are written without normalisation

Before saving, the script checks that no finite value of an unnormalised NaN result reaches byte 256
(numpy's uint8 cast overflows there and the byte depends on the platform) and that the recorded
bytes equal oracle.colorize_numpy.colorize_srgb_u8 on the same float32 map.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)

files_out = {}
cv2 = types.ModuleType("cv2")


def _imwrite(filename, image):
    files_out[filename] = np.array(image, copy=True)
    return True


cv2.imread = lambda filename: None
cv2.imwrite = _imwrite
sys.modules["cv2"] = cv2
sys.path.insert(0, REF)
import image_utils as ref_iu  # noqa: E402

from oracle import colorize_numpy as oc  # noqa: E402

TAGS = ("ramp", "photo", "dark", "nan")


def cases():
    rng = np.random.default_rng(2608)
    out = {}
    # every byte value once and 64 more, byte 0 exactly once and under a lit pixel
    img = rng.integers(1, 256, (16, 20, 3)).astype(np.uint8)
    r8 = np.concatenate([np.arange(256), rng.integers(1, 256, 64)]).astype(np.uint8)
    out["ramp"] = (img, rng.permutation(r8).reshape(16, 20))
    yy, xx = np.mgrid[0:33, 0:31]
    base = 110 + 70 * np.sin(yy / 7.0) * np.cos(xx / 5.0)
    img = np.clip(base[:, :, None] + rng.normal(0, 25, (33, 31, 3)), 0, 255).astype(np.uint8)
    r8 = np.clip(140 + 90 * np.cos(yy / 9.0) * np.sin(xx / 4.0) + rng.normal(0, 6, (33, 31)), 1, 255)
    out["photo"] = (img, r8.astype(np.uint8))
    grey = rng.integers(0, 2, (9, 11, 1)).astype(np.uint8)
    img = np.repeat(grey, 3, axis=2)
    r8 = np.where(grey[:, :, 0] == 1, 255, rng.integers(1, 256, (9, 11))).astype(np.uint8)
    out["dark"] = (img, r8)
    img = np.ones((7, 13, 3), np.uint8)
    r8 = rng.integers(240, 256, (7, 13)).astype(np.uint8)
    img[3, 5], r8[3, 5] = 0, 0
    out["nan"] = (img, r8)
    return out


def main():
    arrays, seen = {}, set()
    for tag, (img, r8) in cases().items():
        r = r8.astype(np.float32) / np.float32(255)
        files_out.clear()
        with np.errstate(all="ignore"):
            refl, shad = ref_iu.colorize(r, img)
            ref_iu.imwrite("/out/x-r_colorized.png", refl, sRGB=True)
            ref_iu.imwrite("/out/x-s_colorized.png", shad, sRGB=True)
            want = oc.colorize_srgb_u8(img, r)
        got = files_out["/out/x-r_colorized.png"], files_out["/out/x-s_colorized.png"]
        for x, g, w in zip((refl, shad), got, want):
            x = np.asarray(x, dtype=np.float64)
            if np.isnan(x).any():           # written as it is: the cast must not overflow
                with np.errstate(all="ignore"):
                    srgb = np.asarray(ref_iu.rgb_to_srgb(np.where(np.isnan(x), 0.0, x)), dtype=np.float64)
                assert np.isfinite(x[~np.isnan(x)]).all() and not (np.trunc(srgb * 255) >= 256).any(), tag
                seen.add("nan")
            else:
                seen.add("norm" if x.max() > 1 else "plain")
            assert g.dtype == np.uint8 and np.array_equal(g, w), tag
        seen.update(np.unique(r8).tolist())
        arrays[tag + "_image"], arrays[tag + "_r8"] = img, r8
        arrays[tag + "_refl_png"], arrays[tag + "_shading_png"] = got
    assert seen >= set(range(256)) | {"nan", "norm", "plain"}, seen
    img, r8 = cases()["ramp"]
    assert (r8 == 0).sum() == 1 and img[r8 == 0].min() > 0          # shading +inf
    img, r8 = cases()["nan"]
    assert (r8 == 0).sum() == 1 and img[r8 == 0].max() == 0         # 0/0
    np.savez_compressed(os.path.join(HERE, "colorize_r8_write.npz"), **arrays)
    print("wrote colorize_r8_write.npz", {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
