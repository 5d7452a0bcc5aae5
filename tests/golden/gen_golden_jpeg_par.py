"""Writes tests/golden/jpeg_par_cases.npz: the fixtures the parallel walk of the JPEG decode adds to tests/golden/jpeg_cases.npz
(tests/test_jpeg_par_host.py, tests/test_gpu_jpeg_par.py).  Each case stresses one thing a walk split into sub-sequences can get wrong:

  p_noise_444_q100   32 x 32 uniform noise, quality 100, 4:4:4: about 87 bytes a block, so sub-sequences of 16 to 64 bytes lie inside one
                     block; dozens of stuffed FF 00, some on granule and sub-sequence borders
  p_flat_420_q30     256 x 256 of one colour, quality 30, 4:2:0: under a byte a block, a sub-sequence holds dozens of blocks and several
                     MCUs (block counting, the DC prefix sums)
  p_ramp_420_q75     64 x 64 horizontal / vertical ramps, quality 75, 4:2:0: a few bytes a block, long DC chains of non-zero differences
  p_rows_420_rst     64 x 64 noise, quality 90, 4:2:0, a restart marker every MCU row: four segments, the predictors reset
  p_gray_odd_q92     37 x 23 gray noise, quality 92: one block an MCU, edge MCUs
  p_422_opt_q97      24 x 40 noise, quality 97, 4:2:2, optimised tables: codes past the 9-bit lookup

Pillow (libjpeg-turbo) encodes seeded numpy content and decodes it again; the file holds each case's bytes (`<name>.jpg`) and Pillow's
pixels (`<name>.rgb`), and the numpy restatement must equal them.  Run from the repository root: python tests/golden/gen_golden_jpeg_par.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import jpeg_ref  # noqa: E402
from gen_golden_jpeg import encode, pillow_rgb  # noqa: E402


def noise(H, W, seed, channels=3):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (H, W, channels) if channels > 1 else (H, W)).astype(np.uint8)


def cases():
    out = {}
    out["p_noise_444_q100"] = encode(noise(32, 32, 31), quality=100, subsampling=0)
    flat = np.empty((256, 256, 3), np.uint8)
    flat[:] = (200, 90, 40)
    out["p_flat_420_q30"] = encode(flat, quality=30, subsampling=2)
    y, x = np.mgrid[0:64, 0:64]
    ramp = np.stack([4 * x, 4 * y, 2 * (x + y)], axis=2).clip(0, 255).astype(np.uint8)
    out["p_ramp_420_q75"] = encode(ramp, quality=75, subsampling=2)
    out["p_rows_420_rst"] = encode(noise(64, 64, 34), quality=90, subsampling=2, restart_marker_rows=1)
    out["p_gray_odd_q92"] = encode(noise(37, 23, 35, channels=1), quality=92)
    out["p_422_opt_q97"] = encode(noise(24, 40, 36), quality=97, subsampling=1, optimize=True)
    return out


def main():
    arrays, stats = {}, {}
    made = cases()
    for name, data in made.items():
        rgb = pillow_rgb(data)
        ref, st = jpeg_ref.decode(data)
        assert np.array_equal(ref, rgb), "%s: the restatement differs from Pillow" % name
        stats[name] = st
        arrays[name + ".jpg"] = np.frombuffer(data, np.uint8)
        arrays[name + ".rgb"] = rgb
    # coverage the tests rely on
    scan = lambda d: d[d.index(b"\xff\xda"):]
    assert scan(made["p_noise_444_q100"]).count(b"\xff\x00") >= 8 and len(made["p_noise_444_q100"]) > 3500
    assert len(made["p_flat_420_q30"]) < 3000 and pillow_rgb(made["p_flat_420_q30"]).shape == (256, 256, 3)
    assert stats["p_rows_420_rst"]["restarts"] == 3
    assert stats["p_422_opt_q97"]["max_code_length"] > 9, stats["p_422_opt_q97"]
    assert pillow_rgb(made["p_gray_odd_q92"]).shape == (37, 23, 3)
    path = os.path.join(HERE, "jpeg_par_cases.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("%s: %d cases, %d bytes; %s" % (path, len(stats), size, {n: len(d) for n, d in made.items()}))


if __name__ == "__main__":
    main()
