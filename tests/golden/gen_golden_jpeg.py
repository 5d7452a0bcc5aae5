"""Writes tests/golden/jpeg_cases.npz: the JPEG fixtures of tests/test_jpeg_host.py and tests/test_gpu_jpeg.py.  Pillow (libjpeg-turbo)
encodes seeded numpy content -- gradients, a sinusoid and noise, so that all coefficient positions and both clamps occur -- and decodes it
again; the file holds each case's bytes (`<name>.jpg`, a uint8 array) and Pillow's pixels (`<name>.rgb`, uint8 [H, W, 3]).  The refusal
cases (`refuse_*.jpg`) are bytes only.  Run from the repository root: python tests/golden/gen_golden_jpeg.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref  # noqa: E402

SUB = {"444": 0, "422": 1, "420": 2}
EDGE_SIZES = [(1, 1), (2, 2), (5, 3), (6, 4), (3, 5), (7, 6), (1, 9), (2, 17), (17, 9), (16, 16), (31, 16)]


def content(H, W, seed, noise=10.0):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([255.0 * x / max(W - 1, 1), 255.0 * y / max(H - 1, 1), 127.5 + 127.5 * np.sin(0.9 * x + 0.5 * y)], axis=2)
    return np.clip(img + rs.normal(0.0, noise, img.shape), 0, 255).astype(np.uint8)


def sparse(H, W, seed):
    """flat areas with isolated high-frequency detail: long zero runs (ZRL) and a skewed symbol histogram (long optimised codes)"""
    rs = np.random.RandomState(seed)
    img = content(H, W, seed, noise=0.0).astype(np.float64)
    y, x = np.mgrid[0:H, 0:W]
    img += ((x + y) % 2)[:, :, None] * rs.uniform(0, 60, (H // 8 + 1, W // 8 + 1, 1)).repeat(8, 0).repeat(8, 1)[:H, :W] * (rs.uniform(size=(H, W, 1)) < 0.5)
    img += rs.normal(0.0, 1.0, img.shape) * np.exp(rs.uniform(0, 4, (H, W, 1)))
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def cases():
    out = {}
    H, W = 40, 56
    out["f_420_q95"] = encode(content(H, W, 1), quality=95, subsampling=2)
    out["f_444_q60"] = encode(content(H, W, 2), quality=60, subsampling=0)
    out["f_422_q85"] = encode(content(H, W, 3), quality=85, subsampling=1)
    out["f_gray_q80"] = encode(content(H, W, 4)[:, :, 0], quality=80)
    out["f_opt_q90"] = encode(sparse(H, W, 5), quality=90, subsampling=2, optimize=True)
    out["f_rst_blocks2"] = encode(content(H, W, 6), quality=90, subsampling=2, restart_marker_blocks=2)
    out["f_rst_rows1_q100"] = encode(content(H, W, 7), quality=100, subsampling=2, restart_marker_rows=1)
    out["f_sat_q50"] = encode((np.random.RandomState(8).randint(0, 2, (H, W, 3)) * 255).astype(np.uint8), quality=50, subsampling=2)
    for (h, w) in EDGE_SIZES:
        for sub in ("420", "422"):
            out["e_%dx%d_%s" % (h, w, sub)] = encode(content(h, w, 100 + 7 * h + w), quality=30 if (h, w) == (17, 9) else 90, subsampling=SUB[sub])
    out["full_256_q95"] = encode(content(256, 256, 9), quality=95, subsampling=2)
    return out


def refusals():
    out = {"refuse_progressive": encode(content(16, 16, 20), quality=80, progressive=True)}
    buf = io.BytesIO()
    Image.fromarray(content(16, 16, 21)).convert("CMYK").save(buf, "JPEG", quality=80)
    out["refuse_cmyk"] = buf.getvalue()
    return out


def main():
    arrays = {}
    stats = {}
    for name, data in cases().items():
        rgb = pillow_rgb(data)
        ref, st = jpeg_ref.decode(data)
        assert np.array_equal(ref, rgb), "%s: the restatement differs from Pillow" % name
        stats[name] = st
        arrays[name + ".jpg"] = np.frombuffer(data, np.uint8)
        arrays[name + ".rgb"] = rgb
    # coverage the tests rely on
    # (an optimised table with a 16-bit code needs a Huffman tree of depth 16, i.e. at least F(18) = 2584 symbols of one table in
    # Fibonacci proportions: out of reach of a 40 x 56 image, whose optimised tables stop at 11 bits.  So: the optimised case must use
    # codes past the 9-bit lookup table, and 16-bit codes must occur in the family under the standard tables.)
    assert stats["f_opt_q90"]["zrl"] >= 1 and stats["f_opt_q90"]["max_code_length"] > 9, stats["f_opt_q90"]
    assert sum(stats[n]["max_code_length"] == 16 for n in stats if n.startswith("f_")) >= 2 and stats["full_256_q95"]["max_code_length"] == 16
    assert stats["f_rst_blocks2"]["restarts"] > 0 and stats["f_rst_rows1_q100"]["restarts"] > 0
    assert stats["f_sat_q50"]["clamp_low"] > 0 and stats["f_sat_q50"]["clamp_high"] > 0, stats["f_sat_q50"]
    for name, data in refusals().items():
        arrays[name + ".jpg"] = np.frombuffer(data, np.uint8)
    path = os.path.join(HERE, "jpeg_cases.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("%s: %d cases, %d bytes; full frame %d bytes" % (path, len(stats), size, len(cases()["full_256_q95"])))


if __name__ == "__main__":
    main()
