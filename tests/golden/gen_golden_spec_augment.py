#!/usr/bin/env python3
"""Generate tests/golden/spec_augment_cases.npz: a record of the REFERENCE's own `spec_augment` (models/audioset_dataset.py:17-55), loaded
read-only by path (librosa, which that file imports and this function never uses, stubbed as tests/golden/gen_golden_audioset_feed.py does).
Per case (tau, F, T, n_freq, n_time) and seed -- `random` and `np.random` both seeded with it -- the function runs on an index-filled array
[1, 40, tau] (no cell is 0 before it), and what is stored is data only: the zero pattern it left (uint8 [40, tau]), CRC32s of both
generators' states afterwards, or `refused` = 1 where its `random.randint` raised (a mask wider than the axis).

    M3T_REFERENCE=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_spec_augment.py
"""
import importlib.util
import os
import random
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

#         tau  F     T   n_freq n_time
CASES = [(97, 20, 20, 1, 1),            # the defaults on a 32-frame clip at 30 fps
         (193, 20, 20, 1, 1),           # ... at 15 fps
         (97, 40, 30, 2, 2),
         (25, 8.5, 10, 4, 4),           # the most masks taken, overlapping; a fractional parameter
         (13, 20, 10, 1, 1),            # a 4-frame clip
         (13, 20, 20, 1, 1),            # ... where T reaches past tau: some seeds are refused
         (97, 60, 20, 1, 1),            # F past the 40 bands: some seeds are refused
         (97, 0, 0, 1, 1),              # f = 0 and t = 0: nothing is masked, four draws are made
         (97, 20, 20, 0, 3), (97, 20, 20, 3, 0)]
SEEDS = list(range(8))


def load_reference():
    ref = os.environ.get("M3T_REFERENCE")
    if not ref:
        raise SystemExit("set M3T_REFERENCE to the reference's checkout")
    sys.modules.setdefault("librosa", types.ModuleType("librosa"))
    spec = importlib.util.spec_from_file_location("reference_audioset_dataset", os.path.join(ref, "models", "audioset_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def random_crc():
    return zlib.crc32(repr(random.getstate()).encode())


def numpy_crc():
    kind, keys, pos, has_gauss, gauss = np.random.get_state()
    return zlib.crc32(keys.tobytes() + repr((kind, int(pos), int(has_gauss), float(gauss))).encode())


def main():
    ref = load_reference()
    out = {"cases": np.array(CASES, np.float64), "seeds": np.array(SEEDS, np.int64)}
    refused = 0
    for c, (tau, F, T, n_freq, n_time) in enumerate(CASES):
        for seed in SEEDS:
            random.seed(seed)
            np.random.seed(seed)
            spec = np.arange(1, 40 * tau + 1, dtype=np.float32).reshape(1, 40, tau)
            key = "c%d.s%d." % (c, seed)
            try:
                got = ref.spec_augment(spec, F, T, n_freq, n_time)
            except ValueError:
                out[key + "refused"] = np.array([1], np.uint8)
                refused += 1
                continue
            assert got.shape == (1, 40, tau)
            out[key + "refused"] = np.array([0], np.uint8)
            out[key + "zero"] = (got[0] == 0).astype(np.uint8)
            out[key + "random_crc"] = np.array([random_crc()], np.uint32)
            out[key + "numpy_crc"] = np.array([numpy_crc()], np.uint32)
    # what the set is there to cover
    assert 0 < refused < len(SEEDS) * 2 and all(out["c%d.s%d.refused" % (c, s)][0] == 0 for c in (0, 1, 2, 3, 4, 7, 8, 9) for s in SEEDS)
    assert not any(out["c7.s%d.zero" % s].any() for s in SEEDS)
    assert any(out["c3.s%d.zero" % s].all(0).any() and out["c3.s%d.zero" % s].all(1).any() for s in SEEDS)
    path = os.path.join(HERE, "spec_augment_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote spec_augment_cases.npz %.1f KB, %d runs, %d refused" % (os.path.getsize(path) / 1024, len(CASES) * len(SEEDS), refused))


if __name__ == "__main__":
    main()
