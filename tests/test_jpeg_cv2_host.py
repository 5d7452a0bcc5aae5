"""For whoever has OpenCV: `cv2.imread` -- the reference's decoder (models/dataset.py:64) -- against the goldens Pillow made
(tests/golden/jpeg_cases.npz).  m3t/jpeg.py pins libjpeg-turbo's default bits and argues from OpenCV's published source that cv2 gives the
same; cv2 is not installed where the project is developed, so this is the run that argument still lacks.  Skipped without cv2."""
import numpy as np
import pytest

import jpeg_cases

cv2 = pytest.importorskip("cv2")
CASES, _ = jpeg_cases.load()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cv2_imread_equals_the_golden(name, tmp_path):
    data, rgb = CASES[name]
    path = str(tmp_path / (name + ".jpg"))
    with open(path, "wb") as f:
        f.write(data)
    img = cv2.imread(path)                                  # BGR; a gray file is replicated into three channels
    assert img is not None and np.array_equal(img, rgb[..., ::-1])
