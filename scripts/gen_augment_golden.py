"""Writes tests/golden/augment/*.npz: for every case of tests/augment_forms.py (one row with everything on) the input image, the row
and what PILLOW makes of it (nopesac_amd.augment.augment_pil: ImageEnhance, convert, ImageFilter.GaussianBlur - no restatement, no
kernel).  The GPU tests hold the kernels to these files directly.  Needs Pillow only:  python scripts/gen_augment_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nopesac_amd.augment import augment_pil     # noqa: E402
from tests import augment_forms as A            # noqa: E402


def main():
    import PIL
    os.makedirs(A.GOLDEN, exist_ok=True)
    rows = dict(A.CHAIN_ROWS, **A.COLOUR_CHAIN_ROWS)
    for k, name in enumerate(A.GOLDEN_CASES):
        image = A.noise_image(37, 53, seed=100 + k) if k % 2 == 0 else A.ramp_image(37, 53)
        row = rows[name]
        np.savez_compressed(os.path.join(A.GOLDEN, name + ".npz"), image=image, expected=augment_pil(image, row), jitter=row.jitter,
                            order=np.array(row.order, np.int32), factors=np.array(row.factors, np.float32), grey=row.grey, blur=row.blur,
                            sigma=np.float32(row.sigma), pillow=np.array(PIL.__version__))
        print("wrote", name)


if __name__ == "__main__":
    main()
