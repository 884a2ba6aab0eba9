#!/usr/bin/env python3
"""Generates the scale-label fixtures under tests/golden/ from the reference's own sample screenshots, in the manner of
make_goldens.py: CPU only, run where the reference tree is (the fixtures it writes are plain data).

For each of four 2560 x 1440 screenshots that show scale labels it writes `<stem>.labels.webp`: rows 370..547, all 657 columns,
of the bottom-right quadrant (the oracle's cropped_brq, RGB), lossless.  The labels and their bars lie in these rows; the rest
of the quadrant is map terrain that the tests do not need.  `scale_labels.json` holds, per stem, the strip's first row and the
texts of the labels the restatement (tests/scale_labels_ref.py) proposes on the WHOLE screenshot, in its order, read by eye
("" where the proposal is no label), with the proposals themselves as (left, top, right, bottom, bar_left, bar_y, bar_right).
A test pastes a strip into a frame of its own (tests/scale_label_cases.py:strip_frame).
"""
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle as o  # noqa: E402
import scale_labels_ref as R  # noqa: E402
from make_goldens import SAMPLES, webp_bytes  # noqa: E402

ROW0, ROW1 = 370, 548
# read by eye off the enlarged crops; "difficult" also proposes two glyphs of the map's grid text that sit over the lower bar
TEXTS = {
    "albasrah.png": ["300m", "900m"],
    "difficult.png": ["300m", "900m", "8", ")"],
    "glorious.png": ["100m", "300m", "900m"],
    "in_mortar.png": ["300m", "900m"],
}


def main():
    table = {}
    for name, texts in sorted(TEXTS.items()):
        stem = name.replace(".", "_")
        rgb = np.array(Image.open(os.path.join(SAMPLES, name)).convert("RGB"))
        H, W, _ = rgb.shape
        assert (W, H) == (2560, 1440), name
        bgra = np.ascontiguousarray(np.dstack([rgb[:, :, 2], rgb[:, :, 1], rgb[:, :, 0], np.full((H, W), 255, np.uint8)]))
        brq = o.crop_to_map(bgra, True)["cropped_brq"]
        assert brq.shape == (ROW1, 657, 3), brq.shape
        res = R.scale_labels(o.ocr_preprocess(brq), o.find_scales_preprocess(brq, 0))
        assert res["header"][0] == res["header"][1] == len(texts), (name, res["header"])
        strip = np.ascontiguousarray(brq[ROW0:ROW1])
        data = webp_bytes(strip)
        assert len(data) < (1 << 20), (name, len(data))
        with open(os.path.join(HERE, stem + ".labels.webp"), "wb") as f:
            f.write(data)
        table[stem] = dict(source=name, row0=ROW0, texts=texts, proposals=[list(map(int, p[:7])) for p in res["labels"]])
        print(stem, len(data), table[stem])
    with open(os.path.join(HERE, "scale_labels.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
