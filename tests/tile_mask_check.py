"""What the streaming passes leave for the line search (include/smh_vision_hip.h, smhv_batch_tile_mask), checked against a marker
mask: shared by tests/test_gpu_configs.py and tests/test_geometry_sweep_gpu.py."""
import numpy as np


def check_tile_mask(fb, f, mask, expect_tiles, ctx):
    """Frame f of FrameBatch fb after a run.  The bit rows are `mask` (uint8 [rh, rw], non-zero = set; bit x + xoff of row y =
    pixel x); the tile-major mask was written exactly when expect_tiles; where it was, the occupancy bytes name exactly the
    non-empty 32 x 8 tiles of those rows and every such tile holds the rows' words (rows of the last tile row beyond the image
    are undefined).  -> (tiled, occ, bits, xoff) as fb.tile_mask gives them."""
    tiled, occ, bits, xoff = fb.tile_mask(f)
    rh, rw = mask.shape
    wcols = bits.shape[1]
    trows = (rh + 7) // 8
    assert (tiled is not None) == bool(expect_tiles), ctx
    assert bits.shape == (rh, wcols), ctx
    px = np.zeros((rh, wcols * 32), np.uint8)
    px[:, xoff:xoff + rw] = mask != 0
    want_bits = np.packbits(px.reshape(rh, wcols, 32), axis=2, bitorder="little").view(np.uint32).reshape(rh, wcols)
    assert np.array_equal(bits, want_bits), ctx
    if tiled is None:
        return tiled, occ, bits, xoff
    assert tiled.shape == (trows, wcols, 8), ctx
    padded = np.zeros((trows * 8, wcols), np.uint32)
    padded[:rh] = bits
    by_tile = padded.reshape(trows, 8, wcols).transpose(0, 2, 1)            # [ty, wx, r]
    nonempty = by_tile.any(axis=2)
    got_occ = np.unpackbits(occ, axis=1, bitorder="little")[:, :wcols].astype(bool)
    assert np.array_equal(got_occ, nonempty), (ctx, int(nonempty.sum()), int(got_occ.sum()))
    tail = rh - (trows - 1) * 8                                               # rows of the last tile row inside the image
    a, b_ = tiled[nonempty], by_tile[nonempty]
    last = np.repeat(np.arange(trows)[:, None], wcols, axis=1)[nonempty] == trows - 1
    assert np.array_equal(a[~last], b_[~last]) and np.array_equal(a[last][:, :tail], b_[last][:, :tail]), ctx
    return tiled, occ, bits, xoff
