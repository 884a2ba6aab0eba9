"""Independent restatement of the meters-per-pixel scan (test infrastructure): plain sequential Python written from
src/vision/mpx_ratio.rs:3-134 -- one row, one column, one pixel at a time.  It shares no code with oracle/smh_oracle.c;
tests/test_scale_host.py compares the two, and the GPU tests rest on the oracle.

Three points the reference leaves to an unchecked read or to release-mode integer arithmetic are defined as the oracle
documents them:
  * a pixel below the image counts as non-zero (the tick test fails there),
  * an anchor with x >= width gives None,
  * `right - left` -- and every other u32 sum of the scan -- wraps modulo 2^32.
"""

MIN_SCALE_WIDTH = 10
MIN_SCALE_VERTICAL_BAR_HEIGHT = 4
_U32 = 1 << 32


def _rust_round(v):
    """f64::round for v >= 0: half away from zero."""
    n = int(v)
    return n + 1 if v - n >= 0.5 else n


def max_scale_y_offset(width):
    return _rust_round((20.0 / 640.0) * float(width)) % _U32


def _is_zero(image, x, y):
    """image.get_pixel(x, y).0[0] == 0; below the image: non-zero."""
    if y >= len(image):
        return False
    return int(image[y][x]) == 0


def _is_tick(image, x, y):
    """mpx_ratio.rs:23-28, 43-48: `(y..y + 4).chain((y..y - 4).rev())` -- the second range is empty (y - 4 < y, and
    y >= 4 so it does not wrap): the pixels (x, y) .. (x, y + 3), one after the other."""
    for ty in range(y, y + MIN_SCALE_VERTICAL_BAR_HEIGHT):
        if not _is_zero(image, x, ty):
            return False
    return True


def find_scale_width(meters, x, y, image):
    """image: rows of pixels (a numpy uint8[h, w] or a list of lists) -> (meters / width, (left, y, right)) or None."""
    height, width = len(image), len(image[0])
    if y < MIN_SCALE_VERTICAL_BAR_HEIGHT:
        return None
    if x >= width:
        return None
    y_end = min(height, (y + max_scale_y_offset(width)) % _U32)
    yy = y
    while yy < y_end:                                   # Go down...
        if _is_zero(image, x, yy):
            right = 0                                   # Go right...
            xx = x
            while xx < width:
                if _is_tick(image, xx, yy):
                    right = xx
                    break
                xx += 1
            if right == 0:
                yy += 1
                continue
            right -= 1
            left = 0                                    # Go left...
            xx = x
            while xx > 0:
                xx -= 1
                if _is_tick(image, xx, yy):
                    left = xx
                    break
            if left == 0:
                yy += 1
                continue
            left += 1
            w = (right - left) % _U32
            if w < MIN_SCALE_WIDTH:
                yy += 1
                continue
            return float(meters) / float(w), (left, yy, right)
        yy += 1
    return None


def calc_meters_to_px_ratio(scales, image):
    """scales: [(meters, x, y)], at most three -> (ratio or None, [(left, y, right) or None per anchor]).  The "Rayon
    ladder" (mpx_ratio.rs:91-125) spelled out: the mean of the successes, summed in index order."""
    if len(scales) == 0:
        return None, []
    assert len(scales) <= 3                             # `_ => unreachable!()`
    found = [find_scale_width(m, x, y, image) for (m, x, y) in scales]
    bars = [f[1] if f is not None else None for f in found]
    r = [f[0] if f is not None else None for f in found]
    if len(r) == 1:
        return r[0], bars
    if len(r) == 2:
        a, b = r
        if a is not None and b is not None:
            return (a + b) / 2.0, bars
        if a is not None:
            return a, bars
        return b, bars
    a, b, c = r
    if a is not None and b is not None and c is not None:
        return (a + b + c) / 3.0, bars
    if a is not None and b is not None:
        return (a + b) / 2.0, bars
    if a is not None and c is not None:
        return (a + c) / 2.0, bars
    if b is not None and c is not None:
        return (b + c) / 2.0, bars
    for v in (a, b, c):
        if v is not None:
            return v, bars
    return None, bars
