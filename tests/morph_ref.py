"""hc_morphology_device / hc_structuring_element restated in numpy (include/hipcanny.h states the contract).  A plain helper
module: tests/test_morph_ref_cpu.py anchors it against scipy.ndimage, tests/test_gpu_morphology.py compares the device with it.

The element is K = len(spans) half-widths: row j covers the columns -spans[j] .. +spans[j] around the anchor (the centre), -1 is
an empty row.  dilate: out(y, x) = max over j, dx of src(y + j - K/2, x + dx); erode: min.  No reflection.  Positions outside
the frame never take part; a window with none inside gives 0 (dilate) or 255 (erode), and the gradient, a saturating difference, 0.  Channels are
independent."""
import numpy as np

ERODE, DILATE, OPEN, CLOSE, GRADIENT = 0, 1, 2, 3, 4
OPS = (ERODE, DILATE, OPEN, CLOSE, GRADIENT)
RECT, CROSS, ELLIPSE = 0, 1, 2
SHAPES = (RECT, CROSS, ELLIPSE)
KSIZES = (3, 5, 7)


def structuring_spans(shape, ksize):
    """cv::getStructuringElement(shape, Size(ksize, ksize)) as half-widths per row."""
    if ksize not in KSIZES or shape not in SHAPES:
        raise ValueError("shape RECT / CROSS / ELLIPSE, ksize 3, 5 or 7")
    r = ksize // 2
    if shape == RECT:
        return [r] * ksize
    if shape == CROSS:
        return [r if j == r else 0 for j in range(ksize)]
    return [int(np.rint(r * np.sqrt((r * r - (j - r) * (j - r)) / float(r * r)))) for j in range(ksize)]


def footprint(spans):
    """The element as a boolean K x K mask."""
    k = len(spans)
    fp = np.zeros((k, k), bool)
    for j, s in enumerate(spans):
        if s >= 0:
            fp[j, k // 2 - s:k // 2 + s + 1] = True
    return fp


def _check(spans):
    k = len(spans)
    if k not in KSIZES or any(s < -1 or s > k // 2 for s in spans) or all(s < 0 for s in spans):
        raise ValueError(f"bad spans {spans}")
    return k


def _extreme(frames, spans, lo):
    """max (lo = 0) or min (lo = 255) over the element; frames (n, H, W) or (n, H, W, C) u8."""
    k = _check(spans)
    a = np.asarray(frames, dtype=np.uint8)
    h, w = a.shape[1:3]
    r = k // 2
    pad = [(0, 0), (r, r), (r, r)] + [(0, 0)] * (a.ndim - 3)
    p = np.pad(a, pad, mode="constant", constant_values=lo)   # the identity of the extreme: outside never takes part
    out = np.full(a.shape, lo, np.uint8)
    pick = np.maximum if lo == 0 else np.minimum
    for j, s in enumerate(spans):
        for dx in range(-s, s + 1):
            out = pick(out, p[:, j:j + h, r + dx:r + dx + w])
    return out


def dilate(frames, spans):
    return _extreme(frames, spans, 0)


def erode(frames, spans):
    return _extreme(frames, spans, 255)


def _sub_sat(d, e):
    """d - e saturated at 0, as cv::morphologyEx subtracts: the erosion exceeds the dilation only where the window holds no
    position inside the frame (0 against 255), and the gradient is 0 there."""
    return np.where(d >= e, d - e, 0).astype(np.uint8)


def morph(frames, op, spans, channels=None):
    """One call of hc_morphology_device on (n, H, W) / (n, H, W, 3) u8 frames (channels: checked against the shape when given)."""
    a = np.asarray(frames, dtype=np.uint8)
    if channels is not None and channels != (a.shape[3] if a.ndim == 4 else 1):
        raise ValueError("channels does not match the frames")
    if op == ERODE:
        return erode(a, spans)
    if op == DILATE:
        return dilate(a, spans)
    if op == OPEN:
        return dilate(erode(a, spans), spans)
    if op == CLOSE:
        return erode(dilate(a, spans), spans)
    if op == GRADIENT:
        return _sub_sat(dilate(a, spans), erode(a, spans))
    raise ValueError("op")


def morph_iterated(frames, op, spans, iterations):
    """cv::morphologyEx with iterations: OPEN = erode^n then dilate^n, CLOSE the reverse, GRADIENT = dilate^n - erode^n."""
    def rep(a, f):
        for _ in range(iterations):
            a = f(a, spans)
        return a
    a = np.asarray(frames, dtype=np.uint8)
    if op == ERODE:
        return rep(a, erode)
    if op == DILATE:
        return rep(a, dilate)
    if op == OPEN:
        return rep(rep(a, erode), dilate)
    if op == CLOSE:
        return rep(rep(a, dilate), erode)
    return _sub_sat(rep(a, dilate), rep(a, erode))
