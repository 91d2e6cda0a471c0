"""numpy restatement of hc_edge_points_device (include/hipcanny.h): cv::countNonZero and cv::findNonZero of one-channel u8
maps, per frame.  A pixel belongs to the list iff its byte is non-zero; the list holds (x, y) int32 pairs in raster order
(np.argwhere is row-major: rows top to bottom, columns left to right inside a row) and is cut to `capacity` points."""
import numpy as np


def count(m):
    return int((np.asarray(m) != 0).sum())


def points(m, capacity=None):
    """(min(count, capacity), 2) int32 = (x, y) of the non-zero pixels of one (H, W) map, in raster order."""
    m = np.asarray(m)
    if m.ndim != 2:
        raise ValueError("one (H, W) map")
    p = np.argwhere(m != 0)[:, ::-1].astype(np.int32)
    return np.ascontiguousarray(p if capacity is None else p[:int(capacity)])


def edge_points(maps, capacity=None):
    """(uint32 counts [n], [points of frame f cut to capacity]) of (n, H, W) maps: what Context.edge_points returns.
    capacity=None: nothing is cut."""
    maps = np.asarray(maps)
    return np.array([count(m) for m in maps], np.uint32), [points(m, capacity) for m in maps]
