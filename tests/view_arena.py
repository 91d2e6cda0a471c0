"""Caller views for the view tests: frames placed at a pitch, a frame stride and a base offset inside a larger flat byte
buffer (the "arena") whose every other byte is a guard.  cv::Mat / GpuMat callers hand the library exactly such views --
rows padded to the allocator's pitch, frames with a gap between them, an ROI whose neighbours are the caller's own pixels
-- and the library's contract is that the bytes outside [row start, row start + row bytes) of every row can neither
change a result (input side) nor be changed (output side).

A plain helper module (no fixtures): tests/test_view_arena_cpu.py tests it, tests/test_gpu_views.py and
tests/fuzz_parity.py use it.

Layout, all in bytes: row r of frame f starts at  lead + base_off + f * frame_stride + r * pitch  and holds row_bytes
bytes; the arena has  lead + base_off + n * frame_stride + trail  bytes.  `lead` and `trail` are at least one pitch plus
64 bytes each, so whatever the kernels may read around a view (whole 8-pixel groups of the last row, never beyond its
pitch) lies inside the allocation: the tests never put a view against the end of an allocation.
"""
from dataclasses import dataclass

import numpy as np

from cudacam_amd import synth

FILLS = ("random", "ff", "parent")


def round_up(v, m):
    return (v + m - 1) // m * m


@dataclass(frozen=True)
class Geometry:
    n: int            # frames
    rows: int         # rows per frame
    row_bytes: int    # bytes of a row that belong to the view
    pitch: int
    frame_stride: int
    base_off: int
    lead: int
    trail: int

    @property
    def offset(self):
        """Offset of the view's first byte in the arena."""
        return self.lead + self.base_off

    @property
    def size(self):
        return self.lead + self.base_off + self.n * self.frame_stride + self.trail

    def row_starts(self):
        """(n, rows) arena offsets of the first byte of every row."""
        f = np.arange(self.n, dtype=np.int64)[:, None] * self.frame_stride
        r = np.arange(self.rows, dtype=np.int64)[None, :] * self.pitch
        return self.offset + f + r

    def index(self):
        """(n, rows, row_bytes) arena offsets of every byte of the view."""
        return self.row_starts()[:, :, None] + np.arange(self.row_bytes, dtype=np.int64)[None, None, :]

    def inside(self):
        """Boolean mask over the arena: True for the bytes of the view."""
        m = np.zeros(self.size, bool)
        m[self.index().reshape(-1)] = True
        return m

    def locate(self, off):
        """(frame, row, column relative to the view's first column, in bytes) of an arena offset.  Offsets before the view
        land in frame 0 with a negative row, offsets in a frame gap or behind the last frame in rows >= `rows`."""
        rel = int(off) - self.offset
        f = min(max(rel // self.frame_stride, 0), self.n - 1) if self.frame_stride else 0
        rel -= f * self.frame_stride
        r = rel // self.pitch
        return int(f), int(r), int(rel - r * self.pitch)


def geometry(n, rows, row_bytes, pitch, frame_stride=None, base_off=0, lead=None, trail=None):
    if frame_stride is None:
        frame_stride = pitch * rows
    need = pitch + 64
    lead = need if lead is None else lead
    trail = need if trail is None else trail
    if pitch < row_bytes:
        raise ValueError(f"pitch {pitch} smaller than a row of {row_bytes} bytes")
    if n > 1 and frame_stride < pitch * rows:
        raise ValueError(f"frame stride {frame_stride} smaller than a frame of {rows} rows at pitch {pitch}")
    if frame_stride < pitch * (rows - 1) + row_bytes:
        raise ValueError("frame stride smaller than the view of one frame")
    if lead < need or trail < need:
        raise ValueError(f"lead / trail must be at least pitch + 64 = {need} bytes")
    if base_off < 0:
        raise ValueError("negative base offset")
    return Geometry(int(n), int(rows), int(row_bytes), int(pitch), int(frame_stride), int(base_off), int(lead), int(trail))


def _frames_as_rows(frames):
    """(n, rows, row_bytes) uint8 view of (n, H, W) / (n, H, W, C) frames of any item size (int16 for the gradient entry)."""
    a = np.ascontiguousarray(frames)
    if a.ndim < 3:
        raise ValueError("frames must be (n, H, W) or (n, H, W, C)")
    n, h = a.shape[:2]
    return a.view(np.uint8).reshape(n, h, -1)


def _fill(size, fill, pitch, seed):
    if fill == "random":
        return np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
    if fill == "ff":
        return np.full(size, 255, np.uint8)
    if fill == "parent":   # the arena read at the view's pitch is one larger natural image: the view is an ROI of it
        rows = (size + pitch - 1) // pitch
        return synth.natural(pitch, rows, 1000 + seed).reshape(-1)[:size].copy()
    raise ValueError(f"fill must be one of {FILLS}")


def make_input(frames, pitch, frame_stride=None, base_off=0, fill="random", lead=None, trail=None, seed=0):
    """Places `frames` in a flat uint8 arena; every byte outside the view is `fill`.  Returns (arena, offset of the view's
    first byte); input_geometry() gives the Geometry of the same arguments."""
    rows = _frames_as_rows(frames)
    g = geometry(rows.shape[0], rows.shape[1], rows.shape[2], pitch, frame_stride, base_off, lead, trail)
    arena = _fill(g.size, fill, g.pitch, seed)
    arena[g.index()] = rows
    return arena, g.offset


def input_geometry(frames, pitch, frame_stride=None, base_off=0, lead=None, trail=None):
    rows = _frames_as_rows(frames)
    return geometry(rows.shape[0], rows.shape[1], rows.shape[2], pitch, frame_stride, base_off, lead, trail)


def read_view(arena, g):
    """The view's bytes as (n, rows, row_bytes)."""
    return np.asarray(arena).reshape(-1)[g.index()]


def make_output(n, rows, row_bytes, pitch, frame_stride=None, base_off=0, lead=None, trail=None, seed=0):
    """An output arena of the same kind of geometry, filled -- view included -- with a seeded pattern of values 1..254: a
    stray 0 or 255 (all an edge map holds) stands out wherever it lands.  Returns (arena, geometry)."""
    g = geometry(n, rows, row_bytes, pitch, frame_stride, base_off, lead, trail)
    arena = np.random.default_rng(0x5EED0000 + seed).integers(1, 255, g.size, dtype=np.uint8)
    return arena, g


def check_output(arena_after, arena_before, geometry, want, what="output view"):
    """Asserts that the view of `arena_after` equals `want` bit for bit and that EVERY byte outside the view's
    [row start, row start + row_bytes) ranges is what it was in `arena_before`."""
    g = geometry
    after = np.asarray(arena_after).reshape(-1)
    before = np.asarray(arena_before).reshape(-1)
    if after.dtype != np.uint8 or before.dtype != np.uint8:
        raise TypeError("arenas are uint8")
    if after.size != g.size or before.size != g.size:
        raise ValueError(f"arena sizes {after.size} / {before.size} do not match the geometry's {g.size}")
    want = np.ascontiguousarray(want)
    wrows = want.view(np.uint8).reshape(-1)
    if wrows.size != g.n * g.rows * g.row_bytes:
        raise ValueError(f"`want` has {wrows.size} bytes, the view {g.n * g.rows * g.row_bytes}")
    wrows = wrows.reshape(g.n, g.rows, g.row_bytes)
    errors = []
    got = after[g.index()]
    if not np.array_equal(got, wrows):
        bad = np.argwhere(got != wrows)
        first = [f"(frame {f}, row {r}, col {c}): got {int(got[f, r, c])}, want {int(wrows[f, r, c])}" for f, r, c in bad[:8]]
        errors.append(f"{len(bad)} of {got.size} bytes inside the view differ; first: " + "; ".join(first))
    changed = after != before
    changed[g.index().reshape(-1)] = False
    if changed.any():
        offs = np.flatnonzero(changed)
        first = []
        for o in offs[:8]:
            f, r, c = g.locate(o)
            first.append(f"offset {int(o)} (frame {f}, row {r}, col {c}): {int(before[o])} -> {int(after[o])}")
        errors.append(f"{len(offs)} bytes OUTSIDE the view were changed (rows are {g.row_bytes} bytes at pitch {g.pitch}); first: "
                      + "; ".join(first))
    if errors:
        raise AssertionError(f"{what}: " + " | ".join(errors))
