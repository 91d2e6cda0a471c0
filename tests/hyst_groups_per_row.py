#!/usr/bin/env python3
"""How many 16-px groups of a map row does the hysteresis change?  CPU only, from the oracle.

k_hyst's write-back (cudacam_amd/csrc/hyst.hip) patches a provisional edge map: of a row whose strong bits changed, only the
16-pixel groups that changed are rewritten, through a queue in LDS.  That suits rows with a few such groups.  This tool counts,
for the benchmark's frames (bench.py's seeds, 1080p, thresholds 10 / 40), the groups per changed row between the oracle's map
before the hysteresis (strong = 255 of the threshold stage) and after its fixpoint, and prints a histogram per content.

The count is per RUN, not per launch: a row that changes in several launches of a run is patched once per launch, each time
with the groups that launch changed, so the figure here is an upper bound of what any single launch sees in that row.

  python tests/hyst_groups_per_row.py [--frames N] > profiles/<dir>/groups_per_row.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cudacam_amd import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

W, H, LOW, HIGH = 1920, 1080, 10, 40
BINS = (1, 2, 3, 4, 8, 16, 24, 32, 48, 64, 96, 121)   # lower edges; 1080p has 120 groups a row


def groups_per_changed_row(img):
    """Changed 16-px groups of every row the hysteresis changes, as an int array (one entry per changed row)."""
    st = O.canny_r(img, LOW, HIGH, stages=True)
    changed = (st["edges"] == 255) & (st["thresh"] != 255)
    pad = (-changed.shape[1]) % 16
    g = np.pad(changed, ((0, 0), (0, pad))).reshape(changed.shape[0], -1, 16).any(axis=2).sum(axis=1)
    return g[g > 0]


def batches(nat_per):
    """The distinct frames of the rotation's batches, as bench.py builds them for rank 0 (planes(kind, 0, bi))."""
    seed = synth.SEED0
    a = synth.frames("natural", W, H, nat_per, seed=seed)
    b = synth.frames("natural", W, H, nat_per, seed=seed + 500)
    pa, pb = a.astype(np.uint32), b.astype(np.uint32)
    pc = np.roll(pa, nat_per // 2, axis=0)[:, ::-1, :]
    yield "natural", a
    yield "natural-B", b
    yield "noise", synth.frames("noise", W, H, 8, seed=seed + 9000)
    yield "blend", ((7 * pa + 38 * pb + 19 * pc) >> 6).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10, help="distinct natural frames per batch (bench.py: 10 at its defaults)")
    a = ap.parse_args()
    O.build()
    print(f"# changed 16-px groups per changed row, oracle, {W}x{H}, thresholds {LOW}/{HIGH}, bench.py seeds (rank 0)")
    print("# per RUN: a row that changes in several launches is patched once per launch with fewer groups each time, so this")
    print("# overstates what a single launch of k_hyst sees in a row")
    for kind, frames in batches(a.frames):
        g = np.concatenate([groups_per_changed_row(f) for f in frames])
        n = len(g)
        print(f"\n## {kind}: {len(frames)} frames, {n} changed rows of {len(frames) * H} ({100.0 * n / (len(frames) * H):.1f} %), "
              f"groups per changed row: mean {g.mean():.1f}, median {int(np.median(g))}, max {int(g.max())}")
        for lo, hi in zip(BINS[:-1], BINS[1:]):
            k = int(((g >= lo) & (g < hi)).sum())
            print(f"{lo:4d} .. {hi - 1:3d}: {k:7d}  {100.0 * k / n:5.1f} %")
        for t in (16, 24, 32, 48, 64):
            print(f"rows with more than {t} groups: {100.0 * (g > t).sum() / n:5.1f} %   with at least {t}: {100.0 * (g >= t).sum() / n:5.1f} %")


if __name__ == "__main__":
    main()
