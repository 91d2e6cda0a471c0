"""What tests/test_gpu_front8_runs.py runs, without a GPU: the forms of the 8-px front kernels, their shapes and set run
lengths, the frames, the references and the non-vacuity rule.  tests/test_front8_runs_inputs_cpu.py asserts the rule for
every (form, shape, batch) with the oracle alone, so a seed that stops working fails there first.

Work split, as plan_front cuts it (tests/cpp/plan_driver.cpp pins the same numbers):
* k_front8 / k_front8o: a set length c gives runs of 6 * ceil((min(max(c, 2), H) + 4) / 6) - 4 rows (2, 8, 14, 20, ..);
* k_front_mx: ceil(H / c) runs of ceil(H / runs) rows; a run of 16 n - 4 rows costs n blocks (12 | 13, 28 | 29).
"""
import collections

import numpy as np

from cudacam_amd import synth

Form = collections.namedtuple("Form", "name kernel mode ch per_channel dense l2 front_form")
FORMS = [
    Form("front8-mono", "f8", "R", 1, False, False, False, 2),
    Form("front8-mono-dense", "f8", "R", 1, False, True, False, 2),
    Form("front8-bgr", "f8", "R", 3, False, False, False, 2),
    Form("front8-per-channel", "f8", "R", 3, True, False, False, 2),
    Form("half-mono", "half", "R", 1, False, False, False, 4),
    Form("half-mono-dense", "half", "R", 1, False, True, False, 4),
    Form("half-bgr", "half", "R", 3, False, False, False, 4),
    Form("half-per-channel", "half", "R", 3, True, False, False, 4),
    Form("front8o-L1", "f8o", "O", 1, False, False, False, 3),
    Form("front8o-L2", "f8o", "O", 1, False, False, True, 3),
    Form("front-mx", "mx", "R", 1, False, False, False, 5),
]
# per kernel: (strip width, width of the provisional map -- W % 8 == 0, two strips --, a second strip of one column)
# (488 columns are three half-strips: with three frames an odd number of units, one half-wave without one)
WIDTHS = {"f8": (496, 504, 497), "f8o": (496, 504, 497), "half": (240, 488, 241), "mx": (216, 224, 217)}
TINY_W, TINY_HEIGHTS = 5, (1, 2, 3, 7, 8)
# Mode R: the reference's defaults; Mode O: 30 / 90 on the L1 magnitude |dx| + |dy|, and the same pair with L2gradient
# (cv::Canny compares sqrt(dx^2 + dy^2), which is between 0.707 and 1 times the L1 magnitude, with the same numbers: the
# rule below holds for it at the same seeds or at the ones listed)
THRESHOLDS = {"R": (10, 40), "O": (30, 90)}

H_B = 41
LEG_A_HEIGHTS = tuple(range(1, 23))                   # (22: a last run of 8 rows behind one of 14)
LEG_A_LENGTHS = (2, 8, 14, 0)                          # 0: the automatic split
LEG_B_LENGTHS = (2, 8, 14, 20, 26, 32, 38, 41, 100)    # every distinct run length of 41 rows, the frame, beyond it
MX_ROWS, MX_LAG = 16, 4   # canny_params.h; tests/test_front8_runs_inputs_cpu.py reads the header and compares


def front8_cut(h, c):
    """(rows per run, runs, rows of the last run) of k_front8 / k_front8o for a set length c >= 1."""
    rows = min(max(c, 2), h)
    run = 6 * max(1, (rows + 4 + 5) // 6) - 4
    runs = (h + run - 1) // run
    return run, runs, h - run * (runs - 1)


def front_mx_run_rows(blocks):
    return MX_ROWS * blocks - MX_LAG


def mx_cut(h, c):
    """(rows per run, runs, rows of the last run) of k_front_mx for a set length c >= 1."""
    nch = max(1, (h + c - 1) // c)
    run = (h + nch - 1) // nch
    runs = (h + run - 1) // run
    return run, runs, h - run * (runs - 1)


def _mx_leg_a():
    """{height: set lengths}.  The heights of LEG_A_HEIGHTS with lengths 2, 8, 14 and 0; a last run of L = 1 .. 16 rows behind one of
    L + 1 (height 2 L + 1, length L + 1); and around every block border R = 16 n - 4: runs of R and R + 1 rows with last
    runs of R - 1, R and R + 1."""
    plan = {h: [2, 8, 14, 0] for h in LEG_A_HEIGHTS}
    for last in range(1, 17):
        plan.setdefault(2 * last + 1, [0]).append(last + 1)
    for blocks in (1, 2):
        r = front_mx_run_rows(blocks)
        for h, c in ((2 * r, r), (2 * r + 1, r + 1), (2 * r + 2, r + 1), (3 * r, r), (3 * r + 3, r + 1)):
            plan.setdefault(h, [0]).append(c)
    return {h: sorted(set(v), key=lambda c: (c == 0, c)) for h, v in sorted(plan.items())}


MX_LEG_A = _mx_leg_a()
# H_B rows: a set length for every distinct run length ceil(41 / k), then beyond the frame
MX_LEG_B_LENGTHS = tuple(sorted({(H_B + k - 1) // k for k in range(1, H_B + 1)})) + (100,)


def leg_a(form):
    """[(width, height, set lengths)]: every height at the provisional-map width, then the tiny width."""
    w = WIDTHS[form.kernel][1]
    if form.kernel == "mx":
        plan = [(w, h, tuple(c)) for h, c in MX_LEG_A.items()]
    else:
        plan = [(w, h, LEG_A_LENGTHS) for h in LEG_A_HEIGHTS]
    return plan + [(TINY_W, h, LEG_A_LENGTHS) for h in TINY_HEIGHTS]


def leg_b(form):
    """[(width, height, set lengths)]: one height, the three widths of the form."""
    lengths = MX_LEG_B_LENGTHS if form.kernel == "mx" else LEG_B_LENGTHS
    return [(w, H_B, lengths) for w in WIDTHS[form.kernel]]


def shapes(form):
    return sorted({(w, h) for w, h, _ in leg_a(form) + leg_b(form)})


# ---- frames ----------------------------------------------------------------------------------------------------------
def content_key(form):
    """Forms with the same key get the same frames and the same reference."""
    return "O-L2" if form.l2 else "O-L1" if form.mode == "O" else "R-pc" if form.per_channel else "R-bgr" if form.ch == 3 else "R-mono"


# Seeds with which, in the reference, every row of every map of both batches holds a candidate and an empty pixel
# (width 5: see PER_FRAME_RULE); found by a search on the CPU from 1 upwards, asserted by
# tests/test_front8_runs_inputs_cpu.py.  {content key: {(width, height): seed}}; every shape not listed: seed 1.
SEEDS = {
    "R-mono": {(5, 2): 4, (504, 17): 2, (504, 20): 2, (241, 41): 2, (488, 4): 2, (488, 20): 5, (224, 14): 2, (224, 16): 2, (224, 18): 2,
               (224, 19): 2, (224, 24): 3, (224, 27): 2, (224, 31): 2, (224, 39): 6, (224, 57): 2, (224, 87): 2},
    "R-bgr": {(5, 2): 4, (504, 16): 2},
    "R-pc": {(5, 2): 4, (504, 17): 2, (504, 20): 2, (241, 41): 2, (488, 4): 2, (488, 20): 5},
    "O-L1": {(5, 1): 2, (5, 2): 2},
    "O-L2": {(5, 1): 2, (5, 2): 2},
}
# (content key, width, height) of the tiny width where no seed below 400 gives the per-row rule: there every map must hold
# a candidate and an empty pixel somewhere
PER_FRAME_RULE = {(k, 5, h) for k in ("R-mono", "R-bgr", "R-pc") for h in (3, 7, 8)} | {(k, 5, h) for k in ("O-L1", "O-L2") for h in (2, 7, 8)}


def seed_for(form, w, h):
    return SEEDS.get(content_key(form), {}).get((w, h), 1)


def stripes(w, h, phase=0):
    """(The same frames as _stripes of tests/test_gpu_mode_o_chunks.py, which stays as it is: keep the two equal.)
    Diagonal bands six pixels wide, "/" on the left half and "\\" on the right: both diagonal NMS branches in every row."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.where(xx < (w + 1) // 2, xx + yy, xx - yy + 6 * h) + phase
    return (((d // 6) & 1) * 200 + 20).astype(np.uint8)


def _mono_batches(w, h, seed):
    """Two batches of three different frames: (natural, noise, stripes) and (stripes, natural, noise) of other seeds -- a
    frame taken for another shows in either."""
    return [[synth.natural(w, h, seed), synth.noise(w, h, seed + 1), stripes(w, h, seed)],
            [stripes(w, h, seed + 3), synth.natural(w, h, seed + 4), synth.noise(w, h, seed + 5)]]


def batches(ch, w, h, seed):
    """[(3, h, w) or (3, h, w, 3) uint8] x 2; three-channel frames have three different planes."""
    out = []
    for m in _mono_batches(w, h, seed):
        if ch == 3:
            m = [np.stack([m[k], m[(k + 1) % 3], m[(k + 2) % 3][::-1]], -1) for k in range(3)]
        out.append(np.ascontiguousarray(np.stack(m)))
    return out


# ---- references ------------------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "frames low high pre edges blur")   # pre / edges / blur: one map per OUTPUT frame (blur: None in Mode O)


def _reference(oracle, key, frames):
    low, high = THRESHOLDS["O" if key.startswith("O") else "R"]
    pre, edges, blur = [], [], []
    for f in frames:
        if key.startswith("O"):
            e, p = oracle.canny_o_stages(f, low, high, key == "O-L2")
            pre.append(p); edges.append(e)
            continue
        planes = [f] if key == "R-mono" else [oracle.gray_bgr(f)] if key == "R-bgr" else [np.ascontiguousarray(f[:, :, c]) for c in range(3)]
        for pl in planes:
            st = oracle.canny_r(pl, low, high, stages=True)
            pre.append(st["thresh"]); edges.append(st["edges"]); blur.append(st["blur"])
    return Ref(frames, low, high, np.stack(pre), np.stack(edges), np.stack(blur) if blur else None)


_cache = {}


def references(oracle, form, w, h):
    """The two batches of a shape with what the oracle makes of them; computed once per (content key, shape)."""
    key = (content_key(form), w, h)
    if key not in _cache:
        _cache[key] = [_reference(oracle, key[0], f) for f in batches(form.ch, w, h, seed_for(form, w, h))]
        for r in _cache[key]:
            for a in r:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return _cache[key]


# ---- non-vacuity -----------------------------------------------------------------------------------------------------
def per_frame_rule(form, w, h):
    return (content_key(form), w, h) in PER_FRAME_RULE


def vacuous(pre, per_frame=False):
    """Why the tri-state maps `pre` (n, h, w) leave a seam nothing to get wrong: '' if every row of every map (per_frame:
    every map) holds a non-zero and a zero pixel."""
    axes = (1, 2) if per_frame else 2
    busy, empty = (pre != 0).any(axis=axes), (pre == 0).any(axis=axes)
    if busy.all() and empty.all():
        return ""
    return f"(map{'' if per_frame else ', row'}) without a candidate {np.argwhere(~busy).tolist()[:6]}, without an empty pixel {np.argwhere(~empty).tolist()[:6]}"


def assert_not_vacuous(oracle, form, w, h):
    if w != TINY_W:
        assert not per_frame_rule(form, w, h), "only the tiny width may fall back to the per-map rule"
    for k, r in enumerate(references(oracle, form, w, h)):
        why = vacuous(r.pre, per_frame_rule(form, w, h))
        assert not why, f"{form.name} {w}x{h} batch {k}, seed {seed_for(form, w, h)}: {why}"
