#!/usr/bin/env python3
"""Seeded CHAINS of device ops and runs on one context: the entries that are not runs (blur, derivatives, automatic thresholds,
edge points, Hough lines, Hough segments, Hough circles, connected components, morphology, distance transform) queued between and behind runs, with no synchronisation but the few the sequence
itself names.  tests/fuzz_sequences.py does this for the runs alone; each entry has a GPU test file of its own for its shapes,
capacities, views and refusals.  What neither reaches is the state the entries share on one context (cudacam_amd/csrc/
device_ops.hip: the scratch buffers that grow and never shrink, the Hough and walk tables cached by geometry) and the one place
where they meet the runs (finish_writers_of: which pipelined runs in flight a reader of edge maps completes first -- and a writer
of a view the caller chooses: blur, the label plane, the morphed frames, the distance and the nearest plane).

Three parts, the first two pure (numpy, the CPU oracle, the numpy restatements; no GPU, no clock):
  make_sequence(seed)   context parameters, 12 .. 20 steps (plain dicts; the synchronisation a stream switch needs, the step that
                        takes a threshold table off again and the final sync are among them), 1 .. 3 circles steps drawn from a
                        generator of their own and inserted among them (add_circles), 1 .. 3 components steps from a third
                        generator inserted among those (add_components), 1 .. 3 morph steps from a fourth (add_morphology) and
                        1 .. 3 dist steps from a fifth (add_distance), and counters that say what the sequence exercises
  Model                 the expected content of EVERY byte of every device buffer the sequence owns, step after step: inputs in
                        arenas of 255s, edge maps with the padding of their pitch, counts between guard words, lists in slots
                        pre-filled with a canary.  A step reads its inputs from the model and writes its outputs back, so values
                        propagate (a run's maps -> points -> lines -> segments; points and gradient planes -> circles; maps ->
                        labels, which a later reader of the same bytes takes for a map; maps -> morphed maps in another output ->
                        whoever reads that output next; maps -> a distance plane over an output, read as a map likewise) and
                        nothing is read from the device in between.
  Executor              queues the same steps through api.Context and, at every "sync" step and at the end, compares every buffer
                        with the model byte for byte -- results, canaries, guards and padding alike.
The per-entry helpers of the GPU test files (_upload / _check) upload a map per call and check one call's buffers; here a buffer
lives through the sequence and is compared whole, so the named cases of tests/test_gpu_device_op_sequences.py use those helpers'
restatements through the model as well and nothing of them is forked.

Pipelined contexts queue ONE hysteresis launch per run (hc_set_tuning) on 32-row tiles (HC_OPT_TEST_HYST_GEOM 1602), and their
first frames hold a weak chain that crosses the tiles (fuzz_sequences.vchain / wobble): the maps a run's queued launches leave
differ from the final ones until the host-side continuation (finish_slot) has rewritten them -- measured on the MI355X for every
size, mode and channel count used here.  A reader that was not ordered behind its writer then reads a different map every time,
not once in a while.  The executor asserts from the context's own report that runs were continued.

Usage: tests/device_op_sequences.py --seed N      prints the steps of one seed; with a GPU, also runs and checks them
       tests/device_op_sequences.py --scan A B    the counters of seeds A .. B - 1 (no GPU): how the committed seeds were chosen
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import auto_thr_ref as AT          # noqa: E402
import ccl_ref as CC               # noqa: E402
import canny_o_ext_ref as X        # noqa: E402
import deriv_ref as D              # noqa: E402
import dist_ref as DR              # noqa: E402
import edge_points_ref as EP       # noqa: E402
import fuzz_sequences as FS        # noqa: E402
import gauss_blur_ref as G         # noqa: E402
import hough_circles_ref as HC     # noqa: E402
import hough_ref as R              # noqa: E402
import hough_segments_ref as S     # noqa: E402
import morph_ref as MR             # noqa: E402
import view_arena as VA            # noqa: E402
from cudacam_amd import api  # noqa: E402

PI = math.pi
SIZES = ((61, 33), (65, 64), (130, 67), (250, 66))   # walks and rows cross a wave, a trip of four chunks, a row chunk (test_gpu_hough*.py)
MAX_BATCH = 4
POOL = 6          # frames of the input pool
NOUT = 3          # rotating output buffers
# Hough geometries (rho, theta, min_theta, max_theta).  A, A_RHO and A_MIN have twelve angles each and three different sets of
# tables: a cache that compared numangle alone would serve the wrong ones.  BIG has 180: tables and scratch grow in mid-sequence.
GEO_A, GEO_A_RHO, GEO_A_MIN, GEO_BIG = (1.0, PI / 12, 0.0, 3.0), (2.0, PI / 12, 0.0, 3.0), (1.0, PI / 12, 0.1, 3.1), (1.0, PI / 180, 0.0, PI)
GEOS = (GEO_A, GEO_A_RHO, GEO_A_MIN, GEO_BIG)
SAME_NUMANGLE = {0: (1, 2), 1: (0, 2), 2: (0, 1), 3: ()}   # index -> the others with equal numangle
CANARY_BYTE = 0xA5   # lists, counts: int32 -0x5A5A5A5B, the canary of the per-entry tests
GUARD = 64           # int32 words around counts and lists
NLIST = 12           # count words of a list slot (3 maps per frame of a per-channel context)
LCAP_MAX, SCAP_MAX, CCAP_MAX = 400, 2000, 1024
CANNY_THR = {3: (50.0, 150.0), 5: (400.0, 1200.0), 7: (3000.0, 9000.0), -1: (160.0, 500.0)}
KINDS = ("run", "canny", "deriv", "rungrad", "blur", "autothr", "thr_on", "thr_off", "points", "lines", "segs", "sync", "stream")
# ... and the one kind that make_steps does not draw: add_circles inserts it, from a generator of its own, so that a seed keeps the
# steps it had before there were circles
CIRCLES_DP, CIRCLES_MIN_DIST, CIRCLES_THRESHOLD, CIRCLES_CC = (1.0, 1.5, 2.0), (0.0, 3.0, 8.0), (2, 4, 8), (16, 300, 4096)
# ... nor the other: add_components inserts `components` steps behind the circles, from a third generator, for the same reason.
# Capacities: 0 with null rows, 0 with row pointers, the background row alone, a few rows (which cuts most frames), every row.
# Label planes of their own (lab0 / lab1) begin 4 * loff bytes into the arena, with lpad bytes behind each row and lgap between frames
COMP_CAPS, COMP_CUTS = ("null", "zero", "one", "cut", "all"), (2, 3, 9)
LAB_LEAD, LAB_OFFS, LAB_PADS, LAB_GAPS = 512, (0, 1, 2, 3), (0, 4, 20), (0, 8, 132)
# ... nor the two newest.  add_morphology inserts `morph` steps behind the components, from a fourth generator: an output arena of
# their own (mor0 / mor1) begins moff bytes into it, with mpad bytes behind each row and mgap between frames -- any alignment, so
# pads and gaps that are no multiples of 4.  The elements: the three shapes at 3 / 5 / 7, and three that are asymmetric in y with an
# empty row.  add_distance inserts `dist` steps behind those, from a fifth: planes of their own (dtp0 / dtp1) are laid out as label
# planes are (LAB_*); side by side, the two ROIs of one plane lie 4 W + 4 * swords bytes apart
MOR_LEAD, MOR_OFFS, MOR_PADS, MOR_GAPS = 512, (0, 1, 2, 3), (0, 1, 7), (0, 3, 129)
MORPH_ASYM = ((1, 0, -1), (2, 1, 0, -1, 1), (-1, 0, 3, 1, 2, 0, 3))
MORPH_DSTS, DIST_NEARS, DT_SIDE_WORDS = ("own", "maps", "sout", "blur"), ("none", "own", "side"), (0, 1, 3)
VIEW_KINDS = ("whole", "frame", "roi", "before", "behind", "sout")
COUNTERS = tuple(f"overlap_{k}" for k in ("whole", "frame", "roi", "sout", "before", "behind", "blur_in", "blur_out")) + (
    "adjacent", "hough_tables_equal_numangle", "seg_tables_equal_numangle", "scratch_growths", "n_above_max_batch", "hough_passes_above_one",
    "line_lists_nonempty", "seg_lists_nonempty", "lists_cut", "staged_runs", "blur_into_pending_copy_dst", "mismatched_geometry", "runs_with_frame_table",
    # circles steps: frames with a count above 0 / above a circle capacity that is not 0; calls of more than one pass; calls that
    # need more scratch than every circles call before them; frames whose stored point count exceeds the point capacity / with
    # more ranked centres than the centre capacity; centres the smallest distance dropped; calls with no deriv step before them /
    # with more frames than the last deriv step wrote; calls with a lines call before and behind them and no sync among the three
    "circle_lists_nonempty", "circle_lists_cut", "circle_passes_above_one", "circle_scratch_growths", "circles_from_cut_points", "circles_centres_cut",
    "circles_dropped_by_min_dist", "circles_on_unwritten_planes", "circles_on_stale_frames", "circles_between_lines",
    # components steps: calls whose map view / whose label plane overlapped the output of a run in flight; frames with more
    # components than a capacity that is not 0; calls with capacity 0; calls of more frames than max_batch; calls whose map view
    # overlaps bytes that an earlier step wrote as labels over an output and no write has covered since; calls that need a
    # larger table than every components call before them; calls of more than one pass
    "components_overlap_map", "components_labels_over_pending", "components_rows_cut", "components_capacity_0", "components_n_above_max_batch",
    "components_of_label_bytes", "ccl_scratch_growths", "ccl_passes_above_one",
    # morph steps: calls whose input / whose output overlapped the output of a run in flight; calls of 3-channel frames; of more
    # frames than max_batch; whose input overlaps label bytes (as components_of_label_bytes); OPEN / CLOSE calls that need more
    # scratch than every one before them / of more than one pass; calls whose output differs from their input; steps that read
    # bytes a morph step wrote into `maps` or `sout` and no write has covered since
    "morph_overlap_in", "morph_out_over_pending", "morph_three_channel", "morph_n_above_max_batch", "morph_of_label_bytes", "morph_scratch_growths",
    "morph_passes_above_one", "morph_output_differs", "morph_read_by_a_later_step",
    # dist steps: calls whose map view / whose distance plane overlapped the output of a run in flight; calls with the two planes
    # side by side; FRAMES without a feature pixel; calls whose map overlaps bytes a morph step wrote; calls of more frames than
    # max_batch; calls with a frame that has a feature pixel and another; steps that read, as a map, bytes a dist step wrote as a
    # distance plane over an output and no write has covered since
    "dist_overlap_map", "dist_plane_over_pending", "dist_side_by_side", "dist_without_features", "dist_of_morph_output", "dist_n_above_max_batch",
    "dist_maps_mixed", "dist_plane_read_as_map")
# ... of which the committed seeds together must reach every one but these four.  A view beside one output that lies inside its
# neighbour is a "whole" or "frame" overlap of that neighbour under another name.  The table of a components call has a word per
# chunk of 8 rows: at most 36 bytes per frame here, while a seeded context's bound, if it has one, is two frames of the largest
# Hough geometry -- so no seeded call can take a second pass: test_components_in_passes_under_a_bound (tests/
# test_gpu_device_op_sequences.py) covers that as a named case.  A table grows where a call of more frames follows one of fewer,
# which five of the committed seeds happen to do; test_the_component_table_grows_while_a_call_is_queued is the case that must.
# The same holds for the intermediate frames of OPEN / CLOSE: one is W x H bytes (3 W x H of 3-channel frames, rows rounded up to 4:
# at most 49,632 bytes here), the seeded bound several hundred KiB, so the twelve frames a seeded call can have fit into one pass:
# test_morphology_in_passes_under_a_bound covers passes, test_the_morphology_scratch_grows_while_a_call_is_queued the growth that
# seeds reach only where a call of more frames happens to follow one of fewer
NOT_REQUIRED = ("overlap_before", "overlap_behind", "ccl_scratch_growths", "ccl_passes_above_one", "morph_scratch_growths", "morph_passes_above_one")
REQUIRED = tuple(c for c in COUNTERS if c not in NOT_REQUIRED)
# Output views that force the staged path (copy_dst), from the families of tests/test_gpu_views.py.  Of those only the odd one
# stages an output (P4, GM and ROI are multiples of 4 throughout); the other two here are its P4 and ROI with the one thing made
# odd that hc_run_device names beside the pitch: the base pointer alone, the frame stride alone.
STAGED_FAMILIES = ("ODDO", "P4_BASE", "ROI_FS")
# The committed seeds (tests/test_gpu_device_op_sequences.py runs them, tests/test_device_op_sequences_cpu.py checks the conditions):
# chosen from --scan 0 300 so that together they reach every counter of REQUIRED, every pipelined one has a reader on a view that
# overlaps a pending writer, every one a segment list that is not empty, and the sizes, modes, channel counts and staged
# families all occur.  The circles steps came later, from a generator of their own (add_circles), and left those 28 every step they
# had; of the circle counters of REQUIRED the 28 reach all but two, for which --scan 0 300 gave 58 (circles_on_stale_frames) and
# 108 (circle_passes_above_one, which takes 61 x 33 frames, a scratch bound and four frames at centre capacity 4096: one seed of the 300).
# The components steps came last, from a third generator (add_components), and left those 30 every step they had, circles
# included.  The 30 reach every components counter of REQUIRED (--scan: labels over a pending output in 3, 15 and 207, label bytes
# read as a map in 15, 22 and 207, more than max_batch frames in 25, the others in a dozen each), so no seed was added for a
# counter.  One was added for a view: in none of the 30 does a components step read the buffer a staged run copies to, the one map
# view at an odd pitch; --scan 0 300 gave 229 (components of `sout` at every row's capacity, the labels over a pending output).
# The morph and dist steps came after that, from a fourth and a fifth generator (add_morphology, add_distance), and left those 31
# every step they had.  Every one of the 31 keeps what the CPU test demands of each sequence (segment, line and circle lists that
# are not empty, a reader over a pending writer) and has a morph step that changes its input and a dist step on a map with feature
# and other pixels, so none was replaced.  Together they reach every new counter of REQUIRED but one (--scan: a morph input over a
# pending output in 6, a distance plane over one in 40 and 141, frames without a feature pixel in 69, 85 and 100, more than
# max_batch frames in 0 and 25, morphed bytes read again in 10, a distance plane read as a map in 10): in none does a morph step
# WRITE over the output of a run in flight, which takes a run directly in front of the step and a free region that is that
# run's.  21 of --scan 0 300 do; 38 is the one among them with the smallest frames (61 x 33, three channels, mode O), and it also
# lays a distance plane over a pending output
SEEDS = (0, 1, 3, 5, 6, 7, 8, 9, 11, 13, 14, 15, 17, 21, 22, 25, 31, 35, 40, 49, 66, 69, 85, 86, 100, 141, 145, 207, 58, 108, 229, 38)


def rup(v, m):
    return (v + m - 1) // m * m


class Mismatch(AssertionError):
    pass


def layout(P):
    """Sizes and offsets (bytes) of every buffer of a sequence with parameters P."""
    w, h, ch = P["w"], P["h"], P["ch"]
    L = dict(w=w, h=h, ch=ch, mb=P.get("max_batch", MAX_BATCH))   # (max_batch: the named cases may ask for another)
    L["nmax"] = L["mb"] * (3 if P["per_channel_ever"] else 1)
    L["pf"] = max(MAX_BATCH, L["nmax"])   # frames of a gradient plane: a circles step of a per-channel context reads up to nmax
    L["ip"] = rup(w, 8) * ch; L["ifs"] = L["ip"] * h; L["ilead"] = rup(L["ip"] + 64, 512)          # frames / blur: whole 8-pixel groups, in place
    L["op"] = rup(w, 4); L["ofs"] = L["op"] * h; L["oreg"] = L["nmax"] * L["ofs"]; L["olead"] = rup(2 * L["ofs"] + 512, 512)
    sp, sfs, sbase = staged_view(P.get("staged", "ODDO"), w, h)
    L["sp"], L["sfs"], L["soff"] = sp, sfs, rup(sp + 64, 512) + sbase
    L["dp"] = rup(2 * ch * w, 8); L["dfs"] = L["dp"] * h
    L["sizes"] = dict(frames=2 * L["ilead"] + POOL * L["ifs"], blur=2 * L["ilead"] + POOL * L["ifs"], maps=2 * L["olead"] + NOUT * L["oreg"],
                      sout=L["soff"] + L["nmax"] * sfs + rup(sp + 64, 512), dxdy=1024 + 2 * L["pf"] * L["dfs"], thr=4 * (2 * GUARD + 2 * MAX_BATCH))
    words = 3 * GUARD + NLIST
    for k in range(2):
        L["sizes"][f"pts{k}"] = 4 * (words + 2 * NLIST * w * h)
        L["sizes"][f"lines{k}"] = 4 * (words + 3 * NLIST * LCAP_MAX)
        L["sizes"][f"segs{k}"] = 4 * (words + 4 * NLIST * SCAP_MAX)
        L["sizes"][f"circ{k}"] = 4 * (words + 4 * NLIST * CCAP_MAX)
    # components: label planes of their own (nmax frames at the largest pad and gap, behind the largest offset), and per output slot
    # the counts between guard words, nmax x (W * H + 1) statistics rows, a guard, as many centroid rows at an 8-byte offset, a guard
    L["cmax"] = w * h + 1
    L["stats_off"] = 4 * (2 * GUARD + NLIST)
    L["cent_off"] = rup(L["stats_off"] + 20 * L["nmax"] * L["cmax"] + 4 * GUARD, 8)
    for k in range(2):
        L["sizes"][f"lab{k}"] = 2 * LAB_LEAD + 4 * LAB_OFFS[-1] + L["nmax"] * ((4 * w + LAB_PADS[-1]) * h + LAB_GAPS[-1])
        L["sizes"][f"comp{k}"] = L["cent_off"] + 16 * L["nmax"] * L["cmax"] + 4 * GUARD
    # morphology: output arenas for nmax one-channel frames or max_batch frames of the context's channels, at the largest pad and
    # gap behind the largest offset.  Distances: planes for nmax frames of two ROIs side by side, at the largest of everything
    for k in range(2):
        L["sizes"][f"mor{k}"] = 2 * MOR_LEAD + MOR_OFFS[-1] + max(L["nmax"] * ((w + MOR_PADS[-1]) * h + MOR_GAPS[-1]), L["mb"] * ((ch * w + MOR_PADS[-1]) * h + MOR_GAPS[-1]))
        L["sizes"][f"dtp{k}"] = 2 * LAB_LEAD + 4 * LAB_OFFS[-1] + L["nmax"] * ((8 * w + 4 * DT_SIDE_WORDS[-1] + LAB_PADS[-1]) * h + LAB_GAPS[-1])
    L["counts_off"] = 4 * GUARD
    L["list_off"] = 4 * (2 * GUARD + NLIST)
    return L


def staged_view(family, w, h):
    """(pitch, frame stride, base offset) of the output view of a staged run."""
    from test_gpu_views import _out_family
    if family == "ODDO":
        return _out_family("ODDO", w, h)
    if family == "P4_BASE":
        p, fs, base = _out_family("P4", w, h)
        return p, fs, base + 1
    if family == "ROI_FS":
        p, fs, base = _out_family("ROI", w, h)
        return p, fs + 2, base
    raise ValueError(family)


def out_start(L, k):
    return L["olead"] + k * L["oreg"]


def resolve_view(L, v):
    """A reader's view of maps: (buffer, offset, pitch, frame stride, frames the view may hold)."""
    kind = v[0]
    w, h, op, ofs = L["w"], L["h"], L["op"], L["ofs"]
    if kind == "whole":
        return "maps", out_start(L, v[1]), op, ofs, L["nmax"]
    if kind == "frame":                 # frames from frame f on: the last frame of a run's output
        return "maps", out_start(L, v[1]) + v[2] * ofs, op, ofs, L["nmax"] - v[2]
    if kind == "roi":                   # begins inside frame f: r0 rows down, c0 bytes in, every pm-th row of the parent
        _, k, f, r0, c0, pm = v
        return "maps", out_start(L, k) + f * ofs + r0 * op + c0, pm * op, pm * ofs, 1
    if kind == "before":                # ends exactly where output k begins
        return "maps", out_start(L, v[1]) - ((h - 1) * op + w), op, ofs, 1
    if kind == "behind":                # begins exactly where the nw maps of a run into output k end
        return "maps", out_start(L, v[1]) + v[2] * ofs, op, ofs, 1
    if kind == "sout":
        return "sout", L["soff"], L["sp"], L["sfs"], L["nmax"]
    raise ValueError(v)


def label_view(L, st):
    """(buffer, offset, pitch, frame stride) of the label plane of a components step: in an arena of its own, or -- one frame --
    laid over output region lslot of `maps`, four bytes for each byte of the region's first frames."""
    if st["dest"] == "over":
        return "maps", out_start(L, st["lslot"]), 4 * L["op"], 4 * L["ofs"]
    pitch = 4 * L["w"] + st["lpad"]
    return f"lab{st['lslot']}", LAB_LEAD + 4 * st["loff"], pitch, pitch * L["h"] + st["lgap"]


def morph_views(L, st):
    """((buffer, offset, pitch, frame stride) of the input, the same of the output) of a morph step.  The input: a view of maps, or
    3-channel frames of the pool from f0 on.  The output: an arena of its own, frames g0 .. of output region mslot of `maps`, of
    `sout`, or -- 3-channel frames -- of the `blur` buffer."""
    w, h = L["w"], L["h"]
    a = ("frames", L["ilead"] + st["f0"] * L["ifs"], L["ip"], L["ifs"]) if st["src"] == "frames" else resolve_view(L, st["view"])[:4]
    if st["dst"] == "own":
        pitch = st["channels"] * w + st["mpad"]
        return a, (f"mor{st['mslot']}", MOR_LEAD + st["moff"], pitch, pitch * h + st["mgap"])
    if st["dst"] == "blur":
        return a, ("blur", L["ilead"] + st["g0"] * L["ifs"], L["ip"], L["ifs"])
    if st["dst"] == "sout":
        return a, ("sout", L["soff"] + st["g0"] * L["sfs"], L["sp"], L["sfs"])
    return a, ("maps", out_start(L, st["mslot"]) + st["g0"] * L["ofs"], L["op"], L["ofs"])


def dist_views(L, st):
    """((buffer, offset, pitch, frame stride) of the distance plane, the same of the nearest plane or None) of a dist step.  The
    distance plane: in an arena of its own or -- one frame -- over output region dslot of `maps`, as label_view lays labels.  The
    nearest plane: none, a view of an arena of its own, or the other ROI of the plane the distances lie in, side by side: equal
    pitch and frame stride, 4 W + 4 * swords bytes to the right of the distances (nleft: to their left)."""
    w, h = L["w"], L["h"]
    if st["dest"] == "over":
        d = ("maps", out_start(L, st["dslot"]), 4 * L["op"], 4 * L["ofs"])
    else:
        apart = 4 * w + 4 * st["swords"] if st["near"] == "side" else 0
        pitch, base = 4 * w + apart + st["dpad"], LAB_LEAD + 4 * st["doff"]
        d = (f"dtp{st['dslot']}", base + (apart if st["nleft"] else 0), pitch, pitch * h + st["dgap"])
        if st["near"] == "side":
            return d, (d[0], base + (0 if st["nleft"] else apart), d[2], d[3])
    if st["near"] == "none":
        return d, None
    pitch = 4 * w + st["npad"]
    return d, (f"dtp{st['nslot']}", LAB_LEAD + 4 * st["noff"], pitch, pitch * h + st["ngap"])


def list_fits(kind, n, cap, width, L):
    """n slots of `cap` entries of `width` words lie inside a list buffer, behind its counts and before its last guard."""
    return n <= NLIST and L["list_off"] + 4 * width * cap * n <= L["sizes"][kind + "0"] - 4 * GUARD


def view_span(L, off, pitch, fs, n, row_bytes):
    return off, off + (n - 1) * fs + (L["h"] - 1) * pitch + row_bytes


def hough_need(w, h, geo, n, bound):
    """(scratch bytes, passes) of hc_hough_lines_device as include/hipcanny.h and host_plan.h state them."""
    na, nr = R.geometry(w, h, *geo)
    per = na * ((nr + 1) // 2) * 8 + (na + 2) * (nr + 2) * 4 + na * 4
    fpp = min(n, (bound or (256 << 20)) // per)
    return fpp * per, (n + fpp - 1) // fpp, per


def circle_need(w, h, dp, cc, n, bound):
    """(scratch bytes, passes, bytes per frame) of hc_hough_circles_device as include/hipcanny.h and plan_hough_circles (host_plan.h)
    state them: the ranked and the kept centres, the peak list, the accumulator, a count per row and per centre, two counts.
    (0, 0, bytes per frame) where one frame exceeds the bound: the entry refuses that call."""
    aw, ah, _ = HC.geometry(w, h, dp, 0.0, 1, 1)
    per = 2 * 16 * cc + 8 * ah * ((aw + 1) // 2) + 4 * (ah + 2) * (aw + 2) + 4 * ah + 4 * cc + 8
    fpp = min(n, (bound or (256 << 20)) // per)
    return (fpp * per, (n + fpp - 1) // fpp, per) if fpp else (0, 0, per)


def ccl_need(h, n, bound):
    """(scratch bytes, passes, bytes per frame) of hc_connected_components_device as include/hipcanny.h and plan_connected_components
    (host_plan.h) state them: a word per chunk of rows and frame of a pass, the rows of a chunk by hist_chunk_rows (canny_params.h)
    from the rows of the whole call -- 8, or all of a lower frame, until H x nframes passes 65,536; then a 8192nd of them, 64 at
    most.  (0, 0, bytes per frame) where one frame exceeds the bound: the entry refuses that call."""
    rows = min(max((h * n + 8191) // 8192, 8), 64, h)
    per = 4 * ((h + rows - 1) // rows)
    fpp = min(n, (bound or (256 << 20)) // per, 65535)
    return (fpp * per, (n + fpp - 1) // fpp, per) if fpp else (0, 0, per)


def morph_need(w, h, channels, op, n, bound):
    """(scratch bytes, passes, bytes per frame) of hc_morphology_device as include/hipcanny.h and plan_morphology (host_plan.h)
    state them: OPEN and CLOSE keep the intermediate frames of a pass as tight frames whose rows of channels * W bytes are rounded
    up to a multiple of 4; the other operations need none and take one pass under any bound.  (0, 0, bytes per frame) where one
    frame exceeds the bound: the entry refuses that call."""
    if op not in (MR.OPEN, MR.CLOSE):
        return 0, 1, 0
    per = rup(channels * w, 4) * h
    fpp = min(n, (bound or (256 << 20)) // per)
    return (fpp * per, (n + fpp - 1) // fpp, per) if fpp else (0, 0, per)


def describe(st):
    return st["kind"] + "(" + ", ".join(f"{k}={v}" for k, v in st.items() if k != "kind") + ")"


# ---- content ----------------------------------------------------------------------------------------------------------------
def chain_frame(w, h, mode, ch, pc, which):
    """A frame whose weak chain crosses the 32-row tiles, so that one queued launch leaves another map than the fixpoint: `which`
    0 is the content that did so on the MI355X for this size, mode and channel count, 1 the other of the two."""
    wob, vch = FS.make_frame("wobble", w, h), FS.vchain(w, h)
    first_wob = h < 40 and mode == "R" and (ch == 1 or pc)
    return (wob if first_wob else vch) if which == 0 else (vch if first_wob else wob)


def make_pool(rng):
    kinds = ["chain0", "chain1"] + [str(k) for k in rng.choice(["natural", "sparse", "wobble", "vchain", "natural"], POOL - 2)]
    seeds = [int(s) for s in rng.integers(1, 1 << 20, POOL)]
    return kinds, seeds


def pool_frames(P):
    w, h, ch = P["w"], P["h"], P["ch"]
    out = []
    for k, s in zip(P["pool_kinds"], P["pool_seeds"]):
        f = chain_frame(w, h, P["mode"], ch, P["per_channel"], int(k[-1])) if k.startswith("chain") else FS.make_frame(k, w, h, s)
        out.append(np.ascontiguousarray(FS.to_channels(f, ch)))
    return np.stack(out)


# ---- the host model -----------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, P, O=None):
        if O is None:
            from oracle import oracle as O
            O.build()
        self.O, self.P = O, dict(P)   # (a copy: an option step of a named case changes the scratch bound)
        self.L = L = layout(P)
        self.w, self.h, self.ch = P["w"], P["h"], P["ch"]
        self.buf = {name: np.full(size, 255, np.uint8) for name, size in L["sizes"].items()}
        for name in self.buf:
            if name[:3] in ("pts", "lin", "seg", "cir", "thr", "com"):
                self.buf[name][:] = CANARY_BYTE
        frames = pool_frames(P)
        self.put("frames", L["ilead"], L["ip"], L["ifs"], frames.reshape(POOL, self.h, -1), log=False)
        for k in range(NOUT):   # the outputs start as empty maps inside their padding of 255s
            self.put("maps", out_start(L, k), L["op"], L["ofs"], np.zeros((L["nmax"], self.h, self.w), np.uint8), log=False)
        self.put("sout", L["soff"], L["sp"], L["sfs"], np.zeros((L["nmax"], self.h, self.w), np.uint8), log=False)
        self.per_channel = bool(P["per_channel"])
        self.table = False
        self.pending = []          # pipelined runs in flight: (buffer, lo, hi, staged)
        self.hough_key = self.seg_key = None
        self.hough_bytes = self.seg_bytes = self.circle_bytes = self.ccl_bytes = self.morph_bytes = 0
        self.label_spans = []      # (buffer, lo, hi) that components steps wrote as labels over outputs and no later write has covered
        self.morph_spans = []      # ... that morph steps wrote into `maps` or `sout`
        self.dist_spans = []       # ... that dist steps wrote as distance planes over outputs
        self.deriv_n = None        # frames the last deriv step wrote (None: the planes still hold the arena's fill)
        self.lines_queued = False  # a lines step since the last sync ...
        self.circles_open = 0      # ... and the circles steps behind it that no lines step has followed yet
        self.counters = dict.fromkeys(COUNTERS, 0)
        self.writes = []           # (step, buffer, lo, hi)
        self.step = -1

    # -- bytes --
    def _index(self, off, pitch, fs, n, rows, row_bytes):
        return (off + np.arange(n)[:, None, None] * fs + np.arange(rows)[None, :, None] * pitch + np.arange(row_bytes)[None, None, :]).astype(np.int64)

    def get(self, name, off, pitch, fs, n, row_bytes):
        return self.buf[name][self._index(off, pitch, fs, n, self.h, row_bytes)]

    def put(self, name, off, pitch, fs, rows3, log=True):
        rows3 = np.ascontiguousarray(rows3).view(np.uint8).reshape(rows3.shape[0], rows3.shape[1], -1)
        n, rows, rb = rows3.shape
        self.buf[name][self._index(off, pitch, fs, n, rows, rb)] = rows3
        if log:
            hi = off + (n - 1) * fs + (rows - 1) * pitch + rb
            self.writes.append((self.step, name, off, hi))
            for spans in (self.label_spans, self.morph_spans, self.dist_spans):   # (the counters' bookkeeping, by byte range)
                spans[:] = [s for s in spans if not (s[0] == name and off <= s[1] and s[2] <= hi)]

    def put_words(self, name, off, words):
        b = np.ascontiguousarray(words).view(np.uint8).reshape(-1)
        self.buf[name][off:off + b.size] = b
        self.writes.append((self.step, name, off, off + b.size))

    def words(self, name, off, count, dtype):
        return self.buf[name][off:off + 4 * count].view(dtype)

    # -- the runs in flight (counters only: expected values never depend on them) --
    def _overlapping(self, name, lo, hi):
        return [p for p in self.pending if p[0] == name and p[1] < hi and lo < p[2]]

    def _finish(self, hit):
        self.pending = [p for p in self.pending if p not in hit]

    def _reader(self, name, lo, hi, kind, counter=None):
        hit = self._overlapping(name, lo, hi)
        if hit:
            self.counters[counter or f"overlap_{kind}"] += 1
            self._finish(hit)
        elif any(p[0] == name and (p[1] == hi or p[2] == lo) for p in self.pending):
            self.counters["adjacent"] += 1

    @staticmethod
    def _touches(spans, name, lo, hi):
        return any(b == name and s0 < hi and lo < s1 for b, s0, s1 in spans)

    def _reads(self, name, lo, hi):
        """Books a read of [lo, hi) of a buffer for the two counters of propagation."""
        self.counters["morph_read_by_a_later_step"] += self._touches(self.morph_spans, name, lo, hi)
        self.counters["dist_plane_read_as_map"] += self._touches(self.dist_spans, name, lo, hi)

    def _run_output(self, out, maps):
        """Writes a run's maps into output `out` (0 .. NOUT - 1 in place, "sout" staged) and books the run as in flight: with
        HC_OPT_PIPELINE that holds for hc_run_device, hc_canny_device ("a run in every sense hc_run_device is one: pipeline slots
        and HC_OPT_PIPELINE", include/hipcanny.h) and hc_run_gradients_device ("stream semantics as hc_run_device") alike."""
        L = self.L
        n = len(maps)
        if out == "sout":
            name, off, pitch, fs = "sout", L["soff"], L["sp"], L["sfs"]
            lo, hi = view_span(L, off, pitch, fs, n, self.w)
            self.counters["staged_runs"] += 1
        else:
            name, off, pitch, fs = "maps", out_start(L, out), L["op"], L["ofs"]
            lo, hi = off, off + n * fs
        self.put(name, off, pitch, fs, maps)
        if self.P["pipeline"]:
            self._finish(self._overlapping(name, lo, hi) + ([p for p in self.pending if p[3]] if out == "sout" else []))
            self.pending = (self.pending + [(name, lo, hi, out == "sout")])[-4:]

    def _frames(self, src, f0, n):
        L = self.L
        return self.get(src, L["ilead"] + f0 * L["ifs"], L["ip"], L["ifs"], n, self.w * self.ch).reshape((n, self.h, self.w) + ((3,) if self.ch == 3 else ()))

    def _thresholds(self, f):
        if self.table:
            self.counters["runs_with_frame_table"] += f == 0
            lo, hi = (int(v) for v in self.words("thr", 4 * GUARD + 8 * f, 2, np.int32))
            return AT.normalised(lo, hi)
        return self.P["low"], self.P["high"]

    # -- steps --
    def apply(self, i, st):
        self.step = i
        getattr(self, "do_" + st["kind"])(st)

    def do_run(self, st):
        fr = self._frames(st["src"], st["f0"], st["n"])
        if self.P["mode"] == "O":
            maps = [self.O.canny_o(f, *self._thresholds(k)) for k, f in enumerate(fr)]
        elif self.per_channel:
            maps = [self.O.canny_r(np.ascontiguousarray(f[:, :, c]), self.P["low"], self.P["high"]) for f in fr for c in range(3)]
        elif self.ch == 1:
            maps = list(self.O.canny_r_batch(fr, self.P["low"], self.P["high"]))
        else:
            maps = [self.O.canny_r(f, self.P["low"], self.P["high"]) for f in fr]
        self._run_output(st["out"], np.stack(maps))

    def do_canny(self, st):
        s = 16.0 if st["aperture"] == 7 else 1.0
        fr = self._frames("frames", st["f0"], st["n"])
        self._run_output(st["out"], np.stack([X.canny_o_from_gradients(*D.sobel16(f, st["aperture"]), st["low"] / s, st["high"] / s, bool(st["l2"])) for f in fr]))

    def _planes(self, n):
        L = self.L
        return [(512 + p * L["pf"] * L["dfs"], L["dp"], L["dfs"]) for p in range(2)]

    def do_deriv(self, st):
        dx, dy = D.sobel16_frames(self._frames("frames", st["f0"], st["n"]), st["ksize"])
        for (off, pitch, fs), plane in zip(self._planes(st["n"]), (dx, dy)):
            self.put("dxdy", off, pitch, fs, plane.reshape(st["n"], self.h, -1))
        self.deriv_n = st["n"]

    def do_rungrad(self, st):
        shape = (st["n"], self.h, self.w) + ((3,) if self.ch == 3 else ())
        dx, dy = (self.get("dxdy", off, pitch, fs, st["n"], 2 * self.ch * self.w).view(np.int16).reshape(shape) for off, pitch, fs in self._planes(st["n"]))
        self._run_output(st["out"], np.stack([X.canny_o_from_gradients(a, b, *self._thresholds(k), False) for k, (a, b) in enumerate(zip(dx, dy))]))

    def blur_views(self, st):
        """((buffer, offset, pitch, frame stride) of the input, the same of the output) of a blur step."""
        L = self.L
        def one(where, f):
            if where in ("frames", "blur"):
                return where, L["ilead"] + f * L["ifs"], L["ip"], L["ifs"]
            if where == "sout":
                return "sout", L["soff"] + f * L["sfs"], L["sp"], L["sfs"]
            return "maps", out_start(L, where) + f * L["ofs"], L["op"], L["ofs"]
        return one(st["src"], st["f0"]), one(st["dst"], st["g0"])

    def do_blur(self, st):
        (a, aoff, ap, afs), (b, boff, bp, bfs) = self.blur_views(st)
        rb, n = self.w * self.ch, st["n"]
        self._reader(a, *view_span(self.L, aoff, ap, afs, n, rb), "blur_in")
        self._reads(a, *view_span(self.L, aoff, ap, afs, n, rb))
        span =view_span(self.L, boff, bp, bfs, n, rb)
        self.counters["blur_into_pending_copy_dst"] += any(p[3] for p in self._overlapping(b, *span))
        self._reader(b, *span, "blur_out")
        src = self.get(a, aoff, ap, afs, n, rb).reshape((n, self.h, self.w) + ((3,) if self.ch == 3 else ()))
        self.put(b, boff, bp, bfs, G.blur_frames(src, G.gaussian_taps_q8(st["ksize"], st["sigma"]), st["border"]).reshape(n, self.h, rb))

    def do_autothr(self, st):
        pairs = [AT.thresholds(f, st["rule"], st["param"]) for f in self._frames("frames", st["f0"], st.get("n", MAX_BATCH))]
        self.put_words("thr", 4 * GUARD, np.array(pairs, np.int32))

    def do_thr_on(self, st):
        self.table = True

    def do_thr_off(self, st):
        self.table = False

    def do_sync(self, st):
        self.pending = []
        self.lines_queued, self.circles_open = False, 0

    def do_stream(self, st):
        self.pending = []
        self.lines_queued, self.circles_open = False, 0

    def do_option(self, st):   # (named cases: hc_set_option completes what is in flight)
        self.pending = []
        if st["option"] == api.OPT_PER_CHANNEL:
            self.per_channel = bool(st["value"])
        if st["option"] == api.OPT_TEST_HOUGH_SCRATCH:
            self.P["hough_bound"] = st["value"]

    def _maps(self, st):
        name, off, pitch, fs, _ = resolve_view(self.L, st["view"])
        self._reader(name, *view_span(self.L, off, pitch, fs, st["n"], self.w), st["view"][0])
        self._reads(name, *view_span(self.L, off, pitch, fs, st["n"], self.w))
        if st["n"] > MAX_BATCH:
            self.counters["n_above_max_batch"] += 1
        return self.get(name, off, pitch, fs, st["n"], self.w)

    def do_points(self, st):
        maps, L, cap, name = self._maps(st), self.L, st["cap"], f"pts{st['slot']}"
        self.put_words(name, L["counts_off"], np.array([EP.count(m) for m in maps], np.uint32))
        for f, m in enumerate(maps):
            p = EP.points(m, cap)
            if len(p):
                self.put_words(name, L["list_off"] + 8 * cap * f, p)
            self.counters["lists_cut"] += EP.count(m) > cap > 0

    def _list(self, name, f, cap, width, dtype):
        """The first min(count, cap) entries of slot f of a list buffer."""
        L = self.L
        count = int(self.words(name, L["counts_off"] + 4 * f, 1, np.uint32)[0])
        k = min(count, cap)
        return self.words(name, L["list_off"] + 4 * width * cap * f, width * k, dtype).reshape(k, width).copy()

    def do_lines(self, st):
        L, geo, cap, name = self.L, GEOS[st["geo"]], st["lcap"], f"lines{st['lslot']}"
        key = (R.geometry(self.w, self.h, *geo)[0],) + geo
        if self.hough_key is not None and key != self.hough_key and key[0] == self.hough_key[0]:
            self.counters["hough_tables_equal_numangle"] += 1
        self.hough_key = key
        self.counters["circles_between_lines"] += self.circles_open
        self.lines_queued, self.circles_open = True, 0
        need, passes, _ = hough_need(self.w, self.h, geo, st["n"], self.P["hough_bound"])
        self.counters["scratch_growths"] += 0 < self.hough_bytes < need
        self.hough_bytes = max(self.hough_bytes, need)
        self.counters["hough_passes_above_one"] += passes > 1
        self.counters["n_above_max_batch"] += st["n"] > MAX_BATCH
        res = [R.hough_lines(self._list(f"pts{st['pslot']}", f, st["pcap"], 2, np.int32), self.w, self.h, geo[0], geo[1], st["threshold"], geo[2], geo[3], cap)
               for f in range(st["n"])]
        self.put_words(name, L["counts_off"], np.array([c for c, _ in res], np.uint32))
        for f, (c, lines) in enumerate(res):
            if len(lines):
                self.put_words(name, L["list_off"] + 12 * cap * f, lines)
            self.counters["line_lists_nonempty"] += c > 0
            self.counters["lists_cut"] += c > cap > 0

    def do_segs(self, st):
        L, geo, cap, name = self.L, GEOS[st["geo"]], st["scap"], f"segs{st['sslot']}"
        maps = self._maps(st)
        key = (R.geometry(self.w, self.h, *geo)[0],) + geo
        if self.seg_key is not None and key != self.seg_key and key[0] == self.seg_key[0]:
            self.counters["seg_tables_equal_numangle"] += 1
        self.seg_key = key
        self.counters["scratch_growths"] += 0 < self.seg_bytes < 4 * st["n"] * st["lcap"]
        self.seg_bytes = max(self.seg_bytes, 4 * st["n"] * st["lcap"])
        self.counters["mismatched_geometry"] += st["geo"] != st["lgeo"]
        res = [S.segments_of(m, self._list(f"lines{st['lslot']}", f, st["lcap"], 3, np.float32), self.w, self.h, *geo, st["min_length"], st["max_gap"], cap)
               for f, m in enumerate(maps)]
        self.put_words(name, L["counts_off"], np.array([c for c, _ in res], np.uint32))
        for f, (c, segs) in enumerate(res):
            if len(segs):
                self.put_words(name, L["list_off"] + 16 * cap * f, segs)
            self.counters["seg_lists_nonempty"] += c > 0
            self.counters["lists_cut"] += c > cap > 0

    def do_circles(self, st):
        """hc_hough_circles_device on the point lists of slot pslot and the first W int16 of every row of the gradient planes --
        whatever they hold: the planes of the last deriv step (on a 3-channel context its interleaved rows, of which the entry
        reads a defined one-channel view), older planes in the frames behind that step's n, the arena's fill (-1, -1: every ray
        a diagonal) where no deriv step wrote.  The entry is no reader of edge maps: it completes no run (no _reader call)."""
        L, n, cap, name, c = self.L, st["n"], st["ccap"], f"circ{st['cslot']}", self.counters
        need, passes, _ = circle_need(self.w, self.h, st["dp"], st["cc"], n, self.P["hough_bound"])
        assert passes, f"one frame of {describe(st)} exceeds the scratch bound: the entry refuses it"
        c["circle_scratch_growths"] += 0 < self.circle_bytes < need
        self.circle_bytes = max(self.circle_bytes, need)
        c["circle_passes_above_one"] += passes > 1
        c["n_above_max_batch"] += n > MAX_BATCH
        c["circles_on_unwritten_planes"] += self.deriv_n is None
        c["circles_on_stale_frames"] += self.deriv_n is not None and n > self.deriv_n
        self.circles_open += self.lines_queued
        pts = [self._list(f"pts{st['pslot']}", f, st["pcap"], 2, np.int32) for f in range(n)]
        stored = self.words(f"pts{st['pslot']}", L["counts_off"], n, np.uint32)
        dx, dy = (self.get("dxdy", off, pitch, fs, n, 2 * self.w).view(np.int16) for off, pitch, fs in self._planes(n))
        par, stats = (st["dp"], st["min_dist"], st["threshold"], st["rmin"], st["rmax"]), {}
        counts, circles = HC.circles_batch(pts, dx, dy, self.w, self.h, *par, centre_capacity=st["cc"], capacity=cap, stats=stats)
        c["circles_dropped_by_min_dist"] += stats.get("dropped", 0)
        self.put_words(name, L["counts_off"], counts)
        for f in range(n):
            if len(circles[f]):
                self.put_words(name, L["list_off"] + 16 * cap * f, circles[f])
            c["circle_lists_nonempty"] += int(counts[f]) > 0
            c["circle_lists_cut"] += int(counts[f]) > cap > 0
            c["circles_from_cut_points"] += int(stored[f]) > st["pcap"]
            c["circles_centres_cut"] += len(HC.centres(HC.accumulate(pts[f], dx[f], dy[f], self.w, self.h, par[0], par[3], par[4]), par[2])) > st["cc"]

    def do_components(self, st):
        """hc_connected_components_device on a view of maps -- whatever bytes it holds: a run's maps, a blur's output, the labels an
        earlier step laid over the region, of which every non-zero byte is foreground.  The entry reads the maps and writes the
        label plane, and completes the runs in flight that write either (as do_blur books its output).  It writes [row, row + 4 W)
        of each label row, the n counts and min(N, capacity) rows per frame, the centroids as float64 bits; nothing behind them."""
        L, n, cap, c = self.L, st["n"], st["cap"], self.counters
        name, off, pitch, fs, _ = resolve_view(L, st["view"])
        mspan = view_span(L, off, pitch, fs, n, self.w)
        c["components_overlap_map"] += bool(self._overlapping(name, *mspan))
        c["components_of_label_bytes"] += any(b == name and lo < mspan[1] and mspan[0] < hi for b, lo, hi in self.label_spans)
        maps = self._maps(st)
        c["components_n_above_max_batch"] += n > MAX_BATCH
        lname, loff, lpitch, lfs = label_view(L, st)
        lspan = view_span(L, loff, lpitch, lfs, n, 4 * self.w)
        assert lname != name or lspan[1] <= mspan[0] or mspan[1] <= lspan[0], f"the label plane of {describe(st)} overlaps its map: the entry refuses it"
        self._reader(lname, *lspan, "labels", counter="components_labels_over_pending")
        need, passes, _ = ccl_need(self.h, n, self.P["hough_bound"])
        assert passes, f"one frame of {describe(st)} exceeds the scratch bound: the entry refuses it"
        c["ccl_scratch_growths"] += 0 < self.ccl_bytes < need
        self.ccl_bytes = max(self.ccl_bytes, need)
        c["ccl_passes_above_one"] += passes > 1
        c["components_capacity_0"] += cap == 0
        labels, counts, stats, cents = CC.connected_components(maps, st["conn"], cap)
        self.put(lname, loff, lpitch, lfs, labels)
        if st["dest"] == "over":
            self.label_spans.append((lname,) + lspan)
        out = f"comp{st['cslot']}"
        self.put_words(out, L["counts_off"], counts)
        for f in range(n):
            c["components_rows_cut"] += int(counts[f]) > cap > 0
            if cap and len(stats[f]):   # (rows: the pointers are null only with capacity 0)
                self.put_words(out, L["stats_off"] + 20 * cap * f, stats[f])
                self.put_words(out, L["cent_off"] + 16 * cap * f, cents[f])

    def do_morph(self, st):
        """hc_morphology_device on a one-channel view of maps (whatever bytes it holds, as do_components) or on 3-channel frames of
        the pool, into a view the step names.  The entry completes the runs in flight that write either view (as do_blur books
        them) and writes exactly [row, row + channels * W) of each output row.  Morphed bytes in `maps` or `sout` are what later
        steps read there."""
        L, n, cn, c = self.L, st["n"], st["channels"], self.counters
        (a, aoff, ap, afs), (b, boff, bp, bfs) = morph_views(L, st)
        rb = cn * self.w
        ispan, ospan = view_span(L, aoff, ap, afs, n, rb), view_span(L, boff, bp, bfs, n, rb)
        assert a != b or ispan[1] <= ospan[0] or ospan[1] <= ispan[0], f"the output of {describe(st)} overlaps its input: the entry refuses it"
        c["morph_overlap_in"] += bool(self._overlapping(a, *ispan))
        c["morph_of_label_bytes"] += self._touches(self.label_spans, a, *ispan)
        if st["src"] == "frames":
            src = self._frames("frames", st["f0"], n)
        else:
            src = self._maps(st)
        self._reader(b, *ospan, "morph_out", counter="morph_out_over_pending")
        c["morph_three_channel"] += cn == 3
        c["morph_n_above_max_batch"] += n > MAX_BATCH
        need, passes, _ = morph_need(self.w, self.h, cn, st["op"], n, self.P["hough_bound"])
        assert passes, f"one intermediate frame of {describe(st)} exceeds the scratch bound: the entry refuses it"
        c["morph_scratch_growths"] += 0 < self.morph_bytes < need
        self.morph_bytes = max(self.morph_bytes, need)
        c["morph_passes_above_one"] += passes > 1
        out = MR.morph(src, st["op"], list(st["spans"]), cn)
        c["morph_output_differs"] += not np.array_equal(out, src)
        self.put(b, boff, bp, bfs, out.reshape(n, self.h, rb))
        if b in ("maps", "sout"):
            self.morph_spans.append((b,) + ospan)

    def do_dist(self, st):
        """hc_distance_transform_device on a view of maps -- whatever bytes it holds -- into a distance plane (squared int32, or the
        float32 root) and, where the step has one, a nearest plane.  The entry completes the runs in flight that write any of the
        three views and writes exactly [row, row + 4 W) of each row of either plane: side by side in one plane, the words between
        and around the two ROIs stay what they were.  A frame without a feature pixel gives HC_DT_NONE / +inf and -1."""
        L, n, c = self.L, st["n"], self.counters
        name, off, pitch, fs, _ = resolve_view(L, st["view"])
        mspan = view_span(L, off, pitch, fs, n, self.w)
        c["dist_overlap_map"] += bool(self._overlapping(name, *mspan))
        c["dist_of_morph_output"] += self._touches(self.morph_spans, name, *mspan)
        maps = self._maps(st)
        c["dist_n_above_max_batch"] += n > MAX_BATCH
        (dn, doff, dpitch, dfs), near = dist_views(L, st)
        dspan = view_span(L, doff, dpitch, dfs, n, 4 * self.w)
        assert dn != name or dspan[1] <= mspan[0] or mspan[1] <= dspan[0], f"the distance plane of {describe(st)} overlaps its map: the entry refuses it"
        self._reader(dn, *dspan, "dist", counter="dist_plane_over_pending")
        c["dist_side_by_side"] += st["near"] == "side"
        feat = DR.features(maps, st["target"])
        c["dist_without_features"] += sum(not f.any() for f in feat)
        c["dist_maps_mixed"] += any(f.any() and not f.all() for f in feat)
        d2, nearest = DR.distance_transform(maps, st["target"], DR.vectorised)
        self.put(dn, doff, dpitch, dfs, DR.root_f32(d2) if st["dtype"] == api.DT_F32 else d2)
        if near is not None:
            self.put(*near, nearest)
        if st["dest"] == "over":
            self.dist_spans.append((dn,) + dspan)


def run_model(P, steps, O=None):
    m = Model(P, O)
    for i, st in enumerate(steps):
        m.apply(i, st)
    return m


# ---- the generator ------------------------------------------------------------------------------------------------------------
def make_params(rng):
    w, h = SIZES[int(rng.integers(0, len(SIZES)))]
    ch = 3 if rng.random() < 0.4 else 1
    mode = "R" if rng.random() < 0.55 else "O"
    pc = bool(ch == 3 and mode == "R" and rng.random() < 0.6)
    P = dict(w=w, h=h, ch=ch, mode=mode, per_channel=pc, per_channel_ever=pc, pipeline=bool(rng.random() < 0.7), low=10 if mode == "R" else 50, high=40 if mode == "R" else 150)
    P["hough_bound"] = 2 * hough_need(w, h, GEO_BIG, 1, 0)[2] if rng.random() < 0.3 else 0   # (as test_several_passes_equal_one: whole frames of the largest geometry)
    P["staged"] = str(rng.choice(STAGED_FAMILIES))
    P["pool_kinds"], P["pool_seeds"] = make_pool(rng)
    return P


def draw_view(rng, L, written, nlim):
    """A reader's view and its n: mostly of an output a run has written."""
    ks = [k for k in range(NOUT) if written.get(k)] or [0]
    k = int(rng.choice(ks))
    nw = written.get(k, 1)
    c = rng.random()
    if c < 0.35:
        return ("whole", k), int(rng.integers(1, nlim + 1))
    if c < 0.55:
        return ("frame", k, nw - 1), 1
    if c < 0.75:
        return ("roi", k, int(rng.integers(0, max(nw - 1, 1))), int(rng.integers(1, 6)), int(rng.integers(0, 3)), int(rng.integers(1, 3))), 1
    if c < 0.85:
        return ("before", k), 1
    if c < 0.93 or not written.get("sout"):
        return ("behind", k, nw), 1
    return ("sout",), int(rng.integers(1, written["sout"] + 1))


def make_steps(P, rng):
    L = layout(P)
    w, h, ch, mode, piped = P["w"], P["h"], P["ch"], P["mode"], P["pipeline"]
    nlim = L["nmax"]
    per = 3 if P["per_channel"] else 1
    steps, written, plist, llist = [], {}, {}, {}
    state = dict(blur=0, deriv=0, table_written=False, table_on=False, stream="own", next_out=0)

    def run_out():
        if rng.random() < 0.25:
            return "sout"
        k, state["next_out"] = state["next_out"], (state["next_out"] + 1) % NOUT
        return k

    def add_run(f0=None, n=None, src="frames", out=None):
        n = int(rng.integers(1, MAX_BATCH + 1)) if n is None else n
        f0 = int(rng.integers(0, POOL - n + 1)) if f0 is None else f0
        out = run_out() if out is None else out
        steps.append(dict(kind="run", src=src, f0=f0, n=n, out=out))
        written[out] = n * per

    def add_points(view=None, n=None, cap=None, slot=None):
        if view is None:
            view, n = draw_view(rng, L, written, nlim)
        cap = int(rng.choice([0, 5, w * h, w * h])) if cap is None else cap
        slot = int(rng.integers(0, 2)) if slot is None else slot
        steps.append(dict(kind="points", view=view, n=n, slot=slot, cap=cap))
        plist[slot] = dict(n=n, cap=cap)

    def add_lines(pslot, geo=None, lcap=None, threshold=None):
        meta = plist[pslot]
        geo = int(rng.choice([0, 0, 1, 2, 3])) if geo is None else geo
        lcap = int(rng.choice([0, 4, 64, LCAP_MAX])) if lcap is None else lcap
        lslot = int(rng.integers(0, 2))
        n = int(rng.integers(1, meta["n"] + 1)) if rng.random() < 0.4 else meta["n"]
        steps.append(dict(kind="lines", pslot=pslot, pcap=meta["cap"], n=n, geo=geo, threshold=int(rng.choice([6, 10, 18])) if threshold is None else threshold, lslot=lslot, lcap=lcap))
        llist[lslot] = dict(n=n, lcap=lcap, geo=geo)

    def add_segs(lslot, view=None, match=None, scap=None):
        meta = llist[lslot]
        if view is None:
            view, _ = draw_view(rng, L, written, nlim)
        n = min(meta["n"], resolve_view(L, view)[4])
        geo = meta["geo"]
        if (rng.random() < 0.2 if match is None else not match) and SAME_NUMANGLE[geo]:
            geo = int(rng.choice(SAME_NUMANGLE[geo]))
        steps.append(dict(kind="segs", view=view, n=n, lslot=lslot, lcap=meta["lcap"], lgeo=meta["geo"], geo=geo, min_length=int(rng.choice([0, 3, 6])), max_gap=int(rng.choice([0, 2, 5])),
                          sslot=int(rng.integers(0, 2)), scap=int(rng.choice([0, 8, SCAP_MAX, SCAP_MAX])) if scap is None else scap))

    # the opening every sequence has: runs on the chain content, then points, lines and segments of the first output, unsynchronised
    add_run(f0=0, n=MAX_BATCH, out=0)
    if piped:
        add_run(f0=1, n=int(rng.integers(2, MAX_BATCH + 1)), out=1)
    add_points(view=("whole", 0), n=int(rng.integers(MAX_BATCH, nlim + 1)) if nlim > MAX_BATCH else MAX_BATCH, cap=w * h, slot=0)
    add_lines(0, geo=0, lcap=64, threshold=6)
    add_segs(steps[-1]["lslot"], view=("whole", 0), match=True, scap=SCAP_MAX)
    total = int(rng.integers(12, 21))
    weights = dict(run=5, canny=2 if mode == "O" else 0, deriv=1, rungrad=2 if mode == "O" else 0, blur=3, autothr=1.5, thr_on=2.5 if mode == "O" else 0, thr_off=0.7 if mode == "O" else 0,
                   points=4, lines=5, segs=5, sync=1.2, stream=0.6)
    def room():   # steps that may still be drawn: the final sync, and the step that takes an installed table off, are kept free
        return total - 1 - int(state["table_on"]) - len(steps)

    while room() > 0:
        kind = str(rng.choice(list(weights), p=np.array(list(weights.values())) / sum(weights.values())))
        if kind == "run":
            from_blur = state["blur"] and rng.random() < 0.35
            n = int(rng.integers(1, (state["blur"] if from_blur else MAX_BATCH) + 1))
            add_run(f0=0 if from_blur else None, n=n, src="blur" if from_blur else "frames")
        elif kind == "canny":
            ap = int(rng.choice([3, 5, 7, -1]))
            n = int(rng.integers(1, MAX_BATCH + 1))
            out = run_out()
            steps.append(dict(kind="canny", f0=int(rng.integers(0, POOL - n + 1)), n=n, out=out, low=CANNY_THR[ap][0], high=CANNY_THR[ap][1], aperture=ap, l2=int(rng.random() < 0.25)))
            written[out] = n
        elif kind == "deriv":
            n = int(rng.integers(1, MAX_BATCH + 1))
            steps.append(dict(kind="deriv", f0=int(rng.integers(0, POOL - n + 1)), n=n, ksize=int(rng.choice([3, 5, 7, -1]))))
            state["deriv"] = n
        elif kind == "rungrad" and state["deriv"]:
            out = run_out()
            n = int(rng.integers(1, state["deriv"] + 1))
            steps.append(dict(kind="rungrad", n=n, out=out))
            written[out] = n
        elif kind == "blur":
            n = int(rng.integers(1, MAX_BATCH + 1))
            outs = [k for k in range(NOUT) if written.get(k)]
            src, f0, dst, g0 = "frames", int(rng.integers(0, POOL - n + 1)), "blur", 0
            if ch == 1 and outs and rng.random() < 0.6:
                if rng.random() < 0.5:     # the input is a run's output (frame 0 of it, or from there on)
                    src, f0, n = int(rng.choice(outs)), 0, int(rng.integers(1, 3))
                else:                       # the output is one, wholly or in part -- or the buffer a staged run copies to
                    dst = "sout" if written.get("sout") and rng.random() < 0.5 else int(rng.choice(outs))
                    g0 = int(rng.integers(0, L["nmax"] - n + 1)) if rng.random() < 0.5 else 0
            steps.append(dict(kind="blur", src=src, f0=f0, dst=dst, g0=g0, n=n, ksize=int(rng.choice([3, 5, 7])), sigma=float(rng.choice([0.0, 1.2])), border=int(rng.integers(0, 2))))
            if dst == "blur":
                state["blur"] = n
            else:
                written[dst] = max(written.get(dst, 0), g0 + n)
        elif kind == "autothr":
            steps.append(dict(kind="autothr", f0=int(rng.integers(0, POOL - MAX_BATCH + 1)), rule=int(rng.integers(0, 2)), param=float(rng.choice([0.33, 0.5]))))
            state["table_written"] = True
            if mode == "O" and not state["table_on"] and room() >= 2 and rng.random() < 0.6:   # ... installed at once, so that later runs read it
                steps.append(dict(kind="thr_on"))
                state["table_on"] = True
        elif kind == "thr_on" and state["table_written"] and not state["table_on"] and room() >= 2:
            steps.append(dict(kind="thr_on"))
            state["table_on"] = True
        elif kind == "thr_off" and state["table_on"]:
            steps.append(dict(kind="thr_off"))
            state["table_on"] = False
        elif kind == "points":
            add_points()
        elif kind == "lines":
            ok = [s for s, m in plist.items() if m["cap"] > 0]
            if ok:
                add_lines(int(rng.choice(ok)))
        elif kind == "segs":
            ok = [s for s, m in llist.items() if m["lcap"] > 0]
            if ok:
                add_segs(int(rng.choice(ok)))
        elif kind == "sync":
            steps.append(dict(kind="sync"))
        elif kind == "stream" and room() >= 1 + (steps[-1]["kind"] != "sync"):   # include/hipcanny.h: a caller who changes the stream between calls that share scratch synchronises first
            if steps[-1]["kind"] != "sync":
                steps.append(dict(kind="sync"))
            state["stream"] = "side" if state["stream"] == "own" else "own"
            steps.append(dict(kind="stream", to=state["stream"]))
    if state["table_on"]:
        steps.append(dict(kind="thr_off"))   # the context's pair is restored with null
    steps.append(dict(kind="sync"))
    return steps


def add_circles(P, steps, rng):
    """Inserts 1 .. 3 circles steps into `steps`: each behind the opening's points step, before the final sync and never directly
    in front of a stream step (the sync there stays adjacent to the switch: include/hipcanny.h on calls that share scratch).  A
    circles step reads the lists of the points step most recently in front of it, whichever slot and capacity, 0 included.  Every
    draw comes from `rng`, a generator of the circles' own: the steps make_steps drew stay what they were, in their order."""
    w, h, bound = P["w"], P["h"], P["hough_bound"]
    steps = list(steps)
    first = next(i for i, st in enumerate(steps) if st["kind"] == "points")
    for _ in range(int(rng.integers(1, 4))):
        at = int(rng.choice([i for i in range(first + 1, len(steps)) if steps[i]["kind"] != "stream"]))   # the step goes in front of steps[at]
        pts = next(st for st in reversed(steps[:at]) if st["kind"] == "points")
        rmin, rmax = ((1, 6), (2, min(w, h) // 2), (3, 66))[int(rng.integers(0, 3))]
        st = dict(kind="circles", pslot=pts["slot"], pcap=pts["cap"], n=int(rng.integers(1, min(pts["n"], MAX_BATCH) + 1)), dp=float(rng.choice(CIRCLES_DP)),
                  min_dist=float(rng.choice(CIRCLES_MIN_DIST)), threshold=int(rng.choice(CIRCLES_THRESHOLD)), rmin=rmin, rmax=rmax, cc=int(rng.choice(CIRCLES_CC)),
                  cslot=int(rng.integers(0, 2)), ccap=int(rng.choice([0, 8, CCAP_MAX])))
        while bound and circle_need(w, h, st["dp"], st["cc"], 1, 0)[2] > bound and st["cc"] > CIRCLES_CC[0]:   # no committed step is refused: the smaller capacity
            st["cc"] = CIRCLES_CC[CIRCLES_CC.index(st["cc"]) - 1]
        steps.insert(at, st)
    return steps


def written_before(P, steps):
    """What make_steps calls `written` once it has drawn `steps`: output -> frames of it that a step has written."""
    per, written = 3 if P["per_channel"] else 1, {}
    for st in steps:
        if st["kind"] == "run":
            written[st["out"]] = st["n"] * per
        elif st["kind"] in ("canny", "rungrad"):
            written[st["out"]] = st["n"]
        elif st["kind"] == "blur" and st["dst"] != "blur":
            written[st["dst"]] = max(written.get(st["dst"], 0), st["g0"] + st["n"])
        elif st["kind"] == "morph" and st["dst"] in ("maps", "sout"):   # (only add_distance meets these)
            out = st["mslot"] if st["dst"] == "maps" else "sout"
            written[out] = max(written.get(out, 0), st["g0"] + st["n"])
    return written


def add_components(P, steps, rng):
    """Inserts 1 .. 3 components steps into `steps`, by the rules of add_circles: behind the opening's points step, before the
    final sync, never directly in front of a stream step, every draw from `rng`, a generator of the components' own.  A step reads
    a view as a points step draws it (draw_view: all six kinds, up to nmax frames) and writes its labels into an arena of their
    own -- or, one frame of them, OVER an output region of `maps` that its map view does not touch: the one place where the entry
    completes a run for the plane it writes.  What later steps read from that region are those label bytes."""
    L = layout(P)
    w, h = P["w"], P["h"]
    steps = list(steps)
    first = next(i for i, st in enumerate(steps) if st["kind"] == "points")
    for _ in range(int(rng.integers(1, 4))):
        at = int(rng.choice([i for i in range(first + 1, len(steps)) if steps[i]["kind"] != "stream"]))   # the step goes in front of steps[at]
        view, n = draw_view(rng, L, written_before(P, steps[:at]), L["nmax"])
        kind = COMP_CAPS[int(rng.integers(0, len(COMP_CAPS)))]
        cap = {"null": 0, "zero": 0, "one": 1, "cut": int(rng.choice(COMP_CUTS)), "all": w * h + 1}[kind]
        st = dict(kind="components", view=view, n=n, conn=int(rng.choice([4, 8])), cap=cap, rows=kind != "null", cslot=int(rng.integers(0, 2)), dest="own",
                  lslot=int(rng.integers(0, 2)), loff=int(rng.choice(LAB_OFFS)), lpad=int(rng.choice(LAB_PADS)), lgap=int(rng.choice(LAB_GAPS)))
        over, k0 = rng.random() < 0.45, int(rng.integers(0, NOUT))
        if over:   # one frame, over the first region from k0 on (cyclically) that the map view stays clear of: it touches two at most
            name, off, pitch, fs, _ = resolve_view(L, view)
            lo, hi = view_span(L, off, pitch, fs, 1, w)
            free = [k for k in ((k0 + j) % NOUT for j in range(NOUT)) if name != "maps" or hi <= out_start(L, k) or out_start(L, k) + 4 * L["ofs"] <= lo]
            st.update(n=1, dest="over", lslot=free[0], loff=0, lpad=4 * (L["op"] - w), lgap=0)
        steps.insert(at, st)
    return steps


def draw_element(rng):
    """ksize half-widths: one of the three shapes at 3, 5 or 7 -- or, one time in four, an element asymmetric in y with an empty row."""
    if rng.random() < 0.25:
        return list(MORPH_ASYM[int(rng.integers(0, len(MORPH_ASYM)))])
    return [int(v) for v in MR.structuring_spans(int(rng.choice(MR.SHAPES)), int(rng.choice(MR.KSIZES)))]


def draw_map_view(rng, L, written, first):
    """draw_view; the first step a generator inserts takes no view beside an output (those mostly hold one value throughout)."""
    view, n = draw_view(rng, L, written, L["nmax"])
    while first and view[0] in ("before", "behind"):
        view, n = draw_view(rng, L, written, L["nmax"])
    return view, n


def add_morphology(P, steps, rng):
    """Inserts 1 .. 3 morph steps into `steps`, by the rules of add_components: behind the opening's points step, before the final
    sync, never directly in front of a stream step, every draw from `rng`, a generator of the morphology's own.  A step reads a
    one-channel view as a points step draws it (all six kinds, up to nmax frames) -- or, on a 3-channel context, sometimes 3-channel
    frames of the pool -- and writes an arena of its own at any alignment, or frames g0 .. of ANOTHER output region of `maps` or of
    `sout` that its input does not touch (for 3-channel frames: of the `blur` buffer): there the entry completes a run for the
    view it writes, and what later steps read from that region are the morphed bytes."""
    L = layout(P)
    w, ch = P["w"], P["ch"]
    steps = list(steps)
    first = next(i for i, st in enumerate(steps) if st["kind"] == "points")
    for j in range(int(rng.integers(1, 4))):
        at = int(rng.choice([i for i in range(first + 1, len(steps)) if steps[i]["kind"] != "stream"]))   # the step goes in front of steps[at]
        st = dict(kind="morph", src="view", view=None, f0=0, n=1, channels=1, op=int(rng.choice(MR.OPS)), spans=draw_element(rng), dst="own", mslot=int(rng.integers(0, 2)),
                  moff=int(rng.choice(MOR_OFFS)), mpad=int(rng.choice(MOR_PADS)), mgap=int(rng.choice(MOR_GAPS)), g0=0)
        c, elsewhere = rng.random(), dict(moff=0, mpad=0, mgap=0)
        if ch == 3 and rng.random() < 0.4:
            n = int(rng.integers(1, MAX_BATCH + 1))
            st.update(src="frames", channels=3, n=n, f0=int(rng.integers(0, POOL - n + 1)))
            if c < 0.4:
                st.update(elsewhere, dst="blur", mslot=0, g0=int(rng.integers(0, POOL - n + 1)))
        else:
            view, n = draw_map_view(rng, L, written_before(P, steps[:at]), j == 0)
            st.update(view=view, n=n)
            name, off, pitch, fs, _ = resolve_view(L, view)
            lo, hi = view_span(L, off, pitch, fs, n, w)
            g0, k0 = int(rng.integers(0, L["nmax"] - n + 1)) if rng.random() < 0.5 else 0, int(rng.integers(0, NOUT))
            # frames g0 .. g0 + n of the first region from k0 on (cyclically) that the input stays clear of
            free = [k for k in ((k0 + i) % NOUT for i in range(NOUT)) if name != "maps" or hi <= out_start(L, k) + g0 * L["ofs"] or out_start(L, k) + (g0 + n) * L["ofs"] <= lo]
            if c >= 0.85 and name != "sout":
                st.update(elsewhere, dst="sout", mslot=0, g0=g0)
            elif c >= 0.4 and free:
                st.update(elsewhere, dst="maps", mslot=free[0], g0=g0)
        steps.insert(at, st)
    return steps


def add_distance(P, steps, rng):
    """Inserts 1 .. 3 dist steps into `steps`, by the same rules, every draw from `rng`, a generator of the distances' own.  A step
    reads a view as a points step draws it and writes its distances into an arena of their own -- or, one frame of them, OVER an
    output region of `maps` that its map view does not touch, exactly as a components step lays its labels.  The nearest plane:
    none, a view of the other arena, or -- with the distances in an arena -- the second ROI of the same plane, side by side."""
    L = layout(P)
    w = P["w"]
    steps = list(steps)
    first = next(i for i, st in enumerate(steps) if st["kind"] == "points")
    for j in range(int(rng.integers(1, 4))):
        at = int(rng.choice([i for i in range(first + 1, len(steps)) if steps[i]["kind"] != "stream"]))   # the step goes in front of steps[at]
        view, n = draw_map_view(rng, L, written_before(P, steps[:at]), j == 0)
        st = dict(kind="dist", view=view, n=n, target=int(rng.integers(0, 2)), dtype=int(rng.integers(0, 2)), dest="own", dslot=int(rng.integers(0, 2)), doff=int(rng.choice(LAB_OFFS)),
                  dpad=int(rng.choice(LAB_PADS)), dgap=int(rng.choice(LAB_GAPS)), near=DIST_NEARS[int(rng.integers(0, len(DIST_NEARS)))], nslot=int(rng.integers(0, 2)),
                  noff=int(rng.choice(LAB_OFFS)), npad=int(rng.choice(LAB_PADS)), ngap=int(rng.choice(LAB_GAPS)), swords=int(rng.choice(DT_SIDE_WORDS)), nleft=bool(rng.random() < 0.3))
        over, k0 = rng.random() < 0.4, int(rng.integers(0, NOUT))
        if over:   # one frame, over the first region from k0 on (cyclically) that the map view stays clear of: it touches two at most
            name, off, pitch, fs, _ = resolve_view(L, view)
            lo, hi = view_span(L, off, pitch, fs, 1, w)
            free = [k for k in ((k0 + i) % NOUT for i in range(NOUT)) if name != "maps" or hi <= out_start(L, k) or out_start(L, k) + 4 * L["ofs"] <= lo]
            st.update(n=1, dest="over", dslot=free[0], doff=0, dpad=4 * (L["op"] - w), dgap=0, near="own" if st["near"] == "side" else st["near"])
        elif st["near"] == "own":
            st["nslot"] = 1 - st["dslot"]   # two planes of their own: one arena each
        if st["near"] != "side":
            st.update(swords=0, nleft=False)
        if st["near"] != "own":
            st.update(nslot=0, noff=0, npad=0, ngap=0)
        steps.insert(at, st)
    return steps


def base_sequence(seed):
    """(context parameters, steps) of a seed as make_steps draws them from numpy.random.default_rng(seed): no circles step."""
    rng = np.random.default_rng(seed)
    P = make_params(rng)
    return P, make_steps(P, rng)


def make_sequence(seed, O=None):
    """(context parameters, steps, counters) of a seed: the steps of numpy.random.default_rng(seed), the circles steps of
    numpy.random.default_rng([seed, 1]) inserted among them, the components steps of numpy.random.default_rng([seed, 2]) inserted
    among those, the morph steps of default_rng([seed, 3]) among those, the dist steps of default_rng([seed, 4]) among those, and
    the host model; nothing else."""
    P, steps = base_sequence(seed)
    steps = add_circles(P, steps, np.random.default_rng([seed, 1]))
    steps = add_components(P, steps, np.random.default_rng([seed, 2]))
    steps = add_morphology(P, steps, np.random.default_rng([seed, 3]))
    steps = add_distance(P, steps, np.random.default_rng([seed, 4]))
    return P, steps, dict(run_model(P, steps, O).counters)


# ---- the executor ---------------------------------------------------------------------------------------------------------------
class Executor:
    """Queues the steps on one context; at "sync" steps (and when told) compares every buffer with the model."""

    def __init__(self, P, O=None, what=""):
        import torch
        self.torch, self.P, self.what = torch, P, what
        self.model = Model(P, O)
        self.L = self.model.L
        self.d = {name: torch.from_numpy(b.copy()).cuda() for name, b in self.model.buf.items()}
        self.ptr = {name: t.data_ptr() for name, t in self.d.items()}
        self.ctx = api.Context(P["w"], P["h"], P["ch"], self.L["mb"], api.MODE_R if P["mode"] == "R" else api.MODE_O)
        self.side = None
        ctx = self.ctx
        ctx.set_thresholds(P["low"], P["high"])
        if P["per_channel"]:
            ctx.set_option(api.OPT_PER_CHANNEL, 1)
        if P["hough_bound"]:
            ctx.set_option(api.OPT_TEST_HOUGH_SCRATCH, P["hough_bound"])
        if P["pipeline"]:
            ctx.set_option(api.OPT_PIPELINE, 1)
            ctx.set_option(api.OPT_TEST_HYST_GEOM, 1602)   # 32-row tiles
            ctx.set_tuning(0, 1)                           # one queued launch: the chain content is continued from the host
        torch.cuda.synchronize()
        self.step = -1
        self.steps = []

    def close(self):
        if self.side is not None and self.ctx.handle:
            self.ctx.use_own_stream()
        self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _out(self, out):
        L = self.L
        if out == "sout":
            return self.ptr["sout"] + L["soff"], L["sp"], L["sfs"]
        return self.ptr["maps"] + out_start(L, out), L["op"], L["ofs"]

    def _view(self, v):
        name, off, pitch, fs, _ = resolve_view(self.L, v)
        return self.ptr[name] + off, pitch, fs

    def _counts(self, name):
        return self.ptr[name] + self.L["counts_off"]

    def _list(self, name):
        return self.ptr[name] + self.L["list_off"]

    def queue(self, st):
        """One step: the model first (it is the record of what the step means), then the call."""
        self.step += 1
        self.steps.append(st)
        self.model.apply(self.step, st)
        L, ctx, k = self.L, self.ctx, st["kind"]
        if k == "run":
            ctx.run_device(self.ptr[st["src"]] + L["ilead"] + st["f0"] * L["ifs"], L["ip"], L["ifs"], *self._out(st["out"]), st["n"])
        elif k == "canny":
            ctx.canny_device(self.ptr["frames"] + L["ilead"] + st["f0"] * L["ifs"], L["ip"], L["ifs"], *self._out(st["out"]), st["n"], st["low"], st["high"], st["aperture"], st["l2"])
        elif k == "deriv":
            (xo, p, fs), (yo, _, _) = self.model._planes(st["n"])
            ctx.derivatives_device(self.ptr["frames"] + L["ilead"] + st["f0"] * L["ifs"], L["ip"], L["ifs"], self.ptr["dxdy"] + xo, self.ptr["dxdy"] + yo, p, fs, st["n"], st["ksize"])
        elif k == "rungrad":
            (xo, p, fs), (yo, _, _) = self.model._planes(st["n"])
            ctx.run_gradients_device(self.ptr["dxdy"] + xo, self.ptr["dxdy"] + yo, p, fs, *self._out(st["out"]), st["n"])
        elif k == "blur":
            (a, aoff, ap, afs), (b, boff, bp, bfs) = self.model.blur_views(st)
            ctx.gaussian_blur_device(self.ptr[a] + aoff, ap, afs, self.ptr[b] + boff, bp, bfs, st["n"], st["ksize"], G.gaussian_taps_q8(st["ksize"], st["sigma"]), st["border"])
        elif k == "autothr":
            ctx.auto_thresholds_device(self.ptr["frames"] + L["ilead"] + st["f0"] * L["ifs"], L["ip"], L["ifs"], st.get("n", MAX_BATCH), st["rule"], st["param"], self.ptr["thr"] + 4 * GUARD)
        elif k == "thr_on":
            ctx.frame_thresholds_device(self.ptr["thr"] + 4 * GUARD, st.get("n", MAX_BATCH))
        elif k == "thr_off":
            ctx.frame_thresholds_device(None)
        elif k == "points":
            name = f"pts{st['slot']}"
            ctx.edge_points_device(*self._view(st["view"]), st["n"], self._counts(name), self._list(name), st["cap"])
        elif k == "lines":
            p, l = f"pts{st['pslot']}", f"lines{st['lslot']}"
            geo = GEOS[st["geo"]]
            ctx.hough_lines_device(self._list(p), self._counts(p), st["pcap"], st["n"], geo[0], geo[1], st["threshold"], geo[2], geo[3], self._counts(l), self._list(l), st["lcap"])
        elif k == "segs":
            l, s = f"lines{st['lslot']}", f"segs{st['sslot']}"
            ctx.hough_segments_device(*self._view(st["view"]), self._list(l), self._counts(l), st["lcap"], st["n"], *GEOS[st["geo"]], st["min_length"], st["max_gap"],
                                      self._counts(s), self._list(s), st["scap"])
        elif k == "circles":
            p, o = f"pts{st['pslot']}", f"circ{st['cslot']}"
            (xo, pitch, fs), (yo, _, _) = self.model._planes(st["n"])
            ctx.hough_circles_device(self._list(p), self._counts(p), st["pcap"], self.ptr["dxdy"] + xo, self.ptr["dxdy"] + yo, pitch, fs, st["n"], st["dp"], st["min_dist"],
                                     st["threshold"], st["rmin"], st["rmax"], st["cc"], self._counts(o), self._list(o), st["ccap"])
        elif k == "components":
            o, (lname, loff, lpitch, lfs) = f"comp{st['cslot']}", label_view(L, st)
            ctx.connected_components_device(*self._view(st["view"]), st["n"], st["conn"], self.ptr[lname] + loff, lpitch, lfs, self._counts(o),
                                            self.ptr[o] + L["stats_off"] if st["rows"] else None, self.ptr[o] + L["cent_off"] if st["rows"] else None, st["cap"])
        elif k == "morph":
            (a, aoff, ap, afs), (b, boff, bp, bfs) = morph_views(L, st)
            ctx.morphology_device(self.ptr[a] + aoff, ap, afs, self.ptr[b] + boff, bp, bfs, st["n"], st["channels"], st["op"], len(st["spans"]), st["spans"])
        elif k == "dist":
            (dn, doff, dpitch, dfs), near = dist_views(L, st)
            nn, noff, npitch, nfs = near or (dn, 0, 0, 0)
            ctx.distance_transform_device(*self._view(st["view"]), st["n"], st["target"], st["dtype"], self.ptr[dn] + doff, dpitch, dfs, self.ptr[nn] + noff if near else None, npitch, nfs)
        elif k == "sync":
            self.check()
        elif k == "stream":
            if st["to"] == "side":
                self.side = self.side or self.torch.cuda.Stream()
                ctx.set_stream(self.side.cuda_stream)
            else:
                ctx.use_own_stream()
        elif k == "option":
            ctx.set_option(st["option"], st["value"])
        else:
            raise ValueError(k)

    def check(self):
        """hc_sync, then every buffer against the model, byte for byte."""
        self.ctx.sync()
        self.torch.cuda.synchronize()
        for name, want in self.model.buf.items():
            got = self.d[name].cpu().numpy()
            if np.array_equal(got, want):
                continue
            bad = np.flatnonzero(got != want)
            o = int(bad[0])
            by = [(i, lo, hi) for i, b, lo, hi in self.model.writes if b == name and lo <= o < hi]
            who = f"step {by[-1][0]}: {describe(self.steps[by[-1][0]])} (bytes {by[-1][1]} .. {by[-1][2]})" if by else "no step of the model (a guard, padding or canary byte was written)"
            w0 = o // 4 * 4
            raise Mismatch(f"{self.what}: at the sync of step {self.step}, buffer {name}: {len(bad)} bytes differ, first at byte {o}: device {int(got[o])} model {int(want[o])} "
                           f"(the word there: device {got[w0:w0 + 4].view(np.int32)[0]} model {want[w0:w0 + 4].view(np.int32)[0]}; next differing bytes {bad[1:6].tolist()}); last written by "
                           f"{who}.  A seed replays with: python tests/device_op_sequences.py --seed <seed>")

    def continued_runs(self):
        """Runs that needed the host-side continuation so far: hc_hysteresis_totals sums the flag hc_last_hysteresis_info
        (api._again_if_continued) reports per run.  Completes the runs in flight."""
        return self.ctx.hysteresis_totals()[1]


def execute(P, steps, O=None, what=""):
    with Executor(P, O, what) as e:
        for st in steps:
            e.queue(st)
        e.check()
        if P["pipeline"]:
            assert e.continued_runs() > 0, f"{what}: no pipelined run of the sequence was continued from the host"
        return e.model


def run_seed(seed, O=None):
    P, steps, _ = make_sequence(seed, O)
    return execute(P, steps, O, f"seed {seed}")


def main(argv):
    from oracle import oracle as O
    O.build()
    if len(argv) > 3 and argv[1] == "--scan":
        for seed in range(int(argv[2]), int(argv[3])):
            P, steps, c = make_sequence(seed, O)
            print(seed, f"{P['w']}x{P['h']} ch{P['ch']} {P['mode']} pc{int(P['per_channel'])} piped{int(P['pipeline'])} bound{int(bool(P['hough_bound']))} {P['staged']}",
                  f"{len(steps)} steps, " + ", ".join(f"{sum(st['kind'] == k for st in steps)} {k}" for k in ("circles", "components", "morph", "dist")),
                  " ".join(f"{k}={v}" for k, v in c.items() if v), flush=True)
        return 0
    if len(argv) > 2 and argv[1] == "--seed":
        seed = int(argv[2])
        P, steps, counters = make_sequence(seed, O)
        print("context:", P)
        for i, st in enumerate(steps):
            print(f"  {i:2d} {describe(st)}")
        print("counters:", {k: v for k, v in counters.items() if v})
        api.preload_hip_runtime()
        import torch
        if not torch.cuda.is_available():
            print("no GPU: the steps were not run")
            return 0
        try:
            execute(P, steps, O, f"seed {seed}")
        except Mismatch as e:
            print("MISMATCH", e)
            return 1
        print(f"seed {seed}: every buffer equals the model")
        return 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv))
