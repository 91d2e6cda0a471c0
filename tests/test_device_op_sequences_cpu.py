"""tests/device_op_sequences.py without a GPU: the committed seeds give the same sequence and the same expected buffers every time,
exercise what they were chosen for (no vacuous sequence), and contain no call an entry would refuse -- by the limits
include/hipcanny.h documents for each entry, checked here on the steps and the layout of the buffers."""
import os
import subprocess

import numpy as np
import pytest

import device_op_sequences as DS
from test_sanitizers import ENV, ROOT, SAN, _cc


@pytest.fixture(scope="module")
def sequences(oracle):
    return {seed: DS.make_sequence(seed, oracle) for seed in DS.SEEDS}


def test_make_sequence_is_deterministic(oracle, sequences):
    for seed in DS.SEEDS:
        assert DS.make_sequence(seed, oracle) == sequences[seed], seed
    for seed, (P, steps, _) in sequences.items():
        assert 12 <= len([st for st in steps if st["kind"] not in ("circles", "components", "morph", "dist")]) <= 20 and len(steps) <= 32 and steps[-1]["kind"] == "sync", seed
        assert (P["w"], P["h"]) in DS.SIZES and P["ch"] in (1, 3) and P["staged"] in DS.STAGED_FAMILIES, seed


def test_the_circles_steps_leave_every_other_step_where_it_was(sequences):
    """The circles steps come from a generator of their own: without them a sequence is, step for step, what
    numpy.random.default_rng(seed) alone gives -- the sequence the seed was chosen for.  Each stands behind the opening's points
    step, reads the lists of the points step most recently in front of it, and none stands directly in front of a stream switch."""
    for seed, (P, steps, _) in sequences.items():
        steps = [st for st in steps if st["kind"] not in ("components", "morph", "dist")]   # (the next tests: what is left is exactly this)
        P0, base = DS.base_sequence(seed)
        assert P0 == P and [st for st in steps if st["kind"] != "circles"] == base and not any(st["kind"] == "circles" for st in base), seed
        at = [i for i, st in enumerate(steps) if st["kind"] == "circles"]
        assert 1 <= len(at) <= 3, seed
        for i in at:
            pts = [st for st in steps[:i] if st["kind"] == "points"]
            assert pts and (steps[i]["pslot"], steps[i]["pcap"]) == (pts[-1]["slot"], pts[-1]["cap"]) and 1 <= steps[i]["n"] <= min(pts[-1]["n"], DS.MAX_BATCH), (seed, i)
            assert steps[i + 1]["kind"] != "stream", (seed, i)


def test_the_components_steps_leave_every_other_step_where_it_was(sequences):
    """One level up: the components steps come from a third generator, and without them a sequence is exactly what add_circles
    makes of the seed's base steps -- the sequence the seed was chosen for, circles included.  None stands directly in front of a
    stream switch.  A label plane laid over an output region is one frame at four times the region's pitch, and its bytes are
    disjoint from those of the map view; a plane of its own lies in its arena."""
    dests = set()
    for seed, (P, steps, _) in sequences.items():
        P0, base = DS.base_sequence(seed)
        with_circles = DS.add_circles(P0, base, np.random.default_rng([seed, 1]))
        steps = [st for st in steps if st["kind"] not in ("morph", "dist")]   # (the next tests: what is left is exactly this)
        assert [st for st in steps if st["kind"] != "components"] == with_circles and not any(st["kind"] == "components" for st in with_circles), seed
        at = [i for i, st in enumerate(steps) if st["kind"] == "components"]
        first = next(i for i, st in enumerate(steps) if st["kind"] == "points")
        assert 1 <= len(at) <= 3 and first < at[0], seed
        L = DS.layout(P)
        for i in at:
            st = steps[i]
            assert steps[i + 1]["kind"] != "stream" and st["view"][0] in DS.VIEW_KINDS and st["conn"] in (4, 8), (seed, i)
            assert (st["cap"], st["rows"]) in [(0, False), (0, True), (1, True), (P["w"] * P["h"] + 1, True)] + [(c, True) for c in DS.COMP_CUTS], (seed, i)
            name, off, pitch, fs, _ = DS.resolve_view(L, st["view"])
            lname, loff, lpitch, lfs = DS.label_view(L, st)
            mspan, lspan = DS.view_span(L, off, pitch, fs, st["n"], P["w"]), DS.view_span(L, loff, lpitch, lfs, st["n"], 4 * P["w"])
            if st["dest"] == "over":
                assert st["n"] == 1 and lname == "maps" and lpitch == 4 * L["op"] and loff == DS.out_start(L, st["lslot"]) and 0 <= st["lslot"] < DS.NOUT, (seed, i)
                assert lspan[1] <= DS.out_start(L, st["lslot"]) + L["oreg"] and L["nmax"] >= 4, (seed, i)
                assert name != "maps" or lspan[1] <= mspan[0] or mspan[1] <= lspan[0], (seed, i, mspan, lspan)
            else:
                assert st["dest"] == "own" and lname in ("lab0", "lab1") and loff % 4 == 0 and lpitch % 4 == 0 and lfs % 4 == 0 and lfs >= lpitch * P["h"], (seed, i)
                assert DS.LAB_LEAD <= lspan[0] and lspan[1] + DS.LAB_LEAD <= L["sizes"][lname], (seed, i)
            dests.add((st["dest"], st["view"][0]))
    assert {d for d, _ in dests} == {"own", "over"} and {v for _, v in dests} == set(DS.VIEW_KINDS), dests


def _inserted(seed, steps, kind, later):
    """The positions of the steps of `kind` among `steps` without the kinds inserted `later`; 1 .. 3, behind the opening's points
    step, none directly in front of a stream switch."""
    steps = [st for st in steps if st["kind"] not in later]
    at = [i for i, st in enumerate(steps) if st["kind"] == kind]
    first = next(i for i, st in enumerate(steps) if st["kind"] == "points")
    assert 1 <= len(at) <= 3 and first < at[0] and all(steps[i + 1]["kind"] != "stream" for i in at), (seed, kind)
    return steps, at


def test_the_morph_steps_leave_every_other_step_where_it_was(sequences):
    """Another level up: the morph steps come from a fourth generator, and without them (and the dist steps) a sequence is exactly
    what add_components makes of it.  An output in an arena lies inside it at any alignment; one laid into `maps`, `sout` or `blur`
    is whole frames of that buffer's own layout that the input's byte range does not touch.  Across the seeds every destination,
    every operation, every element size, every shape and an asymmetric element with an empty row occur."""
    dsts, ops, elements, odd = set(), set(), set(), set()
    for seed, (P, steps, _) in sequences.items():
        P0, base = DS.base_sequence(seed)
        before = DS.add_components(P0, DS.add_circles(P0, base, np.random.default_rng([seed, 1])), np.random.default_rng([seed, 2]))
        steps, at = _inserted(seed, steps, "morph", ("dist",))
        assert [st for st in steps if st["kind"] != "morph"] == before and not any(st["kind"] == "morph" for st in before), seed
        assert steps == DS.add_morphology(P0, before, np.random.default_rng([seed, 3])), seed
        L = DS.layout(P)
        for i in at:
            st = steps[i]
            (a, aoff, ap, afs), (b, boff, bp, bfs) = DS.morph_views(L, st)
            rb = st["channels"] * P["w"]
            ispan, ospan = DS.view_span(L, aoff, ap, afs, st["n"], rb), DS.view_span(L, boff, bp, bfs, st["n"], rb)
            assert st["dst"] in DS.MORPH_DSTS and st["op"] in DS.MR.OPS and len(st["spans"]) in DS.MR.KSIZES and st["channels"] in (1, P["ch"]), (seed, i)
            assert (st["src"], st["view"] is None) in (("view", False), ("frames", True)) and (st["channels"] == 3) == (st["src"] == "frames"), (seed, i)
            assert a != b or ispan[1] <= ospan[0] or ospan[1] <= ispan[0], (seed, i, ispan, ospan)
            if st["dst"] == "own":
                assert b in ("mor0", "mor1") and DS.MOR_LEAD <= ospan[0] and ospan[1] + DS.MOR_LEAD <= L["sizes"][b] and bp >= rb and bfs >= bp * P["h"], (seed, i)
                odd.add((boff % 4, bp % 4 != 0, bfs % 4 != 0))
            elif st["dst"] == "blur":
                assert st["channels"] == 3 and 0 <= st["g0"] and st["g0"] + st["n"] <= DS.POOL and (bp, bfs) == (L["ip"], L["ifs"]), (seed, i)
            elif st["dst"] == "sout":
                assert st["channels"] == 1 and a != "sout" and 0 <= st["g0"] and st["g0"] + st["n"] <= L["nmax"] and (boff, bp, bfs) == (L["soff"] + st["g0"] * L["sfs"], L["sp"], L["sfs"]), (seed, i)
            else:
                assert st["channels"] == 1 and 0 <= st["mslot"] < DS.NOUT and 0 <= st["g0"] and st["g0"] + st["n"] <= L["nmax"] and (bp, bfs) == (L["op"], L["ofs"]), (seed, i)
                assert DS.out_start(L, st["mslot"]) <= ospan[0] and ospan[1] <= DS.out_start(L, st["mslot"]) + L["oreg"], (seed, i)
            dsts.add(st["dst"]); ops.add(st["op"]); elements.add(tuple(st["spans"]))
    assert dsts == set(DS.MORPH_DSTS) and ops == set(DS.MR.OPS), (dsts, ops)
    assert {len(e) for e in elements} == set(DS.MR.KSIZES), elements
    for shape in DS.MR.SHAPES:   # (at 3 the cross and the ellipse are one element: each shape at a size where it is its own)
        assert any(tuple(DS.MR.structuring_spans(shape, k)) in elements for k in (5, 7)), (shape, elements)
    assert any(-1 in e and e != e[::-1] for e in elements), elements
    assert {o[0] for o in odd} == {0, 1, 2, 3} and any(o[1] for o in odd) and any(o[2] for o in odd), odd   # base offsets 0 .. 3, pitches and frame strides that are no multiples of 4


def test_the_dist_steps_leave_every_other_step_where_it_was(sequences):
    """The last level: the dist steps come from a fifth generator, and without them a sequence is exactly what add_morphology makes
    of it.  A distance plane over an output region is one frame at four times the region's pitch, disjoint from the map view; planes
    of their own lie in their arenas at multiples of 4; side by side the two ROIs have one pitch and frame stride, lie 4 W and a few
    words apart and leave their rows disjoint.  Across the seeds both destinations, both targets, both types and all three layouts
    of the nearest plane occur, the side-by-side one with the nearest plane on either side."""
    dests, targets, types, nears, sides = set(), set(), set(), set(), set()
    for seed, (P, steps, _) in sequences.items():
        P0, base = DS.base_sequence(seed)
        before = DS.add_components(P0, DS.add_circles(P0, base, np.random.default_rng([seed, 1])), np.random.default_rng([seed, 2]))
        before = DS.add_morphology(P0, before, np.random.default_rng([seed, 3]))
        steps, at = _inserted(seed, steps, "dist", ())
        assert [st for st in steps if st["kind"] != "dist"] == before and not any(st["kind"] == "dist" for st in before), seed
        L = DS.layout(P)
        row = 4 * P["w"]
        for i in at:
            st = steps[i]
            name, off, pitch, fs, _ = DS.resolve_view(L, st["view"])
            (dn, doff, dp, dfs), near = DS.dist_views(L, st)
            mspan, dspan = DS.view_span(L, off, pitch, fs, st["n"], P["w"]), DS.view_span(L, doff, dp, dfs, st["n"], row)
            assert st["view"][0] in DS.VIEW_KINDS and st["near"] in DS.DIST_NEARS and (near is None) == (st["near"] == "none"), (seed, i)
            if st["dest"] == "over":
                assert st["n"] == 1 and dn == "maps" and dp == 4 * L["op"] and doff == DS.out_start(L, st["dslot"]) and 0 <= st["dslot"] < DS.NOUT and st["near"] != "side", (seed, i)
                assert dspan[1] <= DS.out_start(L, st["dslot"]) + L["oreg"] and L["nmax"] >= 4, (seed, i)
                assert name != "maps" or dspan[1] <= mspan[0] or mspan[1] <= dspan[0], (seed, i, mspan, dspan)
            else:
                assert st["dest"] == "own" and dn in ("dtp0", "dtp1") and dp >= row and dfs >= dp * P["h"], (seed, i)
            for view in (v for v in ((dn, doff, dp, dfs), near) if v is not None and v[0] != "maps"):
                span = DS.view_span(L, *view[1:], st["n"], row)
                assert view[0] in ("dtp0", "dtp1") and DS.LAB_LEAD <= span[0] and span[1] + DS.LAB_LEAD <= L["sizes"][view[0]] and all(v % 4 == 0 for v in view[1:]), (seed, i, view)
            if st["near"] == "side":
                apart = abs(near[1] - doff)
                assert near[0] == dn and near[2:] == (dp, dfs) and apart == row + 4 * st["swords"] and st["swords"] in DS.DT_SIDE_WORDS and dp >= 2 * row + 4 * st["swords"], (seed, i)
                assert (near[1] < doff) == st["nleft"], (seed, i)
                sides.add(st["nleft"])
            elif st["near"] == "own":
                assert near[0] != dn, (seed, i)
            dests.add(st["dest"]); targets.add(st["target"]); types.add(st["dtype"]); nears.add(st["near"])
    assert dests == {"own", "over"} and targets == {DS.DR.TO_NONZERO, DS.DR.TO_ZERO} and types == {DS.api.DT_SQUARED_I32, DS.api.DT_F32}, (dests, targets, types)
    assert nears == set(DS.DIST_NEARS) and sides == {False, True}, (nears, sides)


def test_the_model_gives_identical_buffers_twice(oracle, sequences):
    for seed in DS.SEEDS:
        P, steps, _ = sequences[seed]
        a, b = DS.run_model(P, steps, oracle), DS.run_model(P, steps, oracle)
        assert a.buf.keys() == b.buf.keys() and all(np.array_equal(a.buf[k], b.buf[k]) for k in a.buf), seed
        assert a.counters == b.counters == sequences[seed][2], seed


def vacuous(sequences):
    """What is wrong with a seed list, as text; empty for a good one."""
    bad = []
    total = dict.fromkeys(DS.COUNTERS, 0)
    for seed, (P, steps, c) in sequences.items():
        for k, v in c.items():
            total[k] += v
        if P["pipeline"] and not any(c[f"overlap_{k}"] for k in ("whole", "frame", "roi", "sout", "before", "behind", "blur_in", "blur_out")):
            bad.append(f"seed {seed}: pipelined, but no reader on a view that overlaps a pending writer")
        if not c["seg_lists_nonempty"]:
            bad.append(f"seed {seed}: every segment list is empty")
        if not c["line_lists_nonempty"]:
            bad.append(f"seed {seed}: every line list is empty")
        if not c["morph_output_differs"]:
            bad.append(f"seed {seed}: no morph step whose output differs from its input")
        if not c["dist_maps_mixed"]:
            bad.append(f"seed {seed}: no dist step whose map has a feature pixel and another")
    if total["circle_lists_nonempty"] < len(sequences):
        bad.append(f"{total['circle_lists_nonempty']} circle lists that are not empty in {len(sequences)} sequences")
    bad += [f"no sequence reaches {k}" for k in DS.REQUIRED if not total[k]]
    return bad


def test_no_vacuous_sequences(oracle, sequences):
    assert 24 <= len(DS.SEEDS) <= 33 and len(set(DS.SEEDS)) == len(DS.SEEDS)
    assert vacuous(sequences) == []
    kinds = {k: sum(any(st["kind"] == k for st in steps) for _, steps, _ in sequences.values()) for k in DS.KINDS}
    assert all(kinds[k] > len(DS.SEEDS) // 2 for k in ("run", "blur", "points", "lines", "segs", "sync")), kinds
    assert all(kinds[k] > 0 for k in DS.KINDS), kinds
    assert all(any(st["kind"] == "circles" for st in steps) for _, steps, _ in sequences.values())
    assert sum(P["pipeline"] for P, _, _ in sequences.values()) * 2 >= len(DS.SEEDS)
    assert {(P["w"], P["h"]) for P, _, _ in sequences.values()} == set(DS.SIZES)
    assert any(P["per_channel"] for P, _, _ in sequences.values()) and {P["mode"] for P, _, _ in sequences.values()} == {"R", "O"}
    assert {P["staged"] for P, _, c in sequences.values() if c["staged_runs"]} == set(DS.STAGED_FAMILIES)


def test_the_check_notices_a_vacuous_seed(oracle, sequences):
    """A list in which the only sequences that re-use a numangle with other tables are replaced fails the check."""
    keep = {s: v for s, v in sequences.items() if not v[2]["hough_tables_equal_numangle"]}
    assert keep and any("hough_tables_equal_numangle" in t for t in vacuous(keep))
    P, steps, c = next(v for v in sequences.values() if v[0]["pipeline"])
    cut = [st for st in steps if st["kind"] not in ("points", "segs", "blur", "components", "morph", "dist")]   # no reader left: nothing overlaps a pending writer
    assert any("overlaps a pending writer" in t for t in vacuous({-1: (P, cut, dict(DS.run_model(P, [st for st in cut if st["kind"] != "lines"], oracle).counters))}))


def test_the_staged_views_are_staged():
    """Each family breaks the rule that keeps an output in place (pitch, frame stride and base multiples of 4) in its own way."""
    for w, h in DS.SIZES:
        odd = {f: tuple(v % 4 != 0 for v in DS.staged_view(f, w, h)) for f in DS.STAGED_FAMILIES}
        assert odd["ODDO"][0] and odd["ODDO"][2] and odd["P4_BASE"] == (False, False, True) and odd["ROI_FS"] == (False, True, False), odd


def test_hough_geometries(oracle):
    for w, h in DS.SIZES:
        na = [DS.R.geometry(w, h, *g)[0] for g in DS.GEOS]
        assert na == [12, 12, 12, 180], na
        tabs = [np.concatenate(DS.R.tables(w, h, *g)) for g in DS.GEOS[:3]]
        assert not any(np.array_equal(tabs[a], tabs[b]) for a, b in ((0, 1), (0, 2), (1, 2)))


@pytest.fixture(scope="module")
def circle_plans(tmp_path_factory):
    """plan_hough_circles itself (cudacam_amd/csrc/host_plan.h) on circles steps: tests/cpp/hough_circles_plan_driver.cpp, built as
    tests/test_hough_circles_plan_cpu.py builds it.  Returns plans(P, steps) -> one (scratch bytes, passes, frames per pass) or
    refusal text per step, for the planes and the frame limit the executor gives the entry."""
    exe = str(tmp_path_factory.mktemp("circles") / "hough_circles_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, os.path.join(ROOT, "tests", "cpp", "hough_circles_plan_driver.cpp")])

    def plans(P, steps):
        L = DS.layout(P)
        args = [exe, "plan", str(P["w"]), str(P["h"]), str(L["nmax"] if P["per_channel"] else L["mb"])]
        for st in steps:
            args += [str(st["n"]), str(st["pcap"]), str(L["dp"]), str(L["dfs"]), float(st["dp"]).hex(), float(st["min_dist"]).hex(), str(st["threshold"]), str(st["rmin"]), str(st["rmax"]),
                     str(st["cc"]), str(st["ccap"]), str(P["hough_bound"])]
        out = subprocess.run(args, capture_output=True, text=True, timeout=600, env=ENV)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        rows = out.stdout.splitlines()
        assert len(rows) == len(steps)
        return [r if r.startswith("refused") else tuple(int(v) for v in r.split()) for r in rows]
    return plans


def test_the_plan_driver_refuses_what_the_entry_refuses(circle_plans):
    """The driver's answers are the plan's: a frame too many, a centre capacity of 0 and a bound below one frame are refused."""
    P, _ = DS.base_sequence(DS.SEEDS[0])
    good = dict(kind="circles", pslot=0, pcap=5, n=1, dp=1.0, min_dist=3.0, threshold=2, rmin=1, rmax=6, cc=16, cslot=0, ccap=8)
    got = circle_plans(dict(P, hough_bound=0), [good, dict(good, n=DS.layout(P)["nmax"] + 1), dict(good, cc=0), dict(good, pcap=0, ccap=0)])
    assert isinstance(got[0], tuple) and "nframes out of range" in got[1] and "centre_capacity" in got[2] and got[3] == got[0], got
    assert "scratch bound" in circle_plans(dict(P, hough_bound=DS.circle_need(P["w"], P["h"], 1.0, 16, 1, 0)[2] - 1), [good])[0]


@pytest.fixture(scope="module")
def ccl_plans(tmp_path_factory):
    """plan_connected_components itself on components steps: tests/cpp/ccl_plan_driver.cpp, built as tests/test_ccl_plan_cpu.py
    builds it, a stand-alone program under ASan + UBSan.  Returns plans(P, steps) -> one (scratch bytes, passes, frames per pass,
    rows per chunk) or refusal text per step, for the views and the frame limit the executor gives the entry: every buffer gets an
    address of its own, 256 MiB apart, so the plan sees a map and a label plane inside `maps` as they lie to each other."""
    exe = str(tmp_path_factory.mktemp("ccl") / "ccl_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, os.path.join(ROOT, "tests", "cpp", "ccl_plan_driver.cpp")])
    base = {name: (k + 1) << 28 for k, name in enumerate(("maps", "sout", "lab0", "lab1"))}

    def plans(P, steps):
        L = DS.layout(P)
        args = [exe, "plan", str(P["w"]), str(P["h"]), str(L["nmax"] if P["per_channel"] else L["mb"])]
        for st in steps:
            name, off, pitch, fs, _ = DS.resolve_view(L, st["view"])
            lname, loff, lpitch, lfs = DS.label_view(L, st)
            args += [str(v) for v in (st["n"], st["conn"], base[name] + off, pitch, fs, base[lname] + loff, lpitch, lfs, int(st["rows"]), st["cap"], P["hough_bound"])]
        out = subprocess.run(args, capture_output=True, text=True, timeout=600, env=ENV)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        rows = out.stdout.splitlines()
        assert len(rows) == len(steps)
        return [r if r.startswith("refused") else tuple(int(v) for v in r.split()) for r in rows]
    return plans


def test_the_ccl_plan_driver_refuses_what_the_entry_refuses(ccl_plans):
    """The driver's answers are the plan's: a frame too many, a connectivity of 6, a label plane over its own map, rows asked for
    with null pointers and a bound below one frame are refused; ccl_need says what the plan says where the rows of a chunk change."""
    P, _ = DS.base_sequence(DS.SEEDS[0])
    P = dict(P, hough_bound=0)
    L = DS.layout(P)
    good = dict(kind="components", view=("whole", 1), n=1, conn=8, cap=5, rows=True, cslot=0, dest="over", lslot=0, loff=0, lpad=0, lgap=0)
    got = ccl_plans(P, [good, dict(good, n=L["nmax"] + 1, dest="own"), dict(good, conn=6), dict(good, view=("whole", 0)), dict(good, rows=False), dict(good, rows=False, cap=0),
                        dict(good, view=("frame", 0, 3)), dict(good, view=("behind", 0, 4))])   # the plane covers four frames of the region: the last of them; the bytes behind them
    assert got[0] == DS.ccl_need(P["h"], 1, 0)[:2] + (1, min(P["h"], 8)) and got[5] == got[0] and got[7] == got[0], got
    assert "nframes out of range" in got[1] and "connectivity" in got[2] and "overlap" in got[3] and "null with capacity" in got[4] and "overlap" in got[6], got
    per = DS.ccl_need(P["h"], 1, 0)[2]
    assert "scratch bound" in ccl_plans(dict(P, hough_bound=per - 1), [good])[0] and ccl_plans(dict(P, hough_bound=per), [good])[0][:2] == (per, 1)
    for h, n in ((5, 1), (8, 3), (9, 1), (67, 4), (513, 1), (1030, 1), (1030, 63), (1030, 64), (1080, 600), (1080, 1024)):   # hist_chunk_rows: 8, then 9 .. 64
        for bound in (0, 3 * DS.ccl_need(h, n, 0)[2] + 3):
            Q = dict(P, w=5, h=h, per_channel=False, per_channel_ever=False, max_batch=1024, hough_bound=bound)   # (narrow: 1024 frames stay inside the 256 MiB between two buffers)
            (plan,) = ccl_plans(Q, [dict(good, n=n, dest="own")])
            need = DS.ccl_need(h, n, bound)
            assert plan[:2] == need[:2] and plan[2] * need[2] == need[0] and need[2] == 4 * ((h + plan[3] - 1) // plan[3]), (h, n, bound, plan, need)
    assert DS.ccl_need(1030, 64, 0)[2] == 4 * 115 and DS.ccl_need(1030, 63, 0)[2] == 4 * 129 and DS.ccl_need(67, 5, 80) == (72, 3, 36)


BASES = {name: (k + 1) << 28 for k, name in enumerate(("maps", "sout", "frames", "blur", "mor0", "mor1", "dtp0", "dtp1"))}   # an address per buffer, 256 MiB apart


@pytest.fixture(scope="module")
def morph_plans(tmp_path_factory):
    """plan_morphology itself on morph steps: tests/cpp/morph_plan_driver.cpp, built as tests/test_morph_plan_cpu.py builds it, a
    stand-alone program under ASan + UBSan.  Returns plans(P, steps) -> one (scratch bytes, passes, frames per pass) or refusal
    text per step, for the views, the channel count, the option and the bound the executor gives the entry; every buffer at an
    address of its own, so the plan sees an input and an output inside `maps` as they lie to each other."""
    exe = str(tmp_path_factory.mktemp("morph") / "morph_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, os.path.join(ROOT, "tests", "cpp", "morph_plan_driver.cpp")])

    def plans(P, steps):
        L = DS.layout(P)
        args = [exe, "plan", str(P["w"]), str(P["h"]), str(P["ch"]), str(int(P["per_channel"])), str(L["mb"])]
        for st in steps:
            (a, aoff, ap, afs), (b, boff, bp, bfs) = DS.morph_views(L, st)
            spans = list(st["spans"]) + [0] * (7 - len(st["spans"]))
            args += [str(v) for v in (st["n"], st["channels"], st["op"], len(st["spans"]), *spans, BASES[a] + aoff, ap, afs, BASES[b] + boff, bp, bfs, P["hough_bound"])]
        out = subprocess.run(args, capture_output=True, text=True, timeout=600, env=ENV)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        rows = out.stdout.splitlines()
        assert len(rows) == len(steps)
        return [r if r.startswith("refused") else tuple(int(v) for v in r.split()) for r in rows]
    return plans


@pytest.fixture(scope="module")
def dist_plans(tmp_path_factory):
    """plan_distance_transform itself on dist steps: tests/cpp/dist_plan_driver.cpp, built as tests/test_dist_plan_cpu.py builds
    it.  Returns plans(P, steps) -> one (column groups, row groups, LDS bytes) or refusal text per step; every buffer at an address
    of its own, so the overlap rules -- the side-by-side exception among them -- are the plan's.  `raw`: further groups of twelve
    arguments written by hand, for views that no step describes."""
    exe = str(tmp_path_factory.mktemp("dist") / "dist_plan_driver")
    _cc(["g++", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", exe, os.path.join(ROOT, "tests", "cpp", "dist_plan_driver.cpp")])

    def plans(P, steps, raw=()):
        L = DS.layout(P)
        args = [exe, "plan", str(P["w"]), str(P["h"]), str(L["nmax"] if P["per_channel"] else L["mb"])]
        for st in steps:
            name, off, pitch, fs, _ = DS.resolve_view(L, st["view"])
            (dn, doff, dp, dfs), near = DS.dist_views(L, st)
            nn, noff, npitch, nfs = near or (None, 0, 0, 0)
            args += [str(v) for v in (st["n"], st["target"], st["dtype"], BASES[name] + off, pitch, fs, BASES[dn] + doff, dp, dfs, BASES[nn] + noff if near else 0, npitch, nfs)]
        assert len(raw) % 12 == 0
        out = subprocess.run(args + [str(v) for v in raw], capture_output=True, text=True, timeout=600, env=ENV)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        rows = out.stdout.splitlines()
        assert len(rows) == len(steps) + len(raw) // 12
        return [r if r.startswith("refused") else tuple(int(v) for v in r.split()) for r in rows]
    return plans


MORPH_GOOD = dict(kind="morph", src="view", view=("whole", 0), f0=0, n=2, channels=1, op=DS.MR.CLOSE, spans=[1, 1, 1], dst="maps", mslot=1, moff=0, mpad=0, mgap=0, g0=0)
DIST_GOOD = dict(kind="dist", view=("whole", 0), n=2, target=0, dtype=1, dest="own", dslot=0, doff=1, dpad=4, dgap=8, near="side", nslot=0, noff=0, npad=0, ngap=0, swords=1, nleft=False)


def test_the_morph_plan_driver_refuses_what_the_entry_refuses(morph_plans):
    """The driver's answers are the plan's: a frame too many (by channels and by the option), an output over its input, 3-channel
    frames on a one-channel context, an element of empty rows and a bound below one intermediate frame are refused -- the bound
    only where the operation keeps intermediate frames; morph_need says what the plan says at bounds of 1, 2 and 4 frames."""
    P0, _ = DS.base_sequence(DS.SEEDS[0])
    P = dict(P0, ch=1, per_channel=False, per_channel_ever=False, hough_bound=0)
    L = DS.layout(P)
    w, h = P["w"], P["h"]
    good = MORPH_GOOD
    got = morph_plans(P, [good, dict(good, n=L["mb"] + 1), dict(good, mslot=0), dict(good, mslot=0, g0=1), dict(good, mslot=0, g0=2), dict(good, src="frames", view=None, channels=3, dst="own"),
                          dict(good, spans=[-1, -1, -1]), dict(good, view=("behind", 0, L["nmax"]), n=1), dict(good, view=("behind", 0, L["nmax"]), n=1, dst="own", mpad=1, moff=3)])
    per = DS.rup(w, 4) * h
    assert got[0] == (2 * per, 1, 2) == DS.morph_need(w, h, 1, DS.MR.CLOSE, 2, 0)[:2] + (2,) and got[4] == got[0] and got[8] == (per, 1, 1), got
    assert "nframes out of range" in got[1] and "overlap" in got[2] and "overlap" in got[3] and "3-channel context" in got[5] and "empty" in got[6] and "overlap" in got[7], got
    Q = dict(P0, ch=3, per_channel=True, per_channel_ever=True, hough_bound=0)
    three = dict(good, src="frames", view=None, channels=3, dst="own")
    got = morph_plans(Q, [dict(good, n=12, dst="own"), dict(good, n=13, dst="own"), dict(three, n=4), dict(three, n=5)])
    assert got[0] == (12 * per, 1, 12) and "nframes out of range" in got[1] and got[2] == (4 * DS.rup(3 * w, 4) * h, 1, 4) and "nframes out of range" in got[3], got
    assert "nframes out of range" in morph_plans(dict(Q, per_channel=False), [dict(good, n=5, dst="own")])[0]
    for op in DS.MR.OPS:
        keeps = op in (DS.MR.OPEN, DS.MR.CLOSE)
        (low,) = morph_plans(dict(P, hough_bound=per - 1), [dict(good, op=op)])
        assert ("scratch bound" in low) if keeps else low == (0, 1, 2), (op, low)
        assert (DS.morph_need(w, h, 1, op, 2, per - 1)[1] == 0) == keeps
        for frames in (1, 2, 4):
            bound = frames * per + 3
            (plan,) = morph_plans(dict(P, hough_bound=bound), [dict(good, op=op, n=4)])
            need = DS.morph_need(w, h, 1, op, 4, bound)
            assert plan[:2] == need[:2] and (plan == (frames * per, 4 // frames, frames) if keeps else plan == (0, 1, 4)), (op, frames, plan, need)


def test_the_dist_plan_driver_refuses_what_the_entry_refuses(dist_plans):
    """The driver's answers are the plan's: a frame too many, a plane over its own map, and two planes in one arena that are not
    side by side -- unequal pitch, a word shared per row -- are refused; side by side with either plane on the left is taken."""
    P0, _ = DS.base_sequence(DS.SEEDS[0])
    P = dict(P0, per_channel=False, per_channel_ever=False, hough_bound=0)
    L = DS.layout(P)
    w, h = P["w"], P["h"]
    good = DIST_GOOD
    over = dict(good, n=1, dest="over", dslot=1, doff=0, dpad=4 * (L["op"] - w), dgap=0, near="own", nslot=1, swords=0)
    want = ((w + 63) // 64, (h + 3) // 4, 4 * w)
    got = dist_plans(P, [good, dict(good, nleft=True), dict(good, near="none"), over, dict(good, n=L["mb"] + 1), dict(over, dslot=0), dict(over, view=("frame", 1, 3)),
                         dict(over, view=("behind", 1, 4)), dict(good, near="own", nslot=0, noff=1, npad=4, ngap=8), dict(good, near="own", nslot=1)])
    assert got[0] == got[1] == got[2] == got[3] == got[7] == got[9] == want, got
    assert "nframes out of range" in got[4] and "the map and the distance plane overlap" in got[5] and "the map and the distance plane overlap" in got[6], got
    assert "the distance plane and the nearest plane overlap" in got[8], got   # one base, one pitch: the same plane twice
    # side by side by hand: the nearest ROI of `good` with another pitch, another frame stride, a word to the left
    (dn, doff, dp, dfs), (nn, noff, _, _) = DS.dist_views(L, good)

    def raw(npitch, nfs, shift=0, n=2):
        name, off, pitch, fs, _ = DS.resolve_view(L, good["view"])
        return [n, 0, 1, BASES[name] + off, pitch, fs, BASES[dn] + doff, dp, dfs, BASES[nn] + noff + shift, npitch, nfs]
    rows = dist_plans(P, [], raw(dp, dfs) + raw(dp + 4, dfs + 4 * h) + raw(dp, dfs + 4) + raw(dp, dfs, -8) + raw(dp, dfs + 4, n=1))
    assert rows[0] == rows[4] == want and all("the distance plane and the nearest plane overlap" in r for r in rows[1:4]), rows


def test_no_step_would_be_refused(oracle, sequences, circle_plans, ccl_plans, morph_plans, dist_plans):
    """The documented limits of include/hipcanny.h on every step: frame counts, alignments, views inside their buffers, views of a
    blur that do not overlap, lists and tables read only after they were written with the same strides, stream switches behind a
    synchronisation.  The circles steps are given to plan_hough_circles itself, which also says how much scratch and how many
    passes each takes: circle_need, by which the model counts growths and passes, must say the same.  Likewise the components
    steps, plan_connected_components and ccl_need; the plan is also what says that no label plane overlaps its map.  Likewise the
    morph steps, plan_morphology and morph_need, and the dist steps and plan_distance_transform: the plans judge the overlap rules
    (the side-by-side exception among them), the alignment of the planes and the frame limits by channels and option."""
    nplans = 0
    for seed, (P, steps, _) in sequences.items():
        L = DS.layout(P)
        size = L["sizes"]
        limit = L["nmax"] if P["per_channel"] else DS.MAX_BATCH
        assert L["op"] % 4 == 0 and L["ofs"] % 4 == 0 and L["olead"] % 4 == 0 and L["oreg"] % 4 == 0          # the outputs stay in place
        assert (L["sp"] | L["sfs"] | L["soff"]) % 4 != 0                                                      # ... and this one is staged
        assert L["ip"] >= DS.rup(P["w"], 8) * P["ch"] and L["ip"] % 4 == 0 and L["ilead"] % 4 == 0
        assert L["counts_off"] % 4 == 0 and L["list_off"] % 16 == 0 and L["dp"] % 2 == 0
        plist, llist, table, table_on, deriv, blur, prev = {}, {}, False, False, 0, 0, None
        m0 = DS.Model.__new__(DS.Model)
        m0.L = L
        for i, st in enumerate(steps):
            k, what = st["kind"], f"seed {seed} step {i}: {DS.describe(st)}"
            if k in ("run", "canny", "rungrad", "deriv", "blur", "autothr"):
                assert 1 <= st.get("n", DS.MAX_BATCH) <= DS.MAX_BATCH, what
            if k in ("run", "canny", "deriv", "autothr"):
                assert 0 <= st["f0"] and st["f0"] + st.get("n", DS.MAX_BATCH) <= (blur if st.get("src") == "blur" else DS.POOL), what
            if k in ("canny", "rungrad", "thr_on", "thr_off"):
                assert P["mode"] == "O", what
            if k == "canny":
                assert st["aperture"] in (3, 5, 7, -1) and 0 <= st["low"] <= st["high"], what
            if k == "deriv":
                deriv = st["n"]
            if k == "rungrad":
                assert st["n"] <= deriv, what
            if k == "autothr":
                table = True
                assert 0 <= st["param"] <= 1 and st["rule"] in (0, 1), what
            if k == "thr_on":
                assert table, what
                table_on = True
            if k == "thr_off":
                table_on = False
            if k in ("run", "rungrad") and table_on:
                assert st["n"] <= DS.MAX_BATCH, what
            if k == "blur":
                m = DS.Model.__new__(DS.Model)
                m.L = L
                (a, ao, ap, afs), (b, bo, bp, bfs) = m.blur_views(st)
                rb = P["w"] * P["ch"]
                sa, sb = DS.view_span(L, ao, ap, afs, st["n"], rb), DS.view_span(L, bo, bp, bfs, st["n"], rb)
                assert sa[1] <= size[a] and sb[1] <= size[b] and (a != b or sa[1] <= sb[0] or sb[1] <= sa[0]), what
                assert st["ksize"] in (3, 5, 7) and (P["ch"] == 1 or (a, b) == ("frames", "blur")), what
                if st["dst"] == "blur":
                    blur = st["n"]
            if k in ("points", "segs", "components", "dist") or (k == "morph" and st["src"] == "view"):
                name, off, pitch, fs, maxn = DS.resolve_view(L, st["view"])
                lo, hi = DS.view_span(L, off, pitch, fs, st["n"], P["w"])
                assert 1 <= st["n"] <= min(limit, maxn) and 0 <= lo and hi <= size[name] and pitch >= P["w"] and (st["n"] == 1 or fs >= pitch * P["h"]), what
            if k == "points":
                assert DS.list_fits("pts", st["n"], st["cap"], 2, L), what
                plist[st["slot"]] = (st["n"], st["cap"])
            if k == "lines":
                n, cap = plist[st["pslot"]]
                assert 1 <= st["n"] <= min(n, limit) and st["pcap"] == cap > 0 and st["threshold"] >= 0 and DS.list_fits("lines", st["n"], st["lcap"], 3, L), what
                assert not P["hough_bound"] or DS.hough_need(P["w"], P["h"], DS.GEOS[st["geo"]], 1, 0)[2] <= P["hough_bound"], what
                llist[st["lslot"]] = (st["n"], st["lcap"], st["geo"])
            if k == "segs":
                n, cap, geo = llist[st["lslot"]]
                assert st["n"] <= n and st["lcap"] == cap > 0 and st["lgeo"] == geo and DS.list_fits("segs", st["n"], st["scap"], 4, L), what
                assert st["geo"] == geo or st["geo"] in DS.SAME_NUMANGLE[geo], what
            if k == "circles":
                n, cap = plist[st["pslot"]]
                assert 1 <= st["n"] <= min(n, limit) and st["pcap"] == cap and DS.list_fits("circ", st["n"], st["ccap"], 4, L) and st["ccap"] <= DS.CCAP_MAX, what
                assert (512 + L["pf"] * L["dfs"]) % 2 == 0 and DS.view_span(L, DS.Model._planes(m0, st["n"])[1][0], L["dp"], L["dfs"], st["n"], 2 * P["w"])[1] <= size["dxdy"], what
            if k == "components":
                lname, loff, lpitch, lfs = DS.label_view(L, st)
                assert 0 <= loff and DS.view_span(L, loff, lpitch, lfs, st["n"], 4 * P["w"])[1] <= size[lname] and lpitch >= 4 * P["w"], what
                assert L["stats_off"] % 4 == 0 and L["cent_off"] % 8 == 0 and L["cent_off"] >= L["stats_off"] + 20 * st["n"] * st["cap"] + 4 * DS.GUARD, what
                assert L["cent_off"] + 16 * st["n"] * st["cap"] + 4 * DS.GUARD <= size[f"comp{st['cslot']}"] and st["n"] <= DS.NLIST, what
            if k == "morph":
                (a, ao, ap, afs), (b, bo, bp, bfs) = DS.morph_views(L, st)
                rb = st["channels"] * P["w"]
                sa, sb = DS.view_span(L, ao, ap, afs, st["n"], rb), DS.view_span(L, bo, bp, bfs, st["n"], rb)
                assert 0 <= sa[0] and sa[1] <= size[a] and 0 <= sb[0] and sb[1] <= size[b] and ap >= rb and bp >= rb, what
                assert 1 <= st["n"] <= (DS.MAX_BATCH if st["channels"] == 3 else limit) and (st["channels"] == 1 or P["ch"] == 3), what
            if k == "dist":
                (dn, do, dp, dfs), near = DS.dist_views(L, st)
                for vn, vo, vp, vfs in [(dn, do, dp, dfs)] + ([near] if near else []):
                    lo, hi = DS.view_span(L, vo, vp, vfs, st["n"], 4 * P["w"])
                    assert 0 <= lo and hi <= size[vn] and vp >= 4 * P["w"] and (st["n"] == 1 or vfs >= vp * P["h"]), what
                    assert (vo | vp | vfs) % 4 == 0 and L["olead"] % 4 == 0, what   # (the buffers themselves are 256-byte aligned allocations)
                assert st["target"] in (0, 1) and st["dtype"] in (0, 1), what
            if k == "stream":
                assert prev == "sync", what
            prev = k
        assert not table_on, f"seed {seed}: the table is still installed at the end"
        circles = [st for st in steps if st["kind"] == "circles"]
        for st, plan in zip(circles, circle_plans(P, circles)):
            need = DS.circle_need(P["w"], P["h"], st["dp"], st["cc"], st["n"], P["hough_bound"])
            assert isinstance(plan, tuple) and plan[:2] == need[:2] and plan[1] >= 1 and plan[2] * need[2] == need[0], (seed, DS.describe(st), plan, need)
            nplans += 1
        comps = [st for st in steps if st["kind"] == "components"]
        for st, plan in zip(comps, ccl_plans(P, comps)):
            need = DS.ccl_need(P["h"], st["n"], P["hough_bound"])
            assert isinstance(plan, tuple) and plan[:2] == need[:2] and plan[1] == 1 and plan[2] * need[2] == need[0] and plan[3] == min(P["h"], 8), (seed, DS.describe(st), plan, need)
            nplans += 1
        morphs = [st for st in steps if st["kind"] == "morph"]
        for st, plan in zip(morphs, morph_plans(P, morphs)):
            need = DS.morph_need(P["w"], P["h"], st["channels"], st["op"], st["n"], P["hough_bound"])
            assert isinstance(plan, tuple) and plan[:2] == need[:2] and plan[1] == 1 and plan[2] == st["n"], (seed, DS.describe(st), plan, need)
            nplans += 1
        dists = [st for st in steps if st["kind"] == "dist"]
        for st, plan in zip(dists, dist_plans(P, dists)):
            assert plan == ((P["w"] + 63) // 64, (P["h"] + 3) // 4, 4 * P["w"]), (seed, DS.describe(st), plan)
            nplans += 1
    assert nplans >= 4 * len(sequences)
