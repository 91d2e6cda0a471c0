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
        assert 12 <= len([st for st in steps if st["kind"] not in ("circles", "components")]) <= 20 and len(steps) <= 26 and steps[-1]["kind"] == "sync", seed
        assert (P["w"], P["h"]) in DS.SIZES and P["ch"] in (1, 3) and P["staged"] in DS.STAGED_FAMILIES, seed


def test_the_circles_steps_leave_every_other_step_where_it_was(sequences):
    """The circles steps come from a generator of their own: without them a sequence is, step for step, what
    numpy.random.default_rng(seed) alone gives -- the sequence the seed was chosen for.  Each stands behind the opening's points
    step, reads the lists of the points step most recently in front of it, and none stands directly in front of a stream switch."""
    for seed, (P, steps, _) in sequences.items():
        steps = [st for st in steps if st["kind"] != "components"]   # (the next test: what is left is exactly this)
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
    if total["circle_lists_nonempty"] < len(sequences):
        bad.append(f"{total['circle_lists_nonempty']} circle lists that are not empty in {len(sequences)} sequences")
    bad += [f"no sequence reaches {k}" for k in DS.REQUIRED if not total[k]]
    return bad


def test_no_vacuous_sequences(oracle, sequences):
    assert 24 <= len(DS.SEEDS) <= 32 and len(set(DS.SEEDS)) == len(DS.SEEDS)
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
    cut = [st for st in steps if st["kind"] not in ("points", "segs", "blur", "components")]   # no reader left: nothing overlaps a pending writer
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


def test_no_step_would_be_refused(oracle, sequences, circle_plans, ccl_plans):
    """The documented limits of include/hipcanny.h on every step: frame counts, alignments, views inside their buffers, views of a
    blur that do not overlap, lists and tables read only after they were written with the same strides, stream switches behind a
    synchronisation.  The circles steps are given to plan_hough_circles itself, which also says how much scratch and how many
    passes each takes: circle_need, by which the model counts growths and passes, must say the same.  Likewise the components
    steps, plan_connected_components and ccl_need; the plan is also what says that no label plane overlaps its map."""
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
            if k in ("points", "segs", "components"):
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
    assert nplans >= 2 * len(sequences)
