"""tests/device_op_sequences.py without a GPU: the committed seeds give the same sequence and the same expected buffers every time,
exercise what they were chosen for (no vacuous sequence), and contain no call an entry would refuse -- by the limits
include/hipcanny.h documents for each entry, checked here on the steps and the layout of the buffers."""
import numpy as np
import pytest

import device_op_sequences as DS


@pytest.fixture(scope="module")
def sequences(oracle):
    return {seed: DS.make_sequence(seed, oracle) for seed in DS.SEEDS}


def test_make_sequence_is_deterministic(oracle, sequences):
    for seed in DS.SEEDS:
        assert DS.make_sequence(seed, oracle) == sequences[seed], seed
    for seed, (P, steps, _) in sequences.items():
        assert 12 <= len(steps) <= 20 and steps[-1]["kind"] == "sync", seed
        assert (P["w"], P["h"]) in DS.SIZES and P["ch"] in (1, 3) and P["staged"] in DS.STAGED_FAMILIES, seed


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
    bad += [f"no sequence reaches {k}" for k in DS.REQUIRED if not total[k]]
    return bad


def test_no_vacuous_sequences(oracle, sequences):
    assert 24 <= len(DS.SEEDS) <= 32 and len(set(DS.SEEDS)) == len(DS.SEEDS)
    assert vacuous(sequences) == []
    kinds = {k: sum(any(st["kind"] == k for st in steps) for _, steps, _ in sequences.values()) for k in DS.KINDS}
    assert all(kinds[k] > len(DS.SEEDS) // 2 for k in ("run", "blur", "points", "lines", "segs", "sync")), kinds
    assert all(kinds[k] > 0 for k in DS.KINDS), kinds
    assert sum(P["pipeline"] for P, _, _ in sequences.values()) * 2 >= len(DS.SEEDS)
    assert {(P["w"], P["h"]) for P, _, _ in sequences.values()} == set(DS.SIZES)
    assert any(P["per_channel"] for P, _, _ in sequences.values()) and {P["mode"] for P, _, _ in sequences.values()} == {"R", "O"}
    assert {P["staged"] for P, _, c in sequences.values() if c["staged_runs"]} == set(DS.STAGED_FAMILIES)


def test_the_check_notices_a_vacuous_seed(oracle, sequences):
    """A list in which the only sequences that re-use a numangle with other tables are replaced fails the check."""
    keep = {s: v for s, v in sequences.items() if not v[2]["hough_tables_equal_numangle"]}
    assert keep and any("hough_tables_equal_numangle" in t for t in vacuous(keep))
    P, steps, c = next(v for v in sequences.values() if v[0]["pipeline"])
    cut = [st for st in steps if st["kind"] not in ("points", "segs", "blur")]   # no reader left: nothing overlaps a pending writer
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


def test_no_step_would_be_refused(oracle, sequences):
    """The documented limits of include/hipcanny.h on every step: frame counts, alignments, views inside their buffers, views of a
    blur that do not overlap, lists and tables read only after they were written with the same strides, stream switches behind a
    synchronisation."""
    for seed, (P, steps, _) in sequences.items():
        L = DS.layout(P)
        size = L["sizes"]
        limit = L["nmax"] if P["per_channel"] else DS.MAX_BATCH
        assert L["op"] % 4 == 0 and L["ofs"] % 4 == 0 and L["olead"] % 4 == 0 and L["oreg"] % 4 == 0          # the outputs stay in place
        assert (L["sp"] | L["sfs"] | L["soff"]) % 4 != 0                                                      # ... and this one is staged
        assert L["ip"] >= DS.rup(P["w"], 8) * P["ch"] and L["ip"] % 4 == 0 and L["ilead"] % 4 == 0
        assert L["counts_off"] % 4 == 0 and L["list_off"] % 16 == 0 and L["dp"] % 2 == 0
        plist, llist, table, table_on, deriv, blur, prev = {}, {}, False, False, 0, 0, None
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
            if k in ("points", "segs"):
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
            if k == "stream":
                assert prev == "sync", what
            prev = k
        assert not table_on, f"seed {seed}: the table is still installed at the end"
